"""Affinity inference for SR volumes: the "superhuman" residual 3-D U-Net of the segmentation step, on HIP (csrc/conv3d.hip).

The reference scores a super-resolved volume by predicting 3-D affinities with ``inference_code/model/model_superhuman.py::UNet_PNI``
over overlapping 18x160x160 windows (``inference_code/data/provider_valid.py``), Gaussian-blending them and agglomerating.  This module is
the affinity part:

* ``UNet_PNI``: same constructor signature and ``state_dict`` (196 keys) as the reference; only the shipped configuration
  (``inference_code/config/seg_x{8,16}_superhuman.yaml``) is built, anything else raises ``NotImplementedError``.  Inference only: BatchNorm is
  always the eval-mode affine map, folded into per-channel scale / shift when the weights are packed (once per load / device move).
* ``plan_windows`` / ``get_weight`` / ``predict_volume``: ``Provider_valid`` for ``model_type 'superhuman'`` -- reflect padding, end-clamped
  window origins in ``__getitem__`` order, the Gaussian weight volume and the float32 stitching, bit-equal to the reference's numpy sequence.

Activations are NDHWC float32 on the device (``[B, D, H, W, C]``, channels fastest, optionally a channel slice of a wider buffer); the
network's input ``[B, 1, D, H, W]`` is already that layout, and its last convolution writes the ``[B, 3, D, H, W]`` affinities directly.
"""
from __future__ import annotations

import ctypes as C
from collections import OrderedDict
from dataclasses import dataclass
from typing import Callable, Dict, Optional, Sequence, Tuple

import numpy as np
import torch
import torch.nn as nn

from . import _abi
from ._abi import ACT_ELU, ACT_NONE, ACT_SIGMOID

CROP = (18, 160, 160)               # Provider_valid.crop_size for 'superhuman'
PAD_XY, NUM_XY, STRIDE_XY = 48, 13, 80
# test_split Z -> (z stride, z padding, windows along z): provider_valid.py:126-148
Z_PLANS = {200: (10, 4, 20), 100: (10, 4, 10), 50: (10, 4, 5), 25: (15, 4, 2), 20: (10, 4, 2)}
WINDOW_GFLOP = 173.56               # algorithmic GFLOP of one 18x160x160 window (torch.utils.flop_counter on the reference model)

_SHIPPED = dict(in_planes=1, out_planes=3, filters=[28, 36, 48, 64, 80], upsample_mode="bilinear", decode_ratio=1, merge_mode="add",
                pad_mode="zero", bn_mode="async", relu_mode="elu", do_embed=True, if_sigmoid=True, show_feature=False)
_BN_EPS = 1e-5


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


# --------------------------------------------------------------------------------------------------------------------------- kernels

def pack_conv3d(w: torch.Tensor) -> torch.Tensor:
    """Conv3d weight [cout, cin, kd, kh, kw] -> the gpemsr_conv3d layout [tap][cin/4][cout/16][k 4][n 16] (zero padded), same device."""
    cout, cin, kd, kh, kw = w.shape
    taps, ks4, nt = kd * kh * kw, (cin + 3) // 4, (cout + 15) // 16
    wp = torch.zeros(nt * 16, ks4 * 4, taps, dtype=torch.float32, device=w.device)
    wp[:cout, :cin] = w.detach().to(torch.float32).reshape(cout, cin, taps)
    return wp.reshape(nt, 16, ks4, 4, taps).permute(4, 2, 0, 3, 1).contiguous()


def _cl_geom(t: torch.Tensor, what: str) -> Tuple[int, int]:
    """(per-voxel stride, image stride) of a channels-last [B, D, H, W, C] view with dense voxels."""
    if t.dim() != 5 or t.dtype != torch.float32 or not t.is_cuda:
        raise ValueError(f"{what}: expected a float32 [B, D, H, W, C] tensor on the device")
    ld = t.stride(3)
    if t.stride(4) != 1 or t.stride(2) != t.shape[3] * ld or t.stride(1) != t.shape[2] * t.shape[3] * ld or ld < t.shape[4]:
        raise ValueError(f"{what}: voxels must be dense with channels fastest (a channel slice of a wider buffer is fine)")
    return ld, t.stride(0)


def conv3d(x: torch.Tensor, wp: torch.Tensor, cout: int, kd: int, ks: int, bias: Optional[torch.Tensor] = None,
           scale: Optional[torch.Tensor] = None, shift: Optional[torch.Tensor] = None, residual: Optional[torch.Tensor] = None,
           act: int = ACT_NONE, out: Optional[torch.Tensor] = None, ncdhw: bool = False) -> torch.Tensor:
    """out = act((conv3d(x, W) + bias + residual) * scale + shift), zero padding (kd//2, ks//2, ks//2), stride 1.
    x, residual: channels-last [B, D, H, W, C] views (residual with cout channels); wp from ``pack_conv3d``.  The result is a new
    [B, D, H, W, cout] tensor, or written into ``out`` (a channels-last view, or with ``ncdhw`` a contiguous [B, cout, D, H, W] tensor)."""
    B, D, H, W, cin = x.shape
    in_ld, in_is = _cl_geom(x, "conv3d input")
    if out is None:
        out = torch.empty((B, cout, D, H, W) if ncdhw else (B, D, H, W, cout), dtype=torch.float32, device=x.device)
    if ncdhw:
        if tuple(out.shape) != (B, cout, D, H, W) or not out.is_contiguous():
            raise ValueError("conv3d: an NCDHW output must be a contiguous [B, cout, D, H, W] tensor")
        out_ld, out_cs, out_is = 1, D * H * W, cout * D * H * W
    else:
        if tuple(out.shape) != (B, D, H, W, cout):
            raise ValueError("conv3d: output shape")
        out_ld, out_is = _cl_geom(out, "conv3d output")
        out_cs = 1
    d = _abi.Conv3dDesc()
    d.n, d.d, d.h, d.w = B, D, H, W
    d.inp, d.in_ld, d.in_image_stride = x.data_ptr(), in_ld, in_is
    d.cin, d.cout, d.kd, d.ks = cin, cout, kd, ks
    lib = _abi.load()
    if wp.numel() != lib.gpemsr_conv3d_weight_floats(cin, cout, kd, ks):
        raise ValueError("conv3d: packed weight does not match (cin, cout, kd, ks)")
    d.weight = wp.data_ptr()
    d.bias = bias.data_ptr() if bias is not None else None
    d.scale = scale.data_ptr() if scale is not None else None
    d.shift = shift.data_ptr() if shift is not None else None
    if residual is not None:
        if tuple(residual.shape) != (B, D, H, W, cout):
            raise ValueError("conv3d: residual shape")
        d.residual = residual.data_ptr()
        d.res_ld, d.res_image_stride = _cl_geom(residual, "conv3d residual")
    d.out, d.out_ld, d.out_cstride, d.out_image_stride = out.data_ptr(), out_ld, out_cs, out_is
    d.act = act
    _abi.check(lib.gpemsr_conv3d(C.byref(d), _stream()), "conv3d")
    return out


def maxpool_122(x: torch.Tensor) -> torch.Tensor:
    """MaxPool3d((1, 2, 2)) of a channels-last [B, D, H, W, C] view (the 2-D 2x2 pool over the B*D slices, csrc/elem_bf16.hip)."""
    B, D, H, W, Cc = x.shape
    ld, istride = _cl_geom(x, "maxpool input")
    if B > 1 and istride != D * H * W * ld:
        x = x.contiguous()
        ld = Cc
    out = torch.empty((B, D, H // 2, W // 2, Cc), dtype=torch.float32, device=x.device)
    _abi.check(_abi.load().gpemsr_maxpool2(x.data_ptr(), B * D, H, W, Cc, ld, out.data_ptr(), Cc, _stream()), "maxpool2")
    return out


def upsample_merge(low: torch.Tensor, skip: torch.Tensor, scale: torch.Tensor, shift: torch.Tensor) -> torch.Tensor:
    """ELU(BN(Upsample((1, 2, 2), trilinear, align_corners=True)(low) + skip)) -- up_k's interpolation and cat_k, one pass."""
    B, D, h, w, Cc = low.shape
    if tuple(skip.shape) != (B, D, 2 * h, 2 * w, Cc):
        raise ValueError("upsample_merge: skip shape")
    lo_ld, lo_is = _cl_geom(low, "upsample_merge low")
    sk_ld, sk_is = _cl_geom(skip, "upsample_merge skip")
    if B > 1 and (lo_is != D * h * w * lo_ld or sk_is != D * 4 * h * w * sk_ld):
        raise ValueError("upsample_merge: images must be dense")
    out = torch.empty((B, D, 2 * h, 2 * w, Cc), dtype=torch.float32, device=low.device)
    _abi.check(_abi.load().gpemsr_upsample2_add_bn_elu(low.data_ptr(), lo_ld, skip.data_ptr(), sk_ld, B * D, h, w, Cc, scale.data_ptr(),
                                                        shift.data_ptr(), out.data_ptr(), Cc, _stream()), "upsample2_add_bn_elu")
    return out


# --------------------------------------------------------------------------------------------------------------------------- model

def _conv(cin, cout, k, pad, bias):
    m = nn.Conv3d(cin, cout, kernel_size=k, padding=pad, bias=bias)
    nn.init.kaiming_normal_(m.weight)
    if bias:
        nn.init.constant_(m.bias, 0)
    return m


class _ResBlock(nn.Module):
    """resBlock_pni: r = ELU(BN_a(conv1x3x3(x))); out = ELU(BN_c(r + conv3x3x3(ELU(BN_b(conv3x3x3(r))))))."""

    def __init__(self, cin, cout, momentum):
        super().__init__()
        self.block1 = nn.Sequential(_conv(cin, cout, (1, 3, 3), (0, 1, 1), False), nn.BatchNorm3d(cout, momentum=momentum), nn.ELU(inplace=True))
        self.block2 = nn.Sequential(_conv(cout, cout, 3, 1, False), nn.BatchNorm3d(cout, momentum=momentum), nn.ELU(inplace=True),
                                    _conv(cout, cout, 3, 1, False))
        self.block3 = nn.BatchNorm3d(cout, momentum=momentum)
        self.block4 = nn.ELU(inplace=True)


@dataclass
class _Layer:
    wp: torch.Tensor
    cout: int
    kd: int
    ks: int
    bias: Optional[torch.Tensor] = None
    scale: Optional[torch.Tensor] = None
    shift: Optional[torch.Tensor] = None


def _fold_bn(bn: nn.BatchNorm3d) -> Tuple[torch.Tensor, torch.Tensor]:
    """eval-mode BatchNorm (x - mean) / sqrt(var + eps) * gamma + beta as x * scale + shift (folded in float64)."""
    g, b = bn.weight.detach().double(), bn.bias.detach().double()
    m, v = bn.running_mean.detach().double(), bn.running_var.detach().double()
    s = g / torch.sqrt(v + bn.eps)
    return s.float().contiguous(), (b - m * s).float().contiguous()


class UNet_PNI(nn.Module):
    """The superhuman residual U-Net (Lee et al., arXiv:1706.00120) as the reference deploys it, forward on HIP.  Only the configuration
    the reference ships is built (filters [28, 36, 48, 64, 80], bilinear upsampling, additive merges, zero padding, async BatchNorm, ELU,
    sigmoid output); ``init_mode`` and ``bn_momentum`` only matter for training and are accepted as given."""

    def __init__(self, in_planes=1, out_planes=3, filters=[28, 36, 48, 64, 80], upsample_mode='transposeS', decode_ratio=1,  # noqa: B006
                 merge_mode='cat', pad_mode='zero', bn_mode='async', relu_mode='elu', init_mode='kaiming_normal', bn_momentum=0.001,
                 do_embed=True, if_sigmoid=True, show_feature=False):
        super().__init__()
        given = dict(in_planes=in_planes, out_planes=out_planes, filters=list(filters), upsample_mode=upsample_mode, decode_ratio=decode_ratio,
                     merge_mode=merge_mode, pad_mode=pad_mode, bn_mode=bn_mode, relu_mode=relu_mode, do_embed=do_embed, if_sigmoid=if_sigmoid,
                     show_feature=show_feature)
        for k, v in _SHIPPED.items():
            if given[k] != v:
                raise NotImplementedError(f"UNet_PNI: {k}={given[k]!r} is not built (only the shipped configuration: {k}={v!r})")
        if init_mode != 'kaiming_normal':
            raise NotImplementedError(f"UNet_PNI: init_mode={init_mode!r} (only 'kaiming_normal')")
        f = [filters[0]] + list(filters)            # [28, 28, 36, 48, 64, 80]
        mom = bn_momentum
        self.embed_in = nn.Sequential(_conv(in_planes, f[0], (1, 5, 5), (0, 2, 2), True), nn.ELU(inplace=True))
        self.conv0 = _ResBlock(f[0], f[1], mom)
        self.pool0 = nn.MaxPool3d((1, 2, 2), (1, 2, 2))
        self.conv1 = _ResBlock(f[1], f[2], mom)
        self.pool1 = nn.MaxPool3d((1, 2, 2), (1, 2, 2))
        self.conv2 = _ResBlock(f[2], f[3], mom)
        self.pool2 = nn.MaxPool3d((1, 2, 2), (1, 2, 2))
        self.conv3 = _ResBlock(f[3], f[4], mom)
        self.pool3 = nn.MaxPool3d((1, 2, 2), (1, 2, 2))
        self.center = _ResBlock(f[4], f[5], mom)
        for i, (cin, cout) in enumerate([(f[5], f[4]), (f[4], f[3]), (f[3], f[2]), (f[2], f[1])]):
            up = nn.Sequential(nn.Upsample(scale_factor=(1, 2, 2), mode='trilinear', align_corners=True), _conv(cin, cout, 1, 0, True))
            setattr(self, f"up{i}", up)
            setattr(self, f"cat{i}", nn.Sequential(nn.BatchNorm3d(cout, momentum=mom), nn.ELU(inplace=True)))
            setattr(self, f"conv{4 + i}", _ResBlock(cout, cout, mom))
        self.embed_out = nn.Sequential(_conv(f[0], f[0], (1, 5, 5), (0, 2, 2), True), nn.ELU(inplace=True))
        self.out_put = nn.Sequential(_conv(f[0], out_planes, 1, 0, True))
        self.out_planes = out_planes
        self._packed: Optional[Dict[str, object]] = None
        self._packed_dev = None

    # ---- packing: once per load / device move, on the parameters' device ----
    def _apply(self, fn, *args, **kwargs):
        r = super()._apply(fn, *args, **kwargs)
        self._packed = None
        if self.embed_in[0].weight.is_cuda:
            self._pack()
        return r

    def load_state_dict(self, state_dict, strict: bool = True, *args, **kwargs):
        r = super().load_state_dict(state_dict, strict, *args, **kwargs)
        self._packed = None
        if self.embed_in[0].weight.is_cuda:
            self._pack()
        return r

    def _pack(self):
        def conv(c: nn.Conv3d, bn=None):
            kd, kh, kw = c.kernel_size
            L = _Layer(pack_conv3d(c.weight), c.out_channels, kd, kh,
                       bias=None if c.bias is None else c.bias.detach().float().contiguous())
            if bn is not None:
                L.scale, L.shift = _fold_bn(bn)
            return L

        P: Dict[str, object] = {"embed_in": conv(self.embed_in[0]), "embed_out": conv(self.embed_out[0]), "out_put": conv(self.out_put[0])}
        for name in ["conv0", "conv1", "conv2", "conv3", "center", "conv4", "conv5", "conv6", "conv7"]:
            b = getattr(self, name)
            c3 = _fold_bn(b.block3)
            P[name] = (conv(b.block1[0], b.block1[1]), conv(b.block2[0], b.block2[1]), conv(b.block2[3]), c3)
        for i in range(4):
            P[f"up{i}"] = conv(getattr(self, f"up{i}")[1])
            P[f"cat{i}"] = _fold_bn(getattr(self, f"cat{i}")[0])
        self._packed, self._packed_dev = P, self.embed_in[0].weight.device

    # ---- forward ----
    @staticmethod
    def _run(x, L: _Layer, act, residual=None, out=None, ncdhw=False):
        return conv3d(x, L.wp, L.cout, L.kd, L.ks, bias=L.bias, scale=L.scale, shift=L.shift, residual=residual, act=act, out=out, ncdhw=ncdhw)

    def _res(self, x, name):
        a, b, c, (sc, sh) = self._packed[name]
        r = self._run(x, a, ACT_ELU)
        t = self._run(r, b, ACT_ELU)
        return conv3d(t, c.wp, c.cout, c.kd, c.ks, scale=sc, shift=sh, residual=r, act=ACT_ELU)

    def forward(self, x: torch.Tensor, trace: Optional[Dict[str, torch.Tensor]] = None) -> torch.Tensor:
        """x [B, 1, D, H, W] float32 on the device -> affinities [B, 3, D, H, W] in [0, 1].  D >= 1; H and W multiples of 16.
        trace: optional dict that receives the named intermediates (embed_in, conv0-3, center, cat0-3, conv4-7, embed_out) as [B, C, D, H, W]
        views."""
        if x.dim() != 5 or x.shape[1] != 1:
            raise ValueError(f"UNet_PNI: input must be [B, 1, D, H, W], got {tuple(x.shape)}")
        B, _, D, H, W = x.shape
        if D < 1 or H % 16 or W % 16 or H == 0 or W == 0:
            raise ValueError(f"UNet_PNI: H and W must be positive multiples of 16 (four (1, 2, 2) pools), got {H}x{W}")
        if not x.is_cuda or x.dtype != torch.float32:
            raise ValueError("UNet_PNI: input must be float32 on the device")
        if self._packed is None or self._packed_dev != x.device:
            if self.embed_in[0].weight.device != x.device:
                raise ValueError("UNet_PNI: move the model to the input's device first (model.to(device))")
            self._pack()
        P = self._packed
        keep = (lambda k, t: trace.__setitem__(k, t.permute(0, 4, 1, 2, 3))) if trace is not None else (lambda k, t: None)
        h = self._run(x.contiguous().view(B, D, H, W, 1), P["embed_in"], ACT_ELU)
        keep("embed_in", h)
        skips = []
        for i, name in enumerate(["conv0", "conv1", "conv2", "conv3"]):
            h = self._res(h, name)
            keep(name, h)
            skips.append(h)
            h = maxpool_122(h)
        h = self._res(h, "center")
        keep("center", h)
        for i in range(4):
            u = self._run(h, P[f"up{i}"], ACT_NONE)          # the 1x1 convolution at the low resolution (interpolation weights sum to 1)
            sc, sh = P[f"cat{i}"]
            h = upsample_merge(u, skips[3 - i], sc, sh)
            keep(f"cat{i}", h)
            h = self._res(h, f"conv{4 + i}")
            keep(f"conv{4 + i}", h)
        h = self._run(h, P["embed_out"], ACT_ELU)
        keep("embed_out", h)
        return self._run(h, P["out_put"], ACT_SIGMOID, ncdhw=True)


def build_from_config(model_cfg: dict) -> UNet_PNI:
    """UNet_PNI from the MODEL block of the reference's seg_*_superhuman.yaml (inference_seg.py:85-94)."""
    if model_cfg.get("model_type", "superhuman") != "superhuman":
        raise NotImplementedError(f"model_type {model_cfg.get('model_type')!r}: only 'superhuman' is built")
    return UNet_PNI(in_planes=model_cfg["input_nc"], out_planes=model_cfg["output_nc"], filters=model_cfg["filters"],
                    upsample_mode=model_cfg["upsample_mode"], decode_ratio=model_cfg["decode_ratio"], merge_mode=model_cfg["merge_mode"],
                    pad_mode=model_cfg["pad_mode"], bn_mode=model_cfg["bn_mode"], relu_mode=model_cfg["relu_mode"],
                    init_mode=model_cfg["init_mode"], if_sigmoid=model_cfg.get("if_sigmoid", True))


def load_checkpoint(path: str) -> "OrderedDict[str, torch.Tensor]":
    """The reference's superhuman.pt -> a state dict for UNet_PNI: checkpoint['model_weights'] with the DataParallel 'module.' prefix removed
    (inference_seg.py:96-105)."""
    ck = torch.load(path, map_location="cpu", weights_only=False)
    sd = ck["model_weights"] if isinstance(ck, dict) and "model_weights" in ck else ck
    out = OrderedDict()
    for k, v in sd.items():
        out[k[7:] if k.startswith("module.") else k] = v
    return out


# --------------------------------------------------------------------------------------------------------------------------- volumes

@dataclass
class WindowPlan:
    shape: Tuple[int, int, int]            # the volume [Z, H, W]
    pad: Tuple[int, int, int]              # reflect padding per side
    padded: Tuple[int, int, int]
    origins: np.ndarray                    # [n, 3] int32, padded coordinates, __getitem__ order

    @property
    def n(self) -> int:
        return int(self.origins.shape[0])


def plan_windows(shape: Sequence[int]) -> WindowPlan:
    """Provider_valid's window plan for a [Z, H, W] volume: z stride / padding / count per Z (200, 100, 50, 25, 20; others raise
    NotImplementedError as the reference does), 48 voxels of xy padding and 13 windows per side, origins clamped to the padded end, in index
    order (z outer, then H, then W).  A volume the windows do not cover, or whose padded extent is below one window, raises ValueError."""
    Z, H, W = (int(s) for s in shape)
    if Z not in Z_PLANS:
        raise NotImplementedError(f"plan_windows: {Z} slices (the reference plans 200, 100, 50, 25 or 20)")
    sz, pz, nz = Z_PLANS[Z]
    padded = (Z + 2 * pz, H + 2 * PAD_XY, W + 2 * PAD_XY)
    counts, strides = (nz, NUM_XY, NUM_XY), (sz, STRIDE_XY, STRIDE_XY)
    for a in range(3):
        if padded[a] < CROP[a]:
            raise ValueError(f"plan_windows: padded extent {padded[a]} on axis {a} is smaller than the {CROP[a]}-voxel window")
        if (counts[a] - 1) * strides[a] + CROP[a] < padded[a]:
            raise ValueError(f"plan_windows: {counts[a]} windows of {CROP[a]} at stride {strides[a]} do not cover the padded extent "
                             f"{padded[a]} on axis {a} (the reference would divide by zero there)")
    if H <= PAD_XY or W <= PAD_XY:
        raise ValueError("plan_windows: reflect padding of 48 needs H, W > 48")

    def starts(a):
        return [min(i * strides[a], padded[a] - CROP[a]) for i in range(counts[a])]
    org = [(z, y, x) for z in starts(0) for y in starts(1) for x in starts(2)]
    return WindowPlan((Z, H, W), (pz, PAD_XY, PAD_XY), padded, np.asarray(org, dtype=np.int32))


def get_weight(sigma: float = 0.2, mu: float = 0.0) -> np.ndarray:
    """Provider_valid.get_weight(): the [18, 160, 160] float32 Gaussian blending weight (computed with numpy, as the reference does)."""
    zz, yy, xx = np.meshgrid(np.linspace(-1, 1, CROP[0], dtype=np.float32), np.linspace(-1, 1, CROP[1], dtype=np.float32),
                             np.linspace(-1, 1, CROP[2], dtype=np.float32), indexing='ij')
    dd = np.sqrt(zz * zz + yy * yy + xx * xx)
    return (1e-6 + np.exp(-((dd - mu) ** 2 / (2.0 * sigma ** 2)))).astype(np.float32)


def gather_windows(vol: torch.Tensor, plan: WindowPlan, origins_dev: torch.Tensor, k0: int, nb: int,
                   out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Windows k0 .. k0+nb-1 of the plan as [nb, 1, 18, 160, 160] float32 (uint8 voxels / 255)."""
    Z, H, W = plan.shape
    if out is None:
        out = torch.empty((nb, 1) + CROP, dtype=torch.float32, device=vol.device)
    is_u8 = vol.dtype == torch.uint8
    _abi.check(_abi.load().gpemsr_affinity_gather(vol.data_ptr(), int(is_u8), Z, H, W, *plan.pad, origins_dev[k0:].data_ptr(), nb, *CROP,
                                                  out.data_ptr(), _stream()), "affinity_gather")
    return out


def predict_volume(model: Optional[UNet_PNI], vol: torch.Tensor, batch: int = 4, weight: Optional[np.ndarray] = None,
                   predict: Optional[Callable[[torch.Tensor], torch.Tensor]] = None) -> torch.Tensor:
    """Provider_valid + the inference loop of inference_seg.py:107-129: vol [Z, H, W] uint8 (or float32 in [0, 1]) on the device ->
    affinities [3, Z, H, W] float32 on the device.  Windows run ``batch`` at a time; the stitching is the reference's float32 sequence
    (out += affs * w, wmap += w in window order, then out / wmap), so the result depends on the per-window predictions only.
    weight: the [18, 160, 160] blending weight (default ``get_weight()``); predict: [nb, 1, 18, 160, 160] -> [nb, C, 18, 160, 160]
    (default ``model``)."""
    if vol.dim() != 3 or not vol.is_cuda or vol.dtype not in (torch.uint8, torch.float32):
        raise ValueError("predict_volume: vol must be a [Z, H, W] uint8 or float32 tensor on the device")
    vol = vol.contiguous()
    plan = plan_windows(vol.shape)
    dev = vol.device
    predict = predict if predict is not None else model
    w = torch.from_numpy(np.ascontiguousarray(weight if weight is not None else get_weight(), dtype=np.float32).reshape(CROP)).to(dev)
    org = torch.from_numpy(plan.origins).to(dev)
    Zp, Hp, Wp = plan.padded
    out = wmap = None
    lib = _abi.load()
    bbox = (C.c_int32 * 6)()
    with torch.no_grad():
        for k0 in range(0, plan.n, batch):
            nb = min(batch, plan.n - k0)
            affs = predict(gather_windows(vol, plan, org, k0, nb))
            if affs.dim() != 5 or affs.shape[0] != nb or tuple(affs.shape[2:]) != CROP:
                raise ValueError(f"predict_volume: predictions of shape {tuple(affs.shape)}")
            affs = affs.contiguous()
            nc = affs.shape[1]
            if out is None:
                out = torch.zeros((nc, Zp, Hp, Wp), dtype=torch.float32, device=dev)
                wmap = torch.zeros((Zp, Hp, Wp), dtype=torch.float32, device=dev)
            o = plan.origins[k0:k0 + nb]
            lo, hi = o.min(axis=0), o.max(axis=0) + np.asarray(CROP)
            bbox[:] = [int(lo[0]), int(lo[1]), int(lo[2]), int(hi[0] - lo[0]), int(hi[1] - lo[1]), int(hi[2] - lo[2])]
            _abi.check(lib.gpemsr_affinity_accumulate(affs.data_ptr(), nc, w.data_ptr(), org[k0:].data_ptr(), nb, *CROP, out.data_ptr(),
                                                      wmap.data_ptr(), Zp, Hp, Wp, bbox, _stream()), "affinity_accumulate")
        Z, H, W = plan.shape
        res = torch.empty((out.shape[0], Z, H, W), dtype=torch.float32, device=dev)
        _abi.check(lib.gpemsr_affinity_finalize(out.data_ptr(), wmap.data_ptr(), out.shape[0], Zp, Hp, Wp, *plan.pad, Z, H, W, res.data_ptr(),
                                                _stream()), "affinity_finalize")
    return res


def executed_flop_ratio(D: int = 18, H: int = 160, W: int = 160) -> Tuple[float, float]:
    """(algorithmic GFLOP, executed / algorithmic) of one [1, 1, D, H, W] forward: the MFMA tiles pad cout to 16, cin to 4 and the output
    to 2 x 8 x 16 voxel tiles (tile counts of csrc/conv3d.hip)."""
    f = [28, 28, 36, 48, 64, 80]
    layers = []          # (level, cin, cout, taps)
    layers.append((0, 1, 28, 25))
    for lvl, (i, o) in enumerate(zip(f[:-1], f[1:])):
        layers += [(lvl, i, o, 9), (lvl, o, o, 27), (lvl, o, o, 27)]
    for k, (i, o) in enumerate([(80, 64), (64, 48), (48, 36), (36, 28)]):
        lvl = 3 - k
        layers.append((lvl + 1, i, o, 1))
        layers += [(lvl, o, o, 9), (lvl, o, o, 27), (lvl, o, o, 27)]
    layers += [(0, 28, 28, 25), (0, 28, 3, 1)]
    alg = exe = 0.0
    for lvl, ci, co, taps in layers:
        h, w = H >> lvl, W >> lvl
        alg += 2.0 * D * h * w * ci * co * taps
        vox = (-(-D // 2) * 2) * (-(-h // 8) * 8) * (-(-w // 16) * 16)
        exe += 2.0 * vox * (-(-ci // 4) * 4) * (-(-co // 16) * 16) * taps
    return alg / 1e9, exe / alg
