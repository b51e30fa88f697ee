"""Affinity inference for SR volumes with the MALA 3-D U-Net of the segmentation step, on HIP (csrc/conv3d_mala.hip).

The reference's ``inference_code/config/seg_x{8,16}_MALA.yaml`` predict 3-D affinities with ``inference_code/model/unet3d_mala.py::UNet3D_MALA``
(Funke et al., arXiv:1709.02974) over 53x268x268 windows that each yield a 25x56x56 prediction, placed into the volume without blending
(``inference_code/data/provider_valid.py``, ``model_type 'mala'``).  This module is the affinity part:

* ``UNet3D_MALA``: same constructor signature and ``state_dict`` (39 keys) as the reference, inference only.  Every 3x3x3 convolution is valid
  (no padding) and followed by ``leaky_relu(x, 0.005)``; the decoder merges are ``conv_1x1(dconv(x)) + bias + crop(skip)``.
* ``plan_windows_mala`` / ``predict_volume_mala``: ``Provider_valid`` for 'mala' -- reflect padding (14, 106, 106), stride = output size,
  end-clamped origins in ``__getitem__`` order, and the stitching, where the last window in index order wins.

Activations are NDHWC float32 on the device (``[B, D, H, W, C]``); the network's input ``[B, 1, D, H, W]`` is already that layout, and its
last (1x1) convolution writes the ``[B, out, D, H, W]`` affinities directly (gpemsr_conv3d, csrc/conv3d.hip).
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F
import torch.nn.init as init

from . import _abi
from ._abi import ACT_LRELU_005, ACT_NONE, ACT_SIGMOID
from .affinity import WindowPlan, conv3d, load_checkpoint, pack_conv3d  # noqa: F401  (load_checkpoint: same checkpoint format)

CROP = (53, 268, 268)               # Provider_valid.crop_size for 'mala'
NET_PAD = (14, 106, 106)            # Provider_valid.net_padding: what the network trims per side
OUT = (25, 56, 56)                  # the prediction of one window (= the window stride)
NUM_XY = 19                         # windows per xy axis (non-'fib' datasets)
WINDOW_GFLOP = 392.65               # torch.utils.flop_counter on the reference model, one [1, 1, 53, 268, 268] window
THIN_MAX_COUT = 80                  # gpemsr_conv3d_valid_thin; wider layers run gpemsr_conv3d_valid_wide
_SLOPE = 0.005
_CONVS3 = ["conv1", "conv2", "conv3", "conv4", "conv5", "conv6", "conv7", "conv8", "conv10", "conv11", "conv13", "conv14", "conv16", "conv17"]
_MERGES = [("dconv1", "conv9", 1500, 300), ("dconv2", "conv12", 300, 60), ("dconv3", "conv15", 60, 12)]


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _cl_geom(t: torch.Tensor, what: str) -> Tuple[int, int]:
    """(per-voxel stride, image stride) of a channels-last [B, D, H, W, C] float32 device view with dense voxels."""
    if t.dim() != 5 or t.dtype != torch.float32 or not t.is_cuda:
        raise ValueError(f"{what}: expected a float32 [B, D, H, W, C] tensor on the device")
    ld = t.stride(3)
    if t.stride(4) != 1 or t.stride(2) != t.shape[3] * ld or t.stride(1) != t.shape[2] * t.shape[3] * ld or ld < t.shape[4]:
        raise ValueError(f"{what}: voxels must be dense with channels fastest (a channel slice of a wider buffer is fine)")
    return ld, t.stride(0)


# --------------------------------------------------------------------------------------------------------------------------- kernels

def pack_valid_wide(w: torch.Tensor) -> torch.Tensor:
    """Conv3d weight [cout, cin, 3, 3, 3] -> the gpemsr_conv3d_valid_wide layout [27][cin][coutp] (coutp = cout rounded up to 16), same device."""
    cout, cin = w.shape[:2]
    coutp = (cout + 15) // 16 * 16
    wp = torch.zeros(27, cin, coutp, dtype=torch.float32, device=w.device)
    wp[:, :, :cout] = w.detach().to(torch.float32).reshape(cout, cin, 27).permute(2, 1, 0)
    return wp


def pack_valid(w: torch.Tensor) -> torch.Tensor:
    """The packed weight of a valid 3x3x3 layer for the kernel ``conv3d_valid`` picks (thin for cout <= 80, else wide)."""
    return pack_conv3d(w) if w.shape[0] <= THIN_MAX_COUT else pack_valid_wide(w)


def conv3d_valid(x: torch.Tensor, wp: torch.Tensor, cout: int, bias: Optional[torch.Tensor] = None, act: int = ACT_LRELU_005,
                 out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out = act(conv3d(x, W) + bias), 3x3x3, stride 1, no padding: x [B, D, H, W, cin] (channels-last view) -> [B, D-2, H-2, W-2, cout].
    wp from ``pack_valid``: cout <= 80 runs the halo-in-LDS kernel, wider layers the implicit GEMM (csrc/conv3d_mala.hip)."""
    B, D, H, W, cin = x.shape
    if D < 3 or H < 3 or W < 3:
        raise ValueError(f"conv3d_valid: input {D}x{H}x{W} is smaller than the 3x3x3 kernel")
    in_ld, in_is = _cl_geom(x, "conv3d_valid input")
    shape = (B, D - 2, H - 2, W - 2, cout)
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=x.device)
    if tuple(out.shape) != shape:
        raise ValueError("conv3d_valid: output shape")
    out_ld, out_is = _cl_geom(out, "conv3d_valid output")
    lib = _abi.load()
    thin = cout <= THIN_MAX_COUT
    want = (lib.gpemsr_conv3d_valid_thin_weight_floats if thin else lib.gpemsr_conv3d_valid_wide_weight_floats)(cin, cout)
    if wp.numel() != want or not wp.is_contiguous():
        raise ValueError("conv3d_valid: packed weight does not match (cin, cout)")
    d = _abi.Conv3dValidDesc()
    d.n, d.d, d.h, d.w = B, D, H, W
    d.inp, d.in_ld, d.in_image_stride = x.data_ptr(), in_ld, in_is
    d.cin, d.cout = cin, cout
    d.weight = wp.data_ptr()
    d.bias = bias.data_ptr() if bias is not None else None
    d.out, d.out_ld, d.out_image_stride = out.data_ptr(), out_ld, out_is
    d.act = act
    ws = None
    if not thin:
        nws = lib.gpemsr_conv3d_valid_wide_workspace_floats(B, D, H, W, cin, cout)
        if nws > 0:
            ws = torch.empty(nws, dtype=torch.float32, device=x.device)
            d.workspace, d.workspace_floats = ws.data_ptr(), nws
    _abi.check((lib.gpemsr_conv3d_valid_thin if thin else lib.gpemsr_conv3d_valid_wide)(C.byref(d), _stream()), "conv3d_valid")
    return out


def maxpool_133(x: torch.Tensor) -> torch.Tensor:
    """MaxPool3d((1, 3, 3), stride (1, 3, 3)) of a dense channels-last [B, D, H, W, C] tensor (floor: [B, D, H//3, W//3, C])."""
    B, D, H, W, Cc = x.shape
    ld, istride = _cl_geom(x, "maxpool_133 input")
    if B > 1 and istride != D * H * W * ld:
        x = x.contiguous()
        ld = Cc
    if H < 3 or W < 3:
        raise ValueError(f"maxpool_133: plane {H}x{W} is smaller than the 3x3 window")
    out = torch.empty((B, D, H // 3, W // 3, Cc), dtype=torch.float32, device=x.device)
    _abi.check(_abi.load().gpemsr_maxpool133(x.data_ptr(), ld, B * D, H, W, Cc, out.data_ptr(), Cc, _stream()), "maxpool133")
    return out


def merge_crop(skip_shape: Sequence[int], up_shape: Sequence[int]) -> Tuple[int, int]:
    """crop_and_concat's crop (cz, c) of a skip [.., D, H, W] for an upsampled [.., d, h, w]: c from H, applied to H AND W as
    ``F.pad(bypass, (-c, -c, -c, -c, -cc, -cc))`` does.  Raises ValueError where the reference's assert or its add fails."""
    (Ds, Hs, Ws), (d, h, w) = tuple(skip_shape[-3:]), tuple(up_shape[-3:])
    c, cc = (Hs - h) // 2, (Ds - d) // 2
    if c <= 0 or cc <= 0:
        raise ValueError(f"crop_and_concat: skip {Ds}x{Hs}x{Ws} is not larger than {d}x{h}x{w} (the reference asserts c > 0, cc > 0)")
    if Ds - 2 * cc != d or Hs - 2 * c != h or Ws - 2 * c != w:
        raise ValueError(f"crop_and_concat: skip {Ds}x{Hs}x{Ws} cropped by ({cc}, {c}, {c}) is not {d}x{h}x{w} (the reference's add fails)")
    return cc, c


def mala_merge(x: torch.Tensor, dw: torch.Tensor, wp: torch.Tensor, cout: int, bias: Optional[torch.Tensor], skip: torch.Tensor) -> torch.Tensor:
    """conv_1x1(ConvTranspose3d((1,3,3), stride (1,3,3), groups=C, no bias)(x)) + bias + crop(skip), one pass:
    x [B, d, h, w, cin] -> [B, d, 3h, 3w, cout]; dw [cin, 9] (the transposed-conv weight), wp [cin, coutp] (``pack_1x1``), skip
    [B, D, H, W, cout] (dense images)."""
    B, d, h, w, cin = x.shape
    if skip.dim() != 5 or skip.shape[0] != B or skip.shape[4] != cout:
        raise ValueError(f"mala_merge: skip {tuple(skip.shape)} for input {tuple(x.shape)} and {cout} channels")
    merge_crop(skip.shape[1:4], (d, 3 * h, 3 * w))
    x_ld, x_is = _cl_geom(x, "mala_merge input")
    if B > 1 and x_is != d * h * w * x_ld:
        x = x.contiguous()
        x_ld = cin
    sk_ld, sk_is = _cl_geom(skip, "mala_merge skip")
    if B > 1 and sk_is != skip.shape[1] * skip.shape[2] * skip.shape[3] * sk_ld:
        raise ValueError("mala_merge: skip images must be dense")
    if tuple(dw.shape) != (cin, 9) or not dw.is_contiguous() or tuple(wp.shape) != (cin, (cout + 15) // 16 * 16) or not wp.is_contiguous():
        raise ValueError("mala_merge: weights do not match (cin, cout)")
    out = torch.empty((B, d, 3 * h, 3 * w, cout), dtype=torch.float32, device=x.device)
    _abi.check(_abi.load().gpemsr_mala_merge(x.data_ptr(), x_ld, B, d, h, w, cin, dw.data_ptr(), wp.data_ptr(),
                                             bias.data_ptr() if bias is not None else None, cout, skip.data_ptr(), sk_ld, *skip.shape[1:4],
                                             out.data_ptr(), cout, _stream()), "mala_merge")
    return out


def pack_1x1(w: torch.Tensor) -> torch.Tensor:
    """Conv3d weight [cout, cin, 1, 1, 1] -> [cin, coutp] (coutp = cout rounded up to 16, zero columns)."""
    cout, cin = w.shape[:2]
    wp = torch.zeros(cin, (cout + 15) // 16 * 16, dtype=torch.float32, device=w.device)
    wp[:, :cout] = w.detach().to(torch.float32).reshape(cout, cin).t()
    return wp


# --------------------------------------------------------------------------------------------------------------------------- model

def network_shapes(D: int, H: int, W: int) -> Dict[str, Tuple[int, int, int]]:
    """(d, h, w) of every named tensor of one forward, following the reference's arithmetic; ValueError where the reference fails (a
    convolution or pool on too small an input, a crop it asserts against, or an add of mismatched shapes)."""
    s: Dict[str, Tuple[int, int, int]] = {}

    def conv(name, t):
        if min(t) < 3:
            raise ValueError(f"UNet3D_MALA: {name} input {t} is smaller than its 3x3x3 kernel")
        s[name] = (t[0] - 2, t[1] - 2, t[2] - 2)
        return s[name]

    def pool(name, t):
        if t[1] < 3 or t[2] < 3:
            raise ValueError(f"UNet3D_MALA: {name} input {t} is smaller than its 1x3x3 window")
        s[name] = (t[0], t[1] // 3, t[2] // 3)
        return s[name]

    t = pool("pool1", conv("conv2", conv("conv1", (D, H, W))))
    t = pool("pool2", conv("conv4", conv("conv3", t)))
    t = pool("pool3", conv("conv6", conv("conv5", t)))
    t = conv("conv8", conv("conv7", t))
    for (dconv, _, _, _), mc, skip, (ca, cb) in zip(_MERGES, ["mc1", "mc2", "mc3"], ["conv6", "conv4", "conv2"],
                                                    [("conv10", "conv11"), ("conv13", "conv14"), ("conv16", "conv17")]):
        up = (t[0], 3 * t[1], 3 * t[2])
        merge_crop(s[skip], up)
        s[mc] = up
        t = conv(cb, conv(ca, up))
    if min(t) < 1:
        raise ValueError(f"UNet3D_MALA: the output {t} is empty")
    return s


@dataclass
class _Conv:
    wp: torch.Tensor
    cout: int
    bias: Optional[torch.Tensor]


class UNet3D_MALA(nn.Module):
    """The reference's MALA U-Net (unet3d_mala.py::UNet3D_MALA), forward on HIP.  Channel widths 12 / 60 / 300 / 1500, valid 3x3x3
    convolutions with leaky_relu(0.005), (1,3,3) max pools, depthwise (1,3,3) transposed convolutions + 1x1 convolutions + cropped skip adds
    in the decoder, a 1x1 output convolution (+ sigmoid).  ``init_mode`` only matters for a fresh model and follows the reference."""

    def __init__(self, output_nc=1, if_sigmoid=True, init_mode='kaiming', show_feature=False):
        super().__init__()
        if not 1 <= output_nc <= 80:
            raise NotImplementedError(f"UNet3D_MALA: output_nc={output_nc} is not built (1..80)")
        if init_mode not in ('kaiming', 'xavier', 'orthogonal'):
            raise AttributeError('No this init mode!')
        self.if_sigmoid, self.init_mode, self.show_feature = if_sigmoid, init_mode, show_feature

        def c3(i, o):
            return nn.Conv3d(i, o, 3, stride=1, padding=0, bias=True)

        def up(c):
            return nn.ConvTranspose3d(c, c, (1, 3, 3), stride=(1, 3, 3), padding=0, groups=c, bias=False)
        self.conv1, self.conv2 = c3(1, 12), c3(12, 12)
        self.pool1 = nn.MaxPool3d(kernel_size=(1, 3, 3), stride=(1, 3, 3))
        self.conv3, self.conv4 = c3(12, 60), c3(60, 60)
        self.pool2 = nn.MaxPool3d(kernel_size=(1, 3, 3), stride=(1, 3, 3))
        self.conv5, self.conv6 = c3(60, 300), c3(300, 300)
        self.pool3 = nn.MaxPool3d(kernel_size=(1, 3, 3), stride=(1, 3, 3))
        self.conv7, self.conv8 = c3(300, 1500), c3(1500, 1500)
        self.dconv1 = up(1500)
        self.conv9 = nn.Conv3d(1500, 300, 1, bias=True)
        self.conv10, self.conv11 = c3(300, 300), c3(300, 300)
        self.dconv2 = up(300)
        self.conv12 = nn.Conv3d(300, 60, 1, bias=True)
        self.conv13, self.conv14 = c3(60, 60), c3(60, 60)
        self.dconv3 = up(60)
        self.conv15 = nn.Conv3d(60, 12, 1, bias=True)
        self.conv16, self.conv17 = c3(12, 12), c3(12, 12)
        self.conv18 = nn.Conv3d(12, output_nc, 1, bias=True)
        for m in self.modules():
            if isinstance(m, (nn.Conv3d, nn.ConvTranspose3d)):
                if init_mode == 'kaiming':
                    init.kaiming_normal_(m.weight, _SLOPE, 'fan_in', 'leaky_relu')
                elif init_mode == 'xavier':
                    init.xavier_normal_(m.weight)
                else:
                    init.orthogonal_(m.weight)
        self.output_nc = output_nc
        self._packed: Optional[Dict[str, object]] = None
        self._packed_dev = None

    # ---- packing: once per load / device move, on the parameters' device ----
    def _apply(self, fn, *args, **kwargs):
        r = super()._apply(fn, *args, **kwargs)
        self._packed = None
        if self.conv1.weight.is_cuda:
            self._pack()
        return r

    def load_state_dict(self, state_dict, strict: bool = True, *args, **kwargs):
        r = super().load_state_dict(state_dict, strict, *args, **kwargs)
        self._packed = None
        if self.conv1.weight.is_cuda:
            self._pack()
        return r

    def _pack(self):
        P: Dict[str, object] = {}
        for name in _CONVS3:
            c = getattr(self, name)
            P[name] = _Conv(pack_valid(c.weight), c.out_channels, c.bias.detach().float().contiguous())
        for dname, cname, cin, cout in _MERGES:
            dw = getattr(self, dname).weight.detach().float().reshape(cin, 9).contiguous()
            c = getattr(self, cname)
            P[cname] = (dw, _Conv(pack_1x1(c.weight), cout, c.bias.detach().float().contiguous()))
        c = self.conv18
        P["conv18"] = _Conv(pack_conv3d(c.weight), c.out_channels, c.bias.detach().float().contiguous())
        self._packed, self._packed_dev = P, self.conv1.weight.device

    # ---- forward ----
    def forward(self, x: torch.Tensor, trace: Optional[Dict[str, torch.Tensor]] = None):
        """x [B, 1, D, H, W] float32 on the device -> affinities [B, output_nc, D-28, h, w] (h, w: see ``network_shapes``; 268 -> 56).
        trace: optional dict that receives conv1-8, conv10/11, conv13/14, conv16/17 (after leaky_relu) and mc1-3 as [B, C, D, H, W] views.
        With show_feature the result is the reference's tuple (conv8, conv11, conv14, conv17, output)."""
        if x.dim() != 5 or x.shape[1] != 1:
            raise ValueError(f"UNet3D_MALA: input must be [B, 1, D, H, W], got {tuple(x.shape)}")
        B, _, D, H, W = x.shape
        network_shapes(D, H, W)
        if not x.is_cuda or x.dtype != torch.float32:
            raise ValueError("UNet3D_MALA: input must be float32 on the device")
        if self._packed is None or self._packed_dev != x.device:
            if self.conv1.weight.device != x.device:
                raise ValueError("UNet3D_MALA: move the model to the input's device first (model.to(device))")
            self._pack()
        P = self._packed
        keep = (lambda k, t: trace.__setitem__(k, t.permute(0, 4, 1, 2, 3))) if trace is not None else (lambda k, t: None)
        acts: Dict[str, torch.Tensor] = {}

        def conv(name, h):
            L = P[name]
            acts[name] = conv3d_valid(h, L.wp, L.cout, L.bias, ACT_LRELU_005)
            keep(name, acts[name])
            return acts[name]

        h = x.contiguous().view(B, D, H, W, 1)
        h = maxpool_133(conv("conv2", conv("conv1", h)))
        h = maxpool_133(conv("conv4", conv("conv3", h)))
        h = maxpool_133(conv("conv6", conv("conv5", h)))
        h = conv("conv8", conv("conv7", h))
        for (_, cname, _, _), mc, skip, (ca, cb) in zip(_MERGES, ["mc1", "mc2", "mc3"], ["conv6", "conv4", "conv2"],
                                                        [("conv10", "conv11"), ("conv13", "conv14"), ("conv16", "conv17")]):
            dw, L = P[cname]
            h = mala_merge(h, dw, L.wp, L.cout, L.bias, acts[skip])
            keep(mc, h)
            h = conv(cb, conv(ca, h))
        L = P["conv18"]
        y = conv3d(h, L.wp, L.cout, 1, 1, bias=L.bias, act=ACT_SIGMOID if self.if_sigmoid else ACT_NONE, ncdhw=True)
        if self.show_feature:
            return tuple(acts[k].permute(0, 4, 1, 2, 3) for k in ("conv8", "conv11", "conv14", "conv17")) + (y,)
        return y


def eager_forward(m: UNet3D_MALA, x: torch.Tensor) -> torch.Tensor:
    """The reference's forward in eager torch.nn.functional with m's parameters (MIOpen on the device): the yardstick of
    scripts/affinity_bench.py --model mala and the FLOP count of the tests.  Not used by ``UNet3D_MALA.forward``."""
    def lr(t):
        return F.leaky_relu(t, _SLOPE)

    def crop_add(up, bypass):
        c = (bypass.size()[3] - up.size()[3]) // 2
        cc = (bypass.size()[2] - up.size()[2]) // 2
        return up + F.pad(bypass, (-c, -c, -c, -c, -cc, -cc))
    c1 = lr(m.conv1(x))
    c2 = lr(m.conv2(c1))
    c4 = lr(m.conv4(lr(m.conv3(m.pool1(c2)))))
    c6 = lr(m.conv6(lr(m.conv5(m.pool2(c4)))))
    c8 = lr(m.conv8(lr(m.conv7(m.pool3(c6)))))
    c11 = lr(m.conv11(lr(m.conv10(crop_add(m.conv9(m.dconv1(c8)), c6)))))
    c14 = lr(m.conv14(lr(m.conv13(crop_add(m.conv12(m.dconv2(c11)), c4)))))
    c17 = lr(m.conv17(lr(m.conv16(crop_add(m.conv15(m.dconv3(c14)), c2)))))
    y = m.conv18(c17)
    return torch.sigmoid(y) if m.if_sigmoid else y


def build_from_config(model_cfg: dict) -> UNet3D_MALA:
    """UNet3D_MALA from the MODEL block of the reference's seg_*_MALA.yaml (inference_seg.py:72-75)."""
    if model_cfg.get("model_type") != "mala":
        raise NotImplementedError(f"model_type {model_cfg.get('model_type')!r}: this builds 'mala'")
    return UNet3D_MALA(output_nc=model_cfg["output_nc"], if_sigmoid=model_cfg.get("if_sigmoid", True),
                       init_mode=model_cfg.get("init_mode_mala", "kaiming"))


# --------------------------------------------------------------------------------------------------------------------------- volumes

def plan_windows_mala(shape: Sequence[int]) -> WindowPlan:
    """Provider_valid's plan for 'mala' on a [Z, H, W] volume: reflect padding (14, 106, 106), windows of 53x268x268 at stride 25x56x56,
    Z/25 x 19 x 19 of them, origins clamped to the padded end, in index order (z outer, then H, then W).  An origin is where the window starts
    in the padded volume and also where its 25x56x56 prediction starts in the unpadded one.  ValueError when Z is not a multiple of 25 (the
    reference asserts), H or W <= 106 (reflect padding of 106), or the windows leave voxels uncovered."""
    Z, H, W = (int(s) for s in shape)
    if Z <= 0 or Z % OUT[0]:
        raise ValueError(f"plan_windows_mala: {Z} slices; the reference needs a multiple of 25")
    if H <= NET_PAD[1] or W <= NET_PAD[2]:
        raise ValueError(f"plan_windows_mala: {H}x{W}: reflect padding of 106 needs H, W > 106")
    padded = (Z + 2 * NET_PAD[0], H + 2 * NET_PAD[1], W + 2 * NET_PAD[2])
    counts = (Z // OUT[0], NUM_XY, NUM_XY)
    for a in range(3):
        if (counts[a] - 1) * OUT[a] + CROP[a] < padded[a]:
            raise ValueError(f"plan_windows_mala: {counts[a]} windows at stride {OUT[a]} leave voxels of axis {a} (extent {shape[a]}) "
                             f"uncovered")

    def starts(a):
        return [min(i * OUT[a], padded[a] - CROP[a]) for i in range(counts[a])]
    org = [(z, y, x) for z in starts(0) for y in starts(1) for x in starts(2)]
    return WindowPlan((Z, H, W), NET_PAD, padded, np.asarray(org, dtype=np.int32))


def gather_windows_mala(vol: torch.Tensor, plan: WindowPlan, origins_dev: torch.Tensor, k0: int, nb: int) -> torch.Tensor:
    """Windows k0 .. k0+nb-1 of the plan as [nb, 1, 53, 268, 268] float32 (uint8 voxels / 255), reflect-padded on the fly."""
    Z, H, W = plan.shape
    out = torch.empty((nb, 1) + CROP, dtype=torch.float32, device=vol.device)
    _abi.check(_abi.load().gpemsr_affinity_gather(vol.data_ptr(), int(vol.dtype == torch.uint8), Z, H, W, *plan.pad, origins_dev[k0:].data_ptr(),
                                                  nb, *CROP, out.data_ptr(), _stream()), "affinity_gather")
    return out


def place_windows(preds: torch.Tensor, origins_dev: torch.Tensor, origins: np.ndarray, out: torch.Tensor) -> None:
    """Provider_valid.add_vol for 'mala': preds [nw, nc, 25, 56, 56] written into out [nc, Z, H, W] at origins [nw, 3] (device; the host
    copy bounds the launch); overlaps resolve to the last window in index order."""
    nw, nc = preds.shape[:2]
    if preds.dim() != 5 or tuple(preds.shape[2:]) != OUT or out.dim() != 4 or out.shape[0] != nc or not preds.is_contiguous() \
            or not out.is_contiguous():
        raise ValueError(f"place_windows: predictions {tuple(preds.shape)} into {tuple(out.shape)}")
    lo, hi = origins.min(axis=0), origins.max(axis=0) + np.asarray(OUT)
    bbox = (C.c_int32 * 6)(int(lo[0]), int(lo[1]), int(lo[2]), int(hi[0] - lo[0]), int(hi[1] - lo[1]), int(hi[2] - lo[2]))
    _abi.check(_abi.load().gpemsr_affinity_place(preds.data_ptr(), nc, origins_dev.data_ptr(), nw, *OUT, out.data_ptr(), *out.shape[1:],
                                                 bbox, _stream()), "affinity_place")


def predict_volume_mala(model: Optional[UNet3D_MALA], vol: torch.Tensor, batch: int = 4,
                        predict: Optional[Callable[[torch.Tensor, int], torch.Tensor]] = None) -> torch.Tensor:
    """Provider_valid + the inference loop of inference_seg.py for 'mala': vol [Z, H, W] uint8 (or float32 in [0, 1]) on the device ->
    affinities [C, Z, H, W] float32 on the device.  Windows run ``batch`` at a time, in index order; each prediction overwrites its
    25x56x56 block (the last window wins), voxels no window covers stay 0.  predict(x [nb, 1, 53, 268, 268], k0) -> [nb, C, 25, 56, 56]
    replaces the model (k0: index of the batch's first window)."""
    if vol.dim() != 3 or not vol.is_cuda or vol.dtype not in (torch.uint8, torch.float32):
        raise ValueError("predict_volume_mala: vol must be a [Z, H, W] uint8 or float32 tensor on the device")
    if batch < 1:
        raise ValueError("predict_volume_mala: batch must be >= 1")
    vol = vol.contiguous()
    plan = plan_windows_mala(vol.shape)
    dev = vol.device
    if predict is None:
        if model is None:
            raise ValueError("predict_volume_mala: a model or a predict function is needed")
        predict = lambda x, k0: model(x)  # noqa: E731
    org = torch.from_numpy(plan.origins).to(dev)
    out = None
    with torch.no_grad():
        for k0 in range(0, plan.n, batch):
            nb = min(batch, plan.n - k0)
            preds = predict(gather_windows_mala(vol, plan, org, k0, nb), k0)
            if preds.dim() != 5 or preds.shape[0] != nb or tuple(preds.shape[2:]) != OUT:
                raise ValueError(f"predict_volume_mala: predictions of shape {tuple(preds.shape)}")
            preds = preds.contiguous()
            if out is None:
                out = torch.zeros((preds.shape[1],) + plan.shape, dtype=torch.float32, device=dev)
            place_windows(preds, org[k0:k0 + nb], plan.origins[k0:k0 + nb], out)
    return out


# --------------------------------------------------------------------------------------------------------------------------- accounting

def _layers(D: int, H: int, W: int) -> List[Tuple[str, int, int, int, Tuple[int, int, int]]]:
    """(kind, cin, cout, taps, output (d, h, w)) of every matrix-pipe layer of one [1, 1, D, H, W] forward (merges at the low resolution)."""
    s = network_shapes(D, H, W)
    widths = dict(conv1=(1, 12), conv2=(12, 12), conv3=(12, 60), conv4=(60, 60), conv5=(60, 300), conv6=(300, 300), conv7=(300, 1500),
                  conv8=(1500, 1500), conv10=(300, 300), conv11=(300, 300), conv13=(60, 60), conv14=(60, 60), conv16=(12, 12), conv17=(12, 12))
    L = []
    for name in _CONVS3:
        ci, co = widths[name]
        L.append(("thin" if co <= THIN_MAX_COUT else "wide", ci, co, 27, s[name]))
    for (_, _, ci, co), mc in zip(_MERGES, ["mc1", "mc2", "mc3"]):
        d, h, w = s[mc]
        L.append(("merge", ci, co, 9, (d, h // 3, w // 3)))       # 9 sub-positions x a 1x1 GEMM at the low resolution
    L.append(("out", 12, 3, 1, s["conv17"]))
    return L


def executed_flop_ratio(D: int = 53, H: int = 268, W: int = 268) -> Tuple[float, float]:
    """(algorithmic GFLOP of the convolutions, executed / algorithmic) of one [1, 1, D, H, W] forward on the MFMA tiles of
    csrc/conv3d_mala.hip: thin layers pad cin to 4, cout to 16 and y / x to 4-voxel blocks; wide layers and merges pad M to 128 and cout to
    16; the 1x1 output layer (gpemsr_conv3d) runs 2 x 8 x 16 tiles with cout padded to 16."""
    def up(a, b):
        return -(-a // b) * b
    alg = exe = 0.0
    for kind, ci, co, taps, (d, h, w) in _layers(D, H, W):
        f = 2.0 * d * h * w * ci * co * taps
        alg += f
        if kind == "thin":
            exe += 2.0 * d * up(h, 4) * up(w, 4) * up(ci, 4) * up(co, 16) * taps
        elif kind in ("wide", "merge"):
            exe += 2.0 * up(d * h * w, 128) * up(co, 16) * up(ci, 4) * taps
        else:
            exe += 2.0 * up(d, 2) * up(h, 8) * up(w, 16) * up(ci, 4) * up(co, 16) * taps
    return alg / 1e9, exe / alg
