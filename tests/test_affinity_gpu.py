"""Affinity step on the device: the HIP UNet_PNI against the unmodified reference (tests/golden/affinity_unet_pni.npz), every conv3d
configuration against torch's fp64 conv3d on the host, the window gather / stitching against the reference's float32 sequence
(tests/golden/affinity_windows.npz), predict_volume and the inference_seg.py CLI end to end."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIPPED = dict(filters=[28, 36, 48, 64, 80], upsample_mode="bilinear", merge_mode="add")
HOOKS = ["embed_in", "conv0", "conv1", "conv2", "conv3", "center", "cat0", "cat1", "cat2", "cat3", "conv4", "conv5", "conv6", "conv7",
         "embed_out"]
DEV = torch.device("cuda", 0)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import affinity_golden as AG  # noqa: E402


@pytest.fixture(scope="module")
def G(golden_dir):
    return np.load(os.path.join(golden_dir, "affinity_unet_pni.npz"))


@pytest.fixture(scope="module")
def W(golden_dir):
    return np.load(os.path.join(golden_dir, "affinity_windows.npz"))


@pytest.fixture(scope="module")
def model(G):
    from gpemsr_amd.affinity import UNet_PNI
    m = UNet_PNI(**SHIPPED)
    m.load_state_dict(AG.state_dict(G), strict=True)
    return m.to(DEV).eval()


def synth_affs(x: torch.Tensor) -> torch.Tensor:
    """scripts/gen_golden_affinity.py::synth_affs on the device: [nb, 1, D, H, W] -> [nb, 3, D, H, W], frac(float32((c+1)*0.618) * x)."""
    out = []
    for c in range(3):
        t = x[:, 0] * float(np.float32((c + 1) * 0.618))
        out.append(t - torch.floor(t))
    return torch.stack(out, dim=1)


@pytest.mark.parametrize("case", ["win", "small"])
def test_unet_matches_reference(G, model, case):
    shape = tuple(int(s) for s in G[f"{case}/act/embed_in/shape"])
    shape = (shape[0], 1) + shape[2:]
    xn = AG.window_input(shape, int(G[f"{case}/x_seed"]))
    assert AG.sha256(xn) == str(G[f"{case}/x_sha256"])
    trace = {}
    with torch.no_grad():
        y = model(torch.from_numpy(xn).to(DEV), trace=trace)
    torch.cuda.synchronize()
    y = y.cpu().numpy()
    assert y.shape == tuple(G[f"{case}/y_shape"]) and 0.0 <= y.min() and y.max() <= 1.0
    err = np.abs(y.reshape(-1)[G[f"{case}/y_idx"]] - G[f"{case}/y_val"]).max()
    assert err <= 2e-5, f"affinities differ by {err:.3e}"
    for name in HOOKS:
        a = trace[name].contiguous().cpu().numpy()
        assert a.shape == tuple(G[f"{case}/act/{name}/shape"]), name
        e = np.abs(a.reshape(-1)[G[f"{case}/act/{name}/idx"]] - G[f"{case}/act/{name}/val"]).max() / float(G[f"{case}/act/{name}/maxabs"])
        assert e <= 1e-5, f"{name}: relative error {e:.3e}"


CONV_CASES = [  # cin, cout, kd, ks, epilogue
    (28, 28, 3, 3, "res_bn_elu"), (36, 36, 3, 3, "bn_elu"), (48, 48, 3, 3, "none"), (64, 64, 3, 3, "res_bn_elu"), (80, 80, 3, 3, "bn_elu"),
    (28, 36, 1, 3, "bn_elu"), (36, 48, 1, 3, "bn_elu"), (48, 64, 1, 3, "bn_elu"), (64, 80, 1, 3, "none"), (80, 80, 1, 3, "bn_elu"),
    (1, 28, 1, 5, "bias_elu"), (28, 28, 1, 5, "bias_elu"), (28, 3, 1, 1, "bias_sigmoid"), (80, 64, 1, 1, "bias"), (36, 28, 1, 1, "bias"),
    (28, 36, 3, 3, "res_bn_elu"),
]


@pytest.mark.parametrize("cin,cout,kd,ks,epi", CONV_CASES)
def test_conv3d_against_fp64(cin, cout, kd, ks, epi):
    from gpemsr_amd import _abi
    from gpemsr_amd.affinity import conv3d, pack_conv3d
    g = torch.Generator().manual_seed(cin * 1000 + cout * 10 + kd + ks)
    B, D, H, Wd = 2, 5, 24, 40                     # odd depth, ragged 8 x 16 tiles
    x = torch.randn(B, cin, D, H, Wd, generator=g)
    w = torch.randn(cout, cin, kd, ks, ks, generator=g) / np.sqrt(cin * kd * ks * ks)
    bias = torch.randn(cout, generator=g) if "bias" in epi else None
    sc = torch.rand(cout, generator=g) + 0.5 if "bn" in epi else None
    sh = torch.randn(cout, generator=g) * 0.2 if "bn" in epi else None
    res = torch.randn(B, cout, D, H, Wd, generator=g) if "res" in epi else None
    act = _abi.ACT_ELU if "elu" in epi else (_abi.ACT_SIGMOID if "sigmoid" in epi else _abi.ACT_NONE)
    want = F.conv3d(x.double(), w.double(), None if bias is None else bias.double(), padding=(kd // 2, ks // 2, ks // 2))
    if res is not None:
        want = want + res.double()
    if sc is not None:
        want = want * sc.double().view(1, -1, 1, 1, 1) + sh.double().view(1, -1, 1, 1, 1)
    want = F.elu(want) if act == _abi.ACT_ELU else (torch.sigmoid(want) if act == _abi.ACT_SIGMOID else want)
    # strided channel slices: input at channel 3 of a (cin + 7)-wide buffer, output at channel 5 of a (cout + 6)-wide one, residual at 1
    xb = torch.zeros(B, D, H, Wd, cin + 7, device=DEV)
    xb[..., 3:3 + cin] = x.permute(0, 2, 3, 4, 1).to(DEV)
    rb = None
    if res is not None:
        rb = torch.zeros(B, D, H, Wd, cout + 2, device=DEV)
        rb[..., 1:1 + cout] = res.permute(0, 2, 3, 4, 1).to(DEV)
    outs = []
    for _ in range(2):
        ob = torch.full((B, D, H, Wd, cout + 6), 7.0, device=DEV)
        conv3d(xb[..., 3:3 + cin], pack_conv3d(w.to(DEV)), cout, kd, ks, bias=None if bias is None else bias.to(DEV),
               scale=None if sc is None else sc.to(DEV), shift=None if sh is None else sh.to(DEV),
               residual=None if rb is None else rb[..., 1:1 + cout], act=act, out=ob[..., 5:5 + cout])
        torch.cuda.synchronize()
        outs.append(ob.cpu())
    assert torch.equal(outs[0], outs[1]), "two launches differ"
    assert (outs[0][..., :5] == 7.0).all() and (outs[0][..., 5 + cout:] == 7.0).all(), "wrote outside the output slice"
    got = outs[0][..., 5:5 + cout].permute(0, 4, 1, 2, 3).double()
    err = float((got - want).abs().max() / want.abs().max())
    assert err <= 1e-5, f"relative error {err:.3e}"


def test_conv3d_ncdhw_output_and_upsample_merge():
    from gpemsr_amd.affinity import conv3d, pack_conv3d, upsample_merge
    g = torch.Generator().manual_seed(7)
    x = torch.randn(2, 3, 8, 16, 28, generator=g)          # [B, D, H, W, C]
    w = torch.randn(3, 28, 1, 1, 1, generator=g)
    b = torch.randn(3, generator=g)
    y = conv3d(x.to(DEV), pack_conv3d(w.to(DEV)), 3, 1, 1, bias=b.to(DEV), ncdhw=True)
    want = F.conv3d(x.permute(0, 4, 1, 2, 3).double(), w.double(), b.double())
    assert float((y.cpu().double() - want).abs().max() / want.abs().max()) <= 1e-5
    low = torch.randn(2, 3, 5, 7, 12, generator=g)
    skip = torch.randn(2, 3, 10, 14, 12, generator=g)
    sc, sh = torch.rand(12, generator=g) + 0.5, torch.randn(12, generator=g)
    got = upsample_merge(low.to(DEV), skip.to(DEV), sc.to(DEV), sh.to(DEV)).cpu().double()
    up = F.interpolate(low.permute(0, 4, 1, 2, 3).double(), scale_factor=(1, 2, 2), mode="trilinear", align_corners=True)
    want = F.elu((up + skip.permute(0, 4, 1, 2, 3).double()) * sc.double().view(1, -1, 1, 1, 1) + sh.double().view(1, -1, 1, 1, 1))
    assert float((got.permute(0, 4, 1, 2, 3) - want).abs().max()) <= 1e-5


def test_gather_reproduces_reflect_padded_windows():
    from gpemsr_amd.affinity import plan_windows, gather_windows
    vol = np.random.default_rng(3).integers(0, 256, size=(20, 1024, 1024), dtype=np.uint8)
    plan = plan_windows(vol.shape)
    padded = np.pad(vol.astype(np.float64), ((4, 4), (48, 48), (48, 48)), mode="reflect")
    vd, org = torch.from_numpy(vol).to(DEV), torch.from_numpy(plan.origins).to(DEV)
    for k0 in range(0, plan.n, 64):
        nb = min(64, plan.n - k0)
        got = gather_windows(vd, plan, org, k0, nb).cpu().numpy()
        for j in range(nb):
            z, y, x = plan.origins[k0 + j]
            want = padded[z:z + 18, y:y + 160, x:x + 160].astype(np.float32) / 255.0
            assert np.array_equal(got[j, 0], want), f"window {k0 + j}"
    # float32 volumes are gathered as they are
    vf = torch.from_numpy(vol.astype(np.float32) / 255.0).to(DEV)
    got = gather_windows(vf, plan, org, 100, 3).cpu().numpy()
    z, y, x = plan.origins[101]
    assert np.array_equal(got[1, 0], padded[z:z + 18, y:y + 160, x:x + 160].astype(np.float32) / 255.0)


def test_stitching_bit_equal_to_reference(W):
    from gpemsr_amd.affinity import predict_volume
    vol = np.random.default_rng(int(W["stitch/seed"])).integers(0, 256, size=(50, 1024, 1024), dtype=np.uint8)
    res = predict_volume(None, torch.from_numpy(vol).to(DEV), batch=16, weight=AG.weight_volume(W), predict=synth_affs)
    out = res.cpu().numpy()
    assert out.shape == (3, 50, 1024, 1024) and out.dtype == np.float32
    np.testing.assert_array_equal(out.reshape(-1)[W["stitch/idx"]], W["stitch/val"])
    assert AG.sha256(out) == str(W["stitch/sha256"])


def _host_stitch(plan, preds, weight):
    """Provider_valid.add_vol / get_results in numpy float32, window by window in index order."""
    Zp, Hp, Wp = plan.padded
    out = np.zeros((3, Zp, Hp, Wp), dtype=np.float32)
    wmap = np.zeros((1, Zp, Hp, Wp), dtype=np.float32)
    w = weight[np.newaxis]
    for k, (z, y, x) in enumerate(plan.origins):
        out[:, z:z + 18, y:y + 160, x:x + 160] += preds[k] * w
        wmap[:, z:z + 18, y:y + 160, x:x + 160] += w
    out = out / wmap
    pz, py, px = plan.pad
    return out[:, pz:-pz, py:-py, px:-px]


def test_predict_volume_equals_per_window_forward_and_is_reproducible(model):
    from gpemsr_amd.affinity import plan_windows, gather_windows, get_weight, predict_volume
    vol = np.random.default_rng(9).integers(0, 256, size=(20, 1024, 1024), dtype=np.uint8)
    vd = torch.from_numpy(vol).to(DEV)
    plan = plan_windows(vol.shape)
    assert plan.n == 338
    a = predict_volume(model, vd, batch=8).cpu().numpy()
    b = predict_volume(model, vd, batch=8).cpu().numpy()
    assert np.array_equal(a, b), "two runs differ"
    org = torch.from_numpy(plan.origins).to(DEV)
    preds = np.empty((plan.n, 3, 18, 160, 160), dtype=np.float32)
    with torch.no_grad():
        for k in range(plan.n):
            preds[k] = model(gather_windows(vd, plan, org, k, 1))[0].cpu().numpy()
    want = _host_stitch(plan, preds, get_weight())
    assert np.array_equal(a, want)
    assert 0.0 <= a.min() and a.max() <= 1.0


def test_cli_end_to_end(tmp_path, G, model):
    from gpemsr_amd import png as gpng
    from gpemsr_amd.affinity import predict_volume
    vol = np.random.default_rng(11).integers(0, 256, size=(20, 1024, 1024), dtype=np.uint8)
    data = tmp_path / "x8"
    data.mkdir()
    files = gpng.encode_gray8(torch.from_numpy(vol).to(DEV)).cpu().numpy()
    for i in range(20):
        (data / f"{105 + i}.png").write_bytes(files[i].tobytes())
    sd = {"module." + k: v for k, v in AG.state_dict(G).items()}
    torch.save({"model_weights": sd}, tmp_path / "superhuman.pt")
    from test_affinity_cpu import _write_yaml
    _write_yaml(tmp_path / "seg.yaml")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "inference_seg.py"), "-c", str(tmp_path / "seg.yaml"), "--data", str(data),
                        "--ckpt", str(tmp_path / "superhuman.pt"), "--out", str(tmp_path / "out"), "-ts", "20", "--batch", "8"],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    affs = np.load(tmp_path / "out" / "affs.npy")
    assert affs.shape == (3, 20, 1024, 1024) and affs.dtype == np.float32
    assert 0.0 <= affs.min() and affs.max() <= 1.0
    assert "Inference time=" in (tmp_path / "out" / "scores.txt").read_text()
    want = predict_volume(model, torch.from_numpy(vol).to(DEV), batch=8).cpu().numpy()
    assert np.array_equal(affs, want)
