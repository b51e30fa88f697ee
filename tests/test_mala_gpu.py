"""MALA affinity step on the device: the HIP UNet3D_MALA against the unmodified reference (tests/golden/affinity_mala.npz), the valid
convolutions, the fused decoder merge and the max pool against torch on the host, the last-wins stitching against the reference's
add_vol (tests/golden/affinity_mala_windows.npz), predict_volume_mala and the inference_seg.py CLI end to end."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = torch.device("cuda", 0)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mala_golden as MG  # noqa: E402
TRACED = ["conv1", "conv2", "conv3", "conv4", "conv5", "conv6", "conv7", "conv8", "conv10", "conv11", "conv13", "conv14", "conv16", "conv17",
          "mc1", "mc2", "mc3"]


@pytest.fixture(scope="module")
def G(golden_dir):
    return np.load(os.path.join(golden_dir, "affinity_mala.npz"))


@pytest.fixture(scope="module")
def W(golden_dir):
    return np.load(os.path.join(golden_dir, "affinity_mala_windows.npz"))


@pytest.fixture(scope="module")
def sd(G):
    return MG.state_dict(G)


@pytest.fixture(scope="module")
def model(sd):
    from gpemsr_amd.affinity_mala import UNet3D_MALA
    m = UNet3D_MALA(output_nc=3)
    m.load_state_dict(sd, strict=True)
    return m.to(DEV).eval()


@pytest.mark.parametrize("case", ["win", "small"])
def test_unet_matches_reference(G, model, case):
    shape = (int(G[f"{case}/act/conv1/shape"][0]), 1) + tuple(int(s) + 2 for s in G[f"{case}/act/conv1/shape"][2:])
    xn = MG.window_input(shape, int(G[f"{case}/x_seed"]))
    assert MG.sha256(xn) == str(G[f"{case}/x_sha256"])
    trace = {}
    with torch.no_grad():
        y = model(torch.from_numpy(xn).to(DEV), trace=trace)
    torch.cuda.synchronize()
    y = y.cpu().numpy()
    errs = {}
    for name in TRACED:                       # in network order: the first failing name is where the computation went wrong
        a = trace[name].contiguous().cpu().numpy()
        assert a.shape == tuple(G[f"{case}/act/{name}/shape"]), name
        errs[name] = np.abs(a.reshape(-1)[G[f"{case}/act/{name}/idx"]] - G[f"{case}/act/{name}/val"]).max() / float(G[f"{case}/act/{name}/maxabs"])
    bad = {k: f"{v:.2e}" for k, v in errs.items() if not v <= 1e-5}
    assert not bad, f"relative errors above 1e-5: {bad}"
    assert y.shape == tuple(G[f"{case}/y_shape"]) and 0.0 <= y.min() and y.max() <= 1.0
    # the reference's own float32 result is within 2e-6 of float64 here (spread/affinity); the bar is 1e-5 absolute
    assert float(G["spread/affinity"]) < 1e-5
    err = np.abs(y.reshape(-1)[G[f"{case}/y_idx"]] - G[f"{case}/y_val"]).max()
    assert err <= 1e-5, f"affinities differ by {err:.3e}"


def test_show_feature_returns_the_reference_tuple(G, sd):
    from gpemsr_amd.affinity_mala import UNet3D_MALA
    m = UNet3D_MALA(output_nc=3, show_feature=True)
    m.load_state_dict(sd, strict=True)
    m = m.to(DEV).eval()
    xn = MG.window_input((2, 1, 40, 214, 241), int(G["small/x_seed"]))
    with torch.no_grad():
        out = m(torch.from_numpy(xn).to(DEV))
    assert len(out) == 5 and tuple(out[4].shape) == (2, 3, 12, 2, 29)
    for t, name in zip(out[:4], ["conv8", "conv11", "conv14", "conv17"]):
        assert tuple(t.shape) == tuple(G[f"small/act/{name}/shape"])
    y = out[4].cpu().numpy()
    assert np.abs(y.reshape(-1)[G["small/y_idx"]] - G["small/y_val"]).max() <= 1e-5


VALID_CASES = [  # B, D, H, W, cin, cout, act
    (2, 5, 9, 13, 1, 12, "lrelu"), (1, 6, 19, 23, 12, 12, "lrelu"), (2, 4, 11, 18, 12, 60, "none"), (1, 5, 14, 21, 60, 60, "lrelu"),
    (2, 3, 7, 5, 5, 7, "sigmoid"), (1, 4, 10, 86, 60, 80, "lrelu"),                          # thin (cout <= 80)
    (2, 5, 8, 9, 1, 300, "lrelu"), (1, 6, 11, 13, 60, 300, "lrelu"), (2, 4, 6, 7, 300, 300, "none"), (1, 5, 8, 8, 300, 1500, "lrelu"),
    (2, 4, 6, 6, 1500, 1500, "lrelu"), (1, 3, 5, 9, 7, 100, "sigmoid"), (2, 3, 6, 5, 13, 81, "lrelu"),   # wide (split K on the small ones)
]


@pytest.mark.parametrize("B,D,H,Wd,cin,cout,act", VALID_CASES)
def test_conv3d_valid_against_fp64(B, D, H, Wd, cin, cout, act):
    from gpemsr_amd import _abi
    from gpemsr_amd.affinity_mala import conv3d_valid, pack_valid
    g = torch.Generator().manual_seed(cin * 7919 + cout * 31 + D * H * Wd)
    x = torch.randn(B, cin, D, H, Wd, generator=g)
    w = torch.randn(cout, cin, 3, 3, 3, generator=g) / np.sqrt(cin * 27)
    bias = torch.randn(cout, generator=g)
    code = {"lrelu": _abi.ACT_LRELU_005, "sigmoid": _abi.ACT_SIGMOID, "none": _abi.ACT_NONE}[act]
    want = F.conv3d(x.double(), w.double(), bias.double())
    want = F.leaky_relu(want, 0.005) if act == "lrelu" else (torch.sigmoid(want) if act == "sigmoid" else want)
    # channel slices: the input at channel 4 of a (cin + 8)-wide buffer, the output at channel 3 of a (cout + 5)-wide one
    xb = torch.zeros(B, D, H, Wd, cin + 8, device=DEV)
    xb[..., 4:4 + cin] = x.permute(0, 2, 3, 4, 1).to(DEV)
    wp = pack_valid(w.to(DEV))
    outs = []
    for _ in range(2):
        ob = torch.full((B, D - 2, H - 2, Wd - 2, cout + 5), 7.0, device=DEV)
        conv3d_valid(xb[..., 4:4 + cin], wp, cout, bias.to(DEV), code, out=ob[..., 3:3 + cout])
        torch.cuda.synchronize()
        outs.append(ob.cpu())
    assert torch.equal(outs[0], outs[1]), "two launches differ"
    assert (outs[0][..., :3] == 7.0).all() and (outs[0][..., 3 + cout:] == 7.0).all(), "wrote outside the output slice"
    got = outs[0][..., 3:3 + cout].permute(0, 4, 1, 2, 3).double()
    err = float((got - want).abs().max() / want.abs().max())
    assert err <= 1e-5, f"relative error {err:.3e}"


MERGE_CASES = [  # B, d, h, w, cin, cout, skip (D, H, W)
    (1, 6, 4, 4, 1500, 300, (10, 24, 24)), (2, 5, 2, 5, 300, 60, (11, 66, 75)), (1, 4, 7, 6, 60, 12, (24, 225, 222)),
    (2, 3, 3, 2, 7, 20, (5, 11, 8)),
]


@pytest.mark.parametrize("B,d,h,w,cin,cout,sk", MERGE_CASES)
def test_merge_against_fp64(B, d, h, w, cin, cout, sk):
    from gpemsr_amd.affinity_mala import mala_merge, pack_1x1
    g = torch.Generator().manual_seed(cin * 13 + cout + d * h * w)
    x = torch.randn(B, cin, d, h, w, generator=g)
    wt = torch.randn(cin, 1, 1, 3, 3, generator=g)
    w1 = torch.randn(cout, cin, 1, 1, 1, generator=g) / np.sqrt(cin)
    b1 = torch.randn(cout, generator=g)
    skip = torch.randn((B, cout) + sk, generator=g)
    up = F.conv3d(F.conv_transpose3d(x.double(), wt.double(), stride=(1, 3, 3), groups=cin), w1.double(), b1.double())
    c, cc = (sk[1] - 3 * h) // 2, (sk[0] - d) // 2
    want = up + F.pad(skip.double(), (-c, -c, -c, -c, -cc, -cc))
    got = mala_merge(x.permute(0, 2, 3, 4, 1).contiguous().to(DEV), wt.reshape(cin, 9).contiguous().to(DEV), pack_1x1(w1.to(DEV)), cout,
                     b1.to(DEV), skip.permute(0, 2, 3, 4, 1).contiguous().to(DEV))
    got = got.cpu().permute(0, 4, 1, 2, 3).double()
    assert got.shape == want.shape
    err = float((got - want).abs().max() / want.abs().max())
    assert err <= 1e-5, f"relative error {err:.3e}"


def test_merge_rejects_what_the_reference_cannot_add():
    from gpemsr_amd.affinity_mala import mala_merge, pack_1x1
    x = torch.randn(1, 5, 2, 2, 8, device=DEV)
    dw, wp = torch.randn(8, 9, device=DEV), pack_1x1(torch.randn(4, 8, 1, 1, 1, device=DEV))
    for sk in [(9, 12, 14), (9, 6, 6), (5, 12, 12)]:               # W difference != 2c; c = 0; cc = 0
        with pytest.raises(ValueError):
            mala_merge(x, dw, wp, 4, None, torch.randn((1,) + sk + (4,), device=DEV))


def test_maxpool_is_exact():
    from gpemsr_amd.affinity_mala import maxpool_133
    g = torch.Generator().manual_seed(3)
    for shape in [(2, 3, 29, 31, 12), (1, 2, 9, 9, 60), (1, 1, 8, 4, 300)]:
        x = torch.randn(shape, generator=g)
        got = maxpool_133(x.to(DEV)).cpu()
        want = F.max_pool3d(x.permute(0, 4, 1, 2, 3), (1, 3, 3), (1, 3, 3)).permute(0, 2, 3, 4, 1)
        assert torch.equal(got, want), shape


def synth(x: torch.Tensor, k0: int) -> torch.Tensor:
    """mala_golden.synth_preds on the device for a batch of windows [nb, 1, 53, 268, 268] whose first index is k0."""
    xc = x[:, 0, 14:39, 106:162, 106:162]
    out = []
    for c in range(3):
        t = xc * float(np.float32((c + 1) * 0.618))
        out.append(t - torch.floor(t))
    k = torch.arange(k0, k0 + x.shape[0], device=x.device, dtype=torch.float32).view(-1, 1, 1, 1)
    return torch.stack([o + k for o in out], dim=1)


def test_stitching_bit_equal_to_reference(W):
    from gpemsr_amd.affinity_mala import predict_volume_mala
    vol = np.random.default_rng(int(W["stitch/seed"])).integers(0, 256, size=(50, 1024, 1024), dtype=np.uint8)
    res = predict_volume_mala(None, torch.from_numpy(vol).to(DEV), batch=16, predict=synth)
    out = res.cpu().numpy()
    assert out.shape == (3, 50, 1024, 1024) and out.dtype == np.float32
    np.testing.assert_array_equal(out.reshape(-1)[W["stitch/idx"]], W["stitch/val"])
    assert MG.sha256(out) == str(W["stitch/sha256"])


def test_predict_volume_equals_per_window_forward_and_is_reproducible(model):
    from gpemsr_amd.affinity_mala import gather_windows_mala, plan_windows_mala, predict_volume_mala
    vol = np.random.default_rng(9).integers(0, 256, size=(25, 150, 131), dtype=np.uint8)
    vd = torch.from_numpy(vol).to(DEV)
    plan = plan_windows_mala(vol.shape)
    assert plan.n == 361
    a = predict_volume_mala(model, vd, batch=4).cpu().numpy()
    b = predict_volume_mala(model, vd, batch=4).cpu().numpy()
    assert np.array_equal(a, b), "two runs differ"
    org = torch.from_numpy(plan.origins).to(DEV)
    want = np.zeros((3,) + plan.shape, dtype=np.float32)
    with torch.no_grad():
        for k in range(plan.n):                       # Provider_valid.add_vol: each window overwrites its block, in index order
            z, y, x = plan.origins[k]
            want[:, z:z + 25, y:y + 56, x:x + 56] = model(gather_windows_mala(vd, plan, org, k, 1))[0].cpu().numpy()
    assert np.array_equal(a, want)
    assert 0.0 <= a.min() and a.max() <= 1.0


def test_cli_end_to_end(tmp_path, sd, model):
    from gpemsr_amd import png as gpng
    from gpemsr_amd.affinity_mala import predict_volume_mala
    vol = np.random.default_rng(11).integers(0, 256, size=(25, 160, 160), dtype=np.uint8)
    data = tmp_path / "x8"
    data.mkdir()
    files = gpng.encode_gray8(torch.from_numpy(vol).to(DEV)).cpu().numpy()
    for i in range(25):
        (data / f"{100 + i}.png").write_bytes(files[i].tobytes())
    torch.save({"model_weights": {"module." + k: v for k, v in sd.items()}}, tmp_path / "MALA.pt")
    from test_mala_cpu import _write_yaml
    _write_yaml(tmp_path / "seg.yaml")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "inference_seg.py"), "-c", str(tmp_path / "seg.yaml"), "--data", str(data),
                        "--ckpt", str(tmp_path / "MALA.pt"), "--out", str(tmp_path / "out"), "-ts", "25", "--batch", "4"],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    affs = np.load(tmp_path / "out" / "affs.npy")
    assert affs.shape == (3, 25, 160, 160) and affs.dtype == np.float32
    assert "Inference time=" in (tmp_path / "out" / "scores.txt").read_text()
    want = predict_volume_mala(model, torch.from_numpy(vol).to(DEV), batch=4).cpu().numpy()
    assert np.array_equal(affs, want)
