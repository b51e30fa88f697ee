"""Affinity step, host side: parameter inventory, window plan, blending weight, options, checkpoint loading, CLI plumbing (no device needed).
Golden vectors: scripts/gen_golden_affinity.py on the unmodified reference."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import affinity_golden as AG  # noqa: E402
SHIPPED = dict(filters=[28, 36, 48, 64, 80], upsample_mode="bilinear", merge_mode="add")


@pytest.fixture(scope="module")
def unet_golden(golden_dir):
    return np.load(os.path.join(golden_dir, "affinity_unet_pni.npz"))


@pytest.fixture(scope="module")
def win_golden(golden_dir):
    return np.load(os.path.join(golden_dir, "affinity_windows.npz"))


def test_parameter_inventory_equals_reference(unet_golden):
    from gpemsr_amd.affinity import UNet_PNI
    sd = UNet_PNI(**SHIPPED).state_dict()
    manifest = json.loads(str(unet_golden["manifest"]))
    assert len(manifest) == 196
    assert [[k, list(v.shape), str(v.dtype).replace("torch.", "")] for k, v in sd.items()] == manifest


def test_load_state_dict_strict_accepts_reference_weights(unet_golden):
    from gpemsr_amd.affinity import UNet_PNI
    m = UNet_PNI(**SHIPPED)
    sd = AG.state_dict(unet_golden)            # stored entries + seeded convolution weights, each checked against its SHA-256
    assert len(sd) == 196
    m.load_state_dict(sd, strict=True)
    assert torch.equal(m.state_dict()["conv0.block2.0.weight"], sd["conv0.block2.0.weight"])
    assert tuple(sd["embed_in.0.weight"].shape) == (28, 1, 1, 5, 5)


@pytest.mark.parametrize("z", [20, 25, 50, 100])
def test_plan_windows_matches_reference_origins(win_golden, z):
    from gpemsr_amd.affinity import plan_windows
    p = plan_windows((z, 1024, 1024))
    np.testing.assert_array_equal(p.origins, win_golden[f"origins/{z}"])
    assert p.padded == (z + 8, 1120, 1120) and p.pad == (4, 48, 48)


def test_plan_windows_rejects_what_the_reference_cannot_do():
    from gpemsr_amd.affinity import plan_windows
    assert plan_windows((200, 1024, 1024)).n == 20 * 169
    for z in (18, 30, 49, 125):
        with pytest.raises(NotImplementedError):
            plan_windows((z, 1024, 1024))
    with pytest.raises(ValueError):
        plan_windows((50, 1100, 1024))      # padded 1196 > 12 * 80 + 160: uncovered voxels (the reference divides by zero there)
    with pytest.raises(ValueError):
        plan_windows((50, 1024, 48))        # smaller than one window after padding
    p = plan_windows((20, 512, 768))        # smaller volumes: end-clamped origins, every voxel covered
    assert p.origins[:, 1].max() == 512 + 96 - 160 and p.origins[:, 2].max() == 768 + 96 - 160


def test_weight_volume_within_one_ulp_of_reference(win_golden):
    from gpemsr_amd.affinity import get_weight
    w, ref = get_weight(), AG.weight_volume(win_golden)
    assert w.shape == ref.shape == (18, 160, 160) and w.dtype == np.float32
    assert np.abs(w.view(np.int32).astype(np.int64) - ref.view(np.int32).astype(np.int64)).max() <= 1


@pytest.mark.parametrize("opt", [dict(), dict(SHIPPED, merge_mode="cat"), dict(SHIPPED, upsample_mode="transposeS"),
                                 dict(SHIPPED, filters=[32, 64, 128, 256, 512]), dict(SHIPPED, relu_mode="relu"),
                                 dict(SHIPPED, pad_mode="replicate"), dict(SHIPPED, out_planes=12), dict(SHIPPED, bn_mode="sync"),
                                 dict(SHIPPED, if_sigmoid=False), dict(SHIPPED, in_planes=2), dict(SHIPPED, show_feature=True)])
def test_unsupported_options_raise(opt):
    from gpemsr_amd.affinity import UNet_PNI
    with pytest.raises(NotImplementedError):
        UNet_PNI(**opt)


def test_forward_refuses_host_tensors_and_bad_shapes():
    from gpemsr_amd.affinity import UNet_PNI
    m = UNet_PNI(**SHIPPED)
    with pytest.raises(ValueError):
        m(torch.zeros(1, 1, 18, 160, 150))
    with pytest.raises(ValueError):
        m(torch.zeros(1, 1, 18, 160, 160))     # host tensor: no CPU path


def test_load_checkpoint_strips_module_prefix(tmp_path):
    from gpemsr_amd.affinity import UNet_PNI, load_checkpoint
    sd = UNet_PNI(**SHIPPED).state_dict()
    torch.save({"model_weights": {"module." + k: v for k, v in sd.items()}, "current_iter": 1}, tmp_path / "superhuman.pt")
    got = load_checkpoint(str(tmp_path / "superhuman.pt"))
    assert list(got) == list(sd)
    UNet_PNI(**SHIPPED).load_state_dict(got, strict=True)


def test_flop_accounting():
    from gpemsr_amd.affinity import executed_flop_ratio
    alg, ratio = executed_flop_ratio()
    # the reference's 173.6 GFLOP applies each up_k 1x1 at the high resolution; here it runs before the interpolation (4x fewer)
    assert 170 < alg < 173.6 and 1.0 < ratio < 1.4


def _write_yaml(path):
    path.write_text("NAME: 'seg_3d'\nMODEL:\n    model_type: 'superhuman'\n    input_nc: 1\n    output_nc: 3\n    if_sigmoid: True\n"
                    "    filters:\n        - 28\n        - 36\n        - 48\n        - 64\n        - 80\n    upsample_mode: 'bilinear'\n"
                    "    decode_ratio: 1\n    merge_mode: 'add'\n    pad_mode: 'zero'\n    bn_mode: 'async'\n    relu_mode: 'elu'\n"
                    "    init_mode: 'kaiming_normal'\nDATA:\n    shift_channels: ~\n")


def test_cli_arguments_and_paths(tmp_path):
    sys.path.insert(0, ROOT)
    import inference_seg as cli
    from gpemsr_amd.affinity import build_from_config
    _write_yaml(tmp_path / "seg.yaml")
    d = tmp_path / "data"
    d.mkdir()
    for i in range(105, 125):
        (d / f"{i}.png").write_bytes(b"")
    a = cli.parse_args(["-c", str(tmp_path / "seg.yaml"), "--data", str(d), "--ckpt", "x.pt", "--out", str(tmp_path / "o"), "-ts", "20"])
    assert a.test_split == 20 and a.batch == 4 and a.num_slices == 125
    paths = cli.slice_paths(a.data, a.test_split, a.num_slices)
    assert [os.path.basename(p) for p in paths] == [f"{i}.png" for i in range(105, 125)]
    with pytest.raises(FileNotFoundError):
        cli.slice_paths(a.data, 21)             # 104.png is not there
    m = build_from_config(cli.load_model_cfg(a.cfg))
    assert len(m.state_dict()) == 196
    with pytest.raises(SystemExit):
        cli.parse_args(["-c", "x", "--data", "d", "--ckpt", "c", "--out", "o", "-ts", "0"])
    # the script itself parses its arguments before it needs a device
    r = subprocess.run([sys.executable, os.path.join(ROOT, "inference_seg.py"), "--help"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "--ckpt" in r.stdout
