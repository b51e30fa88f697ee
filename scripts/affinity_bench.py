"""Affinity U-Net throughput on one device: the HIP UNet_PNI (or, with --model mala, UNet3D_MALA) against the same network in plain
torch.nn (torch-ROCm / MIOpen fp32, TF32 off) with the same weights, in one process, and predict_volume(_mala) on a 50 x 1024 x 1024 uint8
volume.  Prints one JSON line.

    python scripts/affinity_bench.py [--model superhuman|mala] [--batches 1,2,4,8] [--reps 5] [--no-volume]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PEAK_TF = 157.3          # MI355X dense fp32 matrix peak


def torch_reference(m):
    """The same network as eager torch.nn modules (MIOpen convolutions), sharing m's parameters."""
    import torch.nn.functional as F

    def res(x, b):
        r = b.block1(x)
        return b.block4(b.block3(r + b.block2(r)))

    def fwd(x):
        h = m.embed_in(x)
        skips = []
        for name in ["conv0", "conv1", "conv2", "conv3"]:
            h = res(h, getattr(m, name))
            skips.append(h)
            h = F.max_pool3d(h, (1, 2, 2), (1, 2, 2))
        h = res(h, m.center)
        for i in range(4):
            h = getattr(m, f"cat{i}")(getattr(m, f"up{i}")(h) + skips[3 - i])
            h = res(h, getattr(m, f"conv{4 + i}"))
        return torch.sigmoid(m.out_put(m.embed_out(h)))
    return fwd


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,2,4,8")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-volume", action="store_true")
    ap.add_argument("--model", choices=["superhuman", "mala"], default="superhuman")
    a = ap.parse_args()
    if a.model == "mala":
        return main_mala(a)
    from gpemsr_amd import affinity as A
    dev = torch.device("cuda", 0)
    torch.backends.cudnn.allow_tf32 = False
    torch.backends.cuda.matmul.allow_tf32 = False
    torch.manual_seed(0)
    m = A.UNet_PNI(filters=[28, 36, 48, 64, 80], upsample_mode="bilinear", merge_mode="add")
    g = torch.Generator().manual_seed(1)
    for mod in m.modules():
        if isinstance(mod, torch.nn.BatchNorm3d):
            c = mod.num_features
            mod.running_mean.copy_(torch.randn(c, generator=g) * 0.2)
            mod.running_var.copy_(torch.rand(c, generator=g) + 0.5)
    m = m.to(dev).eval()
    ref = torch_reference(m)
    alg, ratio = A.executed_flop_ratio()
    res = {"metric": "affinity_unet_pni", "window": [18, 160, 160], "gflop_per_window": A.WINDOW_GFLOP, "executed_over_algorithmic": round(ratio, 4)}
    per = {}
    with torch.no_grad():
        for b in [int(s) for s in a.batches.split(",")]:
            x = torch.rand(b, 1, 18, 160, 160, device=dev)
            t = timed(lambda: m(x), a.reps)
            per[b] = t / b * 1e3
        best = min(per, key=per.get)
        x = torch.rand(best, 1, 18, 160, 160, device=dev)
        t_ref = timed(lambda: ref(x), a.reps) / best * 1e3
        y_hip, y_ref = m(x), ref(x)
        torch.cuda.synchronize()
        diff = float((y_hip - y_ref).abs().max())
    res.update({
        "hip_ms_per_window": {str(k): round(v, 3) for k, v in per.items()},
        "hip_best_batch": best,
        "hip_tflops": round(A.WINDOW_GFLOP / per[best], 2),
        "hip_share_of_fp32_matrix_peak": round(A.WINDOW_GFLOP / per[best] / PEAK_TF, 4),
        "miopen_ms_per_window": round(t_ref, 3),
        "miopen_tflops": round(A.WINDOW_GFLOP / t_ref, 2),
        "speedup_vs_miopen": round(t_ref / per[best], 3),
        "max_abs_diff_hip_vs_miopen": diff,
    })
    if not a.no_volume:
        vol = torch.from_numpy(np.random.default_rng(5).integers(0, 256, size=(50, 1024, 1024), dtype=np.uint8)).to(dev)
        n = A.plan_windows(vol.shape).n
        A.predict_volume(m, vol, batch=best)
        torch.cuda.synchronize()
        t = time.perf_counter()
        A.predict_volume(m, vol, batch=best)
        torch.cuda.synchronize()
        t = time.perf_counter() - t
        res.update({"volume": [50, 1024, 1024], "windows": n, "volume_s": round(t, 3), "windows_per_s": round(n / t, 1),
                    "volume_tflops": round(n * A.WINDOW_GFLOP / t / 1e3, 2)})
    print(json.dumps(res))


def main_mala(a):
    from gpemsr_amd import affinity_mala as A
    dev = torch.device("cuda", 0)
    torch.backends.cudnn.allow_tf32 = False
    torch.backends.cuda.matmul.allow_tf32 = False
    torch.manual_seed(0)
    m = A.UNet3D_MALA(output_nc=3)
    with torch.no_grad():
        for mod in m.modules():                  # the reference initialises biases to torch's default; kept, but made visible
            if isinstance(mod, torch.nn.Conv3d):
                mod.bias.mul_(0.5)
    m = m.to(dev).eval()
    alg, ratio = A.executed_flop_ratio()
    res = {"metric": "affinity_unet3d_mala", "window": list(A.CROP), "gflop_per_window": A.WINDOW_GFLOP,
           "executed_over_algorithmic": round(ratio, 4)}
    per = {}
    with torch.no_grad():
        for b in [int(s) for s in a.batches.split(",")]:
            x = torch.rand(b, 1, *A.CROP, device=dev)
            per[b] = timed(lambda: m(x), a.reps) / b * 1e3
        best = min(per, key=per.get)
        x = torch.rand(best, 1, *A.CROP, device=dev)
        t_ref = timed(lambda: A.eager_forward(m, x), a.reps) / best * 1e3
        y_hip, y_ref = m(x), A.eager_forward(m, x)
        torch.cuda.synchronize()
        diff = float((y_hip - y_ref).abs().max())
    res.update({
        "hip_ms_per_window": {str(k): round(v, 3) for k, v in per.items()},
        "hip_best_batch": best,
        "hip_tflops": round(A.WINDOW_GFLOP / per[best], 2),
        "hip_share_of_fp32_matrix_peak": round(A.WINDOW_GFLOP / per[best] / PEAK_TF, 4),
        "miopen_ms_per_window": round(t_ref, 3),
        "miopen_tflops": round(A.WINDOW_GFLOP / t_ref, 2),
        "speedup_vs_miopen": round(t_ref / per[best], 3),
        "max_abs_diff_hip_vs_miopen": diff,
    })
    if not a.no_volume:
        vol = torch.from_numpy(np.random.default_rng(5).integers(0, 256, size=(50, 1024, 1024), dtype=np.uint8)).to(dev)
        n = A.plan_windows_mala(vol.shape).n
        A.predict_volume_mala(m, vol, batch=best)
        torch.cuda.synchronize()
        t = time.perf_counter()
        A.predict_volume_mala(m, vol, batch=best)
        torch.cuda.synchronize()
        t = time.perf_counter() - t
        res.update({"volume": [50, 1024, 1024], "windows": n, "volume_s": round(t, 3), "windows_per_s": round(n / t, 1),
                    "volume_tflops": round(n * A.WINDOW_GFLOP / t / 1e3, 2)})
    print(json.dumps(res))


if __name__ == "__main__":
    main()
