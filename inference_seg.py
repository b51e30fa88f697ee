"""Affinity inference for an SR volume: the affinity half of the reference's ``inference_code/inference_seg.py`` on HIP.

    python inference_seg.py -c seg_x8_superhuman.yaml --data <dir with 0.png ... 124.png> --ckpt superhuman.pt --out <dir> [-ts 50] [--batch N]
    python inference_seg.py -c seg_x8_MALA.yaml --data <dir> --ckpt MALA.pt --out <dir> [-ts 50] [--batch N]

* reads the reference's YAML unchanged and dispatches on ``MODEL.model_type``: 'superhuman' -> gpemsr_amd.affinity.UNet_PNI (Gaussian-blended
  18x160x160 windows), 'mala' -> gpemsr_amd.affinity_mala.UNet3D_MALA (53x268x268 windows, 25x56x56 predictions placed last-wins; ``-ts``
  must be a multiple of 25)
* loads the checkpoint as the reference does (``model_weights``, DataParallel prefix stripped)
* reads only the slices it uses: the reference loads 0.png .. 124.png and keeps the last ``-ts`` (provider_valid.py:77-83), so this reads
  ``(N - ts).png .. (N - 1).png`` (N = --num-slices, 125), decoded on the device when they are 8-bit grayscale PNGs (gpemsr_amd.png)
* writes ``affs.npy`` ([3, Z, H, W] float32, the reference's layout), ``affs.hdf`` (dataset 'main') when h5py is importable, and
  ``scores.txt`` with the inference time.

Watershed, waterz agglomeration and VOI / ARAND scoring are not part of this tool.
"""
from __future__ import annotations

import argparse
import os
import sys
import time
from typing import List, Optional, Sequence

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def parse_args(argv: Optional[Sequence[str]] = None) -> argparse.Namespace:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("-c", "--cfg", required=True, help="the reference's seg_*_superhuman.yaml or seg_*_MALA.yaml")
    ap.add_argument("--data", required=True, help="directory holding the SR slices <i>.png")
    ap.add_argument("--ckpt", required=True, help="superhuman.pt or MALA.pt (checkpoint['model_weights'])")
    ap.add_argument("--out", required=True, help="output directory (created)")
    ap.add_argument("-ts", "--test_split", type=int, default=50,
                    help="use the last TS slices (superhuman: 20, 25, 50, 100 or 200; MALA: a multiple of 25)")
    ap.add_argument("--num-slices", type=int, default=125, help="slices in the directory's numbering (0 .. N-1; the reference's 125)")
    ap.add_argument("--batch", type=int, default=4, help="windows per network call")
    a = ap.parse_args(argv)
    if a.test_split < 1 or a.test_split > a.num_slices:
        ap.error(f"-ts {a.test_split} outside 1..{a.num_slices}")
    if a.batch < 1:
        ap.error("--batch must be >= 1")
    return a


def slice_paths(data_dir: str, ts: int, num_slices: int = 125) -> List[str]:
    """The files the reference keeps: the last `ts` of 0.png .. (num_slices-1).png, in order."""
    paths = [os.path.join(data_dir, f"{i}.png") for i in range(num_slices - ts, num_slices)]
    missing = [p for p in paths if not os.path.isfile(p)]
    if missing:
        raise FileNotFoundError(f"{len(missing)} slice(s) missing, first: {missing[0]}")
    return paths


def load_model_cfg(path: str) -> dict:
    import yaml
    with open(path) as f:
        cfg = yaml.safe_load(f)
    model = cfg.get("MODEL")
    if not isinstance(model, dict):
        raise ValueError(f"{path}: no MODEL block")
    shift = (cfg.get("DATA") or {}).get("shift_channels")
    if shift is not None:
        raise NotImplementedError("shift_channels variants are not built (output_nc 3 only)")
    if model.get("output_nc") != 3:
        raise NotImplementedError("output_nc must be 3")
    return model


def _module(model_cfg: dict):
    """The module that builds and runs the configured network: gpemsr_amd.affinity (superhuman) or gpemsr_amd.affinity_mala (mala)."""
    kind = model_cfg.get("model_type", "superhuman")
    if kind == "mala":
        from gpemsr_amd import affinity_mala as M
    elif kind == "superhuman":
        from gpemsr_amd import affinity as M
    else:
        raise NotImplementedError(f"model_type {kind!r}: 'superhuman' or 'mala'")
    return M


def build_model(model_cfg: dict):
    return _module(model_cfg).build_from_config(model_cfg)


def check_test_split(model_cfg: dict, ts: int) -> None:
    """The reference's MALA provider asserts a multiple of 25 slices (provider_valid.py:114); superhuman plans are checked by plan_windows."""
    if model_cfg.get("model_type") == "mala" and ts % 25:
        raise ValueError(f"-ts {ts}: MALA needs a multiple of 25 slices")


def read_volume(paths: Sequence[str], device):
    """[Z, H, W] volume on the device: float32 / 255 through the device PNG decoder when every file allows it, else uint8 read on the host."""
    import numpy as np
    import torch
    from gpemsr_amd import png as gpng
    blobs = [open(p, "rb").read() for p in paths]
    dec = gpng.device_decodable(blobs)
    if dec is not None:
        h, w, payloads = dec
        vol, status = gpng.decode_gray8(payloads, h, w, device)
        torch.cuda.current_stream().synchronize()
        gpng.check_status(status, list(paths))
        return vol[:, 0]
    from PIL import Image
    import io
    arr = np.stack([np.asarray(Image.open(io.BytesIO(b))) for b in blobs])
    if arr.ndim != 3:
        raise ValueError("slices must be single-channel images")
    return torch.from_numpy(arr.astype(np.uint8)).to(device)


def main(argv: Optional[Sequence[str]] = None) -> int:
    args = parse_args(argv)
    import numpy as np
    import torch
    model_cfg = load_model_cfg(args.cfg)
    check_test_split(model_cfg, args.test_split)
    A = _module(model_cfg)
    mala = model_cfg.get("model_type") == "mala"
    paths = slice_paths(args.data, args.test_split, args.num_slices)
    if not torch.cuda.is_available():
        raise RuntimeError("inference_seg.py needs a HIP device (there is no CPU path)")
    dev = torch.device("cuda", 0)
    os.makedirs(args.out, exist_ok=True)
    model = build_model(model_cfg)
    model.load_state_dict(A.load_checkpoint(args.ckpt))
    model = model.to(dev).eval()
    vol = read_volume(paths, dev)
    plan = A.plan_windows_mala(vol.shape) if mala else A.plan_windows(vol.shape)
    print(f"volume {tuple(vol.shape)} {vol.dtype}, {plan.n} windows")
    torch.cuda.synchronize()
    t1 = time.time()
    affs = (A.predict_volume_mala if mala else A.predict_volume)(model, vol, batch=args.batch)
    torch.cuda.synchronize()
    cost = time.time() - t1
    print("Inference time=%.6f" % cost)
    out = affs.cpu().numpy()
    np.save(os.path.join(args.out, "affs.npy"), out)
    with open(os.path.join(args.out, "scores.txt"), "w") as f:
        f.write("Inference time=%.6f\n" % cost)
    try:
        import h5py
    except ImportError:
        h5py = None
    if h5py is not None:
        with h5py.File(os.path.join(args.out, "affs.hdf"), "w") as f:
            f.create_dataset("main", data=out, dtype=np.float32, compression="gzip")
    print(f"wrote {args.out}/affs.npy {out.shape}" + (" + affs.hdf" if h5py is not None else ""))
    return 0


if __name__ == "__main__":
    sys.exit(main())
