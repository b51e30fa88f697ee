"""Shared by scripts/gen_golden_affinity.py and the affinity tests: the parts of tests/golden/affinity_*.npz that are regenerated rather
than stored (seeded inputs and convolution weights, the blending weight from its stored octant), so the files stay small.  Every
regenerated array is checked against a SHA-256 that the generator recorded."""
import hashlib
import json

import numpy as np
import torch


def sha256(a: np.ndarray) -> str:
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def window_input(shape, seed: int) -> np.ndarray:
    """Network inputs of affinity_unet_pni.npz."""
    return np.random.default_rng(seed).random(shape, dtype=np.float32)


def conv_weight(shape, index: int, seed: int = 0) -> np.ndarray:
    """Kaiming-normal (fan_in, gain sqrt 2) convolution weight number `index` (state-dict order) of the golden network."""
    fan_in = int(np.prod(shape[1:]))
    return (np.random.default_rng([seed, index]).standard_normal(shape, dtype=np.float32) * np.float32(np.sqrt(2.0 / fan_in))).astype(np.float32)


def is_conv_weight(key: str, shape) -> bool:
    return key.endswith(".weight") and len(shape) == 5


def state_dict(G) -> "dict[str, torch.Tensor]":
    """The golden network's full state dict: stored entries + regenerated convolution weights (each checked against its SHA-256)."""
    sd = {}
    for i, (k, shape, _) in enumerate(json.loads(str(G["manifest"]))):
        if is_conv_weight(k, shape):
            w = conv_weight(tuple(shape), i, int(G["conv_seed"]))
            if sha256(w) != str(G[f"wsha/{k}"]):
                raise AssertionError(f"regenerated {k} differs from the golden's (numpy Generator stream changed?)")
            sd[k] = torch.from_numpy(w)
        else:
            sd[k] = torch.from_numpy(np.asarray(G[f"sd/{k}"]))
    return sd


def weight_volume(W) -> np.ndarray:
    """get_weight() [18, 160, 160] from its stored octant (the volume is mirror-symmetric on every axis), checked against its SHA-256."""
    o = W["weight_octant"]
    z = np.concatenate([o, o[::-1]], axis=0)
    y = np.concatenate([z, z[:, ::-1]], axis=1)
    w = np.ascontiguousarray(np.concatenate([y, y[:, :, ::-1]], axis=2))
    if sha256(w) != str(W["weight_sha256"]):
        raise AssertionError("weight volume rebuilt from its octant differs from the golden's")
    return w
