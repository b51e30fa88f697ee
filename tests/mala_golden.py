"""Shared by scripts/gen_golden_affinity_mala.py and the MALA tests: the seeded parts of tests/golden/affinity_mala*.npz (inputs and every
parameter of the golden network -- conv8's weight alone is 243 MB), each regenerated here and checked against the SHA-256 the generator
recorded."""
import json

import numpy as np
import torch

from affinity_golden import sha256, window_input  # noqa: F401  (re-exported for the tests)

SLOPE = 0.005


def param(shape, index: int, seed: int = 0, fan_in: int = 1) -> np.ndarray:
    """State-dict entry number `index` of the golden network: weights kaiming-normal (fan_in, leaky_relu gain with slope 0.005, as the
    reference's init), biases uniform in +-1/sqrt(fan_in) (torch's default)."""
    rng = np.random.default_rng([seed, index])
    if len(shape) == 5:
        fan_in = int(np.prod(shape[1:]))
        std = np.sqrt(2.0 / (1.0 + SLOPE ** 2)) / np.sqrt(fan_in)
        return (rng.standard_normal(shape, dtype=np.float32) * np.float32(std)).astype(np.float32)
    return rng.uniform(-1.0, 1.0, size=shape).astype(np.float32) * np.float32(1.0 / np.sqrt(fan_in))


def state_dict(G) -> "dict[str, torch.Tensor]":
    """The golden network's state dict, regenerated from the manifest (key, shape, fan_in of biases) and checked against its SHA-256s."""
    sd = {}
    for i, (k, shape, fan_in) in enumerate(json.loads(str(G["manifest"]))):
        a = param(tuple(shape), i, int(G["seed"]), fan_in)
        if sha256(a) != str(G[f"sha/{k}"]):
            raise AssertionError(f"regenerated {k} differs from the golden's (numpy Generator stream changed?)")
        sd[k] = torch.from_numpy(a)
    return sd


def synth_preds(xc: np.ndarray, k: int) -> np.ndarray:
    """Closed-form window 'prediction' of the stitching golden: the window's centre xc [25, 56, 56] float32 and its index k ->
    [3, 25, 56, 56], frac(float32((c+1)*0.618) * xc) + k.  The integer part names the window, so the overlap order is visible."""
    out = []
    for c in range(3):
        t = np.float32((c + 1) * 0.618) * xc
        out.append((t - np.floor(t)) + np.float32(k))
    return np.stack(out).astype(np.float32)
