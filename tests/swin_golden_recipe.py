"""Seed-to-weights recipe of the Swin fixtures (tests/golden/swin_*.npz), shared by tools/make_golden_swin.py (which runs the
reference's backbone/swin.py) and the tests (which run vnext_amd/models/swin.py).

A fixture stores no weights and no input: both are regenerated here from the case's seed, in float64, and checked against
the stored digest.  What it stores are the reference's results, computed in float64: a strided sample and seeded random
projections of every output and of the input gradient, and the parameter gradients of the loss
sum_k <out_k, R_k> (R_k seeded Gaussian): in full for the small tensors (relative-position tables, qkv biases, norms),
as seeded projections for the others.
"""
from __future__ import annotations

import hashlib

import numpy as np
import torch

CASES = {
    # window 7, padding at every stage (32 x 48 -> 16 x 24 -> 8 x 12 -> 4 x 6 tokens), stage 4 smaller than a window
    "swin_w7": dict(kind="model", seed=7001, input=(2, 3, 128, 192), embed_dim=32, depths=[2, 2, 2, 2],
                    num_heads=[1, 2, 4, 8], window_size=7),
    # window 12 (Swin-L's), 56 x 88 -> 28 x 44 -> 14 x 22 -> 7 x 11 tokens
    "swin_w12": dict(kind="model", seed=7002, input=(1, 3, 224, 352), embed_dim=32, depths=[2, 2, 2, 2],
                     num_heads=[1, 2, 4, 8], window_size=12),
    # one SW-MSA block at Swin-L stage-1 width on the 23 x 40 grid of stage 4 at 720p
    "swin_block_l": dict(kind="block", seed=7003, dim=192, num_heads=6, window_size=12, shift_size=6, H=23, W=40, batch=1),
}
N_PROJ = 16            # projections per stored array
MAX_SAMPLE = 4096      # elements of a strided sample


def is_small(name: str) -> bool:
    """parameters whose gradient is stored in full"""
    return (name.endswith("relative_position_bias_table") or name.endswith("qkv.bias") or ".norm" in "." + name
            or name.startswith("norm"))


def fill_params(module: torch.nn.Module, seed: int) -> None:
    """Overwrite every parameter of `module` (float64) with seeded values, in sorted-name order."""
    g = torch.Generator().manual_seed(seed)
    params = dict(module.named_parameters())
    with torch.no_grad():
        for name in sorted(params):
            p = params[name]
            r = torch.randn(p.shape, generator=g, dtype=torch.float64)
            if name.endswith("relative_position_bias_table"):
                v = 0.5 * r
            elif p.dim() == 1 and ("norm" in name) and name.endswith("weight"):
                v = 1.0 + 0.2 * r
            elif p.dim() == 1:
                v = 0.2 * r
            else:
                v = r / np.sqrt(p[0].numel())
            p.copy_(v.to(p.dtype))


def make_input(case: dict) -> torch.Tensor:
    g = torch.Generator().manual_seed(case["seed"] + 1)
    if case["kind"] == "model":
        shape = case["input"]
    else:
        shape = (case["batch"], case["H"] * case["W"], case["dim"])
    return torch.randn(shape, generator=g, dtype=torch.float64)


def digest(module: torch.nn.Module, x: torch.Tensor) -> str:
    h = hashlib.sha256()
    params = dict(module.named_parameters())
    for name in sorted(params):
        h.update(name.encode())
        h.update(params[name].detach().double().contiguous().numpy().tobytes())
    h.update(x.detach().double().contiguous().numpy().tobytes())
    return h.hexdigest()


def _vectors(numel: int, seed: int, n: int = N_PROJ) -> torch.Tensor:
    return torch.randn(n, numel, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


def loss_weights(outputs: dict, seed: int) -> dict:
    """R_k of the loss sum_k <out_k, R_k>, one seeded Gaussian per output, in sorted-key order"""
    g = torch.Generator().manual_seed(seed + 2)
    return {k: torch.randn(outputs[k].shape, generator=g, dtype=torch.float64) for k in sorted(outputs)}


def loss(outputs: dict, weights: dict) -> torch.Tensor:
    return sum((outputs[k] * weights[k].to(outputs[k])).sum() for k in sorted(outputs))


def projections(a: torch.Tensor, seed: int) -> np.ndarray:
    v = _vectors(a.numel(), seed)
    return (v @ a.detach().double().reshape(-1).cpu()).numpy()


def sample(a: torch.Tensor) -> np.ndarray:
    flat = a.detach().double().reshape(-1).cpu()
    step = max(1, flat.numel() // MAX_SAMPLE)
    return flat[::step].numpy()


def summarise(outputs: dict, x_grad: torch.Tensor, params: dict, seed: int) -> dict:
    """the arrays a fixture stores (outputs, input gradient, parameter gradients)"""
    out = {}
    for i, k in enumerate(sorted(outputs)):
        out[f"out_{k}_sample"] = sample(outputs[k])
        out[f"out_{k}_proj"] = projections(outputs[k], seed + 100 + i)
    out["gin_sample"] = sample(x_grad)
    out["gin_proj"] = projections(x_grad, seed + 99)
    for i, name in enumerate(sorted(params)):
        g = params[name].grad
        if is_small(name):
            out[f"g_{name}"] = g.detach().double().cpu().numpy()
        else:
            out[f"gp_{name}"] = projections(g, seed + 1000 + i)
    return out
