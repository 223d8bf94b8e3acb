"""Seed-to-weights recipe of the ResNet fixtures (tests/golden/resnet_d2_r*.npz), shared by tools/make_golden_resnet.py
(which runs detectron2's own BasicStem / BottleneckBlock / ResNet.make_default_stages) and tests/test_resnet_depth.py
(which runs vnext_amd/models/resnet.py).

A fixture stores no weights and no input.  Every tensor of the state dict is regenerated here, in float64, from the case's
seed and the tensor's REFERENCE name (detectron2's: `stem.conv1.norm.running_var`, `res4.7.shortcut.weight`), so the values
do not depend on either implementation's registration order, and a test has to carry them into the trunk through
`load_reference_checkpoint` -- a wrong name map puts them in the wrong place and the outputs disagree.  What a fixture
stores: the reference's state-dict key list, in its order, and its res3 / res4 / res5 outputs for the case's input.
"""
from __future__ import annotations

import hashlib

import numpy as np
import torch

CASES = {
    "resnet_d2_r50": dict(depth=50, seed=5001, input=(1, 3, 32, 48)),
    "resnet_d2_r101": dict(depth=101, seed=5101, input=(1, 3, 32, 48)),
}
OUTPUTS = ("res3", "res4", "res5")


def _generator(seed: int, name: str) -> torch.Generator:
    word = hashlib.sha256(f"{seed}:{name}".encode()).digest()[:8]
    return torch.Generator().manual_seed(int.from_bytes(word, "little") >> 1)


def tensor_for(name: str, shape, seed: int) -> torch.Tensor:
    """the float64 value of the tensor the reference calls `name`"""
    r = torch.randn(tuple(shape), generator=_generator(seed, name), dtype=torch.float64)
    if name.endswith("running_var"):
        return 0.5 + r.abs()
    if name.endswith("norm.weight"):
        return (0.5 if ".conv3." in name else 1.0) + 0.1 * r
    if name.endswith("norm.bias") or name.endswith("running_mean"):
        return 0.1 * r
    fan_in = int(np.prod(shape[1:]))
    return r * (2.0 / fan_in) ** 0.5      # a convolution's filters


def reference_state(keys_and_shapes, seed: int) -> dict:
    """{reference name: tensor} for [(reference name, shape)]"""
    return {k: tensor_for(k, s, seed) for k, s in keys_and_shapes}


def make_input(case: dict) -> torch.Tensor:
    return torch.randn(case["input"], generator=_generator(case["seed"], "input"), dtype=torch.float64)


def digest(state: dict, x: torch.Tensor) -> str:
    h = hashlib.sha256()
    for name in sorted(state):
        h.update(name.encode())
        h.update(state[name].detach().double().contiguous().numpy().tobytes())
    h.update(x.detach().double().contiguous().numpy().tobytes())
    return h.hexdigest()
