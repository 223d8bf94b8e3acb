"""Write tests/golden/resnet_d2_r50.npz and resnet_d2_r101.npz from detectron2's ResNet (CPU, float64).

    python tools/make_golden_resnet.py --vnext /path/to/VNext

executes detectron2/modeling/backbone/resnet.py of a VNext checkout UNMODIFIED and builds the network from its own
BasicStem, BottleneckBlock and ResNet.make_default_stages.  Neither detectron2 (its compiled extension) nor fvcore needs to
be importable: small stand-ins for the names that file imports -- fvcore.nn.weight_init.c2_msra_fill,
detectron2.layers.{CNNBlockBase, Conv2d, DeformConv, ModulatedDeformConv, ShapeSpec, get_norm}, the Backbone base class and
BACKBONE_REGISTRY -- are placed in sys.modules first.  The stand-in Conv2d is torch's convolution followed by its `norm`,
the stand-in frozen batch norm is x * scale + shift with detectron2's buffer names and eps; the deformable convolutions are
never constructed.  Weights and the input come from tests/resnet_golden_recipe.py; rerunning rewrites byte-identical files.
"""
from __future__ import annotations

import argparse
import importlib.util
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import resnet_golden_recipe as R  # noqa: E402
from make_golden_swin import save_npz  # noqa: E402


def _install_stand_ins():
    from torch import nn

    class FrozenBatchNorm2d(nn.Module):
        def __init__(self, num_features, eps=1e-5):
            super().__init__()
            self.eps = eps
            for name, value in (("weight", 1.0), ("bias", 0.0), ("running_mean", 0.0), ("running_var", 1.0)):
                self.register_buffer(name, torch.full((num_features,), value))

        def forward(self, x):
            scale = self.weight * (self.running_var + self.eps).rsqrt()
            shift = self.bias - self.running_mean * scale
            return x * scale.reshape(1, -1, 1, 1) + shift.reshape(1, -1, 1, 1)

    def get_norm(norm, channels):
        if norm != "FrozenBN":
            raise RuntimeError("the fixtures run with frozen batch norm")
        return FrozenBatchNorm2d(channels)

    class Conv2d(nn.Conv2d):
        def __init__(self, *args, norm=None, activation=None, **kwargs):
            super().__init__(*args, **kwargs)
            self.norm, self.activation = norm, activation

        def forward(self, x):
            x = super().forward(x)
            if self.norm is not None:
                x = self.norm(x)
            return self.activation(x) if self.activation is not None else x

    class CNNBlockBase(nn.Module):
        def __init__(self, in_channels, out_channels, stride):
            super().__init__()
            self.in_channels, self.out_channels, self.stride = in_channels, out_channels, stride

    class _Never(nn.Module):
        def __init__(self, *a, **k):
            raise RuntimeError("the fixtures have no deformable stage")

    class _Registry:
        def register(self, obj=None):
            return (lambda c: c) if obj is None else obj

    class Backbone(nn.Module):
        pass

    def module(name, **names):
        m = types.ModuleType(name)
        m.__path__ = []      # a package: the file's relative imports resolve against sys.modules
        for k, v in names.items():
            setattr(m, k, v)
        sys.modules[name] = m
        return m

    module("fvcore")
    module("fvcore.nn")
    module("fvcore.nn.weight_init", c2_msra_fill=lambda layer: None)      # the recipe overwrites every value
    sys.modules["fvcore.nn"].weight_init = sys.modules["fvcore.nn.weight_init"]
    module("detectron2")
    module("detectron2.layers", CNNBlockBase=CNNBlockBase, Conv2d=Conv2d, DeformConv=_Never, ModulatedDeformConv=_Never,
           ShapeSpec=lambda **kw: types.SimpleNamespace(**kw), get_norm=get_norm)
    module("detectron2.modeling")
    module("detectron2.modeling.backbone")
    module("detectron2.modeling.backbone.backbone", Backbone=Backbone)
    module("detectron2.modeling.backbone.build", BACKBONE_REGISTRY=_Registry())


def load_reference(vnext: str):
    _install_stand_ins()
    path = os.path.join(vnext, "detectron2", "modeling", "backbone", "resnet.py")
    spec = importlib.util.spec_from_file_location("detectron2.modeling.backbone.resnet", path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = mod
    spec.loader.exec_module(mod)
    return mod


def run_case(ref, case):
    stages = ref.ResNet.make_default_stages(case["depth"], norm="FrozenBN", stride_in_1x1=False)
    model = ref.ResNet(ref.BasicStem(3, 64, norm="FrozenBN"), stages, out_features=list(R.OUTPUTS)).double().eval()
    own = model.state_dict()
    keys = list(own.keys())
    state = R.reference_state([(k, own[k].shape) for k in keys], case["seed"])
    model.load_state_dict(state, strict=True)
    x = R.make_input(case)
    with torch.no_grad():
        outs = model(x)
    arrays = {name: outs[name].numpy() for name in R.OUTPUTS}
    arrays["state_keys"] = np.array(keys)
    arrays["digest"] = np.array(R.digest(state, x))
    return arrays


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--vnext", required=True, help="root of a VNext checkout (the reference)")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden"))
    args = ap.parse_args()
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    ref = load_reference(args.vnext)
    for name, case in R.CASES.items():
        arrays = run_case(ref, case)
        path = os.path.join(args.out, f"{name}.npz")
        save_npz(path, arrays)
        print(f"{path}: {os.path.getsize(path)} bytes, {len(arrays)} arrays")


if __name__ == "__main__":
    main()
