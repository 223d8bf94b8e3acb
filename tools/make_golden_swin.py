"""Write tests/golden/swin_*.npz from the reference's Swin backbone (CPU, float64).

    python tools/make_golden_swin.py --vnext /path/to/VNext

imports projects/SeqFormer/seqformer/backbone/swin.py of a VNext checkout UNMODIFIED.  Neither timm nor detectron2 is
needed: small stand-ins for the names that file imports (timm.models.layers.{DropPath, to_2tuple, trunc_normal_} and
detectron2.modeling.{BACKBONE_REGISTRY, Backbone, ShapeSpec}) are placed in sys.modules first.  The fixtures run with
drop_path_rate 0, so the DropPath stand-in is never called, and trunc_normal_ only initialises values the recipe then
overwrites.  Weights and inputs come from tests/swin_golden_recipe.py; rerunning rewrites byte-identical files.
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
import swin_golden_recipe as R  # noqa: E402


def _install_stand_ins():
    import torch.nn as nn

    class DropPath(nn.Module):
        def __init__(self, p=0.0):
            super().__init__()
            self.p = p

        def forward(self, x):
            raise RuntimeError("the fixtures run without stochastic depth")

    def to_2tuple(x):
        return tuple(x) if isinstance(x, (tuple, list)) else (x, x)

    def trunc_normal_(t, mean=0.0, std=1.0, a=-2.0, b=2.0):
        return nn.init.trunc_normal_(t, mean=mean, std=std, a=a, b=b)

    layers = types.ModuleType("timm.models.layers")
    layers.DropPath, layers.to_2tuple, layers.trunc_normal_ = DropPath, to_2tuple, trunc_normal_
    timm = types.ModuleType("timm")
    models = types.ModuleType("timm.models")
    timm.models, models.layers = models, layers

    class _Registry:
        def register(self, obj=None):
            return (lambda c: c) if obj is None else obj

    class Backbone(nn.Module):
        pass

    modeling = types.ModuleType("detectron2.modeling")
    modeling.BACKBONE_REGISTRY, modeling.Backbone = _Registry(), Backbone
    modeling.ShapeSpec = lambda **kw: types.SimpleNamespace(**kw)
    d2 = types.ModuleType("detectron2")
    d2.modeling = modeling
    sys.modules.update({"timm": timm, "timm.models": models, "timm.models.layers": layers, "detectron2": d2,
                        "detectron2.modeling": modeling})


def load_reference(vnext: str):
    _install_stand_ins()
    path = os.path.join(vnext, "projects", "SeqFormer", "seqformer", "backbone", "swin.py")
    spec = importlib.util.spec_from_file_location("reference_swin", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def run_case(ref, name, case):
    torch.manual_seed(0)
    if case["kind"] == "model":
        model = ref.SwinTransformer(embed_dim=case["embed_dim"], depths=case["depths"], num_heads=case["num_heads"],
                                    window_size=case["window_size"], drop_path_rate=0.0).double()
        keys = list(model.state_dict().keys())
        R.fill_params(model, case["seed"])
        x = R.make_input(case).requires_grad_(True)
        outputs = model(x)
    else:
        layer = ref.BasicLayer(dim=case["dim"], depth=2, num_heads=case["num_heads"], window_size=case["window_size"])
        layer.blocks = torch.nn.ModuleList([layer.blocks[1]])          # the SW-MSA block alone (BasicLayer builds its mask)
        assert layer.blocks[0].shift_size == case["shift_size"] == layer.shift_size
        layer = layer.double()
        model = layer.blocks[0]
        keys = list(model.state_dict().keys())
        R.fill_params(model, case["seed"])
        x = R.make_input(case).requires_grad_(True)
        outputs = {"out": layer(x, case["H"], case["W"])[0]}
    dig = R.digest(model, x.detach())
    R.loss(outputs, R.loss_weights(outputs, case["seed"])).backward()
    arrays = R.summarise(outputs, x.grad, dict(model.named_parameters()), case["seed"])
    arrays["digest"] = np.array(dig)
    arrays["state_keys"] = np.array(keys)
    return arrays


def save_npz(path, arrays):
    """np.savez's format with fixed member timestamps, so that a rerun rewrites the same bytes"""
    import io
    import zipfile
    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_DEFLATED) as z:
        for k in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arrays[k]), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            z.writestr(info, buf.getvalue())


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--vnext", required=True, help="root of a VNext checkout (the reference)")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden"))
    args = ap.parse_args()
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    ref = load_reference(args.vnext)
    for name, case in R.CASES.items():
        arrays = run_case(ref, name, case)
        path = os.path.join(args.out, f"{name}.npz")
        save_npz(path, arrays)
        print(f"{path}: {os.path.getsize(path)} bytes, {len(arrays)} arrays")


if __name__ == "__main__":
    main()
