"""oracle/make_golden_transformer.py -- TEST INFRASTRUCTURE ONLY (fixture generator).

Imports the reference's projects/SeqFormer/seqformer/models/deformable_transformer.py under a
synthetic package (its two relative imports -- `.ops.modules.MSDeformAttn` and
`..util.misc.inverse_sigmoid` -- are satisfied with the reference's own module file driven by
the reference's pure-PyTorch op, and the reference's own inverse_sigmoid cut out with ast), runs
a small clip through it in fp64 and stores state dict, inputs and outputs in
tests/golden/transformer_seqformer.npz.  It then runs the same transformer once more in train() mode (dropout is
0) with gradients on, applies seeded upstream gradients to every output the detector consumes -- hs, hs_box, memory,
init_ref and the per-layer box predictions, formed as the detector forms them (segmentation_condInst.py:134-150) -- and
stores those gradients and the resulting gradients of every parameter, src{i}, pos{i} and query_embed in
tests/golden/transformer_seqformer_grad.npz.

    python -m oracle.make_golden_transformer
"""
from __future__ import annotations

import importlib.util
import os
import sys
import types

import numpy as np
import torch

from oracle.make_golden_modules import load_module_class
from oracle.ref_extract import extract

REF = "/root/reference/projects/SeqFormer/seqformer"
OUT_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden")


def main():
    torch.set_default_dtype(torch.float64)
    MSDeformAttn = load_module_class(f"{REF}/models/ops/modules/ms_deform_attn.py", "_ref_seq_ops2")
    inv = extract(f"{REF}/util/misc.py", ["inverse_sigmoid"])["inverse_sigmoid"]
    pkg = "_ref_seq_pkg"
    for name in (pkg, pkg + ".models", pkg + ".models.ops", pkg + ".models.ops.modules", pkg + ".util",
                 pkg + ".util.misc"):
        sys.modules[name] = types.ModuleType(name)
        sys.modules[name].__path__ = []
    sys.modules[pkg + ".models.ops.modules"].MSDeformAttn = MSDeformAttn
    sys.modules[pkg + ".util.misc"].inverse_sigmoid = inv
    spec = importlib.util.spec_from_file_location(pkg + ".models.deformable_transformer",
                                                  f"{REF}/models/deformable_transformer.py")
    mod = importlib.util.module_from_spec(spec)
    mod.__package__ = pkg + ".models"
    sys.modules[spec.name] = mod
    spec.loader.exec_module(mod)

    torch.manual_seed(31)      # the constructors below draw their initial weights from the GLOBAL generator: seeded, so that this
    # script regenerates its fixture bit for bit (round-5 review; as make_golden_modules.py)
    gen = torch.Generator().manual_seed(31)
    C, M, L, P, T, N, Q = 32, 1, 3, 4, 2, 2, 6
    tr = mod.DeformableTransformer(d_model=C, nhead=M, num_encoder_layers=1, num_decoder_layers=2,
                                   dim_feedforward=48, dropout=0.0, return_intermediate_dec=True,
                                   num_frames=T, num_feature_levels=L, dec_n_points=P, enc_n_points=P).double()
    with torch.no_grad():
        for p in tr.parameters():
            p.add_(0.05 * torch.randn(p.shape, generator=gen))
    # box refinement heads, as DeformableDETR installs them (deformable_detr.py:95-103)
    bbox = torch.nn.ModuleList([torch.nn.Sequential(torch.nn.Linear(C, C), torch.nn.ReLU(), torch.nn.Linear(C, 4))
                                for _ in range(2)]).double()
    tr.decoder.bbox_embed = bbox
    tr.eval()
    sizes = [(6, 8), (3, 4), (2, 2)]
    srcs = [torch.randn(N, T, C, h, w, generator=gen) for h, w in sizes]
    poss = [torch.randn(N, T, C, h, w, generator=gen) for h, w in sizes]
    masks = []
    for h, w in sizes:
        m = torch.zeros(N, T, h, w, dtype=torch.bool)
        m[1, :, :, w - max(1, w // 4):] = True     # second clip is padded on the right
        masks.append(m)
    query_embed = torch.randn(Q, 2 * C, generator=gen)
    with torch.no_grad():
        hs, hs_box, memory, init_ref, inter_refs, _, _, valid_ratios = tr(srcs, masks, poss, query_embed)
    d = {f"sd.{k}": v.numpy() for k, v in tr.state_dict().items()}
    for i, (s, p, m) in enumerate(zip(srcs, poss, masks)):
        d[f"src{i}"], d[f"pos{i}"], d[f"mask{i}"] = s.numpy(), p.numpy(), m.numpy()
    d.update(query_embed=query_embed.numpy(), hs=hs.numpy(), hs_box=hs_box.numpy(), memory=memory.numpy(),
             init_ref=init_ref.numpy(), inter_refs=inter_refs.numpy(), valid_ratios=valid_ratios.numpy(),
             cfg=np.array([C, M, L, P, T, 1, 2, 48]))
    path = os.path.join(OUT_DIR, "transformer_seqformer.npz")
    np.savez_compressed(path, **d)
    print("transformer fixture", os.path.getsize(path) // 1024, "KiB", tuple(hs.shape), tuple(hs_box.shape))
    write_gradients(tr, inv, srcs, poss, masks, query_embed)


def detector_boxes(bbox_embed, hs_box, init_ref, inter_refs, inverse_sigmoid):
    """The per-layer box predictions as the reference detector forms them (segmentation_condInst.py:134-150)."""
    boxes = []
    for lvl in range(hs_box.shape[0]):
        reference = inverse_sigmoid(init_ref if lvl == 0 else inter_refs[lvl - 1])
        tmp = bbox_embed[lvl](hs_box[lvl])
        if reference.shape[-1] == 4:
            tmp = tmp + reference
        else:
            tmp = torch.cat([tmp[..., :2] + reference, tmp[..., 2:]], -1)
        boxes.append(tmp.sigmoid())
    return torch.stack(boxes)


def write_gradients(tr, inv, srcs, poss, masks, query_embed):
    """train() mode, gradients on: loss = sum_k <G_k, out_k> over the outputs the detector consumes."""
    tr.train()
    tr.zero_grad()
    gen = torch.Generator().manual_seed(131)
    srcs = [s.clone().requires_grad_(True) for s in srcs]
    poss = [p.clone().requires_grad_(True) for p in poss]
    query_embed = query_embed.clone().requires_grad_(True)
    hs, hs_box, memory, init_ref, inter_refs, _, _, _ = tr(srcs, masks, poss, query_embed)
    outs = dict(hs=hs, hs_box=hs_box, memory=memory, init_ref=init_ref,
                boxes=detector_boxes(tr.decoder.bbox_embed, hs_box, init_ref, inter_refs, inv))
    gs = {k: torch.randn(v.shape, generator=gen) for k, v in outs.items()}
    sum((gs[k] * v).sum() for k, v in outs.items()).backward()
    d = {f"G.{k}": v.numpy() for k, v in gs.items()}
    d["boxes"] = outs["boxes"].detach().numpy()
    d.update({f"grad.{n}": p.grad.numpy() for n, p in tr.named_parameters() if p.grad is not None})
    for i, (s, p) in enumerate(zip(srcs, poss)):
        d[f"grad.src{i}"], d[f"grad.pos{i}"] = s.grad.numpy(), p.grad.numpy()
    d["grad.query_embed"] = query_embed.grad.numpy()
    path = os.path.join(OUT_DIR, "transformer_seqformer_grad.npz")
    np.savez_compressed(path, **d)
    print("transformer gradient fixture", os.path.getsize(path) // 1024, "KiB,",
          sum(1 for k in d if k.startswith("grad.")), "gradients")


if __name__ == "__main__":
    main()
