"""The fused class and box losses (vnext_amd/csrc/set_loss.hip, vnext_amd/ops/set_loss.py, the criteria's `fused_set_loss`
switch, train.enable_fused_set_loss): per decoder layer the sigmoid focal sum over all logits against the one-hot target
the matched pairs imply, the matched boxes' L1 and GIoU sums and the number of matched queries whose argmax is their label.

The yardstick of the GPU tests is the criteria's own expression (`compose` below: one-hot, focal, gather, L1, `giou_loss`,
per-layer sums, argmax hits) in float64 on the CPU from the same fp32 inputs, under random upstream gradients on the three
differentiable columns.  The bound is not a constant: on every case the same `compose` runs in fp32 on the device, its
error against float64 is measured, and the fused op is allowed MULTIPLE = 4 times that error, with a floor of 4 * 2^-23
where ATen happens to be exact.

Why four.  The kernel evaluates the same fp32 terms; what differs from ATen is the order of the fp32 sums (a lane adds
every 256th group of its piece, a fixed exchange tree joins the lanes, the four waves in order, then the layer's pieces).
tools/set_loss_sum_order.py emulates that order on the CPU over this file's cases, from the fp32 terms ATen itself
computes, and compares it with the error of ATen's own fp32 sum of the same terms.  Measured (CPU, all cases of CASES, 25
column sums): in the kernel's order every sum is within 1.1e-7 of float64 (focal 1.08e-7, L1 8.96e-8, GIoU 7.42e-8 at
worst) -- less than one unit 2^-23 = 1.19e-7 of the result, so all of them sit under the floor of 4 * 2^-23.  The ratio
to ATen's error is 0.11 .. 1.70 wherever ATen itself is at least half a unit (2^-24) from float64 (worst: focal at
`model_shape` 8.4e-8 against 4.9e-8, 1.70; `K7_Q600_no_alpha` 1.61), and reaches 7.2 (focal) and 3.8 (L1) only on
`disjoint_boxes`, where ATen's own sum happens to land within 1.5e-8 / 1.8e-8 of float64 -- a tenth of a unit, by luck of
the rounding; a ratio to such an error measures the luck, which is what the floor is for.  1.7 with headroom for the
per-term differences the emulation does not see (expf / log1pf against ATen's sigmoid and BCE kernels, fused
multiply-adds, ATen's device reduction order against its CPU one) is 4 -- the multiple test_mask_loss.py arrived at the same
way for the same kind of difference; the raw worst ratio, 7.2, would have given a wider bound, not a narrower one.  The
gradients are element-wise (no long sum): the same multiple of ATen's measured element error applies.

Units: absolute error over the case's largest magnitude, per column of the sums and per gradient tensor; exact equality
for the hit counts (every case's logits keep the top two classes of a row more than 1e-3 apart, and predicted and target
boxes come from continuous distributions, so no case depends on an argmax, maximum or minimum tie).  Every test prints
its figures before it asserts.

Measured on an MI355X (worst op error over the nine cases; ATen fp32 on the same case): focal 1.09e-7 (2.6e-8), L1 9.0e-8
(2.6e-8), GIoU 7.4e-8 (4.8e-8) -- all under the floor of 4.8e-7 --, grad_logits 4.0e-7 (9.8e-7), grad_boxes 3.9e-7
(3.9e-7); the largest ratio where ATen itself is at least 2^-24 off: 1.00 on the sums, 1.22 grad_logits, 1.77 grad_boxes
(`K7_Q600_no_alpha`: 3.1e-7 against 1.7e-7).  DESIGN section 14 has the table."""
import functools
import os
import random
import re
import subprocess

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import GOLDEN_DIR, ROOT

DEV = "cuda:0"
EPS = 2.0 ** -23
MULTIPLE = 4
NAMES = ("vnx_set_loss_forward", "vnx_set_loss_backward")


# ---- the yardstick: the criteria's expression, any dtype / device ----------------------------------------------------
def compose(logits, boxes, lay, clip, qry, tgt, labels, tgt_boxes, alpha=0.25):
    """logits [Ld, N, Q, K], boxes [Ld, N, T, Q, 4], the pair list, labels [n], tgt_boxes [n, T, 4] -> [Ld, 4]: the lines
    of `SetCriterion.forward_all_layers` / `IDOLCriterion.forward_all_layers` before their normalisations (per-layer sums
    as IDOL takes them: segment sums over the flat list)"""
    from vnext_amd.models.criterion import box_cxcywh_to_xyxy, giou_loss
    Ld, T = logits.shape[0], boxes.shape[2]
    dev = logits.device
    lay, clip, qry, tgt, labels = (v.to(dev) for v in (lay, clip, qry, tgt, labels))
    onehot = torch.zeros_like(logits)
    onehot[lay, clip, qry, labels[tgt]] = 1
    p = logits.sigmoid()
    ce = F.binary_cross_entropy_with_logits(logits, onehot, reduction="none")
    p_t = p * onehot + (1 - p) * (1 - onehot)
    focal = ce * (1 - p_t) ** 2.0
    if alpha >= 0:
        focal = (alpha * onehot + (1 - alpha) * (1 - onehot)) * focal
    pred = boxes.transpose(2, 3)[lay, clip, qry]                                   # [R, T, 4]
    want = tgt_boxes.to(pred)[tgt]

    def per_layer(values):
        return torch.zeros(Ld, dtype=values.dtype, device=dev).index_add_(0, lay, values)
    l1 = per_layer((pred - want).abs().flatten(1).sum(1))
    g = giou_loss(box_cxcywh_to_xyxy(pred.flatten(0, 1)), box_cxcywh_to_xyxy(want.flatten(0, 1)))
    g = per_layer(g.view(len(lay), T).sum(1))
    with torch.no_grad():
        hits = per_layer((logits[lay, clip, qry].argmax(-1) == labels[tgt]).to(logits.dtype))
    return torch.stack([focal.sum((1, 2, 3)), l1, g, hits], 1)


def fused(logits, boxes, lay, clip, qry, tgt, labels, tgt_boxes, alpha=0.25):
    from vnext_amd.ops.set_loss import set_class_box_losses
    return set_class_box_losses(logits, boxes, lay, clip, qry, tgt, labels, tgt_boxes, alpha)


def run(fn, case, w, dtype=None, device="cpu"):
    """forward + backward under the upstream gradients w [Ld, 3] -> (sums [Ld, 4], grad_logits, grad_boxes), detached"""
    logits, boxes, lay, clip, qry, tgt, labels, tgt_boxes, kw = case
    cast = (lambda v: v.to(device, dtype)) if dtype is not None else (lambda v: v.to(device))
    x = cast(logits.detach()).requires_grad_(True)
    b = cast(boxes.detach()).requires_grad_(True)
    out = fn(x, b, lay.to(device), clip.to(device), qry.to(device), tgt.to(device), labels.to(device),
             cast(tgt_boxes) if dtype is not None else tgt_boxes.to(device), **kw)
    (out[:, :3] * w.to(out)).sum().backward()
    return out.detach(), x.grad.detach(), b.grad.detach()


# ---- cases -----------------------------------------------------------------------------------------------------------
def _boxes(shape, g, kind="random", target=False):
    """cxcywh from continuous distributions.  `disjoint`: predictions in the left third, targets in the right third;
    `nested`: targets large and central, predictions small and inside them"""
    u = lambda lo, hi: lo + (hi - lo) * torch.rand(*shape, 1, generator=g)      # noqa: E731
    if kind == "disjoint":
        c = u(0.70, 0.85) if target else u(0.15, 0.30)
        return torch.cat([c, u(0.2, 0.8), u(0.05, 0.2), u(0.05, 0.4)], -1)
    if kind == "nested":
        if target:
            return torch.cat([u(0.45, 0.55), u(0.45, 0.55), u(0.6, 0.8), u(0.6, 0.8)], -1)
        return torch.cat([u(0.4, 0.6), u(0.4, 0.6), u(0.05, 0.2), u(0.05, 0.2)], -1)
    return torch.cat([u(0.2, 0.8), u(0.2, 0.8), u(0.05, 0.5), u(0.05, 0.5)], -1)


def synthetic(Ld, N, T, Q, K, sizes, per_layer_counts=None, kind="random", seed=0, **kw):
    """sizes: targets per clip.  Pairs: Hungarian-shaped (every target once per layer, a clip's pairs by ascending query)
    or, with `per_layer_counts`, IDOL-shaped (that many selected queries per layer spread over the clips that have
    targets, targets repeating).  Half of the matched rows are pushed towards their label, so hits occur."""
    g = torch.Generator().manual_seed(seed)
    n_tot = sum(sizes)
    start = np.concatenate([[0], np.cumsum(sizes)])
    labels = torch.randint(0, K, (n_tot,), generator=g)
    tgt_boxes = _boxes((n_tot, T), g, kind, target=True)
    logits = torch.randn(Ld, N, Q, K, generator=g) * 2
    boxes = _boxes((Ld, N, T, Q), g, kind)
    lay, clip, qry, tgt = [], [], [], []
    with_targets = [i for i, n in enumerate(sizes) if n]
    for l in range(Ld):
        for i in range(N):
            if per_layer_counts is None:
                n = sizes[i]
            else:                                        # the layer's count split over the clips with targets
                share = [per_layer_counts[l] // len(with_targets) + (1 if j < per_layer_counts[l] % len(with_targets) else 0)
                         for j in range(len(with_targets))]
                n = share[with_targets.index(i)] if i in with_targets else 0
            if n == 0:
                continue
            q = torch.randperm(Q, generator=g)[:n].sort().values
            t = (torch.randperm(sizes[i], generator=g)[:n] if per_layer_counts is None
                 else torch.randint(0, sizes[i], (n,), generator=g)) + int(start[i])
            lay.append(torch.full((n,), l)); clip.append(torch.full((n,), i)); qry.append(q); tgt.append(t)
    cat = lambda v: torch.cat(v).to(torch.int64) if v else torch.zeros(0, dtype=torch.int64)      # noqa: E731
    lay, clip, qry, tgt = cat(lay), cat(clip), cat(qry), cat(tgt)
    push = torch.rand(len(lay), generator=g) < 0.5
    logits[lay[push], clip[push], qry[push], labels[tgt[push]]] += 5.0
    if K > 1:                                            # no argmax tie: the top two of every row more than 1e-3 apart
        top = logits.topk(2, -1)
        close = (top.values[..., 0] - top.values[..., 1]) <= 2e-3
        logits.scatter_add_(-1, top.indices[..., :1], close[..., None].float() * 0.01)
        top = logits.topk(2, -1).values
        assert float((top[..., 0] - top[..., 1]).min()) > 1e-3
    return logits, boxes, lay, clip, qry, tgt, labels, tgt_boxes, kw


def _fixture_seqformer_inputs():
    g = dict(np.load(os.path.join(GOLDEN_DIR, "criterion_seqformer.npz")))
    bs, nf, Q, K, H, W, layers = (int(v) for v in g["cfg"])
    targets = [{"labels": torch.from_numpy(g[f"t{i}.labels"]), "boxes": torch.from_numpy(g[f"t{i}.boxes"]).float(),
                "masks": torch.from_numpy(g[f"t{i}.masks"]).bool()} for i in range(bs)]
    ind = [[(torch.from_numpy(g[f"l{l}.src{i}"]), torch.from_numpy(g[f"l{l}.tgt{i}"])) for i in range(bs)] for l in range(layers)]
    logits = torch.stack([torch.from_numpy(g[f"l{l}.logits"]) for l in range(layers)]).float()
    boxes = torch.stack([torch.from_numpy(g[f"l{l}.boxes"]) for l in range(layers)]).float()
    masks = torch.cat([torch.cat([torch.from_numpy(g[f"l{l}.masks{i}"]) for i in range(bs)], 1)[0] for l in range(layers)]).float()
    want = {k[5:]: float(v) for k, v in g.items() if k.startswith("loss.")}
    return (K, nf), targets, ind, logits, boxes, masks, want


def _fixture_idol_inputs():
    g = dict(np.load(os.path.join(GOLDEN_DIR, "criterion_idol.npz")))
    bz, Q, K, H, W, layers, C = (int(v) for v in g["cfg"])
    det = [{"labels": torch.from_numpy(g[f"det{i}.labels"]), "boxes": torch.from_numpy(g[f"det{i}.boxes"]).float(),
            "masks": torch.from_numpy(g[f"det{i}.masks"]).bool()} for i in range(bz)]
    ind = [[(torch.from_numpy(g[f"l{l}.sel{i}"]), torch.from_numpy(g[f"l{l}.gt{i}"])) for i in range(bz)] for l in range(layers)]
    logits = torch.stack([torch.from_numpy(g[f"l{l}.logits"]) for l in range(layers)]).float()
    boxes = torch.stack([torch.from_numpy(g[f"l{l}.boxes"]) for l in range(layers)]).float()
    masks = torch.cat([torch.cat([torch.from_numpy(g[f"l{l}.masks{i}"]) for i in range(bz)], 1)[0] for l in range(layers)]).float()
    want = {k[5:]: float(v) for k, v in g.items() if k.startswith("loss.")}
    return K, det, ind, logits, boxes, masks, want


CASES = {
    # one clip without targets
    "tiny_one_clip_without_targets": lambda: synthetic(2, 2, 2, 5, 3, [2, 0]),
    # the model's shape: Ld 6, N 2, T 5, Q 300, K 40, 4 + 3 targets
    "model_shape": lambda: synthetic(6, 2, 5, 300, 40, [4, 3], seed=1),
    # K = 1 (every argmax is class 0); Q not a multiple of 64; K % 4 != 0: the element-per-lane path
    "K1_Q70": lambda: synthetic(3, 1, 1, 70, 1, [5], seed=2),
    # the widest supported row; 32 queries per piece -> five pieces per (layer, clip), the last of two queries
    "K128_Q130": lambda: synthetic(2, 3, 1, 130, 128, [3, 2, 4], seed=3),
    # IDOL-shaped ragged list: per-layer counts (7, 0, 19) -- a layer without pairs, several queries per target
    "idol_ragged_7_0_19": lambda: synthetic(3, 2, 1, 100, 40, [3, 2], per_layer_counts=(7, 0, 19), seed=4),
    # the overlap gate's zero branch
    "disjoint_boxes": lambda: synthetic(2, 2, 2, 40, 8, [3, 3], kind="disjoint", seed=5),
    # the hull equals the target
    "predictions_nested_in_their_target": lambda: synthetic(2, 2, 2, 40, 8, [3, 3], kind="nested", seed=6),
    # no pairs at all: the focal column and grad_logits still right, grad_boxes all zero
    "no_pairs": lambda: synthetic(2, 2, 2, 33, 6, [0, 0], seed=7),
    # K % 4 != 0 with more than one piece per (layer, clip) (585 queries per piece), no class weighting
    "K7_Q600_no_alpha": lambda: synthetic(2, 1, 1, 600, 7, [6], seed=8, alpha=-1.0),
}


@functools.lru_cache(maxsize=None)
def case_and_reference(name):
    """(case, upstream gradients [Ld, 3], the float64 result on the CPU): computed once per case, shared, never modified"""
    case = CASES[name]()
    g = torch.Generator().manual_seed(7)
    w = torch.rand(case[0].shape[0], 3, generator=g) + 0.5
    ref = run(compose, case, w.double(), dtype=torch.float64)
    assert all(bool(torch.isfinite(t).all()) for t in ref), name          # `compose` alone is finite on the case
    return case, w, ref


def errors(got, ref):
    """absolute error over the largest magnitude, per column of the sums and per gradient; 0 / 0 = 0"""
    def rel(a, b):
        err, scale = float((a.double().cpu() - b).abs().max()) if b.numel() else 0.0, float(b.abs().max()) if b.numel() else 0.0
        return err / scale if scale > 0 else (0.0 if err == 0 else float("inf"))
    out = {"focal": rel(got[0][:, 0], ref[0][:, 0]), "l1": rel(got[0][:, 1], ref[0][:, 1]), "giou": rel(got[0][:, 2], ref[0][:, 2]),
           "grad_logits": rel(got[1], ref[1]), "grad_boxes": rel(got[2], ref[2])}
    return out


def held(name, ours, aten, extra=0.0):
    bad = []
    for k in ours:
        allowed = max(MULTIPLE * aten[k], MULTIPLE * EPS) + extra
        print(f"{name} {k}: fused {ours[k]:.3e}, ATen fp32 {aten[k]:.3e}, ratio {ours[k] / max(aten[k], 1e-30):.2f}, "
              f"allowed {allowed:.3e}")
        if not ours[k] <= allowed:
            bad.append((k, ours[k], aten[k], allowed))
    return bad


# ---- CPU ---------------------------------------------------------------------------------------------------------------
def test_entry_points_are_declared_bound_and_exported(hip_lib):
    from vnext_amd import _lib
    header = open(os.path.join(ROOT, "include", "vnext_hip.h")).read()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, header) and name in _lib.SIGNATURES and hasattr(hip_lib, name)
        assert re.search(r" T %s$" % name, out, re.M), name
    assert _lib.ABI_VERSION == 17 and hip_lib.vnx_abi_version() == 17       # additive: the version stays
    assert "#define VNX_ABI_VERSION 17" in header
    assert "#define VNX_SET_LOSS_PIECE %d" % _lib.SET_LOSS_PIECE in header
    assert "#define VNX_SET_LOSS_MAX_ROWS %d" % _lib.SET_LOSS_MAX_ROWS in header


def test_the_switch_and_its_setter():
    import vnext_amd.models  # noqa: F401
    from vnext_amd import train
    from vnext_amd.models.criterion import SetCriterion
    from vnext_amd.models.idol_criterion import IDOLCriterion
    from vnext_amd.registry import build_model, get_idol_cfg, get_seqformer_cfg
    with pytest.raises(ValueError, match="fused_set_loss"):
        train.enable_fused_set_loss(torch.nn.Linear(1, 1))
    tiny_s = {"MODEL.SeqFormer.ENC_LAYERS": 1, "MODEL.SeqFormer.DEC_LAYERS": 1, "MODEL.SeqFormer.DIM_FEEDFORWARD": 64}
    tiny_i = {"MODEL.IDOL.ENC_LAYERS": 1, "MODEL.IDOL.DEC_LAYERS": 1, "MODEL.IDOL.DIM_FEEDFORWARD": 64}
    for cfg, kind in ((get_seqformer_cfg(**{"MODEL.DEVICE": "cpu", **tiny_s}), SetCriterion),
                      (get_idol_cfg(**{"MODEL.DEVICE": "cpu", **tiny_i}), IDOLCriterion)):
        model = build_model(cfg)
        assert isinstance(model.criterion, kind) and model.criterion.fused_set_loss is False       # off on a fresh model
        train.enable_fused_set_loss(model)
        assert model.criterion.fused_set_loss is True and model.criterion.fused_mask_loss is False
        train.enable_fused_set_loss(model, False)
        assert model.criterion.fused_set_loss is False


def test_cpu_tensors_are_rejected():
    case = CASES["tiny_one_clip_without_targets"]()
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        fused(*case[:8])


def test_with_the_switch_on_the_criteria_raise_on_cpu_tensors():
    """No fallback behind the switch: the same inputs that test_criterion.py / test_idol_criterion.py feed on the CPU."""
    from vnext_amd.models.criterion import HungarianMatcher, SetCriterion
    from vnext_amd.models.idol_criterion import IDOLCriterion, OTAMatcher
    (K, nf), targets, ind, logits, boxes, masks, _ = _fixture_seqformer_inputs()
    crit = SetCriterion(K, HungarianMatcher(), {}, ["labels", "boxes", "masks"], mask_out_stride=4, num_frames=nf)
    off = crit.forward_all_layers(logits, boxes, masks, targets, ind)          # off: the ATen path runs on the CPU
    assert "class_error" in off
    crit.fused_set_loss = True
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        crit.forward_all_layers(logits, boxes, masks, targets, ind)
    K, det, iind, il, ib, im, _ = _fixture_idol_inputs()
    icrit = IDOLCriterion(K, OTAMatcher(), {}, ["labels", "boxes", "masks", "reid"], mask_out_stride=4)
    qd = {"contrast": 0, "aux": 0, "count": 0}
    icrit.forward_all_layers(il, ib, im, det, iind, qd)
    icrit.fused_set_loss = True
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        icrit.forward_all_layers(il, ib, im, det, iind, qd)


def test_the_cases_are_finite_and_free_of_ties():
    """`compose` in float64 is finite on every case (asserted where the reference is made), and no case sits on a tie:
    the top two logits of every row more than 1e-3 apart, no coordinate of a matched prediction equal to its target's"""
    from vnext_amd.models.criterion import box_cxcywh_to_xyxy
    for name in CASES:
        (logits, boxes, lay, clip, qry, tgt, labels, tgt_boxes, _), _, ref = case_and_reference(name)
        if logits.shape[-1] > 1:
            top = logits.topk(2, -1).values
            assert float((top[..., 0] - top[..., 1]).min()) > 1e-3, name
        if len(lay):
            a = box_cxcywh_to_xyxy(boxes.transpose(2, 3)[lay, clip, qry])
            b = box_cxcywh_to_xyxy(tgt_boxes[tgt])
            assert float((a - b).abs().min()) > 0 and float((boxes.transpose(2, 3)[lay, clip, qry] - tgt_boxes[tgt]).abs().min()) > 0, name
        assert ref[0].shape == (logits.shape[0], 4)


# ---- GPU: the op against float64 -----------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_op_against_float64(name):
    case, w, ref = case_and_reference(name)
    aten_out = run(compose, case, w, device=DEV)
    got = run(fused, case, w, device=DEV)
    assert got[0].shape == ref[0].shape and got[0].dtype == torch.float32
    assert got[1].shape == case[0].shape and got[2].shape == case[1].shape
    aten, ours = errors(aten_out, ref), errors(got, ref)
    bad = held(name, ours, aten)
    print(f"{name} hits: fused {got[0][:, 3].tolist()}, float64 {ref[0][:, 3].tolist()}")
    assert torch.equal(got[0][:, 3].cpu().double(), ref[0][:, 3])
    assert not bad, bad
    # grad_boxes is exactly zero at every unmatched (l, n, t, q)
    logits, boxes, lay, clip, qry = case[:5]
    matched = torch.zeros(boxes.shape[:4], dtype=torch.bool)
    matched.transpose(2, 3)[lay, clip, qry] = True
    assert not bool(got[2].cpu()[~matched].any())
    if name == "no_pairs":
        assert not bool(got[2].any()) and not bool(got[0][:, 1:].any()) and bool((got[0][:, 0] > 0).all())
    if name == "disjoint_boxes":                       # the gate is closed on every pair: the loss is above 1
        assert float(ref[0][:, 2].min()) > len(lay) // boxes.shape[0] * boxes.shape[2]      # pairs of a layer x frames


@pytest.mark.gpu
def test_a_pair_of_minus_one_contributes_nothing():
    """The device Hungarian matcher answers -1 for a clip whose cost is not finite: the list with such pairs gives
    bit for bit what the list without them gives."""
    case, w, _ = case_and_reference("model_shape")
    logits, boxes, lay, clip, qry, tgt, labels, tgt_boxes, kw = case
    want = run(fused, case, w, device=DEV)
    at = [0, 5, len(lay)]                               # at the head, inside, at the tail
    ins = lambda v, vals: torch.cat([torch.cat([v[a:b], torch.tensor([x])]) for a, b, x in      # noqa: E731
                                     zip([0] + at[:-1], at, vals)] + [v[at[-1]:]])
    with_bad = (logits, boxes, ins(lay, [0, 1, 5]), ins(clip, [0, 1, 1]), ins(qry, [-1, 7, -1]), ins(tgt, [2, -1, -1]),
                labels, tgt_boxes, kw)
    assert len(with_bad[2]) == len(lay) + 3
    got = run(fused, with_bad, w, device=DEV)
    for a, b in zip(got, want):
        assert torch.equal(a, b)


@pytest.mark.gpu
def test_sixteen_bit_inputs_are_read_as_fp32_and_the_gradients_keep_their_type():
    """bf16 logits and boxes against float64 of the same bf16 values.  The sums are fp32: the fp32 bound.  The gradients
    come back in bf16: the fp32 bound plus bf16's unit roundoff 2^-8 of the largest magnitude (8 significant bits -- 7
    stored and the implicit one -- so neighbours are 2^-7 apart and rounding to nearest moves a value by half of that)."""
    case, w, _ = case_and_reference("idol_ragged_7_0_19")
    low = (case[0].bfloat16().float(), case[1].bfloat16().float()) + case[2:]
    ref = run(compose, low, w.double(), dtype=torch.float64)
    aten = errors(run(compose, low, w, device=DEV), ref)
    logits, boxes, lay, clip, qry, tgt, labels, tgt_boxes, kw = case
    x = logits.to(DEV, torch.bfloat16).requires_grad_(True)
    b = boxes.to(DEV, torch.bfloat16).requires_grad_(True)
    out = fused(x, b, lay.to(DEV), clip.to(DEV), qry.to(DEV), tgt.to(DEV), labels.to(DEV), tgt_boxes.to(DEV))
    (out[:, :3] * w.to(DEV)).sum().backward()
    assert out.dtype == torch.float32 and x.grad.dtype == torch.bfloat16 and b.grad.dtype == torch.bfloat16
    ours = errors((out.detach(), x.grad, b.grad), ref)
    bad = held("bf16", {k: v for k, v in ours.items() if not k.startswith("grad")}, aten)
    bad += held("bf16", {k: v for k, v in ours.items() if k.startswith("grad")}, aten, extra=2.0 ** -8)
    assert torch.equal(out[:, 3].cpu().double(), ref[0][:, 3])
    assert not bad, bad


@pytest.mark.gpu
def test_two_calls_are_bit_identical():
    case, w, _ = case_and_reference("model_shape")
    a = run(fused, case, w, device=DEV)
    b = run(fused, case, w, device=DEV)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


# ---- GPU: against the reference's numbers ---------------------------------------------------------------------------------
def _held_to_the_fixture(kind, want, off, on):
    """test_mask_loss.py's rule for the same comparison (its `_held_to_the_fixture`): with the switch on, an entry may be
    four times as far from the fixture's float64 number as the switch-off path on the device is, floor 4 * 2^-23; here
    for EVERY entry of the dict.  (test_criterion.py's rtol 1e-10 is for the float64 run on the CPU.)"""
    assert set(on) == set(off) and set(want) <= set(on)
    bad = []
    for k in sorted(want):
        scale = abs(want[k]) or 1.0
        e_off = abs(float(off[k]) - want[k]) / scale
        e_on = abs(float(on[k]) - want[k]) / scale
        allowed = max(4 * e_off, 4 * EPS)
        print(f"{kind} {k}: fixture {want[k]:.9g}, switch on {e_on:.3e}, switch off {e_off:.3e}, allowed {allowed:.3e}")
        if not e_on <= allowed:
            bad.append((kind, k, e_on, e_off))
    assert not bad, bad


@pytest.mark.gpu
@pytest.mark.parametrize("mask_loss_too", [False, True])
def test_seqformer_criterion_reproduces_the_reference_losses(mask_loss_too):
    from vnext_amd.models.criterion import HungarianMatcher, SetCriterion
    (K, nf), targets, ind, logits, boxes, masks, want = _fixture_seqformer_inputs()
    targets = [{k: v.to(DEV) for k, v in t.items()} for t in targets]
    crit = SetCriterion(K, HungarianMatcher(), {}, ["labels", "boxes", "masks"], mask_out_stride=4, num_frames=nf)
    args = (logits.to(DEV), boxes.to(DEV), masks.to(DEV), targets, ind)
    off = crit.forward_all_layers(*args)
    crit.fused_set_loss, crit.fused_mask_loss = True, mask_loss_too
    on = crit.forward_all_layers(*args)
    assert set(on) == set(want)
    _held_to_the_fixture("seqformer", want, off, on)


@pytest.mark.gpu
@pytest.mark.parametrize("mask_loss_too", [False, True])
def test_idol_criterion_reproduces_the_reference_losses(mask_loss_too):
    from vnext_amd.models.idol_criterion import IDOLCriterion, OTAMatcher
    K, det, ind, logits, boxes, masks, want = _fixture_idol_inputs()
    det = [{k: v.to(DEV) for k, v in t.items()} for t in det]
    crit = IDOLCriterion(K, OTAMatcher(), {}, ["labels", "boxes", "masks", "reid"], mask_out_stride=4)
    args = (logits.to(DEV), boxes.to(DEV), masks.to(DEV), det, ind, {"contrast": 0, "aux": 0, "count": 0})
    want = {k: v for k, v in want.items() if not k.startswith("loss_reid")}      # the reid terms are not what this test looks at
    off = crit.forward_all_layers(*args)
    crit.fused_set_loss, crit.fused_mask_loss = True, mask_loss_too
    on = crit.forward_all_layers(*args)
    _held_to_the_fixture("idol", want, off, on)


# ---- GPU: the models --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def seqformer():
    import vnext_amd.models  # noqa: F401
    from vnext_amd import train
    from vnext_amd.registry import build_model, get_seqformer_cfg
    torch.manual_seed(0)
    # dropout off: the fused dropout sites draw a new mask per call whatever the seed, and steps are compared here
    model = build_model(get_seqformer_cfg(**{"MODEL.DEVICE": DEV, "MODEL.SeqFormer.DROPOUT": 0.0})).train()
    clips = train.synthetic_clips(1, 5, 360, 640, DEV, seed=100, num_instances=4)
    return model, clips


@pytest.mark.gpu
def test_losses_after_the_trunk_do_not_touch_the_host_with_all_three_switches(seqformer):
    """test_device_matching.py's scenario with the fused mask losses and the fused class and box losses on as well:
    under torch's sync-debug mode a device-to-host copy or a blocking pageable upload raises."""
    from vnext_amd import train
    model, clips = seqformer
    targets = model.prepare_targets(clips)
    torch.manual_seed(1)
    x, srcs, hs, memory, logits, boxes, refs = model._run(clips, want_refs=True)
    trunk = (hs, logits, boxes, refs, model._mask_features(srcs, memory))
    train.enable_device_matching(model)
    train.enable_fused_mask_loss(model)
    train.enable_fused_set_loss(model)
    try:
        model._losses_after_trunk(targets, *trunk)           # warm-up: fills the caches of constants
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            losses = model._losses_after_trunk(targets, *trunk)
        finally:
            torch.cuda.set_sync_debug_mode("default")
    finally:
        model.device_matching = False
        model.criterion.fused_mask_loss = False
        model.criterion.fused_set_loss = False
    assert all(v.is_cuda for v in losses.values())
    assert all(bool(torch.isfinite(v)) for v in losses.values())
    assert float(losses["loss_ce"]) > 0 and float(losses["loss_bbox"]) > 0 and float(losses["loss_giou"]) > 0
    assert 0 <= float(losses["class_error"]) <= 100


def _step(model, clips):
    """one seeded forward + backward -> (loss dict, every parameter's gradient)"""
    model.zero_grad(set_to_none=True)
    torch.manual_seed(1)
    random.seed(1)                  # IDOL: select_pos_neg_masks draws its negatives from the host generator
    losses = model(clips)
    sum(losses.values()).backward()
    grads = {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}
    model.zero_grad(set_to_none=True)
    return {k: v.detach().clone() for k, v in losses.items()}, grads


def _steps_agree(model, clips):
    """Switch off twice, on once; the loss dict and EVERY parameter gradient.

    There is no float64 run of a whole model on the device, so ATen's measured error here is what the switch-off path
    shows of itself: the difference between two switch-off steps.  The rule is the one of test_device_matching.py /
    test_mask_loss.py: switch-on may differ from the first switch-off step by ten times that, floor 1e-5 (their floor for
    a path that reassociates fp32 sums rather than reorder atomics).  A loss entry is taken in units of its own value.
    A gradient is taken in units of the largest entry of the gradient of largest norm, and the switch-off difference is
    the LARGEST over all gradients in that unit: every gradient is a linear image of the same grad_logits / grad_boxes /
    grad_masks, and the switch-off path's run-to-run differences are sporadic events (which samples of a deformable
    attention straddle a pixel edge, the order of a few atomics), not a level per tensor.  Measured on the MI355X
    (SeqFormer, 462 gradients): of two switch-off steps 31 gradients came out bit-identical while others differed by up to
    1.6e-4 of the unit (1.2e-3 in another run); the largest switch-on difference was 1.0e-4 (3.1e-4 in that other run) and
    the largest difference after the criterion's inputs were moved by one fp32 ulp 1.0e-4 as well -- the same noise.  A first form of this test that
    took the switch-off difference per tensor failed on one gradient of 462 (encoder.layers.2.linear1.bias: 2.26e-5
    against ten times 1.99e-6) and held on the next run of the same code, where that tensor's difference was below
    1.0e-5: a single sample of a sporadic difference is not a measure of it."""
    model.criterion.fused_set_loss = False
    loss_1, grad_1 = _step(model, clips)
    loss_2, grad_2 = _step(model, clips)
    model.criterion.fused_set_loss = True
    try:
        loss_f, grad_f = _step(model, clips)
    finally:
        model.criterion.fused_set_loss = False
    assert set(loss_f) == set(loss_1) and set(grad_f) == set(grad_1) and len(grad_f) >= 4
    biggest = max(grad_1, key=lambda k: float(grad_1[k].norm()))
    unit = float(grad_1[biggest].abs().max())
    print(f"gradient of largest norm: {biggest}, norm {float(grad_1[biggest].norm()):.4e}, largest entry {unit:.4e}")
    failures = []
    for k in loss_1:
        scale = float(loss_1[k].abs()) or 1.0
        off_off, on_off = float((loss_1[k] - loss_2[k]).abs()) / scale, float((loss_f[k] - loss_1[k]).abs()) / scale
        allowed = max(10 * off_off, 1e-5)
        print(f"loss {k}: on-off {on_off:.3e}, off-off {off_off:.3e}, allowed {allowed:.3e}")
        if not on_off <= allowed:
            failures.append(("loss", k, on_off, allowed))
    off_off = {k: float((grad_1[k] - grad_2[k]).abs().max()) / unit for k in grad_1}
    on_off = {k: float((grad_f[k] - grad_1[k]).abs().max()) / unit for k in grad_1}
    noisiest, worst = max(off_off, key=off_off.get), max(on_off, key=on_off.get)
    allowed = max(10 * off_off[noisiest], 1e-5)
    print(f"{len(grad_1)} gradients; largest off-off {off_off[noisiest]:.3e} ({noisiest}), largest on-off {on_off[worst]:.3e} "
          f"({worst}), allowed {allowed:.3e}; {biggest}: on-off {on_off[biggest]:.3e}, off-off {off_off[biggest]:.3e}")
    for k in grad_1:
        if not on_off[k] <= allowed:
            print(f"grad {k}: on-off {on_off[k]:.3e}, off-off {off_off[k]:.3e}, allowed {allowed:.3e}")
            failures.append(("grad", k, on_off[k], allowed))
    assert not failures, failures


@pytest.mark.gpu
def test_seqformer_step_is_the_same_with_the_fused_set_loss(seqformer):
    model, clips = seqformer
    _steps_agree(model, clips)


@pytest.mark.gpu
def test_idol_step_is_the_same_with_the_fused_set_loss():
    import vnext_amd.models  # noqa: F401
    from vnext_amd import train
    from vnext_amd.registry import build_model, get_idol_cfg
    torch.manual_seed(11)
    tiny = {"MODEL.IDOL.ENC_LAYERS": 1, "MODEL.IDOL.DEC_LAYERS": 2, "MODEL.IDOL.NUM_OBJECT_QUERIES": 110,
            "MODEL.IDOL.DIM_FEEDFORWARD": 64, "MODEL.IDOL.DROPOUT": 0.0}
    model = build_model(get_idol_cfg(**{"MODEL.DEVICE": DEV, **tiny})).train()
    for m in model.modules():
        if isinstance(m, torch.nn.MultiheadAttention):
            m.dropout = 0.0
    pairs = train.synthetic_clips(1, 2, 96, 160, DEV, seed=6, num_instances=3)
    _steps_agree(model, pairs)
