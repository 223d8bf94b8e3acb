"""The fused reid losses (vnext_amd/csrc/reid_loss.hip, vnext_amd/ops/reid_loss.py, `idol_criterion.pack_reid_selections` /
`reid_terms_fused`, the criterion's `fused_reid_loss` switch, train.enable_fused_reid_loss): IDOL's contrastive loss and
auxiliary cosine loss of every instance of every image from one op.

The yardstick of the GPU tests is `heads.loss_reid`'s expression (`yardstick` below, the restatement of
tests/test_idol_criterion.py::_loss_reid_torch kept per instance) in float64 on the CPU from the same fp32 inputs, under
upstream gradients that differ per instance and per column of the op's [J, 2] result.  The bound is the project's rule
(test_mask_loss.py, test_set_loss.py), not a constant: on every case today's fp32 path runs on the device -- the lines of
`heads.loss_reid` on its own kernels, once per image, kept per instance so that each instance's two terms can carry their
own upstream weight (`unfused_terms`) -- its error against float64 is measured, and the fused op is
allowed MULTIPLE = 4 times that error, with a floor of 4 * 2^-23 where the ATen path happens to be exact.  Units: absolute
error over the largest magnitude of that output in the yardstick; separately for the per-image contrast sums, the per-image
aux sums, grad_ref and grad_key.  Every test prints its figures before it asserts.

Measured on an MI355X (worst op error over the seven cases; the unfused fp32 path on the same case): contrast sums 5.1e-8
(6.4e-8), aux sums 5.9e-8 (6.0e-8) -- all under the floor of 4.8e-7 --, grad_key 4.7e-7 (1.2e-6), grad_ref 3.7e-7 (9.8e-7);
where the unfused path is at least 2^-24 off the ratios are 0.11 -- 1.00.  DESIGN section 15 has the table."""
import functools
import os
import random
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import GOLDEN_DIR, ROOT

DEV = "cuda:0"
EPS = 2.0 ** -23
MULTIPLE = 4
NAMES = ("vnx_reid_loss_forward", "vnx_reid_loss_backward")


# ---- the yardstick: heads.loss_reid's expression per instance, any dtype ----------------------------------------------------
def yardstick(ref, key, pos, neg, aux):
    """ref [R, C], key [I, C], pos / neg / aux [R, I] bool -> (contrast [I], aux [I])"""
    dot = ref @ key.t()
    cos = F.normalize(ref, dim=1) @ F.normalize(key, dim=1).t()
    lse_neg = torch.logsumexp(dot.masked_fill(~neg, float("-inf")), dim=0)
    lse_pos = torch.logsumexp((-dot).masked_fill(~pos, float("-inf")), dim=0)
    contrast = F.softplus((lse_neg + lse_pos).clamp_min(torch.finfo(dot.dtype).min))
    a = (((cos - pos.to(cos.dtype)) ** 2) * aux).sum(0) / aux.sum(0).clamp_min(1)
    return contrast, a


def _masks(flags):
    """uint8 [n, R] -> pos, neg, aux [R, n] bool"""
    f = flags.t()
    return (f & 1).bool(), (f & 2).bool(), (f & 4).bool()


def _in_range(case, j):
    key, ref, img, kq, flags = case
    return 0 <= int(img[j]) < key.shape[0] and 0 <= int(kq[j]) < key.shape[1]


def run_yardstick(case, w, dtype=torch.float64):
    """-> (out [J, 2], grad_key, grad_ref) of sum(out * w), on the CPU in `dtype`"""
    key, ref, img, kq, flags = case
    k = key.detach().to(dtype).requires_grad_(True)
    r = ref.detach().to(dtype).requires_grad_(True)
    out = torch.zeros(len(img), 2, dtype=dtype)
    rows = []
    for j in range(len(img)):
        if not _in_range(case, j):
            rows.append(out[j] * 1)
            continue
        b = int(img[j])
        c, a = yardstick(r[b], k[b, kq[j].long()][None], *_masks(flags[j:j + 1]))
        rows.append(torch.stack([c[0], a[0]]))
    out = torch.stack(rows) if rows else out
    loss = (out * w.to(dtype)).sum() + 0 * (k.sum() + r.sum())
    loss.backward()
    return out.detach(), k.grad.detach(), r.grad.detach()


def unfused_terms(ref, key, pos, neg, aux):
    """the lines of vnext_amd.heads.loss_reid on its own kernels (`similarity`), without its final sums over the instances"""
    from vnext_amd.heads import similarity
    dot = similarity(ref, key)
    cos = similarity(ref, key, normalize=True)
    lse_neg = torch.logsumexp(dot.masked_fill(~neg, float("-inf")), dim=0)
    lse_pos = torch.logsumexp((-dot).masked_fill(~pos, float("-inf")), dim=0)
    contrast = F.softplus((lse_neg + lse_pos).clamp_min(torch.finfo(dot.dtype).min))
    a = (((cos - pos.to(cos.dtype)) ** 2) * aux).sum(0) / aux.sum(0).clamp_min(1)
    return contrast, a


def run_unfused(case, w):
    """today's fp32 path on the device, one call per image as `reid_terms` makes it.  An image's lone instance is handed
    over twice and the copy weighted 0: today's similarity backward does not take a single key row."""
    key, ref, img, kq, flags = case
    k = key.detach().to(DEV).requires_grad_(True)
    r = ref.detach().to(DEV).requires_grad_(True)
    out = [None] * len(img)
    for b in range(key.shape[0]):
        js = [j for j in range(len(img)) if int(img[j]) == b]
        if not js:
            continue
        rows = js * 2 if len(js) == 1 else js
        pos, neg, aux = (m.to(DEV) for m in _masks(flags[rows]))
        c, a = unfused_terms(r[b], k[b, kq[rows].long().to(DEV)], pos, neg, aux)
        for n, j in enumerate(js):
            out[j] = torch.stack([c[n], a[n]])
    out = torch.stack(out)
    ((out * w.to(DEV)).sum() + 0 * (k.sum() + r.sum())).backward()
    return out.detach(), k.grad.detach(), r.grad.detach()


def run_fused(case, w, device=DEV, dtype=None):
    from vnext_amd.ops.reid_loss import reid_contrastive_losses
    key, ref, img, kq, flags = case
    cast = (lambda v: v.detach().to(device, dtype)) if dtype is not None else (lambda v: v.detach().to(device))
    k, r = cast(key).requires_grad_(True), cast(ref).requires_grad_(True)
    out = reid_contrastive_losses(k, r, img.to(device), kq.to(device), flags.to(device))
    ((out * w.to(device)).sum() + 0 * (k.sum() + r.sum())).backward()
    return out.detach(), k.grad.detach(), r.grad.detach()


# ---- cases -----------------------------------------------------------------------------------------------------------
def synthetic(B, Q, R, C, counts, seed=0, scale=1.0, special=True, share=True):
    """key [B, Q, C], ref [B, R, C] standard normal times `scale`; counts[b] instances in image b.  Sets with realistic
    sizes (a few positives, most other rows negative, aux = positives + about three times as many negatives).  With
    `special`, an image of five or more instances has: P empty, N empty, A empty, a row in both P and N, every row in all
    three.  With `share`, the second instance of an image shares the first one's key query."""
    g = torch.Generator().manual_seed(seed)
    key, ref = torch.randn(B, Q, C, generator=g) * scale, torch.randn(B, R, C, generator=g) * scale
    img, kq, flags = [], [], []
    for b, n in enumerate(counts):
        q = torch.randperm(Q, generator=g)[:n] if n <= Q else torch.randint(0, Q, (n,), generator=g)
        if share and n >= 2:
            q[1] = q[0]
        for c in range(n):
            order = torch.randperm(R, generator=g)
            n_pos = max(1, min(5, R // 8)) if R > 1 else 1
            pos = torch.zeros(R, dtype=torch.bool)
            pos[order[:n_pos]] = True
            neg = ~pos & (torch.rand(R, generator=g) < 0.9)
            if R > 1 and not neg.any():
                neg[order[-1]] = True
            aux = pos.clone()
            neg_rows = torch.nonzero(neg).flatten()
            aux[neg_rows[torch.randperm(len(neg_rows), generator=g)[:3 * n_pos]]] = True
            if special and n >= 5:
                if c == 0:
                    aux, pos = aux & ~pos, torch.zeros_like(pos)
                elif c == 1:
                    aux, neg = aux & ~neg, torch.zeros_like(neg)
                elif c == 2:
                    aux = torch.zeros_like(aux)
                elif c == 3:
                    neg = neg.clone()
                    neg[order[0]] = True                      # order[0] is a positive: that row is in P and N
                elif c == 4:
                    pos, neg, aux = (torch.ones(R, dtype=torch.bool) for _ in range(3))
            img.append(b)
            kq.append(int(q[c]))
            flags.append(pos.to(torch.uint8) | (neg.to(torch.uint8) << 1) | (aux.to(torch.uint8) << 2))
    return (key, ref, torch.tensor(img, dtype=torch.int32), torch.tensor(kq, dtype=torch.int32),
            torch.stack(flags) if flags else torch.zeros(0, R, dtype=torch.uint8))


CASES = {
    # B = 3 with 1, 0 and 5 instances (the empty image in the middle), a shared key query, the five special instances,
    # Q != R; R and C at every size where the kernels take another path: one row; one short of / one past a wave's 64
    # rows; the model's 300; C = 256 (one 16-byte pass), 64, 37 and 10 (the one-channel-per-lane form)
    "R1_C10_Q7": lambda: synthetic(3, 7, 1, 10, (1, 0, 5), seed=1),
    "R63_C37_Q20": lambda: synthetic(3, 20, 63, 37, (1, 0, 5), seed=2),
    "R65_C64_Q300": lambda: synthetic(3, 300, 65, 64, (1, 0, 5), seed=3),
    "R300_C256_Q110": lambda: synthetic(3, 110, 300, 256, (1, 0, 5), seed=4),
    # more channels than one pass of a wave covers: 16-byte form (256 per pass) and one-channel form (64 per pass)
    "R20_C260_Q9": lambda: synthetic(2, 9, 20, 260, (2, 5), seed=5),
    "R20_C70_Q9": lambda: synthetic(2, 9, 20, 70, (5, 2), seed=6),
    # the bench's IDOL leg with large dots: |dot| above 100 (checked in the CPU test below)
    "large_magnitude": lambda: synthetic(1, 300, 300, 256, (8,), seed=7, scale=1.5, special=False),
}
SHARED = "R300_C256_Q110"


@functools.lru_cache(maxsize=None)
def case_and_reference(name):
    """(case, upstream weights [J, 2], the float64 result on the CPU): computed once per case, shared, never modified"""
    case = CASES[name]()
    g = torch.Generator().manual_seed(11)
    w = torch.rand(len(case[2]), 2, generator=g) + 0.5
    ref = run_yardstick(case, w)
    assert all(bool(torch.isfinite(t).all()) for t in ref), name
    return case, w, ref


def per_image(out, img, B):
    """[J, 2] -> [B, 2] sums over each image's instances"""
    return torch.zeros(B, 2, dtype=out.dtype).index_add_(0, img.long().clamp(0, B - 1), out.cpu())


def errors(got, ref, img, B):
    def rel(a, b):
        err = float((a.double().cpu() - b).abs().max()) if b.numel() else 0.0
        scale = float(b.abs().max()) if b.numel() else 0.0
        return err / scale if scale > 0 else (0.0 if err == 0 else float("inf"))
    s_got, s_ref = per_image(got[0].double(), img, B), per_image(ref[0], img, B)
    return {"contrast": rel(s_got[:, 0], s_ref[:, 0]), "aux": rel(s_got[:, 1], s_ref[:, 1]),
            "grad_key": rel(got[1], ref[1]), "grad_ref": rel(got[2], ref[2])}


def held(name, ours, unfused, extra=0.0):
    bad = []
    for k in ours:
        allowed = max(MULTIPLE * unfused[k], MULTIPLE * EPS) + extra
        print(f"{name} {k}: fused {ours[k]:.3e}, unfused fp32 {unfused[k]:.3e}, ratio {ours[k] / max(unfused[k], 1e-30):.2f}, "
              f"allowed {allowed:.3e}")
        if not ours[k] <= allowed:
            bad.append((k, ours[k], unfused[k], allowed))
    return bad


# ---- the fixtures -------------------------------------------------------------------------------------------------------
def _fixture_reid_loss():
    g = dict(np.load(os.path.join(GOLDEN_DIR, "reid_loss.npz")))
    ref, key = torch.from_numpy(g["ref"]).float(), torch.from_numpy(g["key"]).float()      # [R, C], [I, C]
    I = key.shape[0]
    flags = (torch.from_numpy(g["pos"]).to(torch.uint8) | (torch.from_numpy(g["neg"]).to(torch.uint8) << 1) |
             (torch.from_numpy(g["aux"]).to(torch.uint8) << 2)).t().contiguous()
    case = (key[None], ref[None], torch.zeros(I, dtype=torch.int32), torch.arange(I, dtype=torch.int32), flags)
    return g, case


def _fixture_idol():
    """embeddings, matched and the selection as test_idol_criterion.py builds them"""
    from vnext_amd.models.idol_criterion import select_pos_neg_masks
    g = dict(np.load(os.path.join(GOLDEN_DIR, "criterion_idol.npz")))
    bz, Q, K, H, W, layers, C = (int(v) for v in g["cfg"])
    ref_t = [{k: torch.from_numpy(g[f"ref{i}.{k}"]) for k in ("labels", "boxes", "masks", "inst_id", "valid")} for i in range(bz)]
    head = torch.from_numpy(g["head_w"]).float()
    key = torch.from_numpy(g["hs_key"]).float() @ head.t()
    refe = torch.from_numpy(g["hs_ref"]).float() @ head.t()
    matched = [torch.from_numpy(g[f"matched{i}"]) for i in range(bz)]
    random.seed(5)
    sel = select_pos_neg_masks(torch.from_numpy(g["ref_boxes"]), torch.from_numpy(g["ref_logits"]).sigmoid(), ref_t)
    return g, key, refe, matched, sel


def _yardstick_terms(key, refe, matched, sel):
    from vnext_amd.models.idol_criterion import reid_terms
    fn = lambda *a: tuple(v.sum() for v in yardstick(*a))      # noqa: E731
    return reid_terms(key.double(), refe.double(), matched, sel, fn)


# ---- CPU ---------------------------------------------------------------------------------------------------------------
def test_entry_points_are_declared_bound_and_exported(hip_lib):
    from vnext_amd import _lib
    header = open(os.path.join(ROOT, "include", "vnext_hip.h")).read()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, header) and name in _lib.SIGNATURES and hasattr(hip_lib, name)
        assert re.search(r" T %s$" % name, out, re.M), name
    assert _lib.ABI_VERSION == 17 and hip_lib.vnx_abi_version() == 17       # additive: the version stays
    assert "#define VNX_REID_LOSS_MAX_ROWS %d" % _lib.REID_LOSS_MAX_ROWS in header


def test_the_switch_and_its_setter():
    import vnext_amd.models  # noqa: F401
    from vnext_amd import train
    from vnext_amd.models.idol_criterion import IDOLCriterion
    from vnext_amd.registry import build_model, get_idol_cfg, get_seqformer_cfg
    tiny_s = {"MODEL.SeqFormer.ENC_LAYERS": 1, "MODEL.SeqFormer.DEC_LAYERS": 1, "MODEL.SeqFormer.DIM_FEEDFORWARD": 64}
    tiny_i = {"MODEL.IDOL.ENC_LAYERS": 1, "MODEL.IDOL.DEC_LAYERS": 1, "MODEL.IDOL.DIM_FEEDFORWARD": 64}
    with pytest.raises(ValueError, match="fused_reid_loss"):
        train.enable_fused_reid_loss(build_model(get_seqformer_cfg(**{"MODEL.DEVICE": "cpu", **tiny_s})))
    with pytest.raises(ValueError, match="fused_reid_loss"):
        train.enable_fused_reid_loss(torch.nn.Linear(1, 1))
    model = build_model(get_idol_cfg(**{"MODEL.DEVICE": "cpu", **tiny_i}))
    assert isinstance(model.criterion, IDOLCriterion) and model.criterion.fused_reid_loss is False      # off on a fresh model
    train.enable_fused_reid_loss(model)
    assert model.criterion.fused_reid_loss is True
    assert model.criterion.fused_set_loss is False and model.criterion.fused_mask_loss is False and model.device_matching is False
    train.enable_fused_reid_loss(model, False)
    assert model.criterion.fused_reid_loss is False


def test_cpu_tensors_are_rejected():
    case = CASES["R1_C10_Q7"]()
    from vnext_amd.ops.reid_loss import reid_contrastive_losses
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        reid_contrastive_losses(*case)


def test_with_the_switch_on_cpu_tensors_take_todays_path(monkeypatch):
    """`IDOL.losses` on CPU tensors calls `reid_terms(..., loss_reid)` through the module-level name `loss_reid`, switch on
    or off: the stand-in that test_idol_model.py patches in is what runs, and the losses are the same."""
    import vnext_amd.models.idol as idol_mod
    from oracle.heads_torch_fallback import dynamic_mask_head_torch
    from oracle.msda_torch_fallback import msda_grid_sample
    from vnext_amd import train
    from vnext_amd.ops.modules import ms_deform_attn as mod
    from vnext_amd.registry import build_model, get_idol_cfg
    calls = []

    class Fn:
        @staticmethod
        def apply(value, shapes, lsi, loc, attn, step):
            return msda_grid_sample(value, shapes, loc, attn)

    def stand_in(ref, key, pos, neg, aux):
        calls.append(tuple(key.shape))
        c, a = yardstick(ref, key, pos, neg, aux)
        return c.sum(), a.sum()

    def fused_must_not_run(*a, **k):
        raise AssertionError("the fused path was taken on CPU tensors")
    monkeypatch.setattr(mod, "MSDeformAttnFunction", Fn)
    monkeypatch.setattr(idol_mod, "dynamic_mask_head", dynamic_mask_head_torch)
    monkeypatch.setattr(idol_mod, "loss_reid", stand_in)
    monkeypatch.setattr(idol_mod, "reid_terms_fused", fused_must_not_run)
    tiny = {"MODEL.IDOL.ENC_LAYERS": 1, "MODEL.IDOL.DEC_LAYERS": 1, "MODEL.IDOL.NUM_OBJECT_QUERIES": 110,
            "MODEL.IDOL.DIM_FEEDFORWARD": 64, "MODEL.IDOL.DROPOUT": 0.0}
    torch.manual_seed(2)
    model = build_model(get_idol_cfg(**{"MODEL.DEVICE": "cpu", **tiny})).train()
    pairs = train.synthetic_clips(1, 2, 64, 96, "cpu", seed=9, num_instances=2)
    got = []
    for on in (False, True):
        train.enable_fused_reid_loss(model, on)
        torch.manual_seed(3)
        random.seed(3)
        n = len(calls)
        losses = model.losses(pairs)
        assert len(calls) > n                               # today's path ran, through the patched name
        got.append({k: float(v) for k, v in losses.items()})
    assert got[0] == got[1] and got[0]["loss_reid"] > 0


def test_pack_reid_selections_against_a_hand_written_expectation():
    from vnext_amd.models.idol_criterion import pack_reid_selections, reid_terms
    Q = 6
    col = lambda *rows: torch.tensor([[r in c for c in rows] for r in range(Q)], dtype=torch.bool)      # noqa: E731
    # image 0: targets 0 and 2 valid; image 1: none; image 2: target 1 valid
    sel = [(torch.tensor([0, 2]), col({1}, {4, 5}), col({0, 2, 3}, {0}), col({1, 2}, {0, 4, 5})),
           (torch.zeros(0, dtype=torch.int64), torch.zeros(Q, 0, dtype=torch.bool), torch.zeros(Q, 0, dtype=torch.bool),
            torch.zeros(Q, 0, dtype=torch.bool)),
           (torch.tensor([1]), col(set()), col({0, 1, 2, 3, 4, 5}), col({3}))]
    matched = [torch.tensor([5, 9, 3]), torch.tensor([7]), torch.tensor([2, 0])]
    img, kq, flags, count = pack_reid_selections(matched, sel)
    assert img.dtype == torch.int32 and kq.dtype == torch.int32 and flags.dtype == torch.uint8
    assert img.tolist() == [0, 0, 2] and kq.tolist() == [5, 3, 0] and count == 3
    assert flags.tolist() == [[2, 1 | 4, 2 | 4, 2, 0, 0],
                              [2 | 4, 0, 0, 0, 1 | 4, 1 | 4],
                              [2, 2, 2, 2 | 4, 2, 2]]
    # one staging buffer: the three arrays are views of the same storage, back to back
    assert img.untyped_storage().data_ptr() == kq.untyped_storage().data_ptr() == flags.untyped_storage().data_ptr()
    assert kq.data_ptr() == img.data_ptr() + 4 * 3 and flags.data_ptr() == img.data_ptr() + 8 * 3
    host = reid_terms(torch.zeros(3, 10, 4), torch.zeros(3, Q, 4), matched, sel, lambda *a: (0.0, 0.0))
    assert host["count"] == count
    # nothing valid anywhere: empty arrays, count 0
    img, kq, flags, count = pack_reid_selections(matched[1:2], sel[1:2])
    assert img.numel() == 0 and kq.numel() == 0 and flags.shape == (0, Q) and count == 0


def test_the_cases_are_in_the_ops_domain():
    """every float64 value and gradient is finite (asserted where the reference is made); the large-magnitude case has
    |dot| above 100; no row that carries a gradient has a norm below 1e-6"""
    for name in CASES:
        (key, ref, img, kq, flags), w, yard = case_and_reference(name)
        assert yard[0].shape == (len(img), 2), name
        assert float(key.norm(dim=-1).min()) > 1e-6 and float(ref.norm(dim=-1).min()) > 1e-6, name
    key, ref, img, kq, flags = case_and_reference("large_magnitude")[0]
    dots = torch.stack([ref[int(b)].double() @ key[int(b), int(q)].double() for b, q in zip(img, kq)])
    print("large_magnitude: max |dot| %.1f" % float(dots.abs().max()))
    assert float(dots.abs().max()) > 100
    # the special instances are what the case list says they are
    key, ref, img, kq, flags = case_and_reference(SHARED)[0]
    five = flags[img == 2]
    assert not (five[0] & 1).any() and not (five[1] & 2).any() and not (five[2] & 4).any()
    assert ((five[3] & 3) == 3).any() and (five[4] == 7).all()
    assert int(kq[img == 2][0]) == int(kq[img == 2][1]) and img.tolist() == [0, 2, 2, 2, 2, 2]
    for g, _ in (_fixture_reid_loss(),):
        assert not g["pos"][:, 3].any()                      # the fixture's instance 3 has no positives


def test_the_kernels_use_no_scratch_and_spill_nothing(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    src = os.path.join(ROOT, "vnext_amd", "csrc", "reid_loss.hip")
    p = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-munsafe-fp-atomics", "-I", os.path.dirname(src),
                        "-S", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-o", str(tmp_path / "reid_loss.s"),
                        src], capture_output=True, text=True, check=True)
    usage = {}
    for block in re.split(r"remark: Function Name: ", p.stderr)[1:]:
        name = block.split()[0]
        usage[name] = {k: int(v) for k, v in re.findall(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+) \[-Rpass", block)}
    kernels = {k: v for k, v in usage.items() if "reid_loss" in k}
    print(kernels)
    # the 16-byte and the one-channel form of each of the three kernels
    assert sorted(re.search(r"reid_loss_(\w+?)_kernel", k).group(1) for k in kernels) == ["bwd_key"] * 2 + ["bwd_ref"] * 2 + ["fwd"] * 2
    for name, u in kernels.items():
        assert u["ScratchSize"] == 0 and u["SGPRs Spill"] == 0 and u["VGPRs Spill"] == 0, (name, u)


# ---- GPU: the op against float64 -----------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_op_against_float64(name):
    case, w, ref = case_and_reference(name)
    key, rf, img, kq, flags = case
    B = key.shape[0]
    unfused = errors(run_unfused(case, w), ref, img, B)
    got = run_fused(case, w)
    assert got[0].shape == (len(img), 2) and got[0].dtype == torch.float32
    assert got[1].shape == key.shape and got[2].shape == rf.shape
    assert all(bool(torch.isfinite(t).all()) for t in got)
    bad = held(name, errors(got, ref, img, B), unfused)
    # exactly 0 where P or N is empty; grad_key exactly 0 at rows no instance points to
    empty = ((flags & 1).sum(1) == 0) | ((flags & 2).sum(1) == 0)
    assert not bool(got[0][:, 0].cpu()[empty].any())
    pointed = torch.zeros(key.shape[:2], dtype=torch.bool)
    pointed[img.long(), kq.long()] = True
    assert not bool(got[1].cpu()[~pointed].any())
    assert not bad, bad


@pytest.mark.gpu
def test_fixture_reid_loss_reproduces_the_reference_losses():
    g, case = _fixture_reid_loss()
    n = int(g["n_items"])
    w = torch.ones(len(case[2]), 2)
    yard = run_yardstick(case, w)
    # the yardstick is the reference's number
    np.testing.assert_allclose(float(yard[0][:, 0].sum()) / n, float(g["loss_reid"]), rtol=1e-6)
    np.testing.assert_allclose(float(yard[0][:, 1].sum()) / n, float(g["loss_reid_aux"]), rtol=1e-6)
    unfused = errors(run_unfused(case, w), yard, case[2], 1)
    got = run_fused(case, w)
    bad = held("reid_loss.npz", errors(got, yard, case[2], 1), unfused)
    want = {"contrast": float(g["loss_reid"]), "aux": float(g["loss_reid_aux"])}
    sums = got[0].double().sum(0).cpu() / n
    for col, k in enumerate(("contrast", "aux")):
        e = abs(float(sums[col]) - want[k]) / abs(want[k])
        e_yard = abs(float(yard[0][:, col].sum()) / n - want[k]) / abs(want[k])      # the reference's own fp32 cosine (see test_idol_criterion.py)
        allowed = max(MULTIPLE * unfused[k], MULTIPLE * EPS) + e_yard
        print(f"reid_loss.npz {k}: fixture {want[k]:.9g}, fused {e:.3e}, yardstick {e_yard:.3e}, allowed {allowed:.3e}")
        if not e <= allowed:
            bad.append((k, e, allowed))
    assert float(got[0][3, 0]) == 0.0                        # instance 3 has no positives
    assert not bad, bad


@pytest.mark.gpu
def test_fixture_criterion_idol_through_reid_terms_fused():
    from vnext_amd.heads import loss_reid
    from vnext_amd.models.idol_criterion import IDOLCriterion, OTAMatcher, reid_terms, reid_terms_fused
    g, key, refe, matched, sel = _fixture_idol()
    want = _yardstick_terms(key, refe, matched, sel)
    off = reid_terms(key.to(DEV), refe.to(DEV), matched, sel, loss_reid)
    on = reid_terms_fused(key.to(DEV), refe.to(DEV), matched, sel)
    assert on["count"] == off["count"] == want["count"] == int(g["n_items"])
    bad = []
    for k, fixture in (("contrast", "loss.loss_reid"), ("aux", "loss.loss_reid_aux")):
        scale = abs(float(want[k]))
        e_off, e_on = abs(float(off[k]) - float(want[k])) / scale, abs(float(on[k]) - float(want[k])) / scale
        allowed = max(MULTIPLE * e_off, MULTIPLE * EPS)
        print(f"criterion_idol.npz {k}: float64 {float(want[k]):.9g}, fused {e_on:.3e}, unfused {e_off:.3e}, allowed {allowed:.3e}")
        if not e_on <= allowed:
            bad.append((k, e_on, e_off))
        fx = float(g[fixture])
        f_off, f_on = abs(float(off[k]) / off["count"] - fx) / abs(fx), abs(float(on[k]) / on["count"] - fx) / abs(fx)
        allowed = max(MULTIPLE * f_off, MULTIPLE * EPS)
        print(f"criterion_idol.npz {fixture}: fixture {fx:.9g}, fused {f_on:.3e}, unfused {f_off:.3e}, allowed {allowed:.3e}")
        if not f_on <= allowed:
            bad.append((fixture, f_on, f_off))
    # the criterion with pred_qd from the fused path reproduces the fixture's two reid entries
    bz, Q, K, H, W, layers, C = (int(v) for v in g["cfg"])
    det = [{k: torch.from_numpy(g[f"det{i}.{k}"]).to(DEV) for k in ("labels", "boxes", "masks")} for i in range(bz)]
    ind = [[(torch.from_numpy(g[f"l{l}.sel{i}"]), torch.from_numpy(g[f"l{l}.gt{i}"])) for i in range(bz)] for l in range(layers)]
    logits = torch.stack([torch.from_numpy(g[f"l{l}.logits"]) for l in range(layers)]).float().to(DEV)
    boxes = torch.stack([torch.from_numpy(g[f"l{l}.boxes"]) for l in range(layers)]).float().to(DEV)
    masks = torch.cat([torch.cat([torch.from_numpy(g[f"l{l}.masks{i}"]) for i in range(bz)], 1)[0] for l in range(layers)]).float().to(DEV)
    crit = IDOLCriterion(K, OTAMatcher(), {}, ["labels", "boxes", "masks", "reid"], mask_out_stride=4)
    l_off = crit.forward_all_layers(logits, boxes, masks, det, ind, off)
    l_on = crit.forward_all_layers(logits, boxes, masks, det, ind, on)
    assert set(l_on) == set(l_off)
    for k in ("loss_reid", "loss_reid_aux"):
        fx = float(g["loss." + k])
        f_off, f_on = abs(float(l_off[k]) - fx) / abs(fx), abs(float(l_on[k]) - fx) / abs(fx)
        allowed = max(MULTIPLE * f_off, MULTIPLE * EPS)
        print(f"forward_all_layers {k}: fixture {fx:.9g}, fused {f_on:.3e}, unfused {f_off:.3e}, allowed {allowed:.3e}")
        if not f_on <= allowed:
            bad.append((k, f_on, f_off))
    assert not bad, bad


@pytest.mark.gpu
def test_a_zero_reference_row_with_its_aux_bit_set():
    key, ref, img, kq, flags = (t.clone() for t in case_and_reference("R63_C37_Q20")[0])
    ref[2, 5] = 0
    flags[-1, 5] |= 4
    case = (key, ref, img, kq, flags)
    w = torch.ones(len(img), 2)
    from vnext_amd.ops.reid_loss import reid_contrastive_losses
    with torch.no_grad():
        got = reid_contrastive_losses(key.to(DEV), ref.to(DEV), img.to(DEV), kq.to(DEV), flags.to(DEV)).cpu()
    yard = run_yardstick(case, w)[0]
    assert bool(torch.isfinite(got).all())
    err = float((got.double() - yard).abs().max()) / float(yard.abs().max())
    print(f"zero reference row: error {err:.3e}")
    assert err <= 1e-5                                       # cos = 0 at that row, as F.normalize gives: a different answer would be O(1) off


@pytest.mark.gpu
def test_an_instance_out_of_range_contributes_nothing():
    """key_query = -1 in the middle, img = B at the tail (img stays non-decreasing): (0, 0) for those, everything else bit
    for bit what the call without them gives"""
    case, w, _ = case_and_reference("R65_C64_Q300")
    key, ref, img, kq, flags = case
    want = run_fused(case, w)
    J, B = len(img), key.shape[0]
    at = 3
    ins = lambda v, mid, tail: torch.cat([v[:at], mid, v[at:], tail])      # noqa: E731
    i32 = lambda x: torch.tensor([x], dtype=torch.int32)      # noqa: E731
    bad_case = (key, ref, ins(img, img[at:at + 1], i32(B)), ins(kq, i32(-1), i32(0)),
                ins(flags, flags[:1] | 7, flags[:1] | 7))
    w_bad = ins(w, torch.ones(1, 2), torch.ones(1, 2))
    got = run_fused(bad_case, w_bad)
    keep = [j for j in range(J + 2) if j not in (at, J + 1)]
    assert not bool(got[0][[at, J + 1]].any())
    assert torch.equal(got[0][keep], want[0]) and torch.equal(got[1], want[1]) and torch.equal(got[2], want[2])


@pytest.mark.gpu
def test_no_instances_at_all():
    from vnext_amd.ops.reid_loss import reid_contrastive_losses
    key = torch.randn(2, 5, 8, device=DEV, requires_grad=True)
    ref = torch.randn(2, 7, 8, device=DEV, requires_grad=True)
    e = lambda *s, dt=torch.int32: torch.zeros(*s, dtype=dt, device=DEV)      # noqa: E731
    out = reid_contrastive_losses(key, ref, e(0), e(0), e(0, 7, dt=torch.uint8))
    assert out.shape == (0, 2)
    (out.sum() + 0 * key.sum()).backward()
    assert not bool(key.grad.any())
    with pytest.raises(Exception, match="reference rows"):
        reid_contrastive_losses(key, torch.randn(2, 1025, 8, device=DEV), e(0), e(0), e(0, 1025, dt=torch.uint8))


@pytest.mark.gpu
def test_strided_views_are_read_in_place():
    from vnext_amd.ops.reid_loss import reid_contrastive_losses
    # the halves of one [2 B, Q, C] tensor, as IDOL.losses hands them over (R = Q)
    case, w, ref64 = case_and_reference("large_magnitude")
    key, ref, img, kq, flags = case
    embeds = torch.stack([key, ref], 1).flatten(0, 1).to(DEV).requires_grad_(True)      # [2 B, Q, C]
    dargs = (img.to(DEV), kq.to(DEV), flags.to(DEV))
    out = reid_contrastive_losses(embeds[0::2], embeds[1::2], *dargs)
    (out * w.to(DEV)).sum().backward()
    plain = run_fused(case, w)
    assert torch.equal(out.detach(), plain[0])
    assert torch.equal(embeds.grad[0::2], plain[1]) and torch.equal(embeds.grad[1::2], plain[2])
    unfused = errors(run_unfused(case, w), ref64, img, 1)
    bad = held("embeds.grad", errors((out.detach(), embeds.grad[0::2], embeds.grad[1::2]), ref64, img, 1), unfused)
    assert not bad, bad
    # B = 3 halves of one tensor: image stride 2 Q C
    key, ref, img, kq, flags = synthetic(3, 40, 40, 64, (2, 0, 3), seed=21)
    w3 = torch.rand(len(img), 2, generator=torch.Generator().manual_seed(3)) + 0.5
    embeds = torch.stack([key, ref], 1).flatten(0, 1).to(DEV).requires_grad_(True)
    out = reid_contrastive_losses(embeds[0::2], embeds[1::2], img.to(DEV), kq.to(DEV), flags.to(DEV))
    (out * w3.to(DEV)).sum().backward()
    plain = run_fused((key, ref, img, kq, flags), w3)
    assert torch.equal(out.detach(), plain[0])
    assert torch.equal(embeds.grad[0::2], plain[1]) and torch.equal(embeds.grad[1::2], plain[2])


@pytest.mark.gpu
def test_sixteen_bit_inputs_are_read_as_fp32_and_the_gradients_keep_their_type():
    """bf16 embeddings against float64 of the same bf16 values.  The terms are fp32: the fp32 bound.  The gradients come
    back in bf16: the fp32 bound plus bf16's unit roundoff 2^-8 of the largest magnitude."""
    case, w, _ = case_and_reference("R65_C64_Q300")
    low = (case[0].bfloat16().float(), case[1].bfloat16().float()) + case[2:]
    ref = run_yardstick(low, w)
    B = low[0].shape[0]
    unfused = errors(run_unfused(low, w), ref, low[2], B)
    got = run_fused(case, w, dtype=torch.bfloat16)
    assert got[0].dtype == torch.float32 and got[1].dtype == torch.bfloat16 and got[2].dtype == torch.bfloat16
    ours = errors(got, ref, low[2], B)
    bad = held("bf16", {k: v for k, v in ours.items() if not k.startswith("grad")}, unfused)
    bad += held("bf16", {k: v for k, v in ours.items() if k.startswith("grad")}, unfused, extra=2.0 ** -8)
    assert not bad, bad


@pytest.mark.gpu
def test_two_calls_are_bit_identical():
    case, w, _ = case_and_reference(SHARED)
    a, b = run_fused(case, w), run_fused(case, w)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


@pytest.mark.gpu
def test_backward_through_the_c_abi_writes_every_element_and_nothing_else(hip_lib):
    from vnext_amd import _lib
    case, w, _ = case_and_reference(SHARED)
    key, ref, img, kq, flags = (t.to(DEV).contiguous() for t in case)
    B, Q, C = key.shape
    R, J, G = ref.shape[1], len(img), 64
    st = torch.cuda.current_stream().cuda_stream
    out, dot, rn, stats = (torch.empty(J, n, device=DEV) for n in (2, R, R, 8))
    geo = (key.data_ptr(), Q * C, Q, ref.data_ptr(), R * C, R, C, B, img.data_ptr(), kq.data_ptr(), flags.data_ptr(), J)
    assert hip_lib.vnx_reid_loss_forward(*geo, out.data_ptr(), dot.data_ptr(), rn.data_ptr(), stats.data_ptr(), st) == _lib.VNX_OK
    gk = torch.full((G + B * Q * C + G,), float("nan"), device=DEV)
    gr = torch.full((G + B * R * C + G,), float("nan"), device=DEV)
    go = w.to(DEV).contiguous()
    assert hip_lib.vnx_reid_loss_backward(*geo, dot.data_ptr(), rn.data_ptr(), stats.data_ptr(), go.data_ptr(),
                                          gk[G:].data_ptr(), gr[G:].data_ptr(), st) == _lib.VNX_OK
    torch.cuda.synchronize()
    for buf, n in ((gk, B * Q * C), (gr, B * R * C)):
        assert bool(torch.isnan(buf[:G]).all()) and bool(torch.isnan(buf[G + n:]).all())      # the guards are intact
        assert bool(torch.isfinite(buf[G:G + n]).all())                                       # every element was written
    pointed = torch.zeros(B, Q, dtype=torch.bool)
    pointed[case[2].long(), case[3].long()] = True
    assert not bool(gk[G:G + B * Q * C].view(B, Q, C).cpu()[~pointed].any())
    want = run_fused(case, w)
    assert torch.equal(gk[G:G + B * Q * C].view(B, Q, C), want[1]) and torch.equal(gr[G:G + B * R * C].view(B, R, C), want[2])
    # outside the supported sizes: a status, nothing launched
    bad = list(geo)
    bad[5] = 1025
    assert hip_lib.vnx_reid_loss_forward(*bad, out.data_ptr(), dot.data_ptr(), rn.data_ptr(), stats.data_ptr(), st) == _lib.VNX_ERR_UNSUPPORTED
    bad[5], bad[6] = R, 0
    assert hip_lib.vnx_reid_loss_backward(*bad, dot.data_ptr(), rn.data_ptr(), stats.data_ptr(), go.data_ptr(),
                                          gk[G:].data_ptr(), gr[G:].data_ptr(), st) == _lib.VNX_ERR_UNSUPPORTED


def _selections(counts, Q, seed):
    """per image (inst, pos, neg, aux) and matched ids, as the matcher and sample_aux_masks hand them over"""
    g = torch.Generator().manual_seed(seed)
    sel, matched = [], []
    for n in counts:
        pos = torch.rand(Q, n, generator=g) < 0.02
        neg = ~pos & (torch.rand(Q, n, generator=g) < 0.9)
        aux = pos | (neg & (torch.rand(Q, n, generator=g) < 0.1))
        sel.append((torch.arange(n), pos, neg, aux))
        matched.append(torch.randint(0, Q, (n,), generator=g))
    return matched, sel


class _HostToDevice(torch.utils._python_dispatch.TorchDispatchMode):
    """counts the ops that take a non-empty host tensor and return a device tensor: the uploads.  (The profiler cannot tell
    them apart here: it reports a copy from pinned host memory as `Memcpy DtoD`, like the copies between device tensors.)"""

    def __init__(self):
        super().__init__()
        self.ops = []

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        out = func(*args, **(kwargs or {}))
        if isinstance(out, torch.Tensor) and out.is_cuda and any(
                isinstance(a, torch.Tensor) and not a.is_cuda and a.numel() > 0 for a in args):
            self.ops.append(str(func))
        return out


@pytest.mark.gpu
def test_launch_counts_do_not_depend_on_the_batch():
    """the fused reid stage, forward + backward from the embedding views to embeds.grad: kernel launches and copies under
    torch.profiler, the uploads counted op by op.  What is held equal is the number of device operations, kernels plus
    copies: autograd's backward of `embeds[0::2]` writes the gradient into a slice of a zero tensor, and ATen does that
    with a memcpy where the slice is one contiguous block (B = 1) and with a copy kernel where it is strided (B = 3) --
    19 kernels + 5 copies against 21 + 3 on the MI355X, the op's own three launches in both."""
    from torch.profiler import ProfilerActivity, profile
    from vnext_amd.models.idol_criterion import reid_terms_fused
    Q, C = 300, 256
    counts = {}
    for B, per_image_counts in ((1, (8,)), (3, (4, 0, 6))):
        matched, sel = _selections(per_image_counts, Q, seed=B)
        embeds = torch.randn(2 * B, Q, C, device=DEV, requires_grad=True)

        def stage():
            embeds.grad = None
            qd = reid_terms_fused(embeds[0::2], embeds[1::2], matched, sel)
            (qd["contrast"] / qd["count"] + 1.5 * qd["aux"] / qd["count"]).backward()
        stage()
        torch.cuda.synchronize()
        with _HostToDevice() as uploads:
            stage()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
            stage()
            torch.cuda.synchronize()
        names = [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
        copies = [n for n in names if n.lower().startswith("memcpy")]
        kernels = [n for n in names if not n.lower().startswith(("memcpy", "memset"))]
        print(f"B = {B}: {len(kernels)} kernel launches, {len(copies)} copies {sorted(set(copies))}, uploads {uploads.ops}")
        print("\n".join("    " + n[:110] for n in kernels))
        assert sum("reid_loss" in n for n in kernels) == 3                   # one forward, two backward
        assert len(uploads.ops) == 1, uploads.ops                           # the one packed staging buffer
        counts[B] = len(kernels) + len(copies)
        assert float(embeds.grad.abs().sum()) > 0
    assert counts[1] == counts[3], counts


# ---- GPU: the model -----------------------------------------------------------------------------------------------------
def _step(model, clips):
    """one seeded forward + backward -> (loss dict, every parameter's gradient)"""
    model.zero_grad(set_to_none=True)
    torch.manual_seed(1)
    random.seed(1)                  # select_pos_neg_masks draws its negatives from the host generator
    losses = model(clips)
    sum(losses.values()).backward()
    grads = {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}
    model.zero_grad(set_to_none=True)
    return {k: v.detach().clone() for k, v in losses.items()}, grads


def _agree(tag, first, second, switched):
    """test_set_loss.py's rule (`_steps_agree`): switch-on may differ from the first switch-off step by ten times what
    two switch-off steps differ by, floor 1e-5; a loss in units of its own value, a gradient in units of the largest
    entry of the gradient of largest norm, the switch-off difference the largest over all gradients in that unit."""
    (loss_1, grad_1), (loss_2, grad_2), (loss_f, grad_f) = first, second, switched
    assert set(loss_f) == set(loss_1) and set(grad_f) == set(grad_1) and len(grad_f) >= 4
    biggest = max(grad_1, key=lambda k: float(grad_1[k].norm()))
    unit = float(grad_1[biggest].abs().max())
    failures = []
    for k in loss_1:
        scale = float(loss_1[k].abs()) or 1.0
        off_off, on_off = float((loss_1[k] - loss_2[k]).abs()) / scale, float((loss_f[k] - loss_1[k]).abs()) / scale
        allowed = max(10 * off_off, 1e-5)
        print(f"{tag} loss {k}: on-off {on_off:.3e}, off-off {off_off:.3e}, allowed {allowed:.3e}")
        if not on_off <= allowed:
            failures.append(("loss", k, on_off, allowed))
    off_off = {k: float((grad_1[k] - grad_2[k]).abs().max()) / unit for k in grad_1}
    on_off = {k: float((grad_f[k] - grad_1[k]).abs().max()) / unit for k in grad_1}
    noisiest, worst = max(off_off, key=off_off.get), max(on_off, key=on_off.get)
    allowed = max(10 * off_off[noisiest], 1e-5)
    print(f"{tag} {len(grad_1)} gradients; largest off-off {off_off[noisiest]:.3e} ({noisiest}), largest on-off "
          f"{on_off[worst]:.3e} ({worst}), allowed {allowed:.3e}")
    for k in grad_1:
        if not on_off[k] <= allowed:
            failures.append(("grad", k, on_off[k], allowed))
    return failures


@pytest.mark.gpu
def test_idol_step_is_the_same_with_the_fused_reid_loss():
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
    first, second = _step(model, pairs), _step(model, pairs)
    train.enable_fused_reid_loss(model)
    try:
        fused = _step(model, pairs)
        train.enable_device_matching(model)
        train.enable_fused_mask_loss(model)
        train.enable_fused_set_loss(model)
        all_four = _step(model, pairs)
    finally:
        model.device_matching = False
        model.criterion.fused_mask_loss = model.criterion.fused_set_loss = model.criterion.fused_reid_loss = False
    assert float(first[0]["loss_reid"]) > 0 and float(first[0]["loss_reid_aux"]) > 0
    head = [k for k in fused[1] if k.startswith("reid_embed_head") or ".reid_embed_head" in k]
    assert head and all(float(fused[1][k].abs().max()) > 0 for k in head), head
    failures = _agree("reid", first, second, fused) + _agree("all four", first, second, all_four)
    assert not failures, failures
