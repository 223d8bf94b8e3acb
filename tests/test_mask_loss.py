"""The fused mask losses (vnext_amd/csrc/mask_loss.hip, vnext_amd/ops/mask_loss.py, the criteria's `fused_mask_loss`
switch, train.enable_fused_mask_loss): focal + dice of the matched instances' mask logits, the ground truth read in place.

The yardstick of the GPU tests is the criteria's own expression (slice, pad, gather, the `sigmoid_focal_loss` /
`dice_loss` terms before the final sum) in float64 on the CPU from the same fp32 logits.  The bound is not a constant:
on every case the present fp32 ATen composition runs on the device too, its error against float64 is measured, and the
fused op is allowed FOUR times that error (floor 4 * 2^-23 where ATen happens to be exact).  Why four: the only thing
that differs is the order of an fp32 sum, and a CPU emulation of the kernel's summation (fp32 pieces of 4 096 added in
order) came to at most 2.5 times ATen's fp32 error (focal at M = 288 000: 3.3e-7 against 1.3e-7).  Units: focal = largest
absolute error over the case's largest |focal| (a saturated row's focal term is near zero: a per-row relative error would
measure nothing), dice = absolute (a number in [0, 1]), grad_logits = absolute over max |grad| under random upstream
gradients.  Every test prints the figures before it asserts."""
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
NAMES = ("vnx_mask_loss_forward", "vnx_mask_loss_backward")
PIECE = 4096


# ---- the yardstick: the criteria's expression, any dtype / device ----------------------------------------------------
def compose(logits, gts, row_gt, stride, alpha=0.25, gamma=2.0):
    """logits [R, F, h, w], gts per clip [n_i, F, H_i, W_i] or [n_i, H_i, W_i] -> (focal [R], dice [R]): the lines of
    `SetCriterion.forward_all_layers` / `IDOLCriterion.forward_all_layers`, before the per-layer sums"""
    h, w = logits.shape[-2:]
    gt = []
    for m in gts:
        if m.dim() == 3:
            m = m[:, None]
        m = m[..., stride // 2::stride, stride // 2::stride]
        assert m.shape[-2] <= h and m.shape[-1] <= w
        gt.append(F.pad(m.to(logits.dtype), (0, w - m.shape[-1], 0, h - m.shape[-2])))
    gt = torch.cat(gt).to(logits.device)[row_gt.to(logits.device)].flatten(1)
    src = logits.flatten(1)
    pm = src.sigmoid()
    ce = F.binary_cross_entropy_with_logits(src, gt, reduction="none")
    pt = pm * gt + (1 - pm) * (1 - gt)
    fm = ce * (1 - pt) ** gamma
    if alpha >= 0:
        fm = (alpha * gt + (1 - alpha) * (1 - gt)) * fm
    dice = 1 - (2 * (pm * gt).sum(1) + 1) / (pm.sum(1) + gt.sum(1) + 1)
    return fm.mean(1), dice


def run(fn, logits, gts, row_gt, stride, wf, wd, **kw):
    """forward + backward under the upstream gradients wf, wd -> (focal, dice, grad_logits), detached"""
    x = logits.detach().clone().requires_grad_(True)
    focal, dice = fn(x, gts, row_gt, stride, **kw)
    ((focal * wf.to(focal)).sum() + (dice * wd.to(dice)).sum()).backward()
    return focal.detach(), dice.detach(), x.grad.detach()


def fused(x, gts, row_gt, stride, **kw):
    from vnext_amd.ops.mask_loss import mask_focal_dice
    return mask_focal_dice(x, gts, row_gt, stride, **kw)


# ---- cases -----------------------------------------------------------------------------------------------------------
def blobs(n, frames, H, W, g, fill=None):
    if fill is not None:
        return torch.full((n, frames, H, W), bool(fill))
    yy = torch.arange(H, dtype=torch.float32)[:, None]
    xx = torch.arange(W, dtype=torch.float32)[None, :]
    cy = torch.rand(n, frames, 1, 1, generator=g) * H
    cx = torch.rand(n, frames, 1, 1, generator=g) * W
    rad = 2 + torch.rand(n, frames, 1, 1, generator=g) * max(H, W) / 3
    return ((yy - cy) ** 2 + (xx - cx) ** 2) < rad * rad


def synthetic(frames, h, w, clips, R, stride=4, scale=3.0, fill=None, saturated=False, layered=False, squeeze=False,
              uint8=False, seed=0, **kw):
    """clips: [(n_i, H_i, W_i)].  row_gt: random targets (repeats) or, `layered`, every target once per layer."""
    g = torch.Generator().manual_seed(seed)
    gts = [blobs(n, frames, H, W, g, fill) for n, H, W in clips]
    if squeeze:
        gts = [m[:, 0] for m in gts]                    # IDOL: [n, H, W]
    if uint8:
        gts = [m.to(torch.uint8) for m in gts]
    total = sum(n for n, _, _ in clips)
    row_gt = torch.arange(total).repeat(R // total) if layered else torch.randint(0, total, (R,), generator=g)
    assert len(row_gt) == R
    logits = torch.randn(R, frames, h, w, generator=g) * scale
    if saturated:
        logits = torch.where(torch.rand(R, frames, h, w, generator=g) < 0.5, -30.0, 30.0) + torch.randn(R, frames, h, w, generator=g)
    return logits, gts, row_gt, stride, kw


def fixture_seqformer():
    g = dict(np.load(os.path.join(GOLDEN_DIR, "criterion_seqformer.npz")))
    bs, nf, Q, K, H, W, layers = (int(v) for v in g["cfg"])
    gts = [torch.from_numpy(g[f"t{i}.masks"]).bool() for i in range(bs)]
    start = np.cumsum([0] + [len(m) for m in gts])
    logits = torch.cat([torch.cat([torch.from_numpy(g[f"l{l}.masks{i}"]) for i in range(bs)], 1)[0] for l in range(layers)])
    row_gt = torch.cat([torch.from_numpy(g[f"l{l}.tgt{i}"]).long() + int(start[i]) for l in range(layers) for i in range(bs)])
    return logits.float(), gts, row_gt, 4, {}


def fixture_idol():
    g = dict(np.load(os.path.join(GOLDEN_DIR, "criterion_idol.npz")))
    bz, Q, K, H, W, layers, C = (int(v) for v in g["cfg"])
    gts = [torch.from_numpy(g[f"det{i}.masks"]).bool() for i in range(bz)]
    start = np.cumsum([0] + [len(m) for m in gts])
    logits = torch.cat([torch.cat([torch.from_numpy(g[f"l{l}.masks{i}"]) for i in range(bz)], 1)[0] for l in range(layers)])
    row_gt = torch.cat([torch.from_numpy(g[f"l{l}.gt{i}"]).long() + int(start[i]) for l in range(layers) for i in range(bz)])
    return logits.float(), gts, row_gt, 4, {}


CASES = {
    "fixture_seqformer": fixture_seqformer,
    "fixture_idol": fixture_idol,
    # the benchmark's clip: Ld = 6, 4 instances, T = 5, 360 x 640 -> R = 24, M = 72 000
    "bench_R24_M72000": lambda: synthetic(5, 90, 160, [(4, 360, 640)], 24, layered=True),
    "F1_128_rows_three_images": lambda: synthetic(1, 40, 64, [(5, 160, 256), (3, 150, 250), (4, 160, 256)], 128, squeeze=True),
    # w % 4 != 0 (element-per-lane path); H, W not multiples of the stride and smaller than the canvas (13 x 27 cells = 52 x 108)
    "w27_H50_W106": lambda: synthetic(2, 13, 27, [(3, 50, 106)], 7),
    # w % 4 == 0 but W % 16 != 0 (16-byte logits, byte-wise ground truth); the padded region is most of the canvas
    "gt_much_smaller_than_canvas": lambda: synthetic(5, 32, 48, [(4, 70, 100)], 12),
    "two_sizes_and_an_empty_clip_between": lambda: synthetic(3, 24, 28, [(3, 64, 96), (0, 80, 80), (2, 48, 112)], 15),
    "twenty_clips_of_different_sizes": lambda: synthetic(2, 16, 20, [(1 + i % 2, 30 + i, 80 - 3 * i) for i in range(20)], 45),
    "eighteen_clips_of_one_size": lambda: synthetic(1, 16, 32, [(1, 64, 128)] * 18, 36, layered=True),
    "all_zero_target": lambda: synthetic(2, 20, 32, [(3, 80, 128)], 6, fill=0),
    "all_one_target": lambda: synthetic(2, 20, 32, [(3, 80, 128)], 6, fill=1),
    "logits_of_magnitude_30": lambda: synthetic(2, 20, 32, [(3, 80, 128)], 6, saturated=True),
    "M_one_more_than_a_piece": lambda: synthetic(1, 1, PIECE + 1, [(2, 4, 4 * PIECE + 4)], 3),
    "M_one_fewer_than_two_pieces": lambda: synthetic(1, 1, 2 * PIECE - 1, [(2, 4, 8 * PIECE - 4)], 3),
    "M_four_more_than_a_piece_vector_path": lambda: synthetic(1, 1, PIECE + 4, [(2, 4, 4 * PIECE + 16)], 3),
    "M_four_fewer_than_two_pieces_vector_path": lambda: synthetic(1, 1, 2 * PIECE - 4, [(2, 4, 8 * PIECE - 16)], 3),
    "stride_2_uint8": lambda: synthetic(2, 24, 40, [(3, 47, 80), (2, 48, 75)], 9, stride=2, uint8=True),
    "stride_1_gamma_1p5_no_alpha": lambda: synthetic(1, 24, 40, [(3, 24, 40)], 5, stride=1, alpha=-1.0, gamma=1.5),
}


def errors(got, ref):
    focal, dice, grad = (t.double().cpu() for t in got)
    rf, rd, rg = ref
    return {"focal": float((focal - rf).abs().max()) / float(rf.abs().max()),
            "dice": float((dice - rd).abs().max()),
            "grad": float((grad - rg).abs().max()) / float(rg.abs().max())}


# ---- CPU ---------------------------------------------------------------------------------------------------------------
def test_entry_points_are_declared_bound_and_exported(hip_lib):
    from vnext_amd import _lib
    header = open(os.path.join(ROOT, "include", "vnext_hip.h")).read()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, header) and name in _lib.SIGNATURES and hasattr(hip_lib, name)
        assert re.search(r" T %s$" % name, out, re.M), name
    assert _lib.ABI_VERSION == 17 and hip_lib.vnx_abi_version() == 17       # additive: the version stays
    assert "#define VNX_MASK_LOSS_MAX_CLIPS %d" % _lib.MASK_LOSS_MAX_CLIPS in header
    assert "#define VNX_MASK_LOSS_PIECE %d" % _lib.MASK_LOSS_PIECE in header and _lib.MASK_LOSS_PIECE == PIECE


def test_the_clip_table_has_the_headers_layout():
    import ctypes
    from vnext_amd import _lib
    n = _lib.MASK_LOSS_MAX_CLIPS
    assert ctypes.sizeof(_lib.MaskLossClips) == n * 8 + 3 * n * 4 + 8
    assert [f[0] for f in _lib.MaskLossClips._fields_] == ["masks", "height", "width", "first", "count", "total"]


def test_cpu_tensors_are_rejected():
    from vnext_amd.ops.mask_loss import mask_focal_dice
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        mask_focal_dice(torch.zeros(2, 1, 4, 4), [torch.zeros(2, 1, 16, 16, dtype=torch.bool)], torch.zeros(2, dtype=torch.int64), 4)


def test_the_switch_and_its_setter():
    import vnext_amd.models  # noqa: F401
    from vnext_amd import train
    from vnext_amd.models.criterion import SetCriterion
    from vnext_amd.models.idol_criterion import IDOLCriterion
    from vnext_amd.registry import build_model, get_idol_cfg, get_seqformer_cfg
    with pytest.raises(ValueError, match="fused_mask_loss"):
        train.enable_fused_mask_loss(torch.nn.Linear(1, 1))
    tiny_s = {"MODEL.SeqFormer.ENC_LAYERS": 1, "MODEL.SeqFormer.DEC_LAYERS": 1, "MODEL.SeqFormer.DIM_FEEDFORWARD": 64}
    tiny_i = {"MODEL.IDOL.ENC_LAYERS": 1, "MODEL.IDOL.DEC_LAYERS": 1, "MODEL.IDOL.DIM_FEEDFORWARD": 64}
    for cfg, kind in ((get_seqformer_cfg(**{"MODEL.DEVICE": "cpu", **tiny_s}), SetCriterion),
                      (get_idol_cfg(**{"MODEL.DEVICE": "cpu", **tiny_i}), IDOLCriterion)):
        model = build_model(cfg)
        assert isinstance(model.criterion, kind) and model.criterion.fused_mask_loss is False      # off on a fresh model
        train.enable_fused_mask_loss(model)
        assert model.criterion.fused_mask_loss is True
        train.enable_fused_mask_loss(model, False)
        assert model.criterion.fused_mask_loss is False


def test_with_the_switch_on_the_criteria_raise_on_cpu_tensors():
    """No fallback behind the switch: the same inputs that test_criterion.py / test_idol_criterion.py feed on the CPU."""
    from vnext_amd.models.criterion import HungarianMatcher, SetCriterion
    from vnext_amd.models.idol_criterion import IDOLCriterion, OTAMatcher
    logits, gts, row_gt, stride, _ = fixture_seqformer()
    g = dict(np.load(os.path.join(GOLDEN_DIR, "criterion_seqformer.npz")))
    bs, nf, Q, K, H, W, layers = (int(v) for v in g["cfg"])
    targets = [{"labels": torch.from_numpy(g[f"t{i}.labels"]), "boxes": torch.from_numpy(g[f"t{i}.boxes"]).float(),
                "masks": gts[i]} for i in range(bs)]
    ind = [[(torch.from_numpy(g[f"l{l}.src{i}"]), torch.from_numpy(g[f"l{l}.tgt{i}"])) for i in range(bs)] for l in range(layers)]
    crit = SetCriterion(K, HungarianMatcher(), {}, ["labels", "boxes", "masks"], mask_out_stride=4, num_frames=nf)
    args = (torch.stack([torch.from_numpy(g[f"l{l}.logits"]) for l in range(layers)]).float(),
            torch.stack([torch.from_numpy(g[f"l{l}.boxes"]) for l in range(layers)]).float(), logits, targets, ind)
    crit.forward_all_layers(*args)                                   # off: the ATen path runs on the CPU
    crit.fused_mask_loss = True
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        crit.forward_all_layers(*args)
    n_last = sum(len(q) for q, _ in ind[-1])
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        crit.loss_masks({"pred_masks": logits[-n_last:]}, targets, ind[-1], torch.tensor(5.0))
    il, igts, irow, _, _ = fixture_idol()
    gi = dict(np.load(os.path.join(GOLDEN_DIR, "criterion_idol.npz")))
    bz, Q, K, H, W, layers, C = (int(v) for v in gi["cfg"])
    det = [{"labels": torch.from_numpy(gi[f"det{i}.labels"]), "boxes": torch.from_numpy(gi[f"det{i}.boxes"]).float(),
            "masks": igts[i]} for i in range(bz)]
    iind = [[(torch.from_numpy(gi[f"l{l}.sel{i}"]), torch.from_numpy(gi[f"l{l}.gt{i}"])) for i in range(bz)] for l in range(layers)]
    icrit = IDOLCriterion(K, OTAMatcher(), {}, ["labels", "boxes", "masks", "reid"], mask_out_stride=4)
    iargs = (torch.stack([torch.from_numpy(gi[f"l{l}.logits"]) for l in range(layers)]).float(),
             torch.stack([torch.from_numpy(gi[f"l{l}.boxes"]) for l in range(layers)]).float(), il, det, iind,
             {"contrast": 0, "aux": 0, "count": 0})
    icrit.forward_all_layers(*iargs)
    icrit.fused_mask_loss = True
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        icrit.forward_all_layers(*iargs)


def test_the_three_kernels_use_no_scratch_and_spill_nothing(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    src = os.path.join(ROOT, "vnext_amd", "csrc", "mask_loss.hip")
    p = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-munsafe-fp-atomics", "-I", os.path.dirname(src),
                        "-S", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-o", str(tmp_path / "mask_loss.s"),
                        src], capture_output=True, text=True, check=True)
    usage = {}
    for block in re.split(r"remark: Function Name: ", p.stderr)[1:]:
        name = block.split()[0]
        usage[name] = {k: int(v) for k, v in re.findall(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+) \[-Rpass", block)}
    kernels = {k: v for k, v in usage.items() if "mask_loss" in k}
    print(kernels)
    assert sorted(re.search(r"mask_loss_(\w+?)_kernel", k).group(1) for k in kernels) == ["bwd", "finish", "fwd"]
    for name, u in kernels.items():
        assert u["ScratchSize"] == 0 and u["SGPRs Spill"] == 0 and u["VGPRs Spill"] == 0, (name, u)
    text = open(tmp_path / "mask_loss.s").read()
    assert not re.search(r"^\s+scratch_", text, re.M)            # no scratch instruction
    assert [int(v) for v in re.findall(r"\.private_segment_fixed_size:\s*(\d+)", text)] == [0, 0, 0]


# ---- GPU: the op against float64 -----------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_op_against_float64(name):
    logits, gts, row_gt, stride, kw = CASES[name]()
    R = logits.shape[0]
    g = torch.Generator().manual_seed(7)
    wf, wd = torch.rand(R, generator=g) + 0.5, torch.rand(R, generator=g) + 0.5
    ref = run(compose, logits.double(), gts, row_gt, stride, wf.double(), wd.double(), **kw)
    dl, dg, dr = logits.to(DEV), [m.to(DEV) for m in gts], row_gt.to(DEV)
    aten = errors(run(compose, dl, dg, dr, stride, wf.to(DEV), wd.to(DEV), **kw), ref)
    got = run(fused, dl, dg, dr, stride, wf.to(DEV), wd.to(DEV), **kw)
    assert got[0].shape == (R,) and got[1].shape == (R,) and got[0].dtype == torch.float32 and got[2].shape == logits.shape
    ours = errors(got, ref)
    for k in ("focal", "dice", "grad"):
        allowed = max(4 * aten[k], 4 * EPS)
        print(f"{name} {k}: fused {ours[k]:.3e}, ATen fp32 {aten[k]:.3e}, ratio {ours[k] / max(aten[k], 1e-30):.2f}, "
              f"allowed {allowed:.3e}")
    for k in ("focal", "dice", "grad"):
        assert ours[k] <= max(4 * aten[k], 4 * EPS), (name, k, ours[k], aten[k])


@pytest.mark.gpu
def test_sixteen_bit_logits_are_cast_and_the_gradient_keeps_their_type():
    logits, gts, row_gt, stride, _ = CASES["gt_much_smaller_than_canvas"]()
    x = logits.to(DEV, torch.bfloat16).requires_grad_(True)
    focal, dice = fused(x, [m.to(DEV) for m in gts], row_gt.to(DEV), stride)
    (focal.sum() + dice.sum()).backward()
    f32 = run(fused, x.detach().float(), [m.to(DEV) for m in gts], row_gt.to(DEV), stride, torch.ones(len(row_gt)), torch.ones(len(row_gt)))
    assert focal.dtype == torch.float32 and x.grad.dtype == torch.bfloat16
    assert torch.equal(focal, f32[0]) and torch.equal(dice, f32[1]) and torch.equal(x.grad, f32[2].to(torch.bfloat16))


@pytest.mark.gpu
def test_no_rows_launch_nothing_and_rows_outside_the_targets_have_target_zero():
    gts = [torch.ones(2, 1, 16, 16, dtype=torch.bool, device=DEV)]
    x = torch.zeros(0, 1, 4, 4, device=DEV, requires_grad=True)
    focal, dice = fused(x, gts, torch.zeros(0, dtype=torch.int64, device=DEV), 4)
    assert focal.shape == (0,) and dice.shape == (0,)
    (focal.sum() + dice.sum()).backward()
    assert x.grad.shape == x.shape
    logits = torch.randn(3, 1, 4, 4, device=DEV)
    out = fused(logits, gts, torch.tensor([-1, 2, 7], device=DEV), 4)
    want = fused(logits, [torch.zeros_like(gts[0])], torch.tensor([0, 1, 0], device=DEV), 4)
    assert torch.equal(out[0], want[0]) and torch.equal(out[1], want[1])


# ---- GPU: against the reference's numbers ---------------------------------------------------------------------------------
def _held_to_the_fixture(kind, want, off, on):
    for k in sorted(want):
        if not (k.startswith("loss_mask") or k.startswith("loss_dice")):
            continue
        e_off = abs(float(off[k]) - want[k]) / abs(want[k])
        e_on = abs(float(on[k]) - want[k]) / abs(want[k])
        allowed = max(4 * e_off, 4 * EPS)
        print(f"{kind} {k}: fixture {want[k]:.9g}, switch on {e_on:.3e}, switch off {e_off:.3e}, allowed {allowed:.3e}")
        assert e_on <= allowed, (kind, k, e_on, e_off)


@pytest.mark.gpu
def test_seqformer_criterion_reproduces_the_reference_losses():
    from vnext_amd.models.criterion import HungarianMatcher, SetCriterion
    g = dict(np.load(os.path.join(GOLDEN_DIR, "criterion_seqformer.npz")))
    bs, nf, Q, K, H, W, layers = (int(v) for v in g["cfg"])
    masks, gts, _, _, _ = fixture_seqformer()
    targets = [{"labels": torch.from_numpy(g[f"t{i}.labels"]).to(DEV), "boxes": torch.from_numpy(g[f"t{i}.boxes"]).float().to(DEV),
                "masks": gts[i].to(DEV)} for i in range(bs)]
    ind = [[(torch.from_numpy(g[f"l{l}.src{i}"]), torch.from_numpy(g[f"l{l}.tgt{i}"])) for i in range(bs)] for l in range(layers)]
    crit = SetCriterion(K, HungarianMatcher(), {}, ["labels", "boxes", "masks"], mask_out_stride=4, num_frames=nf)
    args = (torch.stack([torch.from_numpy(g[f"l{l}.logits"]) for l in range(layers)]).float().to(DEV),
            torch.stack([torch.from_numpy(g[f"l{l}.boxes"]) for l in range(layers)]).float().to(DEV), masks.to(DEV), targets, ind)
    want = {k[5:]: float(v) for k, v in g.items() if k.startswith("loss.")}
    off = crit.forward_all_layers(*args)
    n_last = sum(len(q) for q, _ in ind[-1])
    num_boxes = torch.tensor(float(sum(len(t["labels"]) for t in targets)), device=DEV)
    last = {"pred_masks": masks[-n_last:].to(DEV)}
    off_last = crit.loss_masks(last, targets, ind[-1], num_boxes)
    crit.fused_mask_loss = True
    on = crit.forward_all_layers(*args)
    on_last = crit.loss_masks(last, targets, ind[-1], num_boxes)
    assert set(on) == set(off) == set(want)
    _held_to_the_fixture("forward_all_layers", want, off, on)
    _held_to_the_fixture("loss_masks", {k: want[k] for k in ("loss_mask", "loss_dice")}, off_last, on_last)


@pytest.mark.gpu
def test_idol_criterion_reproduces_the_reference_losses():
    from vnext_amd.models.idol_criterion import IDOLCriterion, OTAMatcher
    g = dict(np.load(os.path.join(GOLDEN_DIR, "criterion_idol.npz")))
    bz, Q, K, H, W, layers, C = (int(v) for v in g["cfg"])
    masks, gts, _, _, _ = fixture_idol()
    det = [{"labels": torch.from_numpy(g[f"det{i}.labels"]).to(DEV), "boxes": torch.from_numpy(g[f"det{i}.boxes"]).float().to(DEV),
            "masks": gts[i].to(DEV)} for i in range(bz)]
    ind = [[(torch.from_numpy(g[f"l{l}.sel{i}"]), torch.from_numpy(g[f"l{l}.gt{i}"])) for i in range(bz)] for l in range(layers)]
    crit = IDOLCriterion(K, OTAMatcher(), {}, ["labels", "boxes", "masks", "reid"], mask_out_stride=4)
    args = (torch.stack([torch.from_numpy(g[f"l{l}.logits"]) for l in range(layers)]).float().to(DEV),
            torch.stack([torch.from_numpy(g[f"l{l}.boxes"]) for l in range(layers)]).float().to(DEV), masks.to(DEV), det, ind,
            {"contrast": 0, "aux": 0, "count": 0})          # the reid terms are not what this test looks at
    want = {k[5:]: float(v) for k, v in g.items() if k.startswith("loss.")}
    off = crit.forward_all_layers(*args)
    n_last = sum(int(sel.sum()) for sel, _ in ind[-1])
    last = {"pred_masks": masks[-n_last:].to(DEV)}
    off_last = crit.loss_masks(last, det, None, ind[-1], None)
    crit.fused_mask_loss = True
    on = crit.forward_all_layers(*args)
    on_last = crit.loss_masks(last, det, None, ind[-1], None)
    assert set(on) == set(off)
    _held_to_the_fixture("forward_all_layers", want, off, on)
    _held_to_the_fixture("loss_masks", {k: want[k] for k in ("loss_mask", "loss_dice")}, off_last, on_last)


# ---- GPU: determinism, memory ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_two_calls_are_bit_identical():
    logits, gts, row_gt, stride, _ = CASES["bench_R24_M72000"]()
    g = torch.Generator().manual_seed(3)
    wf, wd = torch.rand(24, generator=g).to(DEV), torch.rand(24, generator=g).to(DEV)
    dl, dg, dr = logits.to(DEV), [m.to(DEV) for m in gts], row_gt.to(DEV)
    a = run(fused, dl, dg, dr, stride, wf, wd)
    b = run(fused, dl, dg, dr, stride, wf, wd)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


@pytest.mark.gpu
def test_forward_and_backward_allocate_little_more_than_the_gradient():
    """Around the op's own forward + backward at R = 24, M = 72 000 the peak of allocated memory rises by at most 1.25
    times the logits' bytes (the gradient, plus partial sums and the allocator's rounding); the ATen expression on the
    same inputs rises by more than that, which shows the measure sees what it claims."""
    logits, gts, row_gt, stride, _ = CASES["bench_R24_M72000"]()
    dl, dg, dr = logits.to(DEV), [m.to(DEV) for m in gts], row_gt.to(DEV)
    ones = torch.ones(24, device=DEV)

    def rise(fn):
        x = dl.clone().requires_grad_(True)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        focal, dice = fn(x, dg, dr, stride)
        ((focal * ones).sum() + (dice * ones).sum()).backward()
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - before
    rise(fused)                                              # warm-up: code objects, cached constants
    nbytes = dl.numel() * 4
    ours, aten = rise(fused), rise(compose)
    print(f"logits {nbytes} B; peak rise fused {ours} B = {ours / nbytes:.3f} x, ATen {aten} B = {aten / nbytes:.2f} x")
    assert ours <= 1.25 * nbytes
    assert aten > 1.25 * nbytes


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
def test_losses_after_the_trunk_do_not_touch_the_host_with_both_switches(seqformer):
    """test_device_matching.py's scenario with the fused mask losses on as well: under torch's sync-debug mode a
    device-to-host copy or a blocking pageable upload raises."""
    from vnext_amd import train
    model, clips = seqformer
    targets = model.prepare_targets(clips)
    torch.manual_seed(1)
    x, srcs, hs, memory, logits, boxes, refs = model._run(clips, want_refs=True)
    trunk = (hs, logits, boxes, refs, model._mask_features(srcs, memory))
    train.enable_device_matching(model)
    train.enable_fused_mask_loss(model)
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
    assert all(v.is_cuda for v in losses.values())
    assert all(bool(torch.isfinite(v)) for v in losses.values())
    assert float(losses["loss_mask"]) > 0 and float(losses["loss_dice"]) > 0


MASK_BRANCH = (".controller.", "mask_head", "mask_branch")


def _step(model, clips):
    """one seeded forward + backward -> (loss dict, gradients of the controller and the mask branch)"""
    model.zero_grad(set_to_none=True)
    torch.manual_seed(1)
    random.seed(1)                  # IDOL: select_pos_neg_masks draws its negatives from the host generator
    losses = model(clips)
    sum(losses.values()).backward()
    grads = {n: p.grad.detach().clone() for n, p in model.named_parameters()
             if p.grad is not None and any(s in n for s in MASK_BRANCH)}
    model.zero_grad(set_to_none=True)
    return {k: v.detach().clone() for k, v in losses.items()}, grads


def _steps_agree(model, clips):
    """Switch off twice, on once.  Losses and the controller / mask-branch gradients with the switch on differ from the
    first switch-off run by at most max(10 * off-off difference, 1e-5 * max|tensor|): the 10 x rule is
    test_device_matching.py's; the floor is ten times its 1e-6 because here an fp32 sum is reassociated, not just
    its atomics reordered."""
    model.criterion.fused_mask_loss = False
    loss_1, grad_1 = _step(model, clips)
    loss_2, grad_2 = _step(model, clips)
    model.criterion.fused_mask_loss = True
    try:
        loss_f, grad_f = _step(model, clips)
    finally:
        model.criterion.fused_mask_loss = False
    assert set(loss_f) == set(loss_1) and set(grad_f) == set(grad_1) and len(grad_f) >= 4
    failures = []
    for kind, f, a, b in (("loss", loss_f, loss_1, loss_2), ("grad", grad_f, grad_1, grad_2)):
        for k in a:
            off_off = float((a[k] - b[k]).abs().max())
            on_off = float((f[k] - a[k]).abs().max())
            allowed = max(10 * off_off, 1e-5 * float(a[k].abs().max()))
            print(f"{kind} {k}: on-off {on_off:.3e}, off-off {off_off:.3e}, allowed {allowed:.3e}")
            if not on_off <= allowed:
                failures.append((kind, k, on_off, allowed))
    assert not failures, failures


@pytest.mark.gpu
def test_seqformer_step_is_the_same_with_the_fused_mask_loss(seqformer):
    model, clips = seqformer
    _steps_agree(model, clips)


@pytest.mark.gpu
def test_idol_step_is_the_same_with_the_fused_mask_loss():
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
