"""SeqFormer's Hungarian matching on the device (vnext_amd/csrc/lsap.hip, vnext_amd/ops/lsap.py,
HungarianMatcher.match_all_layers_device, SeqFormer.device_matching).

The references are scipy's linear_sum_assignment (the solver), HungarianMatcher.cost evaluated in float64 on the CPU (the
cost) and the indices the reference's own HungarianMatcher produced (tests/golden/criterion_seqformer.npz).  Where two
correct solvers may legitimately differ -- an optimum that is not unique, or not unique beyond the rounding of the cost --
the problem is identified by scipy alone (its *gap*: the smallest rise of the optimum when one pair of scipy's solution is
forbidden and the problem solved again), and the number of problems left out that way is capped at 5 %."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch
from scipy.optimize import linear_sum_assignment

from conftest import GOLDEN_DIR, ROOT
from vnext_amd.models.criterion import DeviceMatch, HungarianMatcher, SetCriterion, flat_pairs

NAMES = ("vnx_seqformer_match", "vnx_lsap_solve")
WEIGHTS = dict(cost_class=2.0, cost_bbox=5.0, cost_giou=2.0)      # the fixture's (and the model's) matcher weights


def _matcher():
    return HungarianMatcher(multi_frame=True, **WEIGHTS)


def _fixture(device="cpu"):
    g = dict(np.load(os.path.join(GOLDEN_DIR, "criterion_seqformer.npz")))
    bs, nf, Q, K, H, W, layers = (int(v) for v in g["cfg"])
    targets = [{"labels": torch.from_numpy(g[f"t{i}.labels"]).to(device), "boxes": torch.from_numpy(g[f"t{i}.boxes"]).to(device),
                "masks": torch.from_numpy(g[f"t{i}.masks"]).to(device), "size": torch.tensor([H, W])} for i in range(bs)]
    logits = torch.stack([torch.from_numpy(g[f"l{l}.logits"]) for l in range(layers)]).to(device)
    boxes = torch.stack([torch.from_numpy(g[f"l{l}.boxes"]) for l in range(layers)]).to(device)
    masks = torch.cat([torch.cat([torch.from_numpy(g[f"l{l}.masks{i}"]) for i in range(bs)], 1)[0]
                       for l in range(layers)]).to(device)
    return g, targets, logits, boxes, masks, (bs, nf, Q, K, layers)


def _hand_built_match(g, bs, layers, sizes, device, keys=("src", "tgt")):
    """the DeviceMatch of the fixture's own indices; `keys`: the fixture's names of a pair's two halves (the first half of
    criterion_idol.npz, `sel`, is a bool selection over the queries: its set positions are the queries)"""
    start = np.concatenate([[0], np.cumsum(sizes)])
    lay, clip, qry, tgt = [], [], [], []
    for l in range(layers):
        for i in range(bs):
            q, t = g[f"l{l}.{keys[0]}{i}"], g[f"l{l}.{keys[1]}{i}"]
            if q.dtype == np.bool_:
                q = np.nonzero(q)[0]
            lay.append(np.full_like(q, l)); clip.append(np.full_like(q, i)); qry.append(q); tgt.append(t + start[i])
    return DeviceMatch(*(torch.from_numpy(np.concatenate(a).astype(np.int64)).to(device) for a in (lay, clip, qry, tgt)))


@pytest.mark.parametrize("fixture, keys, labels, layers_at", [("criterion_seqformer", ("src", "tgt"), "t{}.labels", 6),
                                                             ("criterion_idol", ("sel", "gt"), "det{}.labels", 5)])
def test_flat_pairs_equals_the_hand_built_vectors(fixture, keys, labels, layers_at):
    """The one constructor of the pair list against the vectors built by hand here, for both forms the matchers return
    ((query idx, target idx) and (selected [Q] bool, target idx)): the fixture as it is, then with an image without
    targets put between its images and, for the bool form, with a layer in which nothing is selected."""
    g = dict(np.load(os.path.join(GOLDEN_DIR, fixture + ".npz")))
    bs, layers = int(g["cfg"][0]), int(g["cfg"][layers_at])
    assert bs >= 2 and layers >= 2
    sizes = [len(g[labels.format(i)]) for i in range(bs)]

    def both(g, bs, sizes):
        ind = [[tuple(torch.from_numpy(g[f"l{l}.{k}{i}"]) for k in keys) for i in range(bs)] for l in range(layers)]
        got, want = flat_pairs(ind, sizes, "cpu"), _hand_built_match(g, bs, layers, sizes, "cpu", keys)
        assert isinstance(got, DeviceMatch)
        for name, a, b in zip(DeviceMatch._fields, got, want):
            assert a.dtype == torch.int64 and torch.equal(a, b), name
        return got
    whole = both(g, bs, sizes)
    assert len(whole.qry) >= layers * sum(sizes) > 0      # every target in every layer, at least once
    # an image without targets in second place: the images after it move up one, the targets' offsets stay
    first = g[f"l0.{keys[0]}0"]
    wider = {}
    for l in range(layers):
        for i in range(bs):
            for k in keys:
                wider[f"l{l}.{k}{i + (i > 0)}"] = g[f"l{l}.{k}{i}"]
        wider[f"l{l}.{keys[0]}1"] = np.zeros_like(first) if first.dtype == np.bool_ else np.zeros(0, dtype=first.dtype)
        wider[f"l{l}.{keys[1]}1"] = np.zeros(0, dtype=np.int64)
    if first.dtype == np.bool_:                  # ... and nothing selected in layer 0
        for i in range(bs + 1):
            wider[f"l0.{keys[0]}{i}"], wider[f"l0.{keys[1]}{i}"] = np.zeros_like(first), np.zeros(0, dtype=np.int64)
    got = both(wider, bs + 1, sizes[:1] + [0] + sizes[1:])
    assert not bool((got.clip == 1).any()) and int(got.clip.max()) == bs
    assert torch.equal(got.tgt[got.lay == layers - 1], whole.tgt[whole.lay == layers - 1])
    if first.dtype == np.bool_:
        assert not bool((got.lay == 0).any()) and bool((got.lay == 1).any())


def _gap(cost64, maximize=False):
    """scipy's solution of cost64 and its gap (module docstring); inf when no other assignment exists"""
    r, c = linear_sum_assignment(cost64, maximize=maximize)
    best = cost64[r, c].sum()
    gap = np.inf
    for i, j in zip(r, c):
        other = cost64.copy()
        other[i, j] = -np.inf if maximize else np.inf
        try:
            r2, c2 = linear_sum_assignment(other, maximize=maximize)
        except ValueError:                      # forbidding the pair leaves no assignment
            continue
        rise = other[r2, c2].sum() - best
        gap = min(gap, -rise if maximize else rise)
    return r, c, gap


# ---- 1. ABI surface (CPU) ------------------------------------------------------------------------------------------
def test_abi_17_gains_the_two_entry_points():
    from vnext_amd import _lib
    assert _lib.ABI_VERSION == 17
    header = open(os.path.join(ROOT, "include", "vnext_hip.h")).read()
    assert "#define VNX_ABI_VERSION 17" in header
    declared = re.findall(r"\b(vnx_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", header, flags=re.S))
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if len(line.split()) == 3 and line.split()[1] == "T"}
    for name in NAMES:
        assert name in _lib.SIGNATURES
        assert name in declared
        assert name in exported


def test_cpu_tensors_and_models_without_the_switch_are_refused():
    from vnext_amd import train
    from vnext_amd.ops.lsap import lsap_solve, seqformer_match
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        lsap_solve(torch.zeros(3, 2))
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        seqformer_match(torch.zeros(1, 1, 3, 2), torch.zeros(1, 1, 1, 3, 4), torch.zeros(1, dtype=torch.int64),
                        torch.zeros(1, 1, 4), torch.tensor([0, 1], dtype=torch.int32), (1.0, 1.0, 1.0))
    with pytest.raises(ValueError, match="device_matching"):
        train.enable_device_matching(torch.nn.Linear(1, 1))

    class Switch:
        device_matching = False
    m = Switch()
    train.enable_device_matching(m)
    assert m.device_matching is True


# ---- 5. criterion: the device tuple in place of the host list (CPU part: no library needed) ---------------------------
def _criterion_both_ways(device):
    g, targets, logits, boxes, masks, (bs, nf, Q, K, layers) = _fixture(device)
    crit = SetCriterion(K, _matcher(), {}, ["labels", "boxes", "masks"], mask_out_stride=4, num_frames=nf)
    indices_list = [[(torch.from_numpy(g[f"l{l}.src{i}"]), torch.from_numpy(g[f"l{l}.tgt{i}"])) for i in range(bs)]
                    for l in range(layers)]
    want = crit.forward_all_layers(logits, boxes, masks, targets, indices_list)
    match = _hand_built_match(g, bs, layers, [len(t["labels"]) for t in targets], device)
    got = crit.forward_all_layers(logits, boxes, masks, targets, match)
    assert set(got) == set(want) and len(want) == 5 * layers + 1
    return got, want


def test_criterion_takes_the_device_tuple_cpu():
    got, want = _criterion_both_ways("cpu")
    for k in want:
        assert torch.equal(got[k], want[k]), k


@pytest.mark.gpu
def test_criterion_takes_the_device_tuple_gpu():
    """The same index tensors reach the same ATen kernels either way: bit-equal."""
    got, want = _criterion_both_ways("cuda:0")
    for k in want:
        print(k, float(got[k]), float(want[k]))
        assert torch.equal(got[k], want[k]), k


# ---- 2. the solver alone ---------------------------------------------------------------------------------------------
SHAPES = ((300, 1), (300, 4), (300, 20), (300, 64), (7, 7), (5, 12))
KINDS = ("uniform", "normal", "wide")


def _draw(rng, shape, kind):
    if kind == "uniform":
        m = rng.random(shape)
    elif kind == "normal":
        m = rng.standard_normal(shape)
    else:
        m = rng.standard_normal(shape) * 1000 - 5000
    return m.astype(np.float32)


def _check_assignment(r, c, cost32, maximize, want_unique=True):
    """one problem: one-to-one over the short side, scipy's optimum to 1e-9 relative (fp64 solve on fp32 entries: the
    rounding of a sum of <= 64 terms), scipy's indices where scipy's optimum is unique.  -> False when the problem's gap
    leaves the index comparison out."""
    rows, cols = cost32.shape
    k = min(rows, cols)
    assert r.shape == c.shape == (k,)
    assert np.all(np.diff(r) > 0) and r.min() >= 0 and r.max() < rows          # rows ascending, distinct
    assert len(set(c.tolist())) == k and c.min() >= 0 and c.max() < cols
    cost64 = cost32.astype(np.float64)
    sr, sc, gap = _gap(cost64, maximize)
    got, want = cost64[r, c].sum(), cost64[sr, sc].sum()
    assert abs(got - want) <= 1e-9 * abs(want), (got, want)
    if not want_unique:
        return True
    if not gap > 1e-9 * np.abs(cost64).max():
        return False
    np.testing.assert_array_equal(r, sr)
    np.testing.assert_array_equal(c, sc)
    return True


@pytest.mark.gpu
def test_solver_equals_scipy():
    from vnext_amd.ops.lsap import lsap_solve
    dev = "cuda:0"
    problems = left_out = 0
    for seed in range(3):
        rng = np.random.default_rng(seed)
        for shape in SHAPES:
            for kind in KINDS:
                m = _draw(rng, shape, kind)
                for maximize in (False, True):
                    if shape == (5, 12):            # through strides: the transposed view of a [12, 5] matrix
                        d = torch.from_numpy(np.ascontiguousarray(m.T)).to(dev).t()
                        assert not d.is_contiguous()
                    else:
                        d = torch.from_numpy(m).to(dev)
                    r, c = lsap_solve(d, maximize=maximize)
                    assert r.dtype == c.dtype == torch.int64
                    problems += 1
                    left_out += not _check_assignment(r.cpu().numpy(), c.cpu().numpy(), m, maximize)
    print(f"solver: {problems} problems, {left_out} left out of the index comparison by their gap")
    assert problems == 108 and left_out <= 0.05 * problems
    # one call, 18 problems
    rng = np.random.default_rng(7)
    batch = np.stack([_draw(rng, (300, 20), KINDS[i % 3]) for i in range(18)])
    r, c = lsap_solve(torch.from_numpy(batch).to(dev))
    assert r.shape == c.shape == (18, 20)
    out = sum(not _check_assignment(r[i].cpu().numpy(), c[i].cpu().numpy(), batch[i], False) for i in range(18))
    assert out <= 0.05 * 18
    # a constant row: many optima, judged by the cost alone
    m = _draw(np.random.default_rng(11), (7, 7), "normal")
    m[3] = 0.25
    for maximize in (False, True):
        r, c = lsap_solve(torch.from_numpy(m).to(dev), maximize=maximize)
        _check_assignment(r.cpu().numpy(), c.cpu().numpy(), m, maximize, want_unique=False)
    # the same input twice: the same output, bit for bit
    d = torch.from_numpy(batch).to(dev)
    a, b = lsap_solve(d), lsap_solve(d)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


@pytest.mark.gpu
def test_solver_marks_non_finite_problems():
    from vnext_amd.ops.lsap import lsap_solve
    rng = np.random.default_rng(3)
    good = _draw(rng, (300, 4), "normal")
    with_inf, with_nan = good.copy(), good.copy()
    with_inf[17, 2] = np.inf
    with_nan[250, 0] = np.nan
    r, c = lsap_solve(torch.from_numpy(np.stack([with_inf, good, with_nan])).to("cuda:0"))
    r, c = r.cpu().numpy(), c.cpu().numpy()
    for i in (0, 2):
        assert np.all(r[i] == -1) and np.all(c[i] == -1)
    assert _check_assignment(r[1], c[1], good, False)       # the neighbours of a bad problem are solved


# ---- 3. the cost the kernel solves -----------------------------------------------------------------------------------
def _model_sized_case(seed, device):
    """Ld = 6, N = 2, T = 5, Q = 300, K = 40, 4 and 9 targets; the distributions of the criterion fixture's recipe (box
    centres 0.2 + 0.6 rand, sizes 0.05 + 0.3 rand, labels randint(K)), logits randn - 2"""
    Ld, N, T, Q, K = 6, 2, 5, 300, 40
    g = torch.Generator().manual_seed(seed)

    def rand_boxes(*lead):
        return torch.cat([0.2 + 0.6 * torch.rand(*lead, 2, generator=g), 0.05 + 0.3 * torch.rand(*lead, 2, generator=g)], -1)
    logits = torch.randn(Ld, N, Q, K, generator=g) - 2
    boxes = rand_boxes(Ld, N, T, Q)
    targets = [{"labels": torch.randint(0, K, (n,), generator=g).to(device), "boxes": rand_boxes(n, T).to(device)}
               for n in (4, 9)]
    return logits.to(device), boxes.to(device), targets


def _edge_case(device):
    """cost only: a target touching the image border, one of zero width and one with a zero centre coordinate (both
    clamps of the GIoU term matter), a predicted box equal to a target, two identical targets"""
    T, Q, K = 2, 8, 5
    g = torch.Generator().manual_seed(5)
    tgt = torch.tensor([[0.05, 0.5, 0.1, 0.4],       # touches the left border
                        [0.5, 0.5, 0.0, 0.3],        # zero width
                        [0.0, 0.3, 0.2, 0.2],        # centre on the border: cx clamps to 1e-7
                        [0.6, 0.4, 0.3, 0.2],
                        [0.6, 0.4, 0.3, 0.2]])[:, None, :].repeat(1, T, 1)
    boxes = torch.cat([0.2 + 0.6 * torch.rand(1, 1, T, Q, 2, generator=g), 0.05 + 0.3 * torch.rand(1, 1, T, Q, 2, generator=g)], -1)
    boxes[0, 0, :, 0] = tgt[3]
    logits = torch.randn(1, 1, Q, K, generator=g) - 2
    targets = [{"labels": torch.tensor([0, 4, 2, 1, 1]).to(device), "boxes": tgt.to(device)}]
    return logits.to(device), boxes.to(device), targets


def _kernel_match(logits, boxes, targets, return_cost=True):
    from vnext_amd.ops.lsap import seqformer_match
    sizes = [len(t["labels"]) for t in targets]
    start = np.concatenate([[0], np.cumsum(sizes)])
    offsets = torch.tensor(start.tolist(), dtype=torch.int32).to(logits.device)
    labels = torch.cat([t["labels"] for t in targets])
    tb = torch.cat([t["boxes"] for t in targets])
    out = seqformer_match(logits, boxes, labels, tb, offsets, (WEIGHTS["cost_class"], WEIGHTS["cost_bbox"], WEIGHTS["cost_giou"]),
                          return_cost=return_cost, max_targets=max(sizes))
    return out, start


def _own_blocks(cost, start):
    """[Ld, N, Q, n_tot] -> the entries a clip's problem is made of, one flat array"""
    return np.concatenate([cost[:, i, :, start[i]:start[i + 1]].reshape(-1) for i in range(len(start) - 1)])


def _cost_errors(logits, boxes, targets):
    (_, _, cost), start = _kernel_match(logits, boxes, targets)
    # the same inputs for all three: what the kernel is given, fp32 (the fixture stores float64)
    cpu_t = [{"labels": t["labels"].cpu(), "boxes": t["boxes"].cpu().float()} for t in targets]
    l32, b32 = logits.cpu().float(), boxes.cpu().float()
    m = _matcher()
    ref64 = m.cost(l32.double(), b32.double(), cpu_t).numpy()
    ref32 = m.cost(l32, b32, cpu_t).numpy()
    assert ref64.dtype == np.float64 and ref32.dtype == np.float32
    cost = cost.cpu().numpy()
    # columns of other clips' targets are not part of any problem: the kernel leaves them alone (NaN from the op)
    for i in range(len(start) - 1):
        other = np.ones(cost.shape[-1], bool)
        other[start[i]:start[i + 1]] = False
        assert np.isnan(cost[:, i][..., other]).all()
    k, r64, r32 = _own_blocks(cost, start), _own_blocks(ref64, start), _own_blocks(ref32, start)
    assert np.isfinite(k).all()
    e_kernel = np.abs(k.astype(np.float64) - r64).max()
    e32 = np.abs(r32.astype(np.float64) - r64).max()
    bound = 2 * e32 + 4 * float(np.spacing(np.float32(np.abs(r64).max())))
    return e_kernel, e32, bound


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["fixture", "model_sized", "edge"])
def test_kernel_cost_equals_the_float64_expression(which):
    """bound: twice the error of the same expression in fp32 on the CPU (the kernel sums in another order than ATen) + 4 ulp
    of the largest cost magnitude"""
    dev = "cuda:0"
    if which == "fixture":
        _, targets, logits, boxes, _, _ = _fixture(dev)
    elif which == "model_sized":
        logits, boxes, targets = _model_sized_case(0, dev)
    else:
        logits, boxes, targets = _edge_case(dev)
    e_kernel, e32, bound = _cost_errors(logits, boxes, targets)
    print(f"cost {which}: kernel max abs error {e_kernel:.3e}, fp32 CPU expression {e32:.3e}, bound {bound:.3e}")
    assert e_kernel <= bound


# ---- 4. matching against the reference -------------------------------------------------------------------------------
def _split(match, layers, sizes):
    """DeviceMatch -> {(layer, clip): (queries, clip-local targets)} on the host"""
    start = np.concatenate([[0], np.cumsum(sizes)])
    n = int(start[-1])
    lay, clip, qry, tgt = (x.cpu().numpy() for x in match)
    assert lay.shape == clip.shape == qry.shape == tgt.shape == (layers * n,)
    out = {}
    for l in range(layers):
        for i in range(len(sizes)):
            s = slice(l * n + start[i], l * n + start[i + 1])
            assert np.all(lay[s] == l) and np.all(clip[s] == i)
            out[l, i] = (qry[s], tgt[s] - start[i])
    return out


@pytest.mark.gpu
def test_device_matching_equals_the_reference_indices():
    g, targets, logits, boxes, _, (bs, nf, Q, K, layers) = _fixture("cuda:0")
    sizes = [len(t["labels"]) for t in targets]
    assert sizes == [2, 0, 3]                       # the empty clip sits between two others
    match = _matcher().match_all_layers_device(logits, boxes, targets)
    assert isinstance(match, DeviceMatch) and all(x.is_cuda and x.dtype == torch.int64 for x in match)
    got = _split(match, layers, sizes)
    for l in range(layers):
        for i in range(bs):
            np.testing.assert_array_equal(got[l, i][0], g[f"l{l}.src{i}"])
            np.testing.assert_array_equal(got[l, i][1], g[f"l{l}.tgt{i}"])


@pytest.mark.gpu
def test_device_matching_equals_scipy_and_the_host_matcher_at_model_size():
    dev = "cuda:0"
    m = _matcher()
    problems = left_out = 0
    for seed in range(3):
        logits, boxes, targets = _model_sized_case(seed, dev)
        sizes = [len(t["labels"]) for t in targets]
        Ld = logits.shape[0]
        (qry, tgt, cost), start = _kernel_match(logits, boxes, targets)
        match = m.match_all_layers_device(logits, boxes, targets)
        assert torch.equal(match.qry, qry.flatten())          # the model's surface returns what the op returns
        got = _split(match, Ld, sizes)
        host = m.match_all_layers(logits, boxes, targets)
        cpu_t = [{k: v.cpu() for k, v in t.items()} for t in targets]
        ref64 = m.cost(logits.cpu().double(), boxes.cpu().double(), cpu_t).numpy()
        cost = cost.cpu().numpy()
        for l in range(Ld):
            for i in range(len(sizes)):
                # scipy on the cost the kernel solved: every problem
                sr, sc = linear_sum_assignment(cost[l, i, :, start[i]:start[i + 1]].astype(np.float64))
                np.testing.assert_array_equal(got[l, i][0], sr)
                np.testing.assert_array_equal(got[l, i][1], sc)
                # the host matcher on the same device tensors: where neither side's fp32 rounding can flip a pair
                problems += 1
                _, _, gap = _gap(ref64[l, i, :, start[i]:start[i + 1]])
                if not gap > 1e-4:
                    left_out += 1
                    continue
                np.testing.assert_array_equal(got[l, i][0], host[l][i][0].numpy())
                np.testing.assert_array_equal(got[l, i][1], host[l][i][1].numpy())
    print(f"model-sized matching: {problems} problems, {left_out} left out by a gap <= 1e-4")
    assert problems == 36 and left_out <= 0.05 * problems


@pytest.mark.gpu
def test_device_matching_of_a_batch_without_targets():
    dev = "cuda:0"
    nf, Q, K = 2, 5, 4
    targets = [{"labels": torch.zeros(0, dtype=torch.int64, device=dev), "boxes": torch.zeros(0, nf, 4, device=dev),
                "masks": torch.zeros(0, nf, 32, 32, dtype=torch.bool, device=dev)} for _ in range(2)]
    logits, boxes = torch.randn(3, 2, Q, K, device=dev), torch.rand(3, 2, nf, Q, 4, device=dev)
    match = _matcher().match_all_layers_device(logits, boxes, targets)
    assert all(x.numel() == 0 and x.dtype == torch.int64 and x.is_cuda for x in match)
    crit = SetCriterion(K, _matcher(), {}, ["labels", "boxes", "masks"], num_frames=nf)
    losses = crit.forward_all_layers(logits, boxes, torch.zeros(0, nf, 8, 8, device=dev), targets, match)
    assert float(losses["loss_bbox"]) == 0 and float(losses["loss_mask"]) == 0 and float(losses["loss_ce"]) > 0


# ---- 6 / 7. the model ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def seqformer():
    import vnext_amd.models  # noqa: F401
    from vnext_amd import train
    from vnext_amd.registry import build_model, get_seqformer_cfg
    dev = "cuda:0"
    torch.manual_seed(0)
    # dropout off: the fused dropout sites draw a new mask per call whatever the seed, and two steps are compared here
    model = build_model(get_seqformer_cfg(**{"MODEL.DEVICE": dev, "MODEL.SeqFormer.DROPOUT": 0.0})).train()
    clips = train.synthetic_clips(1, 5, 360, 640, dev, seed=100, num_instances=4)
    return model, clips


def _trunk(model, clips):
    torch.manual_seed(1)
    x, srcs, hs, memory, logits, boxes, refs = model._run(clips, want_refs=True)
    return hs, logits, boxes, refs, model._mask_features(srcs, memory)


@pytest.mark.gpu
def test_losses_after_the_trunk_do_not_touch_the_host(seqformer):
    """With the targets prepared and the caches warm, matching, the gather / controller / mask-head block and the
    criterion run under torch's sync-debug mode: a device-to-host copy raises there, and so does a blocking pageable
    upload.  The host matcher does raise, which shows the mode sees what this test claims."""
    from vnext_amd import train
    model, clips = seqformer
    targets = model.prepare_targets(clips)
    trunk = _trunk(model, clips)
    train.enable_device_matching(model)
    try:
        model._losses_after_trunk(targets, *trunk)           # warm-up: fills the caches of constants
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            losses = model._losses_after_trunk(targets, *trunk)
        finally:
            torch.cuda.set_sync_debug_mode("default")
        assert all(v.is_cuda for v in losses.values())
        train.enable_device_matching(model, False)
        torch.cuda.set_sync_debug_mode("error")
        try:
            with pytest.raises(RuntimeError):
                model._losses_after_trunk(targets, *trunk)
        finally:
            torch.cuda.set_sync_debug_mode("default")
    finally:
        model.device_matching = False
    assert all(bool(torch.isfinite(v)) for v in losses.values())


def _step(model, clips):
    """one seeded forward + backward -> (loss dict, gradients of the controller and of class_embed)"""
    model.zero_grad(set_to_none=True)
    torch.manual_seed(1)
    losses = model(clips)
    sum(losses.values()).backward()
    grads = {n: p.grad.detach().clone() for n, p in model.named_parameters()
             if p.grad is not None and (".controller." in n or "class_embed" in n)}
    model.zero_grad(set_to_none=True)
    return {k: v.detach().clone() for k, v in losses.items()}, grads


@pytest.mark.gpu
def test_model_step_is_the_same_with_device_matching(seqformer):
    """Same assignment => same autograd graph; what is left is the order of ATen's atomic adds in the backward of the
    gathers, which two host-path runs differ by as well.  That host-against-host difference is measured here, per
    tensor; the device path is allowed ten times it, with a floor of 1e-6 * max|tensor| where the two host runs agree
    exactly.  The loss terms are held to the same rule."""
    model, clips = seqformer
    m = model.criterion.matcher
    with torch.no_grad():
        targets = model.prepare_targets(clips)
        hs, logits, boxes, refs, feats = _trunk(model, clips)
        a = m.match_all_layers_device(logits, boxes, targets)
        b = m.match_all_layers_device(logits, boxes, targets)
        for x, y in zip(a, b):
            assert torch.equal(x, y)                      # two device-path runs: bit-identical indices
        assert int(a.qry.min()) >= 0
        host = flat_pairs(m.match_all_layers(logits, boxes, targets), [len(t["labels"]) for t in targets], logits.device)
        for x, y in zip(a, host):
            assert torch.equal(x, y)                      # ... and the host matcher's
    model.device_matching = False
    loss_h1, grad_h1 = _step(model, clips)
    loss_h2, grad_h2 = _step(model, clips)
    model.device_matching = True
    try:
        loss_d, grad_d = _step(model, clips)
    finally:
        model.device_matching = False
    assert set(loss_d) == set(loss_h1) and set(grad_d) == set(grad_h1) and len(grad_d) >= 4

    def check(kind, name, d, h1, h2):
        host_diff = float((h1 - h2).abs().max())
        dev_diff = float((d - h1).abs().max())
        allowed = max(10 * host_diff, 1e-6 * float(h1.abs().max()))
        print(f"{kind} {name}: device-host {dev_diff:.3e}, host-host {host_diff:.3e}, allowed {allowed:.3e}")
        assert dev_diff <= allowed, (kind, name)
    for k in loss_h1:
        check("loss", k, loss_d[k], loss_h1[k], loss_h2[k])
    for k in grad_h1:
        check("grad", k, grad_d[k], grad_h1[k], grad_h2[k])


# ---- 7. one pair list per training step ----------------------------------------------------------------------------
def count_flat_pairs(monkeypatch):
    """Put a counting wrapper in place of `flat_pairs` under every name the models package holds it by.
    -> the list of what the calls returned."""
    import vnext_amd.models.criterion as criterion
    import vnext_amd.models.idol as idol
    import vnext_amd.models.idol_criterion as idol_criterion
    import vnext_amd.models.seqformer as seqformer
    made = []

    def counting(*args, **kw):
        made.append(flat_pairs(*args, **kw))
        return made[-1]
    held = [mod for mod in (criterion, idol_criterion, seqformer, idol) if hasattr(mod, "flat_pairs")]
    assert criterion in held
    for mod in held:
        monkeypatch.setattr(mod, "flat_pairs", counting)
    return made


def record_calls(monkeypatch, owner, name):
    """-> the list of (args, kwargs) `owner.name` is called with from now on; the calls go through"""
    real, calls = getattr(owner, name), []

    def recording(*args, **kw):
        calls.append((args, kw))
        return real(*args, **kw)
    monkeypatch.setattr(owner, name, recording)
    return calls


@pytest.mark.gpu
def test_the_pair_list_is_built_once_per_step_on_the_host_matching_path(monkeypatch):
    """Host matching, deep supervision: one `flat_pairs` call per `model(clips)`, and the `DeviceMatch` it returned is
    both what orders the mask head's rows and, the same object, what the criterion is given.  Two decoder layers and two
    clips of 1 and 3 instances: the smallest batch in which a second, differently ordered list would show."""
    import vnext_amd.models  # noqa: F401
    import vnext_amd.models.seqformer as seqformer
    from vnext_amd import train
    from vnext_amd.registry import build_model, get_seqformer_cfg
    dev = "cuda:0"
    tiny = {"MODEL.SeqFormer.ENC_LAYERS": 1, "MODEL.SeqFormer.DEC_LAYERS": 2, "MODEL.SeqFormer.NUM_OBJECT_QUERIES": 12,
            "MODEL.SeqFormer.DIM_FEEDFORWARD": 64, "MODEL.SeqFormer.DROPOUT": 0.0, "INPUT.SAMPLING_FRAME_NUM": 2}
    torch.manual_seed(0)
    model = build_model(get_seqformer_cfg(**{"MODEL.DEVICE": dev, **tiny})).train()
    assert model.device_matching is False and model.deep_supervision
    T = 2
    clips = (train.synthetic_clips(1, T, 128, 192, dev, seed=3, num_instances=1) +
             train.synthetic_clips(1, T, 128, 192, dev, seed=4, num_instances=3))
    made = count_flat_pairs(monkeypatch)
    head = record_calls(monkeypatch, seqformer, "dynamic_mask_head")
    given = record_calls(monkeypatch, model.criterion, "forward_all_layers")
    losses = model(clips)
    assert len(made) == 1
    match = made[0]
    assert len(given) == 1 and given[0][0][4] is match                       # the criterion's `indices_list` argument
    assert len(match.qry) == 2 * (1 + 3) and all(x.is_cuda for x in match)
    assert match.clip.tolist() == [0, 1, 1, 1] * 2 and match.lay.tolist() == [0] * 4 + [1] * 4
    assert len(head) == 1
    image = head[0][0][3]                                                    # the frame each mask-head row reads
    assert torch.equal(image, ((match.clip * T)[:, None] + torch.arange(T, device=dev)[None, :]).flatten().to(torch.int32))
    assert all(bool(torch.isfinite(v)) for v in losses.values())
