"""The loss, matching and selection ops under hipGraph capture: what include/vnext_hip.h promises with "no allocation, no
synchronisation: capturable in a hipGraph" for vnx_lsap_solve / vnx_seqformer_match, vnx_mask_loss_*, vnx_set_loss_*,
vnx_reid_loss_*, vnx_swin_residual_norm_* / vnx_swin_merge_norm_*, vnx_mask_rle_measure / _write, vnx_det_select and
vnx_idol_match, and the SeqFormer loss stage that is made of them.

A captured launch carries its arguments BY VALUE: shapes, strides, thresholds, and for the mask loss a struct of
ground-truth pointers.  What a replay must still do is read the MEMORY those pointers name as it is at replay time -- not
what the host saw when the graph was captured.  `replay_check` pins that: capture on input set 0, overwrite every static
input in place with set s, poison every result buffer, replay, and compare (1) bit for bit with the same call made eagerly
on set s, (2) with the op's own independent reference under the bound its own test file uses, imported from there, and
(3) that no poison is left.  The sets differ in every index input and in every reference output (a property of the
inputs, asserted on the CPU), so a value baked at capture shows.  The harness itself is tested on the CPU with fake
capturers: one that replays honestly passes, one that returns what it recorded at capture, one that writes nothing and
one that reads a stale copy of an index input are caught.

DESIGN.md, "What a captured launch bakes in", lists per op what travels by value."""
import functools

import numpy as np
import pytest
import torch

import test_det_select as DT
import test_device_matching as DM
import test_idol_device_matching as IM
import test_mask_loss as ML
import test_mask_rle as MR
import test_reid_loss as RL
import test_set_loss as SL
import test_swin_glue as SG
from vnext_amd import _lib
from vnext_amd.utils.ytvis_json import rle_encode

DEV = "cuda:0"
INT_SENTINEL = 0x5A5A5A5A


# ---- the harness -----------------------------------------------------------------------------------------------------
def _poison(t):
    """NaN for floats, 0x5A5A5A5A for integers of four bytes or more, 0x5A for one-byte types"""
    if t.dtype.is_floating_point:
        t.fill_(float("nan"))
    elif t.dtype == torch.bool:
        t.fill_(True)
    else:
        t.fill_(INT_SENTINEL if t.element_size() >= 4 else 0x5A)


def _poison_left(t):
    """elements that still hold the poison.  One-byte results are not judged by their value (0x5A is 'Z', a legal
    character of an RLE string): for those the comparison with the eager call and the reference is the check."""
    if t.dtype.is_floating_point:
        return int(torch.isnan(t).sum())
    if t.element_size() >= 4:
        return int((t == INT_SENTINEL).sum())
    return 0


def assert_sets_differ(sets, refs, index_inputs):
    """A property of the inputs alone: every set has set 0's names, shapes and types (the static buffers keep their
    sizes), and set s differs from set 0 in every index input and in every output of the reference."""
    for name in index_inputs:
        assert name in sets[0], f"index input {name} is not an input"
    for s in range(1, len(sets)):
        assert list(sets[s]) == list(sets[0])
        for k, v in sets[0].items():
            w = sets[s][k]
            assert v.shape == w.shape and v.dtype == w.dtype, f"input {k} of set {s} does not fit set 0's buffer"
        for k in index_inputs:
            assert not torch.equal(sets[0][k], sets[s][k]), f"index input {k} is the same in set 0 and set {s}"
        assert list(refs[s]) == list(refs[0]) and len(refs[0]) > 0
        for k, v in refs[0].items():
            assert not torch.equal(torch.as_tensor(v), torch.as_tensor(refs[s][k])), \
                f"reference output {k} is the same for set 0 and set {s}: a baked value would not show"


@functools.lru_cache(maxsize=None)
def side_stream():
    """ONE warm-up stream for every test of this file.  `torch.cuda.Stream()` hands out the 32 streams of a per-device
    pool in turn, so a stream per test would move every later test of the suite 25 places along that pool -- and with a
    stream per test tests/test_idol_model.py's graphed training trunk test, which runs later, did fail on a gradient
    ("Open")."""
    return torch.cuda.Stream()


def hip_graph_capture(run, static):
    """-> (static result buffers, replay): two eager calls on a side stream (they load code objects, fill the caches of
    constants and make the once-per-device hipFuncSetAttribute calls outside the capture), then one call captured with
    its results copied into buffers allocated before the capture.  A capture that raises leaves through the context
    manager, which ends it, and is followed by a synchronize."""
    current = torch.cuda.current_stream()
    side = side_stream()
    side.wait_stream(current)
    with torch.cuda.stream(side):
        for _ in range(2):
            out = run(static)
    current.wait_stream(side)
    torch.cuda.synchronize()
    results = {k: torch.empty(v.shape, dtype=v.dtype, device=v.device) for k, v in out.items()}
    del out
    graph = torch.cuda.CUDAGraph()
    try:
        with torch.cuda.graph(graph):
            for k, v in run(static).items():
                results[k].copy_(v)
    finally:
        torch.cuda.synchronize()

    def replay():
        graph.replay()
        torch.cuda.synchronize()
    return results, replay


def replay_check(make_inputs, run, reference, capture=hip_graph_capture, n_sets=2, *, check=None, index_inputs=(),
                 seeds=None, device=DEV):
    """make_inputs(seed) -> {name: CPU tensor}, every index input included; run({name: tensor on `device`}) -> {name:
    result tensor} (autograd ops: forward and backward under a static upstream gradient, outputs and input gradients);
    reference({name: CPU tensor}) -> {name: CPU tensor}, independent of `run`; check(got, ref, inputs) asserts the op's own
    bound (default: equality with the reference on the names they share); capture(run, static) -> (results, replay).
    See the module docstring for what is asserted."""
    seeds = list(range(n_sets + 1)) if seeds is None else list(seeds)
    assert len(seeds) == n_sets + 1 >= 2
    sets = [make_inputs(s) for s in seeds]
    refs = [reference(x) for x in sets]
    assert_sets_differ(sets, refs, index_inputs)
    static = {k: v.to(device).clone() for k, v in sets[0].items()}
    results, replay = capture(run, static)
    for s in range(1, n_sets + 1):
        for k, v in sets[s].items():
            static[k].copy_(v)
        for r in results.values():
            _poison(r)
        replay()
        got = {k: v.clone() for k, v in results.items()}
        left = {k: _poison_left(v) for k, v in got.items()}
        assert not any(left.values()), f"set {s}: the replay left poisoned elements {left}"
        eager = run({k: v.to(device).clone() for k, v in sets[s].items()})
        assert sorted(eager) == sorted(got)
        for k, v in eager.items():
            assert v.dtype == got[k].dtype and v.shape == got[k].shape, (s, k)
            assert torch.equal(v, got[k]), f"set {s}: replayed {k} is not the eager call's, bit for bit"
        if check is None:
            for k in refs[s]:
                assert torch.equal(got[k].cpu(), refs[s][k]), f"set {s}: {k} is not the reference's"
        else:
            check(got, refs[s], sets[s])


class Case:
    """one op at one shape: what `replay_check` takes.  The input sets and their references are made once per process
    and shared by the CPU test of the inputs and the GPU test; nothing modifies them."""

    def __init__(self, make_inputs, run, reference, check=None, index_inputs=(), seeds=(0, 1, 2)):
        self.make_inputs = functools.lru_cache(maxsize=None)(make_inputs)
        self.run, self.check, self.index_inputs, self.seeds = run, check, tuple(index_inputs), tuple(seeds)
        self._reference, self._refs = reference, {}

    def reference(self, inputs):
        if id(inputs) not in self._refs:            # the sets are kept by make_inputs' cache: the id names one for good
            self._refs[id(inputs)] = (inputs, self._reference(inputs))
        return self._refs[id(inputs)][1]

    def inputs_and_references(self):
        sets = [self.make_inputs(s) for s in self.seeds]
        return sets, [self.reference(x) for x in sets]

    def replay(self, **kw):
        replay_check(self.make_inputs, self.run, self.reference, n_sets=len(self.seeds) - 1, check=self.check,
                     index_inputs=self.index_inputs, seeds=self.seeds, **kw)


# ---- the harness on the CPU, with fake capturers ---------------------------------------------------------------------
def _toy_inputs(seed):
    g = torch.Generator().manual_seed(seed)
    return {"x": torch.randn(16, generator=g), "idx": torch.randperm(16, generator=g)[:5]}


def _toy_run(t):
    return {"picked": t["x"][t["idx"]] * 2, "next": t["idx"] + 1}


def _toy_reference(t):
    return {"picked": (t["x"].double()[t["idx"]] * 2).float(), "next": t["idx"] + 1}      # a doubling is exact


def _toy_check(got, ref, inputs):
    assert torch.equal(got["picked"], ref["picked"]) and torch.equal(got["next"], ref["next"])


def _results_like(run, static):
    return {k: torch.empty_like(v) for k, v in run(static).items()}


def honest_capture(run, static):
    results = _results_like(run, static)

    def replay():
        for k, v in run(static).items():
            results[k].copy_(v)
    return results, replay


def baking_capture(run, static):
    """what a graph that baked its inputs' values would do: every replay returns what the capture computed"""
    recorded = {k: v.clone() for k, v in run(static).items()}
    results = _results_like(run, static)

    def replay():
        for k, v in recorded.items():
            results[k].copy_(v)
    return results, replay


def noop_capture(run, static):
    return _results_like(run, static), lambda: None


def stale_input_capture(name):
    """a replay that reads every input where it is, except `name`: that one as the host saw it at capture"""
    def capture(run, static):
        held = static[name].clone()
        results = _results_like(run, static)

        def replay():
            for k, v in run({**static, name: held}).items():
                results[k].copy_(v)
        return results, replay
    return capture


def _toy(capture, **kw):
    args = dict(check=_toy_check, index_inputs=("idx",), device="cpu")
    args.update(kw)
    replay_check(_toy_inputs, _toy_run, _toy_reference, capture=capture, **args)


def test_the_harness_passes_an_honest_replay():
    _toy(honest_capture)
    _toy(honest_capture, check=None, n_sets=3)


@pytest.mark.parametrize("fake, message", [(baking_capture, "bit for bit"), (noop_capture, "poisoned"),
                                           (stale_input_capture("idx"), "bit for bit"),
                                           (stale_input_capture("x"), "bit for bit")])
def test_the_harness_catches_a_replay_that_does_not_read_its_inputs(fake, message):
    with pytest.raises(AssertionError, match=message):
        _toy(fake)


def test_the_harness_catches_a_wrong_result_that_replays_faithfully():
    """eager and replay agree, the reference does not: the second comparison is not implied by the first"""
    def wrong(t):
        return {"picked": t["x"][t["idx"]] * 2.5, "next": t["idx"] + 1}
    with pytest.raises(AssertionError):
        replay_check(_toy_inputs, wrong, _toy_reference, capture=honest_capture, check=_toy_check, index_inputs=("idx",),
                     device="cpu")
    with pytest.raises(AssertionError, match="reference's"):
        replay_check(_toy_inputs, wrong, _toy_reference, capture=honest_capture, index_inputs=("idx",), device="cpu")


def test_the_harness_refuses_input_sets_that_would_hide_a_baked_value():
    same_index = lambda seed: {**_toy_inputs(seed), "idx": torch.arange(5)}      # noqa: E731
    with pytest.raises(AssertionError, match="index input idx is the same"):
        replay_check(same_index, _toy_run, _toy_reference, capture=honest_capture, index_inputs=("idx",), device="cpu")
    with pytest.raises(AssertionError, match="reference output"):
        replay_check(lambda seed: _toy_inputs(0), _toy_run, _toy_reference, capture=honest_capture, device="cpu")
    grows = lambda seed: {"x": torch.randn(16 + seed), "idx": torch.arange(5) + seed}      # noqa: E731
    with pytest.raises(AssertionError, match="does not fit"):
        replay_check(grows, _toy_run, _toy_reference, capture=honest_capture, device="cpu")


def test_poison_is_seen_in_every_type_it_is_judged_in():
    for dtype in (torch.float32, torch.bfloat16, torch.float64, torch.int32, torch.int64):
        t = torch.zeros(7, dtype=dtype)
        assert _poison_left(t) == 0
        _poison(t)
        assert _poison_left(t) == 7, dtype
    assert int(torch.full((1,), INT_SENTINEL, dtype=torch.int32)[0]) == 0x5A5A5A5A


# ---- the ops ---------------------------------------------------------------------------------------------------------
def _lsap(maximize):
    """batch 3 of [300, 20] and a [5, 12] problem through the transposed view of a [12, 5] buffer.  Reference: scipy,
    under the gap rule of test_device_matching._check_assignment; the seeds leave no problem out (asserted)."""
    def make_inputs(seed):
        rng = np.random.default_rng(1000 + seed)
        return {"batch": torch.from_numpy(np.stack([DM._draw(rng, (300, 20), "normal") for _ in range(3)])),
                "tall": torch.from_numpy(DM._draw(rng, (12, 5), "normal"))}

    def problems(x):
        return list(x["batch"].numpy()) + [np.ascontiguousarray(x["tall"].numpy().T)]

    def run(x):
        from vnext_amd.ops.lsap import lsap_solve
        rows, cols = lsap_solve(x["batch"], maximize=maximize)
        wide = x["tall"].t()
        assert not wide.is_contiguous()
        wide_rows, wide_cols = lsap_solve(wide, maximize=maximize)
        return {"rows": rows, "cols": cols, "wide_rows": wide_rows, "wide_cols": wide_cols}

    def reference(x):
        sol = []
        for m in problems(x):
            r, c, gap = DM._gap(m.astype(np.float64), maximize)
            assert gap > 1e-9 * np.abs(m).max(), "the gap rule would leave this problem out: choose another seed"
            sol.append((torch.from_numpy(r), torch.from_numpy(c)))
        # the rows of the wide problem are 0 .. 4 whatever the costs: held by the check below, not a reference output
        return {"rows": torch.stack([r for r, _ in sol[:3]]), "cols": torch.stack([c for _, c in sol[:3]]),
                "wide_cols": sol[3][1]}

    def check(got, ref, x):
        rows, cols = got["rows"].cpu().numpy(), got["cols"].cpu().numpy()
        pairs = [(rows[i], cols[i]) for i in range(3)] + [(got["wide_rows"].cpu().numpy(), got["wide_cols"].cpu().numpy())]
        for (r, c), m in zip(pairs, problems(x)):
            assert DM._check_assignment(r, c, m, maximize)          # True: compared with scipy's indices, not left out
    return Case(make_inputs, run, reference, check)


SEQ_SHAPE = dict(Ld=2, N=2, T=2, Q=50, K=5)
SEQ_MAX_TARGETS = 5


def _seqformer_match():
    """Ld 2, N 2, T 2, Q 50, K 5, 3 + 4 targets; every later set has 2 + 5: the `offsets` buffer keeps its size and one
    target moves from clip 0 to clip 1.  Reference: HungarianMatcher.cost in float64 + scipy per (layer, clip); the
    leave-out rule of test_device_matching (gap <= 1e-4) leaves nothing out for these seeds (asserted)."""
    Ld, N, T, Q, K = (SEQ_SHAPE[k] for k in ("Ld", "N", "T", "Q", "K"))
    base = 0

    def make_inputs(seed):
        g = torch.Generator().manual_seed(2000 + seed)

        def rand_boxes(*lead):
            return torch.cat([0.2 + 0.6 * torch.rand(*lead, 2, generator=g), 0.05 + 0.3 * torch.rand(*lead, 2, generator=g)], -1)
        first = 3 if seed == base else 2
        return {"logits": torch.randn(Ld, N, Q, K, generator=g) - 2, "boxes": rand_boxes(Ld, N, T, Q),
                "labels": torch.randint(0, K, (7,), generator=g), "tgt_boxes": rand_boxes(7, T),
                "offsets": torch.tensor([0, first, 7], dtype=torch.int32)}

    def run(x):
        from vnext_amd.ops.lsap import seqformer_match
        w = DM.WEIGHTS
        qry, tgt = seqformer_match(x["logits"], x["boxes"], x["labels"], x["tgt_boxes"], x["offsets"],
                                   (w["cost_class"], w["cost_bbox"], w["cost_giou"]), max_targets=SEQ_MAX_TARGETS)
        return {"qry": qry, "tgt": tgt}

    def reference(x):
        start = x["offsets"].tolist()
        assert max(b - a for a, b in zip(start, start[1:])) <= SEQ_MAX_TARGETS
        targets = [{"labels": x["labels"][a:b], "boxes": x["tgt_boxes"][a:b].double()} for a, b in zip(start, start[1:])]
        cost = DM._matcher().cost(x["logits"].double(), x["boxes"].double(), targets).numpy()
        assert cost.dtype == np.float64
        qry, tgt = torch.empty(Ld, 7, dtype=torch.int64), torch.empty(Ld, 7, dtype=torch.int64)
        for l in range(Ld):
            for i, (a, b) in enumerate(zip(start, start[1:])):
                r, c, gap = DM._gap(cost[l, i, :, a:b])
                assert gap > 1e-4, "the leave-out rule would apply: choose another seed"
                qry[l, a:b], tgt[l, a:b] = torch.from_numpy(r), torch.from_numpy(c)
        return {"qry": qry, "tgt": tgt}
    return Case(make_inputs, run, reference, index_inputs=("labels", "offsets"))


def _mask_loss(w, sizes):
    """R 6, F 2, h 5, stride 4, two clips of 2 and 3 targets whose ground truth is overwritten in place in the SAME
    tensors (the launch holds their addresses).  Reference and bound: test_mask_loss's float64 expression and its rule,
    four times the measured error of the fp32 ATen composition on the device, floor 4 * 2^-23."""
    R, F, h, stride = 6, 2, 5, 4

    def make_inputs(seed):
        g = torch.Generator().manual_seed(3000 + seed)
        gts = [ML.blobs(n, F, H, W, g) for n, (H, W) in zip((2, 3), sizes)]
        return {"logits": torch.randn(R, F, h, w, generator=g) * 3, "gt0": gts[0], "gt1": gts[1],
                "row_gt": torch.randint(0, 5, (R,), generator=g), "wf": torch.rand(R, generator=g) + 0.5,
                "wd": torch.rand(R, generator=g) + 0.5}

    def call(fn, x, cast=lambda t: t):
        out = ML.run(fn, cast(x["logits"]), [x["gt0"], x["gt1"]], x["row_gt"], stride, cast(x["wf"]), cast(x["wd"]))
        return dict(zip(("focal", "dice", "grad_logits"), out))

    def check(got, ref, x):
        on_device = {k: v.to(DEV) for k, v in x.items()}
        order = ("focal", "dice", "grad_logits")
        want = tuple(ref[k] for k in order)
        aten = ML.errors(tuple(call(ML.compose, on_device)[k] for k in order), want)
        ours = ML.errors(tuple(got[k] for k in order), want)
        for k in ours:
            allowed = max(4 * aten[k], 4 * ML.EPS)                # test_mask_loss.test_op_against_float64's rule
            print(f"mask loss w={w} {k}: replayed {ours[k]:.3e}, ATen fp32 {aten[k]:.3e}, allowed {allowed:.3e}")
        for k in ours:
            assert ours[k] <= max(4 * aten[k], 4 * ML.EPS), (k, ours[k], aten[k])
    return Case(make_inputs, lambda x: call(ML.fused, x), lambda x: call(ML.compose, x, lambda t: t.double()), check,
                index_inputs=("row_gt", "gt0", "gt1"))


def _set_loss(K):
    """Ld 3, N 2, T 2, Q 40, 3 + 2 targets, every target once per layer (5 pairs per layer), the 15 pairs in a random
    order so that `lay` and `clip` differ from set to set as well.  Reference and bound: test_set_loss's."""
    names = ("logits", "boxes", "lay", "clip", "qry", "tgt", "labels", "tgt_boxes")

    def make_inputs(seed):
        case = SL.synthetic(3, 2, 2, 40, K, [3, 2], seed=4000 + seed)
        g = torch.Generator().manual_seed(4100 + seed)
        order = torch.randperm(15, generator=g)
        x = dict(zip(names, case[:8]))
        for k in ("lay", "clip", "qry", "tgt"):
            x[k] = x[k][order].contiguous()
        x["w"] = torch.rand(3, 3, generator=g) + 0.5
        return x

    def call(fn, x, **kw):
        out = SL.run(fn, tuple(x[k] for k in names) + ({},), x["w"], device=x["logits"].device, **kw)
        return dict(zip(("sums", "grad_logits", "grad_boxes"), out))

    def reference(x):
        y = dict(x, w=x["w"].double())
        return call(SL.compose, y, dtype=torch.float64)

    def check(got, ref, x):
        on_device = {k: v.to(DEV) for k, v in x.items()}
        order = ("sums", "grad_logits", "grad_boxes")
        want = tuple(ref[k] for k in order)
        aten = SL.errors(tuple(call(SL.compose, on_device)[k] for k in order), want)
        bad = SL.held(f"set loss K={K}", SL.errors(tuple(got[k] for k in order), want), aten)
        assert torch.equal(got["sums"][:, 3].cpu().double(), ref["sums"][:, 3])        # the hit counts: exact
        assert not bad, bad
    return Case(make_inputs, lambda x: call(SL.fused, x), reference, check,
                index_inputs=("lay", "clip", "qry", "tgt", "labels"))


def _reid_loss(C):
    """B 2, Q = R = 30, J 5 (2 + 3 instances, 3 + 2 in the later sets); key and ref are the embeds[0::2] / embeds[1::2]
    views of ONE static buffer, read in place.  Reference and bound: test_reid_loss's."""
    B, Q, base = 2, 30, 0

    def make_inputs(seed):
        key, ref, img, kq, flags = RL.synthetic(B, Q, Q, C, (2, 3) if seed == base else (3, 2), seed=5000 + seed)
        g = torch.Generator().manual_seed(5100 + seed)
        return {"embeds": torch.stack([key, ref], 1).flatten(0, 1).contiguous(), "img": img, "key_query": kq,
                "flags": flags, "w": torch.rand(5, 2, generator=g) + 0.5}

    def case_of(x):
        key, ref = x["embeds"][0::2], x["embeds"][1::2]
        assert key.data_ptr() == x["embeds"].data_ptr() and not key.is_contiguous()
        return key, ref, x["img"], x["key_query"], x["flags"]

    def run(x):
        return dict(zip(("out", "grad_key", "grad_ref"), RL.run_fused(case_of(x), x["w"], device=x["embeds"].device)))

    def reference(x):
        return dict(zip(("out", "grad_key", "grad_ref"), RL.run_yardstick(case_of(x), x["w"])))

    def check(got, ref, x):
        order = ("out", "grad_key", "grad_ref")
        want = tuple(ref[k] for k in order)
        unfused = RL.errors(RL.run_unfused(case_of(x), x["w"]), want, x["img"], B)
        bad = RL.held(f"reid loss C={C}", RL.errors(tuple(got[k] for k in order), want, x["img"], B), unfused)
        assert not bad, bad
    return Case(make_inputs, run, reference, check, index_inputs=("img", "key_query", "flags"))


def _layer_norm(gamma, beta):
    """an nn.LayerNorm whose parameters ARE the two static tensors; built without a launch (it is made inside the capture)"""
    norm = torch.nn.LayerNorm(gamma.shape[0], eps=SG.EPS, device="meta")
    norm.weight, norm.bias = torch.nn.Parameter(gamma), torch.nn.Parameter(beta)
    return norm


def _swin_residual(C, tname):
    """(3, 7, C) through ops/swin_glue.residual_norm, forward and backward, with a per-sample scale that drops one
    sample -- another one in every set.  Reference and bound: test_swin_glue's float64 chain, twice the measured error of
    the eager chain in the op's types, and FLOOR."""
    types = SG.TYPES[tname]
    tx, ta, tn = types
    B, L = 3, 7
    order = ("x", "a", "scale", "gamma", "beta", "gy", "gn")

    def make_inputs(seed):
        g = torch.Generator().manual_seed(6000 + 10 * C + seed)
        rnd = lambda *s: torch.randn(*s, generator=g)      # noqa: E731
        scale = torch.full((B,), 1 / SG.KEEP)
        scale[seed % B] = 0.0
        return {"x": (rnd(B, L, C) * 2 + 0.5).to(tx), "a": rnd(B, L, C).to(ta), "scale": scale, "gamma": 1 + 0.2 * rnd(C),
                "beta": 0.2 * rnd(C), "gy": rnd(B, L, C).to(tx), "gn": rnd(B, L, C).to(tn)}

    def run(t):
        norm = _layer_norm(t["gamma"], t["beta"])
        x, a = t["x"].detach().requires_grad_(True), t["a"].detach().requires_grad_(True)
        with torch.autocast("cuda", dtype=SG.BF16, enabled=tn == SG.BF16):
            assert SG.G.fused_applies(x, a, norm)            # the kernel, not the reference expression behind it
            y, n = SG.G.residual_norm(x, a, t["scale"], norm)
        gx, ga, gg, gb = torch.autograd.grad([y, n], [x, a, norm.weight, norm.bias], [t["gy"], t["gn"]])
        return dict(y=y.detach(), n=n.detach(), grad_x=gx, grad_a=ga, grad_gamma=gg, grad_beta=gb)

    def reference(t):
        wide = [t[k].double() if k != "scale" else t[k] for k in order]
        return {k: v.detach() for k, v in SG._chain(*wide, torch.float64).items()}

    def check(got, ref, t):
        chain = SG._chain(*(t[k].to(DEV) for k in order), tn)
        SG._assert_within_measured_tolerance(f"residual {tname} C={C}", got, chain, ref, types, {})
        dropped = int((t["scale"] == 0).nonzero())
        assert torch.equal(got["y"][dropped], t["x"][dropped].to(DEV)) and not bool(got["grad_a"][dropped].any())
    return Case(make_inputs, run, reference, check, index_inputs=("scale",))


def _swin_merge(tname):
    tx, _, tn = SG.TYPES[tname]
    B, H, W, C = 2, 5, 7, 32

    def make_inputs(seed):
        g = torch.Generator().manual_seed(6500 + seed)
        return {"x": (torch.randn(B, H * W, C, generator=g) * 2 + 0.5).to(tx), "gamma": 1 + 0.2 * torch.randn(4 * C, generator=g),
                "beta": 0.2 * torch.randn(4 * C, generator=g),
                "gn": torch.randn(B, ((H + 1) // 2) * ((W + 1) // 2), 4 * C, generator=g).to(tn)}

    def run(t):
        norm = _layer_norm(t["gamma"], t["beta"])
        x = t["x"].detach().requires_grad_(True)
        with torch.autocast("cuda", dtype=SG.BF16, enabled=tn == SG.BF16):
            assert SG.G.merge_applies(x, norm)
            n = SG.G.merge_norm(x, H, W, norm)
        gx, gg, gb = torch.autograd.grad(n, [x, norm.weight, norm.bias], t["gn"])
        return dict(n=n.detach(), grad_x=gx.view(B, H, W, C), grad_gamma=gg, grad_beta=gb)

    def reference(t):
        return SG._merge_reference(t["x"].view(B, H, W, C).double(), H, W, t["gamma"].double(), t["beta"].double(),
                                   t["gn"].double(), torch.float64)

    def check(got, ref, t):
        d = {k: v.to(DEV) for k, v in t.items()}
        chain = SG._merge_reference(d["x"].view(B, H, W, C), H, W, d["gamma"], d["beta"], d["gn"], tn)
        SG._assert_within_measured_tolerance(f"merge {tname}", got, chain, ref, (tx, tn, tn), {})
    return Case(make_inputs, run, reference, check)


RLE_POISON = 0xAB


def _mask_rle(mode):
    """vnx_mask_rle_measure -> torch.cumsum on the device -> vnx_mask_rle_write in ONE graph, the arena sized by the worst
    case (a run per pixel and one more, at most 7 characters each) and poisoned inside the graph.  Reference:
    utils/ytvis_json.rle_encode of the host expression's masks, byte for byte; bytes past the total stay untouched.
    LOGITS: 5 maps of 6 x 10, stride 4, crop 21 x 37 -> 30 x 50, no pixel within test_mask_rle.BAND of the threshold
    (asserted).  BINARY: 3 masks of 17 x 33."""
    if mode == "logits":
        M, h, w, s, ih, iw, oh, ow = 5, 6, 10, 4, 21, 37, 30, 50
        code = _lib.MASK_RLE_LOGITS
    else:
        M, h, w, s, ih, iw, oh, ow = 3, 0, 0, 0, 0, 0, 17, 33
        code = _lib.MASK_RLE_BINARY
    capacity = M * (oh * ow + 1) * 7

    def make_inputs(seed):
        if mode == "logits":
            return {"data": MR.blob_logits(M, h, w, seed=7000 + seed)}
        g = torch.Generator().manual_seed(7500 + seed)
        return {"data": (torch.rand(M, oh, ow, generator=g) > 0.5).to(torch.uint8)}

    def run(t):
        lib, data = _lib.lib(), t["data"]
        stream = _lib.current_stream(data)
        lengths = torch.empty(M, dtype=torch.int64, device=data.device)
        _lib.check(lib.vnx_mask_rle_measure(code, data.data_ptr(), M, h, w, s, ih, iw, oh, ow, lengths.data_ptr(), stream))
        ends = lengths.cumsum(0)
        arena = torch.full((capacity,), RLE_POISON, dtype=torch.uint8, device=data.device)
        _lib.check(lib.vnx_mask_rle_write(code, data.data_ptr(), M, h, w, s, ih, iw, oh, ow, (ends - lengths).data_ptr(),
                                          arena.data_ptr(), capacity, stream))
        return {"lengths": lengths, "arena": arena}

    def reference(t):
        if mode == "logits":
            assert not (np.abs(MR.bilinear_f64(t["data"], s, (ih, iw), (oh, ow))) < MR.BAND).any(), \
                "a pixel sits in the band where the device bit may differ: choose another seed"
            masks = MR.host_expression(t["data"], s, (ih, iw), (oh, ow)).numpy()
        else:
            masks = t["data"].numpy() != 0
        strings = [rle_encode(m)["counts"].encode("ascii") for m in masks]
        assert sum(map(len, strings)) <= capacity
        return {"lengths": torch.tensor([len(x) for x in strings]),
                "arena": torch.frombuffer(bytearray(b"".join(strings)), dtype=torch.uint8)}

    def check(got, ref, t):
        arena, total = got["arena"].cpu(), int(ref["lengths"].sum())
        assert torch.equal(got["lengths"].cpu(), ref["lengths"])
        assert torch.equal(arena[:total], ref["arena"])
        assert bool((arena[total:] == RLE_POISON).all())
    return Case(make_inputs, run, reference, check)


def _det_select(B, Q, K, mode, seeds):
    """test_det_select's inputs and host expression; the seeds are those for which no image of any set is `fragile`
    (asserted).  The whole int32 result -- status, counts, kept list, labels, top-k pairs, -1 fill -- is compared."""
    iou_thr, score_thr, topk = (0.7, None, 100) if mode == "coco" else (0.9, 0.1, None)

    def make_inputs(seed):
        logits, boxes = DT.make_inputs(seed, B, Q, K, iou_thr)
        return {"logits": logits, "boxes": boxes}

    def run(t):
        return {"out": DT.DS.det_select_raw(t["logits"], t["boxes"], -1.0 if score_thr is None else score_thr, iou_thr,
                                            topk or 0)}

    def reference(t):
        for b in range(B):
            assert not DT.fragile(t["logits"][b], t["boxes"][b], iou_thr, score_thr, topk), \
                f"image {b}: an fp32 rounding decides the host expression: choose another seed"
        want = DT.DS.select_detections_host(t["logits"], t["boxes"], iou_thr=iou_thr, score_thr=score_thr, topk=topk)
        out = np.full((B, 4 + 2 * Q + 2 * (topk or 0)), -1, dtype=np.int32)
        for b in range(B):
            n = len(want.kept[b])
            out[b, :4] = (0, n, len(want.topk[b]) if topk else 0, 0)
            out[b, 4:4 + n] = want.kept[b]
            out[b, 4 + Q:4 + 2 * Q] = want.labels[b]
            if topk:
                out[b, 4 + 2 * Q:4 + 2 * Q + 2 * len(want.topk[b])] = want.topk[b].reshape(-1)
        return {"out": torch.from_numpy(out)}
    return Case(make_inputs, run, reference, seeds=seeds)


OTA_Q, OTA_K = 300, 40


def _ota_boxes(n, g, lo=0.1, span=0.3):
    return torch.cat([0.2 + 0.6 * torch.rand(n, 2, generator=g), lo + span * torch.rand(n, 2, generator=g)], -1)


def _ota_predictions(targets, near, g, spread):
    """[Q, K] class probabilities and [Q, 4] boxes, `near` queries placed on every target (test_idol_device_matching's recipe)"""
    boxes = _ota_boxes(OTA_Q, g)
    n = len(targets)
    for r in range(near):
        boxes[r * n:(r + 1) * n] = (targets + spread * (r + 1) * torch.randn(n, 4, generator=g)).clamp(0.02, 0.98)
    return (torch.randn(OTA_Q, OTA_K, generator=g) - 2).sigmoid(), boxes


def _ota_run(targets_max, with_selection):
    def run(t):
        from vnext_amd.ops.ota_match import idol_match
        kw = dict(ref_prob=t["ref_prob"], ref_boxes=t["ref_boxes"], valid=t["valid"],
                  valid_first=int(t["labels"].shape[0]) - int(t["valid"].shape[0])) if with_selection else {}
        return {"out": idol_match(t["det_prob"], t["det_boxes"], t["target_boxes"], t["labels"], t["problems"], targets_max, **kw)}
    return run


def _ota_reference(t):
    """the host matcher as test_idol_device_matching restates it, with its margins: no problem of these seeds is within
    them (asserted), so every problem is compared"""
    ref = {}
    problems = t["problems"].tolist()
    for p in range(t["det_prob"].shape[0]):
        first, n = problems[p]
        selected, gt, matched, fragile, _ = IM._restated_one(t["det_boxes"][p], t["det_prob"][p], t["target_boxes"][first:first + n],
                                                             t["labels"][first:first + n])
        assert not fragile, f"detection problem {p} is within the host matcher's margins: choose another seed"
        ref.update({f"det{p}.selected": torch.from_numpy(selected), f"det{p}.gt": torch.from_numpy(gt),
                    f"det{p}.matched": torch.from_numpy(matched)})
    if "ref_prob" in t:
        first, n = problems[-1]
        v = t["valid"]
        pos, neg, fragile = IM._restated_selection(t["ref_boxes"][0], t["ref_prob"][0], t["target_boxes"][first:first + n][v],
                                                   t["labels"][first:first + n][v])
        assert not fragile, "the selection problem is within the host matcher's margins: choose another seed"
        ref.update({"sel.inst": torch.nonzero(v).flatten(), "sel.pos": torch.from_numpy(pos), "sel.neg": torch.from_numpy(neg)})
    return ref


def _ota_check(targets_max):
    def check(got, ref, t):
        from vnext_amd.ops.ota_match import unpack
        Pd = t["det_prob"].shape[0]
        status, det, sel = unpack(got["out"].cpu(), Pd, OTA_Q, targets_max)
        assert not bool(status.any())
        for p, (selected, gt, matched) in enumerate(det):
            assert torch.equal(selected, ref[f"det{p}.selected"]) and torch.equal(gt, ref[f"det{p}.gt"])
            assert torch.equal(matched, ref[f"det{p}.matched"])
        assert len(sel) == ("ref_prob" in t)
        for inst, pos, neg in sel:
            assert torch.equal(inst, ref["sel.inst"]) and torch.equal(pos, ref["sel.pos"]) and torch.equal(neg, ref["sel.neg"])
    return check


def _ota_small(seeds):
    """2 detection problems and 1 selection problem at Q 300, targets_max 6: 4 + 6 key targets (6 + 4 in the later sets,
    so `problems` changes and the buffers keep their sizes) and 5 reference targets, one of them invalid"""
    base = seeds[0]

    def make_inputs(seed):
        g = torch.Generator().manual_seed(8000 + seed)
        counts = (4, 6) if seed == base else (6, 4)
        tb = _ota_boxes(15, g)
        tb[10:] = (tb[:5] + 0.03 * torch.randn(5, 4, generator=g)).clamp(0.02, 0.98)
        valid = torch.ones(5, dtype=torch.bool)
        valid[(seed - base) % 5] = False
        det = [_ota_predictions(tb[a:a + n], 4, g, 0.02) for a, n in ((0, counts[0]), (counts[0], counts[1]))]
        ref_prob, ref_boxes = _ota_predictions(tb[10:], 4, g, 0.02)
        return {"det_prob": torch.stack([p for p, _ in det]), "det_boxes": torch.stack([b for _, b in det]),
                "ref_prob": ref_prob[None], "ref_boxes": ref_boxes[None], "target_boxes": tb,
                "labels": torch.randint(0, OTA_K, (15,), generator=g), "valid": valid,
                "problems": torch.tensor([[0, counts[0]], [counts[0], counts[1]], [10, 5]], dtype=torch.int32)}
    return Case(make_inputs, _ota_run(6, True), _ota_reference, _ota_check(6),
                index_inputs=("labels", "valid", "problems"), seeds=seeds)


def _ota_big(seeds):
    """one detection problem of 41 targets at Q 300: the dynamic LDS goes above 64 KB (test_idol_device_matching.
    _header_lds_bytes), so the first call on the device -- the harness's eager warm-up -- raises the kernel's limit outside
    the capture, as the header asks.  45 targets in the buffer, the problem's first target moves from set to set."""
    n, base = 41, seeds[0]
    assert IM._header_lds_bytes(n, OTA_Q) > 64 * 1024 >= IM._header_lds_bytes(n - 1, OTA_Q)

    def make_inputs(seed):
        g = torch.Generator().manual_seed(9000 + seed)
        first = (seed - base) % 5
        tb = torch.cat([0.1 + 0.8 * torch.rand(n + 4, 2, generator=g), 0.05 + 0.1 * torch.rand(n + 4, 2, generator=g)], -1)
        prob, boxes = _ota_predictions(tb[first:first + n], 2, g, 0.005)
        return {"det_prob": prob[None], "det_boxes": boxes[None], "target_boxes": tb,
                "labels": torch.randint(0, OTA_K, (n + 4,), generator=g),
                "problems": torch.tensor([[first, n]], dtype=torch.int32)}
    return Case(make_inputs, _ota_run(n, False), _ota_reference, _ota_check(n), index_inputs=("labels", "problems"), seeds=seeds)


# The seeds of the selection and matching cases are listed after the table.  Seeds 0, 1, 2 happen to sit on none of the host
# expressions' own margins; if a recipe changes and one does, the CPU test below fails with "choose another seed".
CASES = {
    "lsap_min": lambda: _lsap(False),
    "lsap_max": lambda: _lsap(True),
    "seqformer_match": _seqformer_match,
    "mask_loss_w8": lambda: _mask_loss(8, ((20, 32), (19, 30))),       # 16-byte ground-truth path and byte path
    "mask_loss_w7": lambda: _mask_loss(7, ((20, 28), (19, 26))),       # the element-per-lane path of the logits
    "set_loss_K4": lambda: _set_loss(4),                               # vector rows
    "set_loss_K3": lambda: _set_loss(3),                               # scalar rows
    "reid_loss_C64": lambda: _reid_loss(64),
    "reid_loss_C10": lambda: _reid_loss(10),
    **{f"swin_residual_C{C}_{t}": (lambda C=C, t=t: _swin_residual(C, t)) for C in (32, 200, 1536) for t in ("fp32", "amp_stage1")},
    "swin_merge_fp32": lambda: _swin_merge("fp32"),
    "swin_merge_amp_stage1": lambda: _swin_merge("amp_stage1"),
    "mask_rle_logits": lambda: _mask_rle("logits"),
    "mask_rle_binary": lambda: _mask_rle("binary"),
    "det_select_coco_4x65x3": lambda: _det_select(4, 65, 3, "coco", DET_SEEDS["coco_4x65x3"]),
    "det_select_video_4x65x3": lambda: _det_select(4, 65, 3, "video", DET_SEEDS["video_4x65x3"]),
    "det_select_coco_1x1024x8": lambda: _det_select(1, 1024, 8, "coco", DET_SEEDS["coco_1x1024x8"]),      # LDS above 64 KB
    "idol_match_targets_max_6": lambda: _ota_small(OTA_SEEDS["small"]),
    "idol_match_targets_max_41": lambda: _ota_big(OTA_SEEDS["big"]),                                     # LDS above 64 KB
}
DET_SEEDS = {"coco_4x65x3": (0, 1, 2), "video_4x65x3": (0, 1, 2), "coco_1x1024x8": (0, 1, 2)}
OTA_SEEDS = {"small": (0, 1, 2), "big": (0, 1, 2)}


@functools.lru_cache(maxsize=None)
def case(name):
    return CASES[name]()


def _names(prefix):
    return [n for n in CASES if n.startswith(prefix)]


@pytest.mark.parametrize("name", list(CASES))
def test_the_input_sets_differ_and_sit_on_none_of_the_references_margins(name):
    """On the CPU, for every op: set s differs from set 0 in every index input and every reference output, and the
    reference's own leave-out rule (scipy's gap, `fragile`, the host matcher's margins, the RLE band) leaves out nothing
    -- the references assert that where they are made."""
    c = case(name)
    sets, refs = c.inputs_and_references()
    assert len(sets) == 3
    assert_sets_differ(sets, refs, c.index_inputs)
    for x in sets:
        assert all(not v.is_cuda for v in x.values())


@pytest.mark.gpu
@pytest.mark.parametrize("name", _names("lsap"))
def test_lsap_solve_replays_on_the_costs_in_memory(name):
    case(name).replay()


@pytest.mark.gpu
def test_seqformer_match_replays_on_the_targets_and_offsets_in_memory():
    case("seqformer_match").replay()


@pytest.mark.gpu
@pytest.mark.parametrize("name", _names("mask_loss"))
def test_mask_focal_dice_replays_on_the_ground_truth_in_memory(name):
    case(name).replay()


@pytest.mark.gpu
@pytest.mark.parametrize("name", _names("set_loss"))
def test_set_class_box_losses_replay_on_the_pair_list_in_memory(name):
    case(name).replay()


@pytest.mark.gpu
@pytest.mark.parametrize("name", _names("reid_loss"))
def test_reid_contrastive_losses_replay_on_the_instance_list_in_memory(name):
    case(name).replay()


@pytest.mark.gpu
@pytest.mark.parametrize("name", _names("swin_residual"))
def test_swin_residual_norm_replays_on_the_scale_in_memory(name):
    case(name).replay()


@pytest.mark.gpu
@pytest.mark.parametrize("name", _names("swin_merge"))
def test_swin_merge_norm_replays(name):
    case(name).replay()


@pytest.mark.gpu
@pytest.mark.parametrize("name", _names("mask_rle"))
def test_mask_rle_measure_scan_and_write_replay_as_one_graph(name):
    case(name).replay()


@pytest.mark.gpu
@pytest.mark.parametrize("name", _names("det_select"))
def test_det_select_replays_on_the_logits_and_boxes_in_memory(name):
    case(name).replay()


@pytest.mark.gpu
@pytest.mark.parametrize("name", _names("idol_match"))
def test_idol_match_replays_on_the_problem_table_in_memory(name):
    case(name).replay()


def test_every_case_is_run_by_one_gpu_test():
    prefixes = ("lsap", "seqformer_match", "mask_loss", "set_loss", "reid_loss", "swin_residual", "swin_merge", "mask_rle",
                "det_select", "idol_match")
    assert sorted(n for p in prefixes for n in _names(p)) == sorted(CASES)


# ---- the capstone: SeqFormer's loss stage as one graph -------------------------------------------------------------------
SPREAD_MULTIPLE = 4


@pytest.mark.gpu
def test_seqformer_loss_stage_replays_on_the_trunk_outputs_in_memory():
    """test_device_matching's model fixture made small (2 decoder layers, 12 queries, a 2-frame 96 x 160 clip, dropout 0)
    with device matching and the fused mask and set losses on: `_losses_after_trunk` is warmed once, captured under
    no_grad with the trunk outputs in static buffers, the buffers are overwritten with the trunk outputs of other frames
    (the targets stay), and the replayed loss dict must equal the eager call on the same tensors.  The equality is
    torch.equal when two eager calls on identical tensors are torch.equal here (checked first); if they are not, the bound
    is SPREAD_MULTIPLE times their measured difference.  Measured on an MI355X: see DESIGN.md."""
    import vnext_amd.models  # noqa: F401
    from vnext_amd import train
    from vnext_amd.registry import build_model, get_seqformer_cfg
    tiny = {"MODEL.SeqFormer.ENC_LAYERS": 1, "MODEL.SeqFormer.DEC_LAYERS": 2, "MODEL.SeqFormer.NUM_OBJECT_QUERIES": 12,
            "MODEL.SeqFormer.DIM_FEEDFORWARD": 64, "MODEL.SeqFormer.DROPOUT": 0.0, "INPUT.SAMPLING_FRAME_NUM": 2}
    torch.manual_seed(0)
    model = build_model(get_seqformer_cfg(**{"MODEL.DEVICE": DEV, **tiny})).train()
    with torch.no_grad():          # a fresh model's box heads end in zero weights: its boxes would not follow the frames
        for head in model.detr.detr.bbox_embed:
            head.layers[-1].weight.normal_(0, 0.02)
    train.enable_device_matching(model)
    train.enable_fused_mask_loss(model)
    train.enable_fused_set_loss(model)
    clips = train.synthetic_clips(1, 2, 96, 160, DEV, seed=100, num_instances=4)
    other = train.synthetic_clips(1, 2, 96, 160, DEV, seed=101, num_instances=4)

    def flat(trunk):
        hs, logits, boxes, refs, feats = trunk
        return [hs, logits, boxes, *refs, feats]

    def stage(tensors):
        hs, logits, boxes, *refs, feats = tensors
        return model._losses_after_trunk(targets, hs, logits, boxes, refs, feats)

    with torch.no_grad():
        targets = model.prepare_targets(clips)
        static = [t.detach().clone() for t in flat(DM._trunk(model, clips))]
        fresh = [t.detach().clone() for t in flat(DM._trunk(model, other))]
        assert all(a.shape == b.shape for a, b in zip(static, fresh))
        # hs, logits, boxes and the mask features follow the frames (the first layer's reference points are the queries' own)
        same = [name for name, i in (("hs", 0), ("logits", 1), ("boxes", 2), ("feats", -1)) if torch.equal(static[i], fresh[i])]
        assert not same, f"{same} are the same for both clips: a baked value would not show"
        side = side_stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            warm = stage(static)                          # fills the caches of constants outside the capture
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        results = {k: torch.empty_like(v) for k, v in warm.items()}
        graph = torch.cuda.CUDAGraph()
        try:
            with torch.cuda.graph(graph):
                for k, v in stage(static).items():
                    results[k].copy_(v)
        finally:
            torch.cuda.synchronize()
        for a, b in zip(static, fresh):
            a.copy_(b)
        for r in results.values():
            _poison(r)
        graph.replay()
        torch.cuda.synchronize()
        got = {k: v.clone() for k, v in results.items()}
        one, two = stage([t.clone() for t in fresh]), stage([t.clone() for t in fresh])
        torch.cuda.synchronize()
    assert set(got) == set(one) == set(warm) and len(got) == 5 * 2 + 1
    spread = {k: float((one[k] - two[k]).abs().max()) for k in one}
    exact = all(torch.equal(one[k], two[k]) for k in one)
    print(f"loss stage: eager against eager on identical tensors: bit-identical {exact}, largest difference {max(spread.values()):.3e}")
    for k in sorted(got):
        assert bool(torch.isfinite(got[k])), k
        if k.startswith("loss_"):                     # (class_error is a count of hits: it may well stay)
            assert not torch.equal(one[k], warm[k]), f"{k} does not change with the trunk outputs: a baked value would not show"
        diff, bound = float((got[k] - one[k]).abs().max()), SPREAD_MULTIPLE * spread[k]
        print(f"loss stage {k}: replay {float(got[k]):.9g}, eager {float(one[k]):.9g}, difference {diff:.3e}, bound {bound:.3e}")
        if exact:
            assert torch.equal(got[k], one[k]), k
        else:
            assert diff <= bound, (k, diff, bound)
