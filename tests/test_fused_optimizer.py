"""`vnext_amd.ops.optim.ClippedAdamW`: gradient-norm clipping and the AdamW update as one op (vnext_amd/csrc/optim.hip).

CPU: the chunk plan, the arena layout, state dicts in both directions with `torch.optim.AdamW`, what raises, the ABI.
GPU: three steps against the same steps in float64, measured against the eager chain (clip_grad_norm_ + single-tensor
AdamW in fp32 on the device) rather than a fixed tolerance -- per tensor
    max|op - f64| <= 2 * max|eager - f64| + ulp32(max|f64|)
(two correct fp32 orderings of the expression differ from each other by about as much as each differs from float64; the
one-ulp floor covers tensors where the eager chain happens to round exactly) -- then skipped tensors, alignment and
strides with guard elements, determinism, non-finite gradients, no synchronisation, the launch count, and a checkpoint
that crosses to a stock AdamW on the device."""
import copy
import math
import os
import re
import time

import numpy as np
import pytest
import torch

from conftest import ROOT
from vnext_amd import _lib
from vnext_amd.ops import optim
from vnext_amd.ops.optim import ClippedAdamW

C = _lib.OPT_CHUNK
DEV = "cuda:0"
MAX_NORM = 0.01
GROUPS = ({"lr": 1e-3, "weight_decay": 1e-2}, {"lr": 3e-4, "weight_decay": 1e-1})
BETAS, EPS = (0.9, 0.999), 1e-8
GUARD = 12345.678


# ---- CPU ---------------------------------------------------------------------------------------------------------------------
def test_chunk_plan_covers_every_element_once_and_no_chunk_crosses_a_tensor():
    counts = [1, 3, C - 1, C, C + 1, 2 * C + 7]
    plan = optim.chunk_plan(counts)
    assert plan.dtype == np.int64 and plan.shape == (1 + 1 + 1 + 1 + 2 + 3, 2)
    seen = [np.zeros(n, dtype=np.int64) for n in counts]
    for t, off in plan.tolist():
        assert 0 <= t < len(counts) and 0 <= off < counts[t] and off % C == 0      # inside its tensor, at a chunk boundary
        seen[t][off:min(off + C, counts[t])] += 1                                   # ... and cut at the tensor's end
    for s in seen:
        assert (s == 1).all()
    assert (np.diff(plan[:, 0]) >= 0).all()
    assert optim.chunk_plan([0, 5, 0]).tolist() == [[1, 0]]
    assert optim.chunk_plan([]).shape == (0, 2)


def _cpu_params(counts=(1, 3, 5, 257)):
    g = torch.Generator().manual_seed(0)
    return [torch.nn.Parameter(torch.randn(n, generator=g)) for n in counts]


def test_arena_slices_are_16_byte_aligned_and_apart():
    counts = [1, 3, 4, 5, 257, C + 1]
    offsets, total = optim.arena_layout(counts)
    assert (offsets % 4 == 0).all() and offsets[0] >= 1
    ends = offsets + np.asarray(counts)
    assert (offsets[1:] > ends[:-1]).all() and total > ends[-1]      # an unused element between two slices and after the last
    params = _cpu_params(counts)
    opt = ClippedAdamW(params, lr=1e-3)
    assert opt.exp_avg_arena.data_ptr() % 16 == 0 and opt.exp_avg_sq_arena.data_ptr() % 16 == 0
    for p, n in zip(params, counts):
        st = opt.state[p]
        for key, arena in (("exp_avg", opt.exp_avg_arena), ("exp_avg_sq", opt.exp_avg_sq_arena)):
            assert st[key].data_ptr() % 16 == 0 and st[key].shape == p.shape and st[key].stride() == p.stride()
            assert arena.data_ptr() <= st[key].data_ptr() < arena.data_ptr() + 4 * arena.numel()
        assert st["step"].dim() == 0 and not st["step"].is_cuda and float(st["step"]) == 0.0


def _fill(opt, params, seed):
    g = torch.Generator().manual_seed(seed)
    for i, p in enumerate(params):
        st = opt.state[p]
        if "exp_avg" not in st:      # a stock optimizer creates its state at the first step
            st["step"] = torch.tensor(0.0)
            st["exp_avg"], st["exp_avg_sq"] = torch.zeros_like(p), torch.zeros_like(p)
        st["exp_avg"].copy_(torch.randn(p.shape, generator=g))
        st["exp_avg_sq"].copy_(torch.rand(p.shape, generator=g))
        st["step"].fill_(float(3 + i))


def test_state_dict_round_trip_with_a_stock_adamw_on_the_cpu():
    mine_p, stock_p = _cpu_params(), _cpu_params()
    groups = lambda ps: [{"params": ps[:2], "lr": 1e-3}, {"params": ps[2:], "lr": 5e-4, "weight_decay": 0.1}]
    mine, stock = ClippedAdamW(groups(mine_p), lr=1e-3), torch.optim.AdamW(groups(stock_p), lr=1e-3)
    assert set(mine.param_groups[0]) == set(stock.param_groups[0])      # the same keys: a group crosses in both directions
    # this one's state dict loads into a stock AdamW
    _fill(mine, mine_p, seed=1)
    sd = copy.deepcopy(mine.state_dict())
    assert set(sd) == {"state", "param_groups"} and set(sd["state"][0]) == {"step", "exp_avg", "exp_avg_sq"}
    stock.load_state_dict(sd)
    for a, b in zip(mine_p, stock_p):
        for key in ("exp_avg", "exp_avg_sq", "step"):
            assert torch.equal(mine.state[a][key], stock.state[b][key]), key
    assert stock.param_groups[1]["lr"] == 5e-4 and stock.param_groups[1]["weight_decay"] == 0.1
    for p in stock_p:      # ... and the stock optimizer steps on it
        p.grad = torch.ones_like(p)
    stock.step()
    assert float(stock.state[stock_p[0]]["step"]) == 4.0
    # a stock AdamW's state dict loads into this one: copied INTO the arenas, the views stay
    _fill(stock, stock_p, seed=2)
    stock.param_groups[0]["lr"] = 7e-4
    before = {p: {k: v.data_ptr() for k, v in mine.state[p].items()} for p in mine_p}
    mine.load_state_dict(copy.deepcopy(stock.state_dict()))
    lo, hi = mine.exp_avg_arena.data_ptr(), mine.exp_avg_arena.data_ptr() + 4 * mine.exp_avg_arena.numel()
    for a, b in zip(mine_p, stock_p):
        for key in ("exp_avg", "exp_avg_sq", "step"):
            assert torch.equal(mine.state[a][key], stock.state[b][key]), key
            assert mine.state[a][key].data_ptr() == before[a][key], key      # still the arena's memory
        assert lo <= mine.state[a]["exp_avg"].data_ptr() < hi
    assert mine.param_groups[0]["lr"] == 7e-4
    # a parameter the loaded dict has no state for starts from zero
    fresh = torch.optim.AdamW(groups(_cpu_params()), lr=1e-3)
    mine.load_state_dict(fresh.state_dict())
    assert float(mine.exp_avg_arena.abs().sum()) == 0.0 and float(mine.state[mine_p[0]]["step"]) == 0.0


def test_unsupported_options_raise_and_name_the_cause():
    with pytest.raises(ValueError, match="amsgrad"):
        ClippedAdamW(_cpu_params(), lr=1e-3, amsgrad=True)
    with pytest.raises(ValueError, match="maximize"):
        ClippedAdamW(_cpu_params(), lr=1e-3, maximize=True)
    with pytest.raises(ValueError, match="capturable"):
        ClippedAdamW(_cpu_params(), lr=1e-3, capturable=True)
    with pytest.raises(ValueError, match="bfloat16"):
        ClippedAdamW([torch.nn.Parameter(torch.zeros(4, dtype=torch.bfloat16))], lr=1e-3)
    stock = torch.optim.AdamW(_cpu_params(), lr=1e-3, amsgrad=True)
    with pytest.raises(ValueError, match="amsgrad"):
        ClippedAdamW(_cpu_params(), lr=1e-3).load_state_dict(stock.state_dict())


def test_step_on_cpu_parameters_raises():
    params = _cpu_params()
    opt = ClippedAdamW(params, lr=1e-3)
    for p in params:
        p.grad = torch.ones_like(p)
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        opt.step()
    assert ClippedAdamW.clips_gradients is True


def test_the_new_symbols_are_declared_and_bound_and_the_abi_version_stays():
    header = open(os.path.join(ROOT, "include", "vnext_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in ("vnx_adamw_grad_norm", "vnx_adamw_clipped_step"):
        assert re.search(r"\bint\s+%s\s*\(" % name, code), name
        assert name in _lib.SIGNATURES
        assert hasattr(_lib.lib(), name)
    assert _lib.ABI_VERSION == 17 and re.search(r"#define\s+VNX_ABI_VERSION\s+17\b", code)
    assert int(re.search(r"#define\s+VNX_ADAMW_CHUNK\s+(\d+)", code).group(1)) == _lib.OPT_CHUNK
    assert int(re.search(r"#define\s+VNX_ADAMW_UNALIGNED\s+(\d+)", code).group(1)) == _lib.ADAMW_UNALIGNED


# ---- GPU: three steps against float64 ---------------------------------------------------------------------------------------
# a tensor of the scenario: (shape, elements before it in its storage, channels-last strides)
MAIN = [((n,), 4, False) for n in (1, 3, 4, 5, 257, C - 1, C, C + 1, 2 * C + 7)]
# a view that starts ONE element into its storage, odd count (the 4-byte path); a 4-D weight in channels-last strides whose
# gradient arrives in contiguous strides (the stride-fix copy)
EXTRA = MAIN + [((C + 3,), 1, False), ((6, 5, 3, 3), 4, True)]
STEPS = 3


def _numel(shape):
    return int(np.prod(shape))


def _inputs(specs, seed):
    """CPU fp32: the initial parameters and the gradients of three steps.  Steps 1 and 3: total norm ~1.5 (150 x max_norm:
    coef < 1); step 2: the same draw scaled by 1e-3, total norm ~1.5e-3 (coef == 1 exactly)."""
    g = torch.Generator().manual_seed(seed)
    p0 = [torch.randn(shape, generator=g) for shape, _, _ in specs]
    grads = [[torch.randn(shape, generator=g) * (1e-2 * (1e-3 if step == 1 else 1.0)) for shape, _, _ in specs]
             for step in range(STEPS)]
    return p0, grads


def _group_of(i):
    return i % 2


def _lr_at(step, gi):
    """between steps 2 and 3 group 1's lr is halved, as a scheduler would"""
    return GROUPS[gi]["lr"] * (0.5 if (step == 2 and gi == 1) else 1.0)


def _f64_steps(p0, grads, missing):
    """the three steps in float64 from the fp32 inputs: clip_grad_norm_'s formula, then the AdamW expression.
    missing: {(step, tensor)} without a gradient.  -> per step (p, m, v lists, total_norm, step counts)"""
    P = [p.double().clone() for p in p0]
    M, V = [torch.zeros_like(p) for p in P], [torch.zeros_like(p) for p in P]
    t, out = [0] * len(P), []
    for step in range(STEPS):
        G = [None if (step, i) in missing else grads[step][i].double() for i in range(len(P))]
        total = math.sqrt(sum(float((g * g).sum()) for g in G if g is not None))
        coef = min(1.0, MAX_NORM / (total + 1e-6))
        for i, g in enumerate(G):
            if g is None:
                continue
            gi = _group_of(i)
            lr, wd, (b1, b2) = _lr_at(step, gi), GROUPS[gi]["weight_decay"], BETAS
            t[i] += 1
            g = g * coef
            P[i] = P[i] * (1.0 - lr * wd)
            M[i] = M[i] + (1.0 - b1) * (g - M[i])
            V[i] = b2 * V[i] + (1.0 - b2) * g * g
            bc1, bc2 = 1.0 - b1 ** t[i], 1.0 - b2 ** t[i]
            P[i] = P[i] - (lr / bc1) * M[i] / (V[i].sqrt() / math.sqrt(bc2) + EPS)
        out.append(([x.clone() for x in P], [x.clone() for x in M], [x.clone() for x in V], total, list(t)))
    return out


def _device_param(value, lead, channels_last):
    """a leaf on the device whose storage has `lead` elements before it and 4 after, all holding GUARD"""
    n = value.numel()
    base = torch.full((lead + n + 4,), GUARD, dtype=torch.float32, device=DEV)
    stride = torch.empty(value.shape).to(memory_format=torch.channels_last).stride() if channels_last else \
        torch.empty(value.shape).stride()
    p = torch.as_strided(base, value.shape, stride, lead)
    p.copy_(value.to(DEV))
    return p.requires_grad_(), base


def _bits(t):
    return t.detach().contiguous().view(torch.int32).cpu()


def _make(kind, specs, p0):
    made = [_device_param(v, lead, cl) for v, (_, lead, cl) in zip(p0, specs)]
    params, bases = [m[0] for m in made], [m[1] for m in made]
    groups = [{"params": [p for i, p in enumerate(params) if _group_of(i) == gi], **GROUPS[gi]} for gi in (0, 1)]
    if kind == "op":
        opt = ClippedAdamW(groups, lr=1e-3, betas=BETAS, eps=EPS, max_norm=MAX_NORM)
    else:
        opt = torch.optim.AdamW(groups, lr=1e-3, betas=BETAS, eps=EPS, foreach=False, fused=False)
    return params, bases, opt


def _arena_gaps(opt):
    gap = torch.ones(opt.exp_avg_arena.numel(), dtype=torch.bool)
    for p, off in zip(opt._params, opt.arena_offsets.tolist()):
        gap[off:off + p.numel()] = False
    return gap.to(DEV)


def _device_steps(kind, specs, p0, grads, missing):
    """the three steps on the device with ClippedAdamW ("op") or clip_grad_norm_ + single-tensor AdamW ("eager")
    -> per step (p, m, v lists as float64 CPU tensors, total_norm, step counts), and what the guards hold afterwards"""
    params, bases, opt = _make(kind, specs, p0)
    if kind == "op":
        gap = _arena_gaps(opt)
        opt.exp_avg_arena[gap] = GUARD
        opt.exp_avg_sq_arena[gap] = GUARD
    out = []
    for step in range(STEPS):
        for gi in (0, 1):
            opt.param_groups[gi]["lr"] = _lr_at(step, gi)
        for i, p in enumerate(params):
            # a fresh, contiguous-strided gradient every step, as autograd makes them
            p.grad = None if (step, i) in missing else grads[step][i].to(DEV).contiguous()
        if kind == "op":
            total = opt.step()
        else:
            total = torch.nn.utils.clip_grad_norm_(params, MAX_NORM)
            opt.step()
        st = [opt.state[p] for p in params]
        zero = lambda p: torch.zeros(p.shape, dtype=torch.float64)
        out.append(([p.detach().cpu().double() for p in params],
                    [s["exp_avg"].cpu().double() if "exp_avg" in s else zero(p) for s, p in zip(st, params)],
                    [s["exp_avg_sq"].cpu().double() if "exp_avg_sq" in s else zero(p) for s, p in zip(st, params)],
                    float(total), [int(float(s["step"])) if "step" in s else 0 for s in st]))
    guards = {}
    if kind == "op":
        guards["p"] = [(_bits(b[:lead]), _bits(b[lead + _numel(shape):])) for b, (shape, lead, _) in zip(bases, specs)]
        guards["m"], guards["v"] = _bits(opt.exp_avg_arena[gap]), _bits(opt.exp_avg_sq_arena[gap])
    return out, guards


def ulp32(x):
    return float(np.spacing(np.float32(abs(x))))


def _hold(label, op, eager, ref):
    """the bound of the module docstring, on one tensor (or one number)"""
    op, eager, ref = (torch.as_tensor(x, dtype=torch.float64) for x in (op, eager, ref))
    e_op, e_eager = float((op - ref).abs().max()), float((eager - ref).abs().max())
    bound = 2.0 * e_eager + ulp32(float(ref.abs().max()))
    print(f"{label:34s} op {e_op:.3e}  eager {e_eager:.3e}  bound {bound:.3e}  max|f64| {float(ref.abs().max()):.3e}")
    return e_op <= bound, f"{label}: op {e_op:.3e} > 2 * eager {e_eager:.3e} + ulp = {bound:.3e}"


def _compare(runs, specs, steps=range(STEPS)):
    ref, op, eager = runs["f64"], runs["op"], runs["eager"]
    failures = []
    for step in steps:
        ok, msg = _hold(f"step {step + 1} total_norm", op[step][3], eager[step][3], ref[step][3])
        failures += [] if ok else [msg]
        for k, name in enumerate(("p", "m", "v")):
            for i, (shape, lead, cl) in enumerate(specs):
                ok, msg = _hold(f"step {step + 1} {name}[{i}] {tuple(shape)}", op[step][k][i], eager[step][k][i], ref[step][k][i])
                failures += [] if ok else [msg]
    assert not failures, "\n".join(failures)


@pytest.fixture(scope="module")
def plain():
    """every tensor has a gradient at every step"""
    p0, grads = _inputs(MAIN, seed=11)
    op, guards = _device_steps("op", MAIN, p0, grads, set())
    eager, _ = _device_steps("eager", MAIN, p0, grads, set())
    return {"f64": _f64_steps(p0, grads, set()), "op": op, "eager": eager, "guards": guards}


SKIPPED = 4      # the 257-element tensor has no gradient at step 2


@pytest.fixture(scope="module")
def ragged():
    """the unaligned view and the channels-last weight beside the others; one tensor without a gradient at step 2"""
    p0, grads = _inputs(EXTRA, seed=12)
    missing = {(1, SKIPPED)}
    op, guards = _device_steps("op", EXTRA, p0, grads, missing)
    eager, _ = _device_steps("eager", EXTRA, p0, grads, missing)
    return {"f64": _f64_steps(p0, grads, missing), "op": op, "eager": eager, "guards": guards}


@pytest.mark.gpu
def test_three_steps_match_float64_as_closely_as_the_eager_chain(plain):
    ref = plain["f64"]
    coefs = [min(1.0, MAX_NORM / (r[3] + 1e-6)) for r in ref]
    assert coefs[0] < 1e-2 and coefs[1] == 1.0 and coefs[2] < 1e-2      # clipped, not clipped, clipped
    assert [r[4] for r in plain["op"]] == [r[4] for r in ref]            # every tensor's step count
    _compare(plain, MAIN)


@pytest.mark.gpu
def test_a_tensor_without_a_gradient_is_left_alone(ragged):
    op, ref = ragged["op"], ragged["f64"]
    for k in range(3):      # p, m, v bit-unchanged over step 2
        assert torch.equal(op[0][k][SKIPPED], op[1][k][SKIPPED])
    assert [r[4][SKIPPED] for r in op] == [1, 1, 2] == [r[4][SKIPPED] for r in ref]
    assert op[1][4][SKIPPED - 1] == 2      # its neighbours went on
    failures = []
    for k, name in enumerate(("p", "m", "v")):      # step 3 against the float64 run that skipped it too
        ok, msg = _hold(f"step 3 {name}[{SKIPPED}]", op[2][k][SKIPPED], ragged["eager"][2][k][SKIPPED], ref[2][k][SKIPPED])
        failures += [] if ok else [msg]
    assert not failures, "\n".join(failures)


@pytest.mark.gpu
def test_unaligned_and_channels_last_tensors_and_the_guards(ragged):
    _compare(ragged, EXTRA)
    want = _bits(torch.full((1,), GUARD, device=DEV))[0]
    for (before, after), (shape, lead, _) in zip(ragged["guards"]["p"], EXTRA):
        assert before.numel() == lead and after.numel() == 4
        assert (before == want).all() and (after == want).all(), shape
    assert ragged["guards"]["m"].numel() >= 2 * len(EXTRA)      # at least an element before and after every slice
    assert (ragged["guards"]["m"] == want).all() and (ragged["guards"]["v"] == want).all()


@pytest.mark.gpu
def test_the_unaligned_view_is_flagged_and_the_stride_fix_copy_runs():
    p0, grads = _inputs(EXTRA, seed=13)
    params, _, opt = _make("op", EXTRA, p0)
    for i, p in enumerate(params):
        p.grad = grads[0][i].to(DEV).contiguous()
    assert params[-2].data_ptr() % 16 == 4 and params[-1].stride() != params[-1].grad.stride()
    host, head, keep = opt._host_tables()
    rows = host[head:].view(optim.ROW)
    order = [i for gi in (0, 1) for i in range(len(EXTRA)) if _group_of(i) == gi]      # the optimizer's order: group by group
    flags = {order[k]: int(rows["flags"][k]) for k in range(len(order))}
    assert flags[len(EXTRA) - 2] == _lib.ADAMW_UNALIGNED
    assert all(f == 0 for i, f in flags.items() if i != len(EXTRA) - 2)
    k = order.index(len(EXTRA) - 1)
    assert int(rows["g"][k]) != params[-1].grad.data_ptr()      # the gradient was copied into the parameter's strides
    assert sum(int(rows["g"][j]) == params[order[j]].grad.data_ptr() for j in range(len(order))) == len(order) - 1


@pytest.mark.gpu
def test_two_runs_are_bit_identical():
    p0, grads = _inputs(MAIN, seed=14)
    a, _ = _device_steps("op", MAIN, p0, grads, set())
    b, _ = _device_steps("op", MAIN, p0, grads, set())
    for ra, rb in zip(a, b):
        assert ra[3] == rb[3]
        for k in range(3):
            for x, y in zip(ra[k], rb[k]):
                assert torch.equal(x, y)


@pytest.mark.gpu
def test_a_non_finite_gradient_propagates_as_in_the_eager_chain():
    specs = [((5,), 4, False), ((257,), 4, False), ((C + 1,), 4, False)]
    p0, grads = _inputs(specs, seed=15)
    grads[0][1][100] = float("inf")
    result = {}
    for kind in ("op", "eager"):
        params, _, opt = _make(kind, specs, p0)
        for i, p in enumerate(params):
            p.grad = grads[0][i].to(DEV)
        if kind == "op":
            total = opt.step()
        else:
            total = torch.nn.utils.clip_grad_norm_(params, MAX_NORM)
            opt.step()
        result[kind] = (float(total), [p.detach().cpu() for p in params])
    assert result["op"][0] == float("inf") == result["eager"][0]
    for a, b in zip(result["op"][1], result["eager"][1]):
        assert torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(torch.isinf(a), torch.isinf(b))
    assert int(torch.isnan(result["op"][1][1]).sum()) == 1 and bool(torch.isnan(result["op"][1][1][100]))


def _ready(specs, seed):
    p0, grads = _inputs(specs, seed)
    params, _, opt = _make("op", specs, p0)

    def set_grads(step=0):
        for i, p in enumerate(params):
            p.grad = grads[step][i].to(DEV)
    return params, opt, set_grads


@pytest.mark.gpu
def test_step_does_not_wait_for_the_device():
    """behind ~100 ms of queued matmuls, step() returns in less than half the time the stream then takes to drain"""
    params, opt, set_grads = _ready(MAIN, seed=16)
    set_grads()
    opt.step()      # the chunk list, the pinned buffer's first allocation
    a = torch.randn(4096, 4096, device=DEV)
    a @ a           # the GEMM's own first call
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(10):
        a @ a
    torch.cuda.synchronize()
    per = (time.perf_counter() - t0) / 10
    n = max(10, int(math.ceil(0.1 / per)))
    set_grads(1)
    torch.cuda.synchronize()
    for _ in range(n):
        a @ a
    t0 = time.perf_counter()
    opt.step()
    t1 = time.perf_counter()
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    print(f"{n} matmuls of {per * 1e3:.2f} ms queued; step() returned after {(t1 - t0) * 1e3:.3f} ms, "
          f"the stream drained {(t2 - t1) * 1e3:.1f} ms later")
    assert (t2 - t0) >= 0.05, "the queue was not long enough to tell"
    assert (t1 - t0) < 0.5 * (t2 - t1)


class _HostToDevice(torch.utils._python_dispatch.TorchDispatchMode):
    """counts the ops that take a non-empty host tensor and return a device tensor: the uploads"""

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
def test_three_launches_and_one_copy_whatever_the_number_of_tensors():
    from torch.profiler import ProfilerActivity, profile
    counts = {}
    for specs in (MAIN, MAIN[-1:]):
        params, opt, set_grads = _ready(specs, seed=17)
        set_grads()
        opt.step()
        set_grads(1)
        torch.cuda.synchronize()
        with _HostToDevice() as uploads:
            opt.step()
        set_grads(2)
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
            opt.step()
            torch.cuda.synchronize()
        names = [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
        copies = [n for n in names if n.lower().startswith("memcpy")]
        # (the profiler also lists torch's own annotation of the call, "Optimizer.step#ClippedAdamW.step", as a device event)
        kernels = [n for n in names if not n.lower().startswith(("memcpy", "memset", "optimizer.step#"))]
        print(f"{len(specs)} tensors: kernels {kernels}, copies {copies}, uploads {uploads.ops}")
        assert sum("adamw" in n for n in kernels) == len(kernels)      # nothing but the op's own kernels
        assert len(uploads.ops) <= 1 and len(copies) <= 1
        counts[len(specs)] = len(kernels)
    assert counts[len(MAIN)] == counts[1] and 1 <= counts[1] <= 3, counts


@pytest.mark.gpu
def test_an_unchanged_table_is_not_uploaded_again():
    """lr 0 and beta 0 make the corrections constant: with the same gradient tensors the second step's rows equal the first's"""
    p = torch.nn.Parameter(torch.randn(300, device=DEV))
    opt = ClippedAdamW([p], lr=1e-3, betas=(0.0, 0.0))
    p.grad = torch.randn(300, device=DEV)
    before = optim.CALLS["upload"]
    opt.step()
    opt.step()
    assert optim.CALLS["upload"] == before + 1
    opt.param_groups[0]["lr"] = 5e-4
    opt.step()
    assert optim.CALLS["upload"] == before + 2


@pytest.mark.gpu
def test_a_checkpoint_crosses_to_a_stock_adamw_on_the_device():
    """one step with ClippedAdamW, its state dict into torch.optim.AdamW, one more step on both (clip_grad_norm_ by hand on
    the stock side): both agree with two float64 steps as closely as two eager steps do"""
    p0, grads = _inputs(MAIN, seed=18)
    ref = _f64_steps(p0, grads, set())
    eager, _ = _device_steps("eager", MAIN, p0, grads, set())
    params, _, opt = _make("op", MAIN, p0)
    for i, p in enumerate(params):
        p.grad = grads[0][i].to(DEV)
    opt.step()
    other, _, stock = _make("eager", MAIN, [p.detach().cpu() for p in params])
    stock.load_state_dict(copy.deepcopy(opt.state_dict()))
    for ps, o in ((params, opt), (other, stock)):
        for i, p in enumerate(ps):
            p.grad = grads[1][i].to(DEV)
        if o is stock:
            torch.nn.utils.clip_grad_norm_(ps, MAX_NORM)
        o.step()
    failures = []
    for label, ps, o in (("op", params, opt), ("stock", other, stock)):
        for i, p in enumerate(ps):
            got = (p.detach().cpu().double(), o.state[p]["exp_avg"].cpu().double(), o.state[p]["exp_avg_sq"].cpu().double())
            assert float(o.state[p]["step"]) == 2.0
            for k, name in enumerate(("p", "m", "v")):
                ok, msg = _hold(f"{label} {name}[{i}]", got[k], eager[1][k][i], ref[1][k][i])
                failures += [] if ok else [msg]
    assert not failures, "\n".join(failures)
