"""The bf16 matrix-core instantiation of the window attention (vnext_amd/csrc/window_attn_mfma.hip, dtype VNX_BF16 of the
same two entry points; ops/window_attention.py _WindowAttentionBF16; WindowAttention.bf16_core;
train.enable_bf16_window_attention).

Yardstick of every numeric comparison: the float64 expression `reference_core` of tests/test_window_attention.py, evaluated
on the SAME bf16-rounded qkv and grad_out (upcast), errors scaled by each array's largest element (`_rel`).  Bound, computed
at run time per array: error <= max(2 e_ATen, 2^-7), where e_ATen is the error of the ATen evaluation of the same expression
under torch.autocast("cuda", bfloat16) against the same float64 reference on the same inputs (factor 2: different rounding
points and the scatter of a maximum; 2^-7: two bf16 ulps of the largest element; an indexing error is O(1)).  A case counts
as a yardstick only if e_ATen < 5e-2 on all four arrays, which is asserted too."""
import functools
import subprocess

import pytest
import torch

from test_swin import IDOL_TINY, SEQ_TINY, SMALL_SWIN, _build, _max_rel
from test_window_attention import HD, _inputs, _rel, reference_core
from vnext_amd import _lib
from vnext_amd import train as T
from vnext_amd.models.swin import WindowAttention
from vnext_amd.ops import window_attention as WA
from vnext_amd.registry import build_model, get_idol_cfg, get_seqformer_cfg

DEV = "cuda:0"
FLOOR = 2.0 ** -7
NAMES = ("out", "grad_qkv", "grad_bias", "grad_table")

# (w, s, H, W, heads, B): N = 1, 16, 25, 49, 64, 121, 144; shift and no shift; image padding in both directions; grids smaller
# than a window; one real token; odd head counts, 48 heads, several images
CASES = [(7, 3, 9, 20, 6, 2), (7, 0, 14, 7, 1, 5), (7, 0, 5, 4, 3, 1), (7, 3, 1, 1, 1, 1), (12, 6, 23, 40, 6, 1),
         (12, 0, 24, 12, 48, 1), (12, 6, 15, 19, 1, 2), (12, 0, 1, 1, 1, 1), (8, 4, 16, 9, 2, 1), (5, 2, 11, 7, 1, 2),
         (4, 1, 8, 8, 2, 1), (11, 5, 13, 22, 2, 1), (1, 0, 3, 2, 1, 1)]


def _run(fn, qkv, bias, table, go):
    """fn(qkv, bias, table) -> out; the four arrays of a case"""
    qkv, bias, table = (t.detach().clone().requires_grad_(True) for t in (qkv, bias, table))
    out = fn(qkv, bias, table)
    out.backward(go.to(out.dtype))
    return {"out": out.detach(), "grad_qkv": qkv.grad, "grad_bias": bias.grad, "grad_table": table.grad}


@functools.lru_cache(maxsize=None)
def _yardstick(case, qkv_scale=1.0):
    """-> (bf16 inputs on the device, float64 reference arrays, e_ATen per array); computed once per case"""
    w, s, H, W, heads, B = case
    qkv, bias, table, go = _inputs(B, H, W, heads, w, seed=w * 1000 + s * 100 + H + W + heads + B)
    scale = HD ** -0.5
    qkv16 = (qkv * qkv_scale).to(DEV).to(torch.bfloat16)
    go16 = go.to(DEV).to(torch.bfloat16)
    bias32, table32 = bias.float().to(DEV), table.float().to(DEV)
    core = lambda q, b, t: reference_core(q, b, t, B, H, W, heads, w, s, scale)  # noqa: E731
    ref = _run(core, qkv16.double(), bias32.double(), table32.double(), go16.double())
    with torch.autocast("cuda", dtype=torch.bfloat16):
        aten = _run(core, qkv16.float(), bias32, table32, go16.float())
    e_aten = {k: _rel(aten[k], ref[k]) for k in NAMES}
    return (qkv16, bias32, table32, go16), ref, e_aten


def _check(got, ref, e_aten, label, yardstick_valid=True):
    errs = {k: _rel(got[k], ref[k]) for k in NAMES}
    print(label, "errors", errs, "ATen", e_aten)
    if yardstick_valid:
        assert all(e < 5e-2 for e in e_aten.values()), ("not a valid yardstick", e_aten)
    for k in NAMES:
        assert bool(torch.isfinite(got[k]).all()), k
        assert errs[k] <= max(2.0 * e_aten[k], FLOOR), (k, errs[k], e_aten[k])
    return errs


def _core_bf16(case):
    w, s, H, W, heads, B = case
    return lambda q, b, t: WA._WindowAttentionBF16.apply(q, b, t, B, H, W, heads, w, s, HD ** -0.5)


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(map(str, c)))
def test_bf16_core_matches_the_yardstick(case):
    """The one-token grids (one real token beside 48 / 143 padded keys) are the sharp cases: every gradient of that single
    row is proportional to one probability, so a rounding acts on one scalar instead of averaging.  Two kernel choices come
    from them: D = rowsum(p o dP) instead of rowsum(dO o O) with the stored bf16 O (6e-2 / 9e-2 on grad_qkv), and p / dS as two
    bf16 terms in the grad_v / grad_k products (9.57e-3 on `(12, 0, 1, 1, 1, 1)` with single terms, against 2^-7)."""
    w, s, H, W, heads, B = case
    (qkv16, bias32, table32, go16), ref, e_aten = _yardstick(case)
    got = _run(_core_bf16(case), qkv16, bias32, table32, go16)
    assert got["out"].dtype == torch.bfloat16 and got["grad_qkv"].dtype == torch.bfloat16
    assert got["grad_bias"].dtype == torch.float32 and got["grad_table"].dtype == torch.float32
    _check(got, ref, e_aten, f"case {case}")
    if (H % w or W % w) and s == 0:
        # the padded tokens' share of the bias gradient is real: the column sum of grad_qkv alone misses the reference by
        # more than the bound, and differs from what the function returns
        colsum = got["grad_qkv"].sum(0, dtype=torch.float32)
        assert _rel(colsum, ref["grad_bias"]) > max(2.0 * e_aten["grad_bias"], FLOOR)
        assert not torch.equal(colsum, got["grad_bias"])


@pytest.mark.gpu
def test_bf16_core_with_large_scores():
    case = (7, 3, 9, 20, 2, 1)
    (qkv16, bias32, table32, go16), ref, e_aten = _yardstick(case, 8.0)
    got = _run(_core_bf16(case), qkv16, bias32, table32, go16)
    # finite and within the same bound.  NOT a yardstick in the sense of the other cases: with scores of ~100 the bf16
    # rounding of q and k alone (2^-9 of each operand) moves a score by tenths, so ATen and the kernel both sit at ~1e-1 of
    # the float64 reference (measured: ATen 0.12 .. 0.21, kernel 0.08 .. 0.15); e_ATen < 5e-2 cannot hold here
    _check(got, ref, e_aten, f"case {case} x 8", yardstick_valid=False)


def _guarded(n, fill, dtype, guard=64):
    buf = torch.full((n + 2 * guard,), fill, dtype=dtype, device=DEV)
    return buf, buf[guard:guard + n], guard


@pytest.mark.gpu
@pytest.mark.parametrize("w,s,H,W,heads,B", [(7, 3, 9, 20, 6, 2), (12, 6, 23, 40, 6, 1), (12, 0, 5, 4, 48, 1)])
def test_c_abi_bf16_guard_words_every_element_written_bit_identical(w, s, H, W, heads, B):
    lib = _lib.lib()
    C = heads * HD
    rows = B * H * W
    qkv, bias, table, go = (t.to(DEV) for t in _inputs(B, H, W, heads, w, seed=77))
    qkv, go = qkv.to(torch.bfloat16).contiguous(), go.to(torch.bfloat16).contiguous()
    bias, table = bias.float().contiguous(), table.float().contiguous()
    scale = HD ** -0.5
    sentinel = 12288.0                                # finite, exact in bf16
    stream = _lib.current_stream(qkv)
    bf, f32 = torch.bfloat16, torch.float32

    def intact(bufs):
        for name, (buf, view, guard) in bufs.items():
            assert bool((buf[:guard] == sentinel).all()) and bool((buf[guard + view.numel():] == sentinel).all()), name

    fwd = []
    for _ in range(2):
        bufs = {"out": _guarded(rows * C, sentinel, bf), "lse": _guarded(rows * heads, sentinel, f32)}
        _lib.check(lib.vnx_window_attention_forward(_lib.VNX_BF16, qkv.data_ptr(), bias.data_ptr(), table.data_ptr(),
                                                    bufs["out"][1].data_ptr(), bufs["lse"][1].data_ptr(), B, H, W, heads,
                                                    HD, 3 * C, w, s, scale, stream))
        torch.cuda.synchronize()
        intact(bufs)
        for name in bufs:
            assert not bool((bufs[name][1] == sentinel).any()), name
            assert bool(torch.isfinite(bufs[name][1]).all()), name
        fwd.append([bufs[n][1].clone() for n in ("out", "lse")])
    for a, b in zip(*fwd):
        assert torch.equal(a, b)
    out, lse = fwd[0]
    nbytes = lib.vnx_window_attention_partial_bytes(B, H, W, heads, w)
    results = []
    for _ in range(2):
        bufs = {"g": _guarded(rows * 3 * C, sentinel, bf), "gt": _guarded(table.numel(), sentinel, f32),
                "gp": _guarded(3 * C, sentinel, f32), "part": _guarded(nbytes // 4, sentinel, f32)}
        _lib.check(lib.vnx_window_attention_backward(
            _lib.VNX_BF16, qkv.data_ptr(), bias.data_ptr(), table.data_ptr(), out.data_ptr(), lse.data_ptr(),
            go.data_ptr(), bufs["g"][1].data_ptr(), bufs["gt"][1].data_ptr(), bufs["gp"][1].data_ptr(),
            bufs["part"][1].data_ptr(), nbytes, B, H, W, heads, HD, 3 * C, w, s, scale, stream))
        torch.cuda.synchronize()
        intact(bufs)
        for name in ("g", "gt", "gp"):                                  # every element written
            assert not bool((bufs[name][1] == sentinel).any()), name
            assert bool(torch.isfinite(bufs[name][1]).all()), name
        results.append([bufs[n][1].clone() for n in ("g", "gt", "gp")])
    for a, b in zip(*results):
        assert torch.equal(a, b)


@pytest.mark.gpu
def test_bf16_argument_checks_before_any_launch():
    lib = _lib.lib()
    t = torch.zeros(16384, device=DEV)
    stream = _lib.current_stream(t)
    p = t.data_ptr()
    bf = _lib.VNX_BF16
    fwd, bwd = lib.vnx_window_attention_forward, lib.vnx_window_attention_backward
    # fp16 stays unsupported
    assert fwd(_lib.VNX_F16, p, p, p, p, p, 1, 7, 7, 1, 32, 96, 7, 0, 0.17, stream) == 2
    assert bwd(_lib.VNX_F16, p, p, p, p, p, p, p, p, p, p, 65536, 1, 7, 7, 1, 32, 96, 7, 0, 0.17, stream) == 2
    # bf16: a row stride that is a multiple of 4 but not of 8 elements; misaligned qkv / out
    assert fwd(bf, p, p, p, p, p, 1, 7, 7, 1, 32, 100, 7, 0, 0.17, stream) == 1
    assert bwd(bf, p, p, p, p, p, p, p, p, p, p, 65536, 1, 7, 7, 1, 32, 100, 7, 0, 0.17, stream) == 1
    assert fwd(bf, p + 2, p, p, p, p, 1, 7, 7, 1, 32, 96, 7, 0, 0.17, stream) == 1
    assert fwd(bf, p, p, p, p + 8, p, 1, 7, 7, 1, 32, 96, 7, 0, 0.17, stream) == 1
    assert bwd(bf, p, p, p, p, p, p, p + 2, p, p, p, 65536, 1, 7, 7, 1, 32, 96, 7, 0, 0.17, stream) == 1
    # head_dim 64, window 13, 49 heads; a partial buffer too small
    assert fwd(bf, p, p, p, p, p, 1, 7, 7, 1, 64, 192, 7, 0, 0.125, stream) == 2
    assert fwd(bf, p, p, p, p, p, 1, 13, 13, 1, 32, 96, 13, 0, 0.17, stream) == 2
    assert bwd(bf, p, p, p, p, p, p, p, p, p, p, 65536, 1, 13, 13, 1, 32, 96, 13, 0, 0.17, stream) == 2
    assert fwd(bf, p, p, p, p, p, 1, 7, 7, 49, 32, 49 * 96, 7, 0, 0.17, stream) == 2
    assert bwd(bf, p, p, p, p, p, p, p, p, p, p, 4, 1, 7, 7, 1, 32, 96, 7, 0, 0.17, stream) == 3
    torch.cuda.synchronize()
    assert bool((t == 0).all())                       # nothing ran


@pytest.fixture
def dtype_spy(monkeypatch):
    """records the dtype argument of every vnx_window_attention_forward / _backward made through the package"""
    lib = _lib.lib()
    seen = {"fwd": [], "bwd": []}

    class Spy:
        def __getattr__(self, name):
            return getattr(lib, name)

        def vnx_window_attention_forward(self, *args):
            seen["fwd"].append(args[0])
            return lib.vnx_window_attention_forward(*args)

        def vnx_window_attention_backward(self, *args):
            seen["bwd"].append(args[0])
            return lib.vnx_window_attention_backward(*args)
    monkeypatch.setattr(_lib, "lib", lambda: Spy())
    return seen


def _block_setup(device):
    torch.manual_seed(3)
    attn = WindowAttention(64, 7, 2).to(device)
    with torch.no_grad():
        attn.relative_position_bias_table.normal_(0.0, 1.0)
    H, W = 9, 10
    x = torch.randn(2, H * W, 64, device=device)
    return attn, x, H, W


@pytest.mark.gpu
def test_block_takes_the_bf16_core_only_under_bf16_autocast_with_the_switch_on(dtype_spy):
    attn, x, H, W = _block_setup(DEV)
    block = lambda: WA.window_attention_block(x, H, W, attn, 7, 3)  # noqa: E731
    outs = {}
    with torch.no_grad():
        for on in (False, True):
            attn.bf16_core = on
            with torch.autocast("cuda", dtype=torch.bfloat16):
                outs["amp", on] = block()
            with torch.autocast("cuda", dtype=torch.float16):
                outs["half", on] = block()
            outs["fp32", on] = block()
    assert dtype_spy["fwd"] == [_lib.VNX_F32] * 3 + [_lib.VNX_BF16, _lib.VNX_F32, _lib.VNX_F32]
    assert outs["amp", True].dtype == torch.bfloat16 and outs["fp32", True].dtype == torch.float32
    assert torch.equal(outs["fp32", True], outs["fp32", False])
    assert torch.equal(outs["half", True], outs["half", False])
    # switch on against switch off under autocast: within the yardstick bound, e_ATen being the error of the reference
    # expression of the block under the same autocast against the block in float64
    with torch.no_grad():
        ref = WA.reference_block(x.double(), H, W, attn.double(), 7, 3)
        attn.float()
        with torch.autocast("cuda", dtype=torch.bfloat16):
            aten = WA.reference_block(x, H, W, attn, 7, 3)
    e_aten = _rel(aten, ref)
    err = _rel(outs["amp", True], outs["amp", False])
    print("block: on vs off", err, "ATen", e_aten, "on vs float64", _rel(outs["amp", True], ref))
    assert e_aten < 5e-2
    assert err <= max(2.0 * e_aten, FLOOR)
    # the backward goes the same way
    attn.bf16_core = True
    xg = x.clone().requires_grad_(True)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        WA.window_attention_block(xg, H, W, attn, 7, 3).float().sum().backward()
    assert dtype_spy["bwd"] == [_lib.VNX_BF16]
    assert bool(torch.isfinite(xg.grad).all()) and float(xg.grad.abs().sum()) > 0
    assert attn.qkv.bias.grad.dtype == torch.float32 and float(attn.qkv.bias.grad.abs().sum()) > 0


@pytest.mark.gpu
def test_swin_backbone_with_the_bf16_core_under_autocast(dtype_spy):
    """the bound of the existing autocast test (test_swin.py) for the default path: finite, within 5e-2 of fp32"""
    module, x = _build("swin_w7", DEV, torch.float32)
    T.enable_bf16_window_attention(module)
    with torch.no_grad():
        ref = module(x)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            amp = module(x)
    assert dtype_spy["fwd"] == [_lib.VNX_F32] * 8 + [_lib.VNX_BF16] * 8
    for k in ref:
        assert torch.isfinite(amp[k]).all()
        assert _max_rel(amp[k].float().cpu().numpy(), ref[k].cpu().numpy()) < 5e-2, k


@pytest.mark.gpu
@pytest.mark.parametrize("arch", ["SeqFormer", "IDOL"])
def test_training_step_under_bf16_autocast_with_the_bf16_core(arch, dtype_spy):
    torch.manual_seed(31)
    if arch == "SeqFormer":
        cfg = get_seqformer_cfg(**{"MODEL.DEVICE": DEV, **SEQ_TINY, **SMALL_SWIN})
    else:
        cfg = get_idol_cfg(**{"MODEL.DEVICE": DEV, **IDOL_TINY, **SMALL_SWIN})
    model = build_model(cfg).train()
    T.enable_bf16_window_attention(model)
    clips = T.synthetic_clips(2, 2, 96, 160, DEV, seed=5, num_instances=2)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        losses = model(clips)
    assert all(torch.isfinite(v) for v in losses.values())
    sum(losses.values()).backward()
    assert len(dtype_spy["fwd"]) >= 8 and set(dtype_spy["fwd"]) == {_lib.VNX_BF16}
    assert len(dtype_spy["bwd"]) >= 7 and set(dtype_spy["bwd"]) == {_lib.VNX_BF16}
    bb = model.detr.detr.backbone
    dead = [n for n, p in bb.named_parameters() if p.requires_grad and (p.grad is None or not float(p.grad.abs().sum()) > 0)]
    assert not dead, dead
    assert all(torch.isfinite(p.grad).all() for p in bb.parameters() if p.grad is not None)


@pytest.mark.gpu
def test_graph_replayed_inference_with_the_bf16_core_equals_eager(dtype_spy):
    import numpy as np
    torch.manual_seed(5)
    model = build_model(get_seqformer_cfg(**{"MODEL.DEVICE": DEV, **SEQ_TINY, **SMALL_SWIN})).eval()
    T.enable_bf16_window_attention(model)
    clips = T.synthetic_clips(2, 2, 96, 160, DEV, seed=8, num_instances=0)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        graphed = [model([c]) for c in clips]
        assert len(model._graphs) == 1
        model.graph_inference = False
        eager = [model([c]) for c in clips]
    assert dtype_spy["fwd"] and set(dtype_spy["fwd"]) == {_lib.VNX_BF16}
    for g, e in zip(graphed, eager):
        assert g["pred_labels"] == e["pred_labels"]
        np.testing.assert_allclose(g["pred_scores"], e["pred_scores"], rtol=1e-5)
        for mg, me in zip(g["pred_masks"], e["pred_masks"]):
            assert float((mg != me).float().mean()) < 1e-3


# ---- without a GPU ---------------------------------------------------------------------------------------------------------

def test_enable_bf16_window_attention_sets_and_clears_every_switch():
    model = build_model(get_seqformer_cfg(**{"MODEL.DEVICE": "cpu", **SEQ_TINY, **SMALL_SWIN}))
    mods = [m for m in model.modules() if isinstance(m, WindowAttention)]
    assert len(mods) == 8 and not any(m.bf16_core for m in mods)          # off by default
    T.enable_bf16_window_attention(model)
    assert all(m.bf16_core is True for m in mods)
    T.enable_bf16_window_attention(model, on=False)
    assert all(m.bf16_core is False for m in mods)


def test_enable_bf16_window_attention_raises_without_a_swin_backbone():
    model = build_model(get_seqformer_cfg(**{"MODEL.DEVICE": "cpu", **SEQ_TINY}))
    with pytest.raises(ValueError):
        T.enable_bf16_window_attention(model)


def test_switch_changes_nothing_on_cpu_tensors():
    attn, x, H, W = _block_setup("cpu")
    with torch.no_grad():
        off = WA.window_attention_block(x, H, W, attn, 7, 3)
        attn.bf16_core = True
        on = WA.window_attention_block(x, H, W, attn, 7, 3)
        with torch.autocast("cpu", dtype=torch.bfloat16):
            on_amp = WA.window_attention_block(x, H, W, attn, 7, 3)
        attn.bf16_core = False
        with torch.autocast("cpu", dtype=torch.bfloat16):
            off_amp = WA.window_attention_block(x, H, W, attn, 7, 3)
    assert torch.equal(on, off) and torch.equal(on_amp, off_amp)


def test_abi_version_and_window_attention_symbols_unchanged():
    assert _lib.lib().vnx_abi_version() == 17 and _lib.ABI_VERSION == 17
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True)
    names = sorted(line.split()[-1] for line in out.splitlines() if " T vnx_window_attention" in line)
    assert names == ["vnx_window_attention_backward", "vnx_window_attention_forward", "vnx_window_attention_partial_bytes"]
