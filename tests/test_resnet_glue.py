"""The fused element-wise glue of the ResNet trunk (vnext_amd/csrc/resnet_glue.hip, vnext_amd/ops/resnet_glue.py) on the
GPU: the three entry points through the C ABI (guard words around what they write, unaligned views) and through the Python
ops, the epilogue's autograd, the trunk with the switch on against the switch off with float64 as the judge, and the ops
inside a captured graph.

fp32 results are held to `torch.equal` with the eager expression on the same tensors; 16-bit results to the fp32 sum
rounded once.  NaN positions are compared separately (NaN != NaN)."""
import pytest
import torch
import torch.nn.functional as F

import resnet_golden_recipe as R
from vnext_amd import _lib
from vnext_amd import train as T
from vnext_amd.models import resnet
from vnext_amd.models.resnet import ResNetTrunk
from vnext_amd.ops import resnet_glue as G
from vnext_amd.utils.checkpoint import load_reference_checkpoint, reference_state_dict

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NCHW, NHWC = _lib.LAYOUT_NCHW, _lib.LAYOUT_NHWC
CODES = {torch.float32: _lib.VNX_F32, torch.bfloat16: _lib.VNX_BF16, torch.float16: _lib.VNX_F16}
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
# (layout, (n, c, h, w)).  The issue's list, then: h * w = 17 (against 8 elements per 16 bytes), h * w = 32 (a whole number
# of 16-byte chunks per plane for every type: one shift per chunk), h * w = 12 (whole chunks in fp32 only) and two
# workgroups' worth of chunks in each layout.
EPILOGUE_CASES = [(NCHW, (2, 3, 3, 5)), (NCHW, (1, 1, 1, 1)), (NCHW, (2, 64, 1, 1)), (NCHW, (1, 5, 7, 9)),
                  (NHWC, (2, 64, 3, 5)), (NHWC, (1, 6, 3, 5)), (NHWC, (1, 256, 1, 1)),
                  (NCHW, (1, 3, 1, 17)), (NHWC, (1, 3, 1, 17)), (NCHW, (2, 5, 4, 8)), (NCHW, (1, 3, 3, 4)),
                  (NCHW, (2, 24, 8, 16)), (NHWC, (3, 40, 5, 7))]
FORMS = ["plain", "res", "res_bias"]
GUARD = 16      # elements in front of and behind a buffer the kernel writes


def _values(shape, dtype, seed, special=True):
    """negative values, exact zeros, and (special) one NaN and one +inf, logical [n, c, h, w]"""
    g = torch.Generator(device=DEV).manual_seed(seed)
    t = torch.randn(shape, device=DEV, generator=g)
    flat = t.view(-1)
    flat[::5] = 0.0
    if special and flat.numel() >= 4:
        flat[1] = float("nan")
        flat[flat.numel() - 2] = float("inf")
    return t.to(dtype)


def _memory(t, layout):
    """the flat memory image of logical [n, c, h, w] in `layout`"""
    return (t.permute(0, 2, 3, 1) if layout == NHWC else t).contiguous().reshape(-1)


def _logical(flat, shape, layout):
    n, c, h, w = shape
    return flat.reshape(n, h, w, c).permute(0, 3, 1, 2) if layout == NHWC else flat.reshape(n, c, h, w)


def _guarded(image, offset):
    """a buffer with `offset` elements in front of a copy of `image` and GUARD behind -> (buffer, the view)"""
    buf = torch.full((offset + image.numel() + GUARD,), 777.0, dtype=image.dtype, device=DEV)
    view = buf[offset:offset + image.numel()]
    view.copy_(image)
    return buf, view


def _guards_intact(buf, view, offset):
    want = torch.full_like(buf, 777.0)
    return torch.equal(buf[:offset], want[:offset]) and torch.equal(buf[offset + view.numel():], want[offset + view.numel():])


def _same(got, want):
    """equal, NaN positions compared separately"""
    nan = torch.isnan(want)
    zero = torch.zeros_like(want)
    return torch.equal(torch.isnan(got), nan) and torch.equal(torch.where(nan, zero, got), torch.where(nan, zero, want))


def _epilogue_reference(y, b, r, rb):
    """fp32: the eager chain itself.  16-bit: the fp32 sum, rounded once."""
    v = lambda t: t.float().reshape(1, -1, 1, 1) if t.dim() == 1 else t.float()      # noqa: E731
    if y.dtype == torch.float32:
        out = y + b.reshape(1, -1, 1, 1)
        if r is not None:
            out = out + (r if rb is None else r + rb.reshape(1, -1, 1, 1))
        return torch.relu(out)
    out = v(y) + v(b)
    if r is not None:
        out = out + (v(r) if rb is None else v(r) + v(rb))
    return out.clamp_min(0).to(y.dtype)


def _operands(shape, dtype, form, seed):
    y = _values(shape, dtype, seed)
    b = _values((1, shape[1], 1, 1), dtype, seed + 1, special=False).reshape(-1).contiguous()
    r = _values(shape, dtype, seed + 2).roll(3, dims=-1) if form != "plain" else None
    rb = _values((1, shape[1], 1, 1), dtype, seed + 3, special=False).reshape(-1).contiguous() if form == "res_bias" else None
    return y, b, r, rb


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16", "f16"])
@pytest.mark.parametrize("layout,shape", EPILOGUE_CASES, ids=[f"{'nhwc' if l else 'nchw'}-{'x'.join(map(str, s))}" for l, s in EPILOGUE_CASES])
def test_epilogue_forward_through_the_c_abi(layout, shape, dtype):
    lib = _lib.lib()
    n, c, h, w = shape
    for form in FORMS:
        y, b, r, rb = _operands(shape, dtype, form, 100 + 7 * FORMS.index(form))
        want = _epilogue_reference(y, b, r, rb)
        for offset in (GUARD, 1):      # 16-byte aligned, and a view one element off: element accesses
            buf, view = _guarded(_memory(y, layout), offset)
            res_image = _memory(r, layout).clone() if r is not None else None
            res_before = res_image.clone() if r is not None else None
            ptr = lambda t: t.data_ptr() if t is not None else None      # noqa: E731
            _lib.check(lib.vnx_conv_epilogue_forward(CODES[dtype], layout, view.data_ptr(), b.data_ptr(), ptr(res_image),
                                                     ptr(rb), n, c, h * w, _lib.current_stream(y)))
            assert _same(_logical(view, shape, layout), want), (form, offset)
            assert _guards_intact(buf, view, offset), (form, offset)
            if r is not None:
                assert _same(res_image, res_before), (form, offset)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16", "f16"])
@pytest.mark.parametrize("layout,shape", EPILOGUE_CASES, ids=[f"{'nhwc' if l else 'nchw'}-{'x'.join(map(str, s))}" for l, s in EPILOGUE_CASES])
def test_epilogue_forward_through_the_python_op(layout, shape, dtype):
    fmt = torch.channels_last if layout == NHWC else torch.contiguous_format
    for form in FORMS:
        y, b, r, rb = _operands(shape, dtype, form, 300 + 7 * FORMS.index(form))
        want = _epilogue_reference(y, b, r, rb)
        y = y.contiguous(memory_format=fmt)
        r = r.contiguous(memory_format=fmt) if r is not None else None
        r_before = r.clone() if r is not None else None
        out = G.conv_epilogue(y, b, r, rb)
        assert out.data_ptr() == y.data_ptr() and out.stride() == y.stride()      # in place
        assert _same(out, want), form
        if r is not None:
            assert _same(r, r_before), form
        if dtype == torch.float32:
            assert _same(G.conv_epilogue_reference(*_operands(shape, dtype, form, 300 + 7 * FORMS.index(form))), want)


def test_epilogue_refuses_what_it_does_not_take():
    y = torch.zeros(1, 4, 2, 2, device=DEV)
    b = torch.zeros(4, device=DEV)
    with pytest.raises(RuntimeError, match="CPU"):
        G.conv_epilogue(y.cpu(), b.cpu())
    with pytest.raises(ValueError):
        G.conv_epilogue(y[:, :, :, ::2], b)                      # neither contiguous nor channels-last
    with pytest.raises(ValueError):
        G.conv_epilogue(y, b.double())
    with pytest.raises(ValueError):
        G.conv_epilogue(y, b, None, b)
    lib = _lib.lib()
    assert lib.vnx_conv_epilogue_forward(_lib.VNX_F64, NCHW, y.data_ptr(), b.data_ptr(), None, None, 1, 4, 4,
                                         _lib.current_stream(y)) == _lib.VNX_ERR_UNSUPPORTED
    assert lib.vnx_conv_epilogue_forward(_lib.VNX_F32, 2, y.data_ptr(), b.data_ptr(), None, None, 1, 4, 4,
                                         _lib.current_stream(y)) == _lib.VNX_ERR_UNSUPPORTED
    assert lib.vnx_conv_epilogue_forward(_lib.VNX_F32, NCHW, y.data_ptr(), b.data_ptr(), None, b.data_ptr(), 1, 4, 4,
                                         _lib.current_stream(y)) != _lib.VNX_OK      # res_bias without res
    assert torch.count_nonzero(y) == 0


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16", "f16"])
def test_epilogue_backward_through_the_c_abi(dtype):
    lib = _lib.lib()
    for count in (1, 7, 8, 1003, 2048):
        y = _values((1, 1, 1, count), dtype, 500 + count, special=False).reshape(-1).clamp_min(0)
        gy = _values((1, 1, 1, count), dtype, 600 + count, special=False).reshape(-1)
        want = gy * (y > 0)
        for offset in (GUARD, 1):
            buf, view = _guarded(torch.zeros_like(gy), offset)
            yb, yv = _guarded(y, offset)
            gb, gv = _guarded(gy, offset)
            _lib.check(lib.vnx_conv_epilogue_backward(CODES[dtype], gv.data_ptr(), yv.data_ptr(), view.data_ptr(), count,
                                                      _lib.current_stream(y)))
            assert torch.equal(view, want), (count, offset)
            assert _guards_intact(buf, view, offset) and torch.equal(yv, y) and torch.equal(gv, gy)


@pytest.mark.parametrize("layout", [NCHW, NHWC], ids=["nchw", "nhwc"])
@pytest.mark.parametrize("form", FORMS)
def test_epilogue_autograd_equals_the_eager_chain(form, layout):
    shape = (2, 12, 5, 7)
    fmt = torch.channels_last if layout == NHWC else torch.contiguous_format
    y0, b, r0, rb = _operands(shape, torch.float32, form, 700)
    y0, r0 = y0.nan_to_num(0.0, 1.0, -1.0), (r0.nan_to_num(0.0, 1.0, -1.0) if r0 is not None else None)
    weight = _values(shape, torch.float32, 710, special=False)
    grads = []
    for fused in (False, True):
        a = y0.clone().contiguous(memory_format=fmt).requires_grad_(True)
        r = r0.clone().contiguous(memory_format=fmt).requires_grad_(True) if r0 is not None else None
        bias = b.clone().requires_grad_(True)
        y = a * 1.0                                              # a convolution's output: not a leaf
        if fused:
            out = G.conv_epilogue(y, bias, r, rb)
            assert out is y or out.data_ptr() == y.data_ptr()
        else:
            out = G.conv_epilogue_reference(y, bias.detach(), r, rb)
        (out * weight).sum().backward()
        assert bias.grad is None                                 # a frozen norm's shift: no gradient
        grads.append((out.detach().clone(), a.grad, r.grad if r is not None else None))
    (o0, ga0, gr0), (o1, ga1, gr1) = grads
    assert torch.equal(o0, o1) and torch.equal(ga0, ga1)
    assert torch.equal(ga1, weight * (o1 > 0))
    if r0 is not None:
        assert torch.equal(gr0, gr1)


STEM_SIZES = [(7, 9), (1, 1), (1, 6), (8, 8)]


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16", "f16"])
@pytest.mark.parametrize("layout", [NCHW, NHWC], ids=["nchw", "nhwc"])
@pytest.mark.parametrize("h,w", STEM_SIZES)
def test_stem_pool(h, w, layout, dtype):
    lib = _lib.lib()
    fmt = torch.channels_last if layout == NHWC else torch.contiguous_format
    for n, c in ((2, 8), (1, 3), (3, 64)):      # 16 bytes of channels per pixel in every type / an odd c / the stem's own
        x = _values((n, c, h, w), dtype, 800 + c)
        b = _values((1, c, 1, 1), dtype, 801 + c, special=False).reshape(-1).contiguous()
        ref32 = F.max_pool2d(F.relu(x.float() + b.float().reshape(1, -1, 1, 1)), 3, 2, 1)
        want = ref32.to(dtype)                                   # 16-bit: the rounding of the fp32 result
        if dtype == torch.float32:
            assert _same(F.max_pool2d(F.relu(x + b.reshape(1, -1, 1, 1)), 3, 2, 1), want)
        oh, ow = (h - 1) // 2 + 1, (w - 1) // 2 + 1
        assert want.shape == (n, c, oh, ow)
        for offset in (GUARD, 1):
            buf, view = _guarded(torch.zeros(n * c * oh * ow, dtype=dtype, device=DEV), offset)
            xb, xv = _guarded(_memory(x, layout), offset)
            _lib.check(lib.vnx_stem_pool_forward(CODES[dtype], layout, xv.data_ptr(), b.data_ptr(), view.data_ptr(), n, c, h, w,
                                                 _lib.current_stream(x)))
            assert _same(_logical(view, (n, c, oh, ow), layout), want), (n, c, offset)
            assert _guards_intact(buf, view, offset)
        with torch.no_grad():
            out = G.stem_pool(x.contiguous(memory_format=fmt), b)
        assert _same(out, want) and out.shape == want.shape
        if layout == NHWC:
            assert out.is_contiguous(memory_format=torch.channels_last)


def test_stem_pool_takes_the_eager_chain_when_the_stem_wants_a_gradient(monkeypatch):
    x = _values((1, 8, 7, 9), torch.float32, 900, special=False).requires_grad_(True)
    b = torch.randn(8, device=DEV)
    calls = []
    monkeypatch.setattr(G, "stem_pool_reference", lambda y, bias: calls.append("eager") or F.max_pool2d(F.relu(y + bias.reshape(1, -1, 1, 1)), 3, 2, 1))
    out = G.stem_pool(x * 1.0, b)
    assert calls == ["eager"] and out.grad_fn is not None
    out.sum().backward()
    assert x.grad is not None
    with torch.no_grad():
        fused = G.stem_pool(x * 1.0, b)
    assert calls == ["eager"] and torch.equal(fused, out.detach())
    # the trunk: an unfrozen stem keeps the eager stem, a frozen one (or no grad) takes the fused pass
    trunk = ResNetTrunk(50).to(DEV)
    trunk.fused_glue = True
    img = torch.randn(1, 3, 32, 32, device=DEV)
    assert not trunk._stem_fused(img)
    assert trunk.freeze(1)._stem_fused(img) and not trunk._stem_fused(img.clone().requires_grad_(True))
    with torch.no_grad():
        assert ResNetTrunk(50)._stem_fused(img)


# ---- the trunk, switch on against switch off, float64 as the judge ----------------------------------------------------------

def _seeded_trunk(depth, seed):
    """a float32 trunk on the GPU and its float64 twin on the CPU with the same seeded weights and norm statistics (the
    recipe of the detectron2 fixtures: non-trivial shifts), stem and res2 frozen"""
    torch.manual_seed(seed)
    trunk = ResNetTrunk(depth)
    shapes = [(k, v.shape) for k, v in reference_state_dict(trunk).items()]
    state = {k: v.float() for k, v in R.reference_state(shapes, seed).items()}       # fp32 values, held exactly by both
    load_reference_checkpoint(trunk, state)
    twin = ResNetTrunk(depth).double()
    load_reference_checkpoint(twin, {k: v.double() for k, v in state.items()})
    return trunk.freeze(2).to(DEV), twin.freeze(2)


_TRUNKS = {}


def _trunk_case(depth):
    """(trunk, twin, input, loss weights, float64 results per (training, rounded input)) -- built once per depth"""
    if depth not in _TRUNKS:
        trunk, twin = _seeded_trunk(depth, 40 + depth)
        g = torch.Generator().manual_seed(depth)
        x = torch.randn(2, 3, 64, 96, generator=g)
        weights = [torch.randn(2, c, 64 // s, 96 // s, generator=g) for c, s in zip(trunk.num_channels, trunk.strides)]
        _TRUNKS[depth] = (trunk, twin, x, weights, {})
    return _TRUNKS[depth]


def _run(trunk, x, weights, training, autocast):
    """-> {name: array}: the outputs and, in training mode, the input's and the trainable filters' gradients"""
    trunk.train(training)
    trunk.zero_grad(set_to_none=True)
    x = x.clone().requires_grad_(training)
    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast and x.is_cuda), torch.set_grad_enabled(training):
        outs = trunk(x)
    res = {f"res{i + 3}": o.detach().double().cpu() for i, o in enumerate(outs)}
    if training:
        sum((o.double() * w.to(o.device).double()).sum() for o, w in zip(outs, weights)).backward()
        res["grad_input"] = x.grad.double().cpu()
        res.update({"grad_" + k: p.grad.double().cpu() for k, p in trunk.named_parameters() if p.requires_grad})
    return res


@pytest.mark.parametrize("autocast", [False, True], ids=["fp32", "bf16_autocast"])
@pytest.mark.parametrize("training", [False, True], ids=["eval_nchw", "train_channels_last"])
@pytest.mark.parametrize("depth", [50, 101])
def test_trunk_with_the_switch_on_is_no_worse_than_off(depth, training, autocast, monkeypatch):
    """Required per array: e_on <= 2 * e_off (largest error against the float64 trunk), or the two arrays equal.
    Deterministic convolution algorithms are requested for both legs, so that the verdict is the same in every process:
    without that the switch-off leg run twice in one process differed from ITSELF by up to 2.34 x in a weight gradient's
    largest error under bf16 (the backward convolutions are not bit-reproducible).
    Measured on an MI355X: in every fp32 leg the two legs' arrays are EQUAL, outputs and gradients (res5 off by 8.1e-5 for
    depth 50 and 5.5e-4 for depth 101 in both); the bf16 eval legs, where the tail's fp32 sum is rounded once, hold the
    bound (res5: 0.70 against 0.95, 6.26 against 6.39).  In the bf16 TRAINING legs the arrays are equal as well, because
    there the trunk keeps the eager tail (models/resnet.py: `_Bottleneck._forward_fused`): with the fused tail in a bf16
    training step this test missed the bound -- depth 50 in 1 gradient array of 46 (ratio 2.66), depth 101 in 3 of 97 (up
    to 3.16), median ratios 0.92 / 1.03 -- and the code was changed, not the bound."""
    trunk, twin, x, weights, judged = _trunk_case(depth)
    monkeypatch.setattr(resnet, "CHANNELS_LAST", training)       # training steps run channels-last, inference NCHW
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)
    monkeypatch.setattr(torch.backends.cudnn, "benchmark", False)
    x_seen = x.bfloat16().float() if autocast else x            # under autocast the judge sees the bf16-rounded input
    if (training, autocast) not in judged:
        judged[(training, autocast)] = _run(twin, x_seen.double(), weights, training, False)
    want = judged[(training, autocast)]
    legs = {}
    for on in (False, True):
        T.enable_fused_resnet_glue(trunk, on)
        legs[on] = _run(trunk, x_seen.to(DEV), weights, training, autocast)
    trunk.fused_glue = False
    assert set(legs[True]) == set(legs[False]) == set(want)
    if training:      # the input's gradient and every trainable filter's: three or four per block of res3 .. res5
        assert "grad_input" in want and len(want) >= 4 + 3 * sum(map(len, (trunk.res3, trunk.res4, trunk.res5)))
    worst = []
    for name, ref in want.items():
        e_off = float((legs[False][name] - ref).abs().max())
        e_on = float((legs[True][name] - ref).abs().max())
        if not (e_on <= 2 * e_off or torch.equal(legs[True][name], legs[False][name])):
            worst.append((name, e_on, e_off, float(ref.abs().max())))
    print(f"depth {depth} training {training} autocast {autocast}: {len(want)} arrays, "
          f"res5 e_on {float((legs[True]['res5'] - want['res5']).abs().max()):.3e} "
          f"e_off {float((legs[False]['res5'] - want['res5']).abs().max()):.3e}, misses {worst[:5]}")
    assert not worst, worst[:10]


def test_trunk_switch_on_launches_the_kernels(monkeypatch):
    """the switch is not a no-op: with it on the trunk calls the three entry points, 3 per block + the stem's one"""
    trunk, _, x, _, _ = _trunk_case(50)
    counts = {"epilogue": 0, "pool": 0}
    real_e, real_p = G.conv_epilogue, G.stem_pool
    monkeypatch.setattr(G, "conv_epilogue", lambda *a: counts.__setitem__("epilogue", counts["epilogue"] + 1) or real_e(*a))
    monkeypatch.setattr(G, "stem_pool", lambda *a: counts.__setitem__("pool", counts["pool"] + 1) or real_p(*a))
    trunk.eval()
    trunk.fused_glue = True
    with torch.no_grad():
        trunk(x.to(DEV))
    trunk.fused_glue = False
    assert counts == {"epilogue": 48, "pool": 1}
    with torch.no_grad():
        trunk(x.to(DEV))
    assert counts == {"epilogue": 48, "pool": 1}
    # a 16-bit training step keeps the eager tail: 2 epilogues per block; fp32 training and 16-bit without grad take all 3
    for autocast, grad, want in ((True, True, 32), (False, True, 48), (True, False, 48)):
        counts.update(epilogue=0, pool=0)
        trunk.fused_glue = True
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast), torch.set_grad_enabled(grad):
            trunk(x.to(DEV))
        trunk.fused_glue = False
        assert counts == {"epilogue": want, "pool": 1}, (autocast, grad)


def test_the_three_ops_inside_a_captured_graph():
    shape = (2, 16, 6, 10)
    y_in = [_values(shape, torch.float32, 1000 + i, special=False) for i in range(2)]
    r_in = [_values(shape, torch.float32, 1010 + i, special=False) for i in range(2)]
    g_in = [_values(shape, torch.float32, 1020 + i, special=False) for i in range(2)]
    b, rb = torch.randn(16, device=DEV), torch.randn(16, device=DEV)
    sy, sr, sg = y_in[0].clone(), r_in[0].clone(), g_in[0].clone()
    work, grad_in = torch.empty_like(sy), torch.empty_like(sy)
    lib = _lib.lib()

    def body():
        work.copy_(sy)
        out = G.conv_epilogue(work, b, sr, rb)
        _lib.check(lib.vnx_conv_epilogue_backward(_lib.VNX_F32, sg.data_ptr(), out.data_ptr(), grad_in.data_ptr(),
                                                  out.numel(), _lib.current_stream(out)))
        return out, G.stem_pool(sy, b)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side), torch.no_grad():
        body()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.no_grad(), torch.cuda.graph(graph):
        out, pooled = body()
    for i in (1, 0):
        sy.copy_(y_in[i]); sr.copy_(r_in[i]); sg.copy_(g_in[i])
        graph.replay()
        with torch.no_grad():
            want = G.conv_epilogue(y_in[i].clone(), b, r_in[i], rb)
            assert torch.equal(out, want) and torch.equal(out, G.conv_epilogue_reference(y_in[i], b, r_in[i], rb))
            assert torch.equal(grad_in, g_in[i] * (want > 0))
            assert torch.equal(pooled, G.stem_pool(y_in[i], b)) and torch.equal(pooled, G.stem_pool_reference(y_in[i], b))
