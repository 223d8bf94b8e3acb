"""Parity checks the round-1 review asked for ("Close the parity gaps"):
(a) FULL tensors -- every query, all three gradients -- against the oracle at the BASELINE shapes
    decoder-360p (the headline), decoder-720p and encoder-360p, fp32;
(b) bf16 forward and backward at decoder-720p (BASELINE config 3) within the north star's 1e-2;
(c) the grid_sample statement of the reference's fallback (the CPU baseline of bench.py) against the
    golden vectors generated from the reference;
(d) the reference-side binding printed in INTEGRATION.md section 2, executed verbatim."""
import os
import re
import types

import numpy as np
import pytest
import torch

from conftest import ROOT, golden_names, load_golden
from oracle import msda_oracle as O

S360 = [(48, 80), (24, 40), (12, 20), (6, 10)]
S720 = [(92, 160), (46, 80), (23, 40), (12, 20)]
DEV = "cuda:0"


def case(shapes, B, Lq, seed, uniform=True):
    g = torch.Generator().manual_seed(seed)
    sh = torch.tensor(shapes, dtype=torch.long)
    S = int(sh.prod(1).sum())
    lsi = torch.cat((sh.new_zeros((1,)), sh.prod(1).cumsum(0)[:-1]))
    value = torch.randn(B, S, 8, 32, generator=g)
    if uniform:
        loc = torch.rand(B, Lq, 8, 4, 4, 2, generator=g)
    else:
        ref = torch.rand(B, Lq, 1, 1, 1, 2, generator=g)
        wh = torch.stack([sh[:, 1], sh[:, 0]], -1).float().view(1, 1, 1, 4, 1, 2)
        loc = (ref + 3.0 * torch.randn(B, Lq, 8, 4, 4, 2, generator=g) / wh).contiguous()
    attn = torch.softmax(torch.randn(B, Lq, 8, 16, generator=g), -1).view(B, Lq, 8, 4, 4).contiguous()
    go = torch.randn(B, Lq, 256, generator=g)
    return sh, lsi, value, loc, attn, go


def scale(x):
    return max(1e-30, float(np.abs(x).max()))


def off_the_pixel_grid(loc, sh, eps=1e-4):
    """[B,Lq,M,L,P,1] mask of samples whose pixel coordinates are at least `eps` away from an integer.  The
    gradient with respect to the location is discontinuous across a pixel boundary (another pair of taps takes
    over), so a sample that fp32 and fp64 arithmetic put on different sides has no common reference value
    there; everything else the op produces is continuous in the location.  The lines themselves are tested in
    test_msda_lattice.py, on power-of-two maps where fp32 and fp64 agree on the side."""
    wh = torch.stack([sh[:, 1], sh[:, 0]], -1).double().view(1, 1, 1, -1, 1, 2)
    px = loc.double() * wh - 0.5
    return ((px - px.round()).abs() > eps).all(-1, keepdim=True).numpy()


# ----------------------------------------------------------------------------------- (a) full tensors
@pytest.mark.gpu
@pytest.mark.parametrize("name,shapes,Lq,uniform", [
    ("decoder_360p", S360, 300, True),        # the headline shape
    ("decoder_720p", S720, 300, True),
    ("encoder_360p", S360, 5100, False),
])
def test_full_tensors_all_gradients_fp32(name, shapes, Lq, uniform):
    import MultiScaleDeformableAttention as MSDA
    B = 5 if Lq == 300 else 2
    sh, lsi, value, loc, attn, go = case(shapes, B, Lq, seed=23, uniform=uniform)
    dv, ds, di, dl, da, dg = (t.to(DEV) for t in (value, sh, lsi, loc, attn, go))
    out = MSDA.ms_deform_attn_forward(dv, ds, di, dl, da, 64)
    gv, gl, ga = MSDA.ms_deform_attn_backward(dv, ds, di, dl, da, dg, 64)
    torch.cuda.synchronize()
    args = (value.double().numpy(), sh.numpy(), lsi.numpy(), loc.double().numpy(), attn.double().numpy())
    want = O.msda_forward(*args, nthreads=8)
    rv, rl, ra = O.msda_backward(*args, go.double().numpy(), nthreads=8)
    np.testing.assert_allclose(out.double().cpu().numpy(), want, rtol=0, atol=1e-5 * scale(want))
    np.testing.assert_allclose(gv.double().cpu().numpy(), rv, rtol=0, atol=2e-5 * scale(rv))
    ok = off_the_pixel_grid(loc, sh)
    assert ok.mean() > 0.999
    np.testing.assert_allclose(gl.double().cpu().numpy() * ok, rl * ok, rtol=0, atol=2e-5 * scale(rl))
    np.testing.assert_allclose(ga.double().cpu().numpy(), ra, rtol=0, atol=2e-5 * scale(ra))
    # and the reference's own criterion for the forward (ops/test.py:56)
    assert np.allclose(out.cpu().numpy(), want, rtol=1e-2, atol=1e-3)


# -------------------------------------------------------------------------------------- (b) bf16, config 3
@pytest.mark.gpu
@pytest.mark.parametrize("loc_bf16", [False, True])
def test_bf16_forward_backward_decoder_720p(loc_bf16):
    """IDOL 720p pair in bf16: value / grad_out bf16, locations fp32 (autocast) or bf16.  Tolerance 1e-2 of
    each tensor's scale (north star), against the fp64 oracle fed with the SAME rounded inputs."""
    import MultiScaleDeformableAttention as MSDA
    sh, lsi, value, loc, attn, go = case(S720, 2, 300, seed=31)
    ld = torch.bfloat16 if loc_bf16 else torch.float32
    v16, g16 = value.bfloat16(), go.bfloat16()
    l_in, a_in = loc.to(ld), attn.to(ld)
    out = MSDA.ms_deform_attn_forward(v16.to(DEV), sh.to(DEV), lsi.to(DEV), l_in.to(DEV), a_in.to(DEV), 64)
    gv, gl, ga = MSDA.ms_deform_attn_backward(v16.to(DEV), sh.to(DEV), lsi.to(DEV), l_in.to(DEV), a_in.to(DEV), g16.to(DEV), 64)
    torch.cuda.synchronize()
    assert out.dtype == gv.dtype == torch.bfloat16 and gl.dtype == ga.dtype == ld
    args = (v16.double().numpy(), sh.numpy(), lsi.numpy(), l_in.double().numpy(), a_in.double().numpy())
    want = O.msda_forward(*args, nthreads=8)
    rv, rl, ra = O.msda_backward(*args, g16.double().numpy(), nthreads=8)
    for got, ref in ((out, want), (gv, rv), (gl, rl), (ga, ra)):
        np.testing.assert_allclose(got.double().cpu().numpy(), ref, rtol=0, atol=1e-2 * scale(ref))


# ------------------------------------------------------------------------- (c) the CPU-baseline technique
@pytest.mark.parametrize("name", [n for n in golden_names() if "d1025" not in n and "d2048" not in n and "d3096" not in n])
def test_grid_sample_fallback_matches_the_reference_goldens(name):
    """oracle/msda_torch_fallback.py is what bench.py times as the reference's pure-PyTorch path and what the
    CPU model tests use as the op: hold it to the vectors generated from the reference function itself."""
    from oracle.msda_torch_fallback import msda_grid_sample
    g = load_golden(name)
    v, l, a = (torch.from_numpy(np.ascontiguousarray(g[k])).double().requires_grad_(True) for k in ("value", "loc", "attn"))
    out = msda_grid_sample(v, g["shapes"], l, a)
    np.testing.assert_allclose(out.detach().numpy(), g["out_f64"], rtol=1e-9, atol=1e-12 * scale(g["out_f64"]))
    if "grad_out" in g and "grad_loc" in g:
        out.backward(torch.from_numpy(np.ascontiguousarray(g["grad_out"])).double())
        np.testing.assert_allclose(l.grad.numpy(), g["grad_loc"], rtol=1e-8, atol=1e-11 * scale(g["grad_loc"]))
        np.testing.assert_allclose(a.grad.numpy(), g["grad_attn"], rtol=1e-8, atol=1e-11 * scale(g["grad_attn"]))
        if "grad_value" in g:
            np.testing.assert_allclose(v.grad.numpy(), g["grad_value"], rtol=1e-8, atol=1e-11 * scale(g["grad_value"]))


@pytest.mark.parametrize("name", [n for n in golden_names() if "d1025" not in n and "d2048" not in n and "d3096" not in n])
def test_frame_loop_fallback_matches_the_reference_goldens(name):
    """msda_core_frames -- the reference's function as the module's frame loop drives it, what bench.py reports as
    `cpu_baseline.value` since round 5 -- on the same vectors, every batch element presented as a frame of one clip."""
    from oracle.msda_torch_fallback import msda_core_frames
    g = load_golden(name)
    v, l, a = (torch.from_numpy(np.ascontiguousarray(g[k])).double().requires_grad_(True) for k in ("value", "loc", "attn"))
    sizes = [tuple(int(x) for x in hw) for hw in g["shapes"]]
    out = msda_core_frames(v.unsqueeze(0), sizes, l.unsqueeze(0), a.unsqueeze(0))[0]
    np.testing.assert_allclose(out.detach().numpy(), g["out_f64"], rtol=1e-9, atol=1e-12 * scale(g["out_f64"]))
    if "grad_out" in g and "grad_loc" in g:
        out.backward(torch.from_numpy(np.ascontiguousarray(g["grad_out"])).double())
        np.testing.assert_allclose(l.grad.numpy(), g["grad_loc"], rtol=1e-8, atol=1e-11 * scale(g["grad_loc"]))
        np.testing.assert_allclose(a.grad.numpy(), g["grad_attn"], rtol=1e-8, atol=1e-11 * scale(g["grad_attn"]))
        if "grad_value" in g:
            np.testing.assert_allclose(v.grad.numpy(), g["grad_value"], rtol=1e-8, atol=1e-11 * scale(g["grad_value"]))


# --------------------------------------------------------------------------- (d) the INTEGRATION.md stub
def integration_stub_source():
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    blocks = re.findall(r"```python\n(.*?)```", text, flags=re.S)
    stub = [b for b in blocks if "_msda_hip.py" in b]
    assert len(stub) == 1, "INTEGRATION.md section 2 must hold exactly one reference-side stub"
    return stub[0]


def test_integration_stub_is_present_and_self_contained():
    src = integration_stub_source()
    compile(src, "INTEGRATION.md:_msda_hip.py", "exec")
    assert "vnx_msda_forward" in src and "vnx_msda_backward" in src and "import vnext_amd" not in src


@pytest.mark.gpu
def test_integration_stub_runs_verbatim_under_the_reference_function():
    """Execute the stub text exactly as printed (only the library path resolves to the in-tree build) and drive
    it the way the reference's MSDeformAttnFunction does (ops/functions/ms_deform_attn_func.py:21-39)."""
    from torch.autograd import Function
    from torch.autograd.function import once_differentiable
    from vnext_amd import _lib
    src = integration_stub_source()
    assert 'ctypes.CDLL("libvnext_hip.so")' in src
    mod = types.ModuleType("_msda_hip")
    import ctypes
    real_cdll = ctypes.CDLL
    ctypes.CDLL = lambda name, *a, **k: real_cdll(_lib.LIB_PATH if name == "libvnext_hip.so" else name, *a, **k)
    try:
        exec(compile(src, "INTEGRATION.md:_msda_hip.py", "exec"), mod.__dict__)
    finally:
        ctypes.CDLL = real_cdll
    MSDA = mod

    class MSDeformAttnFunction(Function):          # the reference's class body, func.py:21-39
        @staticmethod
        def forward(ctx, value, value_spatial_shapes, value_level_start_index, sampling_locations, attention_weights,
                    im2col_step):
            ctx.im2col_step = im2col_step
            output = MSDA.ms_deform_attn_forward(value, value_spatial_shapes, value_level_start_index,
                                                 sampling_locations, attention_weights, ctx.im2col_step)
            ctx.save_for_backward(value, value_spatial_shapes, value_level_start_index, sampling_locations,
                                  attention_weights)
            return output

        @staticmethod
        @once_differentiable
        def backward(ctx, grad_output):
            value, value_spatial_shapes, value_level_start_index, sampling_locations, attention_weights = ctx.saved_tensors
            grad_value, grad_sampling_loc, grad_attn_weight = MSDA.ms_deform_attn_backward(
                value, value_spatial_shapes, value_level_start_index, sampling_locations, attention_weights,
                grad_output.contiguous(), ctx.im2col_step)
            return grad_value, None, None, grad_sampling_loc, grad_attn_weight, None

    sh, lsi, value, loc, attn, go = case([(12, 20), (6, 10), (3, 5), (2, 3)], 2, 37, seed=4)
    v, l, a = (t.to(DEV).requires_grad_(True) for t in (value, loc, attn))
    out = MSDeformAttnFunction.apply(v, sh.to(DEV), lsi.to(DEV), l, a, 64)
    out.backward(go.to(DEV))
    torch.cuda.synchronize()
    args = (value.double().numpy(), sh.numpy(), lsi.numpy(), loc.double().numpy(), attn.double().numpy())
    want = O.msda_forward(*args)
    rv, rl, ra = O.msda_backward(*args, go.double().numpy())
    np.testing.assert_allclose(out.detach().double().cpu().numpy(), want, rtol=0, atol=1e-5 * scale(want))
    np.testing.assert_allclose(v.grad.double().cpu().numpy(), rv, rtol=0, atol=2e-5 * scale(rv))
    np.testing.assert_allclose(l.grad.double().cpu().numpy(), rl, rtol=0, atol=2e-5 * scale(rl))
    np.testing.assert_allclose(a.grad.double().cpu().numpy(), ra, rtol=0, atol=2e-5 * scale(ra))
