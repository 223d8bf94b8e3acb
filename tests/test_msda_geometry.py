"""MSDA backward at geometries other than the default models' 4 levels x 4 points: the self-decoding grad_value kernel
(vnext_amd/csrc/msda_d32_gvdirect.hip) with 5 to 64 points, one to eight levels, query counts around a pass
(min(304, 1216 / P) queries) and batch x heads on both sides of gvd_units_min's switch -- the geometries where a unit's
rows may need more slots than the walk's 768 (gvd_level_split, msda_units.h; the host side of it: test_gvdirect_model.py).

Everything through the C ABI (vnx_msda_backward, and vnx_msda_fused_backward where L * P == 16) into buffers prefilled
with NaN between guard words: every element must be written, finite and next to the fp64 C oracle, and no guard word may
change.  grad_value is held per level, each against its own largest element: a coarse level's rows are few, and a global
scale would hide them behind a fine level's.  Last, MSDeformAttn with 8 points at the decoder's shape against the same
module in float64 through the grid_sample statement (oracle/msda_torch_fallback.py).
Reference semantics: ms_deform_im2col_cuda.cuh:87-159 (scatter), :253-298 (decode)."""
import copy
import math
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu

from oracle import msda_oracle as O  # noqa: E402
from vnext_amd import _lib  # noqa: E402

DEV = "cuda:0"
QC = 304                                                   # kGvdQc (msda_units.h)
P360 = [(48, 80), (24, 40), (12, 20), (6, 10)]
P360_8 = P360 + [(3, 5), (2, 3), (1, 2), (1, 1)]
GUARD = 256                                                # elements before and after every output buffer
SENTINEL = -1234.5
CODE = {torch.float32: _lib.VNX_F32, torch.bfloat16: _lib.VNX_BF16, torch.float16: _lib.VNX_F16}
TOL16 = {torch.bfloat16: 8e-3, torch.float16: 2e-3}       # test_msda_gvdirect.py::test_sixteen_bit_values


def pass_queries(P):
    return min(QC, 4 * QC // P)


def make_case(shapes, B, M, Lq, P, seed, centre=None):
    """locations uniform over a square a little larger than the map (some samples outside), softmax weights"""
    g = torch.Generator().manual_seed(seed)
    sh = torch.tensor(shapes, dtype=torch.long)
    L = len(shapes)
    S = int(sh.prod(1).sum())
    lsi = torch.cat((sh.new_zeros((1,)), sh.prod(1).cumsum(0)[:-1]))
    value = torch.randn(B, S, M, 32, generator=g)
    loc = torch.rand(B, Lq, M, L, P, 2, generator=g) * 1.2 - 0.1
    if centre is not None:
        loc = centre + 0.004 * torch.rand(B, Lq, M, L, P, 2, generator=g)
    attn = torch.softmax(torch.randn(B, Lq, M, L * P, generator=g), -1).view(B, Lq, M, L, P)
    go = torch.randn(B, Lq, M * 32, generator=g)
    return sh, lsi, value, loc.contiguous(), attn.contiguous(), go


class Guarded:
    """a NaN-filled output between two runs of guard words"""

    def __init__(self, shape, dtype):
        self.n, self.dtype = math.prod(shape), dtype
        self.buf = torch.full((self.n + 2 * GUARD,), float("nan"), dtype=dtype, device=DEV)
        self.buf[:GUARD] = SENTINEL
        self.buf[GUARD + self.n:] = SENTINEL
        self.view = self.buf[GUARD:GUARD + self.n].view(shape)

    def ptr(self):
        return self.view.data_ptr()

    def read(self, name):
        s = torch.tensor(SENTINEL, dtype=self.dtype, device=DEV)
        assert bool((self.buf[:GUARD] == s).all()), f"{name}: a guard word before the buffer was overwritten"
        assert bool((self.buf[GUARD + self.n:] == s).all()), f"{name}: a guard word after the buffer was overwritten"
        nan = int(torch.isnan(self.view).sum())
        assert nan == 0, f"{name}: {nan} of {self.n} elements never written"
        assert bool(torch.isfinite(self.view).all()), f"{name}: non-finite elements"
        return self.view.double().cpu().numpy()


def scale(x):
    return max(1e-30, float(np.abs(x).max()))


def boundary_mask(loc, sh, eps=1e-4):
    """samples not within eps pixels of a pixel line: there the bilinear gradient jumps, and fp32 and fp64 may disagree
    on the side.  The lines themselves are tested in test_msda_lattice.py, on power-of-two maps where the two agree."""
    wh = torch.stack([sh[:, 1], sh[:, 0]], -1).double().view(1, 1, 1, -1, 1, 2)
    px = loc.double() * wh - 0.5
    return ((px - px.round()).abs() > eps).all(-1, keepdim=True).numpy()


def assert_levels(gv, rv, sh, lsi, tol):
    """grad_value [B, S, M, 32] level by level, each scaled by its own largest element"""
    for l, (h, w) in enumerate(sh.tolist()):
        s0 = int(lsi[l])
        got, want = gv[:, s0:s0 + h * w], rv[:, s0:s0 + h * w]
        np.testing.assert_allclose(got, want, rtol=0, atol=tol * scale(want), err_msg=f"grad_value, level {l} ({h} x {w})")


def plain_backward(case, vdt=torch.float32, ldt=torch.float32):
    sh, lsi, value, loc, attn, go = case
    B, S, M, D = value.shape
    _, Lq, _, L, P, _ = loc.shape
    v, lo, a, g = value.to(DEV, vdt), loc.to(DEV, ldt), attn.to(DEV, ldt), go.to(DEV, vdt)
    shd, lsid = sh.to(DEV), lsi.to(DEV)
    outs = [Guarded(value.shape, vdt), Guarded(loc.shape, ldt), Guarded(attn.shape, ldt)]
    lib = _lib.lib()
    flags = _lib.MSDA_LEVELS_PACKED
    n = lib.vnx_msda_backward_workspace_bytes(CODE[vdt], CODE[ldt], B, S, M, D, L, Lq, P, flags)
    assert n == 0, "below 1 024 queries with packed levels the self-decoding grad_value kernel runs, without workspace"
    st = lib.vnx_msda_backward(CODE[vdt], CODE[ldt], v.data_ptr(), shd.data_ptr(), lsid.data_ptr(), lo.data_ptr(), a.data_ptr(),
                               g.data_ptr(), outs[0].ptr(), outs[1].ptr(), outs[2].ptr(), B, S, M, D, L, Lq, P, flags, None, 0,
                               torch.cuda.current_stream().cuda_stream)
    _lib.check(st)
    torch.cuda.synchronize()
    return [o.read(name) for o, name in zip(outs, ("grad_value", "grad_sampling_loc", "grad_attn_weight"))]


def oracle(case, vdt=torch.float32, ldt=torch.float32):
    sh, lsi, value, loc, attn, go = case
    return O.msda_backward(value.to(vdt).double().numpy(), sh.numpy(), lsi.numpy(), loc.to(ldt).double().numpy(),
                           attn.to(ldt).double().numpy(), go.to(vdt).double().numpy(), nthreads=8)


def check_fp32(case, tol=2e-5):
    gv, gl, ga = plain_backward(case)
    rv, rl, ra = oracle(case)
    sh, lsi = case[0], case[1]
    assert_levels(gv, rv, sh, lsi, tol)
    ok = boundary_mask(case[3], sh)
    np.testing.assert_allclose(gl * ok, rl * ok, rtol=0, atol=tol * scale(rl), err_msg="grad_sampling_loc")
    np.testing.assert_allclose(ga, ra, rtol=0, atol=tol * scale(ra), err_msg="grad_attn_weight")


# ---- the two geometries worked out in the issue: rows past slot 768 of a unit were never stored -------------------------
@pytest.mark.parametrize("B,M", [(2, 4), (10, 8)])
def test_one_level_of_1100_pixels_at_16_points(B, M):
    """25 x 44 = 1 100 pixels in two units of 550 rows; 4 x 16 x 300 taps made the rows take two groups each (1 100 slots)"""
    check_fp32(make_case([(25, 44)], B, M, 300, 16, seed=B * M))


@pytest.mark.parametrize("B", [5, 10])
def test_360p_pyramid_at_8_points(B):
    """B x M = 80: one unit per small level, the 240-pixel one's rows on four groups (960 slots) before the fix; B x M = 40:
    the small levels cut in two"""
    check_fp32(make_case(P360, B, 8, 300, 8, seed=B))


# ---- point counts, level counts, query counts ---------------------------------------------------------------------------
@pytest.mark.parametrize("L,P", [(4, 5), (4, 8), (4, 16), (2, 32), (1, 64), (8, 8)])
def test_point_counts(L, P):
    check_fp32(make_case(P360_8[:L], 2, 8, 300, P, seed=L * 100 + P))


@pytest.mark.parametrize("P", [8, 16])
@pytest.mark.parametrize("which", ["1", "qc-1", "qc", "qc+1", "300", "1023"])
def test_query_counts_around_a_pass(P, which):
    """one pass, exactly one, one query into a second, and several (1 023 at 16 points: 14 passes of 76)"""
    qc = pass_queries(P)
    Lq = {"1": 1, "qc-1": qc - 1, "qc": qc, "qc+1": qc + 1, "300": 300, "1023": 1023}[which]
    check_fp32(make_case(P360, 2, 8, Lq, P, seed=P * 1000 + Lq))


@pytest.mark.parametrize("L,P", [(1, 16), (4, 16)])
def test_every_sample_on_one_spot(L, P):
    """every tap of a pass on four pixels of each level: one row's segment is the whole sorted list (4 x P x qc taps)"""
    check_fp32(make_case(P360[:L], 2, 4, 300, P, seed=7, centre=0.37), tol=4e-5)


# ---- 16-bit values -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geometry", ["360p-P8-B10", "25x44-P16"])
@pytest.mark.parametrize("vdt", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("loc16", [False, True])
def test_sixteen_bit_values(geometry, vdt, loc16):
    case = make_case(P360, 10, 8, 300, 8, seed=21) if geometry == "360p-P8-B10" else make_case([(25, 44)], 2, 8, 300, 16, seed=22)
    ldt = vdt if loc16 else torch.float32
    gv, gl, ga = plain_backward(case, vdt, ldt)
    rv, rl, ra = oracle(case, vdt, ldt)
    tol = TOL16[vdt]
    assert_levels(gv, rv, case[0], case[1], tol)
    np.testing.assert_allclose(ga, ra, rtol=0, atol=(3e-2 if loc16 else tol) * scale(ra), err_msg="grad_attn_weight")


# ---- levels x points == 16: the plain and the fused backward ------------------------------------------------------------
def fused_inputs(shapes, B, M, Lq, P, seed):
    g = torch.Generator().manual_seed(seed)
    L = len(shapes)
    S = sum(h * w for h, w in shapes)
    value = torch.randn(B, S, M, 32, generator=g)
    offsets = torch.randn(B, Lq, M, L, P, 2, generator=g) * 2.0
    logits = torch.randn(B, Lq, M, L * P, generator=g) * 2
    ref = torch.rand(B, Lq, L, 2, generator=g)
    go = torch.randn(B, Lq, M * 32, generator=g)
    return value, offsets, logits, ref, go


def compose64(shapes, offsets, logits, ref):
    """the module's expressions in float64 (IDOL ops/modules/ms_deform_attn.py:99-108, 2-d reference points)"""
    B, Lq, M, L, P, _ = offsets.shape
    attn = torch.softmax(logits.double(), -1).view(B, Lq, M, L, P)
    norm = torch.tensor([[w, h] for h, w in shapes], dtype=torch.float64)
    loc = ref.double()[:, :, None, :, None, :] + offsets.double() / norm[None, None, None, :, None, :]
    return loc, attn, norm


@pytest.mark.parametrize("L,P", [(1, 16), (2, 8), (8, 2)])
@pytest.mark.parametrize("B", [2, 10])
def test_sixteen_samples_per_head_plain(L, P, B):
    check_fp32(make_case(P360_8[:L], B, 8, 300, P, seed=B * 10 + L))


@pytest.mark.parametrize("L,P", [(1, 16), (2, 8), (8, 2), (4, 4)])
@pytest.mark.parametrize("B", [2, 10])
@pytest.mark.parametrize("vdt", [torch.float32, torch.bfloat16])
def test_sixteen_samples_per_head_fused(L, P, B, vdt):
    """vnx_msda_fused_backward (softmax and locations inside the kernels; fp32 queries): grad_value from the decoded
    locations the grad_loc kernel leaves (compact layout), the offsets', logits' and reference points' gradients"""
    shapes = P360_8[:L] if L != 1 else [(25, 44)]
    M, Lq = 8, 300
    value, offsets, logits, ref, go = fused_inputs(shapes, B, M, Lq, P, seed=B * 100 + L * 10 + P)
    S = value.shape[1]
    from vnext_amd.ops.functions import level_tensors
    shd, lsid = level_tensors(shapes, DEV)
    v, off, lg, rf, g = value.to(DEV, vdt), offsets.to(DEV), logits.to(DEV), ref.to(DEV), go.to(DEV, vdt)
    outs = [Guarded(value.shape, vdt), Guarded(offsets.shape, torch.float32), Guarded(logits.shape, torch.float32),
            Guarded((B, Lq, L, 2), torch.float32)]
    lib = _lib.lib()
    n = lib.vnx_msda_fused_backward_workspace_bytes(CODE[vdt], B, S, M, L, Lq, P)
    ws = torch.empty(max(n, 1), dtype=torch.uint8, device=DEV)
    st = lib.vnx_msda_fused_backward(CODE[vdt], _lib.VNX_F32, v.data_ptr(), shd.data_ptr(), lsid.data_ptr(), off.data_ptr(),
                                     lg.data_ptr(), rf.data_ptr(), g.data_ptr(), outs[0].ptr(), outs[1].ptr(), outs[2].ptr(),
                                     outs[3].ptr(), B, S, M, 32, L, Lq, P, 2, 1, ws.data_ptr(), n,
                                     torch.cuda.current_stream().cuda_stream)
    _lib.check(st)
    torch.cuda.synchronize()
    gv, goff, glog, gref = [o.read(k) for o, k in zip(outs, ("grad_value", "grad_offsets", "grad_logits", "grad_reference"))]

    loc64, attn64, norm = compose64(shapes, offsets, logits, ref)
    sh = torch.tensor(shapes, dtype=torch.long)
    lsi = torch.cat((sh.new_zeros((1,)), sh.prod(1).cumsum(0)[:-1]))
    rv, rl, ra = O.msda_backward(value.to(vdt).double().numpy(), sh.numpy(), lsi.numpy(), loc64.numpy(), attn64.numpy(),
                                 go.to(vdt).double().numpy(), nthreads=8)
    a = attn64.numpy().reshape(B, Lq, M, L * P)
    ga = ra.reshape(B, Lq, M, L * P)
    rlog = a * (ga - (a * ga).sum(-1, keepdims=True))
    roff = rl / norm.numpy()[None, None, None, :, None, :]
    tol = 2e-5 if vdt == torch.float32 else 1e-2
    assert_levels(gv, rv, sh, lsi, tol if vdt == torch.float32 else TOL16[vdt])
    ok = boundary_mask(loc64, sh, 1e-4 if vdt == torch.float32 else 1e-3)
    np.testing.assert_allclose(goff * ok, roff * ok, rtol=0, atol=tol * scale(roff), err_msg="grad_offsets")
    np.testing.assert_allclose(glog, rlog, rtol=0, atol=tol * scale(rlog), err_msg="grad_logits")
    # the reference point of (batch, query, level) gathers the location gradients of all its heads and points
    ok_ref = ok.reshape(B, Lq, M, L, P).all(axis=(2, 4))[..., None]
    rref = rl.sum(axis=(2, 4))
    np.testing.assert_allclose(gref * ok_ref, rref * ok_ref, rtol=0, atol=tol * scale(rref), err_msg="grad_reference_points")


# ---- the module ---------------------------------------------------------------------------------------------------------
def test_module_with_8_points_at_the_decoder_shape(monkeypatch):
    """MSDeformAttn(n_points=8): 10 frames, 300 queries, the 360p pyramid -- the decoder call whose 240-pixel level lost
    rows 192-239 of every (frame, head).  Forward and every gradient against the module in float64 through grid_sample.
    Every sample lies at least 0.05 pixels from a pixel line (reference points on pixel centres, offsets of integer + 0.25
    pixels plus less than 0.2 from the query), so fp32 and fp64 agree on every bilinear cell."""
    from oracle.msda_torch_fallback import msda_grid_sample
    from vnext_amd.ops.functions import level_tensors
    from vnext_amd.ops.modules import ms_deform_attn as mod

    B, Lq, C, M, L, P = 10, 300, 256, 8, 4, 8
    g = torch.Generator().manual_seed(8)
    m = mod.MSDeformAttnIDOL(C, L, M, P)
    with torch.no_grad():
        m.sampling_offsets.bias.copy_(m.sampling_offsets.bias.round() + 0.25)
        m.sampling_offsets.weight.copy_((torch.rand(m.sampling_offsets.weight.shape, generator=g) * 2 - 1) * (0.18 / C))
        m.attention_weights.weight.copy_(torch.randn(m.attention_weights.weight.shape, generator=g) * 0.05)
        m.attention_weights.bias.copy_(torch.randn(m.attention_weights.bias.shape, generator=g) * 0.5)
        m.value_proj.bias.copy_(torch.randn(C, generator=g) * 0.1)
        m.output_proj.bias.copy_(torch.randn(C, generator=g) * 0.1)
    S = sum(h * w for h, w in P360)
    query = torch.rand(B, Lq, C, generator=g) * 2 - 1                 # |offset - bias| <= 0.18 px
    src = torch.randn(B, S, C, generator=g)
    ref = torch.empty(B, Lq, L, 2)
    for l, (h, w) in enumerate(P360):
        ref[:, :, l, 0] = (torch.randint(0, w, (B, Lq), generator=g).float() + 0.5) / w
        ref[:, :, l, 1] = (torch.randint(0, h, (B, Lq), generator=g).float() + 0.5) / h
    go = torch.randn(B, Lq, C, generator=g)

    def run(module, dev, dtype, shapes, lsi):
        leaves = [t.to(dev, dtype).requires_grad_(True) for t in (query, ref, src)]
        out, loc, _ = module(leaves[0], leaves[1], leaves[2], shapes, lsi)
        out.backward(go.to(dev, dtype))
        return out, loc, leaves

    m_gpu = copy.deepcopy(m).to(DEV)
    shd, lsid = level_tensors(P360, DEV)
    out, _, leaves = run(m_gpu, DEV, torch.float32, shd, lsid)
    torch.cuda.synchronize()

    class GridSample:
        @staticmethod
        def apply(value, shapes_, lsi_, loc, attn, step):
            return msda_grid_sample(value, shapes_, loc, attn)

    monkeypatch.setattr(mod, "MSDeformAttnFunction", GridSample)
    m64 = copy.deepcopy(m).double()
    sh = torch.tensor(P360, dtype=torch.long)
    lsi = torch.cat((sh.new_zeros((1,)), sh.prod(1).cumsum(0)[:-1]))
    out64, loc64, leaves64 = run(m64, "cpu", torch.float64, sh, lsi)
    px = loc64.detach() * torch.tensor([[w, h] for h, w in P360], dtype=torch.float64)[None, None, None, :, None, :] - 0.5
    assert float((px - px.round()).abs().min()) >= 0.05           # the construction above holds

    def close(got, want, tol, what):
        want = want.detach().numpy()
        np.testing.assert_allclose(got.detach().double().cpu().numpy(), want, rtol=0, atol=tol * scale(want), err_msg=what)

    close(out, out64, 2e-5, "output")
    close(leaves[0].grad, leaves64[0].grad, 5e-5, "grad query")
    close(leaves[1].grad, leaves64[1].grad, 5e-5, "grad reference_points")
    gsrc, gsrc64 = leaves[2].grad, leaves64[2].grad
    for l, (h, w) in enumerate(P360):
        s0 = int(lsi[l])
        close(gsrc[:, s0:s0 + h * w], gsrc64[:, s0:s0 + h * w], 5e-5, f"grad input_flatten, level {l} ({h} x {w})")
    for (n1, p1), (n2, p2) in zip(m_gpu.named_parameters(), m64.named_parameters()):
        assert n1 == n2 and p1.grad is not None and p2.grad is not None, n1
        close(p1.grad, p2.grad, 1e-4, n1)
