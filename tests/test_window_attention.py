"""The fused shifted-window attention (vnext_amd/csrc/window_attn.hip, ops/window_attention.py) against a float64 torch
expression of the reference's block (pad after norm1, roll, partition, relative-position bias, SW-MSA mask, softmax, reverse,
inverse roll, crop): outputs, grad_qkv, the table gradient and the qkv-bias gradient including the padded tokens; the
backward's determinism; guard words around every buffer; the shapes the kernel refuses."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from vnext_amd import _lib
from vnext_amd.models.swin import relative_position_index
from vnext_amd.ops.window_attention import _WindowAttention, shift_mask, window_partition, window_reverse

HD = 32


def reference_core(qkv, bias, table, B, H, W, heads, w, s, scale):
    """float64: qkv [B*H*W, 3C] without bias -> context [B*H*W, C], the reference's way"""
    C = heads * HD
    x = qkv.view(B, H, W, 3 * C)
    pad_r, pad_b = (w - W % w) % w, (w - H % w) % w
    x = F.pad(x, (0, 0, 0, pad_r, 0, pad_b)) + bias            # a padded token's q / k / v: the bias
    Hp, Wp = x.shape[1], x.shape[2]
    if s > 0:
        x = torch.roll(x, shifts=(-s, -s), dims=(1, 2))
    xw = window_partition(x, w).view(-1, w * w, 3 * C)
    Bn, N = xw.shape[:2]
    q, k, v = xw.view(Bn, N, 3, heads, HD).permute(2, 0, 3, 1, 4)
    a = (q * scale) @ k.transpose(-2, -1)
    idx = relative_position_index(w).to(qkv.device)
    a = a + table[idx.view(-1)].view(N, N, -1).permute(2, 0, 1).unsqueeze(0)
    if s > 0:
        mask = shift_mask(Hp, Wp, w, s, qkv.device, qkv.dtype)
        nW = mask.shape[0]
        a = (a.view(Bn // nW, nW, heads, N, N) + mask.unsqueeze(1).unsqueeze(0)).view(-1, heads, N, N)
    o = (a.softmax(-1) @ v).transpose(1, 2).reshape(Bn, w, w, C)
    o = window_reverse(o, w, Hp, Wp)
    if s > 0:
        o = torch.roll(o, shifts=(s, s), dims=(1, 2))
    return o[:, :H, :W, :].reshape(B * H * W, C)


def _inputs(B, H, W, heads, w, seed):
    g = torch.Generator().manual_seed(seed)
    C = heads * HD
    qkv = torch.randn(B * H * W, 3 * C, generator=g, dtype=torch.float64)
    bias = torch.randn(3 * C, generator=g, dtype=torch.float64)
    table = 2.0 * torch.randn((2 * w - 1) ** 2, heads, generator=g, dtype=torch.float64)
    go = torch.randn(B * H * W, C, generator=g, dtype=torch.float64)
    return qkv, bias, table, go


def _rel(got, want):
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    return float((got - want).abs().max()) / max(1e-30, float(want.abs().max()))


def _grid():
    cases = []
    for w in (7, 12):
        for s in (0, w // 2):
            for H, W in ((2 * w, w), (w + 3, 2 * w - 5), (w - 2, w - 3), (1, 1)):
                for heads, B in ((1, 5), (6, 1), (48, 1)):
                    cases.append((w, s, H, W, heads, B))
    return cases


@pytest.mark.gpu
@pytest.mark.parametrize("w,s,H,W,heads,B", _grid())
def test_kernel_matches_float64_reference(w, s, H, W, heads, B):
    dev = "cuda:0"
    qkv, bias, table, go = _inputs(B, H, W, heads, w, seed=w * 1000 + s * 100 + H + W + heads + B)
    scale = HD ** -0.5
    r_qkv, r_bias, r_table = (t.to(dev).requires_grad_(True) for t in (qkv, bias, table))
    ref = reference_core(r_qkv, r_bias, r_table, B, H, W, heads, w, s, scale)
    ref.backward(go.to(dev))
    k_qkv, k_bias, k_table = (t.float().to(dev).requires_grad_(True) for t in (qkv, bias, table))
    out = _WindowAttention.apply(k_qkv, k_bias, k_table, B, H, W, heads, w, s, scale)
    out.backward(go.float().to(dev))
    torch.cuda.synchronize()
    # errors scaled by each array's largest element.  The gradients get a looser bound: dS = p (dP - D) cancels, and on the
    # tiny grids (one real token beside up to 143 identical padded keys) fp32 loses ~2e-4 of the largest gradient there;
    # an indexing error is O(1)
    assert _rel(out, ref) < 2e-5
    assert _rel(k_qkv.grad, r_qkv.grad) < 1e-3
    assert _rel(k_table.grad, r_table.grad) < 1e-3
    assert _rel(k_bias.grad, r_bias.grad) < 1e-3
    if (H % w or W % w) and s == 0:
        # the padded tokens' share of the bias gradient is real (the test above would miss a kernel that dropped it only if
        # it were zero): the grad of the real tokens alone differs from the full one
        assert _rel(k_qkv.grad.sum(0), r_bias.grad) > 1e-4


def _guarded(n, fill, dev, guard=64):
    buf = torch.full((n + 2 * guard,), fill, dtype=torch.float32, device=dev)
    return buf, buf[guard:guard + n], guard


@pytest.mark.gpu
@pytest.mark.parametrize("w,s,H,W,heads,B", [(7, 3, 9, 20, 6, 2), (12, 6, 23, 40, 6, 1), (12, 0, 5, 4, 48, 1)])
def test_backward_bit_identical_and_guard_words_intact(w, s, H, W, heads, B):
    dev = "cuda:0"
    lib = _lib.lib()
    C = heads * HD
    rows = B * H * W
    qkv, bias, table, go = (t.float().to(dev).contiguous() for t in _inputs(B, H, W, heads, w, seed=77))
    scale = HD ** -0.5
    sentinel = 1234.5
    stream = _lib.current_stream(qkv)
    bufs = {}
    for name, n in (("out", rows * C), ("lse", rows * heads)):
        bufs[name] = _guarded(n, sentinel, dev)
    _lib.check(lib.vnx_window_attention_forward(_lib.VNX_F32, qkv.data_ptr(), bias.data_ptr(), table.data_ptr(),
                                                bufs["out"][1].data_ptr(), bufs["lse"][1].data_ptr(), B, H, W, heads, HD,
                                                3 * C, w, s, scale, stream))
    nbytes = lib.vnx_window_attention_partial_bytes(B, H, W, heads, w)
    assert nbytes == B * ((H + w - 1) // w) * ((W + w - 1) // w) * heads * ((2 * w - 1) ** 2 + 64) * 4
    results = []
    for _ in range(2):
        for name, n in (("g", rows * 3 * C), ("gt", table.numel()), ("gp", 3 * C), ("part", nbytes // 4)):
            bufs[name] = _guarded(n, sentinel, dev)
        _lib.check(lib.vnx_window_attention_backward(
            _lib.VNX_F32, qkv.data_ptr(), bias.data_ptr(), table.data_ptr(), bufs["out"][1].data_ptr(),
            bufs["lse"][1].data_ptr(), go.data_ptr(), bufs["g"][1].data_ptr(), bufs["gt"][1].data_ptr(),
            bufs["gp"][1].data_ptr(), bufs["part"][1].data_ptr(), nbytes, B, H, W, heads, HD, 3 * C, w, s, scale, stream))
        torch.cuda.synchronize()
        for name, (buf, view, guard) in bufs.items():
            assert bool((buf[:guard] == sentinel).all()) and bool((buf[guard + view.numel():] == sentinel).all()), name
        for name in ("out", "lse", "g", "gt", "gp"):                  # every element written
            assert not bool((bufs[name][1] == sentinel).any()), name
        results.append([bufs[n][1].clone() for n in ("g", "gt", "gp")])
    for a, b in zip(*results):
        assert torch.equal(a, b)


@pytest.mark.gpu
def test_unsupported_shapes_raise_before_launching():
    dev = "cuda:0"
    lib = _lib.lib()
    t = torch.zeros(4096, device=dev)
    stream = _lib.current_stream(t)
    p = t.data_ptr()
    # head_dim 64
    st = lib.vnx_window_attention_forward(_lib.VNX_F32, p, p, p, p, p, 1, 7, 7, 1, 64, 192, 7, 0, 0.125, stream)
    assert st == 2
    # window 13
    st = lib.vnx_window_attention_forward(_lib.VNX_F32, p, p, p, p, p, 1, 13, 13, 1, 32, 96, 13, 0, 0.17, stream)
    assert st == 2
    st = lib.vnx_window_attention_backward(_lib.VNX_F32, p, p, p, p, p, p, p, p, p, p, 16384, 1, 13, 13, 1, 32, 96, 13, 0,
                                           0.17, stream)
    assert st == 2
    # 49 heads; a partial buffer too small
    assert lib.vnx_window_attention_forward(_lib.VNX_F32, p, p, p, p, p, 1, 7, 7, 49, 32, 49 * 96, 7, 0, 0.17, stream) == 2
    assert lib.vnx_window_attention_backward(_lib.VNX_F32, p, p, p, p, p, p, p, p, p, p, 4, 1, 7, 7, 1, 32, 96, 7, 0, 0.17,
                                             stream) == 3
    with pytest.raises(_lib.VnextHipError):
        _lib.check(lib.vnx_window_attention_forward(_lib.VNX_F32, p, p, p, p, p, 1, 7, 7, 1, 64, 192, 7, 0, 0.125, stream))
    torch.cuda.synchronize()
    assert bool((t == 0).all())                        # nothing ran


def test_partial_bytes_formula_without_a_gpu():
    from vnext_amd import _lib as L
    lib = L.lib()
    assert lib.vnx_window_attention_partial_bytes(5, 184, 320, 6, 12) == 5 * 16 * 27 * 6 * (23 * 23 + 64) * 4
    assert lib.vnx_window_attention_partial_bytes(1, 1, 1, 1, 13) == 0
    np.testing.assert_equal(relative_position_index(2).tolist(), [[4, 3, 1, 0], [5, 4, 2, 1], [7, 6, 4, 3], [8, 7, 5, 4]])
