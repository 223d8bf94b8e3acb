"""Dense result masks from the logits in one device pass (vnext_amd/csrc/mask_dense.hip, vnext_amd/ops/mask_dense.py):
the bits of the RLE encoder it shares its sampling code with, the masks of the models' eager chain."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import ROOT
from test_mask_rle import BAND, bilinear_f64, blob_logits, host_expression, nearest_index
from vnext_amd import _lib
from vnext_amd.ops import mask_dense
from vnext_amd.ops.mask_dense import bits_pitch, masks_from_logits, unpack_bits
from vnext_amd.ops.mask_rle import encode_logits
from vnext_amd.utils.ytvis_json import rle_decode

IMAGES = [(92, 164), (89, 159), (61, 123)]            # crops of the 92 x 164 grid of blob_logits(5, 23, 41), stride 4


def out_sizes(image):
    ih, iw = image
    return [image, (2 * ih, 2 * iw), (ih // 3, iw // 2), (ih + 7, iw - 11), (17, 63), (17, 64), (17, 65), (3, 129), (1, 1),
            (5, 7)]


# ---- CPU -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stride,hw,image,out", [(4, (6, 10), (24, 40), (30, 50)), (4, (6, 10), (21, 37), (21, 37)),
                                                 (8, (5, 7), (33, 50), (20, 31)), (4, (9, 16), (36, 64), (72, 129))])
def test_cpu_masks_are_the_host_expression(stride, hw, image, out):
    logits = blob_logits(4, *hw, seed=stride + hw[0])
    want = host_expression(logits, stride, image, out)
    got = masks_from_logits(logits, stride, image, out)
    assert got.dtype == torch.bool and got.shape == want.shape and torch.equal(got, want)
    assert torch.equal(masks_from_logits(logits.double(), stride, image, out), want)        # other dtypes: cast to fp32
    packed = masks_from_logits(logits, stride, image, out, bits=True)
    pitch = bits_pitch(out[1])
    assert packed.dtype == torch.uint8 and tuple(packed.shape) == (4, out[0], pitch) and pitch % 8 == 0
    ref = np.zeros((4, out[0], pitch), np.uint8)
    ref[:, :, :(out[1] + 7) // 8] = np.packbits(want.numpy(), axis=-1, bitorder="little")
    assert np.array_equal(packed.numpy(), ref)
    assert torch.equal(unpack_bits(packed, out[1]), want)
    empty = masks_from_logits(logits[:0], stride, image, out)
    assert empty.dtype == torch.bool and tuple(empty.shape) == (0,) + tuple(out)


@pytest.mark.parametrize("width", [1, 7, 8, 9, 63, 64, 65, 129])
def test_cpu_unpack_bits_round_trips(width):
    g = torch.Generator().manual_seed(width)
    masks = torch.rand(3, 5, width, generator=g) > 0.5
    packed = mask_dense.pack_bits(masks)
    assert tuple(packed.shape) == (3, 5, 8 * ((width + 63) // 64))
    back = unpack_bits(packed, width)
    assert back.dtype == torch.bool and torch.equal(back, masks)
    assert not unpack_bits(packed, packed.shape[-1] * 8)[..., width:].any()                 # the padding is zero
    with pytest.raises(ValueError):
        unpack_bits(packed, packed.shape[-1] * 8 + 1)


def test_abi_17_exports_the_entry_point():
    with open(os.path.join(ROOT, "include", "vnext_hip.h")) as f:
        header = f.read()
    assert "int vnx_mask_dense(int format, const void* logits, int masks" in header
    assert "VNX_MASK_DENSE_U8 = 0" in header and "VNX_MASK_DENSE_BITS = 1" in header
    assert "#define VNX_ABI_VERSION 17" in header
    assert "vnx_mask_dense" in _lib.SIGNATURES
    assert (_lib.MASK_DENSE_U8, _lib.MASK_DENSE_BITS) == (0, 1)
    assert hasattr(_lib.product_lib(), "vnx_mask_dense")
    assert _lib.ABI_VERSION == 17 and _lib.product_lib().vnx_abi_version() == 17


# ---- GPU -----------------------------------------------------------------------------------------------------------
DEV = "cuda:0"


def both_forms(logits, stride, image, out):
    """the op's two forms on the device -> bool [M, oh, ow] on the host, twice"""
    dev = logits.to(DEV)
    u8 = masks_from_logits(dev, stride, image, out)
    packed = masks_from_logits(dev, stride, image, out, bits=True)
    assert u8.dtype == torch.bool and tuple(u8.shape) == (logits.shape[0],) + tuple(out) and u8.is_cuda
    assert packed.dtype == torch.uint8 and tuple(packed.shape) == (logits.shape[0], out[0], bits_pitch(out[1]))
    assert (u8.view(torch.uint8) <= 1).all()
    assert not unpack_bits(packed, packed.shape[-1] * 8)[..., out[1]:].any()
    return u8.cpu(), unpack_bits(packed, out[1]).cpu()


def assert_equals_the_encoder(logits, stride, image, out):
    u8, bits = both_forms(logits, stride, image, out)
    rle = np.stack([rle_decode(r) for r in encode_logits(logits.to(DEV), stride, image, out)])
    assert np.array_equal(u8.numpy(), rle), (stride, image, out)
    assert np.array_equal(bits.numpy(), rle), (stride, image, out)


@pytest.fixture(scope="module")
def blobs():
    return blob_logits(5, 23, 41, seed=27)


def rounding_map(M, h, w, seed):
    """+-(1 + j 2^-23), j in 0..7: neighbouring values of opposite sign nearly cancel in the bilinear sums"""
    g = torch.Generator().manual_seed(seed)
    sign = torch.where(torch.rand(M, h, w, generator=g) > 0.5, 1.0, -1.0)
    j = torch.randint(0, 8, (M, h, w), generator=g)
    return sign * (1 + j.float() * 2.0 ** -23)


def cancelling_map(M, h, w, stride, seed):
    """Columns (and rows) alternate between +b (1 + j 2^-23) and -a (1 + j 2^-23), where (a, b) / (a + b) are the weights
    of one sub-pixel phase of the stride (stride 4: 3/8 and 5/8; stride 8: 7/16 and 9/16): at that phase a * (+b) + b * (-a)
    cancels to the last bits, so the sign of the value IS its rounding -- which product was fused into which sum decides
    it.  (The +-1 map of `rounding_map` never comes closer to zero than 1/64 at these strides.)"""
    a, b = (3.0, 5.0) if stride == 4 else (7.0, 9.0)
    g = torch.Generator().manual_seed(seed)
    j = torch.randint(0, 8, (M, h, w), generator=g).float() * 2.0 ** -23
    col = torch.where(torch.arange(w) % 2 == 0, b, -a)[None, None, :]
    flip = torch.where(torch.rand(M, h, 1, generator=g) > 0.5, 1.0, -1.0)                  # whole rows change sign
    return (col * flip * (1 + j)).contiguous()


@pytest.mark.gpu
def test_bit_for_bit_the_encoder_on_the_blob_inputs(blobs):
    for image in IMAGES:
        for out in out_sizes(image):
            assert_equals_the_encoder(blobs, 4, image, out)


@pytest.mark.gpu
def test_bit_for_bit_the_encoder_on_exact_zeros():
    flat = torch.zeros(2, 10, 12)
    flat[1, 3:6, 4:9] = 1.0
    for out in [(40, 48), (57, 71), (20, 129)]:
        assert_equals_the_encoder(flat, 4, (40, 48), out)
    u8, _ = both_forms(flat, 4, (40, 48), (40, 48))
    assert not u8[0].any() and u8[1].any()                     # value > 0: an exact zero is not set


@pytest.mark.gpu
@pytest.mark.parametrize("stride", [4, 8])
def test_bit_for_bit_the_encoder_on_rounding_sensitive_maps(stride):
    h, w = 13, 19
    H, W = h * stride, w * stride
    for maps in (rounding_map(4, h, w, seed=stride), cancelling_map(4, h, w, stride, seed=10 + stride)):
        for image, out in [((H, W), (H, W)), ((H - 3, W - 5), (H + 9, W + 30)), ((H, W), (2 * H - 1, 129))]:
            assert_equals_the_encoder(maps, stride, image, out)
    # the second map does what it was built for: at full size a good share of its values lies within rounding of zero
    v = bilinear_f64(cancelling_map(4, h, w, stride, seed=10 + stride), stride, (H, W), (H, W))
    assert (np.abs(v) < 1e-5).mean() > 0.05


@pytest.mark.gpu
def test_equal_to_the_eager_chain(blobs):
    for image in IMAGES:
        for out in out_sizes(image):
            v = bilinear_f64(blobs, 4, image, out)
            assert not (np.abs(v) < BAND).any(), (image, out)                # the empty band first
            want = host_expression(blobs.to(DEV), 4, image, out).cpu()
            u8, bits = both_forms(blobs, 4, image, out)
            assert torch.equal(u8, want), (image, out)
            assert torch.equal(bits, want), (image, out)
            assert np.array_equal(want.numpy(), v > 0)


@pytest.mark.gpu
@pytest.mark.parametrize("n_in,n_out", [(40, 60), (37, 101), (97, 31), (720, 1280)])
def test_nearest_index_maps_equal_torch(n_in, n_out):
    """stride 1 (bilinear = the map itself), a +-1 map: any wrong row / column flips a bit"""
    g = torch.Generator().manual_seed(n_in + n_out)
    sign = torch.where(torch.rand(3, n_in, 17, generator=g) > 0.5, 1.0, -1.0)
    want = F.interpolate(sign[:, None], size=(n_out, 23), mode="nearest")[:, 0] > 0
    assert (nearest_index(n_in, n_out) == F.interpolate(torch.arange(n_in, dtype=torch.float32)[None, None, :, None],
                                                        size=(n_out, 1))[0, 0, :, 0].long().numpy()).all()
    for got in both_forms(sign, 1, (n_in, 17), (n_out, 23)):
        assert torch.equal(got, want)
    signt = sign.transpose(1, 2).contiguous()
    want = F.interpolate(signt[:, None], size=(23, n_out), mode="nearest")[:, 0] > 0
    for got in both_forms(signt, 1, (17, n_in), (23, n_out)):
        assert torch.equal(got, want)


GUARD = 64


def raw(fmt, logits, stride, image, out, fill, lead):
    """the C entry point on a buffer of `fill` bytes with GUARD bytes of 0xAB around `out`, which starts `lead` bytes into an
    aligned allocation -> (the output bytes [M, oh, pitch], the whole buffer), on the host"""
    M, h, w = logits.shape
    pitch = out[1] if fmt == _lib.MASK_DENSE_U8 else bits_pitch(out[1])
    n = M * out[0] * pitch
    buf = torch.full((lead + n + GUARD,), 0xAB, dtype=torch.uint8, device=DEV)
    buf[lead:lead + n] = fill
    _lib.check(_lib.lib().vnx_mask_dense(fmt, logits.data_ptr(), M, h, w, stride, image[0], image[1], out[0], out[1],
                                         buf.data_ptr() + lead, n, _lib.current_stream(logits)))
    host = buf.cpu()
    return host[lead:lead + n].view(M, out[0], pitch), host


@pytest.mark.gpu
@pytest.mark.parametrize("out", [(17, 63), (17, 64), (17, 65), (3, 129), (1, 1), (5, 7), (37, 2049), (3, 4100)])
def test_guard_bytes_padding_and_determinism(blobs, out):
    """Rows of any width at an odd byte offset (U8), pitch padding on a buffer of 0xFF (BITS), widths on both sides of a
    ballot word and of the 2048-column tile, more rows than a task holds: nothing outside `out` is touched, every byte
    inside it is written, and two runs are byte-identical."""
    logits, image = blobs.to(DEV), (92, 164)
    assert logits.data_ptr() % 256 == 0
    want = masks_from_logits(logits, 4, image, out).cpu()
    for fmt, lead in ((_lib.MASK_DENSE_U8, GUARD + 1), (_lib.MASK_DENSE_U8, GUARD + 6), (_lib.MASK_DENSE_BITS, GUARD)):
        for fill in (0xFF, 0x00):
            a, whole = raw(fmt, logits, 4, image, out, fill, lead)
            b, _ = raw(fmt, logits, 4, image, out, fill, lead)
            assert torch.equal(a, b)
            assert (whole[:lead] == 0xAB).all() and (whole[lead + a.numel():] == 0xAB).all()
            if fmt == _lib.MASK_DENSE_U8:
                assert torch.equal(a.view(torch.bool), want)
            else:
                every = unpack_bits(a, a.shape[-1] * 8)
                assert torch.equal(every[..., :out[1]], want) and not every[..., out[1]:].any()


@pytest.mark.gpu
def test_more_rows_than_a_grid_dimension():
    g = torch.Generator().manual_seed(70)
    sign = torch.where(torch.rand(70, 3, 3, generator=g) > 0.5, 1.0, -1.0)
    want = F.interpolate(sign[:, None], size=(1000, 8), mode="nearest")[:, 0] > 0
    for got in both_forms(sign, 1, (3, 3), (1000, 8)):          # 70 000 rows
        assert torch.equal(got, want)


@pytest.mark.gpu
def test_more_than_2_31_output_bytes():
    side = 27000
    logits = torch.randn(3, 4, 4, generator=torch.Generator().manual_seed(33))
    v = bilinear_f64(logits, 4, (16, 16), (16, 16))
    assert not (np.abs(v) < BAND).any()
    small = v > 0                                               # [3, 16, 16]: the masks on the upsampled grid
    assert all(0.3 < small[m].mean() < 0.7 for m in range(3))
    idx = nearest_index(16, side)                               # the output is small[:, idx][:, :, idx]
    per = np.bincount(idx, minlength=16).astype(np.int64)       # output rows (= columns) per source index
    assert 3 * side * side > 2 ** 31
    out = masks_from_logits(logits.to(DEV), 4, (16, 16), (side, side))
    assert tuple(out.shape) == (3, side, side)
    assert (out.view(torch.uint8) <= 1).all()
    counts = [int(out[m].sum(dtype=torch.int64)) for m in range(3)]
    assert counts == [int(per @ small[m].astype(np.int64) @ per) for m in range(3)]
    rows = 40
    first, last = out[0, :rows].cpu().numpy(), out[2, -rows:].cpu().numpy()
    assert np.array_equal(first, small[0][idx[:rows]][:, idx])
    assert np.array_equal(last, small[2][idx[-rows:]][:, idx])


@pytest.mark.gpu
def test_refusals_before_a_launch():
    lib = _lib.lib()
    x = torch.zeros(2, 8, 8, device=DEV)
    out = torch.empty(2 * 32 * 32 + 8, dtype=torch.uint8, device=DEV)
    st = _lib.current_stream(x)
    U, B = _lib.MASK_DENSE_U8, _lib.MASK_DENSE_BITS
    assert out.data_ptr() % 8 == 0

    def refused(*args, status=1):
        assert lib.vnx_mask_dense(*args, st) == status, args
        assert b"vnx_mask_dense" in lib.vnx_last_error()
    n = 2 * 32 * 32
    refused(U, x.data_ptr(), -1, 8, 8, 4, 32, 32, 32, 32, out.data_ptr(), n)                  # M < 0
    refused(U, x.data_ptr(), 2, 0, 8, 4, 32, 32, 32, 32, out.data_ptr(), n)                   # non-positive sizes
    refused(U, x.data_ptr(), 2, 8, 0, 4, 32, 32, 32, 32, out.data_ptr(), n)
    refused(U, x.data_ptr(), 2, 8, 8, 0, 32, 32, 32, 32, out.data_ptr(), n)
    refused(U, x.data_ptr(), 2, 8, 8, 4, 0, 32, 32, 32, out.data_ptr(), n)
    refused(U, x.data_ptr(), 2, 8, 8, 4, 32, 32, 0, 32, out.data_ptr(), n)
    refused(U, x.data_ptr(), 2, 8, 8, 4, 32, 32, 32, 0, out.data_ptr(), n)
    refused(U, x.data_ptr(), 2, 8, 8, 4, 33, 32, 32, 32, out.data_ptr(), n)                   # crop larger than the upsampled map
    refused(U, x.data_ptr(), 2, 8, 8, 4, 32, 33, 32, 32, out.data_ptr(), n)
    refused(U, None, 2, 8, 8, 4, 32, 32, 32, 32, out.data_ptr(), n)                           # null pointers
    refused(U, x.data_ptr(), 2, 8, 8, 4, 32, 32, 32, 32, None, n)
    refused(U, x.data_ptr() + 2, 2, 8, 8, 4, 32, 32, 32, 32, out.data_ptr(), n)               # misaligned logits
    refused(B, x.data_ptr(), 2, 8, 8, 4, 32, 32, 32, 32, out.data_ptr() + 4, 2 * 32 * 8)      # BITS: out not 8-byte aligned
    refused(U, x.data_ptr(), 2, 8, 8, 4, 32, 32, 32, 32, out.data_ptr(), n - 1)               # out_bytes too small
    refused(B, x.data_ptr(), 2, 8, 8, 4, 32, 32, 32, 32, out.data_ptr(), 2 * 32 * 8 - 1)
    refused(U, x.data_ptr(), 2, 8, 8, 4, 32, 32, 32, 32, out.data_ptr(), -1)
    refused(U, x.data_ptr(), 2, 8, 8, 4, 32, 32, 2 ** 31 - 1, 2 ** 31 - 1, out.data_ptr(), 2 ** 62)      # (no overflow)
    refused(7, x.data_ptr(), 2, 8, 8, 4, 32, 32, 32, 32, out.data_ptr(), n)                   # unknown format
    refused(U, x.data_ptr(), 2, 65536, 32768, 4, 32, 32, 32, 32, out.data_ptr(), n, status=2)  # h * w >= 2^31
    out.fill_(0xAB)
    assert lib.vnx_mask_dense(U, None, 0, 8, 8, 4, 32, 32, 32, 32, None, 0, st) == 0          # M == 0: a no-op
    assert lib.vnx_mask_dense(B, None, 0, 8, 8, 4, 32, 32, 32, 32, out.data_ptr(), n, st) == 0
    assert lib.vnx_mask_dense(U, x.data_ptr(), 2, 8, 8, 4, 32, 32, 32, 32, out.data_ptr() + 3, n, st) == 0      # U8: any offset
    torch.cuda.synchronize()
    assert (out[:3] == 0xAB).all() and (out[3:3 + n] == 0).all() and (out[3 + n:] == 0xAB).all()
    with pytest.raises(_lib.VnextHipError, match="bad sizes"):
        masks_from_logits(x, 4, (40, 32), (32, 32))
    with pytest.raises(ValueError):
        masks_from_logits(x[0], 4, (32, 32), (32, 32))
    empty = masks_from_logits(x[:0], 4, (32, 32), (32, 32))
    assert empty.is_cuda and empty.dtype == torch.bool and tuple(empty.shape) == (0, 32, 32)


@pytest.mark.gpu
@pytest.mark.parametrize("bits", [False, True])
def test_capture_and_replay(bits):
    image, out = (89, 159), (101, 203)
    static_in = blob_logits(5, 23, 41, seed=1).to(DEV)
    masks_from_logits(static_in, 4, image, out, bits=bits)      # (the library is loaded before the capture)
    torch.cuda.synchronize()
    calls = mask_dense.CALLS["masks_from_logits"]
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static_out = masks_from_logits(static_in, 4, image, out, bits=bits)
    assert mask_dense.CALLS["masks_from_logits"] == calls + 1
    for seed in (2, 3):
        fresh = blob_logits(5, 23, 41, seed=seed).to(DEV)
        want = masks_from_logits(fresh, 4, image, out, bits=bits).clone()
        static_in.copy_(fresh)
        static_out.view(torch.uint8).fill_(0xAB)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(static_out, want)
    assert not torch.equal(masks_from_logits(blob_logits(5, 23, 41, seed=2).to(DEV), 4, image, out, bits=bits),
                           masks_from_logits(blob_logits(5, 23, 41, seed=3).to(DEV), 4, image, out, bits=bits))
