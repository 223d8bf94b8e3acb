"""MSDA on samples that lie exactly ON pixel lines and map borders: the cell chosen at an integer coordinate, `> -1` against
`>= -1`, `< H` against `<= H`, and taps of weight exactly zero that belong to the next unit, tile box or level
(ms_deform_im2col_cuda.cuh:285-288 the decode and its range test, :38-45 floor and fractions, :55-78 the four tap rules).

Every other MSDA test draws fp32 locations on maps whose sizes are not powers of two: there a pixel coordinate is never an
integer, fp32 and fp64 may take different sides of a line, and grad_sampling_loc -- which jumps across a line -- is compared
with the samples near a line masked out (boundary_mask, off_the_pixel_grid).  Here the level sizes are powers of two and the
locations are (p + 0.5) / size with p from a fixed menu (`lattice_case`), so that the location, the pixel coordinate and, for
the fused prologue, the raw offsets are exact in the kernels' own number formats: fp32 and fp64 agree on every cell, and
every output is compared on EVERY element against the float64 C oracle (oracle/msda_oracle_body.inc:19-32), grad_sampling_loc
included, with no mask.

The first tests run without a GPU and pin the premise: the inputs are exact, the oracle agrees with itself across
precisions, a wrong cell convention is visible (in grad_sampling_loc, at order one), and where the grid_sample statement of
the op stops being an authority (a coordinate exactly -1)."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import msda_oracle as O  # noqa: E402
from test_msda_geometry import CODE, TOL16, Guarded, assert_levels, scale  # noqa: E402
from vnext_amd import _lib  # noqa: E402

DEV = "cuda:0"
DECODER = ((32, 64), (16, 32), (8, 16), (4, 8))                   # S = 2 720
STAGED = ((8, 16), (4, 8), (2, 4), (1, 2))                       # every level fits the slab forward's LDS
DEGENERATE = ((16, 16), (1, 1), (1, 32), (32, 1))                 # one pixel, one row, one column
TWO_LEVELS = ((64, 64), (16, 16))
PYRAMIDS = (DECODER, STAGED, DEGENERATE, TWO_LEVELS)
HALF = ((16, 32), (8, 16), (4, 8), (2, 4))                        # fp16 locations: sides <= 32, steps of 1/4
BF16 = ((8, 16), (4, 8), (2, 4), (1, 2))                          # bf16 locations: sides <= 16, steps of 1/2
CODES = dict(CODE)
CODES[torch.float64] = _lib.VNX_F64

# ---- the menu ---------------------------------------------------------------------------------------------------------------
# `d` is the smallest power of two for which the coordinate, the coordinate + 0.5 (the location times the size) and, for the
# fused prologue, the raw offset are exactly representable: 2^-24 at -1 + d in fp32, coarser next to n.
CLASSES = ("interior", "fraction", "-1.5", "-1-d", "-1", "-1+d", "-0.5", "n-1", "n-d", "n", "n+0.5", "k-d", "k+d")
WEIGHTS = (0.34, 0.14, 0.02, 0.02, 0.045, 0.04, 0.03, 0.06, 0.04, 0.045, 0.02, 0.10, 0.10)
FRACTIONS = {torch.float32: (0.25, 0.5, 0.75), torch.float16: (0.25, 0.5, 0.75), torch.bfloat16: (0.5,)}
MAX_SIDE = {torch.float32: 1 << 16, torch.float16: 32, torch.bfloat16: 16}
INTEGER_QUOTA, BORDER_QUOTA = 0.40, 0.05


def exact_in(x, dtype):
    """float64 tensor -> which elements survive a round trip through `dtype`"""
    return x.to(dtype).double() == x


def smallest_delta(line, sign, must):
    """per element the smallest power of two d with line + sign * d + shift exact in dtype for every (shift, dtype) of `must`"""
    delta = torch.zeros_like(line)
    found = torch.zeros_like(line, dtype=torch.bool)
    for e in range(-30, 1):
        cand = line + sign * 2.0 ** e
        ok = torch.ones_like(found)
        for shift, dtype in must:
            ok &= exact_in(cand + shift, dtype)
        delta = torch.where(ok & ~found, torch.full_like(delta, 2.0 ** e), delta)
        found |= ok
    assert bool(found.all()), "no representable neighbour of a pixel line"
    return delta


def class_labels(count, g):
    """a shuffled list of `count` class indices holding every class, in the proportions of WEIGHTS (the rest: interior)"""
    counts = [max(1, int(w * count)) for w in WEIGHTS]
    counts[0] += count - sum(counts)
    assert counts[0] >= 1, f"{count} samples per level cannot hold every menu class"
    labels = torch.repeat_interleave(torch.arange(len(CLASSES)), torch.tensor(counts))
    return labels[torch.randperm(count, generator=g)]


def draw_axis(n, count, g, dtype, pivot=None, pivot_dtype=None):
    """`count` pixel coordinates (float64) on an axis of n pixels, and their classes.  `pivot`: the reference pixel of each
    sample (fused prologue): coordinate - pivot must be exact in `pivot_dtype` too."""
    labels = class_labels(count, g)
    fr = torch.tensor(FRACTIONS[dtype], dtype=torch.float64)

    def ints(lo, hi):      # [lo, hi)
        return torch.randint(lo, hi, (count,), generator=g).double()

    interior = ints(0, max(n - 1, 1))
    fraction = ints(-1, n) + fr[torch.randint(0, len(fr), (count,), generator=g)]
    line = ints(0, n)
    fixed = {"-1.5": -1.5, "-1": -1.0, "-0.5": -0.5, "n-1": n - 1.0, "n": float(n), "n+0.5": n + 0.5}
    beside = {"-1-d": -1.0, "-1+d": -1.0, "n-d": float(n)}              # the line a neighbour lies beside; k-d, k+d: drawn
    base = torch.zeros(count, dtype=torch.float64)
    sign = torch.zeros(count, dtype=torch.float64)
    for c, name in enumerate(CLASSES):
        sel = labels == c
        if name == "interior":
            base[sel] = interior[sel]
        elif name == "fraction":
            base[sel] = fraction[sel]
        elif name in fixed:
            base[sel] = fixed[name]
        else:
            base[sel] = beside[name] if name in beside else line[sel]
            sign[sel] = -1.0 if name.endswith("-d") else 1.0
    must = [(0.0, dtype), (0.5, dtype)]
    if pivot is not None:
        must.append((-pivot, pivot_dtype))
    px = base + sign * smallest_delta(base, sign, must)
    return px, labels


def sizes_of(shapes):
    sh = torch.tensor(shapes, dtype=torch.long)
    lsi = torch.cat((sh.new_zeros((1,)), sh.prod(1).cumsum(0)[:-1]))
    return sh, lsi


def pixel_coordinates(loc, sh):
    """[B, Lq, M, L, P, 2] float64 pixel coordinates (x, y) of a lattice case's locations: exact"""
    wh = torch.stack([sh[:, 1], sh[:, 0]], -1).double().view(1, 1, 1, -1, 1, 2)
    return loc.double() * wh - 0.5


def assert_lattice(loc64, labels, shapes, loc_dtype):
    """the generator's own guarantees: exact inputs, quotas, every class on every level and axis"""
    sh, _ = sizes_of(shapes)
    for h, w in shapes:
        for n in (h, w):
            assert n >= 1 and n & (n - 1) == 0 and n <= MAX_SIDE[loc_dtype], f"a side of {n} pixels with {loc_dtype} locations"
    loc = loc64.to(loc_dtype)
    assert bool((loc.double() == loc64).all()), "a location is not exact in the locations' type"
    px64 = pixel_coordinates(loc64, sh)
    wh32 = torch.stack([sh[:, 1], sh[:, 0]], -1).float().view(1, 1, 1, -1, 1, 2)
    px32 = loc.float() * wh32 - 0.5                                  # the kernels' expression (cuh:285-286) in their type
    assert bool((px32.double() == px64).all()), "a pixel coordinate differs between float32 and float64"
    n = torch.stack([sh[:, 1], sh[:, 0]], -1).double().view(1, 1, 1, -1, 1, 2)
    integer = float((px64 == px64.round()).double().mean())
    border = float(((px64 == -1) | (px64 == n)).double().mean())
    assert integer >= INTEGER_QUOTA, f"{integer:.3f} of the coordinates are integers"
    assert border >= BORDER_QUOTA, f"{border:.3f} of the coordinates are exactly -1 or n"
    for l in range(len(shapes)):
        for axis in (0, 1):
            seen = torch.bincount(labels[l][axis], minlength=len(CLASSES))
            missing = [CLASSES[c] for c in range(len(CLASSES)) if seen[c] == 0]
            assert not missing, f"level {l}, axis {'xy'[axis]}: no sample of {missing}"
    return loc, integer, border


def lattice_case(shapes, B, M, Lq, P, seed, loc_dtype=torch.float32):
    """-> shapes, level starts, value, loc (in loc_dtype), attn, grad_out; raises unless the lattice's guarantees hold"""
    g = torch.Generator().manual_seed(seed)
    sh, lsi = sizes_of(shapes)
    L, S = len(shapes), int(sh.prod(1).sum())
    loc64 = torch.empty(B, Lq, M, L, P, 2, dtype=torch.float64)
    labels = []
    for l, (h, w) in enumerate(shapes):
        x, cx = draw_axis(w, B * Lq * M * P, g, loc_dtype)
        y, cy = draw_axis(h, B * Lq * M * P, g, loc_dtype)
        loc64[:, :, :, l, :, 0] = ((x + 0.5) / w).view(B, Lq, M, P)
        loc64[:, :, :, l, :, 1] = ((y + 0.5) / h).view(B, Lq, M, P)
        labels.append((cx, cy))
    loc, _, _ = assert_lattice(loc64, labels, shapes, loc_dtype)
    value = torch.randn(B, S, M, 32, generator=g)
    attn = torch.softmax(torch.randn(B, Lq, M, L * P, generator=g), -1).view(B, Lq, M, L, P).contiguous()
    go = torch.randn(B, Lq, M * 32, generator=g)
    return sh, lsi, value, loc.contiguous(), attn, go


def prologue(offsets, ref, ref_div, shapes, P):
    """the module's location arithmetic (IDOL ops/modules/ms_deform_attn.py:102-108) in the tensors' own type, in the order the
    fused kernels evaluate it (msda_d32.hip: fused_decode)"""
    r = ref.repeat_interleave(ref_div, 0)
    if ref.shape[-1] == 2:
        norm = torch.tensor([[w, h] for h, w in shapes], dtype=offsets.dtype)
        return r[:, :, None, :, None, :] + offsets / norm[None, None, None, :, None, :]
    return r[:, :, None, :, None, :2] + offsets / P * r[:, :, None, :, None, 2:] * 0.5


def fused_lattice_case(shapes, B, M, Lq, P, seed, ref_dim=2, ref_div=1, off_dtype=torch.float32, queries_are_pixels=False):
    """the fused prologue's raw inputs for lattice locations: reference points on pixel centres (i + 0.5) / size of each level
    (fp32), offsets = menu - i (2-component reference points) or that times 8 / (size x box side) with box sides that are
    powers of two (4-component, P = 4), so that the fp32 prologue gives the fp64 locations bit for bit.
    -> dict(sh, lsi, value, offsets, logits, ref, go, loc64, ref_div)"""
    assert B % ref_div == 0 and (ref_dim == 2 or P == 4)
    g = torch.Generator().manual_seed(seed)
    sh, lsi = sizes_of(shapes)
    L, S, Br = len(shapes), int(sh.prod(1).sum()), B // ref_div
    if queries_are_pixels:
        assert Lq == S
        qx, qy = [], []
        for h, w in shapes:
            ys, xs = torch.meshgrid(torch.arange(h) + 0.5, torch.arange(w) + 0.5, indexing="ij")
            qx.append(xs.reshape(-1) / w)
            qy.append(ys.reshape(-1) / h)
        qx, qy = torch.cat(qx).double(), torch.cat(qy).double()
    loc64 = torch.empty(B, Lq, M, L, P, 2, dtype=torch.float64)
    offsets = torch.empty(B, Lq, M, L, P, 2, dtype=torch.float64)
    ref = torch.empty(Br, Lq, L, ref_dim, dtype=torch.float64)
    labels = []
    for l, (h, w) in enumerate(shapes):
        per_axis = []
        for axis, n in ((0, w), (1, h)):
            if queries_are_pixels:      # the pixel of this level under the query (its own pixel on its own level)
                i = torch.floor((qx, qy)[axis] * n).view(1, Lq).expand(Br, Lq)
            else:
                i = torch.randint(0, n, (Br, Lq), generator=g).double()
            ref[:, :, l, axis] = (i + 0.5) / n
            gain = torch.ones(Br, Lq, dtype=torch.float64)
            if ref_dim == 4:
                side = 2.0 ** -torch.randint(1, 4, (Br, Lq), generator=g).double()      # 1/2, 1/4, 1/8 of the map
                ref[:, :, l, 2 + axis] = side
                gain = 8.0 / (n * side)                                                  # location = centre + offset / 4 * side / 2
            pivot = i.repeat_interleave(ref_div, 0).view(B, Lq, 1, 1).expand(B, Lq, M, P).reshape(-1)
            px, c = draw_axis(n, B * Lq * M * P, g, torch.float32, pivot, off_dtype)
            gain = gain.repeat_interleave(ref_div, 0).view(B, Lq, 1, 1)
            offsets[:, :, :, l, :, axis] = (px - pivot).view(B, Lq, M, P) * gain
            loc64[:, :, :, l, :, axis] = ((px + 0.5) / n).view(B, Lq, M, P)
            per_axis.append(c)
        labels.append(tuple(per_axis))
    assert_lattice(loc64, labels, shapes, torch.float32)
    off = offsets.to(off_dtype)
    assert bool((off.double() == offsets).all()), "an offset is not exact in the offsets' type"
    ref32 = ref.float()
    assert bool((ref32.double() == ref).all())
    got = prologue(off.float(), ref32, ref_div, shapes, P)
    assert got.dtype == torch.float32 and bool((got.double() == loc64).all()), "the fp32 prologue does not reproduce the locations"
    assert bool((prologue(offsets, ref, ref_div, shapes, P) == loc64).all())
    value = torch.randn(B, S, M, 32, generator=g)
    logits = (torch.randn(B, Lq, M, L * P, generator=g) * 2).to(off_dtype)
    go = torch.randn(B, Lq, M * 32, generator=g)
    return dict(shapes=shapes, sh=sh, lsi=lsi, value=value, offsets=off.contiguous(), logits=logits, ref=ref32.contiguous(), go=go,
                loc64=loc64, ref_div=ref_div, P=P)


case_of = functools.lru_cache(maxsize=8)(lattice_case)
fused_case_of = functools.lru_cache(maxsize=4)(fused_lattice_case)


@functools.lru_cache(maxsize=8)
def oracle_of(key, vdt=torch.float32, ldt=torch.float32):
    """float64 C oracle on the inputs as the kernels see them (rounded to their types): forward and the three gradients"""
    sh, lsi, value, loc, attn, go = case_of(*key)
    args = (value.to(vdt).double().numpy(), sh.numpy(), lsi.numpy(), loc.to(ldt).double().numpy(), attn.to(ldt).double().numpy())
    return (O.msda_forward(*args, nthreads=8),) + tuple(O.msda_backward(*args, go.to(vdt).double().numpy(), nthreads=8))


# ---- what a mismatch in grad_sampling_loc looks like ----------------------------------------------------------------------
def class_of(v, n):
    """menu class of one pixel coordinate, from its value"""
    for name, x in (("-1.5", -1.5), ("-1", -1.0), ("-0.5", -0.5), ("n", float(n)), ("n+0.5", n + 0.5), ("n-1", n - 1.0)):
        if v == x:
            return name
    if v == np.floor(v):
        return "interior"
    f = v - np.floor(v)
    if f in (0.25, 0.5, 0.75):
        return "fraction"
    if v < -1:
        return "-1-d"
    if v < -0.75:
        return "-1+d"
    if v > n - 0.25:
        return "n-d"
    return "k+d" if f < 0.25 else "k-d"


def outside(px, sh):
    """[B, Lq, M, L, P] samples that fail the reference's range test (cuh:288): all their gradients are exactly zero"""
    n = torch.stack([sh[:, 1], sh[:, 0]], -1).double().view(1, 1, 1, -1, 1, 2)
    return (~((px > -1) & (px < n)).all(-1)).numpy()


def assert_per_sample(got, want, tol, px, sh, what):
    """a per-sample gradient [B, Lq, M, L, P, (2)] on EVERY element; a failure names the levels and the menu classes"""
    got, want = got.reshape(px.shape[:5] + (-1,)), want.reshape(px.shape[:5] + (-1,))
    err = np.abs(got - want)
    bad = (err > tol * scale(want)).any(-1)
    out = outside(px, sh)
    assert np.all(want[out] == 0), f"{what}: the oracle is not zero on a sample outside the map"
    leak = (got != 0).any(-1) & out
    if not bad.any() and not leak.any():
        return
    pxn = px.numpy()
    n = torch.stack([sh[:, 1], sh[:, 0]], -1).double().view(1, 1, 1, -1, 1, 2).numpy()
    sel = bad | leak
    integer = int(((pxn == np.round(pxn)).any(-1) & sel).sum())
    border = int((((pxn == -1) | (pxn == n)).any(-1) & sel).sum())
    levels, classes = {}, {}
    for idx in np.argwhere(sel)[:2000]:
        l = int(idx[3])
        levels[l] = levels.get(l, 0) + 1
        x, y = pxn[tuple(idx)]
        key = (class_of(x, int(sh[l, 1])), class_of(y, int(sh[l, 0])))
        classes[key] = classes.get(key, 0) + 1
    worst = np.unravel_index(err.max(-1).argmax(), bad.shape)
    raise AssertionError(
        f"{what}: {int(bad.sum())} of {bad.size} samples beyond {tol:g} of scale (largest {err.max() / scale(want):.3g} at "
        f"[b, q, m, l, p] = {tuple(int(i) for i in worst)}, pixel {tuple(float(v) for v in pxn[worst])}: got {got[worst]}, "
        f"oracle {want[worst]}); {int(leak.sum())} samples outside the map with a gradient that is not exactly zero; of these "
        f"{int(sel.sum())} samples {integer} have an integer coordinate and {border} a coordinate at -1 or n; by level "
        f"{dict(sorted(levels.items()))}; by (x, y) class {dict(sorted(classes.items(), key=lambda kv: -kv[1])[:12])} "
        f"(levels and classes: of the first 2 000)")


# =============================================================================================================== CPU tests
CPU_KEY = (DECODER, 2, 4, 150, 4, 3)          # B, M, Lq, P, seed


@pytest.mark.parametrize("shapes", PYRAMIDS + (HALF, BF16), ids=["decoder", "staged", "degenerate", "two-levels", "half", "bf16"])
@pytest.mark.parametrize("loc_dtype", [torch.float32, torch.float16, torch.bfloat16], ids=["f32", "f16", "bf16"])
def test_lattice_is_exact_and_meets_its_quotas(shapes, loc_dtype):
    """lattice_case raises unless locations and pixel coordinates are exact in loc_dtype / float32 and the quotas hold; 16-bit
    locations get the pyramids small enough for their significands (a larger one must be refused)"""
    P = 16 // len(shapes)
    if max(max(s) for s in shapes) > MAX_SIDE[loc_dtype]:
        with pytest.raises(AssertionError):
            lattice_case(shapes, 2, 8, 37, P, seed=1, loc_dtype=loc_dtype)
        return
    for Lq in (1, 37):
        sh, lsi, value, loc, attn, go = lattice_case(shapes, 2, 8, Lq, P, seed=1, loc_dtype=loc_dtype)
        assert loc.dtype == loc_dtype and loc.shape == (2, Lq, 8, len(shapes), P, 2)
        px = pixel_coordinates(loc, sh)
        n = torch.stack([sh[:, 1], sh[:, 0]], -1).double().view(1, 1, 1, -1, 1, 2)
        assert float((px == px.round()).double().mean()) >= INTEGER_QUOTA
        assert float(((px == -1) | (px == n)).double().mean()) >= BORDER_QUOTA
        assert float(px.min()) == -1.5 and bool((px.amax((0, 1, 2, 4)) == n.view(-1, 2) + 0.5).all())
        if loc_dtype == torch.float32:
            assert float((px + 1).abs()[px > -1].min()) == 2.0 ** -24         # -1 + d, just inside


@pytest.mark.parametrize("ref_dim,ref_div,off_dtype,pixels", [(2, 1, torch.float32, False), (2, 2, torch.float32, True),
                                                               (4, 1, torch.float32, False), (4, 2, torch.float32, True),
                                                               (2, 1, torch.bfloat16, False), (4, 1, torch.bfloat16, False)])
def test_fused_lattice_reproduces_the_locations_bit_for_bit(ref_dim, ref_div, off_dtype, pixels):
    """fused_lattice_case raises unless the fp32 prologue on its raw inputs gives the fp64 lattice locations exactly"""
    shapes = STAGED if pixels else DECODER
    Lq = sum(h * w for h, w in shapes) if pixels else 37
    c = fused_lattice_case(shapes, 2, 8, Lq, 4, seed=2, ref_dim=ref_dim, ref_div=ref_div, off_dtype=off_dtype,
                           queries_are_pixels=pixels)
    assert c["offsets"].dtype == off_dtype and c["ref"].shape == (2 // ref_div, Lq, 4, ref_dim)
    loc = prologue(c["offsets"].float(), c["ref"], ref_div, shapes, 4)
    assert torch.equal(loc.double(), c["loc64"])


def relative(a, b):
    return float(np.abs(a - b).max()) / scale(b)


@pytest.mark.parametrize("shapes", PYRAMIDS, ids=["decoder", "staged", "degenerate", "two-levels"])
def test_oracle_precisions_agree_on_the_lattice(shapes):
    """msda_oracle in float32 against float64, all four outputs, nothing left out: 1e-6 of each output's largest element.
    Observed maxima (forward, grad_value, grad_loc, grad_attn), B = 2, M = 4, Lq = 150, seed 3:
      decoder     1.1e-7  1.3e-7  1.6e-7  1.3e-7
      staged      1.1e-7  4.6e-7  1.7e-7  2.2e-7
      degenerate  1.3e-7  4.8e-7  2.2e-7  1.5e-7
      two-levels  0.8e-7  1.2e-7  1.6e-7  2.2e-7
    (grad_value of the small pyramids sums thousands of taps per pixel in float32), so the reference alone stays well inside
    the GPU tolerances (1e-5 / 2e-5) with no sample masked."""
    P = 16 // len(shapes)
    sh, lsi, value, loc, attn, go = lattice_case(shapes, 2, 4, 150, P, seed=3)
    a32 = (value.numpy(), sh.numpy(), lsi.numpy(), loc.numpy(), attn.numpy())
    a64 = tuple(x.astype(np.float64) if x.dtype == np.float32 else x for x in a32)
    got = (O.msda_forward(*a32),) + tuple(O.msda_backward(*a32, go.numpy()))
    want = (O.msda_forward(*a64),) + tuple(O.msda_backward(*a64, go.double().numpy()))
    errs = [relative(g.astype(np.float64), w) for g, w in zip(got, want)]
    print("oracle f32 vs f64 (forward, grad_value, grad_loc, grad_attn):", " ".join(f"{e:.2e}" for e in errs))
    assert got[0].dtype == np.float32 and want[0].dtype == np.float64
    for name, e in zip(("forward", "grad_value", "grad_loc", "grad_attn"), errs):
        assert e <= 1e-6, f"{name}: {e:.3e}"


def test_the_other_cell_is_visible_in_grad_loc_only():
    """every integer coordinate moved 2^-20 px to the left (the cell on the other side of its line): the oracle's grad_loc
    changes at order one (observed 1.79 of its scale), the continuous outputs by ~1e-6 (observed: forward 2.5e-6,
    grad_value 1.6e-6, grad_attn 2.0e-6) -- only grad_sampling_loc on the lattice can see a wrong convention"""
    sh, lsi, value, loc, attn, go = case_of(*CPU_KEY)
    px = pixel_coordinates(loc, sh)
    wh = torch.stack([sh[:, 1], sh[:, 0]], -1).double().view(1, 1, 1, -1, 1, 2)
    moved = torch.where(px == px.round(), px - 2.0 ** -20, px)
    loc2 = (moved + 0.5) / wh

    def run(l):
        a = (value.double().numpy(), sh.numpy(), lsi.numpy(), l.double().numpy(), attn.double().numpy())
        return (O.msda_forward(*a),) + tuple(O.msda_backward(*a, go.double().numpy()))
    here, there = run(loc), run(loc2)
    # (-1 - 2^-20 is outside as -1 was; n - 2^-20 comes inside with a vanishing weight: continuous as well)
    errs = [relative(t, h) for t, h in zip(there, here)]
    print("other cell (forward, grad_value, grad_loc, grad_attn):", " ".join(f"{e:.2e}" for e in errs))
    assert errs[2] > 0.1
    assert errs[0] < 1e-5 and errs[1] < 1e-5 and errs[3] < 1e-5


def test_numpy_loop_statement_equals_the_oracle_forward():
    """the independent loop statement of the forward (zero-padded map, no corner rules) on a small lattice case"""
    sh, lsi, value, loc, attn, go = lattice_case(DECODER, 1, 2, 8, 4, seed=4)
    a = (value.double().numpy(), sh.numpy(), lsi.numpy(), loc.double().numpy(), attn.double().numpy())
    want = O.msda_forward(*a)
    got = O.msda_numpy_small(*a)
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-12 * scale(want))


def test_grid_sample_agrees_except_where_a_coordinate_is_minus_one():
    """fp64 autograd through the grid_sample statement (oracle/msda_torch_fallback.py) equals the C oracle to 1e-10 of scale on
    the forward, grad_value, grad_attn and the grad_loc of every sample -- except samples with a coordinate exactly -1:
    grid_sample differentiates the padded tap there, the reference's kernel fails its range test `h > -1 && w > -1`
    (ms_deform_im2col_cuda.cuh:288) and leaves all three gradients zero (:365-374).  So the C oracle, not a grid_sample
    composition, is the authority for the lattice tests."""
    from oracle.msda_torch_fallback import msda_grid_sample
    sh, lsi, value, loc, attn, go = case_of(*CPU_KEY)
    v, lo, a = (t.double().requires_grad_(True) for t in (value, loc, attn))
    out = msda_grid_sample(v, sh.tolist(), lo, a)
    out.backward(go.double())
    args = (value.double().numpy(), sh.numpy(), lsi.numpy(), loc.double().numpy(), attn.double().numpy())
    want, rv, rl, ra = (O.msda_forward(*args),) + tuple(O.msda_backward(*args, go.double().numpy()))
    assert relative(out.detach().numpy(), want) <= 1e-10
    assert relative(v.grad.numpy(), rv) <= 1e-10
    assert relative(a.grad.numpy(), ra) <= 1e-10
    px = pixel_coordinates(loc, sh)
    minus_one = (px == -1).any(-1).numpy()                                    # [B, Lq, M, L, P]
    gl = lo.grad.numpy()
    assert float(np.abs(gl - rl)[~minus_one].max()) <= 1e-10 * scale(rl)
    assert minus_one.sum() > 100 and np.all(rl[minus_one] == 0)
    differ = (np.abs(gl - rl) > 1e-10 * scale(rl)).any(-1) & minus_one
    assert differ.sum() >= 1, "grid_sample no longer differentiates the padded tap at -1: the docstring is out of date"
    # the comparison the GPU tests make, fed with this gradient, fails and says where: every failing sample has a coordinate
    # at -1 (an integer), and a gradient that is not exactly zero outside the map
    with pytest.raises(AssertionError) as info:
        assert_per_sample(gl, rl, 2e-5, px, sh, "grad_sampling_loc")
    import re
    m = re.search(r"of these (\d+) samples (\d+) have an integer coordinate and (\d+) a coordinate at -1 or n; by level (\{.*?\})",
                  str(info.value))
    assert m and m.group(1) == m.group(2) == m.group(3) and int(m.group(1)) >= differ.sum(), str(info.value)
    assert all(f"{l}:" in m.group(4) for l in range(4)) and "'-1'" in str(info.value)


# =============================================================================================================== GPU tests
@pytest.fixture(autouse=True)
def _auto_variant():
    yield
    _lib.set_kernel_variant(0)


def dev(t, dtype):
    return t.to(DEV, dtype).contiguous()


def gpu_forward(case, variant=0, vdt=torch.float32, ldt=torch.float32):
    """vnx_msda_forward into a NaN-filled buffer between guard words"""
    sh, lsi, value, loc, attn, go = case
    B, S, M, D = value.shape
    _, Lq, _, L, P, _ = loc.shape
    v, lo, a, shd, lsid = dev(value, vdt), dev(loc, ldt), dev(attn, ldt), sh.to(DEV), lsi.to(DEV)
    out = Guarded((B, Lq, M * D), vdt)
    _lib.set_kernel_variant(variant)
    st = _lib.lib().vnx_msda_forward(CODES[vdt], CODES[ldt], v.data_ptr(), shd.data_ptr(), lsid.data_ptr(), lo.data_ptr(),
                                     a.data_ptr(), out.ptr(), B, S, M, D, L, Lq, P, torch.cuda.current_stream().cuda_stream)
    _lib.check(st)
    torch.cuda.synchronize()
    return out.read("output")


def gpu_backward(case, variant=0, vdt=torch.float32, ldt=torch.float32):
    """vnx_msda_backward (packed levels, as every model call) into three guarded buffers"""
    sh, lsi, value, loc, attn, go = case
    B, S, M, D = value.shape
    _, Lq, _, L, P, _ = loc.shape
    v, lo, a, g = dev(value, vdt), dev(loc, ldt), dev(attn, ldt), dev(go, vdt)
    shd, lsid = sh.to(DEV), lsi.to(DEV)
    outs = [Guarded(value.shape, vdt), Guarded(loc.shape, ldt), Guarded(attn.shape, ldt)]
    _lib.set_kernel_variant(variant)
    lib = _lib.lib()
    flags = _lib.MSDA_LEVELS_PACKED
    n = lib.vnx_msda_backward_workspace_bytes(CODES[vdt], CODES[ldt], B, S, M, D, L, Lq, P, flags)
    ws = torch.empty(max(n, 1), dtype=torch.uint8, device=DEV)
    st = lib.vnx_msda_backward(CODES[vdt], CODES[ldt], v.data_ptr(), shd.data_ptr(), lsid.data_ptr(), lo.data_ptr(), a.data_ptr(),
                               g.data_ptr(), outs[0].ptr(), outs[1].ptr(), outs[2].ptr(), B, S, M, D, L, Lq, P, flags,
                               ws.data_ptr() if n else None, n, torch.cuda.current_stream().cuda_stream)
    _lib.check(st)
    torch.cuda.synchronize()
    return [o.read(name) for o, name in zip(outs, ("grad_value", "grad_sampling_loc", "grad_attn_weight"))]


def check_forward(key, variant=0, vdt=torch.float32, ldt=torch.float32, tol=1e-5):
    case = case_of(*key)
    want = oracle_of(key, vdt, ldt)[0]
    got = gpu_forward(case, variant, vdt, ldt)
    err = relative(got, want)
    print(f"forward variant {variant}: {err:.2e} of scale (tolerance {tol:g})")
    if vdt == torch.float64:
        np.testing.assert_allclose(got, want, rtol=1e-9, atol=1e-12 * scale(want), err_msg="output")
    else:
        np.testing.assert_allclose(got, want, rtol=0, atol=tol * scale(want), err_msg="output")


def check_backward(key, variant=0, vdt=torch.float32, ldt=torch.float32, tol=2e-5):
    case = case_of(*key)
    sh, lsi = case[0], case[1]
    _, rv, rl, ra = oracle_of(key, vdt, ldt)
    gv, gl, ga = gpu_backward(case, variant, vdt, ldt)
    px = pixel_coordinates(case[3], sh)
    print(f"backward variant {variant}: grad_value {relative(gv, rv):.2e} grad_loc {relative(gl, rl):.2e} "
          f"grad_attn {relative(ga, ra):.2e} of scale (tolerance {tol:g})")
    if vdt == torch.float64:
        for name, got, want in (("grad_value", gv, rv), ("grad_sampling_loc", gl, rl), ("grad_attn_weight", ga, ra)):
            np.testing.assert_allclose(got, want, rtol=1e-9, atol=1e-12 * scale(want), err_msg=name)
        tol = 1e-9
    assert_levels(gv, rv, sh, lsi, tol)
    assert_per_sample(gl, rl, tol, px, sh, "grad_sampling_loc")
    assert_per_sample(ga, ra, tol, px, sh, "grad_attn_weight")


FWD_VARIANTS = [0, 1, 2, 3, 4, 5, 12, 13, 14, 15]                                      # test_msda_gpu.py
BWD_VARIANTS = [0, 1, 2, 3, 5, 12, 15, 300, 303, 420, 425, 430, 431, 444]              # whole backwards only, no timing ablation


def decoder_key(B, Lq):
    return (DECODER, B, 8, Lq, 4, 100 * B + Lq)


# ---- the decoder shape ------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("variant", FWD_VARIANTS)
@pytest.mark.parametrize("Lq", [300, 37, 1])
@pytest.mark.parametrize("B", [2, 10])
def test_decoder_forward(B, Lq, variant):
    check_forward(decoder_key(B, Lq), variant)


@pytest.mark.gpu
@pytest.mark.parametrize("variant", BWD_VARIANTS)
@pytest.mark.parametrize("Lq", [300, 37, 1])
@pytest.mark.parametrize("B", [2, 10])
def test_decoder_backward(B, Lq, variant):
    """B x M = 16 and 80 heads: both sides of gvd_units_min's switch"""
    check_backward(decoder_key(B, Lq), variant)


@pytest.mark.gpu
def test_decoder_float64_through_the_generic_kernel():
    key = decoder_key(2, 300)
    check_forward(key, 0, torch.float64, torch.float64)
    check_backward(key, 0, torch.float64, torch.float64)


# ---- the encoder shape: queries = pixels, Lq = S = 2 720 (slab forward and slab grad_loc by themselves, grad_value record- or
# tile-fed) -------------------------------------------------------------------------------------------------------------------
ENCODER_KEY = (DECODER, 2, 8, 2720, 4, 77)


@pytest.mark.gpu
@pytest.mark.parametrize("variant", [0, 730, 731, 733, 430, 431])
def test_encoder_forward_and_backward(variant):
    check_forward(ENCODER_KEY, variant)
    check_backward(ENCODER_KEY, variant)


# ---- which levels are staged; degenerate levels ---------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("shapes", [STAGED, DEGENERATE, TWO_LEVELS], ids=["staged", "degenerate", "two-levels"])
def test_staged_and_degenerate_levels(shapes):
    """the slab forward forced (730) and a decoder backward: everything staged; a 1 x 1 level (menu -1.5 ... 1.5), a one-row
    and a one-column level; L = 2 with P = 8"""
    key = (shapes, 2, 8, 300, 16 // len(shapes), 11)
    check_forward(key, 730)
    check_forward(key, 0)
    check_backward(key, 0)


# ---- other point counts on the self-decoding path ---------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("L,P", [(1, 16), (2, 8), (4, 8)])
def test_other_point_counts(L, P):
    key = (DECODER[:L], 2, 8, 300, P, 10 * L + P)
    check_forward(key)
    check_backward(key)


# ---- 16-bit -----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("vdt", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
@pytest.mark.parametrize("which", ["decoder", "encoder"])
def test_sixteen_bit_values_with_fp32_locations(which, vdt):
    key = decoder_key(2, 300) if which == "decoder" else ENCODER_KEY
    check_forward(key, 0, vdt, torch.float32, TOL16[vdt])
    check_backward(key, 0, vdt, torch.float32, TOL16[vdt])


@pytest.mark.gpu
@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
def test_sixteen_bit_locations_on_the_reduced_lattice(dt):
    """bf16 has 8 significant bits: sides <= 16, steps of 1/2; fp16 has 11: sides <= 32, steps of 1/4"""
    key = (BF16 if dt == torch.bfloat16 else HALF, 2, 8, 300, 4, 5, dt)
    check_forward(key, 0, dt, dt, TOL16[dt])
    check_backward(key, 0, dt, dt, TOL16[dt])


# ---- the fused prologue -----------------------------------------------------------------------------------------------------
def fused_expected(c, vdt):
    """the fp64 prologue in torch around the C oracle's core: loc and attn from the raw inputs, grad_loc / grad_attn from the
    oracle, pulled back to offsets, logits and reference points by autograd of (loc * gl).sum() + (attn * ga).sum()"""
    off, lg, ref = (c[k].double().requires_grad_(True) for k in ("offsets", "logits", "ref"))
    B, Lq, M, L, P, _ = off.shape
    loc = prologue(off, ref, c["ref_div"], c["shapes"], P)
    attn = torch.softmax(lg, -1).view(B, Lq, M, L, P)
    assert torch.equal(loc.detach(), c["loc64"])
    args = (c["value"].to(vdt).double().numpy(), c["sh"].numpy(), c["lsi"].numpy(), loc.detach().numpy(), attn.detach().numpy())
    want = O.msda_forward(*args, nthreads=8)
    rv, rl, ra = O.msda_backward(*args, c["go"].to(vdt).double().numpy(), nthreads=8)
    goff, glog, gref = torch.autograd.grad((loc * torch.from_numpy(rl)).sum() + (attn * torch.from_numpy(ra)).sum(), (off, lg, ref))
    return want, rv, goff.numpy(), glog.numpy(), gref.numpy()[..., :2]


def gpu_fused(c, variant, vdt, ref_grad):
    """vnx_msda_fused_forward and vnx_msda_fused_backward into guarded buffers"""
    from vnext_amd.ops.functions import level_tensors
    value, off, lg, ref, go = c["value"], c["offsets"], c["logits"], c["ref"], c["go"]
    B, S, M, D = value.shape
    _, Lq, _, L, P, _ = off.shape
    qdt = off.dtype
    ref_dim = ref.shape[-1] | (_lib.MSDA_REF_F32 if qdt != torch.float32 else 0)
    shd, lsid = level_tensors(c["shapes"], DEV)
    v, o, lgd, rf, g = dev(value, vdt), off.to(DEV), lg.to(DEV), ref.to(DEV), dev(go, vdt)
    out = Guarded((B, Lq, M * D), vdt)
    outs = [Guarded(value.shape, vdt), Guarded(off.shape, qdt), Guarded(lg.shape, qdt)] + \
        ([Guarded((B, Lq, L, 2), torch.float32)] if ref_grad else [])
    _lib.set_kernel_variant(variant)
    lib = _lib.lib()
    stream = torch.cuda.current_stream().cuda_stream
    _lib.check(lib.vnx_msda_fused_forward(CODES[vdt], CODES[qdt], v.data_ptr(), shd.data_ptr(), lsid.data_ptr(), o.data_ptr(),
                                          lgd.data_ptr(), rf.data_ptr(), out.ptr(), B, S, M, D, L, Lq, P, ref_dim, c["ref_div"], stream))
    n = lib.vnx_msda_fused_backward_workspace_bytes(CODES[vdt], B, S, M, L, Lq, P)
    ws = torch.empty(max(n, 1), dtype=torch.uint8, device=DEV)
    _lib.check(lib.vnx_msda_fused_backward(CODES[vdt], CODES[qdt], v.data_ptr(), shd.data_ptr(), lsid.data_ptr(), o.data_ptr(),
                                           lgd.data_ptr(), rf.data_ptr(), g.data_ptr(), outs[0].ptr(), outs[1].ptr(), outs[2].ptr(),
                                           outs[3].ptr() if ref_grad else None, B, S, M, D, L, Lq, P, ref_dim, c["ref_div"],
                                           ws.data_ptr(), n, stream))
    torch.cuda.synchronize()
    names = ("grad_value", "grad_offsets", "grad_logits", "grad_reference_points")
    return [out.read("output")] + [x.read(k) for x, k in zip(outs, names)]


def check_fused(c, variant, vdt, ref_grad, fwd_tol=3e-5, tol=5e-5, tol_value=None):
    """tolerances: test_msda_fused.py (forward 3e-5 of scale) and test_parity_r3.py (gradients 5e-5; 16-bit 1e-2)"""
    want, rv, roff, rlog, rref = fused_expected(c, vdt)
    got = gpu_fused(c, variant, vdt, ref_grad)
    sh, lsi = c["sh"], c["lsi"]
    px = pixel_coordinates(c["loc64"], sh)
    errs = [relative(got[0], want), relative(got[1], rv), relative(got[2], roff), relative(got[3], rlog)]
    print(f"fused variant {variant}: forward {errs[0]:.2e} grad_value {errs[1]:.2e} grad_offsets {errs[2]:.2e} "
          f"grad_logits {errs[3]:.2e}" + (f" grad_reference {relative(got[4], rref):.2e}" if ref_grad else "") +
          f" of scale (tolerances {fwd_tol:g} / {tol:g})")
    np.testing.assert_allclose(got[0], want, rtol=0, atol=fwd_tol * scale(want), err_msg="output")
    assert_levels(got[1], rv, sh, lsi, tol_value or tol)
    assert_per_sample(got[2], roff, tol, px, sh, "grad_offsets")
    np.testing.assert_allclose(got[3], rlog, rtol=0, atol=tol * scale(rlog), err_msg="grad_logits")
    if ref_grad:
        np.testing.assert_allclose(got[4], rref, rtol=0, atol=tol * scale(rref), err_msg="grad_reference_points")


FUSED_LAYOUTS = [(2, 1, True), (2, 1, False), (2, 2, False), (4, 1, False), (4, 2, False)]     # ref_dim, ref_div, ref_grad


@pytest.mark.gpu
@pytest.mark.parametrize("ref_dim,ref_div,ref_grad", FUSED_LAYOUTS)
def test_fused_prologue_at_the_decoder_shape(ref_dim, ref_div, ref_grad):
    c = fused_case_of(DECODER, 2, 8, 300, 4, 31 + ref_dim, ref_dim, ref_div)
    check_fused(c, 0, torch.float32, ref_grad)


@pytest.mark.gpu
@pytest.mark.parametrize("variant", [0, 734])
@pytest.mark.parametrize("ref_dim,ref_div,ref_grad", FUSED_LAYOUTS)
def test_fused_prologue_at_the_encoder_shape(ref_dim, ref_div, ref_grad, variant):
    c = fused_case_of(DECODER, 2, 8, 2720, 4, 41 + ref_dim, ref_dim, ref_div, torch.float32, True)
    check_fused(c, variant, torch.float32, ref_grad)


@pytest.mark.gpu
@pytest.mark.parametrize("L,P", [(1, 16), (2, 8)])
def test_fused_prologue_at_other_point_counts(L, P):
    c = fused_case_of(DECODER[:L], 2, 8, 300, P, 51 + L)
    check_fused(c, 0, torch.float32, True)


@pytest.mark.gpu
@pytest.mark.parametrize("ref_dim", [2, 4])
def test_fused_bf16_offsets_and_logits_beside_fp32_reference_points(ref_dim):
    """what torch.autocast(bfloat16) leaves at the op (VNX_MSDA_REF_F32): bf16 value, offsets and logits, fp32 reference
    points; the offsets are exact in bf16, so the locations are the lattice's all the same"""
    c = fused_case_of(DECODER, 2, 8, 300, 4, 61 + ref_dim, ref_dim, 1, torch.bfloat16)
    check_fused(c, 0, torch.bfloat16, ref_dim == 2, fwd_tol=1e-2, tol=1e-2, tol_value=TOL16[torch.bfloat16])
