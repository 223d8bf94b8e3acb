"""The matching kernel of the AP evaluators (vnext_amd/csrc/ap_match.hip through vnext_amd/ops/ap_match.py) against
`match_host`, the plain-Python statement of the reference's decisions.  Every comparison is exact."""
import functools

import numpy as np
import pytest

from vnext_amd import _lib
from vnext_amd.ops import ap_match as M

AREA_RNG = np.array([[0, 1e10], [0, 1024], [1024, 9216], [9216, 1e10]], dtype=np.float64)
THRS = np.linspace(.5, 0.95, 10)
# ties are frequent, and the values the decisions turn on are in: a threshold itself, the cap 1 - 1e-10 and 1.0
IOU_VALUES = np.array([0.0, 0.0, 0.0, 0.3, 0.5, 0.55, 0.75, 0.95, 1 - 1e-10, 1.0])
AREAS = np.array([0.0, 500.0, 1024.0, 1024.5, 5000.0, 9216.0, 9216.5, 20000.0])     # on and around every boundary
NAMES = ("dt_match", "dt_ignore", "gt_match", "gt_ignore")
FORCED = [(100, 65), (100, 33), (0, 65), (100, 0), (0, 0), (1, 1), (3, 2), (1, 65), (3, 33)]


def random_problems(seed=0, problems=200, gaps=True):
    """-> (table, ious, gt_crowd, gt_area, dt_area, area_rng, thrs) in numpy; D in {0, 1, 3, 100}, G in {0, 1, 2, 33, 65}, a
    third of the ground truths crowds; with `gaps`, elements between the problems that no problem owns"""
    rng = np.random.default_rng(seed)
    rows, n_dt, n_gt, n_iou = [], 0, 0, 0
    for p in range(problems):
        if p < len(FORCED):
            D, G = FORCED[p]
        else:
            D = int(rng.choice([0, 1, 3, 100], p=[0.2, 0.35, 0.35, 0.1]))
            G = int(rng.choice([0, 1, 2, 33, 65], p=[0.15, 0.3, 0.3, 0.15, 0.1]))
        if gaps and p % 7 == 3:
            n_dt, n_gt, n_iou = n_dt + 2, n_gt + 3, n_iou + 5
        rows.append((D, G, n_dt, n_gt, n_iou))
        n_dt, n_gt, n_iou = n_dt + D, n_gt + G, n_iou + D * G
    order = rng.permutation(problems)                        # the table's rows need not follow the arrays' order
    table = np.array(rows, dtype=np.int64)[order]
    return (table, rng.choice(IOU_VALUES, n_iou), (rng.random(n_gt) < 1 / 3).astype(np.uint8), rng.choice(AREAS, n_gt),
            rng.choice(AREAS, n_dt), AREA_RNG.copy(), THRS.copy())


@functools.lru_cache(maxsize=None)
def reference():
    """the 200 problems and `match_host`'s answer, computed once"""
    args = random_problems(seed=0, problems=200)
    return args, M.match_host(*args)


def assert_same(got, want):
    for name in NAMES:
        x, y = getattr(got, name), getattr(want, name)
        assert x.dtype == y.dtype and x.shape == y.shape, name
        assert (x == y).all(), (name, int((x != y).sum()))


# ---- the host statement, by hand ---------------------------------------------------------------------------------------
def test_match_host_by_hand():
    """One problem, D = 4, G = 3: two regular ground truths and a crowd (last).  d0 sees both regular ones at 0.8: the
    later one wins the tie.  d1 sees g1 at 0.9 (taken) and g0 at 0.6.  d2 and d3 see only the crowd: both take it."""
    ious = np.array([[0.8, 0.8, 0.0], [0.6, 0.9, 0.0], [0.0, 0.0, 0.9], [0.1, 0.2, 0.7]])
    table = np.array([[4, 3, 0, 0, 0]])
    m = M.match_host(table, ious, [0, 0, 1], [100.0, 100.0, 100.0], [100.0, 100.0, 100.0, 2000.0],
                     [[0, 1e10], [0, 1024]], [0.5, 0.65, 0.95])
    assert m.dt_match[0].tolist() == [[1, 0, 2, 2], [1, -1, 2, 2], [-1, -1, -1, -1]]
    assert m.gt_match[0].tolist() == [[1, 0, 3], [-1, 0, 3], [-1, -1, -1]]
    assert m.gt_ignore.tolist() == [[0, 0, 1], [0, 0, 1]]
    assert m.dt_ignore[0].tolist() == [[0, 0, 1, 1], [0, 0, 1, 1], [0, 0, 0, 0]]
    # the small range: the unmatched d3 (area 2000) is ignored there, the matched ones take their ground truth's flag
    assert m.dt_ignore[1].tolist() == [[0, 0, 1, 1], [0, 0, 1, 1], [0, 0, 0, 1]]
    # a regular match ends the walk before the ignored ones: with g0, g1 outside the range they are ignored as well and
    # d0 takes the last of the three at its best IoU
    m = M.match_host(table, ious, [0, 0, 1], [5000.0, 5000.0, 100.0], [1.0] * 4, [[0, 1024]], [0.5])
    assert m.gt_ignore.tolist() == [[1, 1, 1]] and m.dt_match[0, 0].tolist() == [1, 0, 2, 2]
    # 1 - 1e-10 is the cap of the threshold: an IoU of exactly that value matches at threshold 1.0, one below does not
    for v, want in ((1 - 1e-10, 0), (1 - 2e-10, -1), (1.0, 0)):
        m = M.match_host([[1, 1, 0, 0, 0]], [v], [0], [10.0], [10.0], [[0, 1e10]], [1.0])
        assert m.dt_match.reshape(-1).tolist() == [want]


def test_a_table_that_leaves_its_arrays_raises_on_the_host():
    args = list(random_problems(seed=1, problems=4, gaps=False))
    for col, name in ((2, "dt"), (3, "gt"), (4, "iou")):
        bad = args[0].copy()
        bad[0, col] += 10 ** 6
        for fn in (M.match_host, M.match_vectorised):
            with pytest.raises(ValueError, match="points outside its arrays"):
                fn(bad, *args[1:])


def test_cpu_tensors_raise():
    import torch
    args = random_problems(seed=1, problems=4)
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        M.ap_match(*(torch.from_numpy(a) for a in args))
    assert (M.MAX_GT, M.MAX_LANES) == (512, 64)


# ---- the kernel ----------------------------------------------------------------------------------------------------------
def on_device(args):
    import torch
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in args]


@pytest.mark.gpu
def test_kernel_equals_match_host_on_200_random_problems():
    args, want = reference()
    D, G = args[0][:, 0], args[0][:, 1]
    assert set(D.tolist()) == {0, 1, 3, 100} and set(G.tolist()) == {0, 1, 2, 33, 65} and len(D) == 200
    assert ((D == 100) & (G == 65)).any() and 0.25 < args[2].mean() < 0.42
    assert (want.dt_match >= 0).mean() > 0.05 and (want.dt_ignore != 0).any() and (want.gt_ignore == 0).any()
    got = M.ap_match(*on_device(args))
    assert not got.host_fallback
    assert_same(got.numpy(), want)
    again = M.ap_match(*on_device(args)).numpy()             # no atomics: byte-identical run to run
    for name in NAMES:
        assert getattr(again, name).tobytes() == getattr(got.numpy(), name).tobytes()


@pytest.mark.gpu
def test_one_ground_truth_above_the_limit_takes_the_host():
    rng = np.random.default_rng(3)
    G = M.MAX_GT + 1
    for g, fallback in ((G, True), (M.MAX_GT, False)):
        table = np.array([[2, 3, 0, 0, 0], [3, g, 2, 3, 6]], dtype=np.int64)
        args = (table, rng.choice(IOU_VALUES, 6 + 3 * g), (rng.random(3 + g) < 1 / 3).astype(np.uint8),
                rng.choice(AREAS, 3 + g), rng.choice(AREAS, 5), AREA_RNG, THRS)
        got = M.ap_match(*on_device(args))
        assert got.host_fallback is fallback
        assert_same(got.numpy(), M.match_host(*args))
    # more lanes than a wave has: 7 area ranges x 10 thresholds
    wide = np.concatenate([AREA_RNG, AREA_RNG[1:]])
    args = random_problems(seed=2, problems=12)[:5] + (wide, THRS)
    got = M.ap_match(*on_device(args))
    assert got.host_fallback and got.dt_match.shape[0] == 7
    assert_same(got.numpy(), M.match_host(*args))


@pytest.mark.gpu
def test_a_row_past_the_end_sets_the_status_and_writes_nothing():
    import torch
    args = list(random_problems(seed=4, problems=6, gaps=False))
    table = args[0]
    n_dt, n_gt = len(args[4]), len(args[3])
    A, T, GUARD, FILL = len(AREA_RNG), len(THRS), 64, 77

    def run(table):
        dev = on_device([table] + args[1:])
        bufs = [torch.full((n + 2 * GUARD,), FILL, dtype=dt, device="cuda")
                for n, dt in ((A * T * n_dt, torch.int32), (A * T * n_dt, torch.uint8), (A * T * n_gt, torch.int32),
                              (A * n_gt, torch.uint8))]
        views = [b[GUARD:len(b) - GUARD] for b in bufs]
        out = M.Matches(views[0].view(A, T, n_dt), views[1].view(A, T, n_dt), views[2].view(A, T, n_gt),
                        views[3].view(A, n_gt))
        status = torch.zeros(1, dtype=torch.int32, device="cuda")
        M.match_into(*dev, out, status)
        torch.cuda.synchronize()
        for b in bufs:
            assert (b[:GUARD] == FILL).all() and (b[len(b) - GUARD:] == FILL).all()
        return out.numpy(), int(status)

    # every row bad, each in another way: nothing at all is written
    rows = []
    for p, (col, value) in enumerate(((2, n_dt), (3, n_gt + 1), (4, len(args[1]) + 1), (0, -1), (2, -5), (1, 2 ** 40))):
        row = table[p].copy()
        row[col] = value
        rows.append(row)
    rows[0][0] = max(rows[0][0], 1)                          # D >= 1 at offset n_dt: one past the end
    out, status = run(np.array(rows, dtype=np.int64))
    assert status == _lib.AP_MATCH_BAD_TABLE
    for name in NAMES:
        assert (getattr(out, name) == FILL).all(), name
    # one bad row among good ones: the good ones are matched, the bad one's slots keep the fill
    want = M.match_host(*args)
    p = int(np.argmax(table[:, 0] * table[:, 1]))            # the row to break owns detections and ground truths
    D, G, dof, gof, _ = table[p].tolist()
    assert D > 0 and G > 0
    bad = table.copy()
    bad[p, 4] = len(args[1]) - D * G + 1                     # its IoU matrix ends one past the end
    out, status = run(bad)
    assert status == _lib.AP_MATCH_BAD_TABLE
    for name in NAMES:
        got, ref = getattr(out, name).copy(), getattr(want, name)
        sl = slice(gof, gof + G) if name.startswith("gt") else slice(dof, dof + D)
        assert (got[..., sl] == FILL).all(), name
        got[..., sl] = ref[..., sl]
        assert (got == ref).all(), name
    with pytest.raises(ValueError, match="points outside its arrays"):
        M.ap_match(*on_device([bad] + args[1:]))
    out, status = run(table)                                 # and the table as it was
    assert status == 0
    assert_same(out, want)
