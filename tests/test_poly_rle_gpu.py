"""GPU: vnx_poly_rle (vnext_amd/csrc/poly_rle.hip) against the host restatement (vnext_amd/ops/poly_rle.py), with no
tolerance: run ends, set pixels, rows and slot padding are compared word for word."""
import numpy as np
import pytest
import torch

from test_poly_rle import golden, sweep_triangles
from vnext_amd import _lib
from vnext_amd.ops import poly_rle as P
from vnext_amd.ops import video_iou as V

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def assert_equals_host(objects, sizes, counts=None, all_on_device=True):
    """one polygons_to_runs call on the device: every object's runs, ones, row and slot padding equal the host's"""
    planned = P.plan_objects(objects, sizes)
    assert planned[2].all() == all_on_device
    t = P.polygons_to_runs(objects, sizes, device=DEV, planned=planned)
    assert t.is_cuda and t.ends.dtype == torch.int32 and t.rows.shape == (len(objects), 4)
    assert not t.status.cpu().numpy().any()
    n = t.numpy()
    counts = [P.object_counts_host(o, *s) for o, s in zip(objects, sizes)] if counts is None else counts
    want = V.runs_from_counts(counts, sizes)
    assert (n.rows[:, 1:] == want.rows[:, 1:]).all()
    lens = want.rows[:, 1].astype(np.int64)
    at = np.repeat(n.rows[:, 0].astype(np.int64), lens) + (np.arange(lens.sum()) - np.repeat(np.cumsum(lens) - lens, lens))
    assert (n.ends[at] == want.ends).all() and (n.ones[at] == want.ones).all()
    assert (t.slot_rows[:, 0] == n.rows[:, 0]).all() and (t.slot_rows[:, 1] >= lens).all()
    for m in np.flatnonzero(t.slot_rows[:, 1] > lens)[:2000]:                     # the padding: zero-length runs at h * w
        a, b = n.rows[m, 0] + lens[m], t.slot_rows[m].sum()
        assert (n.ends[a:b] == n.rows[m, 2]).all() and (n.ones[a:b] == n.rows[m, 3]).all(), m
    return t


def test_contraction_sweep():
    """20 000 triangles on the 0.2 grid in one launch, of which the fixture's `sweep_fused` would change under a fused
    multiply-add: the kernel's line expressions are a product and two additions, as in an x86-64 build of the original"""
    fx = golden()
    assert len(fx["sweep_fused"]) >= 10
    xy, want = sweep_triangles()
    h, w = (int(v) for v in fx["sweep_size"])
    assert_equals_host([[p] for p in xy], [(h, w)] * len(xy), counts=want)


def test_every_edge_direction():
    """fans of triangles whose first edge runs over every vector of [-30, 30]^2 upsampled units"""
    objects = [[[12.0, 12.0, 12.0 + a / 5, 12.0 + b / 5, 15.4, 9.8]] for a in range(-30, 31) for b in range(-30, 31)]
    assert_equals_host(objects, [(24, 24)] * len(objects))


def ring(k, cx, cy, r, seed):
    rng = np.random.default_rng(seed)
    th = np.sort(rng.uniform(0, 2 * np.pi, k))
    rad = r * (1 + 0.2 * np.sin(7 * th) + 0.07 * np.sin(31 * th + 1))
    xy = np.empty(2 * k)
    xy[0::2], xy[1::2] = cx + rad * np.cos(th), cy + rad * np.sin(th)
    return xy


SHAPES = [
    ("ring of 600 vertices", [ring(600, 320, 240, 150, 0)], (480, 640)),
    ("ring leaving the canvas", [ring(300, 600, 400, 150, 1)], (480, 640)),
    ("wholly outside, left", [[-9.5, -3, -2.5, -3, -2.5, -1]], (5, 6)),
    ("wholly outside, right and below", [[7, 6, 9, 6, 9, 9]], (5, 6)),
    ("touches row h in the last column", [[4, 3, 6, 3, 6, 5, 4, 5]], (5, 6)),
    ("beyond row h in the last column", [[3.5, 2.5, 8, 2.5, 8, 9, 3.5, 9]], (5, 6)),
    ("the whole canvas", [[0, 0, 6, 0, 6, 5, 0, 5]], (5, 6)),
    ("repeated vertices", [[1, 1, 1, 1, 5, 1, 5, 5, 5, 5, 5, 5]], (8, 8)),
    ("the reference's dummy", [[0.0] * 6], (7, 9)),
    ("no polygon", [], (7, 9)),
    ("a box", [1, 1, 2, 2], (4, 5)),
    ("two boxes", [[1, 1, 2, 2], [4, 1, 1, 3]], (5, 6)),
    ("disjoint", [[1, 1, 4, 1, 4, 4], [10, 10, 14, 10, 14, 14, 10, 14]], (16, 18)),
    ("nested", [[1, 1, 14, 1, 14, 14, 1, 14], [4, 4, 8, 4, 8, 8, 4, 8]], (16, 18)),
    ("overlapping", [[1, 1, 9, 1, 9, 9, 1, 9], [5, 5, 14, 5, 14, 14, 5, 14], [0.5, 7.2, 16.1, 8.4, 3.3, 12.9]], (16, 18)),
    ("an identical pair", [[1, 1, 9, 2, 5, 9], [1, 1, 9, 2, 5, 9]], (16, 18)),
    ("abutting", [[1, 1, 5, 1, 5, 5, 1, 5], [5, 1, 9, 1, 9, 5, 5, 5]], (16, 18)),
    ("1 x 1", [[0, 0, 1, 0, 1, 1, 0, 1]], (1, 1)),
    ("1 x 1, outside", [[2, 0, 3, 0, 3, 1]], (1, 1)),
    ("1 x N", [[2.4, -1, 9.7, -1, 9.7, 3, 2.4, 3]], (1, 13)),
    ("N x 1", [[-1, 2.4, 3, 2.4, 3, 9.7, -1, 9.7]], (13, 1)),
    ("bow tie", [[1, 1, 14, 12, 14, 1, 1, 12]], (16, 18)),
    ("pentagram", [[8, 1, 12.1, 14.5, 1.3, 6.2, 14.7, 6.2, 3.9, 14.5]], (16, 18)),
    ("negative coordinates", [[-7.3, -2.2, 11.9, 3.1, 4.4, 19.6]], (16, 18)),
]


def test_shapes():
    assert_equals_host([s[1] for s in SHAPES], [s[2] for s in SHAPES])


def test_objects_beyond_the_caps_are_spliced_in_from_the_host():
    rng = np.random.default_rng(5)
    big = np.empty(2 * 1500)
    big[0::2], big[1::2] = rng.uniform(0, 60, 1500), rng.uniform(0, 50, 1500)    # more vertices than the kernel takes
    objects = [[[1, 1, 5, 1, 5, 5]], [big], [1, 1, 2, 2], [big[:400]], []]
    sizes = [(8, 8), (50, 60), (4, 5), (50, 60), (3, 3)]
    assert P.plan_objects(objects, sizes)[2].tolist() == [True, False, True, False, True]
    t = assert_equals_host(objects, sizes, all_on_device=False)
    both = V.concat_tables(t, t).numpy()
    assert (both.rows[5:, 0] == both.rows[:5, 0] + len(t.ends)).all()


def raw_launch(coords, prow, orow, run_slots, guard=64, fill=-7):
    """vnx_poly_rle on hand-made tables, the output arenas between guard words"""
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)          # noqa: E731
    c, p, o = up(np.asarray(coords, np.float64)), up(np.asarray(prow, np.int32).reshape(-1, 4)), \
        up(np.asarray(orow, np.int32).reshape(-1, 6))
    M = o.shape[0]
    ends = torch.full((run_slots + 2 * guard,), fill, dtype=torch.int32, device=DEV)
    ones = ends.clone()
    rows = torch.full((M + 2, 4), fill, dtype=torch.int32, device=DEV)
    status = torch.full((M + 2,), fill, dtype=torch.int32, device=DEV)
    _lib.check(_lib.lib().vnx_poly_rle(c.data_ptr(), c.shape[0], p.data_ptr(), p.shape[0], o.data_ptr(), M,
                                       ends[guard:].data_ptr(), ones[guard:].data_ptr(), run_slots, rows[1:].data_ptr(),
                                       status[1:].data_ptr(), torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    ends, ones, rows, status = (t.cpu().numpy() for t in (ends, ones, rows, status))
    for arena in (ends, ones):
        assert (arena[:guard] == fill).all() and (arena[guard + run_slots:] == fill).all()
    assert (rows[0] == fill).all() and (rows[-1] == fill).all() and status[0] == fill and status[-1] == fill
    return ends[guard:guard + run_slots], ones[guard:guard + run_slots], rows[1:-1], status[1:-1]


def test_every_status_bit_without_a_fault():
    """malformed TABLES, one object per case, good neighbours between them: each returns its status, the empty table and
    writes nothing outside its own slot"""
    tri = [1, 1, 5, 1, 5, 5]
    want = P.poly_counts_host(tri, 8, 8)                                          # 7 runs
    many = [float(v) for k in range(_lib.POLY_RLE_MAX_VERTICES + 1) for v in (k % 7, k % 5)]
    cases = [                       # (polygons of the object, h, w, slot size, expected status)
        ([tri], 8, 8, 8, 0),
        ([[1, 1, float("nan"), 1, 5, 5]], 8, 8, 8, _lib.POLY_RLE_BAD_COORD),
        ([[1, 1, 2.0 ** 25, 1, 5, 5]], 8, 8, 8, _lib.POLY_RLE_BAD_COORD),
        ([[1, 1, float("inf"), 1, 5, 5]], 8, 8, 8, _lib.POLY_RLE_BAD_COORD),
        ([tri[:4]], 8, 8, 8, _lib.POLY_RLE_FEW_VERTICES),
        ([tri], 0, 8, 8, _lib.POLY_RLE_BAD_SIZE),
        ([tri], 65536, 32768, 8, _lib.POLY_RLE_BAD_SIZE),
        ([many], 8, 8, 8, _lib.POLY_RLE_CAP),
        ([[0, 0, 60000, 0, 60000, 5]], 8, 8, 8, _lib.POLY_RLE_CAP),               # more dense points than the cap
        ([tri] * (_lib.POLY_RLE_MAX_POLYGONS + 1), 8, 8, 8, _lib.POLY_RLE_CAP),
        ([tri], 8, 8, 3, _lib.POLY_RLE_BAD_SLOT),                                 # 7 runs do not fit 3 words
        ([tri], 8, 8, 8, 0),
    ]
    coords, prow, orow, off = [], [], [], 0
    for m, (polys, h, w, slot, _) in enumerate(cases):
        orow.append([len(prow), len(polys), off, slot, h, w])
        for p in polys:
            prow.append([len(coords), len(p) // 2, m, 0])
            coords += p
        off += slot
    n = len(cases)
    # tables that point outside: a slot beyond the arena, a negative slot offset, polygons beyond the table, coordinates
    # beyond the arena, a polygon that names another object
    extra = [([len(prow) - 1, 1, off - 4, 8, 8, 8], None), ([len(prow) - 1, 1, -3, 8, 8, 8], None),
             ([len(prow) - 1, 5, 0, 0, 8, 8], None), ([len(prow), 1, 0, 0, 8, 8], [len(coords) - 2, 3, n + 3, 0]),
             ([0, 1, 0, 0, 8, 8], None)]
    for row, poly in extra:
        orow.append(row)
        if poly is not None:
            prow.append(poly)
    ends, ones, rows, status = raw_launch(coords, prow, orow, off)
    assert status[:n].tolist() == [c[4] for c in cases]
    assert all(int(s) == _lib.POLY_RLE_BAD_SLOT for s in status[n:]), status[n:]
    for m, (polys, h, w, slot, st) in enumerate(cases):
        o = orow[m][2]
        hw = h * w if 1 <= h * w < 2 ** 31 else 0
        if st == 0:
            assert rows[m].tolist() == [o, 7, 64, sum(want[1::2])]
            assert ends[o:o + 7].tolist() == np.cumsum(want).tolist() and ends[o + 7] == 64 and ones[o + 7] == rows[m, 3]
        else:                                                                     # the empty table, the slot the empty mask
            assert rows[m].tolist() == [o, 0, hw, 0]
            assert (ends[o:o + slot] == hw).all() and (ones[o:o + slot] == 0).all()
    assert (rows[n:, 1] == 0).all() and (rows[n:, 3] == 0).all()


def test_an_oversized_slot_is_capped():
    big = _lib.POLY_RLE_MAX_CROSSINGS + 40
    ends, ones, rows, status = raw_launch([1, 1, 5, 1, 5, 5], [[0, 3, 0, 0]], [[0, 1, 0, big, 8, 8]], big, fill=-7)
    assert status.tolist() == [_lib.POLY_RLE_CAP] and rows[0].tolist() == [0, 0, 64, 0]
    assert (ends[:_lib.POLY_RLE_MAX_CROSSINGS + 1] == 64).all() and (ends[_lib.POLY_RLE_MAX_CROSSINGS + 1:] == -7).all()


def test_two_runs_are_byte_identical():
    objects, sizes = [s[1] for s in SHAPES] * 8, [s[2] for s in SHAPES] * 8
    a = P.polygons_to_runs(objects, sizes, device=DEV)
    b = P.polygons_to_runs(objects, sizes, device=DEV)
    for x, y in zip((a.ends, a.ones, a.rows, a.status), (b.ends, b.ones, b.rows, b.status)):
        assert torch.equal(x, y)


def test_replays_in_a_hip_graph_on_other_coordinates():
    """one capture of the launch, replayed on other coordinates of the same layout (same vertex counts, same slots)"""
    from test_graph_capture import hip_graph_capture
    rng = np.random.default_rng(6)
    sizes = [(24, 30)] * 40

    def draw():
        return [[rng.uniform(-3, 33, 2 * k) for k in (3, 5, 8)[:1 + m % 3]] for m in range(40)]
    sets = [draw() for _ in range(3)]
    planned = P.plan_objects(sets[0], sizes)
    slots = np.full(40, (3 + 5 + 8) * 30 + 3 + 1)            # the bound of ANY such object: at most w per edge, + 1 per polygon, + 1
    assert (planned[1] <= slots).all()
    tables = [P.pack_tables(P.plan_objects(o, sizes)[0], sizes, slots) for o in sets]
    assert all((t[1] == tables[0][1]).all() and (t[2] == tables[0][2]).all() for t in tables)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)          # noqa: E731
    static = {"coords": up(tables[0][0]), "prow": up(tables[0][1]), "orow": up(tables[0][2])}

    def run(s):
        t, status = P.poly_rle_device(s["coords"], s["prow"], s["orow"], tables[0][3])
        return {"ends": t.ends, "ones": t.ones, "rows": t.rows, "status": status}
    results, replay = hip_graph_capture(run, static)
    for objects, (coords, _, _, _) in list(zip(sets, tables))[1:]:
        static["coords"].copy_(up(coords))
        replay()
        assert not results["status"].any()
        rows, ends = results["rows"].cpu().numpy(), results["ends"].cpu().numpy()
        for m, o in enumerate(objects):
            c = P.object_counts_host(o, *sizes[m])
            assert rows[m, 1] == len(c) and ends[rows[m, 0]:rows[m, 0] + len(c)].tolist() == np.cumsum(c).tolist()
