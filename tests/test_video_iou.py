"""The run-table decode and the video IoU sums on the device (vnext_amd/csrc/video_iou.hip) against the numpy path
(vnext_amd/ops/video_iou.py), through the C ABI and through the Python ops; the evaluator end to end on the device
against the reference's numbers (tests/golden/ytvis_eval.npz)."""
import functools
import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN_DIR
from vnext_amd import _lib
from vnext_amd.evaluation import YTVISEval
from vnext_amd.ops import video_iou as V
from vnext_amd.utils.ytvis_json import counts_to_string, rle_encode, string_to_counts

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD, SENTINEL = 64, -0x5A5A5A5B


@functools.lru_cache(maxsize=None)
def golden():
    return dict(np.load(os.path.join(GOLDEN_DIR, "ytvis_eval.npz")))


def golden_documents():
    fx = golden()
    return json.loads(str(fx["gt_json"])), json.loads(str(fx["dt_json"]))


def alternating(h, w):
    return (np.arange(h * w) % 2 == 1).reshape((h, w), order="F")


def counted(n, seed):
    """a string of exactly n counts (differences of both signs among them) and its size"""
    rng = np.random.default_rng(seed)
    counts = rng.integers(1, 40, n)
    counts[rng.random(n) < 0.2] = 0
    counts[0] = 7
    counts[-1] = 9
    if n > 10:
        counts[5], counts[7], counts[9] = 1500, 2, 40000          # +-: three- and four-character differences
    return counts_to_string(counts.tolist()), (1, int(counts.sum()))


@functools.lru_cache(maxsize=None)
def decode_cases():
    """[(name, string, (h, w))]"""
    cases = []
    gt, recs = golden_documents()
    segs = [s for r in recs[:8] + recs[-3:] for s in r["segmentations"] if s]
    segs += [s for a in gt["annotations"] for s in a["segmentations"] if s and isinstance(s["counts"], str)]
    cases += [(f"fixture{i}", s["counts"], tuple(s["size"])) for i, s in enumerate(segs)]
    cases += [(f"{n} counts", *counted(n, n)) for n in (1, 2, 3, 4, 63, 64, 65, 129)]
    for k in (60, 61, 62, 63, 64, 125, 126, 127):          # a three-character count across the 64-byte steps of the decode
        counts = [3] * k + [5000, 3, 3, 70000, 2]
        s = counts_to_string(counts)
        assert len(s) == k + 3 + 1 + 3 + 4 + 1           # the stored differences: 4997, 0, -4997, 69997, -1
        cases.append((f"straddle {k}", s, (1, sum(counts))))
    cases.append(("checkerboard", rle_encode(alternating(24, 40))["counts"], (24, 40)))
    one = np.zeros((200, 200), bool)
    one[199, 199] = True
    cases.append(("one pixel", rle_encode(one)["counts"], (200, 200)))
    assert len(cases[-1][1]) == 5 and len(string_to_counts(cases[-2][1])) == 960
    cases.append(("empty", rle_encode(np.zeros((37, 53), bool))["counts"], (37, 53)))
    cases.append(("full", rle_encode(np.ones((37, 53), bool))["counts"], (37, 53)))
    rng = np.random.default_rng(0)
    cases.append(("random", rle_encode(rng.random((97, 131)) > 0.5)["counts"], (97, 131)))
    assert any(x < 0 for _, s, _ in cases for x in _stored_values(s))
    return cases


def _stored_values(s):
    c = string_to_counts(s)
    return [x - (c[i - 2] if i > 2 else 0) for i, x in enumerate(c)]


def raw_decode(strings, sizes):
    """the two launches through the C ABI, guard words around both run arenas
    -> (runs, ends, ones, rows, status, guards_intact)"""
    lib = _lib.lib()
    arena, offsets, lengths = V._string_arena(strings)
    M = len(strings)
    up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).astype(dt)).to(DEV)       # noqa: E731
    d_arena = up(np.concatenate((arena, np.zeros(1, np.uint8))), np.uint8)
    d_off, d_len = up(offsets, np.int64), up(lengths, np.int64)
    d_px = up([h * w for h, w in sizes], np.int32)
    runs = torch.full((M,), -1, dtype=torch.int32, device=DEV)
    st = _lib.current_stream(runs)
    _lib.check(lib.vnx_rle_runs_measure(d_arena.data_ptr(), len(arena), d_off.data_ptr(), d_len.data_ptr(), M,
                                        runs.data_ptr(), st))
    total = int(runs.sum())
    run_off = (runs.cumsum(0) - runs).to(torch.int32)
    ends = torch.full((total + 2 * GUARD,), SENTINEL, dtype=torch.int32, device=DEV)
    ones = torch.full((total + 2 * GUARD,), SENTINEL, dtype=torch.int32, device=DEV)
    rows = torch.full((M, 4), SENTINEL, dtype=torch.int32, device=DEV)
    status = torch.full((M,), SENTINEL, dtype=torch.int32, device=DEV)
    _lib.check(lib.vnx_rle_runs_write(d_arena.data_ptr(), len(arena), d_off.data_ptr(), d_len.data_ptr(), d_px.data_ptr(),
                                      run_off.data_ptr(), runs.data_ptr(), M, ends[GUARD:].data_ptr(),
                                      ones[GUARD:].data_ptr(), total, rows.data_ptr(), status.data_ptr(), st))
    e, o = ends.cpu().numpy(), ones.cpu().numpy()
    intact = all((a[:GUARD] == SENTINEL).all() and (a[GUARD + total:] == SENTINEL).all() for a in (e, o))
    return (runs.cpu().numpy(), e[GUARD:GUARD + total], o[GUARD:GUARD + total], rows.cpu().numpy(),
            status.cpu().numpy(), intact)


def test_decode_equals_the_host_builder_case_by_case():
    for name, s, size in decode_cases():
        want = V.runs_from_counts([string_to_counts(s)], [size])
        runs, ends, ones, rows, status, intact = raw_decode([s], [size])
        assert status.tolist() == [0] and intact, name
        assert runs.tolist() == [len(want.ends)], name
        assert (ends == want.ends).all() and (ones == want.ones).all() and (rows == want.rows).all(), name
        got = V.decode_strings([s], [size], device=DEV).numpy()
        assert (got.ends == want.ends).all() and (got.ones == want.ones).all() and (got.rows == want.rows).all(), name


def test_decode_of_a_mixed_batch_stays_inside_its_arenas():
    names, strings, sizes = zip(*decode_cases())
    want = V.runs_from_counts([string_to_counts(s) for s in strings], sizes)
    runs, ends, ones, rows, status, intact = raw_decode(strings, sizes)
    assert intact and not status.any() and len(strings) > 60          # more masks than one workgroup's four
    assert (runs == want.rows[:, 1]).all()
    assert (ends == want.ends).all() and (ones == want.ones).all() and (rows == want.rows).all()
    again = raw_decode(strings, sizes)                                  # two runs are byte-identical
    assert all(a.tobytes() == b.tobytes() for a, b in zip((runs, ends, ones, rows, status), again))
    got = V.decode_strings(list(strings), list(sizes), device=DEV)
    assert got.is_cuda and (got.numpy().ends == want.ends).all() and (got.numpy().rows == want.rows).all()
    empty = V.decode_strings([], [], device=DEV)
    assert len(empty) == 0 and empty.is_cuda


def test_each_malformed_kind_sets_its_status_and_nothing_else():
    h, w = 24, 40
    good = rle_encode(alternating(h, w))["counts"]
    blob = rle_encode(np.random.default_rng(4).random((h, w)) > 0.5)["counts"]
    kinds = [("\x7f" + blob[1:], _lib.RLE_RUNS_BAD_BYTE), ("/" + blob[1:], _lib.RLE_RUNS_BAD_BYTE),
             (blob[:-1] + "o", _lib.RLE_RUNS_TRUNCATED), (counts_to_string([h * w + 5, -5]), _lib.RLE_RUNS_NEGATIVE),
             ("o" * 7 + "0" + counts_to_string([h * w]), _lib.RLE_RUNS_NEGATIVE),       # a count of eight characters
             (counts_to_string([h * w - 1]), _lib.RLE_RUNS_BAD_SUM), ("", _lib.RLE_RUNS_BAD_SUM),
             (blob + "1", _lib.RLE_RUNS_BAD_SUM), ("o" * 70, _lib.RLE_RUNS_TRUNCATED)]
    want = V.runs_from_counts([string_to_counts(good)], [(h, w)])
    for bad, bit in kinds:
        strings = [good, bad, good, blob]
        runs, ends, ones, rows, status, intact = raw_decode(strings, [(h, w)] * 4)
        assert intact, (bad, bit)
        assert status[0] == status[2] == status[3] == 0 and status[1] & bit, (bad, bit, status)
        assert V.string_counts_checked(bad, h * w)[1] & bit, (bad, bit)
        assert rows[1].tolist() == [runs[0], 0, h * w, 0]                          # the empty table
        for m in (0, 2):                                                           # the neighbours' slots and rows
            off = rows[m, 0]
            assert rows[m].tolist() == [runs[:m].sum(), 960, h * w, 480]
            assert (ends[off:off + 960] == want.ends).all() and (ones[off:off + 960] == want.ones).all()
        assert rows[3, 0] == runs[:3].sum() and rows[3, 1] == len(string_to_counts(blob))
        with pytest.raises(ValueError, match="malformed RLE string of mask 1"):
            V.decode_strings(strings, [(h, w)] * 4, device=DEV)
        with pytest.raises(ValueError, match="malformed RLE string of the second"):
            V.decode_strings(strings, [(h, w)] * 4, device=DEV, labels=["a", "the second", "c", "d"])


def test_decode_refuses_slices_outside_the_byte_arena():
    lib = _lib.lib()
    arena = torch.full((16,), 48 + 4, dtype=torch.uint8, device=DEV)               # "4444...": counts of 4
    off = torch.tensor([0, 8, -1, 1 << 40], dtype=torch.int64, device=DEV)
    length = torch.tensor([1, 9, 1, 1], dtype=torch.int64, device=DEV)
    px = torch.tensor([4, 36, 4, 4], dtype=torch.int32, device=DEV)
    runs = torch.empty(4, dtype=torch.int32, device=DEV)
    st = _lib.current_stream(runs)
    _lib.check(lib.vnx_rle_runs_measure(arena.data_ptr(), 16, off.data_ptr(), length.data_ptr(), 4, runs.data_ptr(), st))
    assert runs.tolist() == [1, 0, 0, 0]
    ends, ones = torch.zeros(8, dtype=torch.int32, device=DEV), torch.zeros(8, dtype=torch.int32, device=DEV)
    rows, status = torch.zeros(4, 4, dtype=torch.int32, device=DEV), torch.zeros(4, dtype=torch.int32, device=DEV)
    run_off = torch.tensor([0, 1, 1, 1], dtype=torch.int32, device=DEV)
    _lib.check(lib.vnx_rle_runs_write(arena.data_ptr(), 16, off.data_ptr(), length.data_ptr(), px.data_ptr(),
                                      run_off.data_ptr(), runs.data_ptr(), 4, ends.data_ptr(), ones.data_ptr(), 1,
                                      rows.data_ptr(), status.data_ptr(), st))
    assert status[0] == 0 and all(int(s) & _lib.RLE_RUNS_BAD_SLOT for s in status[1:])
    assert ends.tolist() == [4] + [0] * 7 and rows[1:, 1].tolist() == [0, 0, 0]
    # a slot that the measure launch did not size: refused, nothing written
    runs[0] = 0
    ends.zero_()
    _lib.check(lib.vnx_rle_runs_write(arena.data_ptr(), 16, off.data_ptr(), length.data_ptr(), px.data_ptr(),
                                      run_off.data_ptr(), runs.data_ptr(), 4, ends.data_ptr(), ones.data_ptr(), 1,
                                      rows.data_ptr(), status.data_ptr(), st))
    assert int(status[0]) & _lib.RLE_RUNS_BAD_SLOT and not ends.any()
    assert lib.vnx_rle_runs_write(arena.data_ptr(), 16, off.data_ptr(), length.data_ptr(), px.data_ptr(),
                                  run_off.data_ptr(), runs.data_ptr(), 4, ends.data_ptr(), ones.data_ptr(), 1 << 31,
                                  rows.data_ptr(), status.data_ptr(), st) == _lib.VNX_ERR_UNSUPPORTED
    assert lib.vnx_rle_runs_measure(None, 0, None, None, 0, None, st) == 0          # masks == 0: a no-op
    assert lib.vnx_rle_runs_measure(arena.data_ptr(), 16, None, length.data_ptr(), 4, runs.data_ptr(), st) == 1


# ---- sums ----------------------------------------------------------------------------------------------------------------
def raw_sums(tables, frame_mask, tracks, pairs):
    """vnx_video_iou_sums through the C ABI on host tables, the output between guard words -> (int64 [P, 4], intact)"""
    lib = _lib.lib()
    t = tables.to(DEV)
    fm, tr, pr = V._tracks_and_pairs(frame_mask, tracks, pairs)
    up = lambda a: torch.from_numpy(np.concatenate((a.reshape(-1), np.zeros(2, np.int32)))).to(DEV)   # noqa: E731
    d_fm, d_tr, d_pr = up(fm), up(tr), up(pr)
    P = len(pr)
    out = torch.full((4 * P + 2 * GUARD,), SENTINEL, dtype=torch.int64, device=DEV)
    _lib.check(lib.vnx_video_iou_sums(t.ends.data_ptr(), t.ones.data_ptr(), len(t.ends), t.rows.data_ptr(), len(t),
                                      d_fm.data_ptr(), len(fm), d_tr.data_ptr(), len(tr), d_pr.data_ptr(), P,
                                      out[GUARD:].data_ptr(), _lib.current_stream(out)))
    o = out.cpu().numpy()
    return o[GUARD:GUARD + 4 * P].reshape(P, 4), bool((o[:GUARD] == SENTINEL).all() and (o[GUARD + 4 * P:] == SENTINEL).all())


def blobs(h, w, n, seed):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    out = []
    for _ in range(n):
        m = np.zeros((h, w), bool)
        for _ in range(int(rng.integers(1, 4))):
            cy, cx, r = rng.uniform(0, h), rng.uniform(0, w), rng.uniform(2, max(h, w) / 3)
            m |= (yy - cy) ** 2 + (xx - cx) ** 2 <= r * r
        out.append(m ^ (rng.random((h, w)) > 0.97))
    return out


@functools.lru_cache(maxsize=None)
def sums_case():
    """tables of two mask sizes, tracks with absent frames, every (detection, ground truth) pair of each size"""
    masks = blobs(37, 53, 30, 1) + blobs(97, 131, 30, 2)
    masks += [np.zeros((24, 40), bool), alternating(24, 40), np.ones((24, 40), bool)]       # runs: 1, 960, 2
    tables = V.runs_from_counts([string_to_counts(rle_encode(m)["counts"]) for m in masks], [m.shape for m in masks])
    assert tables.rows[60:, 1].tolist() == [1, 960, 2]
    rng = np.random.default_rng(3)
    frame_mask, tracks = [], []
    for base in (0, 30):
        for _ in range(7):                                        # seven tracks of five frames per size
            tracks.append((len(frame_mask), 5))
            ids = base + rng.integers(0, 30, 5)
            ids[rng.random(5) < 0.3] = -1
            frame_mask += ids.tolist()
    tracks += [(len(frame_mask), 1), (len(frame_mask) + 1, 1), (len(frame_mask) + 2, 1)]
    frame_mask += [60, 61, 62]
    pairs = [(d, g) for base in (0, 7) for d in range(base, base + 7) for g in range(base, base + 7)]
    pairs += [(14, 15), (15, 14), (15, 15), (16, 15), (14, 14)]   # 1 run against 960, both ways round
    return tables, frame_mask, tracks, pairs


def test_sums_equal_the_numpy_path():
    tables, frame_mask, tracks, pairs = sums_case()
    assert any(m < 0 for m in frame_mask)
    want = V.pair_sums_host(tables, frame_mask, tracks, pairs)
    assert not want[:, 3].any() and (want[:, 0] > 0).sum() > 40
    assert want[-5:].tolist() == [[0, 0, 480, 0], [0, 480, 0, 0], [480, 480, 480, 0], [480, 960, 480, 0], [0, 0, 0, 0]]
    got, intact = raw_sums(tables, frame_mask, tracks, pairs)
    assert intact and (got == want).all()
    again, _ = raw_sums(tables, frame_mask, tracks, pairs)
    assert got.tobytes() == again.tobytes()                       # two runs are byte-identical
    assert (V.pair_sums(tables.to(DEV), frame_mask, tracks, pairs) == want).all()
    for P in (1, 0, 5):                                           # one pair, none, a last workgroup that is not full
        got, intact = raw_sums(tables, frame_mask, tracks, pairs[:P])
        assert intact and (got == want[:P]).all()
        assert (V.pair_sums(tables.to(DEV), frame_mask, tracks, pairs[:P]) == want[:P]).all()


def test_sums_on_the_fixture_pairs():
    gt, recs = golden_documents()
    fx = golden()
    host = YTVISEval(gt, device="cpu", area_rng=fx["area_rng"].tolist()).add(recs)
    dev = YTVISEval(gt, device=DEV, area_rng=fx["area_rng"].tolist()).add(recs)
    seen = {}

    def spy(name, fn):
        def wrapped(tables, frame_mask, tracks, pairs):
            seen[name] = fn(tables, frame_mask, tracks, pairs)
            seen[name + " cuda"] = tables.is_cuda
            return seen[name]
        return wrapped
    real = V.pair_sums
    try:
        V.pair_sums = spy("host", real)
        host.evaluate()
        V.pair_sums = spy("dev", real)
        dev.evaluate()
    finally:
        V.pair_sums = real
    assert seen["dev cuda"] and not seen["host cuda"]
    assert seen["host"].shape == seen["dev"].shape and len(seen["host"]) > 100
    assert (seen["host"] == seen["dev"]).all()


def test_mismatched_tracks_set_the_status_and_read_nothing_outside():
    tables, frame_mask, tracks, pairs = sums_case()
    F = len(frame_mask)
    tracks = list(tracks) + [(0, 4), (F - 2, 5), (-1, 2), (F - 1, 1)]              # 17: shorter; 18, 19: outside; 20
    bad_pairs = [(0, 17), (17, 0), (0, 7), (0, 18), (19, 19), (0, 99), (-1, 0), (0, 0), (20, 20)]
    want = V.pair_sums_host(tables, frame_mask, tracks, bad_pairs)
    assert want[:, 3].tolist() == [1, 1, 2, 4, 4, 4, 4, 0, 0] and not want[:7, :3].any()
    got, intact = raw_sums(tables, frame_mask, tracks, bad_pairs)
    assert intact and (got == want).all()
    # rows and mask indices that point outside the tables
    broken = V.RunTables(tables.ends, tables.ones, tables.rows.copy())
    broken.rows[3] = (len(tables.ends) - 2, 5, 37 * 53, 7)
    broken.rows[4] = (-4, 5, 37 * 53, 7)
    fm = [3, 4, len(tables), 0]
    tr = [(0, 1), (1, 1), (2, 1), (3, 1)]
    pr = [(0, 3), (3, 1), (2, 3), (3, 3)]
    want = V.pair_sums_host(broken, fm, tr, pr)
    assert want[:, 3].tolist() == [4, 4, 4, 0]
    got, intact = raw_sums(broken, fm, tr, pr)
    assert intact and (got == want).all()
    lib = _lib.lib()
    assert lib.vnx_video_iou_sums(None, None, 0, None, 0, None, 0, None, 0, None, 0, None, None) == 0     # P == 0
    assert lib.vnx_video_iou_sums(None, None, 0, None, 0, None, 0, None, 0, None, -1, None, None) == 1
    with pytest.raises(ValueError, match="differ in frame count"):
        gt, recs = golden_documents()
        short = dict(recs[0], segmentations=recs[0]["segmentations"][:-1])
        YTVISEval(gt, device=DEV).add([short]).evaluate()


# ---- end to end ------------------------------------------------------------------------------------------------------------
def test_evaluator_on_the_device_reproduces_the_reference():
    from test_ytvis_eval import assert_equals_golden
    gt, recs = golden_documents()
    fx = golden()
    res = YTVISEval(gt, device="cuda", area_rng=fx["area_rng"].tolist()).add(recs).evaluate()
    assert_equals_golden(res, fx)
    assert YTVISEval(gt, area_rng=fx["area_rng"].tolist()).device == "cuda"         # None: the device when there is one
    with pytest.raises(ValueError, match="malformed RLE string of record 0 .*frame 1"):
        segs = [dict(s) for s in recs[0]["segmentations"]]
        segs[1]["counts"] = segs[1]["counts"][:-1] + "o"
        YTVISEval(gt, device="cuda").add([dict(recs[0], segmentations=segs)]).evaluate()


def test_the_three_matching_routes_agree_on_the_device_and_the_kernel_route_repeats():
    from test_ytvis_eval import assert_same_eval_vids
    gt, recs = golden_documents()
    res = {}
    for name, matching in (("device", "device"), ("vectorised", "vectorised"), ("host", "host"), ("again", "device")):
        ev = YTVISEval(gt, device="cuda", area_rng=golden()["area_rng"].tolist(), matching=matching).add(recs)
        res[name] = ev.evaluate()
        assert ev.timings["matching"] == matching and not ev.timings["host_fallback"]
    for name in ("vectorised", "host", "again"):
        for k in ("precision", "recall", "scores", "stats"):
            assert res[name][k].tobytes() == res["device"][k].tobytes(), (name, k)
        assert_same_eval_vids(res[name], res["device"])
    for key in res["device"]["ious"]:
        assert np.asarray(res["again"]["ious"][key]).tobytes() == np.asarray(res["device"]["ious"][key]).tobytes()
