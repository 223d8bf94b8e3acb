"""The device tracker's memory bank, read back after every frame, and frames of more than 64 detections.

`tests/test_tracker.py` compares the ids of a frame; here the state blob of `vnext_amd/csrc/tracker.hip` is decoded
(`DeviceTracker.tracklets()`) and compared, frame by frame, with the host-side `IDOL_Tracker` (copies: bit-equal) and
with a float64 restatement of `update_memo` / `_memo` (`_Shadow`: the momentum embedding and the matched-against
embedding, within a derived bound).  The videos are `_crowded_video` of tests/test_tracker.py with the embeddings scaled
by sqrt(8 / (9 C)), which puts a track's self-dot near 8: there the host tracker decides the same in fp32 and in
float64 (`test_host_decisions_do_not_depend_on_fp32_rounding`), so an id that differs is a fault and not a rounding.
"""
import ctypes
import functools
import math

import numpy as np
import pytest
import torch

from test_tracker import ARGS, _crowded_video, _torch_scores
from vnext_amd.models import tracker as trk

U = 2.0 ** -24          # unit roundoff of fp32
TOL_UNITS = 64          # atol = 64 u S, S = max |embedding| of the video (derivation: _check_state)


# ---------------------------------------------------------------------------------------------------
# layout (no GPU)

@pytest.mark.parametrize("capacity,channels,memory_len", [
    (1, 4, 1), (1, 68, 16), (100, 4, 16), (100, 68, 1), (100, 32, 3), (2048, 4, 1), (2048, 68, 16), (2048, 256, 3),
    (64, 256, 3), (1024, 256, 10), (7, 12, 5)])
def test_state_layout_equals_the_librarys_size(hip_lib, capacity, channels, memory_len):
    """`state_layout` (what `DeviceTracker.tracklets()` decodes with) against `trk_views` of tracker.hip."""
    from vnext_amd import _lib
    cfg = _lib.TrackerConfig(capacity=capacity, channels=channels, memory_len=memory_len, memo_tracklet_frames=10,
                             match_metric=0, long_match=1, frame_weight=1, temporal_weight=1, nms_thr_pre=0.5,
                             nms_thr_post=0.05, init_score_thr=0.2, addnew_score_thr=0.2, match_score_thr=0.5,
                             memo_momentum=0.8)
    layout, total = trk.state_layout(capacity, channels, memory_len)
    assert total == hip_lib.vnx_tracker_state_bytes(ctypes.addressof(cfg)) > 0
    # the order of trk_views, every array on a 16-byte boundary, nothing overlapping
    assert list(layout) == ["hdr", "slot_id", "last_frame", "exist", "label", "long_len", "embed", "memo", "long_embed",
                            "long_score"]
    end = 0
    for name, (offset, dtype, shape) in layout.items():
        assert offset % 16 == 0 and offset >= end and np.dtype(dtype).itemsize == 4, name
        end = offset + 4 * int(np.prod(shape))
    assert layout["hdr"][0] == 0 and layout["slot_id"][0] == 64 and total - end < 16
    assert layout["long_embed"][2] == (capacity, memory_len, channels) and layout["long_score"][2] == (capacity, memory_len)


# ---------------------------------------------------------------------------------------------------
# the float64 bank

class _Shadow(object):
    """`update_memo` and `_memo` of vnext_amd/models/tracker.py in numpy float64, driven by the ids of a frame."""

    def __init__(self, memo_momentum, memory_len, memo_tracklet_frames, long_match, temporal_weight, **_):
        self.m, self.memory_len, self.frames = float(memo_momentum), int(memory_len), int(memo_tracklet_frames)
        self.long_match, self.temporal_weight = bool(long_match), bool(temporal_weight)
        self.t = {}

    def update(self, ids, scores, embeds, labels, frame_id, unplaced=()):
        for i, k in enumerate(int(x) for x in ids):
            if k < 0 or k in unplaced:
                continue
            e = embeds[i].astype(np.float64)
            if k in self.t:
                v = self.t[k]
                v["embed"] = (1.0 - self.m) * v["embed"] + self.m * e
                v["long_embed"] = (v["long_embed"] + [e])[-self.memory_len:]
                v["long_score"] = (v["long_score"] + [float(scores[i])])[-self.memory_len:]
                v["exist_frame"] += 1
            else:
                v = self.t[k] = dict(embed=e, long_embed=[e], long_score=[float(scores[i])], exist_frame=1)
            v["label"], v["last_frame"] = int(labels[i]), frame_id
        for k in [k for k, v in self.t.items() if frame_id - v["last_frame"] >= self.frames]:
            del self.t[k]

    def memo(self, k):
        v = self.t[k]
        if not self.long_match:
            return v["embed"]
        w = np.array(v["long_score"], dtype=np.float64)
        if self.temporal_weight:
            w = w + np.arange(1, len(w) + 1, dtype=np.float64) / len(w)
        return (w[:, None] * np.stack(v["long_embed"])).sum(0) / w.sum()


class _CappedHost(trk.IDOL_Tracker):
    """IDOL_Tracker with the device tracker's one extra rule: a new tracklet that finds none of `capacity` slots
    free at the start of the frame keeps its id but is not remembered (`counters()[1]` counts them)."""

    def __init__(self, capacity, **kw):
        super().__init__(**kw)
        self.capacity, self.unplaced, self.last_unplaced = capacity, 0, ()

    def update_memo(self, ids, scores, embeds, labels, frame_id):
        free = self.capacity - len(self.tracklets)
        new = [int(k) for k in ids if k > -1 and int(k) not in self.tracklets]
        super().update_memo(ids, scores, embeds, labels, frame_id)
        self.last_unplaced = tuple(new[max(free, 0):])
        self.unplaced += len(self.last_unplaced)
        for k in self.last_unplaced:
            self.tracklets.pop(k, None)


# ---------------------------------------------------------------------------------------------------
# videos and scenarios

EMPTY_AT = 7


@functools.lru_cache(maxsize=None)
def _video(seed, objects, frames, C, h, w, clutter):
    """`_crowded_video` with a track's self-dot near 8 and one empty frame; built once, shared, never written to."""
    scale = math.sqrt(8.0 / (9.0 * C))
    video = [(b, l, m, e * scale) for b, l, m, e in _crowded_video(seed, frames=frames, objects=objects, C=C, h=h, w=w,
                                                                   clutter=clutter)]
    video[EMPTY_AT] = (torch.zeros(0, 5), torch.zeros(0, dtype=torch.long), torch.zeros(0, 1, h, w), torch.zeros(0, C))
    return tuple(video)


V150 = dict(objects=150, frames=24, C=32, h=32, w=48, clutter=6)
# name -> video, tracker options on top of ARGS, capacity, frame_id = step * t, and what the row exists for:
# `most`: detections in the largest frame must exceed it; `shift`: some tracklet outlives memory_len;
# `reuse`: more tracklets than slots; `continues`: at least half of the assigned ids continue a track.  Three rows
# cannot meet the last one, whatever the tracker does: one slot remembers one tracklet of a hundred, a tracklet
# that expires in the frame that made it is never continued, and 150 identities do not separate in 4 channels
# (the host tracker continues about a fifth of them there); these assert `continued > 0`, or == 0 for the expiry.
SCENARIOS = {
    "model_setting_nw3": dict(video=V150, most=128, shift=True),
    "model_width_nw6": dict(video=dict(objects=400, frames=20, C=256, h=40, w=64, clutter=20), most=320, shift=True),
    "memory16_channels68": dict(video=dict(V150, frames=32, C=68), opts=dict(memory_len=16, memo_momentum=0.5), shift=True),
    "memory1_channels4": dict(video=dict(V150, C=4), opts=dict(memory_len=1), shift=True, continues=False),
    "capacity100_reuse": dict(video=dict(objects=40, frames=30, C=32, h=24, w=40, clutter=6),
                              opts=dict(memo_tracklet_frames=3), capacity=100, most=30, reuse=True, shift=True),
    "capacity2048": dict(video=V150, capacity=2048, shift=True),
    "capacity1": dict(video=V150, capacity=1, continues=False),
    "short_match_momentum0": dict(video=V150, opts=dict(long_match=False, memo_momentum=0.0)),
    "short_match_momentum1": dict(video=V150, opts=dict(long_match=False, memo_momentum=1.0)),
    "expire_at_once": dict(video=V150, opts=dict(memo_tracklet_frames=0), continues=False),
    "expire_after_one": dict(video=V150, opts=dict(memo_tracklet_frames=1), shift=True),
    "frame_id_gaps": dict(video=V150, opts=dict(memo_tracklet_frames=4), step=3, shift=True),
    "softmax": dict(video=V150, opts=dict(long_match=False, frame_weight=True, temporal_weight=False, memory_len=4,
                                          match_metric="softmax", match_score_thr=0.6)),
    "cosine": dict(video=V150, opts=dict(long_match=True, frame_weight=True, temporal_weight=True, memory_len=5,
                                         match_metric="cosine", match_score_thr=0.7), shift=True),
}
SEEDS = (1, 2)
BOUNDARY_N = (63, 64, 65, 128, 129, 512)


@functools.lru_cache(maxsize=None)
def _boundary_frames(n, C=64):
    """Two frames of exactly n detections on 16 x 32 masks.  Detection i owns the pixels [i b, (i + 1) b), b = 3 (1 for
    n = 512); exact duplicates of an earlier block (removed by the NMS, -3), one-pixel overlaps with a low score
    (duplicates, -2), low scores on a block of their own (back-drops, -1), all on both sides of the 64-detection words.
    The second frame shows the identities in reverse order, so every continued tracklet is matched from another
    word, and adds new tracklets.  Self-dots near 16: with up to 512 tracklets the bi-softmax still decides by far."""
    g = torch.Generator().manual_seed(1000 + n)
    pixels, b = 16 * 32, (3 if 3 * n <= 16 * 32 else 1)
    dup = {i for i in (5, 63, 64, n - 1) if i < n}
    overlap = {i for i in (9, 70, n - 6) if i < n} if b == 3 else set()
    low = {i for i in (12, 66, n - 5) if i < n}
    fresh = {i for i in (20, 65, n - 7) if i < n}
    assert not (dup & overlap or dup & low or overlap & low or fresh & (dup | overlap | low))
    ident = math.sqrt(16.0 / C) * torch.randn(n, C, generator=g)
    masks = torch.full((n, pixels), -3.0)
    for i in range(n):
        if i in dup:
            masks[i, (i - 3) * b:(i - 2) * b] = 3.0
        elif i in overlap:
            masks[i, (i - 2) * b] = 3.0
        else:
            masks[i, i * b:(i + 1) * b] = 3.0
    scores = torch.linspace(0.95, 0.30, n)
    scores[sorted(overlap | low)] = 0.1
    frames = []
    for t in range(2):
        if t == 0:
            embeds = ident.clone()
        else:
            embeds = ident.flip(0) + 0.02 * torch.randn(n, C, generator=g)
            for i in sorted(fresh | overlap | low):
                embeds[i] = math.sqrt(16.0 / C) * torch.randn(C, generator=g)
        frames.append((torch.cat([torch.rand(n, 4, generator=g), scores[:, None]], 1), torch.arange(n) % 5,
                       masks.reshape(n, 1, 16, 32).clone(), embeds))
    return tuple(frames), (len(dup), len(overlap), len(low))


def _tie_frames(C=32):
    """A and B are made together (slots 0 and 1), A expires, C takes A's slot with a higher id than B; every
    embedding of B and C is the same e, bit for bit, so the last frame's detection scores B and C equally."""
    g = torch.Generator().manual_seed(7)
    e = torch.randn(C, generator=g)
    e = e * math.sqrt(8.0) / e.norm()
    a = torch.randn(C, generator=g)
    a = a - (a @ e) / (e @ e) * e
    a = a * math.sqrt(8.0) / a.norm()

    def frame(embeds, scores):
        n = len(embeds)
        masks = torch.full((n, 1, 8, 16), -3.0)
        for i in range(n):
            masks[i, 0, i, 0:4] = 3.0
        return (torch.cat([torch.rand(n, 4, generator=g), torch.tensor(scores)[:, None]], 1),
                torch.zeros(n, dtype=torch.long), masks, torch.stack(embeds))
    return (frame([a, e], [0.9, 0.8]), frame([e], [0.9]), frame([e], [0.9]), frame([e, e], [0.9, 0.8]),
            frame([e], [0.9]))


TIE_OPTS = dict(long_match=False, frame_weight=False, temporal_weight=False, memo_momentum=0.5, memo_tracklet_frames=2)


def _cases():
    """every (name, video, args, capacity, step) the GPU tests run: the decision-stability test covers them all"""
    for name, sc in SCENARIOS.items():
        for seed in SEEDS:
            yield (f"{name}-seed{seed}", _video(seed, **sc["video"]), dict(ARGS, **sc.get("opts", {})),
                   sc.get("capacity", 1024), sc.get("step", 1))
    for n in BOUNDARY_N:
        yield f"boundary-{n}", _boundary_frames(n)[0], dict(ARGS), 1024, 1
    yield "tie", _tie_frames(), dict(ARGS, **TIE_OPTS), 8, 1


def _host(args, capacity):
    return _CappedHost(capacity, **args) if capacity == 1 else trk.IDOL_Tracker(**args)


# ---------------------------------------------------------------------------------------------------
# the premise: on these videos the host tracker's decisions have margins that fp32 rounding does not reach

def test_host_decisions_do_not_depend_on_fp32_rounding(monkeypatch):
    """The host tracker on the CPU, association scores in fp32 and in float64: zero differing ids, for every scenario and
    seed below.  (The saturated video of tests/test_tracker.py fails this by hundreds of ids and is not used here.)"""
    monkeypatch.setattr(trk, "_pairwise_dot", lambda a, b: a @ b.t())
    differing = {}
    for name, video, args, capacity, step in _cases():
        runs = []
        for double in (False, True):
            monkeypatch.setattr(trk, "_match_scores", (lambda e, m, metric: _torch_scores(e.double(), m.double(), metric))
                                if double else _torch_scores)
            host = _host(args, capacity)
            runs.append([host.match(b, l, m, e, step * t, list(range(b.shape[0])))[2].numpy()
                         for t, (b, l, m, e) in enumerate(video)])
        diff = sum(int(np.sum(x != y)) if x.shape == y.shape else max(len(x), len(y)) for x, y in zip(*runs))
        if diff:
            differing[name] = diff
    assert not differing


# ---------------------------------------------------------------------------------------------------
# the differential

def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.int32)


def _check_state(dev, host, shadow, S, tag, worst):
    """The device bank against the host's (structure and copies: equal) and the float64 shadow (embed, memo: atol).

    Every stored value is a convex combination of input embeddings, so |x| <= S.  `memo` is a weighted mean of at most
    memory_len rows: the weights (1 add each), their sum (memory_len adds), the products and the accumulation
    (2 memory_len), one division: at most 2 memory_len + 4 = 36 roundings, each of relative size u on values bounded
    by S.  `embed` is a recurrence x <- (1 - m) x + m e with at most 4 u S fresh error per step (two products, one sum,
    1 - m rounded to fp32), of which a fraction (1 - m) survives each step: it settles at 4 u S / m = 8 u S for
    m >= 0.5, and m = 0 copies.  64 u S covers both."""
    got = dev.tracklets()
    assert set(got) == set(host.tracklets) == set(shadow.t), tag
    if not got:
        return
    keys = list(host.tracklets)
    h_embed = torch.stack([host.tracklets[k]["embed"] for k in keys]).cpu().numpy()
    h_memo = host._memo(None)[0].cpu().numpy()
    h_long = torch.cat([torch.stack(host.tracklets[k]["long_embed"]) for k in keys]).cpu().numpy()
    atol, at = TOL_UNITS * U * S, 0
    for r, k in enumerate(keys):
        d, h, s = got[k], host.tracklets[k], shadow.t[k]
        n = len(h["long_score"])
        where = f"{tag} tracklet {k} (slot {d['slot']})"
        assert (d["exist_frame"], d["label"], d["last_frame"], len(d["long_score"]), len(d["long_embed"])) == \
            (h["exist_frame"], h["label"], h["last_frame"], n, len(h["long_embed"])), where
        assert (s["exist_frame"], s["label"], s["last_frame"], len(s["long_score"])) == \
            (h["exist_frame"], h["label"], h["last_frame"], n), where
        np.testing.assert_array_equal(_bits(d["long_score"]), _bits(h["long_score"]), err_msg=where)
        np.testing.assert_array_equal(_bits(d["long_embed"]), _bits(h_long[at:at + n]), err_msg=where)
        np.testing.assert_array_equal(d["long_embed"].astype(np.float64), np.stack(s["long_embed"]), err_msg=where)
        at += n
        for what, dv, hv, want in (("embed", d["embed"], h_embed[r], s["embed"]), ("memo", d["memo"], h_memo[r], shadow.memo(k))):
            e_dev, e_host = float(np.abs(dv - want).max()), float(np.abs(hv - want).max())
            worst["dev_" + what] = max(worst.get("dev_" + what, 0.0), e_dev / (U * S))
            worst["host_" + what] = max(worst.get("host_" + what, 0.0), e_host / (U * S))
            assert e_host <= atol, f"{where}: host {what} off by {e_host / (U * S):.1f} u S: the bound is wrong for the reference"
            assert e_dev <= atol, f"{where}: device {what} off by {e_dev / (U * S):.1f} u S (host {e_host / (U * S):.1f})"


def _run_pair(tag, video, args, capacity, step=1):
    """Host and device tracker side by side on the GPU, the shadow on the host; everything asserted after every frame."""
    host, dev, shadow = _host(args, capacity), trk.DeviceTracker(capacity=capacity, **args), _Shadow(**args)
    S = max(float(e.abs().max()) for _, _, _, e in video if e.numel())
    stats = dict(most=0, assigned=0, continued=0, longest=0, frames=0, worst={}, ids=[])
    for t, (bboxes, labels, masks, embeds) in enumerate(video):
        b, l, m, e = (x.to("cuda:0") for x in (bboxes, labels, masks, embeds))
        n, where = b.shape[0], f"{tag} frame {t}"
        before = set(host.tracklets)
        _, _, ids_h, kept_h = host.match(b, l, m, e, step * t, list(range(n)))
        ids_d = dev.match_device(b, l, m, e, step * t).cpu().numpy()
        kept = np.array(kept_h, dtype=np.int64)
        want = np.full(n, -3, dtype=np.int64)
        want[kept] = ids_h.numpy()
        np.testing.assert_array_equal(ids_d, want, err_msg=where)
        stats["ids"].append(want)
        if n:
            shadow.update(ids_h.numpy(), bboxes[kept, 4].numpy(), embeds[kept].numpy(), labels[kept].numpy(), step * t,
                          unplaced=getattr(host, "last_unplaced", ()))
        _check_state(dev, host, shadow, S, where, stats["worst"])
        stats["most"] = max(stats["most"], n)
        stats["frames"] += n > 0
        stats["assigned"] += int((ids_h >= 0).sum())
        stats["continued"] += sum(1 for k in ids_h.tolist() if k in before)
        stats["longest"] = max([stats["longest"]] + [v["exist_frame"] for v in host.tracklets.values()])
    created, unplaced, frames = dev.counters()
    assert (created, unplaced, frames) == (host.num_tracklets, getattr(host, "unplaced", 0), stats["frames"]), tag
    stats.update(created=created, unplaced=unplaced, host=host, dev=dev)
    print(f"[tracker state] {tag}: most {stats['most']} created {created} unplaced {unplaced} continued "
          f"{stats['continued']}/{stats['assigned']} longest {stats['longest']} worst/(u S) "
          + " ".join(f"{k} {v:.2f}" for k, v in sorted(stats["worst"].items())))
    return stats


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(SCENARIOS))
def test_device_bank_equals_the_host_bank_after_every_frame(name):
    """Ids, live set, counters, remembered scores and rows (bit-equal), embed and memo (64 u S of float64), per frame.

    The one-slot row runs against `_CappedHost`, which states the device's rule for a full bank, so ids, state and
    counters are compared on every frame there too, not only while nothing was left unplaced.

    Largest errors seen on an MI355X, in units of u S (bound: 64), over all rows, seeds and the hand-built cases:
    device embed 1.33, device memo 2.54 (memory_len 16); host embed 1.71, host memo 3.27 (memory_len 16).  Both sit a
    factor of twenty under the bound, which is a worst case over 36 roundings; a wrong weight, row or momentum moves a
    value by a fraction of S, 2^20 units, so the bound separates them with room on either side."""
    sc = SCENARIOS[name]
    args, capacity = dict(ARGS, **sc.get("opts", {})), sc.get("capacity", 1024)
    for seed in SEEDS:
        video = _video(seed, **sc["video"])
        st = _run_pair(f"{name} seed {seed}", video, args, capacity, sc.get("step", 1))
        assert st["frames"] == len(video) - 1                       # the empty frame is a no-op
        assert st["most"] > sc.get("most", 64)
        if capacity > 1:
            assert st["unplaced"] == 0
        else:
            assert st["unplaced"] > 0 and len(st["dev"].tracklets()) <= 1
        if sc.get("shift"):
            assert st["longest"] > args["memory_len"]                # the append dropped an oldest entry
        if sc.get("reuse"):
            assert st["created"] > capacity
        if sc.get("continues", True):
            assert 2 * st["continued"] >= st["assigned"] > 0
        else:
            assert (st["continued"] > 0) == (args["memo_tracklet_frames"] > 0) and st["assigned"] > 0


@pytest.mark.gpu
@pytest.mark.parametrize("n", BOUNDARY_N)
def test_frames_at_the_word_boundaries(n):
    """Exactly n detections: the last-word mask of the NMS, the ballot rounds that number new tracklets, the strided
    loops; one creating frame and one matching frame whose partners sit in other 64-detection words."""
    frames, (dups, overlaps, lows) = _boundary_frames(n)
    st = _run_pair(f"boundary {n}", frames, dict(ARGS), 1024)
    first = st["ids"][0]
    made = n - dups - overlaps - lows
    assert (int((first == -3).sum()), int((first == -2).sum()), int((first == -1).sum())) == (dups, overlaps, lows)
    assert int((first >= 0).sum()) == made and first.max() == made - 1
    assert st["most"] == n and st["unplaced"] == 0
    # frame 1: a position continues a track unless it or its partner n - 1 - i was special, or it shows a new object
    assert st["continued"] >= n - 2 * (dups + overlaps + lows) - 3 and st["created"] > made


@pytest.mark.gpu
def test_a_tie_goes_to_the_older_tracklet_not_the_lower_slot():
    frames = _tie_frames()
    st = _run_pair("tie", frames, dict(ARGS, **TIE_OPTS), 8)
    got = st["dev"].tracklets()
    assert set(got) == {1, 2} and got[2]["slot"] == 0 and got[1]["slot"] == 1       # C sits below B: the case is not vacuous
    e = frames[1][3][0].numpy()
    assert np.array_equal(_bits(got[1]["embed"]), _bits(e)) and np.array_equal(_bits(got[2]["embed"]), _bits(e))
    assert got[1]["exist_frame"] == 5 and got[1]["last_frame"] == 4 and got[2]["exist_frame"] == 1   # B took the last frame
