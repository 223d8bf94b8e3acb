"""SeqFormer's clip matching on the device (vnext_amd/csrc/clip_link.hip, `DeviceVideos`) against the host `Videos`.

The exact-id comparisons need assignments that fp32 rounding cannot flip.  That is a condition on the INPUTS, checked on
the CPU in float64 (`margins`): for every update of every video used here, the optimum beats the best assignment that
avoids any one of its positive pairs by >= 1e-4, and every positive score is >= 1e-4 away from the 0.01 threshold."""
import ctypes
import functools
import os
import re
import types

import numpy as np
import pytest
import torch
from scipy.optimize import linear_sum_assignment

from conftest import GOLDEN_DIR, ROOT
from vnext_amd import _lib
from vnext_amd import train
from vnext_amd.models import tracker as trk
from vnext_amd.models.clip_matching import Clips, DeviceVideos, Videos
from vnext_amd.ops import clip_link
from vnext_amd.ops.clip_link import ClipLinkUnsupported

DEV = "cuda:0"
MARGIN = 1e-4


# ---- planted videos ------------------------------------------------------------------------------------------------------
def clip_frames(L, clen, stride):
    """the clips `SeqFormer.inference` cuts a video of L frames into"""
    out = []
    for start in range(0, L, stride):
        end, last = start + clen, False
        if end >= L:
            start, end, last = max(0, L - clen), L, True
        out.append(list(range(start, end)))
        if last:
            break
    return out


def planted_video(L, clen, stride, h=7, w=9, seed=0, tracks=4, K=5, show=0.8, empty=(), whole=False):
    """Background logit -8; each track a 2-3 x 2-4 rectangle of +4 that drifts one pixel per frame, alive on a random
    frame interval (`whole`: the whole video); a clip shows each live track with probability `show`, adds two one-off
    2 x 2 blobs and N(0, 0.5^2) noise, permutes its instances and draws random class probabilities.
    -> [(frames, cls [n, K], logits [n, T, h, w])] float32."""
    rng = np.random.RandomState(seed)
    tr = []
    for _ in range(tracks):
        hh, ww = rng.randint(2, 4), rng.randint(2, 5)
        y0, x0 = rng.randint(0, h - hh + 1), rng.randint(0, w - ww + 1)
        dy, dx = rng.randint(-1, 2), rng.randint(-1, 2)
        t0 = rng.randint(0, L)
        t1 = rng.randint(t0, L)
        tr.append((hh, ww, y0, x0, dy, dx, 0 if whole else t0, L - 1 if whole else t1))
    clips = []
    for c, frames in enumerate(clip_frames(L, clen, stride)):
        T, inst = len(frames), []
        for hh, ww, y0, x0, dy, dx, t0, t1 in tr:
            if any(t0 <= f <= t1 for f in frames) and rng.rand() < show:
                m = np.full((T, h, w), -8.0)
                for k, f in enumerate(frames):
                    if t0 <= f <= t1:
                        y, x = int(np.clip(y0 + dy * f, 0, h - hh)), int(np.clip(x0 + dx * f, 0, w - ww))
                        m[k, y:y + hh, x:x + ww] = 4.0
                inst.append(m)
        for _ in range(2):
            m = np.full((T, h, w), -8.0)
            y, x = rng.randint(0, h - 1), rng.randint(0, w - 1)
            m[:, y:y + 2, x:x + 2] = 4.0
            inst.append(m)
        if c in empty:
            inst = []
        n = len(inst)
        logits = (np.stack(inst) if n else np.zeros((0, T, h, w))) + rng.normal(0.0, 0.5, (n, T, h, w))
        logits = logits[rng.permutation(n)]
        clips.append((frames, rng.rand(n, K).astype(np.float32), logits.astype(np.float32)))
    return clips


# the issue's nine shape settings, a 16-instance video, K = 40, and two frames of more than one pixel chunk (1024 pixels):
# one on the 16-byte path (H * W a multiple of 4), one on the scalar path.  Seeds: the lowest that meets the margin
# condition (test_margin_condition_of_every_planted_video asserts it for each).
CASES = {
    "overlap2": dict(L=9, clen=4, stride=2, h=10, w=14, seed=0),
    "stride1": dict(L=7, clen=3, stride=1, seed=0),
    "ring_wraps": dict(L=12, clen=5, stride=1, seed=0),
    "no_shared_frame": dict(L=8, clen=2, stride=2, seed=0),
    "gaps": dict(L=10, clen=2, stride=3, seed=0),
    "short_video": dict(L=3, clen=5, stride=1, seed=0),
    "one_frame_clips": dict(L=6, clen=1, stride=1, seed=0),
    "empty_mid": dict(L=12, clen=5, stride=1, seed=0, empty=(3,)),
    "empty_first": dict(L=12, clen=5, stride=1, seed=0, empty=(0,)),
    "sixteen": dict(L=7, clen=3, stride=1, h=14, w=18, seed=0, tracks=14, show=1.0, whole=True),
    "k40": dict(L=7, clen=3, stride=1, seed=1, K=40),
    "two_chunks_vec": dict(L=5, clen=3, stride=1, h=32, w=36, seed=0),
    "two_chunks_scalar": dict(L=5, clen=3, stride=1, h=33, w=37, seed=0),
}


def _siou64(video, clip):
    """the statements of Videos.get_siou in float64, from the logits"""
    n_i = clip.num_instance
    siou, count = np.zeros((video.num_inst, n_i)), np.zeros(video.num_inst)
    in_pos = {f: k for k, f in enumerate(clip.frame_idx)}
    b_all = torch.sigmoid(clip.mask_logits.double().cpu()).flatten(2).numpy()
    for frame_idx, ids, logits, _, _ in video.clips[max(video.num_clip - len(clip.frame_idx), 0):]:
        shared = [(k, in_pos[f]) for k, f in enumerate(frame_idx) if f in in_pos]
        if not shared or len(ids) == 0:
            continue
        a_all = torch.sigmoid(logits.double().cpu()).flatten(2).numpy()
        a = a_all[:, [k for k, _ in shared]].reshape(len(ids), -1)
        b = b_all[:, [j for _, j in shared]].reshape(n_i, -1)
        inter = a @ b.T
        union = a.sum(1)[:, None] + b.sum(1)[None, :] - inter
        ids = ids.cpu().numpy()
        siou[ids] += inter / (union + 1e-6)
        count[ids] += 1
    return siou / (count[:, None] + 1e-6)


class RecordingVideos(Videos):
    """the host path, keeping per update its fp32 scores and their float64 recomputation"""

    def __init__(self, *a):
        super().__init__(*a)
        self.log, self.ids = [], []

    def get_siou(self, input_clip):
        s = super().get_siou(input_clip)
        self.log.append((s.double().cpu().numpy(), _siou64(self, input_clip)))
        return s

    def update(self, input_clip):
        super().update(input_clip)
        self.ids.append(self.clips[-1][1].cpu().tolist())


def margins(score):
    """score [tracks, n] float64 -> (gap between the optimum and the best assignment that avoids any one of its positive
    pairs, distance of the positive scores from the threshold); inf where there is nothing to compare"""
    pos = score[score > 0]
    dist = float(np.abs(pos - 0.01).min()) if pos.size else np.inf
    m = score * (score > 0.01)
    rows, cols = linear_sum_assignment(m, maximize=True)
    best, gap = m[rows, cols].sum(), np.inf
    for r, c in zip(rows, cols):
        if m[r, c] > 0:
            alt = m.copy()
            alt[r, c] = -1e6
            ar, ac = linear_sum_assignment(alt, maximize=True)
            gap = min(gap, best - alt[ar, ac].sum())
    return float(gap), dist


def _as_clip(frames, cls, logits, device):
    cls, logits = torch.as_tensor(cls).to(device), torch.as_tensor(logits).to(device)
    return Clips(frames, types.SimpleNamespace(pred_classes=cls.argmax(1) if len(cls) else cls.new_zeros(0, dtype=torch.long),
                                               scores=cls.max(1)[0] if len(cls) else cls.new_zeros(0), cls_probs=cls,
                                               pred_masks=logits))


def run_host(clips, clen, L, K, hw, device):
    video = RecordingVideos(clen, L, K, hw, device)
    for frames, cls, logits in clips:
        video.update(_as_clip(frames, cls, logits, device))
    cls, logits = video.get_result()
    return video, cls.cpu().numpy(), logits.cpu().numpy()


@functools.lru_cache(maxsize=None)
def host_reference(name):
    """the host `Videos` on the CPU (its GEMM as `a @ b.t()`, as tests/test_clip_matching.py runs it), once per video"""
    c = dict(CASES[name])
    clips = planted_video(**c)
    h, w, K = clips[0][2].shape[-2], clips[0][2].shape[-1], clips[0][1].shape[1]
    old = trk._pairwise_dot
    trk._pairwise_dot = lambda a, b: a @ b.t()
    try:
        video, cls, logits = run_host(clips, c["clen"], c["L"], K, (h, w), "cpu")
    finally:
        trk._pairwise_dot = old
    m = [margins(s64) for _, s64 in video.log]
    return dict(clips=clips, clen=c["clen"], L=c["L"], K=K, hw=(h, w), ids=video.ids, num_inst=video.num_inst, cls=cls,
                logits=logits, gap=min([g for g, _ in m], default=np.inf), dist=min([d for _, d in m], default=np.inf),
                log=video.log)


def run_device(ref, capacity=120, **kw):
    video = DeviceVideos(ref["clen"], ref["L"], ref["K"], ref["hw"], DEV, capacity=capacity, **kw)
    ids = [video.update_logits(frames, torch.as_tensor(cls).to(DEV), torch.as_tensor(logits).to(DEV))
           for frames, cls, logits in ref["clips"]]
    return video, ids


def assert_same_tracks(got_cls, got_logits, want_cls, want_logits):
    assert got_cls.shape == want_cls.shape and got_logits.shape == want_logits.shape
    np.testing.assert_allclose(got_cls, want_cls, rtol=1e-5, atol=1e-5)
    np.testing.assert_array_equal(np.isnan(got_logits), np.isnan(want_logits))
    np.testing.assert_allclose(np.nan_to_num(got_logits), np.nan_to_num(want_logits), rtol=1e-5, atol=1e-5)


# ---- CPU -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(CASES))
def test_margin_condition_of_every_planted_video(name):
    ref = host_reference(name)
    print(f"{name}: gap {ref['gap']:.3e}, distance from the threshold {ref['dist']:.3e}, {ref['num_inst']} tracks, "
          f"{len(ref['log'])} scored updates")
    assert ref["gap"] >= MARGIN and ref["dist"] >= MARGIN


def test_planted_videos_cover_what_they_are_for():
    assert max(len(c[1]) for c in host_reference("sixteen")["clips"]) == 16
    assert host_reference("k40")["K"] == 40
    assert len(host_reference("ring_wraps")["clips"]) > 5                     # more clips than ring slots
    assert len(host_reference("empty_mid")["clips"][3][1]) == 0 and len(host_reference("empty_first")["clips"][0][1]) == 0
    assert np.isnan(host_reference("gaps")["logits"]).any()
    assert not host_reference("no_shared_frame")["log"] or all(s.max() == 0 for s, _ in host_reference("no_shared_frame")["log"])
    assert len(host_reference("short_video")["clips"]) == 1 and len(host_reference("short_video")["clips"][0][0]) == 3
    assert any(len(s) for s, _ in host_reference("overlap2")["log"])          # matches happen at all


def test_device_videos_has_no_cpu_form():
    clips = planted_video(5, 3, 1)
    video = DeviceVideos(3, 5, 5, (7, 9), "cpu")
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        video.update_logits(clips[0][0], torch.as_tensor(clips[0][1]), torch.as_tensor(clips[0][2]))
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        video.update(_as_clip(*clips[0], "cpu"))
    with pytest.raises(RuntimeError, match="Not implemented on the CPU.*Videos"):
        clip_link.new_state(clip_link.config(3, 16, 63, 5, 5, 120), "cpu")


def test_switch_is_off_by_default_and_only_seqformer_has_it():
    import vnext_amd.models  # noqa: F401
    from vnext_amd.registry import build_model, get_idol_cfg, get_seqformer_cfg
    tiny = {"ENC_LAYERS": 1, "DEC_LAYERS": 1, "NUM_OBJECT_QUERIES": 4, "DIM_FEEDFORWARD": 32}
    model = build_model(get_seqformer_cfg(**{"MODEL.DEVICE": "cpu", **{f"MODEL.SeqFormer.{k}": v for k, v in tiny.items()}}))
    assert model.device_clip_matching is False
    train.enable_device_clip_matching(model)
    assert model.device_clip_matching is True
    train.enable_device_clip_matching(model, False)
    assert model.device_clip_matching is False
    idol = build_model(get_idol_cfg(**{"MODEL.DEVICE": "cpu", **{f"MODEL.IDOL.{k}": v for k, v in tiny.items()}}))
    with pytest.raises(ValueError, match="device_clip_matching"):
        train.enable_device_clip_matching(idol)


def test_new_symbols_are_declared_and_the_abi_version_stays():
    text = open(os.path.join(ROOT, "include", "vnext_hip.h")).read()
    for name in ("vnx_clip_link_state_bytes", "vnx_clip_link_workspace_bytes", "vnx_clip_link_reset", "vnx_clip_link_update",
                 "vnx_clip_link_result"):
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in _lib.SIGNATURES
    assert "vnx_debug_clip_link_score_layout" in _lib.DEBUG_SIGNATURES
    assert "vnx_debug_clip_link_score_layout" in open(os.path.join(ROOT, "include", "vnext_hip_debug.h")).read()
    assert _lib.ABI_VERSION == 17 and re.search(r"#define VNX_ABI_VERSION 17\b", text)
    assert ctypes.sizeof(_lib.ClipLinkConfig) == 24 and ctypes.sizeof(_lib.ClipLinkPlan) == 4 * 27 + 128
    assert (clip_link.MAX_INSTANCES, clip_link.MAX_FRAMES) == (16, 8)


def test_plan_lists_the_shared_frames_oldest_first():
    p = clip_link.plan([4, 5, 6], 2, [(0, [2, 3, 4]), (1, [0, 1]), (3, [5, 6, 7])])
    assert (p.frames, p.write_slot, p.slots) == (3, 2, 2) and list(p.frame_index)[:3] == [4, 5, 6]
    assert (p.slot[0], p.pairs[0], p.stored_pos[0][0], p.incoming_pos[0][0]) == (0, 1, 2, 0)
    assert (p.slot[1], p.pairs[1]) == (3, 2)
    assert [(p.stored_pos[1][i], p.incoming_pos[1][i]) for i in range(2)] == [(0, 1), (1, 2)]
    assert clip_link.plan(list(range(9)), 0, []).frames == 9                  # too long: the call refuses it by its length


# ---- GPU -------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("v", [0, 1])
def test_reference_fixture_through_device_videos(v):
    g = dict(np.load(os.path.join(GOLDEN_DIR, "clip_matching.npz")))
    n_clips, L, clen, K, h, w = (int(x) for x in g[f"v{v}.cfg"])
    video = DeviceVideos(clen, L, K, (h, w), DEV)
    for c in range(n_clips):
        cls = torch.from_numpy(g[f"v{v}.c{c}.cls"]).to(DEV)
        logits = torch.from_numpy(g[f"v{v}.c{c}.logits"]).to(DEV)
        res = types.SimpleNamespace(pred_classes=cls.argmax(1), scores=cls.max(1)[0], cls_probs=cls, pred_masks=logits)
        video.update(Clips(g[f"v{v}.c{c}.frames"].tolist(), res))
    out_cls, out_logits = video.get_result()
    np.testing.assert_allclose(out_cls.cpu().numpy(), g[f"v{v}.out_cls"], rtol=1e-5, atol=1e-6)
    want, got = g[f"v{v}.out_logits"], out_logits.cpu().numpy()
    assert got.shape == want.shape
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want))
    np.testing.assert_allclose(np.nan_to_num(got), np.nan_to_num(want), rtol=1e-5, atol=1e-5)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_same_tracks_as_the_host_videos(name):
    ref = host_reference(name)
    assert ref["gap"] >= MARGIN and ref["dist"] >= MARGIN
    video, ids = run_device(ref)
    assert [i.cpu().tolist() for i in ids] == ref["ids"]
    assert video.counters() == (ref["num_inst"], 0, len(ref["clips"]))
    cls, logits = video.get_result()
    assert_same_tracks(cls.cpu().numpy(), logits.cpu().numpy(), ref["cls"], ref["logits"])


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["overlap2", "ring_wraps", "sixteen", "two_chunks_scalar"])
def test_scores_against_float64(name):
    """the score matrix launch 2 matched on (vnx_debug_clip_link_score_layout) against the float64 recomputation: its
    error is at most max(2 x the host path's fp32 error on the same inputs, 1e-6).  The host path here is `Videos` on the
    GPU, its product on the similarity kernel."""
    ref = host_reference(name)
    host, _, _ = run_host(ref["clips"], ref["clen"], ref["L"], ref["K"], ref["hw"], DEV)
    assert host.ids == ref["ids"]
    video = DeviceVideos(ref["clen"], ref["L"], ref["K"], ref["hw"], DEV)
    log, scored = iter(host.log), 0
    num_inst = 0
    for (frames, cls, logits), ids in zip(ref["clips"], ref["ids"]):
        video.update_logits(frames, torch.as_tensor(cls).to(DEV), torch.as_tensor(logits).to(DEV))
        if num_inst and len(ids):
            s32, s64 = next(log)
            tracks, got = clip_link.debug_scores(video.workspace, len(ids))
            tracks, got = tracks.cpu().numpy(), got.double().cpu().numpy()
            err_host = float(np.abs(s32 - s64).max())
            err = float(np.abs(got - s64[tracks]).max()) if len(tracks) else 0.0
            rest = np.delete(s64, tracks, axis=0)
            print(f"{name} clip {frames}: {len(tracks)} rows of {s64.shape[0]} tracks, device error {err:.3e}, host error "
                  f"{err_host:.3e}, bound {max(2 * err_host, 1e-6):.3e}")
            assert len(set(tracks.tolist())) == len(tracks)
            assert rest.size == 0 or rest.max() == 0                          # the rows left out are the all-zero ones
            assert err <= max(2 * err_host, 1e-6)
            scored += 1
        num_inst = max([num_inst] + [i + 1 for i in ids])
    assert scored > 0


@pytest.mark.gpu
def test_bit_identical_run_to_run():
    ref = host_reference("ring_wraps")
    runs = []
    for _ in range(2):
        video, ids = run_device(ref)
        runs.append((torch.cat(ids), *video.get_result()))
    for a, b in zip(*runs):
        assert torch.equal(torch.nan_to_num(a, nan=12345.0), torch.nan_to_num(b, nan=12345.0))
        assert torch.equal(torch.isnan(a), torch.isnan(b))


@pytest.mark.gpu
def test_guard_words_around_the_outputs():
    """ids_out and both result tensors sit between guard words and start from a sentinel / NaN: an element nobody wrote,
    or a write outside, shows."""
    ref = host_reference("gaps")                                              # has frames no clip covers: real NaNs
    G = 64
    video = DeviceVideos(ref["clen"], ref["L"], ref["K"], ref["hw"], DEV)
    for (frames, cls, logits), want in zip(ref["clips"], ref["ids"]):
        buf = torch.full((len(want) + 2 * G,), -777, dtype=torch.int64, device=DEV)
        ids = video.update_logits(frames, torch.as_tensor(cls).to(DEV), torch.as_tensor(logits).to(DEV),
                                  ids_out=buf[G:G + len(want)])
        assert ids.cpu().tolist() == want
        assert bool((buf[:G] == -777).all()) and bool((buf[G + len(want):] == -777).all())
    N, L, K, hw = ref["num_inst"], ref["L"], ref["K"], ref["hw"][0] * ref["hw"][1]
    SENT = 3.0e38
    cbuf = torch.full((N * K + 2 * G,), SENT, device=DEV)
    lbuf = torch.full((N * L * hw + 2 * G,), SENT, device=DEV)
    cls, logits = video.get_result(cls_out=cbuf[G:G + N * K].view(N, K), logits_out=lbuf[G:G + N * L * hw].view(N, L, hw))
    for buf, n in ((cbuf, N * K), (lbuf, N * L * hw)):
        assert bool((buf[:G] == SENT).all()) and bool((buf[G + n:] == SENT).all())
        assert not bool((buf[G:G + n] == SENT).any())
    assert_same_tracks(cls.cpu().numpy(), logits.cpu().numpy(), ref["cls"], ref["logits"])


@pytest.mark.gpu
def test_limits_refuse_before_any_launch():
    ref = host_reference("ring_wraps")
    video, _ = run_device(dict(ref, clips=ref["clips"][:2]))
    torch.cuda.synchronize()
    before, clips_before = video.state.clone(), video.num_clip
    h, w = ref["hw"]
    with pytest.raises(ClipLinkUnsupported, match="17 instances"):
        video.update_logits([2, 3, 4, 5, 6], torch.rand(17, ref["K"], device=DEV), torch.randn(17, 5, h, w, device=DEV))
    with pytest.raises(ClipLinkUnsupported, match="9 frames"):
        video.update_logits(list(range(2, 11)), torch.rand(3, ref["K"], device=DEV), torch.randn(3, 9, h, w, device=DEV))
    torch.cuda.synchronize()
    assert torch.equal(video.state, before) and video.num_clip == clips_before
    with pytest.raises(ClipLinkUnsupported, match="up to 8 frames"):         # a ring of 9 clips
        DeviceVideos(9, 12, ref["K"], ref["hw"], DEV).update_logits(
            list(range(9)), torch.rand(3, ref["K"], device=DEV), torch.randn(3, 9, h, w, device=DEV))
    # the state goes on as if nothing had been asked
    ids = [video.update_logits(f, torch.as_tensor(c).to(DEV), torch.as_tensor(l).to(DEV)) for f, c, l in ref["clips"][2:]]
    assert [i.cpu().tolist() for i in ids] == ref["ids"][2:]


@pytest.mark.gpu
def test_overflow_is_counted_and_refused_at_the_result():
    ref = host_reference("ring_wraps")
    assert ref["num_inst"] > 4
    video, ids = run_device(ref, capacity=4)
    opened, lost, clips = video.counters()
    assert opened == 4 and lost > 0 and clips == len(ref["clips"])
    flat = torch.cat(ids).cpu()
    assert int((flat == -1).sum()) == lost and int(flat.max()) == 3
    with pytest.raises(ClipLinkUnsupported, match="no free track"):
        video.get_result()


@pytest.mark.gpu
def test_update_loop_does_not_synchronise():
    """torch's sync-debug mode in its "error" setting (this build honours it on ROCm: the host path raises under it)"""
    ref = host_reference("ring_wraps")
    dev_clips = [(f, torch.as_tensor(c).to(DEV), torch.as_tensor(l).to(DEV)) for f, c, l in ref["clips"]]
    DeviceVideos(ref["clen"], ref["L"], ref["K"], ref["hw"], DEV).update_logits(*dev_clips[0])      # warm-up: loads the library
    video = DeviceVideos(ref["clen"], ref["L"], ref["K"], ref["hw"], DEV)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        ids = [video.update_logits(*c) for c in dev_clips]
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert [i.cpu().tolist() for i in ids] == ref["ids"]
    host = Videos(ref["clen"], ref["L"], ref["K"], ref["hw"], DEV)
    host.update(_as_clip(*ref["clips"][0], DEV))
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):
            host.update(_as_clip(*ref["clips"][1], DEV))
    finally:
        torch.cuda.set_sync_debug_mode("default")


SEQ_TINY = {"MODEL.SeqFormer.ENC_LAYERS": 1, "MODEL.SeqFormer.DEC_LAYERS": 2, "MODEL.SeqFormer.NUM_OBJECT_QUERIES": 12,
            "MODEL.SeqFormer.DIM_FEEDFORWARD": 64, "MODEL.SeqFormer.DROPOUT": 0.0}
MODEL_SEED = 6      # gap 1.4e-3 on its two scored updates; seeds 0 - 9 all meet the condition (1.6e-4 at the least, seed 9)


def _tiny_model_and_video(monkeypatch):
    """a tiny SeqFormer with CLIP_MATCHING over 7 frames at 96 x 160 (tests/test_model_ddp.py's size), clips of 3 frames
    every 2.  The clip trunk's kernels are not bitwise deterministic between calls, so its outputs are kept per clip and
    replayed: both paths link the very same logits."""
    import vnext_amd.models  # noqa: F401
    from vnext_amd.registry import build_model, get_seqformer_cfg
    torch.manual_seed(MODEL_SEED)
    cfg = get_seqformer_cfg(**{"MODEL.DEVICE": DEV, "MODEL.SeqFormer.CLIP_MATCHING": True, "MODEL.SeqFormer.CLIP_LENGTH": 3,
                               "MODEL.SeqFormer.CLIP_STRIDE": 2, "MODEL.SeqFormer.APPLY_CLS_THRES": 0.0, **SEQ_TINY})
    model = build_model(cfg).eval()
    g = torch.Generator().manual_seed(2)
    video = [{"video_id": 7, "image": [(torch.rand(3, 96, 160, generator=g) * 255).to(DEV) for _ in range(7)],
              "height": 100, "width": 170, "length": 7}]
    kept, real = {}, model._top_instances

    def top_instances(frames):
        key = tuple(f.data_ptr() for f in frames)
        if key not in kept:
            kept[key] = tuple(t.clone() for t in real(frames))
        return kept[key]
    monkeypatch.setattr(model, "_top_instances", top_instances)
    return model, video


def _count_calls(monkeypatch, cls, name):
    calls, real = [], getattr(cls, name)

    def counted(self, *a, **k):
        calls.append(1)
        return real(self, *a, **k)
    monkeypatch.setattr(cls, name, counted)
    return calls


@pytest.mark.gpu
def test_model_gives_the_same_video_with_the_switch_on(monkeypatch):
    model, video = _tiny_model_and_video(monkeypatch)
    # `inference` moves the frames to the device itself: hand it device frames so the replay key (their addresses) holds
    scores = []
    real_siou = Videos.get_siou

    def recording_siou(self, clip):
        s = real_siou(self, clip)
        scores.append(s.double().cpu().numpy())
        return s
    monkeypatch.setattr(Videos, "get_siou", recording_siou)
    device_calls = _count_calls(monkeypatch, DeviceVideos, "update_logits")
    host_calls = _count_calls(monkeypatch, Videos, "update")
    off = model(video)
    off_records = model.ytvis_results(video)
    assert len(host_calls) == 6 and not device_calls
    # the margin condition on the host path's own score matrices (seed MODEL_SEED)
    for s in scores:
        gap, dist = margins(s)
        print(f"model: scores {s.shape}, gap {gap:.3e}, distance from the threshold {dist:.3e}")
        assert gap >= MARGIN and dist >= MARGIN
    train.enable_device_clip_matching(model)
    capacities, real_start = [], DeviceVideos._start

    def recording_start(self):
        capacities.append(self.capacity)
        return real_start(self)
    monkeypatch.setattr(DeviceVideos, "_start", recording_start)
    on = model(video)
    on_records = model.ytvis_results(video)
    assert len(device_calls) == 6 and len(host_calls) == 6
    assert capacities == [30, 30]                                             # 3 clips x 10 instances, not 7 frames x 10
    assert on["pred_labels"] == off["pred_labels"] and on["image_size"] == off["image_size"]
    np.testing.assert_allclose(on["pred_scores"], off["pred_scores"], rtol=1e-5, atol=1e-5)
    assert len(on["pred_masks"]) == len(off["pred_masks"]) >= 10
    assert all(torch.equal(a, b) for a, b in zip(on["pred_masks"], off["pred_masks"]))
    assert len(on_records) == len(off_records)
    for a, b in zip(on_records, off_records):
        assert a["score"] == pytest.approx(b["score"], rel=1e-5, abs=1e-5)
        assert {k: v for k, v in a.items() if k != "score"} == {k: v for k, v in b.items() if k != "score"}


@pytest.mark.gpu
def test_model_falls_back_to_the_host_path_beyond_a_limit(monkeypatch):
    model, video = _tiny_model_and_video(monkeypatch)
    off = model(video)
    train.enable_device_clip_matching(model)
    monkeypatch.setattr(DeviceVideos, "MAX_INSTANCES", 4)                     # the clips carry 10 instances
    device_calls = _count_calls(monkeypatch, DeviceVideos, "update_logits")
    host_calls = _count_calls(monkeypatch, Videos, "update")
    on = model(video)
    assert len(device_calls) == 1 and len(host_calls) == 3                    # refused at the first clip, redone on the host
    assert on["pred_labels"] == off["pred_labels"] and on["pred_scores"] == off["pred_scores"]
    assert all(torch.equal(a, b) for a, b in zip(on["pred_masks"], off["pred_masks"]))


@pytest.mark.gpu
def test_a_state_the_device_cannot_hold_is_refused(monkeypatch):
    def no_memory(nbytes, device):
        raise torch.cuda.OutOfMemoryError("planted")
    monkeypatch.setattr(clip_link, "_alloc", no_memory)
    with pytest.raises(ClipLinkUnsupported, match="does not fit"):
        clip_link.new_state(clip_link.config(3, 16, 63, 5, 5, 120), DEV)


def test_model_sizes_the_state_by_its_clip_count():
    """7 frames as clips of 3 every 2 are 3 clips: with 10 instances each the state needs 30 tracks, not 70"""
    assert len(clip_frames(7, 3, 2)) == 3
    assert DeviceVideos(3, 7, 5, (7, 9), "cpu", max_instances=10, num_clips=3).capacity == 30
    assert DeviceVideos(3, 7, 5, (7, 9), "cpu", max_instances=10).capacity == 70
    assert DeviceVideos(5, 36, 40, (90, 160), "cpu", max_instances=10, num_clips=32).capacity == 120


@pytest.mark.gpu
def test_moved_solver_still_agrees_with_scipy():
    from vnext_amd.ops.lsap import lsap_solve
    g = torch.Generator().manual_seed(3)
    for _ in range(3):
        cost = torch.rand(6, 9, generator=g)
        rows, cols = lsap_solve(cost.to(DEV))
        want_r, want_c = linear_sum_assignment(cost.numpy())
        assert rows.cpu().tolist() == want_r.tolist() and cols.cpu().tolist() == want_c.tolist()
