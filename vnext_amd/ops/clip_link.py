"""SeqFormer's clip matching with the video's state in device memory (vnext_amd/csrc/clip_link.hip): one call per clip,
three launches, no host copy.

`new_state` sizes and zeroes one video's state, `update` links one clip -- sIoU against the stored clips on the shared
frames, assignment, new tracks, the running sums -- and returns the track of every instance as a device tensor, `result`
divides the sums out.  The frame lists stay with the host, which owns them: `plan` turns them into the shared-frame pairs
that travel to the kernels by value.  No call here synchronises or copies to the host; reading the counters does
(`models.clip_matching.DeviceVideos.counters`).

CUDA tensors only, like the other kernels of this package: there is no CPU implementation behind these calls (the host
form of the linkage is `models.clip_matching.Videos`).
"""
from __future__ import annotations

import ctypes

import torch

from .. import _lib

MAX_INSTANCES, MAX_FRAMES = _lib.CLIP_LINK_MAX_INSTANCES, _lib.CLIP_LINK_MAX_FRAMES


class ClipLinkUnsupported(_lib.VnextHipError):
    """The clip, or the video, is outside what the kernels take (instances, frames, track capacity): link it with `Videos`."""


def _check(status: int) -> None:
    if status == _lib.VNX_ERR_UNSUPPORTED:
        raise ClipLinkUnsupported(_lib.lib().vnx_last_error().decode())
    _lib.check(status)


def _cpu(what):
    return RuntimeError(f"{what}: Not implemented on the CPU (models.clip_matching.Videos is the host form)")


def _alloc(nbytes, device):
    return torch.empty(nbytes, dtype=torch.uint8, device=device)


def config(ring, max_instances, pixels, video_length, classes, capacity):
    return _lib.ClipLinkConfig(ring=int(ring), max_instances=int(max_instances), pixels=int(pixels),
                               video_length=int(video_length), classes=int(classes), capacity=int(capacity))


def new_state(cfg, device):
    """-> (state, workspace): uint8 device tensors, the state zeroed on the current stream.  Raises ClipLinkUnsupported
    for a configuration beyond the kernels' limits, or a state the device has no memory for."""
    device = torch.device(device)
    if device.type != "cuda":
        raise _cpu("clip_link.new_state")
    lib, ptr = _lib.lib(), ctypes.addressof(cfg)
    with torch.cuda.device(device):
        if lib.vnx_clip_link_state_bytes(ptr) == 0:      # a refused configuration: reset returns its status
            _check(lib.vnx_clip_link_reset(ptr, None, None))
        try:
            state = _alloc(lib.vnx_clip_link_state_bytes(ptr), device)
            workspace = _alloc(lib.vnx_clip_link_workspace_bytes(ptr), device)
        except torch.cuda.OutOfMemoryError as e:      # `total` grows with capacity x video_length x pixels
            raise ClipLinkUnsupported(f"clip_link.new_state: a state of {lib.vnx_clip_link_state_bytes(ptr)} bytes "
                                      f"does not fit the device's free memory") from e
        _check(lib.vnx_clip_link_reset(ptr, state.data_ptr(), _lib.current_stream(state)))
    return state, workspace


def plan(frame_idx, write_slot, stored):
    """The incoming clip's frames, the ring slot it goes to and `stored` = [(ring slot, frame list)] of the clips it is
    compared with, oldest first -> vnx_clip_link_plan: per stored clip that shares a frame, the shared (stored position,
    incoming position) pairs.  A clip of more than MAX_FRAMES frames gets a plan that names its length alone (the call
    refuses it)."""
    p = _lib.ClipLinkPlan(frames=len(frame_idx), write_slot=int(write_slot))
    if len(frame_idx) > MAX_FRAMES:
        return p
    at = {}
    for k, f in enumerate(frame_idx):
        p.frame_index[k] = int(f)
        at[int(f)] = k
    for slot, frames in stored:
        shared = [(k, at[int(f)]) for k, f in enumerate(frames) if int(f) in at]
        if not shared:
            continue
        a = p.slots
        p.slot[a], p.pairs[a] = int(slot), len(shared)
        for i, (k, j) in enumerate(shared):
            p.stored_pos[a][i], p.incoming_pos[a][i] = k, j
        p.slots = a + 1
    return p


def update(cfg, state, workspace, mask_logits, cls_probs, link_plan, ids_out=None):
    """mask_logits fp32 [n, T, HW] and cls_probs fp32 [n, K], contiguous on the device -> ids int64 [n] on the device
    (`ids_out` if given).  Raises ClipLinkUnsupported, the state untouched, for a clip beyond the state's limits."""
    if not state.is_cuda or not mask_logits.is_cuda:
        raise _cpu("clip_link.update")
    n = int(mask_logits.shape[0])
    if mask_logits.dtype != torch.float32 or cls_probs.dtype != torch.float32 or not mask_logits.is_contiguous() or \
            not cls_probs.is_contiguous() or mask_logits.dim() != 3 or tuple(cls_probs.shape) != (n, cfg.classes) or \
            tuple(mask_logits.shape[1:]) != (link_plan.frames, cfg.pixels):
        raise ValueError(f"clip_link.update: contiguous fp32 [n, {link_plan.frames}, {cfg.pixels}] logits and "
                         f"[n, {cfg.classes}] probabilities expected, got {tuple(mask_logits.shape)} {mask_logits.dtype} / "
                         f"{tuple(cls_probs.shape)} {cls_probs.dtype}")
    with torch.cuda.device(state.device):
        ids = torch.empty(n, dtype=torch.int64, device=state.device) if ids_out is None else ids_out
        if ids.dtype != torch.int64 or ids.numel() != n or not ids.is_contiguous():
            raise ValueError("clip_link.update: ids_out must be a contiguous int64 [n]")
        _check(_lib.lib().vnx_clip_link_update(
            ctypes.addressof(cfg), state.data_ptr(), mask_logits.data_ptr(), cls_probs.data_ptr(),
            ctypes.addressof(link_plan), n, ids.data_ptr(), workspace.data_ptr(), workspace.numel(),
            _lib.current_stream(state)))
    return ids


def result(cfg, state, num_tracks, cls_out=None, logits_out=None):
    """-> (cls [num_tracks, K], logits [num_tracks, L, HW]) of the first `num_tracks` tracks: the class probabilities and
    mask logits averaged over the clips that hold each; NaN where no clip of a track covers a frame."""
    if not state.is_cuda:
        raise _cpu("clip_link.result")
    n = int(num_tracks)
    with torch.cuda.device(state.device):
        cls = torch.empty(n, cfg.classes, device=state.device) if cls_out is None else cls_out
        logits = torch.empty(n, cfg.video_length, cfg.pixels, device=state.device) if logits_out is None else logits_out
        for t, shape in ((cls, (n, cfg.classes)), (logits, (n, cfg.video_length, cfg.pixels))):
            if t.dtype != torch.float32 or tuple(t.shape) != shape or not t.is_contiguous():
                raise ValueError(f"clip_link.result: contiguous fp32 {shape} output expected")
        _check(_lib.lib().vnx_clip_link_result(ctypes.addressof(cfg), state.data_ptr(), n, cls.data_ptr(),
                                               logits.data_ptr(), _lib.current_stream(state)))
    return cls, logits


def debug_scores(workspace, num_instances):
    """What the last `update` on this workspace matched on (include/vnext_hip_debug.h) -> (tracks int32 [rows], scores
    fp32 [rows, n]): per track held by a stored clip of the window, its mean sIoU against every incoming instance, before
    the threshold.  Synchronises."""
    rows_off, tracks_off, scores_off = ctypes.c_size_t(), ctypes.c_size_t(), ctypes.c_size_t()
    rows_max, stride = ctypes.c_int(), ctypes.c_int()
    _lib.check(_lib.lib().vnx_debug_clip_link_score_layout(ctypes.byref(rows_off), ctypes.byref(tracks_off),
                                                           ctypes.byref(scores_off), ctypes.byref(rows_max),
                                                           ctypes.byref(stride)))
    rows = int(workspace[rows_off.value:rows_off.value + 4].view(torch.int32).item())
    tracks = workspace[tracks_off.value:tracks_off.value + 4 * rows_max.value].view(torch.int32)[:rows]
    scores = workspace[scores_off.value:scores_off.value + 4 * rows_max.value * stride.value].view(torch.float32)
    return tracks.clone(), scores.view(rows_max.value, stride.value)[:rows, :num_instances].clone()
