"""Clip-level instance tracking for long SeqFormer videos.

Same decisions and results as `Videos` / `Clips` of
projects/SeqFormer/seqformer/models/clip_output.py:11-144 (overlapping clips are linked by the
space-time IoU of their masks on the shared frames, Hungarian matching at threshold 0.01, a
track's mask logits / class probabilities are the average over the clips that contain it).

Laid out for the machine differently.  The reference keeps two dense
[num_clips, 120, video_length, H/4, W/4] float tensors (19 GB for a 36-frame 360p video, hence its
MERGE_ON_CPU default) and evaluates the sIoU by broadcasting to [C, N_s, N_i, T, HW].  Here a clip
stores only its own frames ([n, clip_len, HW]), and the sIoU of a stored clip against the incoming one
is ONE matrix product on the matrix cores -- intersections = A . B^T over the shared frames' pixels,
unions from the two row sums -- so everything stays on the device; the only host step is the
[N_s, N_i] Hungarian assignment.
"""
from __future__ import annotations

from typing import List

import torch
from scipy.optimize import linear_sum_assignment

from . import tracker as _trk      # shares the similarity entry point (tests swap it for torch.mm on CPU)
from ..ops import clip_link


class Clips:
    """One clip's kept instances (clip_output.py:131-144): cls_probs [n, K], mask_logits [n, T, h, w]."""

    def __init__(self, frame_idx: List[int], results):
        self.frame_idx = list(frame_idx)
        self.frame_set = set(frame_idx)
        self.classes, self.scores = results.pred_classes, results.scores
        self.cls_probs = results.cls_probs
        self.mask_logits = results.pred_masks
        self.mask_probs = results.pred_masks.sigmoid()
        self.num_instance = len(self.scores)


class Videos:
    def __init__(self, num_frames, video_length, num_classes, image_size, device):
        self.num_frames, self.video_length, self.num_classes = num_frames, video_length, num_classes
        self.image_size, self.device = tuple(image_size), device
        self.match_threshold = 0.01
        self.num_inst = 0
        self.saved_idx_set = set()
        self.clips = []     # per stored clip: (frame_idx, track ids [n], logits [n,T,h,w], probs [n,T,hw], cls [n,K])

    @property
    def num_clip(self):
        return len(self.clips)

    def get_siou(self, input_clip):
        """-> [num_inst, N_i]: mean over the recent clips that contain the track of the space-time
        IoU on the frames shared with the incoming clip (clip_output.py:36-63, 73-81)."""
        n_i = input_clip.num_instance
        siou = torch.zeros(self.num_inst, n_i, device=self.device)
        count = torch.zeros(self.num_inst, device=self.device)
        in_pos = {f: k for k, f in enumerate(input_clip.frame_idx)}
        b_all = input_clip.mask_probs.flatten(2).to(self.device, torch.float32)          # [N_i, T_in, HW]
        for frame_idx, ids, _, probs, _ in self.clips[max(self.num_clip - len(input_clip.frame_idx), 0):]:
            shared = [(k, in_pos[f]) for k, f in enumerate(frame_idx) if f in in_pos and f in self.saved_idx_set]
            if not shared or len(ids) == 0:
                continue
            a = probs[:, [k for k, _ in shared]].flatten(1)                                # [n_c, |shared| HW]
            b = b_all[:, [j for _, j in shared]].flatten(1)
            inter = _trk._pairwise_dot(a.contiguous(), b.contiguous())                     # one GEMM
            union = a.sum(1)[:, None] + b.sum(1)[None, :] - inter
            siou[ids] += inter / (union + 1e-6)
            count[ids] += 1
        return siou / (count[:, None] + 1e-6)

    def update(self, input_clip):
        n_i = input_clip.num_instance
        scores = self.get_siou(input_clip) if (self.num_inst and n_i) else torch.zeros(self.num_inst, n_i)
        above = scores > self.match_threshold
        host = (scores * above.float()).cpu().numpy()
        above = above.cpu().numpy()
        rows, cols = linear_sum_assignment(host, maximize=True) if host.size else ([], [])
        track_of = {}
        for r, c in zip(rows, cols):
            if above[r, c]:
                track_of[int(c)] = int(r)
        for c in range(n_i):                       # unmatched instances open new tracks, in input order
            if c not in track_of:
                track_of[c] = self.num_inst
                self.num_inst += 1
        ids = torch.tensor([track_of[c] for c in range(n_i)], dtype=torch.long, device=self.device)
        logits = input_clip.mask_logits.to(self.device, torch.float32)
        self.clips.append((list(input_clip.frame_idx), ids, logits, input_clip.mask_probs.flatten(2).to(self.device, torch.float32),
                           input_clip.cls_probs.to(self.device, torch.float32)))
        self.saved_idx_set.update(input_clip.frame_set)

    def get_result(self):
        """-> (class probabilities [N, K], mask logits [N, video_length, h, w]); frames no clip of a
        track covers are 0/0 = NaN as in the reference (they threshold to background)."""
        h, w = self.image_size
        total = torch.zeros(self.num_inst, self.video_length, h, w, device=self.device)
        seen = torch.zeros(self.num_inst, self.video_length, device=self.device)
        cls = torch.zeros(self.num_inst, self.num_classes, device=self.device)
        in_clips = torch.zeros(self.num_inst, device=self.device)
        for frame_idx, ids, logits, _, cls_probs in self.clips:
            if len(ids) == 0:
                continue
            f = torch.tensor(frame_idx, dtype=torch.long, device=self.device)
            total[ids[:, None], f[None, :]] += logits
            seen[ids[:, None], f[None, :]] += 1
            cls[ids] += cls_probs
            in_clips[ids] += 1
        return cls / in_clips[:, None], total / seen[..., None, None]


class DeviceVideos:
    """`Videos` with the video's state in device memory (vnext_amd/csrc/clip_link.hip, vnext_amd/ops/clip_link.py): the
    last `num_frames` clips' mask probabilities, every track's running sums and the track counter live there, a clip
    costs one call of three launches and nothing is copied to the host before `get_result`.  Same constructor as
    `Videos` plus `capacity` (tracks the state has room for; the reference's num_max_inst), `max_instances`
    (instances of a clip at most) and `num_clips` (when the caller knows it: with max_instances it bounds the tracks).

    update_logits(frame_idx, cls_probs, mask_logits[, ids_out]) -> ids [n] int64 ON THE DEVICE, no synchronisation.
    update(clip)      the same for a `Clips` object (its sigmoid copy is not used).
    get_result()      -> (cls [N, K], logits [N, L, h, w]); one host copy, of the three counters.
    Raises ClipLinkUnsupported -- link the video with `Videos` -- for a clip of more instances or frames than the kernels
    take, and from get_result when an instance found no free track.  The same ids as `Videos` wherever no assignment and
    no comparison with the threshold is decided by fp32 rounding of a score.
    """
    MAX_INSTANCES = clip_link.MAX_INSTANCES      # what the kernels take: a state is never built for more

    def __init__(self, num_frames, video_length, num_classes, image_size, device, capacity=120, max_instances=16,
                 num_clips=None):
        self.num_frames, self.video_length, self.num_classes = int(num_frames), int(video_length), int(num_classes)
        self.image_size, self.device = tuple(int(v) for v in image_size), device
        self.max_instances = max(1, min(int(max_instances), self.MAX_INSTANCES))
        # a clip opens at most max_instances tracks, and clips that start on distinct frames are at most video_length
        clips = self.video_length if num_clips is None else max(1, int(num_clips))
        self.capacity = max(1, min(int(capacity), self.max_instances * clips))
        self.num_clip = 0
        self.recent = []        # the ring as the host sees it: (slot, frame list) of the last num_frames clips, oldest first
        self.cfg = self.state = self.workspace = None

    def _start(self):
        self.cfg = clip_link.config(self.num_frames, self.max_instances, self.image_size[0] * self.image_size[1],
                                    self.video_length, self.num_classes, self.capacity)
        self.state, self.workspace = clip_link.new_state(self.cfg, self.device)

    def counters(self):
        """(tracks opened, instances that found no free track, clips taken) -- one host copy."""
        if self.state is None:
            return 0, 0, 0
        return tuple(self.state[:12].view(torch.int32).tolist())

    @property
    def num_inst(self):
        return self.counters()[0]

    def update_logits(self, frame_idx, cls_probs, mask_logits, ids_out=None):
        if not mask_logits.is_cuda or not cls_probs.is_cuda:
            raise RuntimeError("DeviceVideos: Not implemented on the CPU (Videos is the host form)")
        if self.state is None:
            self._start()
        frame_idx = [int(f) for f in frame_idx]
        n = mask_logits.shape[0]
        logits = mask_logits.reshape(n, len(frame_idx), self.cfg.pixels).to(torch.float32).contiguous()
        probs = cls_probs.reshape(n, self.num_classes).to(torch.float32).contiguous()
        slot = self.num_clip % self.num_frames
        # Videos.get_siou looks at the last len(frame_idx) clips
        window = self.recent[max(len(self.recent) - len(frame_idx), 0):]
        ids = clip_link.update(self.cfg, self.state, self.workspace, logits, probs,
                               clip_link.plan(frame_idx, slot, window), ids_out)
        self.recent = (self.recent + [(slot, frame_idx)])[-self.num_frames:]
        self.num_clip += 1
        return ids

    def update(self, input_clip):
        return self.update_logits(input_clip.frame_idx, input_clip.cls_probs, input_clip.mask_logits)

    def get_result(self, cls_out=None, logits_out=None):
        """-> (class probabilities [N, K], mask logits [N, video_length, h, w]), as `Videos.get_result`; written into
        `cls_out` [N, K] / `logits_out` [N, video_length, h * w] when the caller brings them."""
        h, w = self.image_size
        if self.state is None:
            return (torch.zeros(0, self.num_classes, device=self.device),
                    torch.zeros(0, self.video_length, h, w, device=self.device))
        opened, lost, _ = self.counters()
        if lost:
            raise clip_link.ClipLinkUnsupported(
                f"DeviceVideos: {lost} instances found no free track (capacity {self.capacity})")
        cls, logits = clip_link.result(self.cfg, self.state, opened, cls_out, logits_out)
        return cls, logits.view(opened, self.video_length, h, w)
