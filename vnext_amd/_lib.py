"""ctypes binding of libvnext_hip.so (include/vnext_hip.h).

The library is the product: there is no CPU or PyTorch fallback behind these
calls.  If the .so is missing `lib()` raises; run `python -m vnext_amd.build`
(or `__graft_entry__.build()`) first.
"""
from __future__ import annotations

import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libvnext_hip.so")
# the development build (-DVNX_DEV_VARIANTS + tools/experiments/msda_tile): forced kernel variants for tests and A/B timing
DEV_LIB_PATH = os.path.join(_HERE, "lib", "libvnext_hip_dev.so")

VNX_F32, VNX_F64, VNX_BF16, VNX_F16 = 0, 1, 2, 3
VNX_OK = 0
VNX_ERR_UNSUPPORTED = 2
ABI_VERSION = 17
MSDA_LEVELS_PACKED = 1
MSDA_REF_F32 = 0x100       # or-ed into ref_dim of vnx_msda_fused_*: fp32 reference points beside 16-bit offsets / logits
MASK_RLE_LOGITS, MASK_RLE_BINARY = 0, 1   # vnx_mask_rle_*: input modes
MASK_DENSE_U8, MASK_DENSE_BITS = 0, 1     # vnx_mask_dense: output formats
MSDA_FORK = 2              # vnx_msda_backward: grad_value kernel on the library's side stream (include/vnext_hip.h)
# limits of include/vnext_hip.h, by their names there
MASK_LOSS_MAX_CLIPS, MASK_LOSS_PIECE = 16, 4096            # VNX_MASK_LOSS_MAX_CLIPS, VNX_MASK_LOSS_PIECE
SET_LOSS_PIECE, SET_LOSS_MAX_ROWS = 4096, 1024             # VNX_SET_LOSS_PIECE, VNX_SET_LOSS_MAX_ROWS
REID_LOSS_MAX_ROWS = 1024                                  # VNX_REID_LOSS_MAX_ROWS
CLIP_LINK_MAX_INSTANCES, CLIP_LINK_MAX_FRAMES = 16, 8      # VNX_CLIP_LINK_MAX_INSTANCES, VNX_CLIP_LINK_MAX_FRAMES
INGEST_MAX_LEVELS, INGEST_MAX_POS_FEATS = 8, 128           # VNX_INGEST_MAX_LEVELS, VNX_INGEST_MAX_POS_FEATS
RESIZE_MAX_KSIZE = 17                                      # VNX_RESIZE_MAX_KSIZE
LAYOUT_NCHW, LAYOUT_NHWC = 0, 1                            # VNX_LAYOUT_NCHW, VNX_LAYOUT_NHWC
OPT_CHUNK, ADAMW_UNALIGNED = 4096, 1                       # VNX_ADAMW_CHUNK, VNX_ADAMW_UNALIGNED
# VNX_RLE_RUNS_* status bits of vnx_rle_runs_write, VNX_VIDEO_IOU_* status values of vnx_video_iou_sums
RLE_RUNS_BAD_BYTE, RLE_RUNS_TRUNCATED, RLE_RUNS_NEGATIVE, RLE_RUNS_BAD_SUM, RLE_RUNS_BAD_SLOT = 1, 2, 4, 8, 16
VIDEO_IOU_FRAMES, VIDEO_IOU_PIXELS, VIDEO_IOU_BAD_TABLE = 1, 2, 4
AP_MATCH_MAX_GT, AP_MATCH_MAX_LANES = 512, 64              # VNX_AP_MATCH_MAX_GT, VNX_AP_MATCH_MAX_LANES
AP_MATCH_BAD_TABLE, AP_MATCH_GT_LIMIT = 1, 2               # VNX_AP_MATCH_* status values of vnx_ap_match
# VNX_POLY_RLE_MAX_* caps and VNX_POLY_RLE_* status bits of vnx_poly_rle
POLY_RLE_MAX_VERTICES, POLY_RLE_MAX_CROSSINGS, POLY_RLE_MAX_POINTS, POLY_RLE_MAX_POLYGONS = 1024, 4096, 262144, 256
POLY_RLE_BAD_COORD, POLY_RLE_FEW_VERTICES, POLY_RLE_BAD_SIZE, POLY_RLE_CAP, POLY_RLE_BAD_SLOT = 1, 2, 4, 8, 16

_vp, _i, _sz, _ll = ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, ctypes.c_longlong

# name -> (restype, argtypes); mirrors include/vnext_hip.h declaration by declaration
SIGNATURES = {
    "vnx_abi_version": (_i, []),
    "vnx_status_string": (ctypes.c_char_p, [_i]),
    "vnx_last_error": (ctypes.c_char_p, []),
    "vnx_msda_forward": (_i, [_i, _i, _vp, _vp, _vp, _vp, _vp, _vp] + [_i] * 7 + [_vp]),
    "vnx_msda_backward_workspace_bytes": (_sz, [_i] * 10),
    "vnx_msda_backward": (_i, [_i, _i] + [_vp] * 9 + [_i] * 8 + [_vp, _sz, _vp]),
    "vnx_msda_fused_forward": (_i, [_i, _i] + [_vp] * 7 + [_i] * 9 + [_vp]),
    "vnx_msda_fused_backward_workspace_bytes": (_sz, [_i] * 7),
    "vnx_msda_fused_backward": (_i, [_i, _i] + [_vp] * 11 + [_i] * 9 + [_vp, _sz, _vp]),
    "vnx_dynamic_mask_head_forward": (_i, [_i] + [_vp] * 5 + [_i] * 7 + [_vp]),
    "vnx_dynamic_mask_head_backward": (_i, [_i] + [_vp] * 8 + [_i] * 7 + [_vp]),
    "vnx_dynamic_mask_head_forward_train": (_i, [_i] + [_vp] * 8 + [_i] * 7 + [_vp]),
    "vnx_dynamic_mask_head_backward_zeroed": (_i, [_i] + [_vp] * 8 + [_i] * 7 + [_vp]),
    "vnx_reid_similarity": (_i, [_i] + [_vp] * 3 + [_i] * 7 + [_vp]),
    "vnx_reid_bisoftmax": (_i, [_i] + [_vp] * 2 + [_i] * 4 + [_vp]),
    "vnx_mask_intersections_workspace_bytes": (_sz, [_i, _i]),
    "vnx_mask_intersections": (_i, [_vp, _i, _i, _vp, _vp, _sz, _vp]),
    "vnx_tracker_state_bytes": (_sz, [_vp]),
    "vnx_tracker_reset": (_i, [_vp, _vp, _vp]),
    "vnx_tracker_frame_workspace_bytes": (_sz, [_vp, _i, _i]),
    "vnx_tracker_frame": (_i, [_vp] * 6 + [_i] * 3 + [_vp, _vp, _sz, _vp]),
    "vnx_add_dropout_layernorm_partial_bytes": (_sz, []),
    "vnx_add_dropout_layernorm_forward": (_i, [_i] + [_vp] * 8 + [_ll, _i, ctypes.c_float, ctypes.c_float, ctypes.c_ulonglong, _vp, _vp]),
    "vnx_add_dropout_layernorm_backward": (_i, [_i] + [_vp] * 10 + [_ll, _i, ctypes.c_float, ctypes.c_ulonglong, _vp, _vp]),
    "vnx_bias_relu_dropout_partial_bytes": (_sz, [_i]),
    "vnx_refine_boxes_forward": (_i, [_i, _vp, _vp, _vp, _ll, _i, ctypes.c_float, _vp]),
    "vnx_refine_boxes_backward": (_i, [_i, _vp, _vp, _vp, _vp, _vp, _ll, _i, ctypes.c_float, _vp]),
    "vnx_time_weighted_sum_forward": (_i, [_i, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp]),
    "vnx_time_weighted_sum_backward": (_i, [_i, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp]),
    "vnx_query_self_attention_forward": (_i, [_i, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, ctypes.c_float, ctypes.c_ulonglong, _vp, _vp]),
    "vnx_query_self_attention_backward": (_i, [_i, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, ctypes.c_float,
                                               ctypes.c_ulonglong, _vp, _vp]),
    "vnx_bias_relu_dropout_forward": (_i, [_i, _vp, _vp, _vp, _ll, _i, _i, ctypes.c_float, ctypes.c_ulonglong, _vp, _vp]),
    "vnx_bias_relu_dropout_backward": (_i, [_i, _vp, _vp, _vp, _vp, _vp, _vp, _ll, _i, ctypes.c_float, _vp]),
    "vnx_window_attention_partial_bytes": (_sz, [_i] * 5),
    "vnx_window_attention_forward": (_i, [_i] + [_vp] * 5 + [_i] * 8 + [ctypes.c_float, _vp]),
    "vnx_window_attention_backward": (_i, [_i] + [_vp] * 10 + [_sz] + [_i] * 8 + [ctypes.c_float, _vp]),
    "vnx_mask_rle_measure": (_i, [_i, _vp] + [_i] * 8 + [_vp, _vp]),
    "vnx_mask_rle_write": (_i, [_i, _vp] + [_i] * 8 + [_vp, _vp, _ll, _vp]),
    "vnx_mask_dense": (_i, [_i, _vp] + [_i] * 8 + [_vp, _ll, _vp]),
    "vnx_seqformer_match": (_i, [_vp] * 5 + [_i] * 7 + [ctypes.c_float] * 3 + [_vp] * 4),
    "vnx_lsap_solve": (_i, [_vp, _i, _i, _i, _ll, _ll, _ll, _i, _vp, _vp, _vp]),
    "vnx_mask_loss_forward": (_i, [_vp] * 3 + [_i] * 5 + [ctypes.c_float] * 2 + [_vp, _sz] + [_vp] * 4),
    "vnx_mask_loss_backward": (_i, [_vp] * 3 + [_i] * 5 + [ctypes.c_float] * 2 + [_vp] * 5),
    "vnx_set_loss_forward": (_i, [_vp] * 8 + [_i] * 7 + [ctypes.c_float, _vp, _sz, _vp, _vp]),
    "vnx_set_loss_backward": (_i, [_vp] * 8 + [_i] * 7 + [ctypes.c_float] + [_vp] * 4),
    "vnx_idol_match_max_targets": (_i, [_i]),
    "vnx_idol_match_out_words": (_i, [_i, _i]),
    "vnx_idol_match": (_i, [_vp] * 8 + [_i] * 7 + [_vp, _i, _vp]),
    "vnx_det_select_out_words": (_i, [_i, _i]),
    "vnx_det_select": (_i, [_vp, _vp, _i, _i, _i, ctypes.c_float, ctypes.c_float, _i, _vp, _i, _vp]),
    "vnx_reid_loss_forward": (_i, [_vp, _ll, _i, _vp, _ll, _i, _i, _i, _vp, _vp, _vp, _i] + [_vp] * 5),
    "vnx_reid_loss_backward": (_i, [_vp, _ll, _i, _vp, _ll, _i, _i, _i, _vp, _vp, _vp, _i] + [_vp] * 7),
    "vnx_swin_glue_partial_bytes": (_sz, [_ll, _i]),
    "vnx_swin_residual_norm_forward": (_i, [_i] * 3 + [_vp] * 8 + [_ll, _i, _ll, ctypes.c_float, _vp]),
    "vnx_swin_residual_norm_backward": (_i, [_i] * 3 + [_vp] * 11 + [_sz, _ll, _i, _ll, _vp]),
    "vnx_swin_merge_norm_forward": (_i, [_i] * 2 + [_vp] * 5 + [_i] * 4 + [ctypes.c_float, _vp]),
    "vnx_swin_merge_norm_backward": (_i, [_i] * 2 + [_vp] * 8 + [_sz] + [_i] * 4 + [_vp]),
    "vnx_conv_epilogue_forward": (_i, [_i, _i] + [_vp] * 4 + [_ll] * 3 + [_vp]),
    "vnx_conv_epilogue_backward": (_i, [_i] + [_vp] * 3 + [_ll, _vp]),
    "vnx_stem_pool_forward": (_i, [_i, _i] + [_vp] * 3 + [_ll] * 4 + [_vp]),
    "vnx_clip_link_state_bytes": (_sz, [_vp]),
    "vnx_clip_link_workspace_bytes": (_sz, [_vp]),
    "vnx_clip_link_reset": (_i, [_vp, _vp, _vp]),
    "vnx_clip_link_update": (_i, [_vp] * 5 + [_i, _vp, _vp, _sz, _vp]),
    "vnx_clip_link_result": (_i, [_vp, _vp, _i, _vp, _vp, _vp]),
    "vnx_ingest_frames": (_i, [_vp, _sz, _vp, _i, _i, _i] + [ctypes.c_float] * 6 + [_i, _vp, _vp, _vp]),
    "vnx_ingest_levels": (_i, [_vp, _i, _i, _i, _i, ctypes.POINTER(_i), _i, _vp, _vp, ctypes.POINTER(_vp),
                               ctypes.POINTER(_vp), _vp]),
    "vnx_resize_ingest_frames": (_i, [_vp, _sz, _vp, _vp, _vp, _sz, _i, _i, _i] + [ctypes.c_float] * 6 +
                                 [_i, _i, _vp, _vp, _vp]),
    "vnx_augment_frames": (_i, [_vp, _sz, _vp, _vp, _vp, _sz, _i, _i, _i] + [ctypes.c_float] * 6 + [_i, _i, _vp, _vp, _vp]),
    "vnx_augment_masks_workspace": (_sz, [_i, _i, _i]),
    "vnx_augment_masks": (_i, [_vp, _sz, _vp, _i, _vp, _vp, _vp, _sz, _i, _i, _i, _vp, _sz, _vp, _vp, _vp, _sz, _vp]),
    "vnx_resize_window_bytes": (_i, [_vp, _sz, _vp, _vp, _sz, _i, _i, _i, _i, _vp]),
    "vnx_augment_color_workspace": (_sz, [_i, _i, _i]),
    "vnx_augment_frames_color": (_i, [_vp, _sz, _vp, _vp, _vp, _sz, _vp, _i, _i, _i] + [ctypes.c_float] * 6 +
                                 [_i, _i, _i, _sz, _vp, _vp, _vp]),
    "vnx_adamw_grad_norm":(_i, [_vp, _i, _vp, _ll, ctypes.c_double, _vp, _vp, _vp]),
    "vnx_adamw_clipped_step": (_i, [_vp, _i, _vp, _i, _vp, _ll, _vp, _vp]),
    "vnx_rle_runs_measure": (_i, [_vp, _ll, _vp, _vp, _i, _vp, _vp]),
    "vnx_rle_runs_write": (_i, [_vp, _ll] + [_vp] * 5 + [_i, _vp, _vp, _ll, _vp, _vp, _vp]),
    "vnx_video_iou_sums": (_i, [_vp, _vp, _ll, _vp, _i, _vp, _ll, _vp, _i, _vp, _ll, _vp, _vp]),
    "vnx_ap_match": (_i, [_vp, _ll, _vp, _ll, _vp, _vp, _ll, _vp, _ll, _vp, _i, _vp, _i] + [_vp] * 6),
    "vnx_poly_rle": (_i, [_vp, _ll, _vp, _i, _vp, _i, _vp, _vp, _ll, _vp, _vp, _vp]),
}
# measurement aids of include/vnext_hip_debug.h (bench.py, tools/): not part of the drop-in boundary
DEBUG_SIGNATURES = {
    "vnx_debug_wall_clock_khz": (_i, []),
    "vnx_debug_row_gather_probe": (_i, [_vp, _sz, _vp, _sz, _i, _vp, _vp]),
    "vnx_debug_gvtiles_units": (_i, [_vp, _i, _i, _i, _i, _i, ctypes.POINTER(_i), ctypes.POINTER(_i),
                                    ctypes.POINTER(_ll), ctypes.POINTER(_ll)]),
    "vnx_debug_gvdirect_units": (_i, [_vp, _i, _i, _i, _i, ctypes.POINTER(_i), ctypes.POINTER(_i), _vp, _vp, _vp]),
    "vnx_debug_clip_link_score_layout": (_i, [ctypes.POINTER(_sz)] * 3 + [ctypes.POINTER(_i)] * 2),
}
# include/vnext_hip_dev.h: exported by the development library only
DEV_SIGNATURES = {
    "vnx_set_kernel_variant": (None, [_i]),
    "vnx_get_kernel_variant": (_i, []),
    "vnx_debug_arm_stamps": (None, [_vp, _ll]),
    "vnx_debug_stamp_regions": (_i, [ctypes.POINTER(_i), ctypes.POINTER(_ll), ctypes.POINTER(_ll), _i]),
    "vnx_debug_read_rec_stamps": (_i, [ctypes.POINTER(ctypes.c_ulonglong), _i]),
    "vnx_debug_read_tile_stamps": (_i, [ctypes.POINTER(ctypes.c_ulonglong), _i]),
    "vnx_debug_read_gvd_stamps": (_i, [ctypes.POINTER(ctypes.c_ulonglong), _i]),
}


class TrackerConfig(ctypes.Structure):
    """`vnx_tracker_config` of include/vnext_hip.h, field by field."""
    _fields_ = [(k, _i) for k in ("capacity", "channels", "memory_len", "memo_tracklet_frames", "match_metric",
                                  "long_match", "frame_weight", "temporal_weight")] + \
               [(k, ctypes.c_float) for k in ("nms_thr_pre", "nms_thr_post", "init_score_thr", "addnew_score_thr",
                                              "match_score_thr", "memo_momentum")]


class ClipLinkConfig(ctypes.Structure):
    """`vnx_clip_link_config` of include/vnext_hip.h, field by field."""
    _fields_ = [(k, _i) for k in ("ring", "max_instances", "pixels", "video_length", "classes", "capacity")]


class ClipLinkPlan(ctypes.Structure):
    """`vnx_clip_link_plan` of include/vnext_hip.h, field by field: read on the host during the call, handed to the
    kernels by value."""
    _fields_ = [("frames", _i), ("frame_index", _i * CLIP_LINK_MAX_FRAMES), ("write_slot", _i), ("slots", _i),
                ("slot", _i * CLIP_LINK_MAX_FRAMES), ("pairs", _i * CLIP_LINK_MAX_FRAMES),
                ("stored_pos", (ctypes.c_ubyte * CLIP_LINK_MAX_FRAMES) * CLIP_LINK_MAX_FRAMES),
                ("incoming_pos", (ctypes.c_ubyte * CLIP_LINK_MAX_FRAMES) * CLIP_LINK_MAX_FRAMES)]


class MaskLossClips(ctypes.Structure):
    """`vnx_mask_loss_clips` of include/vnext_hip.h, field by field: read on the host during the call, handed to the
    kernels by value."""
    _fields_ = [("masks", _vp * MASK_LOSS_MAX_CLIPS), ("height", _i * MASK_LOSS_MAX_CLIPS),
                ("width", _i * MASK_LOSS_MAX_CLIPS), ("first", _i * MASK_LOSS_MAX_CLIPS), ("count", _i), ("total", _i)]


class AdamWTensor(ctypes.Structure):
    """`vnx_adamw_tensor` of include/vnext_hip.h, field by field: a row of the tensor table in device memory (64 bytes)."""
    _fields_ = [("p", _vp), ("g", _vp), ("m", _vp), ("v", _vp), ("numel", _ll), ("group", _i), ("flags", _i),
                ("bias_correction1", ctypes.c_float), ("bias_correction2_sqrt", ctypes.c_float), ("reserved", _i * 2)]


class AdamWGroup(ctypes.Structure):
    """`vnx_adamw_group` of include/vnext_hip.h, field by field: a row of the group table in device memory (64 bytes)."""
    _fields_ = [(k, ctypes.c_double) for k in ("lr", "weight_decay", "beta1", "beta2", "eps", "decay", "one_minus_beta1",
                                              "one_minus_beta2")]


_lib = None          # the product library
_dev = None          # the development library, loaded on the first request for a kernel variant
_active_dev = False  # True while a non-zero kernel variant is set: lib() then hands out the development library


class VnextHipError(RuntimeError):
    pass


def _load(path: str, tables) -> ctypes.CDLL:
    if not os.path.exists(path):
        raise VnextHipError(
            f"{path} is missing: the HIP library is the only implementation of this "
            "path (no CPU fallback). Build it with `python -m vnext_amd.build`.")
    # torch ships its own libamdhip64.so.7; import it first so this library binds to
    # the HIP runtime torch's allocator and streams live in.
    import torch  # noqa: F401
    cdll = ctypes.CDLL(path, mode=ctypes.RTLD_LOCAL)
    for table in tables:
        for name, (res, args) in table.items():
            fn = getattr(cdll, name)
            fn.restype = res
            fn.argtypes = args
    if cdll.vnx_abi_version() != ABI_VERSION:
        raise VnextHipError(f"ABI version {cdll.vnx_abi_version()} != {ABI_VERSION}; rebuild")
    return cdll


def product_lib() -> ctypes.CDLL:
    global _lib
    if _lib is None:
        path = os.environ.get("VNX_HIP_LIB") or LIB_PATH    # override: experiment builds (tools/bench_ab.sh)
        _lib = _load(path, (SIGNATURES, DEBUG_SIGNATURES))
    return _lib


def dev_lib() -> ctypes.CDLL:
    """libvnext_hip_dev.so (include/vnext_hip_dev.h): tests and tools only."""
    global _dev
    if _dev is None:
        _dev = _load(os.environ.get("VNX_HIP_DEV_LIB") or DEV_LIB_PATH, (SIGNATURES, DEBUG_SIGNATURES, DEV_SIGNATURES))
    return _dev


def lib() -> ctypes.CDLL:
    """The library every op of this package calls: the product -- except while a test or a tool holds a non-zero
    kernel variant (set_kernel_variant), when it is the development build that has variants at all."""
    return dev_lib() if _active_dev else product_lib()


def check(status: int) -> None:
    if status != VNX_OK:
        l = lib()
        raise VnextHipError(
            f"{l.vnx_status_string(status).decode()}: {l.vnx_last_error().decode()}")


def current_stream(tensor) -> int:
    """hipStream_t of torch's current stream on the tensor's device."""
    import torch
    return torch.cuda.current_stream(tensor.device).cuda_stream


def set_kernel_variant(v: int) -> None:
    """Tests / tools: route this package's ops through the development library with kernel variant `v` (forced
    configurations, archived kernels, timing ablations: include/vnext_hip_dev.h); 0 returns to the product library,
    which has no variants."""
    global _active_dev
    v = int(v)
    if v != 0:
        dev_lib().vnx_set_kernel_variant(v)
        _active_dev = True
    else:
        if _dev is not None:
            _dev.vnx_set_kernel_variant(0)
        _active_dev = False
