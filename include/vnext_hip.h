/*
 * include/vnext_hip.h -- C ABI of libvnext_hip.so (MI355X / gfx950).
 *
 * This is the drop-in boundary for VNext's data-parallel hot path.  Every entry
 * point takes plain device pointers, sizes and a HIP stream, returns an int
 * status, never allocates, never synchronises and never keeps a pointer after
 * it returns, so a call is re-entrant and hipGraph-capturable.  No torch type
 * appears here; the Python module `MultiScaleDeformableAttention` (repo root)
 * and vnext_amd/ bind these symbols through ctypes (INTEGRATION.md shows the
 * binding a VNext maintainer would add).
 *
 * Reference interfaces replaced (paths relative to the VNext tree):
 *   vnx_msda_forward   <- ms_deform_attn_forward
 *        projects/SeqFormer/seqformer/models/ops/src/ms_deform_attn.h:20-39,
 *        src/cuda/ms_deform_attn_cuda.cu:20-80, src/vision.cpp:14
 *   vnx_msda_backward  <- ms_deform_attn_backward
 *        .../src/ms_deform_attn.h:41-61, src/cuda/ms_deform_attn_cuda.cu:83-153,
 *        src/vision.cpp:15
 *
 * Tensor layouts are the reference's (all contiguous, ms_deform_attn_cuda.cu:28-38):
 *   value            [batch, spatial_size, num_heads, channels]
 *   spatial_shapes   [num_levels, 2]  int64, (H_l, W_l), DEVICE memory
 *   level_start_index[num_levels]     int64, DEVICE memory
 *   sampling_loc     [batch, num_query, num_heads, num_levels, num_point, 2]  (x, y) in [0,1]
 *   attn_weight      [batch, num_query, num_heads, num_levels, num_point]
 *   output / grad_output [batch, num_query, num_heads*channels]
 */
#ifndef VNEXT_HIP_H_
#define VNEXT_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VNX_ABI_VERSION 17

/* element types */
enum {
  VNX_F32 = 0,
  VNX_F64 = 1,
  VNX_BF16 = 2,
  VNX_F16 = 3
};

/* status codes */
enum {
  VNX_OK = 0,
  VNX_ERR_INVALID_ARGUMENT = 1, /* null pointer, non-positive size, bad dtype combination */
  VNX_ERR_UNSUPPORTED = 2,      /* shape outside what the kernels address (see vnx_last_error) */
  VNX_ERR_WORKSPACE = 3,        /* workspace missing or too small */
  VNX_ERR_LAUNCH = 4            /* hipGetLastError() != hipSuccess after the launch */
};

/* Library identification.  vnx_abi_version() == VNX_ABI_VERSION. */
int vnx_abi_version(void);
/* Static string for a status code. */
const char* vnx_status_string(int status);
/* Thread-local detail of the last non-OK status returned on this thread. */
const char* vnx_last_error(void);

/*
 * Multi-scale deformable attention, forward.
 *   output[b,q,m,:] = sum_{l,k} attn[b,q,m,l,k] * bilinear(value_l[b,:,m,:], loc[b,q,m,l,k])
 * zero padding outside the maps, pixel convention x*W-0.5 / y*H-0.5
 * (ms_deform_im2col_cuda.cuh:285-288).  `output` is fully written (it does not
 * need the reference's zero pre-fill, ms_deform_attn_cuda.cu:54).
 *
 * value_dtype: type of value and output (F32, F64, BF16, F16).
 * loc_dtype  : type of sampling_loc and attn_weight; equal to value_dtype, or
 *              VNX_F32 with a 16-bit value (the autocast case).
 * The reference's im2col_step chunking (ms_deform_attn_cuda.cu:50-75) is a host
 * concern and is not part of this ABI: one call covers the whole batch.
 */
int vnx_msda_forward(int value_dtype, int loc_dtype,
                     const void* value, const int64_t* spatial_shapes,
                     const int64_t* level_start_index, const void* sampling_loc,
                     const void* attn_weight, void* output,
                     int batch, int spatial_size, int num_heads, int channels,
                     int num_levels, int num_query, int num_point,
                     void* hip_stream);

/* flags of vnx_msda_backward */
enum {
  /*
   * The caller guarantees the levels are packed back to back in order:
   * level_start_index[l] == sum_{j<l} H_j*W_j and the sum over all levels ==
   * spatial_size -- the layout the reference always builds
   * (projects/SeqFormer/seqformer/models/deformable_transformer.py:97-106).
   * Without the flag the library works out the same predicate ON THE DEVICE and
   * issues both the fast kernels and the general ones, each set exiting at once when
   * the predicate is not theirs (no host synchronisation, ~2 empty launches).
   */
  VNX_MSDA_LEVELS_PACKED = 1,
  /*
   * Fork the call: a backward call below 1 024 queries (32-channel heads) is two halves neither of which reads what the
   * other writes (grad_value; grad_sampling_loc + grad_attn_weight).  By default they are ONE launch whose workgroups take
   * either role (fp32 locations, 4 levels x 4 points: the decoders' calls) or two launches one after the other on `hip_stream`.  With this flag the grad_value kernel is launched on a side stream the library keeps per host thread
   * and device (created on first use, never synchronised with the host), between an event recorded on `hip_stream` and an
   * event `hip_stream` then waits for: the two kernels share the GPU, `hip_stream` sees the call as one operation, a stream
   * capture records a fork and a join.  Measured on MI355X / ROCm 7.2: the pair then spans 24.3
   * instead of 29.1 us, but the two cross-queue dependencies cost a captured graph 9 us per call and an eager caller
   * 19 us -- a loss today, hence opt-in.
   */
  VNX_MSDA_FORK = 2
};

/*
 * Bytes of scratch vnx_msda_backward needs for these sizes and flags.  32-channel heads: below 1 024
 * queries NONE (since ABI 12: the grad_value kernel decodes the op's own inputs; until ABI 11 the grad_loc
 * kernel left it 20 B per sample of records + unit tags); from 1 024 queries up (4 levels x 4 points) what
 * the grad_loc kernel hands the grad_value kernel -- 8 B per (batch, head, level, query tile), a tile
 * being the queries one wave of the grad_loc kernel handles (4 on calls of up to 262 144 query rows, 8
 * beyond), plus the fp32 partial rows in which the query pieces of the coarse levels meet (at most
 * 16 x min(S, 4 096) rows of 128 B per (batch, head) on calls of fewer than 32 (batch, head) pairs, 4 x
 * from 32 pairs up) -- size the scratch with this function, not by hand.  16-bit values additionally need an fp32 [B, S, M, 32] image of grad_value when the levels are
 * not promised packed (the general path accumulates with fp32 atomics), or on the record-fed path with
 * >= 1 024 queries (other level / point counts than 4 x 4).  Other head widths: that image for 16-bit
 * values, else 0.
 */
size_t vnx_msda_backward_workspace_bytes(int value_dtype, int loc_dtype, int batch,
                                         int spatial_size, int num_heads, int channels,
                                         int num_levels, int num_query, int num_point, int flags);

/*
 * Multi-scale deformable attention, backward (ms_deform_im2col_cuda.cuh:87-159).
 * All three gradient buffers are fully written; they need no zero pre-fill by
 * the caller (the reference's three at::zeros_like, ms_deform_attn_cuda.cu:121-123,
 * disappear, or happen on `hip_stream` inside the call where the general path
 * still needs one).
 *   grad_value        like value        (value_dtype)
 *   grad_sampling_loc like sampling_loc (loc_dtype)
 *   grad_attn_weight  like attn_weight  (loc_dtype)
 * With 32-channel heads and packed levels grad_value is produced without global
 * atomics (one owner per row, accumulation in LDS); otherwise it is accumulated
 * with hardware floating-point atomics as in the reference.  Either way its
 * low-order bits depend on scheduling.
 */
int vnx_msda_backward(int value_dtype, int loc_dtype,
                      const void* value, const int64_t* spatial_shapes,
                      const int64_t* level_start_index, const void* sampling_loc,
                      const void* attn_weight, const void* grad_output,
                      void* grad_value, void* grad_sampling_loc, void* grad_attn_weight,
                      int batch, int spatial_size, int num_heads, int channels,
                      int num_levels, int num_query, int num_point, int flags,
                      void* workspace, size_t workspace_bytes,
                      void* hip_stream);

/*
 * MSDeformAttn with the module's prologue fused in.  Instead of
 * sampling_locations / attention_weights the kernels take what the module computes them from:
 *   sampling_offsets  [batch, num_query, num_heads, num_levels, num_point, 2]  output of the
 *                     `sampling_offsets` Linear
 *   attention_logits  [batch, num_query, num_heads, num_levels * num_point]    output of the
 *                     `attention_weights` Linear, BEFORE the softmax
 *   reference_points  [batch / reference_batch_div, num_query, num_levels, ref_dim]
 * and evaluate   attention = softmax(logits)   and
 *   ref_dim 2:  location = reference + offsets / (W_l, H_l)
 *   ref_dim 4:  location = reference_xy + offsets / num_point * reference_wh * 0.5
 * (projects/IDOL/idol/models/ops/modules/ms_deform_attn.py:99-108; SeqFormer :99-112, :159-161)
 * inside the sampling kernels, so the two intermediate tensors never exist in memory.
 * reference_batch_div > 1: that many consecutive batch elements share one reference row (the
 * frames of a clip in SeqFormer's encoder).  Requirements: channels == 32,
 * num_levels * num_point == 16, value f32 or bf16 (offsets / logits / references all
 * `query_dtype`: f32, or bf16 with a bf16 value; ABI 14: `ref_dim | VNX_MSDA_REF_F32` says the
 * reference points are fp32 although offsets / logits are bf16 -- under torch.autocast the two
 * Linears emit bf16 while the reference points stay fp32, and rounding positions to 8 mantissa
 * bits would cost more than half a pixel at 720p), PACKED levels (level_start_index = running
 * sum of H*W; the backward's grad_value kernel does nothing on the device otherwise).  Anything
 * else: VNX_ERR_UNSUPPORTED -- use vnx_msda_forward / vnx_msda_backward.
 * Backward: grad_sampling_offsets / grad_attention_logits like their inputs; grad_value like
 * value; grad_reference_points (optional, fp32 [batch, num_query, num_levels, 2], ref_dim 2
 * and reference_batch_div 1 only) is zero-filled inside and accumulated over heads with fp32
 * atomics.  workspace: vnx_msda_fused_backward_workspace_bytes(...) bytes of device memory.
 */
#define VNX_MSDA_REF_F32 0x100      /* or-ed into ref_dim of vnx_msda_fused_forward / _backward (see above) */
int vnx_msda_fused_forward(int value_dtype, int query_dtype, const void* value, const int64_t* spatial_shapes,
                           const int64_t* level_start_index, const void* sampling_offsets,
                           const void* attention_logits, const void* reference_points, void* output,
                           int batch, int spatial_size, int num_heads, int channels, int num_levels,
                           int num_query, int num_point, int ref_dim, int reference_batch_div, void* hip_stream);
size_t vnx_msda_fused_backward_workspace_bytes(int value_dtype, int batch, int spatial_size, int num_heads,
                                               int num_levels, int num_query, int num_point);
int vnx_msda_fused_backward(int value_dtype, int query_dtype, const void* value, const int64_t* spatial_shapes,
                            const int64_t* level_start_index, const void* sampling_offsets,
                            const void* attention_logits, const void* reference_points, const void* grad_output,
                            void* grad_value, void* grad_sampling_offsets, void* grad_attention_logits,
                            float* grad_reference_points, int batch, int spatial_size, int num_heads,
                            int channels, int num_levels, int num_query, int num_point, int ref_dim,
                            int reference_batch_div, void* workspace, size_t workspace_bytes, void* hip_stream);

/*
 * CondInst-style dynamic mask head, forward (per-instance 1x1 conv stack 10->8->8->1 on
 * [relative coordinates | 8 mask features], ReLU between, then the x2 "aligned bilinear"
 * up-sampling), fused into one kernel.  Replaces the op chain
 *   CondInst_segm.dynamic_mask_with_coords + mask_heads_forward + parse_dynamic_params +
 *   compute_locations + aligned_bilinear
 *   (projects/SeqFormer/seqformer/models/segmentation_condInst.py:425-493, 404-422, 614-637,
 *    665-678, 640-662; same code in projects/IDOL/idol/models/segmentation_condInst.py:398-468).
 *   mask_feats       [num_images, channels=8, height, width]          (stride-8 mask features)
 *   reference_points [num_insts, 2]   (x, y) in image pixels
 *   params           [num_insts, num_params=169]  split [w0(80) w1(64) w2(8) b0(8) b1(8) b2(1)]
 *   inst_image       [num_insts] int32: the image each instance belongs to (the reference's
 *                    `num_insts` list, expanded; DEVICE memory)
 *   out              [num_insts, 2*height, 2*width], fully written
 * `stride` is mask_feat_stride (8): pixel centres are x*stride + stride/2.
 * Limits (VNX_ERR_UNSUPPORTED beyond them): width <= 3 711 columns of the stride-8 feature map -- images up to 29 688 pixels
 * wide; the kernel keeps one row of logits + 384 pixels per wave in LDS -- and height * width < 2^26.
 */
int vnx_dynamic_mask_head_forward(int dtype, const void* mask_feats, const void* reference_points,
                                  const void* params, const int32_t* inst_image, void* out,
                                  int num_images, int channels, int height, int width,
                                  int num_insts, int num_params, int stride, void* hip_stream);

/*
 * Dynamic mask head, backward (the training path, forward_mask_head_train,
 * segmentation_condInst.py:354-401): gradients of the chain above with respect to the mask
 * features, the reference points and the per-instance parameters, contracted with grad_out.
 * Replaces what autograd runs for the reference: the transposes of pad/interpolate/pad, three
 * grouped-conv backward-data + three backward-weight launches (groups = num_insts), the ReLU
 * masks and the reduction over the `repeat`ed feature map (:452-456).  Nothing is saved by
 * the forward; the hidden layers are recomputed.
 *   grad_out    [num_insts, 2*height, 2*width]
 *   grad_feats  [num_images, 8, height, width]   sum over the instances of each image
 *   grad_ref    [num_insts, 2]
 *   grad_params [num_insts, 169]
 * All three outputs are fully defined on return (zero-filled inside, then accumulated with
 * fp32 atomics: the order of the sums over pixels / instances is not fixed, as in the
 * reference's cuDNN/MIOpen weight-gradient kernels).
 */
int vnx_dynamic_mask_head_backward(int dtype, const void* mask_feats, const void* reference_points,
                                   const void* params, const int32_t* inst_image, const void* grad_out,
                                   void* grad_feats, void* grad_ref, void* grad_params,
                                   int num_images, int channels, int height, int width,
                                   int num_insts, int num_params, int stride, void* hip_stream);

/*
 * The training pair (ABI 15): the forward of a call whose backward will follow, and that backward.
 * `vnx_dynamic_mask_head_forward_train` is `vnx_dynamic_mask_head_forward` whose launch ALSO zero-fills the three gradient
 * buffers the backward accumulates into (each thread of the forward's grid a slice, before anything else: the buffers are
 * outputs of the later backward, nothing in the forward reads them); `vnx_dynamic_mask_head_backward_zeroed` is
 * `vnx_dynamic_mask_head_backward` WITHOUT its own zero-fill launch -- the caller guarantees that grad_feats / grad_ref /
 * grad_params hold zeros (from the forward above, or any other fill) and that nothing wrote to them since.  Same arguments,
 * same limits, same results; one launch fewer per training step (4.8 us of the 35-us training forward + backward at the
 * bench's shape).  What `forward_mask_head_train` (segmentation_condInst.py:354-401) needs from autograd is unchanged: the
 * Python side allocates the three buffers at forward time and hands them to the backward (vnext_amd/heads/dynamic_mask.py).
 */
int vnx_dynamic_mask_head_forward_train(int dtype, const void* mask_feats, const void* reference_points,
                                        const void* params, const int32_t* inst_image, void* out,
                                        void* grad_feats, void* grad_ref, void* grad_params,
                                        int num_images, int channels, int height, int width,
                                        int num_insts, int num_params, int stride, void* hip_stream);
int vnx_dynamic_mask_head_backward_zeroed(int dtype, const void* mask_feats, const void* reference_points,
                                          const void* params, const int32_t* inst_image, const void* grad_out,
                                          void* grad_feats, void* grad_ref, void* grad_params,
                                          int num_images, int channels, int height, int width,
                                          int num_insts, int num_params, int stride, void* hip_stream);

/*
 * IDOL re-identification head: similarity matrix  out[i, j] = <a_i, b_j>  for a [n, channels]
 * (row stride lda) and b [k, channels] (row stride ldb), on the matrix cores in exact fp32.
 * normalize != 0 fuses F.normalize(., p=2, dim=1, eps=1e-12) of both operands (cosine).
 * Replaces torch.mm(embeds, memo_embeds.t()) / the cosine variant
 * (projects/IDOL/idol/models/tracker.py:229-244) and the per-instance
 * einsum('nc,kc->nk') calls of projects/IDOL/idol/models/pos_neg_select.py:47,58-62.
 * Rows must be 16-byte aligned (lda, ldb multiples of 4).  out [n, k], row stride ldo.
 */
int vnx_reid_similarity(int dtype, const void* a, const void* b, void* out, int n, int k,
                        int channels, int lda, int ldb, int ldo, int normalize, void* hip_stream);

/*
 * Bi-directional softmax association score (tracker.py:232-235):
 *   out = (softmax(sim, dim=1) + softmax(sim, dim=0)) / 2      sim, out [n, k], n, k <= 4096
 */
int vnx_reid_bisoftmax(int dtype, const void* sim, void* out, int n, int k, int lds, int ldo,
                       void* hip_stream);

/*
 * Pairwise intersections of binarised masks:  inter[i, j] = |{p : logit_i[p] > 0 and logit_j[p] > 0}|
 * (sigmoid > 0.5 is logit > 0), exact int32, symmetric, diagonal = areas.  mask_logits [num_masks,
 * mask_pixels] fp32 contiguous.  Replaces the pairwise mask_iou launches of
 * projects/IDOL/idol/models/tracker.py:17-46 (the IoU is (inter + 1e-6) / (area_i + area_j - inter + 1e-6)).
 * Masks become bit words (one ballot per 64 pixels), intersections are popcounts.
 */
size_t vnx_mask_intersections_workspace_bytes(int num_masks, int mask_pixels);
int vnx_mask_intersections(const float* mask_logits, int num_masks, int mask_pixels, int32_t* inter,
                           void* workspace, size_t workspace_bytes, void* hip_stream);

/*
 * IDOL's online tracker with the memory bank on the device: IDOL_Tracker.match + update_memo + memo
 * (projects/IDOL/idol/models/tracker.py:103-298), one call per frame, no host round trip.
 * The fields are the constructor arguments of the reference class (tracker.py:52-98) plus the sizes
 * of the device-resident memory.
 */
typedef struct vnx_tracker_config {
  int capacity;              /* tracklet slots alive at a time, 1..2048 */
  int channels;              /* embedding width, multiple of 4 */
  int memory_len;            /* remembered embeddings per tracklet (long_embed / long_score), 1..16 */
  int memo_tracklet_frames;  /* a tracklet unseen for this many frames is dropped */
  int match_metric;          /* 0 bisoftmax, 1 softmax, 2 cosine */
  int long_match;            /* match against the score-weighted mean of the remembered embeddings */
  int frame_weight;          /* several candidates above 0.5: prefer the longer-lived tracklet */
  int temporal_weight;       /* long_match weights += 1/L, 2/L, ..., 1 (newest) */
  float nms_thr_pre;
  float nms_thr_post;
  float init_score_thr;
  float addnew_score_thr;
  float match_score_thr;
  float memo_momentum;
} vnx_tracker_config;

/*
 * state: a caller-owned device blob of vnx_tracker_state_bytes(cfg) bytes, 16-byte aligned;
 * vnx_tracker_reset empties it (start of a video).  The library keeps no pointer to it.
 * Its first three int32 are {tracklets created so far, tracklets that found no free slot (should stay 0:
 * raise `capacity`), frames processed}.
 */
size_t vnx_tracker_state_bytes(const vnx_tracker_config* cfg);
int vnx_tracker_reset(const vnx_tracker_config* cfg, void* state, void* hip_stream);
size_t vnx_tracker_frame_workspace_bytes(const vnx_tracker_config* cfg, int num_dets, int mask_pixels);
/*
 * One frame.  Detections in descending score order, as the reference's caller passes them:
 *   mask_logits [num_dets, mask_pixels] fp32, embeds [num_dets, channels] fp32 (16-byte aligned),
 *   det_scores [num_dets] fp32 (bboxes[:, 4]), labels [num_dets] int64, num_dets <= 512.
 * ids_out [num_dets] int64, for EVERY input detection: the tracklet id (>= 0), -1 = back-drop,
 * -2 = unassigned duplicate (the reference's values), -3 = removed by the mask NMS (the reference
 * drops those rows from its return value: `valids`, tracker.py:212-219).
 * Enqueues four kernels on hip_stream; no synchronisation, no allocation.  num_dets == 0 is a no-op.
 */
int vnx_tracker_frame(const vnx_tracker_config* cfg, void* state, const float* mask_logits,
                      const float* embeds, const float* det_scores, const int64_t* labels,
                      int num_dets, int mask_pixels, int frame_id, int64_t* ids_out,
                      void* workspace, size_t workspace_bytes, void* hip_stream);

/*
 * y = LayerNorm(x + dropout(r)) over rows of 256 channels, in one pass: the chain that closes every sub-layer of the
 * deformable transformer (projects/SeqFormer/seqformer/models/deformable_transformer.py:201-236,286-385:
 * `src = src + self.dropout1(src2); src = self.norm1(src)`), three ATen launches forward and four backward per site.
 *   x, r, y, z [rows, 256] fp32 contiguous; gamma, beta [256]; stats [rows, 2] = {mean, rstd} per row.
 *   dtype (ABI 14) names the element type of the BRANCH -- r and grad_r: VNX_F32, VNX_BF16 or VNX_F16 -- and nothing else: under
 *   torch.autocast(bfloat16) the Linear or attention output that arrives here is bf16 while the residual stream x, the
 *   LayerNorm and its output are fp32 (the eager chain's types: the sum promotes, autocast runs layer_norm in fp32).
 *   Arithmetic is fp32 either way; grad_r is rounded once on its way out.
 *   z = x + dropout(r) is an OUTPUT the backward needs (r is dead afterwards).  p = drop probability (0 in eval mode),
 *   kept elements are scaled by 1 / (1 - p).  The mask is not stored: element e is kept iff hash(seed, e) >= p * 2^32,
 *   and the backward recomputes it from the same `seed` -- pass the same value to both calls, a fresh one per
 *   forward call.  seed_device (may be null): a 64-bit word in DEVICE memory that the kernels read and mix into
 *   `seed`.  A host integer is baked into a captured hipGraph, so every replay of a captured training step would
 *   drop the same elements; a device word the caller bumps once per step (inside the graph) gives each replay fresh
 *   masks.  It must hold the same value when the matching backward runs.
 *   r_bias (may be null; ABI 11): a [256] vector added to every row of r before the dropout -- the bias of the Linear
 *   that produced r, when that GEMM ran without it -- so that its gradient falls out of this op's backward for free
 *   (grad_r_bias = column sums of grad_r) instead of costing the caller a reduction launch per Linear.
 * Backward: grad_x = d loss / d x, grad_r = d loss / d r (both [rows, 256]), grad_gamma, grad_beta [256] and, when
 * grad_r_bias is not null, grad_r_bias [256] (overwritten, not accumulated; summed in a fixed order).  partial: scratch
 * of vnx_add_dropout_layernorm_partial_bytes() bytes.
 */
size_t vnx_add_dropout_layernorm_partial_bytes(void);
int vnx_add_dropout_layernorm_forward(int dtype, const void* x, const void* r, const void* r_bias, const void* gamma, const void* beta,
                                      void* y, void* z, void* stats, long long rows, int channels, float p, float eps,
                                      unsigned long long seed, const unsigned long long* seed_device,
                                      void* hip_stream);
int vnx_add_dropout_layernorm_backward(int dtype, const void* grad_y, const void* z, const void* stats,
                                       const void* gamma, void* grad_x, void* grad_r, void* grad_gamma, void* grad_beta,
                                       void* grad_r_bias, void* partial, long long rows, int channels, float p, unsigned long long seed,
                                       const unsigned long long* seed_device, void* hip_stream);

/*
 * Bias / activation epilogues of a library GEMM that ran WITHOUT its bias, IN PLACE over h [rows, channels] -- dtype:
 * VNX_F32, or (ABI 14) VNX_BF16 / VNX_F16 for the output of a 16-bit GEMM under autocast: h, grad and grad_h in that type, the bias, its
 * gradient and the partial sums fp32, arithmetic fp32 -- (channels a multiple of 4, <= 4 096), with the bias gradient produced
 * by the backward pass itself:
 *   relu != 0: y = dropout(relu(h + bias)) -- the middle of a transformer FFN
 *     (projects/SeqFormer/seqformer/models/deformable_transformer.py:226-229,330-338: relu, dropout and, in the backward,
 *     masked_scale, threshold_backward and linear1's bias-gradient reduction: five ATen launches and 11.5 passes over the
 *     hidden tensor; here two launches + a small reduction and 2 + 3 passes);
 *   relu == 0 (p must be 0): y = h + bias.
 *   row_zero (may be null): one byte per row; rows with a non-zero byte are written as zeros -- the padding mask of
 *     `value = value_proj(x).masked_fill(mask[..., None], 0)` (projects/SeqFormer/seqformer/models/ops/modules/ms_deform_attn.py:94-96),
 *     which ATen runs as a copy + a fill forward and again backward, plus the bias reduction.
 * bias may be null.  Dropout as in vnx_add_dropout_layernorm_* (hash of (seed, element), seed_device for captured graphs).
 * Backward: grad_h = grad where the row is kept (and, with the ReLU, where y > 0, times 1 / (1 - p): y > 0 <=> the
 * element passed the ReLU and was kept, so y -- the forward's output -- is all it needs; y = null when relu == 0);
 * grad_h may be the same buffer as grad.  grad_bias [channels] = the column sums of grad_h (may be null; partial: scratch
 * of vnx_bias_relu_dropout_partial_bytes(channels) bytes, needed with grad_bias; fixed summation order).
 */
size_t vnx_bias_relu_dropout_partial_bytes(int channels);
int vnx_bias_relu_dropout_forward(int dtype, void* h, const void* bias, const unsigned char* row_zero, long long rows,
                                  int channels, int relu, float p, unsigned long long seed,
                                  const unsigned long long* seed_device, void* hip_stream);
int vnx_bias_relu_dropout_backward(int dtype, const void* grad, const void* y, const unsigned char* row_zero, void* grad_h,
                                   void* grad_bias, void* partial, long long rows, int channels, float p, void* hip_stream);

/*
 * Self-attention over the object queries of a decoder layer (ABI 13) -- what `nn.MultiheadAttention(256, 8, dropout)` does
 * between its input and output projections (projects/SeqFormer/seqformer/models/deformable_transformer.py:286-323 and the
 * `_box` twin; IDOL's decoder layer the same), for ALL heads in one launch forward and one backward:
 *   out[b, i, h] = sum_j dropout(softmax_j((q_i + bq) . (k_j + bk) / sqrt(head_dim)))_ij (v_j + bv)
 * qkv: fp32 [batch * queries][row_stride], a row = q | k | v (channels = heads * head_dim each) of one query as the
 * in-projection GEMMs left them, WITHOUT bias; in_proj_bias [3 * channels] (may be null) is added here.  head_dim must be 32.
 * out [batch, queries, channels] fp32; lse [batch * heads * queries] fp32 (the log-sum-exp of a row's scaled scores: all the
 * backward needs to recompute the probabilities, which are never stored).  Dropout on the probabilities as in
 * vnx_add_dropout_layernorm_* (hash of (seed, element), seed_device for captured graphs; p = 0: none).
 * Backward: grad_qkv [batch * queries][grad_row_stride], the same row layout (gradients of the rows BEFORE the bias; the
 * bias gradient is their column sum), every element written.  No workspace, no atomics, fixed summation order.
 */
int vnx_query_self_attention_forward(int dtype, const void* qkv, const void* in_proj_bias, void* out, void* lse, int batch,
                                     int queries, int heads, int head_dim, int row_stride, float p, unsigned long long seed,
                                     const unsigned long long* seed_device, void* hip_stream);
int vnx_query_self_attention_backward(int dtype, const void* qkv, const void* in_proj_bias, const void* out, const void* lse,
                                      const void* grad_out, void* grad_qkv, int batch, int queries, int heads, int head_dim,
                                      int row_stride, int grad_row_stride, float p, unsigned long long seed,
                                      const unsigned long long* seed_device, void* hip_stream);

/*
 * Two element-wise chains of a decoder layer, one launch forward and one backward each (ABI 13; fp32):
 *  - iterative box refinement (projects/SeqFormer/seqformer/models/deformable_transformer.py:366-380; IDOL :350-365):
 *      out[r] = sigmoid(delta[r] + inverse_sigmoid(reference[r]))        reference rows of 4 components, or
 *      out[r] = sigmoid((delta[r][:2] + inverse_sigmoid(reference[r]), delta[r][2:]))     of 2 (the first layer),
 *    inverse_sigmoid(x) = log(max(clamp(x, 0, 1), eps) / max(1 - clamp(x, 0, 1), eps))  (util/misc.py:493-497).
 *    delta, out [rows, 4]; reference [rows, ref_components].  Backward: grad_delta [rows, 4] and, unless null, grad_reference
 *    [rows, ref_components] (the clamps differentiated as autograd does: the gradient passes where min <= x <= max).
 *  - SeqFormer's temporal weighting of an instance query's frame-level context (:305-312):
 *      weights = softmax(logits, over the frames);  out[n, q, :] = sum_t weights[n, t, q] x[n, t, q, :]
 *    x [clips, frames, queries, channels] (channels a multiple of 4, frames <= 16), logits and weights [clips, frames,
 *    queries], out [clips, queries, channels].  Backward: grad_x (shape of x) and grad_logits from grad_out, x and the weights.
 */
int vnx_refine_boxes_forward(int dtype, const void* delta, const void* reference, void* out, long long rows, int ref_components,
                             float eps, void* hip_stream);
int vnx_refine_boxes_backward(int dtype, const void* grad_out, const void* out, const void* reference, void* grad_delta,
                              void* grad_reference, long long rows, int ref_components, float eps, void* hip_stream);
int vnx_time_weighted_sum_forward(int dtype, const void* x, const void* logits, void* out, void* weights, int clips, int frames,
                                  int queries, int channels, void* hip_stream);
int vnx_time_weighted_sum_backward(int dtype, const void* grad_out, const void* x, const void* weights, void* grad_x,
                                   void* grad_logits, int clips, int frames, int queries, int channels, void* hip_stream);

/*
 * Shifted-window multi-head self-attention of a Swin Transformer block (ABI 16) -- what WindowAttention does between its
 * qkv and proj Linears, with the block's pad / cyclic shift / window partition / reverse / crop around it
 * (projects/SeqFormer/seqformer/backbone/swin.py:129-169, 233-293, 404-452), for ALL windows, heads and images of a block in
 * one launch forward and one backward (+ one small reduction launch):
 *   x_pad = F.pad(tokens to Hp = ceil(H / w) w, Wp = ceil(W / w) w); rolled by (-shift, -shift); windows of w x w;
 *   out_window = softmax(scale q k^T + relative_position_bias + mask) v,  mask = -100.0 between the reference's 3 x 3 shift
 *   regions of the rolled Hp x Wp grid (shift > 0 only); then window reverse, the inverse roll and the crop to H x W.
 * qkv: fp32 [batch * height * width][row_stride], image-row order, a row = q | k | v (channels = heads * head_dim each) of
 * the UNPADDED, UNSHIFTED token as the qkv GEMM left it, WITHOUT bias; qkv_bias [3 * channels] (may be null) is added here,
 * and a padded token's q / k / v IS qkv_bias (the reference pads after norm1): padded tokens are keys and values of every
 * window they fall in; padded query rows are dropped.  bias_table: relative_position_bias_table [(2 w - 1)^2][heads].
 * scale: head_dim^-0.5 or qk_scale.  Limits (VNX_ERR_UNSUPPORTED, before any launch): head_dim 32, 1 <= window <= 12,
 * 1 <= heads <= 48; height, width >= 1 and 0 <= shift < window.  qkv, qkv_bias, out, grad_out, grad_qkv 16-byte aligned.
 * Forward: out [batch * height * width][channels] (real tokens, image-row order: the proj GEMM's input); lse [batch * height
 * * width][heads] fp32, the log-sum-exp of each query row's scores (the backward recomputes the probabilities from it; the
 * scores are never stored).
 * Backward: grad_qkv [batch * height * width][row_stride], the 3 * channels columns of every row written (the gradients
 * BEFORE the bias: the real tokens' share of qkv_bias's gradient is their column sum); grad_bias_table [(2 w - 1)^2][heads];
 * grad_pad_bias [3 * channels] (may be null): the k and v gradients summed over the PADDED tokens, q third zero -- add it to
 * the column sum for qkv_bias's gradient.  partial: caller-allocated scratch of vnx_window_attention_partial_bytes(batch,
 * height, width, heads, window) bytes = batch * windows * heads * ((2 w - 1)^2 + 64) * 4, windows = ceil(height / w) *
 * ceil(width / w).  No atomics: the table and pad-bias gradients are per-workgroup partials reduced in a fixed order,
 * bit-identical run to run.  No allocation, no synchronisation: capturable in a hipGraph.
 * dtype: VNX_F32 (all arrays fp32, as above), or VNX_BF16 (additive: a value that used to be refused; no symbol or signature
 * changed, VNX_ABI_VERSION stays 17) -- the matrix-core instantiation (window_attn_mfma.hip) for the output of a bf16 qkv
 * GEMM under autocast.  VNX_F16 and everything else: VNX_ERR_UNSUPPORTED before any launch.  With VNX_BF16:
 *   - qkv, out, grad_out and grad_qkv are bf16; qkv_bias, bias_table, lse, grad_bias_table, grad_pad_bias and partial stay
 *     fp32 (they are fp32 parameters under autocast); same shapes, same limits, same partial size;
 *   - row_stride is in ELEMENTS and must be a multiple of 8 (16-byte rows; fp32: a multiple of 4), the same five pointers
 *     16-byte aligned;
 *   - bf16 rounding happens at the matrix-core operands -- q, k, v = bf16_rne(float(qkv) + qkv_bias), the probabilities p
 *     for the p v product, dS for the grad_q product, grad_out as it arrives -- and at the final stores of out and
 *     grad_qkv, nowhere else; for grad_v = p^T grad_out and grad_k = dS^T q, which sum over the (possibly few) real query
 *     rows, p and dS enter as two bf16 terms each (the rounded value and the bf16 of what the rounding left): scale (applied to the fp32 score), the bias-table and mask adds,
 *     max / sum / lse, D = rowsum(p o dP), dS = p (dP - D), every accumulator and the table / pad-bias partials are fp32.
 *     The backward does not read `out` (D comes from its own p and dP); pass it all the same.
 *   Forward and backward are bit-identical run to run; no atomics.
 */
size_t vnx_window_attention_partial_bytes(int batch, int height, int width, int heads, int window);
int vnx_window_attention_forward(int dtype, const void* qkv, const void* qkv_bias, const void* bias_table, void* out,
                                 void* lse, int batch, int height, int width, int heads, int head_dim, int row_stride,
                                 int window, int shift, float scale, void* hip_stream);
int vnx_window_attention_backward(int dtype, const void* qkv, const void* qkv_bias, const void* bias_table,
                                  const void* out, const void* lse, const void* grad_out, void* grad_qkv,
                                  void* grad_bias_table, void* grad_pad_bias, void* partial, size_t partial_bytes,
                                  int batch, int height, int width, int heads, int head_dim, int row_stride, int window,
                                  int shift, float scale, void* hip_stream);

/*
 * COCO compressed RLE strings of a batch of masks (ABI 17): what a YTVIS results file holds per (instance, frame), the
 * strings of vnext_amd/utils/ytvis_json.py rle_encode (pycocotools rleEncode + rleToString) byte for byte.  Runs over
 * the column-major mask, the first run counts zeros; from the fourth count on the string holds count[i] - count[i-2];
 * 5-bit groups + 48, 0x20 = more follows, sign termination on 0x10 (at most 7 characters per count).
 * mode VNX_MASK_RLE_LOGITS: input fp32 [masks][height][width] mask logits (4-byte aligned); output pixel (y, x) of the
 *   out_height x out_width mask takes yi = min(floor(y * (image_height / out_height as fp32)), image_height - 1), xi
 *   likewise (ATen "nearest" on the crop), and the bit is v > 0 for v = ATen's align_corners=False bilinear value of the
 *   stride-times upsampled map at (yi, xi) -- sigmoid(v) > 0.5 apart from |v| within fp32 rounding of 0.
 *   1 <= image_height <= height * stride, 1 <= image_width <= width * stride.
 * mode VNX_MASK_RLE_BINARY: input uint8 / bool [masks][out_height][out_width], a pixel is set when its byte is non-zero;
 *   height, width, stride and the image size are not read.
 * Limits (before any launch): out_height * out_width < 2^31 and height * width < 2^31 (VNX_ERR_UNSUPPORTED); null
 * pointers, masks < 0, non-positive sizes, a crop larger than the upsampled map, arena_bytes < 0
 * (VNX_ERR_INVALID_ARGUMENT).  masks == 0 is a no-op.
 * measure: lengths int64 [masks], each mask's string length.  write: offsets int64 [masks], where each string starts in
 * arena (an exclusive scan of the lengths), arena of arena_bytes >= the sum of the lengths; the strings are written
 * without terminators, no byte at or past arena_bytes is written.  One workgroup per mask, no atomics: the output is a
 * function of the input alone.  No workspace, no allocation, no synchronisation: capturable in a hipGraph.
 */
enum {
  VNX_MASK_RLE_LOGITS = 0,
  VNX_MASK_RLE_BINARY = 1
};
int vnx_mask_rle_measure(int mode, const void* input, int masks, int height, int width, int stride, int image_height,
                         int image_width, int out_height, int out_width, void* lengths, void* hip_stream);
int vnx_mask_rle_write(int mode, const void* input, int masks, int height, int width, int stride, int image_height,
                       int image_width, int out_height, int out_width, const void* offsets, void* arena,
                       long long arena_bytes, void* hip_stream);

/*
 * The thresholded result masks themselves, at the output size, from the mask logits in one launch (mask_dense.hip).
 * ADDITIVE: this symbol was added without a change to any existing signature, so VNX_ABI_VERSION stays 17 and a
 * binding written against the earlier ABI 17 keeps working; a binding that needs it looks the symbol up.
 *
 * logits fp32 [masks][height][width] (4-byte aligned).  Output pixel (y, x) of mask m is the bit VNX_MASK_RLE_LOGITS
 * encodes, from the same device code: yi = min(floor(y * (image_height / out_height as fp32)), image_height - 1), xi
 * likewise, v = ATen's align_corners=False bilinear value of the stride-times upsampled map at (yi, xi), bit = v > 0 --
 * sigmoid(v) > 0.5 apart from |v| within fp32 rounding of 0.  The two entry points agree on every pixel.
 * format VNX_MASK_DENSE_U8:   out uint8 [masks][out_height][out_width], 0 or 1; any byte alignment.
 * format VNX_MASK_DENSE_BITS: out [masks][out_height][pitch] bytes, pitch = 8 * ceil(out_width / 64); pixel x is bit
 *   x & 7 of byte x >> 3 of its row (numpy bitorder="little"), padding bits and bytes are zero; out 8-byte aligned.
 * out_bytes: the size of out; every byte of the masks * out_height rows is written, no byte outside them.
 * Before any launch: an unknown format, masks < 0, non-positive sizes, out_bytes < 0 or smaller than the rows, a crop
 * larger than the upsampled map, null or misaligned pointers (VNX_ERR_INVALID_ARGUMENT); height * width >= 2^31
 * (VNX_ERR_UNSUPPORTED).  masks == 0 is a no-op.  The output may exceed 2^31 bytes and masks * out_height any grid
 * dimension.  No atomics: the output is a function of the input alone.  No workspace, no allocation, no
 * synchronisation: capturable in a hipGraph.
 */
enum {
  VNX_MASK_DENSE_U8 = 0,
  VNX_MASK_DENSE_BITS = 1
};
int vnx_mask_dense(int format, const void* logits, int masks, int height, int width, int stride, int image_height,
                   int image_width, int out_height, int out_width, void* out, long long out_bytes, void* hip_stream);

/*
 * Linear sum assignment on the device: SeqFormer's Hungarian matching without a host round trip (lsap.hip).
 * ADDITIVE: these two symbols were added without a change to any existing signature, so VNX_ABI_VERSION stays 17 and a
 * binding written against the earlier ABI 17 keeps working; a binding that needs them looks the symbols up.
 *
 * One launch, one wave64 per problem, shortest augmenting paths with fp64 dual variables on fp32 costs (the algorithm
 * of scipy.optimize.linear_sum_assignment, Crouse 2016): on the same cost matrix the result is scipy's whenever the
 * optimum is unique; ties go to the lower index of the long side.  No atomics, fixed evaluation order: bit-identical
 * run to run.  No workspace, no allocation, no synchronisation: capturable in a hipGraph.
 * A problem with a non-finite cost entry gets -1 in every output slot (scipy raises there; a kernel cannot).
 *
 * vnx_seqformer_match: layers x clips problems, the cost block of each computed in the kernel from
 *   logits [layers][clips][queries][classes] fp32, boxes [layers][clips][frames][queries][4] fp32 (cx, cy, w, h),
 *   labels int64 [targets_total] and target_boxes fp32 [targets_total][frames][4] (the clips' targets back to back),
 *   offsets int32 [clips + 1] (clip i owns targets offsets[i] .. offsets[i + 1] - 1), as
 *     cost_bbox * || box - target ||_2 over the clip's frames * 4 coordinates
 *     + cost_class * (pos - neg), the focal terms with alpha 0.25, gamma 2 and 1e-8 inside the logs
 *     + cost_giou * (- mean over frames of GIoU), the targets clamped to [1e-7, 1] for this term only, 1e-7 on the hull
 *   (HungarianMatcher.cost of SeqFormer, matcher.py:53-96).  Every target is assigned to one query.
 *   Outputs int64 [layers][targets_total]: at a clip's offset its matched queries in ascending order (query_index) and
 *   the target of each, counted from the clip's first (target_index) -- linear_sum_assignment's order with queries as
 *   rows.  cost_out (may be null): fp32 [layers][clips][queries][targets_total]; the kernel writes the block it solved
 *   (the columns of the clip's own targets) and leaves the other columns alone.
 *   targets_max: an upper bound of the largest clip's target count, known on the host; it sizes the LDS.  A clip with
 *   more targets than that, or a label outside [0, classes), gets -1.  VNX_ERR_UNSUPPORTED before any launch when
 *   targets_max > queries or queries * targets_max * 4 + queries * 28 + targets_max * 12 bytes exceed 160 KB
 *   (300 queries: 128 targets) -- the caller then matches on the host.  targets_total == 0 is a no-op.
 * vnx_lsap_solve: batch problems on cost matrices in device memory, element (b, r, c) at
 *   cost[b * batch_stride + r * row_stride + c * col_stride] (fp32, strides in elements), minimised, or maximised when
 *   maximize != 0.  Outputs int64 [batch][min(rows, cols)]: row_index ascending and col_index of each -- what
 *   linear_sum_assignment returns.  The same LDS limit on min(rows, cols) x max(rows, cols).
 */
int vnx_seqformer_match(const void* logits, const void* boxes, const void* labels, const void* target_boxes,
                        const void* offsets, int layers, int clips, int frames, int queries, int classes,
                        int targets_total, int targets_max, float cost_class, float cost_bbox, float cost_giou,
                        void* query_index, void* target_index, void* cost_out, void* hip_stream);
int vnx_lsap_solve(const void* cost, int batch, int rows, int cols, long long batch_stride, long long row_stride,
                   long long col_stride, int maximize, void* row_index, void* col_index, void* hip_stream);

/*
 * The mask losses of both criteria -- sigmoid focal + dice over the matched instances' mask logits -- in one pass each
 * way, the ground truth read in place (mask_loss.hip).  ADDITIVE: two symbols and one struct, no existing signature
 * changed, so VNX_ABI_VERSION stays 17; a binding that needs them looks the symbols up.
 *
 *   logits fp32 [rows][frames][height][width] contiguous (one row = one matched instance of one decoder layer),
 *   row_gt int64 [rows] on the device: the row's target, counted over the clips' targets laid back to back,
 *   clips: per clip a bool / uint8 device tensor [n_i][frames][H_i][W_i] at image resolution, contiguous (0 / non-zero).
 * The target of logit (r, f, y, x) is  masks[row_gt[r]][f][y * stride + stride / 2][x * stride + stride / 2]  where that
 * pixel exists and 0 where it does not (segmentation_condInst.py / deformable_detr.py: slice [s/2::s], zero-pad to the
 * canvas).  A row whose row_gt is outside [0, total) has target 0 everywhere.  With p = sigmoid(logit):
 *   focal[r] = mean over the row of  alpha_t * ce * (1 - p_t)^gamma    (sigmoid_focal_loss before .sum() / num_boxes;
 *                                                                       alpha < 0: no alpha_t, as there)
 *   dice[r]  = 1 - (2 sum(p t) + 1) / (sum(p) + sum(t) + 1)            (dice_loss likewise)
 *   row_sums [rows][3] = {sum(p t), sum(p), sum(t)}: what the backward needs; nothing of the logits' size is kept.
 * vnx_mask_loss_clips is read on the host during the call and travels to the kernels by value: nothing is uploaded and
 * the library keeps no pointer to it.  Clip i owns targets first[i] .. first[i + 1] - 1 (the last one up to total - 1);
 * first[0] = 0; a clip without targets may have a null pointer.
 * Forward: a workgroup sums one piece of VNX_MASK_LOSS_PIECE logits of a row into partial [rows][pieces][4] fp32
 * (pieces = ceil(frames * height * width / VNX_MASK_LOSS_PIECE); caller-owned, 16-byte aligned, need not be zeroed), a
 * second small launch adds a row's pieces in a fixed order.  Backward: one element-wise launch,
 *   grad_logits = grad_focal[r] / M * dfocal/dlogit + grad_dice[r] * ddice/dp * p (1 - p),
 * recomputed from logits and masks.  No atomics: bit-identical run to run.  No allocation, no synchronisation:
 * capturable in a hipGraph.  rows == 0 is a no-op.  Any height, width, H_i, W_i and stride >= 1; 16-byte loads where
 * width % 4 == 0 (logits) and stride == 4 with W_i % 16 == 0 (masks).
 */
#define VNX_MASK_LOSS_MAX_CLIPS 16
#define VNX_MASK_LOSS_PIECE 4096
typedef struct vnx_mask_loss_clips {
  const void* masks[VNX_MASK_LOSS_MAX_CLIPS]; /* device pointer of clip i's [n_i][frames][H_i][W_i] bytes */
  int height[VNX_MASK_LOSS_MAX_CLIPS];        /* H_i */
  int width[VNX_MASK_LOSS_MAX_CLIPS];         /* W_i */
  int first[VNX_MASK_LOSS_MAX_CLIPS];         /* index of clip i's first target among all targets */
  int count;                                  /* clips in use, 0..VNX_MASK_LOSS_MAX_CLIPS */
  int total;                                  /* targets of all clips */
} vnx_mask_loss_clips;
int vnx_mask_loss_forward(const void* logits, const vnx_mask_loss_clips* clips, const void* row_gt, int rows, int frames,
                          int height, int width, int stride, float alpha, float gamma, void* partial,
                          size_t partial_bytes, void* focal, void* dice, void* row_sums, void* hip_stream);
int vnx_mask_loss_backward(const void* logits, const vnx_mask_loss_clips* clips, const void* row_gt, int rows, int frames,
                           int height, int width, int stride, float alpha, float gamma, const void* row_sums,
                           const void* grad_focal, const void* grad_dice, void* grad_logits, void* hip_stream);

/*
 * The class and box losses of both criteria for every decoder layer at once (set_loss.hip): the sigmoid focal loss over
 * all logits against the one-hot target the pair list implies, the matched boxes' L1 and GIoU losses, and the count of
 * matched queries whose argmax is their label.  ADDITIVE: two symbols, no existing signature changed, so VNX_ABI_VERSION
 * stays 17; a binding that needs them looks the symbols up.
 *
 *   logits fp32 [layers][clips][queries][classes], boxes fp32 [layers][clips][frames][queries][4] (cx, cy, w, h), contiguous;
 *   lay, clip, qry, tgt int64 [pairs] on the device: query qry[r] of (layer lay[r], clip clip[r]) is matched to target
 *     tgt[r], counted over the clips' targets laid back to back;
 *   labels int64 [targets_total], target_boxes fp32 [targets_total][frames][4].
 * out fp32 [layers][4], per layer:
 *   [0] sum over (clip, query, class) of  alpha_t * ce * (1 - p_t)^2  (gamma = 2; alpha < 0: no alpha_t), the target 1 at
 *       (clip[r], qry[r], labels[tgt[r]]) of the layer's pairs and 0 elsewhere -- never materialised;
 *   [1] sum over the layer's pairs, frames and coordinates of |box - target box|;
 *   [2] sum over the layer's pairs and frames of 1 - GIoU of the xyxy forms: intersection only where both extents are
 *       positive, 1e-7 added to union and hull in the denominators, hull extents not clamped;
 *   [3] the number of the layer's pairs whose first maximum over the classes is labels[tgt[r]] (not differentiable).
 * PRECONDITIONS: a (lay, clip, qry) triple appears at most once.  A pair with a negative qry or tgt, or any index outside
 * its array, contributes nothing; a label outside [0, classes) sets no target and scores no hit.
 * Forward: a workgroup owns one piece of one (layer, clip): rows = clamp(VNX_SET_LOSS_PIECE / classes, 1,
 * VNX_SET_LOSS_MAX_ROWS) consecutive queries; it writes one partial [4]; partial fp32 [layers][clips * pieces][4] with
 * pieces = ceil(queries / rows) is caller-owned, 16-byte aligned like out, and need not be zeroed.  A second small launch
 * adds a layer's partials in a fixed order.  Backward: ONE launch writes every element of grad_logits (= grad_out[l][0] *
 * dfocal/dlogit) and of grad_boxes (grad_out[l][1] * sign(box - target) + grad_out[l][2] * d(1 - GIoU)/dbox at matched
 * (layer, clip, frame, query), 0 elsewhere), recomputed from the inputs; grad_out [layers][4] fp32, its column 3 ignored.
 * At an exact tie a maximum / minimum splits its gradient evenly between its operands, and sign(0) = 0, as ATen does.
 * No atomics: bit-identical run to run.  No allocation, no synchronisation: capturable in a hipGraph.  pairs == 0 is valid
 * (the pair pointers may then be null): column 0 and grad_logits are computed, the rest is 0.
 */
#define VNX_SET_LOSS_PIECE 4096
#define VNX_SET_LOSS_MAX_ROWS 1024
int vnx_set_loss_forward(const void* logits, const void* boxes, const void* lay, const void* clip, const void* qry,
                         const void* tgt, const void* labels, const void* target_boxes, int layers, int clips, int frames,
                         int queries, int classes, int pairs, int targets_total, float alpha, void* partial,
                         size_t partial_bytes, void* out, void* hip_stream);
int vnx_set_loss_backward(const void* logits, const void* boxes, const void* lay, const void* clip, const void* qry,
                          const void* tgt, const void* labels, const void* target_boxes, int layers, int clips, int frames,
                          int queries, int classes, int pairs, int targets_total, float alpha, const void* grad_out,
                          void* grad_logits, void* grad_boxes, void* hip_stream);

/*
 * IDOL's simOTA matching and the contrastive positive / negative sets on the device (ota_match.hip).  ADDITIVE: three
 * symbols, no existing signature changed, so VNX_ABI_VERSION stays 17; a binding that needs them looks the symbols up.
 *
 * One launch, one workgroup (four wave64) per problem; det_problems detection problems first, then ref_problems
 * selection problems.  All floating-point inputs fp32 and contiguous:
 *   det_prob [det_problems][queries][classes], ref_prob [ref_problems][queries][classes]: class PROBABILITIES (the
 *     caller applies the sigmoid, in the precision its host path does),
 *   det_boxes [det_problems][queries][4], ref_boxes [ref_problems][queries][4]: (cx, cy, w, h),
 *   target_boxes [targets_total][4] and labels int64 [targets_total]: the targets of every image back to back, the key
 *     images' first; valid uint8 [targets_total - valid_first]: the flag of target t at valid[t - valid_first] (read by
 *     selection problems only, whose targets start at valid_first or later),
 *   problems int32 [det_problems + ref_problems][2]: (first target, target count) of each problem.
 * A detection problem is the reference's simOTA matching of one (decoder layer, key image): cost = focal class term
 * (alpha 0.25, gamma 2, 1e-8 inside the logs) + 3 * -GIoU (1e-7 on the hull) + 100 where the query centre is not in (box
 * AND centre region, radius 2.5 / 32) + 10000 where it is in no box and no centre region; k of a target = the sum of its
 * 10 largest IoUs, truncated, at least 1; the target takes its k cheapest queries; a query claimed by several targets
 * keeps the cheapest; a target left without a query takes its cheapest one after 100000 was added to the rows already
 * matched (in place, fp32), repeated until every target has a query.  A selection problem does the same on the targets
 * whose valid flag is set, then a second time with the 100 largest IoUs on the cost the first pass left.  Equal values: the
 * lower index.  No atomics, fixed evaluation order: bit-identical run to run.  No workspace, no allocation, no
 * synchronisation.  A call that needs more than 64 KB of LDS (41 targets or more at 300 queries) raises the kernel's
 * dynamic-LDS limit with hipFuncSetAttribute, once per device, the first time such a call is made there: make that call
 * once outside a stream capture.
 * out int32 [det_problems + ref_problems][out_stride], out_stride >= vnx_idol_match_out_words(targets_max, queries):
 *   [0] status: 0 solved; 1 a non-finite cost or IoU; 2 the repair loop reached its bound (count + 8 rounds); 3 a label
 *       outside [0, classes) or a (first, count) outside the arrays / above targets_max.  Not 0: no result, match on the host.
 *   [1] n: the problem's targets (detection) / valid targets (selection)
 *   detection: [2 .. 2 + queries) the lowest target assigned to the query or -1; then n words: the cheapest query
 *     assigned to each target
 *   selection: [2 .. 2 + n) the valid targets, counted from the problem's first; from word 2 + targets_max on, bytes
 *     [targets_max][queries]: bit 0 = assigned by the first pass (positive), bit 1 = NOT assigned by the second (negative)
 *   the rest of the stride is filled (-1 in index fields, 0 in the bytes).
 * targets_max: an upper bound of the largest problem's count, known on the host; it sizes the LDS.  VNX_ERR_UNSUPPORTED
 * before any launch -- the caller then matches on the host -- when
 *   - with Qp = queries rounded up to a multiple of 4, targets_max * (5 Qp + 8) + 9 Qp + 4 queries + 576 bytes exceed
 *     163 840 (the 160 KB of a CU).  vnx_idol_match_max_targets(queries) is the largest targets_max that fits: 105 at
 *     300 queries (105 * 1508 + 4476 = 162 816 bytes; 106 would need 164 324);
 *   - the device refuses the dynamic-LDS limit such a call needs;
 *   - there are targets and queries < 10 (< 100 with selection problems).
 */
int vnx_idol_match_max_targets(int queries);
int vnx_idol_match_out_words(int targets_max, int queries);
int vnx_idol_match(const void* det_prob, const void* det_boxes, const void* ref_prob, const void* ref_boxes,
                   const void* target_boxes, const void* labels, const void* valid, const void* problems,
                   int det_problems, int ref_problems, int queries, int classes, int targets_total, int valid_first,
                   int targets_max, void* out, int out_stride, void* hip_stream);

/*
 * IDOL's re-identification losses -- the contrastive loss and the auxiliary cosine loss -- of every instance of every image
 * of a step (reid_loss.hip).  ADDITIVE: two symbols, no existing signature changed, so VNX_ABI_VERSION stays 17; a binding
 * that needs them looks the symbols up.
 *
 *   key fp32 [images][key_rows][channels], ref fp32 [images][ref_rows][channels]: rows contiguous, image i at
 *     base + i * image_stride ELEMENTS (the two interleaved halves of one [2 images, rows, channels] tensor are read in place);
 *   img, key_query int32 [instances] on the device: instance j compares row key_query[j] of key image img[j] with every row
 *     of reference image img[j]; img is non-decreasing;
 *   flags uint8 [instances][ref_rows]: bit 0 positive (P), bit 1 negative (N), bit 2 aux sample (A).
 * With k the key row, dot_r = <ref_r, k> and cos_r = dot_r / (max(|ref_r|, 1e-12) * max(|k|, 1e-12)):
 *   out[j][0] = softplus(logsumexp_{r in N} dot_r + logsumexp_{r in P} -dot_r), exactly 0 when P or N is empty (stable: the
 *               maxima are taken out first);
 *   out[j][1] = sum_{r in A} (cos_r - [r in P])^2 / max(|A|, 1).
 * An instance whose img is outside [0, images) or whose key_query is outside [0, key_rows) reads nothing, gets (0, 0) and
 * contributes no gradient.
 * Forward: ONE launch, a workgroup per instance; it also leaves what the backward needs: dot fp32 [instances][ref_rows],
 * ref_norm fp32 [instances][ref_rows] (|ref_r|) and stats fp32 [instances][8] = {|k|, max_N, sum_N, max_P, sum_P, |A|,
 * P and N both non-empty, 0} -- caller-owned, need not be zeroed; nothing of the embeddings' size.  instances == 0: no launch.
 * Backward: TWO launches write every element of grad_ref [images][ref_rows][channels] and grad_key [images][key_rows][channels]
 * (contiguous; zero where no instance reaches), grad_out fp32 [instances][2]; two instances that share a key row add, in list
 * order.  The clamp of the norms is differentiated as a clamp_min.  No atomics, no memset: bit-identical run to run.  No
 * allocation, no synchronisation: capturable in a hipGraph.  instances == 0 is valid: both gradients are zero.
 * VNX_ERR_UNSUPPORTED, nothing launched: channels, key_rows or images < 1, ref_rows outside [1, VNX_REID_LOSS_MAX_ROWS].
 * 16-byte loads where channels % 4 == 0 and bases and strides are 16-byte aligned; any channel count otherwise.
 */
#define VNX_REID_LOSS_MAX_ROWS 1024
int vnx_reid_loss_forward(const void* key, long long key_image_stride, int key_rows, const void* ref,
                          long long ref_image_stride, int ref_rows, int channels, int images, const void* img,
                          const void* key_query, const void* flags, int instances, void* out, void* dot, void* ref_norm,
                          void* stats, void* hip_stream);
int vnx_reid_loss_backward(const void* key, long long key_image_stride, int key_rows, const void* ref,
                           long long ref_image_stride, int ref_rows, int channels, int images, const void* img,
                           const void* key_query, const void* flags, int instances, const void* dot, const void* ref_norm,
                           const void* stats, const void* grad_out, void* grad_key, void* grad_ref, void* hip_stream);

/*
 * The element-wise glue of a Swin stage (swin_glue.hip): stochastic depth + residual add + the pre-norm LayerNorm of the
 * next branch, and PatchMerging's pad + 2x2 gather + LayerNorm.  ADDITIVE: five symbols, no existing signature changed, so
 * VNX_ABI_VERSION stays 17; a binding that needs them looks the symbols up.
 *
 * Residual + LayerNorm.  Rows of `channels` values, contiguous; sample b owns rows [b, b + 1) * rows_per_sample:
 *   y[r] = x[r] + scale[b] * a[r]                        scale fp32 [samples] on the device, or null = 1
 *   n[r] = LayerNorm(y[r]; gamma, beta, eps)             stats fp32 [rows][2] = (mean, rstd), written with n
 * a null: y = x and y is not written (pass y null): a plain LayerNorm.  gamma null: no n, no stats (pass beta, n, stats
 * null): a plain scaled add.  Both null is an error.  A sample whose scale is 0 does not read its branch: its y equals x bit
 * for bit, and the backward writes exactly 0 into its grad_a.
 * Types (x_dtype names x, y, grad_y, grad_x; a_dtype a and grad_a; n_dtype n and grad_n): exactly
 *   (VNX_F32, VNX_F32, VNX_F32), (VNX_F32, VNX_BF16, VNX_BF16), (VNX_BF16, VNX_BF16, VNX_BF16)
 * -- what the library chain produces without autocast, under bf16 autocast on an fp32 stream, and on a bf16 stream.  Pass
 * the triple also where a or n is null.  gamma, beta, scale, stats and all arithmetic are fp32; n is the LayerNorm of y as
 * STORED (a bf16 stream: of the rounded y), which is what the backward recomputes xhat from.
 * Backward: grad_y and grad_n may each be null (= zero; grad_n must be null where gamma is).  g = grad_y +
 * LayerNormBackward(grad_n; y, stats, gamma);  grad_x = g;  grad_a = scale[b] * g (null: not wanted).  Every element of
 * grad_x and grad_a is written -- no memset, no accumulation.  With gamma: grad_gamma and grad_beta fp32 [channels] leave
 * as per-workgroup partial rows in `partial` (at least vnx_swin_glue_partial_bytes(rows, channels) bytes, sized by the
 * launch and not by a maximum; need not be zeroed), which a finishing launch adds in a fixed order.  No atomics:
 * bit-identical run to run.  rows == 0 is valid (the parameter gradients are zero).
 *
 * PatchMerging gather + LayerNorm.  x [batch][height][width][channels] (x_dtype), n [batch][ceil(height / 2) *
 * ceil(width / 2)][4 * channels] (n_dtype): the row of output token (i, j) is x[2i][2j] | x[2i+1][2j] | x[2i][2j+1] |
 * x[2i+1][2j+1], a position outside the grid contributing zeros (the reference's pad of an odd height or width), normalised
 * over 4 * channels; stats fp32 [output rows][2].  No padded copy, no concatenated copy.  Types (x_dtype, n_dtype):
 * (VNX_F32, VNX_F32), (VNX_F32, VNX_BF16), (VNX_BF16, VNX_BF16).  Backward: every element of grad_x (x's shape and type)
 * is written by the one output row that owns it; grad_gamma / grad_beta fp32 [4 * channels] as above, `partial` at least
 * vnx_swin_glue_partial_bytes(output rows, 4 * channels) bytes.
 *
 * VNX_ERR_UNSUPPORTED before any launch: another type triple; a row width (channels; 4 * channels of the merge) outside
 * [32, 3072] or no multiple of 8; a pointer that is not 16-byte aligned.  All accesses are 16 bytes wide.  One launch
 * forward; backward one launch, two with a LayerNorm.  No allocation, no synchronisation: capturable in a hipGraph.
 */
size_t vnx_swin_glue_partial_bytes(long long rows, int channels);
int vnx_swin_residual_norm_forward(int x_dtype, int a_dtype, int n_dtype, const void* x, const void* a, const void* scale,
                                   const void* gamma, const void* beta, void* y, void* n, void* stats, long long rows,
                                   int channels, long long rows_per_sample, float eps, void* hip_stream);
int vnx_swin_residual_norm_backward(int x_dtype, int a_dtype, int n_dtype, const void* grad_y, const void* grad_n,
                                    const void* y, const void* stats, const void* gamma, const void* scale, void* grad_x,
                                    void* grad_a, void* grad_gamma, void* grad_beta, void* partial, size_t partial_bytes,
                                    long long rows, int channels, long long rows_per_sample, void* hip_stream);
int vnx_swin_merge_norm_forward(int x_dtype, int n_dtype, const void* x, const void* gamma, const void* beta, void* n,
                                void* stats, int batch, int height, int width, int channels, float eps, void* hip_stream);
int vnx_swin_merge_norm_backward(int x_dtype, int n_dtype, const void* grad_n, const void* x, const void* stats,
                                 const void* gamma, void* grad_x, void* grad_gamma, void* grad_beta, void* partial,
                                 size_t partial_bytes, int batch, int height, int width, int channels, void* hip_stream);

/*
 * The element-wise glue of the ResNet trunk (resnet_glue.hip): what follows a convolution whose frozen batch norm is folded
 * into its filters -- the shift, the ReLU, the residual add; the stem's shift, ReLU and max-pool.  ADDITIVE: three symbols, no
 * existing signature changed, so VNX_ABI_VERSION stays 17; a binding that needs them looks the symbols up.
 *
 * dtype names every array of a call, the shifts included: VNX_F32, VNX_BF16 or VNX_F16.  layout: VNX_LAYOUT_NCHW (the channel
 * of flat element i is (i / hw) % c) or VNX_LAYOUT_NHWC (i % c); arrays are dense in that layout.  All sizes are 64-bit and
 * so is every index; a size above 2^31 or more than 2^46 elements is VNX_ERR_INVALID_ARGUMENT.
 *
 * vnx_conv_epilogue_forward:  y <- relu((y + bias[ch]) + (res + res_bias[ch])), in place on the convolution's output y
 * [n][c][hw].  res (y's shape) and res_bias [c] may each be null (res_bias only with res): without res it is the shift + ReLU
 * after a block's first two convolutions, with res the block's tail -- an identity shortcut passes no res_bias, a projection
 * shortcut the raw output of its convolution and that convolution's shift.  res is only read and must not overlap y.  fp32:
 * the additions run in exactly that order, so the result is the eager chain's bit for bit.  16-bit: operands widened, the
 * sum formed in fp32 and rounded ONCE.  NaN and +-inf propagate as in clamp_min.  16-byte accesses where the pointers are
 * 16-byte aligned; the shift is one value per access where hw (NCHW) is a multiple of the 16-byte width, a 16-byte load
 * where c (NHWC) is, and looked up element by element otherwise (plane heads and tails, an odd c); an unaligned pointer and
 * the array's tail take element accesses.
 *
 * vnx_conv_epilogue_backward:  grad_in[i] = y[i] > 0 ? grad_y[i] : 0 over `count` elements (y: the forward's result, all
 * three arrays in one layout).  The one tensor is the gradient of the convolution's output AND of res; the shifts are
 * constants of a frozen norm.
 *
 * vnx_stem_pool_forward:  out = max_pool2d(relu(conv_out + bias[ch]), kernel 3, stride 2, padding 1): conv_out [n][c][h][w]
 * (or [n][h][w][c]) is read once and only out [n][c][oh][ow], oh = (h - 1) / 2 + 1, ow = (w - 1) / 2 + 1, is written.  A NaN
 * in a window is that window's result, as in ATen.  16-bit: the rounding of the fp32 result.  Forward only.
 *
 * One launch each.  No allocation, no synchronisation: capturable in a hipGraph.
 */
#define VNX_LAYOUT_NCHW 0
#define VNX_LAYOUT_NHWC 1
int vnx_conv_epilogue_forward(int dtype, int layout, void* y, const void* bias, const void* res, const void* res_bias,
                              long long n, long long c, long long hw, void* hip_stream);
int vnx_conv_epilogue_backward(int dtype, const void* grad_y, const void* y, void* grad_in, long long count,
                               void* hip_stream);
int vnx_stem_pool_forward(int dtype, int layout, const void* conv_out, const void* bias, void* out, long long n, long long c,
                          long long h, long long w, void* hip_stream);

/*
 * Detection selection of a batch of images (det_select.hip): best class per query, score threshold, class-aware greedy
 * box NMS and the top-k over (kept query, class) -- IDOL's per-frame candidate selection and its COCO-pretrain inference.
 * ADDITIVE: two symbols, no existing signature changed, so VNX_ABI_VERSION stays 17; a binding that needs them looks the
 * symbols up.
 *
 * One launch, one workgroup (four wave64) per image.  logits fp32 [batch][queries][classes] (pre-sigmoid), boxes fp32
 * [batch][queries][4] = (cx, cy, w, h), both contiguous, boxes 16-byte aligned.  Per image:
 *   1. every query's label = the first argmax of its logits (equal maxima: the lowest class);
 *   2. candidates = the queries with 1 / (1 + expf(-max logit)) > score_thr in fp32.  A negative score_thr admits every
 *      query.  No candidate: the result is the single best query (the lowest index among equals) and no NMS runs;
 *   3. the candidates in (max logit descending, query index ascending) order -- the logit, not its sigmoid;
 *   4. greedy NMS in that order: a live candidate removes every later one with the same label and IoU > iou_thr; a removed
 *      one removes nothing.  xyxy = c -+ 0.5 * wh, area = (x1 - x0) * (y1 - y0), IoU = inter / (area_a + area_b - inter)
 *      with inter the product of the clamped overlaps: fp32, no contraction, IEEE division -- the comparison agrees bit for
 *      bit with the same expression on the host; 0 / 0 compares false;
 *   5. topk > 0: the min(topk, kept * classes) largest logits of the kept queries, in (logit descending, flat index
 *      position_in_kept_order * classes + class ascending) order.
 * Scores are not produced: a caller forms them from the logits it holds.  Integer LDS counters only, every global result a
 * plain store: bit-identical run to run.  No workspace, no allocation, no synchronisation.  A call with more than 64 KB of
 * LDS (queries above 720) raises the kernel's dynamic-LDS limit with hipFuncSetAttribute, once per device, the first time
 * such a call is made there: make that call once outside a stream capture.
 * out int32 [batch][out_stride], out_stride >= vnx_det_select_out_words(queries, topk) = 4 + 2 queries + 2 topk:
 *   [0] status: 0 ok; 1 a non-finite logit or box in this image: nothing selected, [1] = [2] = 0, every list -1
 *   [1] kept queries   [2] top-k entries   [3] 0
 *   [4, 4 + queries) the kept queries in NMS order, then -1
 *   [4 + queries, 4 + 2 queries) every query's label
 *   then topk pairs (query, class), the unused ones -1.  Words of the stride beyond that are not written.
 * batch == 0: VNX_OK, no launch.  VNX_ERR_UNSUPPORTED before any launch, the output untouched: queries above what the LDS
 * of a CU holds (1280: 256 W (W + 1) + 40 queries + 8 W + 3136 bytes with W = ceil(queries / 64), against 163 840),
 * classes above 4096, queries * classes >= 2^24, topk above 256, or a device that refuses the dynamic-LDS limit.
 */
int vnx_det_select_out_words(int queries, int topk);
int vnx_det_select(const void* logits, const void* boxes, int batch, int queries, int classes, float score_thr,
                   float iou_thr, int topk, void* out, int out_stride, void* hip_stream);

/*
 * SeqFormer's clip matching with the video's state in device memory (clip_link.hip): what `Videos` of
 * models/clip_matching.py does per clip -- sIoU of the incoming clip's masks against the stored clips on the shared frames,
 * the mean over the clips that hold a track, threshold 0.01, assignment, new tracks for the unmatched, the running sums of
 * the result -- in three launches on the caller's stream, with no copy to the host.  ADDITIVE: five symbols, no existing
 * signature changed, so VNX_ABI_VERSION stays 17; a binding that needs them looks the symbols up.
 *
 * vnx_clip_link_config describes one video's state; the same values go to every call on that state.
 *   ring: stored clips kept = frames of a clip at most (the model's CLIP_LENGTH), 1..VNX_CLIP_LINK_MAX_FRAMES
 *   max_instances: instances of a clip at most, 1..VNX_CLIP_LINK_MAX_INSTANCES     pixels: H * W of a mask
 *   video_length: frames of the video     classes: columns of cls_probs
 *   capacity: tracks the state has room for.  An instance that finds none gets id -1 and raises the second counter.
 * Beyond the two limits: VNX_ERR_UNSUPPORTED (vnx_clip_link_state_bytes / _workspace_bytes: 0) with vnx_last_error naming
 * them, nothing launched.
 * state: vnx_clip_link_state_bytes(cfg) bytes of device memory, 16-byte aligned, zeroed by vnx_clip_link_reset (a memset
 * on the stream).  Its first three int32 are counters: tracks opened, instances that found no free track, clips taken.
 *
 * vnx_clip_link_update: one clip.  mask_logits fp32 [num_instances][plan->frames][pixels], cls_probs fp32
 * [num_instances][classes], ids_out int64 [num_instances] (the track of every instance, in input order), all on the
 * device and contiguous.  The frame lists stay with the host, which owns them; vnx_clip_link_plan is read on the host
 * during the call and travels to the kernels by value:
 *   frames, frame_index[]: the incoming clip's frames in the video (distinct, inside video_length)
 *   write_slot: the ring slot that stores the incoming clip
 *   slots, slot[], pairs[], stored_pos[][], incoming_pos[][]: the stored clips that share a frame with the incoming one,
 *     OLDEST FIRST (the order their scores are added in), and for each the shared frames as (position in the stored clip,
 *     position in the incoming clip).  A listed slot that holds an empty clip does not count, as in `Videos.get_siou`.
 * num_instances == 0 is legal: the clip is stored empty.  num_instances above max_instances or frames above ring:
 * VNX_ERR_UNSUPPORTED before any launch, the state untouched.  workspace: vnx_clip_link_workspace_bytes(cfg) bytes,
 * 16-byte aligned, scratch of this call.  No atomics and every sum in a fixed order: bit-identical run to run.
 *
 * vnx_clip_link_result: cls_out fp32 [num_tracks][classes] = cls / in_clips and logits_out fp32
 * [num_tracks][video_length][pixels] = total / seen of the first num_tracks tracks; 0 / 0 = NaN where no clip of a track
 * covers a frame, as in the reference.
 */
#define VNX_CLIP_LINK_MAX_INSTANCES 16
#define VNX_CLIP_LINK_MAX_FRAMES 8
typedef struct vnx_clip_link_config {
  int ring, max_instances, pixels, video_length, classes, capacity;
} vnx_clip_link_config;
typedef struct vnx_clip_link_plan {
  int frames;
  int frame_index[VNX_CLIP_LINK_MAX_FRAMES];
  int write_slot;
  int slots;
  int slot[VNX_CLIP_LINK_MAX_FRAMES];
  int pairs[VNX_CLIP_LINK_MAX_FRAMES];
  unsigned char stored_pos[VNX_CLIP_LINK_MAX_FRAMES][VNX_CLIP_LINK_MAX_FRAMES];
  unsigned char incoming_pos[VNX_CLIP_LINK_MAX_FRAMES][VNX_CLIP_LINK_MAX_FRAMES];
} vnx_clip_link_plan;
size_t vnx_clip_link_state_bytes(const vnx_clip_link_config* cfg);
size_t vnx_clip_link_workspace_bytes(const vnx_clip_link_config* cfg);
int vnx_clip_link_reset(const vnx_clip_link_config* cfg, void* state, void* hip_stream);
int vnx_clip_link_update(const vnx_clip_link_config* cfg, void* state, const void* mask_logits, const void* cls_probs,
                         const vnx_clip_link_plan* plan, int num_instances, void* ids_out, void* workspace,
                         size_t workspace_bytes, void* hip_stream);
int vnx_clip_link_result(const vnx_clip_link_config* cfg, const void* state, int num_tracks, void* cls_out,
                         void* logits_out, void* hip_stream);

/*
 * uint8 frames to network inputs (ingest.hip): normalise + pad + padding mask in one launch, and the per-level padding masks
 * and sine positions of the padded batch in one more.  ADDITIVE: two symbols, no existing signature changed, so
 * VNX_ABI_VERSION stays 17; a binding that needs them looks the symbols up.
 *
 * pixels: uint8 device buffer of pixel_bytes bytes, 4-byte aligned, holding each frame's three CHW planes back to back
 * (R plane, G plane, B plane of h x w bytes each).  table: int32 device [batch][3] = {byte offset of the frame's first plane
 * inside pixels (any value: no alignment asked), h, w}.  The geometry is read from memory by the kernels, not by the host:
 * a captured launch replays on new pixels AND new frame sizes; batch, height, width, the layout, mean / std, the level
 * sizes, num_pos_feats and the two tables are baked in.  A row that does not describe planes inside pixels (a negative
 * value, h > height, w > width, offset + 3 h w > pixel_bytes) is taken as an empty frame (all padding) by
 * vnx_ingest_frames; no read leaves the buffer whatever the table holds.
 *
 * vnx_ingest_frames: height, width multiples of 32.  x fp32 [batch][3][height][width] (channels_last 0) or
 * [batch][height][width][3] (channels_last 1), mask uint8 / bool [batch][height][width], both 16-byte aligned.  Inside a
 * frame x = (float(u) - mean[c]) / std[c] -- an IEEE subtract, then a correctly rounded IEEE divide -- and mask = 0; outside
 * x = 0 and mask = 1.  Every element of both is written: no memset is needed before the call.
 *
 * vnx_ingest_levels: for num_levels <= VNX_INGEST_MAX_LEVELS levels, level_sizes = host int [num_levels][2] = (h_l, w_l):
 *   masks[l] uint8 / bool [batch][h_l][w_l]: torch's nearest resize of the padding mask (source index
 *     min(int(floorf(dst * scale)), in - 1), scale = float(in) / out);
 *   positions[l] fp32 [batch][h_l][w_l][2 * num_pos_feats], 16-byte aligned: the normalised sine position embedding of
 *     that mask (models/position_encoding.py, normalize=True, scale 2 pi), the y half first, sin on even and cos on odd
 *     features -- fp32 operations in the order of the eager chain.
 * masks and positions are host arrays of num_levels device pointers.  dim_t, degenerate: fp32 device [num_pos_feats],
 * 16-byte aligned: temperature ** (2 * (i / 2) / num_pos_feats), and the embedding's value where the row / column holds no
 * valid pixel (its normaliser is 0 and the sine's argument about -3.1e6 / dim_t: the caller supplies what its reference
 * computes there).  num_pos_feats: a multiple of 4 up to VNX_INGEST_MAX_POS_FEATS, else VNX_ERR_UNSUPPORTED.
 *
 * One launch each; no atomics, no workspace, no allocation, no synchronisation: both are capturable.  batch == 0 (or
 * num_levels == 0): VNX_OK, no launch.
 */
#define VNX_INGEST_MAX_LEVELS 8
#define VNX_INGEST_MAX_POS_FEATS 128
int vnx_ingest_frames(const void* pixels, size_t pixel_bytes, const void* table, int batch, int height, int width,
                      float mean0, float mean1, float mean2, float std0, float std1, float std2, int channels_last,
                      void* x, void* mask, void* hip_stream);
int vnx_ingest_levels(const void* table, int batch, int height, int width, int num_levels, const int* level_sizes,
                      int num_pos_feats, const void* dim_t, const void* degenerate, void* const* masks,
                      void* const* positions, void* hip_stream);

/*
 * Test-time resize fused into the ingest (resize.hip): staged uint8 source frames to the x and mask of vnx_ingest_frames, of
 * the frames RESIZED as Pillow's Image.resize(..., BILINEAR) resizes 8-bit images -- byte for byte -- in one launch.
 * ADDITIVE: one symbol, no existing signature changed, so VNX_ABI_VERSION stays 17; a binding that needs it looks it up.
 *
 * pixels: uint8 device buffer of pixel_bytes bytes, 4-byte aligned.  interleaved 0: each frame is three planes of h x w bytes
 * back to back (CHW); interleaved 1: h x w pixels of 3 bytes (HWC).  src_table: int32 device [batch][3] = {byte offset of the
 * frame inside pixels (any value: no alignment asked), h, w}.  dst_table: int32 device [batch][3] = {0, nh, nw}, the target
 * sizes: the table vnx_ingest_levels takes for the resized batch.  coeffs: int32 device buffer of coeff_words words; its first
 * 6 * batch words are a row per frame {bounds offset, weights offset, ksize} for the horizontal pass (w -> nw), then the same
 * for the vertical pass (h -> nh), offsets in words from the start of coeffs.  bounds: int32 [n_out][2] = {first source
 * index, tap count}; weights: int32 [n_out][ksize], 22-bit fixed point, non-negative: Pillow's precompute_coeffs for the
 * bilinear filter, normalised and rounded as its 8-bit path does (the caller computes them in double; the kernel never
 * evaluates the filter).  ksize 0: the axis keeps its size and the pass is skipped.  A pass is
 * min((2^21 + sum_t weight[t] * src[first + t]) >> 22, 255); the horizontal pass runs first and is rounded to bytes.
 * 1 <= ksize <= VNX_RESIZE_MAX_KSIZE: a downscale of up to 8x, any upscale.
 *
 * Everything the kernel needs of the frames is read from memory by the kernel, not by the host: a captured launch replays
 * on new pixels (and on other sizes, as long as the tables and coefficients in memory describe them); batch, height, width,
 * the layouts and mean / std are baked in.  A frame whose rows do not describe bytes inside pixels, a target inside height x
 * width and tables inside coeffs (a negative value, nh > height, nw > width, offset + 3 h w > pixel_bytes, ksize above the
 * limit, ksize 0 on an axis whose size changes, table offsets outside coeffs) is taken as an empty frame (all padding), and
 * table entries are clamped to the source: no read leaves a buffer whatever the tables hold.
 *
 * height, width multiples of 32.  x fp32 [batch][3][height][width] (channels_last 0) or [batch][height][width][3]
 * (channels_last 1), mask uint8 / bool [batch][height][width], both 16-byte aligned.  Inside a resized frame
 * x = (float(u) - mean[c]) / std[c] -- an IEEE subtract, then a correctly rounded IEEE divide -- and mask = 0; outside x = 0
 * and mask = 1.  A frame whose target equals its source gives exactly what vnx_ingest_frames gives.  Every element of both
 * is written: no memset is needed before the call.  One launch; no atomics, no workspace, no allocation, no
 * synchronisation: capturable.  batch == 0: VNX_OK, no launch.
 */
#define VNX_RESIZE_MAX_KSIZE 17
int vnx_resize_ingest_frames(const void* pixels, size_t pixel_bytes, const void* src_table, const void* dst_table,
                             const void* coeffs, size_t coeff_words, int batch, int height, int width, float mean0,
                             float mean1, float mean2, float std0, float std1, float std2, int channels_last,
                             int interleaved, void* x, void* mask, void* hip_stream);

/*
 * Training-time augmentation on the device (augment.hip): crop, Pillow's bilinear resize and a horizontal flip of uint8
 * source frames into x and mask, and the same geometry applied to the ground-truth masks straight from their COCO run
 * lengths, with the masks' boxes.  ADDITIVE: three symbols, no existing signature changed, so VNX_ABI_VERSION stays 17.
 *
 * vnx_augment_frames: the arguments, outputs and guarantees of vnx_resize_ingest_frames (the same device code), with wider
 * rows.  src_table: int32 device [batch][8] = {byte offset, h, w, x0, y0, cw, ch, flip}: the crop window of cw x ch pixels
 * at (x0, y0) inside the h x w frame, and flip != 0 for a horizontal flip of the RESIZED window (output column x takes
 * resized column nw - 1 - x, as np.flip(resized, axis=1)).  The rows of pixels keep the pitch w (CHW: plane stride h * w).
 * coeffs: its first 8 * batch words are a row per frame: the two triples of vnx_resize_ingest_frames, for (cw -> nw) and
 * (ch -> nh), then the word offsets of the frame's two NEAREST index tables, int32 [nw] of (cw -> nw) and int32 [nh] of
 * (ch -> nh) (read by vnx_augment_masks only).  A window that leaves the frame makes an empty frame, like every other
 * malformed row.  A row with the full window and flip 0 gives what vnx_resize_ingest_frames gives, bit for bit.
 *
 * vnx_augment_masks: n_masks (instance, frame) masks of a step.  ends: int32 device [n_ends], the masks' run END positions
 * back to back: per mask the cumulative sums of its COCO counts (column-major positions p = x * h + y; runs of zeros and
 * ones alternate, zeros first; zero-length runs are legal).  mask_rows: int32 device [n_masks][4] = {offset of the mask's
 * ends, n_runs, frame index, byte offset of the mask's output inside masks}.  src_table, dst_table, coeffs: the tables of
 * vnx_augment_frames for the n_frames frames (dst_table [n_frames][3] = {0, nh, nw}).  height, width: the padded size,
 * multiples of 32 (it sizes the launch; nh <= height, nw <= width).  Output pixel (y, x) of a mask is the value of source
 * pixel (y0 + ytab[y], x0 + xtab[flip ? nw - 1 - x : x]): the parity of the number of ends <= xs * h + ys.  The nearest
 * tables are Pillow's, which accumulates them in double (tab[i] = int(xo); xo += n_in / n_out, from xo = 0.5 * n_in /
 * n_out): the host makes them; the kernel only reads them, clamped to the window.
 *   masks uint8 / bool, mask_bytes bytes: mask m is [nh][nw] of its frame at its row's byte offset; every byte of it written.
 *   boxes fp32 [n_masks][4] = {min x, min y, max x + 1, max y + 1} over the mask's set pixels; nonempty uint8 [n_masks].
 *   An empty mask gives a zero box and nonempty 0.
 * n_runs == 1 is the empty mask.  Runs outside ends, or whose last end is not h * w, are taken as the empty mask; a row that
 * names no frame, a malformed frame or an output range outside masks writes no mask bytes and gives a zero box.  No read
 * leaves a buffer whatever the tables hold.  workspace: vnx_augment_masks_workspace(n_masks, height, width) bytes, 16-byte
 * aligned (16 bytes per (mask, 32 x 32 tile): the tiles' boxes; every slot is written, no memset).  Two launches; no
 * atomics, no allocation, no synchronisation: capturable, and bit-identical run to run.  n_masks == 0: VNX_OK, no launch.
 */
int vnx_augment_frames(const void* pixels, size_t pixel_bytes, const void* src_table, const void* dst_table,
                       const void* coeffs, size_t coeff_words, int batch, int height, int width, float mean0, float mean1,
                       float mean2, float std0, float std1, float std2, int channels_last, int interleaved, void* x,
                       void* mask, void* hip_stream);
size_t vnx_augment_masks_workspace(int n_masks, int height, int width);
int vnx_augment_masks(const void* ends, size_t n_ends, const void* mask_rows, int n_masks, const void* src_table,
                      const void* dst_table, const void* coeffs, size_t coeff_words, int n_frames, int height, int width,
                      void* masks, size_t mask_bytes, void* boxes, void* nonempty, void* workspace, size_t workspace_bytes,
                      void* hip_stream);

/*
 * The first resample of a two-resample augmentation chain (augment.hip; flip -> resize -> crop -> resize, the COCO
 * pre-training mapper's): a frame resized to (h1, w1) as Pillow's Image.resize(..., BILINEAR) resizes 8-bit images, of which
 * only a crop window is computed, stored as BYTES into the pixel buffer itself, where vnx_augment_frames reads it as a source
 * frame.  ADDITIVE: one symbol, no existing signature changed, so VNX_ABI_VERSION stays 17.  The same device code as
 * vnx_resize_ingest_frames and vnx_augment_frames.
 *
 * pixels: uint8 device buffer of pixel_bytes bytes, 4-byte aligned, read AND written.  interleaved: as above, for the source
 * frames and for the stored windows alike.  win_table: int32 device [batch][16] = {byte offset of the source frame, h, w, h1,
 * w1, x0, y0, cw, ch, byte offset of the window's slot, then {bounds offset, weights offset, ksize} of (w -> w1) and of
 * (h -> h1)}: the window of cw x ch pixels at (x0, y0) inside the RESIZED h1 x w1 image; the coefficient tables are those of
 * vnx_resize_ingest_frames for the whole axes (w1 and h1 rows), offsets in words from the start of coeffs, ksize 0 where
 * the axis keeps its size.  The slot takes 3 * ch * cw bytes at any byte offset: CHW three planes of ch x cw, HWC ch x cw
 * pixels of 3 bytes, row pitch cw.  height, width: multiples of 32, at least every ch and cw (they size the launch).
 *
 * A row whose window leaves (h1, w1) or height x width, whose source bytes or slot leave pixels, whose slot overlaps its own
 * source frame, or whose tables are malformed as for vnx_resize_ingest_frames writes NOTHING: its slot keeps its bytes.  No
 * read leaves pixels or coeffs and no write leaves the row's slot, whatever the table holds; slots of different rows must
 * not overlap each other or any source frame of the launch (the caller lays them out).  Everything is read from device
 * memory by the kernel: a captured launch replays on other pixels, sizes and windows of the same batch, height and width.
 * One launch; 16-byte stores wherever 16 aligned bytes lie inside one tile row of a slot, byte stores at the ends; no
 * atomics, no workspace, no allocation, no synchronisation: capturable.  batch == 0: VNX_OK, no launch.
 */
int vnx_resize_window_bytes(void* pixels, size_t pixel_bytes, const void* win_table, const void* coeffs, size_t coeff_words,
                            int batch, int height, int width, int interleaved, void* hip_stream);

/*
 * Colour augmentation inside the frame launch (augment.hip): vnx_augment_frames with detectron2's RandomBrightness,
 * RandomContrast and RandomSaturation applied, in that order and per frame, to the resized and flipped BYTES before they are
 * normalised.  ADDITIVE: two symbols, no existing signature changed, so VNX_ABI_VERSION stays 17.
 *
 * Every argument of vnx_augment_frames keeps its meaning.  color_table: int32 device [batch][8] = {flags, the brightness
 * weight's float bit pattern, the contrast weight as a double (low word, high word), the saturation weight likewise, 0, 0};
 * flags: 1 brightness, 2 contrast, 4 saturation; a row with flags 0 gives what vnx_augment_frames gives, bit for bit.  Each
 * step returns bytes through clip(x, 0, 255) and truncation, so the next one sees bytes:
 *   brightness  x = float(w) * float(u): one rounding, in float;
 *   contrast    x = (1 - w) * m + w * double(u), m = the integer sum of the frame's own nh * nw * 3 bytes AFTER brightness
 *               divided once, in double; the padding and the other frames do not count;
 *   saturation  g = u0 * 0.299 + u1 * 0.587 + u2 * 0.114 (three rounded products, summed left to right, on the channels in
 *               stored order), x = (1 - w) * g + w * double(u_c) per channel.
 * Every product and every sum is rounded on its own (no fused multiply-add): the results are numpy's, byte for byte.
 *
 * contrast == 0: ONE launch; a row that asks for contrast is then malformed.  contrast != 0: TWO launches -- the first stores
 * the post-brightness bytes and a sum per 32 x 32 tile into the workspace, the second folds a frame's sums and finishes.  The
 * workspace is vnx_augment_color_workspace(batch, height, width) bytes INSIDE pixels at byte workspace_offset (a multiple of
 * 16), behind every source frame; pixels is written there and nowhere else.  Every slot of it that is read was written by
 * the first launch: no memset, no atomics, bit-identical run to run.
 * A malformed row -- those of vnx_augment_frames, a flag beyond the three, a weight in use that is not finite, source bytes
 * that reach into the workspace -- makes an empty frame.  No read leaves a buffer whatever the tables hold.  The weights live
 * in device memory: a captured launch replays on other pixels, geometry and weights.  batch == 0: VNX_OK, no launch.
 */
size_t vnx_augment_color_workspace(int batch, int height, int width);
int vnx_augment_frames_color(void* pixels, size_t pixel_bytes, const void* src_table, const void* dst_table,
                             const void* coeffs, size_t coeff_words, const void* color_table, int batch, int height, int width,
                             float mean0, float mean1, float mean2, float std0, float std1, float std2, int channels_last,
                             int interleaved, int contrast, size_t workspace_offset, void* x, void* mask, void* hip_stream);

/*
 * Clipped AdamW step (optim.hip): the full-model gradient norm, clip_grad_norm_'s coefficient and the decoupled AdamW
 * update of EVERY parameter tensor of a model in three launches, whatever the number of tensors.  ADDITIVE: two symbols, no
 * existing signature changed, so VNX_ABI_VERSION stays 17; a binding that needs them looks the symbols up.
 *
 * The kernels work from three tables in device memory.
 *   tensors: vnx_adamw_tensor [n_tensors], 16-byte aligned, one row per parameter tensor: the fp32 device pointers p, g, m, v
 *     (numel elements each, walked as flat memory), the index of the tensor's row in groups, flags, and the tensor's two
 *     bias corrections 1 - beta1^step and sqrt(1 - beta2^step) of the step being taken, computed by the caller in double.
 *     g == NULL: the tensor is skipped this step (nothing of it is read or written; it adds 0 to the norm).
 *     VNX_ADAMW_UNALIGNED in flags: one of the four pointers is not 16-byte aligned; the tensor takes 4-byte accesses.  A
 *     row WITHOUT the flag promises four 16-byte aligned pointers.
 *   groups: vnx_adamw_group [n_groups], 16-byte aligned, doubles: lr, weight_decay, beta1, beta2, eps, and decay = 1 - lr *
 *     weight_decay, 1 - beta1, 1 - beta2 as the caller computes them.
 *   chunks: int64 [n_chunks][2] = {tensor index, element offset}: the tensors cut into pieces of VNX_ADAMW_CHUNK elements
 *     (the last piece of a tensor may be shorter; offsets are multiples of VNX_ADAMW_CHUNK; no piece crosses a tensor).  The
 *     list depends on the element counts alone; one workgroup handles one chunk.  A chunk that names no tensor or lies
 *     outside its tensor is ignored (its partial is 0).
 *
 * vnx_adamw_grad_norm, two launches: every chunk's sum of g^2, accumulated in fp32, goes to its own slot of partials (fp32
 * [n_chunks]; EVERY slot is written, no memset is needed), then one workgroup folds the slots in a fixed order in double
 * and leaves total_norm = sqrt(sum) and coef = min(1, max_norm / (total_norm + 1e-6)) -- torch.nn.utils.clip_grad_norm_'s
 * expression for the L2 norm with error_if_nonfinite=False; a NaN norm gives a NaN coefficient, an infinite one 0 -- in
 * norm, 16 bytes, 8-byte aligned: {float total_norm, float coef, double coef}.
 *
 * vnx_adamw_clipped_step, one launch: with g' = g * coef (coef read from norm in device memory: no host synchronisation)
 *   p <- p * decay;  m <- m + (1 - beta1) (g' - m);  v <- beta2 v + (1 - beta2) g'^2;
 *   p <- p - (lr / bc1) * m / (sqrt(v) / bc2_sqrt + eps)
 * on fp32 tensors: torch.optim.AdamW (decoupled weight decay, no amsgrad, no maximize).  The multiply-adds of the three
 * updates run in double and each result is rounded to fp32 once; the denominator is fp32, with a correctly rounded square root
 * and divisions, from the new fp32 m and v.  The clipped gradients are NOT written back
 * -- g is only read; this is the one difference from clip_grad_norm_ followed by AdamW.step, which leaves g rescaled in
 * place.  Non-finite gradients get no special case: they propagate into m, v and p as the expression says.
 *
 * 16-byte loads and stores on tensors without VNX_ADAMW_UNALIGNED, 4-byte ones on the others and on a tensor's last numel % 4
 * elements; no read or write outside [0, numel) of any tensor.  No atomics anywhere: two runs on the same inputs are
 * bit-identical.  No workspace beyond partials, no allocation, no synchronisation.  n_chunks == 0: vnx_adamw_grad_norm
 * still writes norm (total_norm 0, coef 1) in one launch; vnx_adamw_clipped_step returns VNX_OK without a launch.
 */
#define VNX_ADAMW_CHUNK 4096
#define VNX_ADAMW_UNALIGNED 1
typedef struct vnx_adamw_tensor {
  void* p;
  const void* g;
  void* m;
  void* v;
  long long numel;
  int group;
  int flags;
  float bias_correction1;      /* 1 - beta1^step */
  float bias_correction2_sqrt; /* sqrt(1 - beta2^step) */
  int reserved[2];
} vnx_adamw_tensor;            /* 64 bytes */
typedef struct vnx_adamw_group {
  double lr, weight_decay, beta1, beta2, eps;
  double decay, one_minus_beta1, one_minus_beta2;
} vnx_adamw_group;             /* 64 bytes */
int vnx_adamw_grad_norm(const void* tensors, int n_tensors, const void* chunks, long long n_chunks, double max_norm,
                        void* partials, void* norm, void* hip_stream);
int vnx_adamw_clipped_step(const void* tensors, int n_tensors, const void* groups, int n_groups, const void* chunks,
                           long long n_chunks, const void* norm, void* hip_stream);

/*
 * Video mask IoU from run lengths: the integer sums of the YTVIS evaluator's IoU (YTVOSeval.computeIoU) and the decode of
 * compressed COCO RLE strings into the run tables they are taken from (video_iou.hip; ABI 17, additive).
 *
 * A mask is a slice of two int32 arenas of run_slots elements each: ends[k] = the column-major pixel index at which run
 * k ends (the cumulative sum of the COCO counts; run 0 counts zeros), ones[k] = the number of set pixels below ends[k].
 * A pixel's bit is the parity of the upper bound of its index in ends, so zero-length runs are harmless.  rows int32
 * [masks][4] = {arena offset, runs, pixel count h * w, area}, 16-byte aligned.
 *
 * vnx_rle_runs_measure / vnx_rle_runs_write turn strings in the format stated at vnx_mask_rle_* (a byte arena of
 * arena_bytes, offsets and lengths int64 [masks]) into such tables.  A string has as many counts as it has bytes without
 * the continuation bit (byte - 48) & 0x20: measure writes that number to runs int32 [masks]; the caller scans it into
 * run_offsets int32 [masks] and passes both back to write with pixels int32 [masks] (h * w of each mask) and arenas of
 * run_slots >= the sum.  write fills the slots, rows and status int32 [masks]: 0, or an OR of the VNX_RLE_RUNS_* bits --
 * a byte outside 48..111; a string that ends inside a count; a negative count or one of more than 7 characters; runs
 * that do not sum to the pixel count (an empty string included); a string outside the byte arena, a slot outside the
 * run arenas or not of the measured size.  A mask with a non-zero status gets the empty table (runs 0, area 0; the
 * contents of its own slot are unspecified).  Whatever the bytes are, no read leaves [offset, offset + length) of a
 * string and no write leaves a mask's slot.  One wave per string; no atomics, no workspace, no allocation, no
 * synchronisation.  masks == 0 is a no-op; run_slots >= 2^31 is VNX_ERR_UNSUPPORTED.
 *
 * vnx_video_iou_sums: frame_mask int32 [frame_slots] = the mask index per (track, frame), -1 where the track has no mask
 * in that frame; tracks int32 [n_tracks][2] = {first, frames} into frame_mask; pairs int32 [n_pairs][2] = {detection
 * track, ground-truth track} (both 8-byte aligned).  sums int64 [n_pairs][4] = {sum over the frames of the intersection,
 * of the detection's area, of the ground truth's area, status}; an absent mask has area 0 and no intersection, so the
 * IoU of the pair is I / (A_d + A_g - I) (0 when that is 0), formed by the caller in double.  status is non-zero, with
 * zero sums, when the two tracks differ in frame count (VNX_VIDEO_IOU_FRAMES), a frame's two masks differ in pixel
 * count (VNX_VIDEO_IOU_PIXELS) or an index or a row points outside its table (VNX_VIDEO_IOU_BAD_TABLE): nothing outside
 * the tables the sizes describe is read.  One wave per pair, no atomics, no workspace: the output is a function of the
 * input alone.  n_pairs == 0 is a no-op.
 */
enum {
  VNX_RLE_RUNS_BAD_BYTE = 1,
  VNX_RLE_RUNS_TRUNCATED = 2,
  VNX_RLE_RUNS_NEGATIVE = 4,
  VNX_RLE_RUNS_BAD_SUM = 8,
  VNX_RLE_RUNS_BAD_SLOT = 16
};
enum {
  VNX_VIDEO_IOU_FRAMES = 1,
  VNX_VIDEO_IOU_PIXELS = 2,
  VNX_VIDEO_IOU_BAD_TABLE = 4
};
int vnx_rle_runs_measure(const void* bytes, long long arena_bytes, const void* offsets, const void* lengths, int masks,
                         void* runs, void* hip_stream);
int vnx_rle_runs_write(const void* bytes, long long arena_bytes, const void* offsets, const void* lengths,
                       const void* pixels, const void* run_offsets, const void* runs, int masks, void* ends, void* ones,
                       long long run_slots, void* rows, void* status, void* hip_stream);
int vnx_video_iou_sums(const void* ends, const void* ones, long long run_slots, const void* rows, int masks,
                       const void* frame_mask, long long frame_slots, const void* tracks, int n_tracks,
                       const void* pairs, long long n_pairs, void* sums, void* hip_stream);

/*
 * The greedy matching of the COCO-style AP evaluators (COCOeval.evaluateImg, YTVOSeval.evaluateVid) for every (image,
 * category) problem of an evaluation, all area ranges and all IoU thresholds in one launch (ap_match.hip; host
 * specification: vnext_amd/ops/ap_match.py match_host).  ADDITIVE: one symbol, no existing signature changed, so
 * VNX_ABI_VERSION stays 17; a binding that needs it looks it up.
 *
 * table int64 [problems][5] = {D, G, detection offset, ground-truth offset, IoU offset}: problem p owns detections
 * [offset, offset + D) of dt_area double [n_dt], ground truths [offset, offset + G) of gt_crowd uint8 [n_gt] and gt_area
 * double [n_gt], and the row-major [D][G] matrix at its IoU offset in ious double [n_iou].  The detections stand in the
 * order the reference visits them (by score, cut to the last maxDets), the ground truths in their given order.
 * area_rng double [n_area][2] = {low, high}, thrs double [n_thrs].
 *
 * Per (area range a, threshold t, problem): a ground truth is ignored when it is a crowd or its area is < low or >
 * high.  The detections take, one after the other, the ground truth of the highest IoU >= min(thrs[t], 1 - 1e-10)
 * among those still free (a crowd stays free), the later one on a tie, where "later" is the reference's order: the
 * ground truths that are not ignored in their given order, then the ignored ones, which are looked at only while the
 * detection holds no match.  Outputs, in problem-local indices, -1 for none: dt_match int32 [n_area][n_thrs][n_dt] (the
 * ground truth a detection took), dt_ignore uint8 [n_area][n_thrs][n_dt] (that ground truth's ignore flag; for a
 * detection without a match, whether its area is < low or > high), gt_match int32 [n_area][n_thrs][n_gt] (the last
 * detection that took it), gt_ignore uint8 [n_area][n_gt].  Ids are the caller's: it maps the indices.
 *
 * One wave64 per problem, one lane per (a, t), the lane's bit sets in LDS; no atomics, no workspace, every element
 * written by one lane: the result is byte-identical run to run.  Elements no problem owns are not written.
 * Limits: n_area * n_thrs <= VNX_AP_MATCH_MAX_LANES (VNX_ERR_UNSUPPORTED beyond) and G <= VNX_AP_MATCH_MAX_GT per problem.
 * status int32 [1], zeroed by the caller: a row with G above the limit writes nothing and stores VNX_AP_MATCH_GT_LIMIT;
 * a row with a negative entry or a range that leaves n_dt, n_gt or n_iou writes nothing, reads nothing beyond the row
 * and stores VNX_AP_MATCH_BAD_TABLE (with several such rows one of their codes stays).  Rows that overlap each other
 * are not detected.  problems == 0 is a no-op.  Not measured against a host implementation in C; the timings of
 * profiles/coco_eval.json compare it with this package's numpy route.
 */
#define VNX_AP_MATCH_MAX_GT 512
#define VNX_AP_MATCH_MAX_LANES 64
enum {
  VNX_AP_MATCH_BAD_TABLE = 1,
  VNX_AP_MATCH_GT_LIMIT = 2
};
int vnx_ap_match(const void* table, long long problems, const void* ious, long long n_iou, const void* gt_crowd,
                 const void* gt_area, long long n_gt, const void* dt_area, long long n_dt, const void* area_rng,
                 int n_area, const void* thrs, int n_thrs, void* dt_match, void* dt_ignore, void* gt_match,
                 void* gt_ignore, void* status, void* hip_stream);

/*
 * COCO polygons to run tables: pycocotools' frPyObjects (rleFrPoly) + merge (the union) for one annotation per workgroup
 * (poly_rle.hip; host specification, step by step: vnext_amd/ops/poly_rle.py object_counts_host, to which the kernel is held
 * count for count).  ADDITIVE: one symbol, no existing signature changed, so VNX_ABI_VERSION stays 17.
 *
 * coords double [n_coords], 8-byte aligned: the polygons' x0, y0, x1, y1, ... back to back.  poly_rows int32 [n_polys][4],
 * 16-byte aligned = {coordinate offset, vertices, object, 0}.  obj_rows int32 [n_objects][6] = {first polygon, polygons,
 * run-slot offset, slot size, h, w}: object m owns polygons [first, first + polygons) of poly_rows (each must name m) and
 * the words [offset, offset + slot size) of ends and ones, int32 [run_slots] each.  An object without polygons is the
 * empty mask.  A box is passed as its 4-vertex polygon.
 *
 * Per object: ends[offset + k] = the k-th run end of the union of its polygons' even-odd masks (h * w the last),
 * ones[offset + k] = the set pixels below it, rows int32 [n_objects][4] = {offset, runs, h * w, area} as
 * vnx_rle_runs_write leaves them.  The caller sizes the slot from a bound (the sum over the object's polygons of 1 + the sum
 * over the edges of min(|X[j+1] - X[j]| / 5 + 1, w), X = (int)(5 x + 0.5), plus 1); the words of the slot beyond the runs
 * are padded with ends = h * w and ones = area (zero-length runs), so a consumer may take the slot size for the run count.
 * The line expressions are evaluated in double as a product and two additions, without contraction, the divisions IEEE.
 *
 * status int32 [n_objects]: 0, or an OR of the VNX_POLY_RLE_* bits -- a coordinate that is not finite or beyond 2^24 in
 * magnitude; a polygon of fewer than 3 vertices; h * w outside [1, 2^31); more than VNX_POLY_RLE_MAX_VERTICES vertices in a
 * polygon, VNX_POLY_RLE_MAX_POINTS dense points (the sum over the edges of max(|dX|, |dY|) + 1) or VNX_POLY_RLE_MAX_POLYGONS
 * polygons in an object, VNX_POLY_RLE_MAX_CROSSINGS crossings in a polygon or toggles in an object, or a slot of more than
 * VNX_POLY_RLE_MAX_CROSSINGS + 1 words; a row, a polygon or a slot outside its table, a polygon that names another object,
 * or a slot smaller than the runs.  A flagged object gets the empty table (runs 0, area 0) and, where its slot lies inside
 * the arenas, a slot filled with ends = h * w (0 for a bad size) and ones = 0 up to the cap.  Whatever the tables hold, no
 * read leaves a buffer and no write leaves the object's slot.  One wave64 per object; no atomics, no workspace, no
 * allocation, no synchronisation: capturable, and bit-identical run to run.  n_objects == 0 is a no-op; run_slots or
 * n_coords >= 2^31 is VNX_ERR_UNSUPPORTED.
 */
#define VNX_POLY_RLE_MAX_VERTICES 1024
#define VNX_POLY_RLE_MAX_CROSSINGS 4096
#define VNX_POLY_RLE_MAX_POINTS 262144
#define VNX_POLY_RLE_MAX_POLYGONS 256
enum {
  VNX_POLY_RLE_BAD_COORD = 1,
  VNX_POLY_RLE_FEW_VERTICES = 2,
  VNX_POLY_RLE_BAD_SIZE = 4,
  VNX_POLY_RLE_CAP = 8,
  VNX_POLY_RLE_BAD_SLOT = 16
};
int vnx_poly_rle(const void* coords, long long n_coords, const void* poly_rows, int n_polys, const void* obj_rows,
                 int n_objects, void* ends, void* ones, long long run_slots, void* rows, void* status, void* hip_stream);

/* (The kernel-variant override of rounds 1-3 -- a process-wide A/B knob -- is no longer part of this library: it lives in
 *  the development build only, include/vnext_hip_dev.h.  Every call here selects its kernels from its own arguments.) */

#ifdef __cplusplus
}
#endif
#endif /* VNEXT_HIP_H_ */
