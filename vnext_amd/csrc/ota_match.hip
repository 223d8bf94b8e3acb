// ota_match.hip -- IDOL's simOTA matching and the contrastive positive / negative sets on the device.
//
// One launch for all problems of a training step, ONE WORKGROUP OF FOUR WAVE64 PER PROBLEM.  Two kinds of problem, told
// apart by the problem's number against OtaArgs::n_det:
//   detection  (decoder layer, key image):  OTAMatcher._one   = ota_cost, dynamic_k_matching(10), the two index outputs
//   selection  (reference image, last layer): select_pos_neg_masks up to its sampling loop = ota_cost on the VALID
//              instances (compacted in order here), dynamic_k_matching(10) -> pos, dynamic_k_matching(100) ON THE COST
//              THE FIRST PASS REPAIRED -> neg = ~M
// (vnext_amd/models/idol_criterion.py, which mirrors the reference's matcher.py:69-173 and pos_neg_select.py).
//
// Arithmetic.  fp32, operation by operation as the ATen expressions of the host form, contraction off for the whole
// file: the eight strict comparisons of in_boxes_info are then bit-identical to the host's on the same inputs; the cost
// differs from the host's by the rounding of logf only.  Every choice among equal values goes to the LOWER index (the
// first minimum is what ATen's CPU argmin returns; torch.topk's choice among equal costs is unspecified).
//
// Four waves, not one: the k-smallest / k-largest selections are rank counts -- element q is selected when fewer than k
// elements precede it in (value, index) order -- which is Q x Q comparisons per column whatever k is, so the k = 100 pass
// of a selection problem costs what the k = 10 pass does (100 extractions by a wave-wide arg-min would be 100 dependent
// reductions per column).  The count is independent per q: 256 threads take the 300 queries of a column in two rounds
// against LDS broadcast reads; one wave would need five.  What the four waves pay is a workgroup barrier where one wave
// would need none -- a handful per column.  The arg-mins over a column (repair loop, `matched`) are a wave each, columns
// dealt round-robin to the waves.
//
// No atomics, every reduction in a fixed order: the output is a function of the input alone.  The repair loop is uniform
// across the workgroup (its condition is read from LDS after a barrier) and bounded; a problem that reaches the bound, one
// with a non-finite cost or IoU and one with a label outside [0, K) set the status word and write an empty result.
//
// LDS of a problem with n targets and Q queries (ota_lds_bytes; Qp = Q rounded up to 4):
//   cost fp32 [n][Qp] (target-major: the lanes of a column pass read consecutive banks) | ikey, ckey int32 [Qp] (the
//   current column's IoUs and costs as ordered integers, transient) | rank int32 [Q] | top fp32 [128] | col_has int32 [n] |
//   inst int32 [n] | 16 words | M uint8 [n][Qp] (bit 0 the matching, bit 1 the first pass's matching kept for `pos`) |
//   multi uint8 [Qp]
// n (5 Qp + 8) + 9 Qp + 4 Q + 576 bytes.  Q = 300: 4 476 B + n x 1 508 B, n <= 105 in the 160 KB of a gfx950 CU.
//
// Output, int32 words, `stride` per problem (ota_out_words):
//   [0] status (0 solved, 1 non-finite, 2 repair loop bound, 3 bad label / offsets)   [1] n (targets / valid instances)
//   detection: [2 .. 2+Q) gt_of_query (-1, or the lowest target the query is assigned to)  [2+Q .. 2+Q+n) matched
//   selection: [2 .. 2+n) the valid instances' indices in the image  then, from word 2 + n_cap, bytes [n_cap][Q]:
//              bit 0 pos, bit 1 neg of (instance, query)
//   every other word of the stride is -1 (detection) / -1 in the instance list and 0 in the bytes (selection).
#include <limits.h>

#include "vnx_common.h"

#pragma clang fp contract(off)

// the loops over targets and queries are short and their bounds are run-time values: unrolled or interleaved, each keeps a
// handful of remainder predicates alive in SGPRs across the whole matching, which spills
#define VNX_PLAIN_LOOP _Pragma("clang loop unroll(disable) vectorize(disable) interleave(disable)")

namespace vnx {
namespace {

constexpr int kOtaThreads = 256;
constexpr int kOtaWaves = kOtaThreads / kWave;
constexpr int kOtaTop = 128;                      // >= the largest candidate count (100)
constexpr size_t kOtaLdsBytes = 160 * 1024;       // LDS of a gfx950 CU

__host__ __device__ inline size_t ota_lds_bytes(int n, int Q) {
  const size_t Qp = pad4(Q);
  return size_t(n) * (5 * Qp + 8) + 9 * Qp + size_t(4) * Q + 4 * kOtaTop + 64;
}
__host__ __device__ inline int ota_out_words(int n_cap, int Q) {
  const int det = Q + n_cap, sel = n_cap + (n_cap * Q + 3) / 4;
  return 2 + (det > sel ? det : sel);
}

struct OtaArgs {
  const float* det_prob;      // [n_det][Q][K]
  const float* det_boxes;     // [n_det][Q][4]
  const float* ref_prob;      // [n_ref][Q][K]
  const float* ref_boxes;     // [n_ref][Q][4]
  const float* tgt_boxes;     // [n_tot][4]
  const int64_t* labels;      // [n_tot]
  const uint8_t* valid;       // [n_tot - valid_first]: target t's flag at valid[t - valid_first]
  const int32_t* problems;    // [n_det + n_ref][2] = (first target, count)
  int32_t* out;               // [n_det + n_ref][stride]
  int n_det, n_ref, Q, K, n_tot, valid_first, n_cap, stride;
};

struct OtaLds {
  float* cost;      // [n][Qp]
  int* ikey;        // [Qp] the current column's IoUs as ordered integers (order_key), the pad -inf
  int* ckey;        // [Qp] the current column's costs likewise, the pad +inf
  int* rank;        // [Q]
  float* top;       // [kOtaTop]
  int* col_has;     // [n]
  int* inst;        // [n]
  int* misc;        // [16]
  uint8_t* M;       // [n][Qp]
  uint8_t* multi;   // [Qp]
};

__device__ __forceinline__ OtaLds ota_carve(unsigned char* smem, int n, int Q) {
  OtaLds s;
  s.cost = reinterpret_cast<float*>(smem);
  s.ikey = reinterpret_cast<int*>(s.cost + size_t(n) * pad4(Q));
  s.ckey = s.ikey + pad4(Q);
  s.rank = s.ckey + pad4(Q);
  s.top = reinterpret_cast<float*>(s.rank + Q);
  s.col_has = reinterpret_cast<int*>(s.top + kOtaTop);
  s.inst = s.col_has + n;
  s.misc = s.inst + n;
  s.M = reinterpret_cast<uint8_t*>(s.misc + 16);
  s.multi = s.M + size_t(n) * pad4(Q);
  return s;
}

typedef int vnx_i4 __attribute__((ext_vector_type(4)));

struct Box { float x0, y0, x1, y1; };

// box_cxcywh_to_xyxy: c - 0.5 * wh, c + 0.5 * wh
__device__ __forceinline__ Box to_xyxy(vnx_f4 b) {
  const float hw = 0.5f * b.z, hh = 0.5f * b.w;
  return Box{b.x - hw, b.y - hh, b.x + hw, b.y + hh};
}
__device__ __forceinline__ float box_area(const Box& b) { return (b.x1 - b.x0) * (b.y1 - b.y0); }

// _pairwise_iou / pairwise_giou: the intersection and the union are the same expressions in both
__device__ __forceinline__ void iou_terms(const Box& a, const Box& b, float& inter, float& uni) {
  const float iw = fmaxf(fminf(a.x1, b.x1) - fmaxf(a.x0, b.x0), 0.f);
  const float ih = fmaxf(fminf(a.y1, b.y1) - fmaxf(a.y0, b.y0), 0.f);
  inter = iw * ih;
  uni = box_area(a) + box_area(b) - inter;
}
__device__ __forceinline__ float pair_iou(const Box& a, const Box& b) {
  float inter, uni;
  iou_terms(a, b, inter, uni);
  return inter / uni;
}

// true on any thread -> true on all (misc[1] is the flag; three barriers: it is free again on return)
__device__ __forceinline__ bool block_any(const OtaLds& s, bool pred) {
  if (threadIdx.x == 0) s.misc[1] = 0;
  __syncthreads();
  if (pred) s.misc[1] = 1;
  __syncthreads();
  const bool r = s.misc[1] != 0;
  __syncthreads();
  return r;
}

// arg-min of column c over its queries (all of them, or those assigned to it), by one wave: ties to the lower query
__device__ __forceinline__ int column_argmin(const OtaLds& s, int c, int Q, int Qp, bool assigned_only, int lane) {
  const float* col = s.cost + size_t(c) * Qp;
  const uint8_t* m = s.M + size_t(c) * Qp;
  float best = __builtin_huge_valf();
  int best_q = INT_MAX;
  VNX_PLAIN_LOOP for (int q = lane; q < Q; q += kWave) {
    if (assigned_only && !(m[q] & 1)) continue;
    const float v = col[q];
    if (best_q == INT_MAX || v < best) { best = v; best_q = q; }      // ascending q: a tie keeps the lower query
  }
  VNX_PLAIN_LOOP for (int off = 32; off > 0; off >>= 1) {
    const float ov = __shfl_xor(best, off, kWave);
    const int oq = __shfl_xor(best_q, off, kWave);
    if (oq != INT_MAX && (best_q == INT_MAX || ov < best || (ov == best && oq < best_q))) { best = ov; best_q = oq; }
  }
  return best_q;
}

// M[multi rows] = 0; M[multi rows, argmin over the row] = 1  (bit 0; the first minimum)
__device__ __forceinline__ void keep_cheapest(const OtaLds& s, int q, int n, int Q, int Qp) {
  float best = s.cost[q];
  int keep = 0;
  VNX_PLAIN_LOOP for (int c = 1; c < n; ++c) {
    const float v = s.cost[size_t(c) * Qp + q];
    if (v < best) { best = v; keep = c; }
  }
  VNX_PLAIN_LOOP for (int c = 0; c < n; ++c) {
    uint8_t* m = s.M + size_t(c) * Qp + q;
    *m = uint8_t((*m & 2) | (c == keep ? 1 : 0));
  }
}

__device__ __forceinline__ int row_count(const OtaLds& s, int q, int n, int Qp) {
  int cnt = 0;
  VNX_PLAIN_LOOP for (int c = 0; c < n; ++c) cnt += s.M[size_t(c) * Qp + q] & 1;
  return cnt;
}

// dynamic_k_matching(cost, iou, kc) on the cost block in LDS, which it modifies as the host form does.  Bit 0 of M is the
// result; bit 1 is kept when keep_bit1.  -> 0, or 2 when the repair loop reaches its bound.  Entered and left by all threads.
__device__ int dynamic_k(const OtaLds& s, int n, int Q, int kc, bool keep_bit1, const float* __restrict__ boxes,
                         const float* __restrict__ tgt_boxes, int off) {
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  const int Qp = pad4(Q);
  VNX_PLAIN_LOOP for (int c = 0; c < n; ++c) {
    const Box g = to_xyxy(*reinterpret_cast<const vnx_f4*>(tgt_boxes + size_t(off + s.inst[c]) * 4));
    const float* col = s.cost + size_t(c) * Qp;
    VNX_PLAIN_LOOP for (int q = tid; q < Q; q += kOtaThreads) {
      s.ikey[q] = order_key(pair_iou(to_xyxy(*reinterpret_cast<const vnx_f4*>(boxes + size_t(q) * 4)), g));
      s.ckey[q] = order_key(col[q]);
    }
    __syncthreads();
    VNX_PLAIN_LOOP for (int q = tid; q < Q; q += kOtaThreads) {
      const int vi = s.ikey[q], vc = s.ckey[q];
      int ri = 0, rc = 0;      // elements before q among the largest IoUs / the smallest costs
      VNX_PLAIN_LOOP for (int j = 0; j < Qp; j += 4) {       // 16-byte LDS reads, every lane the same address; the pads never count
        const vnx_i4 iv = *reinterpret_cast<const vnx_i4*>(s.ikey + j), cv = *reinterpret_cast<const vnx_i4*>(s.ckey + j);
        const int t0 = int(unsigned(j - q) >> 31), t1 = int(unsigned(j + 1 - q) >> 31);      // j < q
        const int t2 = int(unsigned(j + 2 - q) >> 31), t3 = int(unsigned(j + 3 - q) >> 31);
        ri += iv.x > vi - t0;
        ri += iv.y > vi - t1;
        ri += iv.z > vi - t2;
        ri += iv.w > vi - t3;
        rc += cv.x < vc + t0;
        rc += cv.y < vc + t1;
        rc += cv.z < vc + t2;
        rc += cv.w < vc + t3;
      }
      if (ri < kc) s.top[ri] = pair_iou(to_xyxy(*reinterpret_cast<const vnx_f4*>(boxes + size_t(q) * 4)), g);
      s.rank[q] = rc;
    }
    __syncthreads();
    float sum = 0.f;             // topk(iou, kc)[0].sum(0): largest first, every thread the same sum
    VNX_PLAIN_LOOP for (int r = 0; r < kc; ++r) sum += s.top[r];
    int k = int(sum);            // .int(): towards zero
    k = k < 1 ? 1 : k;
    VNX_PLAIN_LOOP for (int q = tid; q < Q; q += kOtaThreads) {
      uint8_t* m = s.M + size_t(c) * Qp + q;
      *m = uint8_t((keep_bit1 ? (*m & 2) : 0) | (s.rank[q] < k ? 1 : 0));
    }
    __syncthreads();
  }
  // queries claimed by several boxes: the mask the repair loop keeps using
  VNX_PLAIN_LOOP for (int q = tid; q < Q; q += kOtaThreads) {
    const bool multi = row_count(s, q, n, Qp) > 1;
    s.multi[q] = multi;
    if (multi) keep_cheapest(s, q, n, Q, Qp);
  }
  __syncthreads();
  VNX_PLAIN_LOOP for (int iter = 0;; ++iter) {
    VNX_PLAIN_LOOP for (int c = tid; c < n; c += kOtaThreads) s.col_has[c] = 0;
    __syncthreads();
    VNX_PLAIN_LOOP for (int q = tid; q < Q; q += kOtaThreads)
      VNX_PLAIN_LOOP for (int c = 0; c < n; ++c)
        if (s.M[size_t(c) * Qp + q] & 1) s.col_has[c] = 1;
    __syncthreads();
    bool empty = false;
    VNX_PLAIN_LOOP for (int c = 0; c < n; ++c) empty = empty || !s.col_has[c];
    if (!empty) return 0;
    if (iter >= n + 8) return 2;
    VNX_PLAIN_LOOP for (int q = tid; q < Q; q += kOtaThreads)
      if (row_count(s, q, n, Qp) > 0)
        VNX_PLAIN_LOOP for (int c = 0; c < n; ++c) s.cost[size_t(c) * Qp + q] += 100000.f;
    __syncthreads();
    VNX_PLAIN_LOOP for (int c = wave; c < n; c += kOtaWaves) {
      if (s.col_has[c]) continue;
      const int best = column_argmin(s, c, Q, Qp, false, lane);
      if (lane == 0) s.M[size_t(c) * Qp + best] |= 1;
    }
    __syncthreads();
    bool several = false;
    VNX_PLAIN_LOOP for (int q = tid; q < Q; q += kOtaThreads) several = several || row_count(s, q, n, Qp) > 1;
    if (block_any(s, several)) {
      VNX_PLAIN_LOOP for (int q = tid; q < Q; q += kOtaThreads)
        if (s.multi[q]) keep_cheapest(s, q, n, Q, Qp);
    }
    __syncthreads();
  }
}

// the whole stride of a problem without a result
__device__ void write_empty(const OtaArgs& a, int32_t* out, bool selection, int status, int n) {
  const int tid = threadIdx.x;
  const int ints = selection ? 2 + a.n_cap : a.stride;
  VNX_PLAIN_LOOP for (int i = 2 + tid; i < ints; i += kOtaThreads) out[i] = -1;
  VNX_PLAIN_LOOP for (int i = ints + tid; i < a.stride; i += kOtaThreads) out[i] = 0;
  if (tid == 0) { out[0] = status; out[1] = n; }
}

__global__ __launch_bounds__(kOtaThreads) void idol_match_kernel(OtaArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  const int p = blockIdx.x;
  const bool selection = p >= a.n_det;
  const int Q = a.Q, K = a.K, Qp = pad4(Q);
  int32_t* out = a.out + size_t(p) * a.stride;
  const int off = a.problems[2 * p], cnt = a.problems[2 * p + 1];
  if (cnt < 0 || off < 0 || cnt > a.n_tot || off > a.n_tot - cnt || cnt > a.n_cap || (selection && off < a.valid_first)) {
    write_empty(a, out, selection, 3, 0);      // outside the arrays or the LDS the launch asked for: nothing is addressed
    return;
  }
  if (cnt == 0) {
    write_empty(a, out, selection, 0, 0);
    return;
  }
  const OtaLds s = ota_carve(smem, a.n_cap, Q);
  const float* prob = selection ? a.ref_prob + size_t(p - a.n_det) * Q * K : a.det_prob + size_t(p) * Q * K;
  const float* boxes = selection ? a.ref_boxes + size_t(p - a.n_det) * Q * 4 : a.det_boxes + size_t(p) * Q * 4;
  // the problem's instances: all targets, or the valid ones in order
  if (selection) {
    const uint8_t* valid = a.valid + (off - a.valid_first);
    VNX_PLAIN_LOOP for (int t = tid; t < cnt; t += kOtaThreads) {
      int before = 0;
      VNX_PLAIN_LOOP for (int j = 0; j < t; ++j) before += valid[j] != 0;
      const bool v = valid[t] != 0;
      if (v) s.inst[before] = t;
      if (t == cnt - 1) s.misc[0] = before + (v ? 1 : 0);
    }
  } else {
    VNX_PLAIN_LOOP for (int t = tid; t < cnt; t += kOtaThreads) s.inst[t] = t;
    if (tid == 0) s.misc[0] = cnt;
  }
  __syncthreads();
  const int n = s.misc[0];
  if (n == 0) {
    write_empty(a, out, selection, 0, 0);
    return;
  }
  // the pads of the key rows the rank counts read four at a time: never smaller than a cost, never larger than an IoU
  if (tid < Qp - Q) {
    s.ckey[Q + tid] = order_key(__builtin_huge_valf());
    s.ikey[Q + tid] = order_key(-__builtin_huge_valf());
  }
  // ---- ota_cost ----------------------------------------------------------------------------------------------------
  const float r = 2.5f / 32.f;                 // center_radius / expanded_strides
  bool bad = false, bad_label = false;
  VNX_PLAIN_LOOP for (int q = tid; q < Q; q += kOtaThreads) {
    const vnx_f4 qb = *reinterpret_cast<const vnx_f4*>(boxes + size_t(q) * 4);
    const Box b = to_xyxy(qb);
    const float cx = qb.x, cy = qb.y;
    bool in_any_box = false, in_any_ctr = false;
    VNX_PLAIN_LOOP for (int c = 0; c < n; ++c) {
      const int t = off + s.inst[c];
      const vnx_f4 gb = *reinterpret_cast<const vnx_f4*>(a.tgt_boxes + size_t(t) * 4);
      const Box g = to_xyxy(gb);
      const int64_t label = a.labels[t];
      if (label < 0 || label >= K) { bad_label = true; continue; }
      // in_boxes_info: eight strict comparisons
      const bool in_box = (cx > g.x0) & (cx < g.x1) & (cy > g.y0) & (cy < g.y1);
      const bool in_ctr = (cx > gb.x - r) & (cx < gb.x + r) & (cy > gb.y - r) & (cy < gb.y + r);
      in_any_box |= in_box;
      in_any_ctr |= in_ctr;
      // focal class cost: alpha 0.25, gamma 2, 1e-8 inside both logs
      const float pr = prob[size_t(q) * K + label];
      const float neg = 0.75f * (pr * pr) * -logf(1.f - pr + 1e-8f);
      const float pos = 0.25f * ((1.f - pr) * (1.f - pr)) * -logf(pr + 1e-8f);
      float inter, uni;
      iou_terms(b, g, inter, uni);
      const float iou = inter / uni;
      const float hw = fmaxf(fmaxf(b.x1, g.x1) - fminf(b.x0, g.x0), 0.f), hh = fmaxf(fmaxf(b.y1, g.y1) - fminf(b.y0, g.y0), 0.f);
      const float hull = hw * hh;
      const float giou = iou - (hull - uni) / (hull + 1e-7f);
      const float cost = (pos - neg) + 3.f * -giou + ((in_box & in_ctr) ? 0.f : 100.f);
      bad = bad || !isfinite(cost) || !isfinite(iou);
      s.cost[size_t(c) * Qp + q] = cost;
    }
    if (!(in_any_box | in_any_ctr))
      VNX_PLAIN_LOOP for (int c = 0; c < n; ++c) s.cost[size_t(c) * Qp + q] += 10000.f;
  }
  const bool any_label = block_any(s, bad_label);
  if (block_any(s, bad) || any_label) {
    write_empty(a, out, selection, any_label ? 3 : 1, n);
    return;
  }
  // ---- the matching(s) ---------------------------------------------------------------------------------------------
  int status = 0;
  VNX_PLAIN_LOOP for (int pass = 0; pass < (selection ? 2 : 1) && status == 0; ++pass) {
    if (pass == 1) {
      VNX_PLAIN_LOOP for (int q = tid; q < Q; q += kOtaThreads)     // keep the first pass's matching in bit 1
        VNX_PLAIN_LOOP for (int c = 0; c < n; ++c) {
          uint8_t* m = s.M + size_t(c) * Qp + q;
          *m = (*m & 1) ? 3 : 0;
        }
      __syncthreads();
    }
    status = dynamic_k(s, n, Q, pass ? 100 : 10, pass == 1, boxes, a.tgt_boxes, off);
  }
  if (status != 0) {
    write_empty(a, out, selection, status, n);
    return;
  }
  // ---- outputs -------------------------------------------------------------------------------------------------------
  if (!selection) {
    VNX_PLAIN_LOOP for (int q = tid; q < Q; q += kOtaThreads) {
      int g = -1;
      VNX_PLAIN_LOOP for (int c = n - 1; c >= 0; --c)
        if (s.M[size_t(c) * Qp + q] & 1) g = c;
      out[2 + q] = g;
    }
    VNX_PLAIN_LOOP for (int c = wave; c < n; c += kOtaWaves) {
      const int best = column_argmin(s, c, Q, Qp, true, lane);
      if (lane == 0) out[2 + Q + c] = best;
    }
    VNX_PLAIN_LOOP for (int i = 2 + Q + n + tid; i < a.stride; i += kOtaThreads) out[i] = -1;
  } else {
    VNX_PLAIN_LOOP for (int c = tid; c < a.n_cap; c += kOtaThreads) out[2 + c] = c < n ? s.inst[c] : -1;
    uint8_t* bytes = reinterpret_cast<uint8_t*>(out + 2 + a.n_cap);
    VNX_PLAIN_LOOP for (int c = 0; c < n; ++c)
      VNX_PLAIN_LOOP for (int q = tid; q < Q; q += kOtaThreads) {
        const uint8_t m = s.M[size_t(c) * Qp + q];
        bytes[size_t(c) * Q + q] = uint8_t(((m >> 1) & 1) | ((m & 1) ? 0 : 2));
      }
    const size_t total = size_t(a.stride - 2 - a.n_cap) * 4;
    VNX_PLAIN_LOOP for (size_t i = size_t(n) * Q + tid; i < total; i += kOtaThreads) bytes[i] = 0;
  }
  if (tid == 0) { out[0] = 0; out[1] = n; }
}

}  // namespace

}  // namespace vnx

using namespace vnx;

extern "C" int vnx_idol_match_max_targets(int queries) {      // targets of one problem at most
  if (queries < 1) return 0;
  int n = 0;
  while (ota_lds_bytes(n + 1, queries) <= kOtaLdsBytes) ++n;
  return n;
}

extern "C" int vnx_idol_match_out_words(int targets_max, int queries) {      // int32 words of one problem's output
  return targets_max < 0 || queries < 1 ? 0 : ota_out_words(targets_max, queries);
}

extern "C" int vnx_idol_match(const void* det_prob, const void* det_boxes, const void* ref_prob, const void* ref_boxes,
                              const void* target_boxes, const void* labels, const void* valid, const void* problems,
                              int det_problems, int ref_problems, int queries, int classes, int targets_total,
                              int valid_first, int targets_max, void* out, int out_stride, void* hip_stream) {
  const char* fn = "vnx_idol_match";
  if (det_problems < 0 || ref_problems < 0 || queries < 1 || classes < 1 || targets_total < 0 || targets_max < 0 ||
      targets_max > targets_total || valid_first < 0 || valid_first > targets_total) {
    set_error("%s: bad sizes (%d + %d problems, queries %d, classes %d, targets %d, first reference target %d, largest "
              "problem %d)", fn, det_problems, ref_problems, queries, classes, targets_total, valid_first, targets_max);
    return VNX_ERR_INVALID_ARGUMENT;
  }
  const int64_t P = int64_t(det_problems) + ref_problems;
  if (P == 0) return VNX_OK;
  if (targets_max > 0 && (queries < 10 || (ref_problems > 0 && queries < 100))) {
    set_error("%s: %d queries: the matching takes the 10 largest IoUs of a column, the selection the 100 largest", fn, queries);
    return VNX_ERR_UNSUPPORTED;
  }
  if (ota_lds_bytes(targets_max, queries) > kOtaLdsBytes) {
    set_error("%s: %d targets of one problem against %d queries: at most %d fit the LDS of a CU", fn, targets_max, queries,
              vnx_idol_match_max_targets(queries));
    return VNX_ERR_UNSUPPORTED;
  }
  if (P >= (int64_t(1) << 24) || int64_t(queries) * classes >= (int64_t(1) << 31) || int64_t(queries) >= (int64_t(1) << 20)) {
    set_error("%s: %lld problems of %d x %d are outside what the kernel addresses", fn, (long long)P, queries, classes);
    return VNX_ERR_UNSUPPORTED;
  }
  if (out_stride < ota_out_words(targets_max, queries)) {
    set_error("%s: out_stride %d < the %d words of a problem", fn, out_stride, ota_out_words(targets_max, queries));
    return VNX_ERR_INVALID_ARGUMENT;
  }
  if (!problems || !out || (det_problems && (!det_prob || !det_boxes)) || (ref_problems && (!ref_prob || !ref_boxes)) ||
      (targets_total && (!target_boxes || !labels)) || (ref_problems && targets_total > valid_first && !valid)) {
    set_error("%s: null pointer argument", fn);
    return VNX_ERR_INVALID_ARGUMENT;
  }
  const size_t lds = ota_lds_bytes(targets_max, queries);
  if (lds > 64 * 1024) {      // more than 64 KB of dynamic LDS has to be asked for, once per device
    constexpr int kDevices = 64;
    static std::atomic<bool> asked[kDevices];
    int device = -1;
    if (hipGetDevice(&device) != hipSuccess || device < 0) device = -1;
    if (device < 0 || device >= kDevices || !asked[device].load(std::memory_order_acquire)) {
      const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(idol_match_kernel),
                                               hipFuncAttributeMaxDynamicSharedMemorySize, int(kOtaLdsBytes));
      if (e != hipSuccess) {      // this size cannot run here: the caller matches on the host, as for a problem above the cap
        (void)hipGetLastError();
        set_error("%s: %zu bytes of LDS for %d targets: hipFuncSetAttribute(max dynamic LDS) failed: %s", fn, lds, targets_max,
                  hipGetErrorString(e));
        return VNX_ERR_UNSUPPORTED;
      }
      if (device >= 0 && device < kDevices) asked[device].store(true, std::memory_order_release);
    }
  }
  const OtaArgs a{(const float*)det_prob, (const float*)det_boxes, (const float*)ref_prob, (const float*)ref_boxes,
                  (const float*)target_boxes, (const int64_t*)labels, (const uint8_t*)valid, (const int32_t*)problems,
                  (int32_t*)out, det_problems, ref_problems, queries, classes, targets_total, valid_first, targets_max,
                  out_stride};
  hipLaunchKernelGGL(idol_match_kernel, dim3(unsigned(P)), dim3(kOtaThreads), lds, (hipStream_t)hip_stream, a);
  return check_launch(fn);
}
