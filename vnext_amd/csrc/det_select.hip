// det_select.hip -- per-image detection selection on the device: best class per query, score threshold, class-aware
// greedy box NMS and (COCO mode) the top-k over (kept query, class).
//
// One launch for a batch of images, ONE WORKGROUP OF FOUR WAVE64 PER IMAGE.  It serves the two selections of IDOL's
// inference (vnext_amd/models/idol.py):
//   video (IDOL.select_candidates): candidates = queries whose best class score is > score_thr, the single best query when
//          there is none (no NMS then), class-aware NMS at iou_thr, no top-k (topk = 0)
//   COCO  (IDOL.coco_postprocess):  score_thr < 0 (every sigmoid is above it: every query is a candidate), NMS, then the
//          min(topk, kept * K) largest class scores of the kept queries
//
// Arithmetic.  fp32, operation by operation as the host expression (box_cxcywh_to_xyxy, class_aware_nms), contraction off
// for the whole file and IEEE division: `iou > thr` is bit-identical to the host's on the same inputs (0 / 0 is NaN: two
// zero-size boxes suppress nothing).  Orders are taken on the LOGIT as an ordered integer, never on its sigmoid (monotone,
// and defined where fp32 sigmoids collide); every choice among equal values goes to the LOWER index.  The score test is
// 1 / (1 + expf(-max logit)) > score_thr.
//
// Steps of an image (Q queries, K classes, n candidates, W = ceil(n / 64)):
//   1. max logit and first argmax of every query: 16 / 4 / 1 lanes per query by K, consecutive classes on consecutive lanes
//   2. rank of every candidate in (logit descending, query ascending) order: a rank count on the integer keys, Q x Q
//      comparisons over the four waves against 16-byte LDS broadcast reads (as ota_match.hip); boxes, areas and labels are
//      scattered to LDS in that order
//   3. the suppression relation as a bit matrix in LDS: one __ballot word per (row i, 64 candidates after i); only the
//      words from i / 64 on exist (block-triangular storage: half the square)
//   4. one wave walks the rows block by block: the 64 diagonal words of a block are held one per lane and resolved with
//      lane reads alone (a removed row suppresses nothing: greedy), then every later word of the live rows is OR-reduced
//      across the wave into the `removed` bit set
//   5. COCO mode: radix select (8-bit digits, LDS histogram of integer counts) on the 56-bit key (logit key, then the
//      lower flat index position_in_kept_order * K + class first), which stops at the first digit whose bucket is taken
//      whole; the at most `topk` survivors are rank-sorted
// The integer LDS counters make no result depend on their order; all global results are plain vector stores: the output is
// a function of the input alone.
//
// LDS (det_lds_bytes; Qp = Q rounded up to 4, Wq = ceil(Q / 64)): 256 Wq (Wq + 1) bytes of bit matrix + 40 Qp + 8 Wq +
// about 3.2 KB: 22.8 KB at Q = 300, 114 KB at Q = 1024; the 160 KB of a CU hold Q = 1280.
//
// Output, int32 words, `stride` per image (det_out_words = 4 + 2 Q + 2 topk):
//   [0] status (0 ok, 1 a non-finite logit or box: nothing selected)  [1] kept  [2] top-k entries  [3] 0
//   [4, 4+Q) kept queries in NMS order then -1   [4+Q, 4+2Q) every query's label (-1 with status 1)
//   then topk pairs (query, class), the unused ones -1.  Words beyond are not written.
#include <limits.h>

#include "vnx_common.h"

#pragma clang fp contract(off)

#define VNX_PLAIN_LOOP _Pragma("clang loop unroll(disable) vectorize(disable) interleave(disable)")

namespace vnx {
namespace {

constexpr int kDetThreads = 256;
constexpr int kDetWaves = kDetThreads / kWave;
constexpr int kDetTopMax = 256;                   // top-k entries at most (one thread each in the final rank sort)
constexpr int kDetMaxClasses = 4096;
constexpr int kDetFlatBits = 24;                  // Q * K < 2^24: the flat index field of the top-k key
constexpr size_t kDetLdsBytes = 160 * 1024;       // LDS of a gfx950 CU

typedef unsigned long long u64;
typedef int det_i4 __attribute__((ext_vector_type(4)));

__host__ __device__ inline int det_words(int n) { return (n + 63) >> 6; }
// rows of block b (64 rows) hold the words b .. W-1: the first word of row i
__host__ __device__ inline int det_row_offset(int i, int W) {
  const int b = i >> 6;
  return 64 * (b * W - b * (b - 1) / 2) + (i & 63) * (W - b);
}
__host__ __device__ inline size_t det_lds_bytes(int Q) {
  const size_t Qp = pad4(Q), W = det_words(Q);
  return 8 * (64 * W * (W + 1) / 2) + 8 * ((W + 1) & ~size_t(1)) + 16 * Qp + 6 * 4 * Qp + 8 * kDetTopMax + 4 * 256 + 64;
}
__host__ __device__ inline int det_out_words(int Q, int topk) { return 4 + 2 * Q + 2 * topk; }

struct DetArgs {
  const float* logits;      // [B][Q][K]
  const float* boxes;       // [B][Q][4] cxcywh
  int32_t* out;             // [B][stride]
  int Q, K, topk, stride;
  float score_thr, iou_thr;
};

struct DetLds {
  u64* mat;         // block-triangular bit matrix
  u64* rem;         // [W] removed bits
  vnx_f4* sbox;     // [Qp] xyxy in candidate order
  int* key;         // [Qp] max logit as an ordered integer, INT_MIN = no candidate (and the pad)
  int* label;       // [Qp]
  int* ord;         // [Qp] candidate order -> query
  float* sarea;     // [Qp]
  int* slabel;      // [Qp]
  int* kq;          // [Qp] kept order -> query (before that: the candidate flags)
  u64* sel;         // [kDetTopMax]
  int* hist;        // [256]
  int* misc;        // [16]: 0-3 wave sums, 4 flag, 5 digit, 6 remaining, 7 bucket, 8 slot counter
};

__device__ __forceinline__ DetLds det_carve(unsigned char* smem, int Q) {
  const size_t Qp = pad4(Q), W = det_words(Q);
  DetLds s;
  s.mat = reinterpret_cast<u64*>(smem);
  s.rem = s.mat + 64 * W * (W + 1) / 2;
  s.sbox = reinterpret_cast<vnx_f4*>(s.rem + ((W + 1) & ~size_t(1)));
  s.key = reinterpret_cast<int*>(s.sbox + Qp);
  s.label = s.key + Qp;
  s.ord = s.label + Qp;
  s.sarea = reinterpret_cast<float*>(s.ord + Qp);
  s.slabel = reinterpret_cast<int*>(s.sarea + Qp);
  s.kq = s.slabel + Qp;
  s.sel = reinterpret_cast<u64*>(s.kq + Qp);
  s.hist = reinterpret_cast<int*>(s.sel + kDetTopMax);
  s.misc = s.hist + 256;
  return s;
}

__device__ __forceinline__ int det_wave_sum(int v) {
  VNX_PLAIN_LOOP for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, kWave);
  return v;
}

// sum over the workgroup, the same on every thread (misc[0..3]; free again on return)
__device__ __forceinline__ int det_block_sum(const DetLds& s, int v) {
  v = det_wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & (kWave - 1)) == 0) s.misc[threadIdx.x / kWave] = v;
  __syncthreads();
  const int r = s.misc[0] + s.misc[1] + s.misc[2] + s.misc[3];
  __syncthreads();
  return r;
}

__device__ __forceinline__ u64 det_readlane(u64 v, int lane) {      // lane uniform
  const unsigned lo = unsigned(__builtin_amdgcn_readlane(int(unsigned(v)), lane));
  const unsigned hi = unsigned(__builtin_amdgcn_readlane(int(unsigned(v >> 32)), lane));
  return (u64(hi) << 32) | lo;
}

__device__ __forceinline__ u64 det_wave_or(u64 v) {
  unsigned lo = unsigned(v), hi = unsigned(v >> 32);
  VNX_PLAIN_LOOP for (int off = 32; off > 0; off >>= 1) {
    lo |= unsigned(__shfl_xor(int(lo), off, kWave));
    hi |= unsigned(__shfl_xor(int(hi), off, kWave));
  }
  return (u64(hi) << 32) | lo;
}

// the top-k key of flat entry i: (logit key as unsigned, larger first) then (flat index, lower first)
__device__ __forceinline__ u64 det_topk_key(const DetLds& s, const float* __restrict__ logits, int K, int i) {
  const int p = int(unsigned(i) / unsigned(K)), c = i - p * K;
  const float v = logits[size_t(s.kq[p]) * K + c];
  const unsigned uk = unsigned(order_key(v)) ^ 0x80000000u;
  return (u64(uk) << kDetFlatBits) | u64(((1u << kDetFlatBits) - 1u) - unsigned(i));
}

__global__ __launch_bounds__(kDetThreads) void det_select_kernel(DetArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  const int Q = a.Q, K = a.K, Qp = pad4(Q);
  const DetLds s = det_carve(smem, Q);
  const float* logits = a.logits + size_t(blockIdx.x) * Q * K;
  const float* boxes = a.boxes + size_t(blockIdx.x) * Q * 4;
  int32_t* out = a.out + size_t(blockIdx.x) * a.stride;
  int32_t* out_top = out + 4 + 2 * Q;

  // ---- 1. best class of every query, the candidate flags ---------------------------------------------------------------
  const int G = K >= 32 ? 16 : K >= 8 ? 4 : 1;      // lanes per query
  const int per = kDetThreads / G, g = tid & (G - 1), slot = tid / G;
  bool bad = false;
  int mine = 0;
  VNX_PLAIN_LOOP for (int q0 = 0; q0 < Q; q0 += per) {      // uniform trip count: the shuffles below see every lane
    const int q = q0 + slot;
    float best = -__builtin_huge_valf();
    int bc = INT_MAX;
    if (q < Q) {
      const float* row = logits + size_t(q) * K;
      for (int c = g; c < K; c += G) {
        const float v = row[c];
        bad = bad || !isfinite(v);
        if (bc == INT_MAX || v > best) { best = v; bc = c; }      // ascending c: equal maxima keep the lower class
      }
    }
    VNX_PLAIN_LOOP for (int off = G >> 1; off > 0; off >>= 1) {
      const float ov = __shfl_xor(best, off, kWave);
      const int oc = __shfl_xor(bc, off, kWave);
      if (oc != INT_MAX && (bc == INT_MAX || ov > best || (ov == best && oc < bc))) { best = ov; bc = oc; }
    }
    if (q < Q && g == 0) {
      const bool cand = 1.f / (1.f + expf(-best)) > a.score_thr;
      s.key[q] = order_key(best);
      s.label[q] = bc;
      s.kq[q] = cand;
      mine += cand;
    }
  }
  VNX_PLAIN_LOOP for (int q = tid; q < Q; q += kDetThreads) {
    const vnx_f4 b = *reinterpret_cast<const vnx_f4*>(boxes + size_t(q) * 4);
    bad = bad || !isfinite(b.x) || !isfinite(b.y) || !isfinite(b.z) || !isfinite(b.w);
  }
  if (det_block_sum(s, bad ? 1 : 0) != 0) {
    VNX_PLAIN_LOOP for (int i = 4 + tid; i < 4 + 2 * Q + 2 * a.topk; i += kDetThreads) out[i] = -1;
    if (tid < 4) out[tid] = tid == 0 ? 1 : 0;
    return;
  }
  const int n_cand = det_block_sum(s, mine);
  const bool single = n_cand == 0;      // nothing above the threshold: the best query alone, no NMS
  const int n = single ? 1 : n_cand;
  VNX_PLAIN_LOOP for (int q = tid; q < Qp; q += kDetThreads)
    if (q >= Q || !(single || s.kq[q])) s.key[q] = INT_MIN;
  __syncthreads();

  // ---- 2. candidate order: rank counts on the keys, boxes / areas / labels scattered in that order ----------------------
  VNX_PLAIN_LOOP for (int q = tid; q < Q; q += kDetThreads) {
    const int vq = s.key[q];
    if (vq == INT_MIN) continue;
    int r = 0;      // candidates before q: a larger key, or the same key and a lower index
    VNX_PLAIN_LOOP for (int j = 0; j < Qp; j += 4) {
      const det_i4 kv = *reinterpret_cast<const det_i4*>(s.key + j);
      r += kv.x > vq - int(unsigned(j - q) >> 31);
      r += kv.y > vq - int(unsigned(j + 1 - q) >> 31);
      r += kv.z > vq - int(unsigned(j + 2 - q) >> 31);
      r += kv.w > vq - int(unsigned(j + 3 - q) >> 31);
    }
    const vnx_f4 b = *reinterpret_cast<const vnx_f4*>(boxes + size_t(q) * 4);
    const float hw = 0.5f * b.z, hh = 0.5f * b.w;      // box_cxcywh_to_xyxy: c - 0.5 * wh, c + 0.5 * wh
    const vnx_f4 x = {b.x - hw, b.y - hh, b.x + hw, b.y + hh};
    s.ord[r] = q;
    s.sbox[r] = x;
    s.sarea[r] = (x.z - x.x) * (x.w - x.y);
    s.slabel[r] = s.label[q];
  }
  __syncthreads();

  // ---- 3. suppression bits: word (i, w) = candidates j in [64 w, 64 w + 64) after i that i removes ------------------------
  const int W = det_words(n);
  if (n > 1) {
    VNX_PLAIN_LOOP for (int i = wave; i < n; i += kDetWaves) {
      const vnx_f4 bi = s.sbox[i];
      const float ai = s.sarea[i];
      const int li = s.slabel[i];
      u64* row = s.mat + det_row_offset(i, W);
      VNX_PLAIN_LOOP for (int w = i >> 6; w < W; ++w) {
        const int j = w * 64 + lane;
        bool hit = false;
        if (j > i && j < n && s.slabel[j] == li) {
          const vnx_f4 bj = s.sbox[j];
          const float iw = fmaxf(fminf(bi.z, bj.z) - fmaxf(bi.x, bj.x), 0.f);
          const float ih = fmaxf(fminf(bi.w, bj.w) - fmaxf(bi.y, bj.y), 0.f);
          const float inter = iw * ih;
          hit = inter / (ai + s.sarea[j] - inter) > a.iou_thr;
        }
        const u64 word = __ballot(hit);
        if (lane == 0) row[w - (i >> 6)] = word;
      }
    }
  }
  __syncthreads();

  // ---- 4. the greedy walk, by one wave: lane w holds word w of `removed` ---------------------------------------------
  if (wave == 0) {
    u64 remw = 0;
    if (n == 1) {
      remw = lane == 0 ? ~u64(1) : 0;
    } else {
      VNX_PLAIN_LOOP for (int b = 0; b < W; ++b) {
        const int i = b * 64 + lane;
        const u64 diag = i < n ? s.mat[det_row_offset(i, W)] : 0;      // row i's word b
        u64 cur = det_readlane(remw, b);
        if (n - b * 64 < 64) cur |= ~u64(0) << (n - b * 64);          // positions past the last candidate
        u64 todo = __ballot(diag != 0);
        while (todo) {                                               // ascending rows; a removed row suppresses nothing
          const int k = __builtin_ctzll(todo);
          todo &= todo - 1;
          if (!((cur >> k) & 1)) cur |= det_readlane(diag, k);
        }
        const bool live = !((cur >> lane) & 1);
        VNX_PLAIN_LOOP for (int w = b + 1; w < W; ++w) {
          const u64 part = live ? s.mat[det_row_offset(i, W) + (w - b)] : 0;
          const u64 all = det_wave_or(part);
          if (lane == w) remw |= all;
        }
        if (lane == b) remw = cur;
      }
    }
    if (lane < W) s.rem[lane] = remw;
  }
  __syncthreads();

  // ---- kept queries in NMS order -------------------------------------------------------------------------------------------
  int kept = 0;
  VNX_PLAIN_LOOP for (int w = 0; w < W; ++w) kept += __builtin_popcountll(~s.rem[w]);
  VNX_PLAIN_LOOP for (int i = tid; i < n; i += kDetThreads) {
    const u64 word = s.rem[i >> 6];
    if ((word >> (i & 63)) & 1) continue;
    int pos = __builtin_popcountll(~word & ((u64(1) << (i & 63)) - 1));
    VNX_PLAIN_LOOP for (int w = 0; w < (i >> 6); ++w) pos += __builtin_popcountll(~s.rem[w]);
    s.kq[pos] = s.ord[i];
  }
  __syncthreads();
  VNX_PLAIN_LOOP for (int r = tid; r < Q; r += kDetThreads) {
    out[4 + r] = r < kept ? s.kq[r] : -1;
    out[4 + Q + r] = s.label[r];
  }

  // ---- 5. top-k over (kept query, class) ---------------------------------------------------------------------------------
  const int items = kept * K;
  const int ntop = a.topk < items ? a.topk : items;
  if (tid == 0) { out[0] = 0; out[1] = kept; out[2] = ntop; out[3] = 0; }
  if (a.topk == 0) return;
  u64 prefix = 0, thr = 0;
  int need = ntop;
  VNX_PLAIN_LOOP for (int shift = 48; shift >= 0; shift -= 8) {
    s.hist[tid] = 0;
    if (tid == 0) s.misc[8] = 0;
    __syncthreads();
    VNX_PLAIN_LOOP for (int i0 = tid; i0 < items; i0 += 4 * kDetThreads) {
      u64 c[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int i = i0 + u * kDetThreads;
        c[u] = i < items ? det_topk_key(s, logits, K, i) : 0;
      }
#pragma unroll
      for (int u = 0; u < 4; ++u)
        if (i0 + u * kDetThreads < items && ((c[u] >> shift) >> 8) == prefix) atomicAdd(&s.hist[int(c[u] >> shift) & 255], 1);
    }
    __syncthreads();
    // entries in the buckets above 255 - tid, and in that bucket: the digit is where the count reaches `need`
    const int v = s.hist[255 - tid];
    int incl = v;
    VNX_PLAIN_LOOP for (int off = 1; off < kWave; off <<= 1) {
      const int o = __shfl_up(incl, off, kWave);
      if (lane >= off) incl += o;
    }
    if (lane == kWave - 1) s.misc[wave] = incl;
    __syncthreads();
    VNX_PLAIN_LOOP for (int w = 0; w < wave; ++w) incl += s.misc[w];
    if (incl >= need && incl - v < need) { s.misc[5] = 255 - tid; s.misc[6] = need - (incl - v); s.misc[7] = v; }
    __syncthreads();
    prefix = (prefix << 8) | u64(s.misc[5]);
    need = s.misc[6];
    const bool whole = s.misc[7] == need;
    thr = prefix << shift;
    __syncthreads();
    if (whole || shift == 0) break;      // the whole bucket is taken: everything at or above its first key
  }
  VNX_PLAIN_LOOP for (int i = tid; i < items; i += kDetThreads) {
    const u64 c = det_topk_key(s, logits, K, i);
    if (c >= thr) {
      const int at = atomicAdd(&s.misc[8], 1);
      if (at < kDetTopMax) s.sel[at] = c;
    }
  }
  __syncthreads();
  if (tid < ntop) {
    const u64 c = s.sel[tid];
    int r = 0;
    VNX_PLAIN_LOOP for (int j = 0; j < ntop; ++j) r += s.sel[j] > c;      // the keys are distinct
    const int flat = int(((1u << kDetFlatBits) - 1u) - unsigned(c & ((u64(1) << kDetFlatBits) - 1)));
    const int p = int(unsigned(flat) / unsigned(K));
    if (p < kept) {
      out_top[2 * r] = s.kq[p];
      out_top[2 * r + 1] = flat - p * K;
    }
  }
  VNX_PLAIN_LOOP for (int i = 2 * ntop + tid; i < 2 * a.topk; i += kDetThreads) out_top[i] = -1;
}

}  // namespace

}  // namespace vnx

using namespace vnx;

extern "C" int vnx_det_select_out_words(int queries, int topk) {      // int32 words of one image's output
  return queries < 1 || topk < 0 ? 0 : det_out_words(queries, topk);
}

extern "C" int vnx_det_select(const void* logits, const void* boxes, int batch, int queries, int classes, float score_thr,
                              float iou_thr, int topk, void* out, int out_stride, void* hip_stream) {
  const char* fn = "vnx_det_select";
  if (batch < 0 || queries < 1 || classes < 1 || topk < 0) {
    set_error("%s: bad sizes (batch %d, queries %d, classes %d, topk %d)", fn, batch, queries, classes, topk);
    return VNX_ERR_INVALID_ARGUMENT;
  }
  if (batch == 0) return VNX_OK;
  if (classes > kDetMaxClasses || topk > kDetTopMax || int64_t(queries) * classes >= (int64_t(1) << kDetFlatBits)) {
    set_error("%s: %d queries x %d classes, topk %d: at most %d classes, queries x classes below 2^%d, topk at most %d", fn,
              queries, classes, topk, kDetMaxClasses, kDetFlatBits, kDetTopMax);
    return VNX_ERR_UNSUPPORTED;
  }
  if (det_lds_bytes(queries) > kDetLdsBytes) {
    set_error("%s: %d queries need %zu bytes of LDS, a CU has %zu", fn, queries, det_lds_bytes(queries), kDetLdsBytes);
    return VNX_ERR_UNSUPPORTED;
  }
  if (int64_t(batch) * queries * classes >= (int64_t(1) << 40)) {
    set_error("%s: %d images of %d x %d are outside what the kernel addresses", fn, batch, queries, classes);
    return VNX_ERR_UNSUPPORTED;
  }
  if (out_stride < det_out_words(queries, topk)) {
    set_error("%s: out_stride %d < the %d words of an image", fn, out_stride, det_out_words(queries, topk));
    return VNX_ERR_INVALID_ARGUMENT;
  }
  if (!logits || !boxes || !out) {
    set_error("%s: null pointer argument", fn);
    return VNX_ERR_INVALID_ARGUMENT;
  }
  if ((reinterpret_cast<uintptr_t>(boxes) & 15) != 0) {
    set_error("%s: boxes must be 16-byte aligned", fn);
    return VNX_ERR_INVALID_ARGUMENT;
  }
  const size_t lds = det_lds_bytes(queries);
  if (lds > 64 * 1024) {      // more than 64 KB of dynamic LDS has to be asked for, once per device
    constexpr int kDevices = 64;
    static std::atomic<bool> asked[kDevices];
    int device = -1;
    if (hipGetDevice(&device) != hipSuccess || device < 0) device = -1;
    if (device < 0 || device >= kDevices || !asked[device].load(std::memory_order_acquire)) {
      const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(det_select_kernel),
                                               hipFuncAttributeMaxDynamicSharedMemorySize, int(kDetLdsBytes));
      if (e != hipSuccess) {
        (void)hipGetLastError();
        set_error("%s: %zu bytes of LDS for %d queries: hipFuncSetAttribute(max dynamic LDS) failed: %s", fn, lds, queries,
                  hipGetErrorString(e));
        return VNX_ERR_UNSUPPORTED;
      }
      if (device >= 0 && device < kDevices) asked[device].store(true, std::memory_order_release);
    }
  }
  const DetArgs a{(const float*)logits, (const float*)boxes, (int32_t*)out, queries, classes, topk, out_stride, score_thr,
                  iou_thr};
  hipLaunchKernelGGL(det_select_kernel, dim3(unsigned(batch)), dim3(kDetThreads), lds, (hipStream_t)hip_stream, a);
  return check_launch(fn);
}
