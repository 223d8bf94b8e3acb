// self_attn.hip -- the self-attention over the object queries of a deformable-transformer DECODER layer, scores to context in
// ONE pass, and its backward in one launch (the glue of the 6 + 6 layer stack; VERDICT r4
// item 6).
//
// Reference: `tgt2 = self.self_attn(q.transpose(0, 1), k.transpose(0, 1), tgt.transpose(0, 1))[0].transpose(0, 1)` with
// q = k = tgt + query_pos (projects/SeqFormer/seqformer/models/deformable_transformer.py:286-323 and the `_box` twin,
// IDOL's decoder layer the same): nn.MultiheadAttention over 300 queries, 8 heads of 32 channels, dropout 0.1 on the attention
// probabilities.  ATen runs, per call, three projections on transposed copies, a scale, a batched GEMM, softmax, dropout, a
// batched GEMM, a copy back and -- `need_weights` defaults to True -- a mean over the heads that nobody reads: 18 launches
// forward, about 27 backward, twelve calls per SeqFormer step (box queries: 80 (batch, head) pairs of 300 x 300 scores each).
//
// Here the caller hands over the projected rows [rows = batch * queries][3 C] (q | k | v, C = 32 heads' channels, no bias) and
// the in-projection bias; one kernel does bias + scale + scores + softmax + dropout + context for all heads, keeping the
// 300 x 300 probabilities in registers (online softmax: they are never written), and one kernel the whole backward,
// recomputing them from the saved log-sum-exp.
//   * forward: a workgroup = 32 query rows of one (batch, head), 8 lanes per row; lane j of a row takes keys j, j + 8, ... --
//     a whole 32-channel dot per lane, NO cross-lane traffic per key -- with the keys / values of the head staged through LDS in
//     chunks of 64 rows padded to 36 floats (the 8 rows a wave instruction reads then fall into 8 different bank quads).  The 8
//     partial (max, sum, context) states of a row are merged once at the end.
//   * backward, one launch, two kinds of workgroups: "query" workgroups (same map) compute grad_q; "key" workgroups own 32 key
//     rows, 8 lanes per row over the queries, and compute grad_k and grad_v.  Both recompute the probabilities from q, k and the
//     log-sum-exp; D_i = <grad_out_i, out_i> is recomputed where it is needed.
//   * dropout: keep(b, h, i, j) = hash(seed, element) >= p 2^32, the hash and the seed handling of add_norm.hip: no mask stored.
// Arithmetic: 2 x 300 x 300 x 32 x 2 flops per (batch, head) forward -- vector FMAs, not MFMA: the whole call is 0.9 GFLOP at
// the box-query shape and the point is the 40 launches it replaces, not the matrix rate.
#include "vnx_common.h"

namespace vnx {

typedef float sa_f4 __attribute__((ext_vector_type(4)));
typedef float sa_f2 __attribute__((ext_vector_type(2)));

constexpr int kSaHd = 32;            // channels per head
constexpr int kSaRows = 32;          // query (or key) rows per workgroup
constexpr int kSaLanes = 8;          // lanes per row
constexpr int kSaThreads = kSaRows * kSaLanes;
constexpr int kSaChunk = 64;         // rows staged in LDS per step
constexpr int kSaPad = 36;           // floats per staged row (144 B: the 8 rows a wave instruction reads hit 8 different bank quads)
constexpr int kSaPerLane = kSaChunk / kSaLanes;
constexpr float kSaLowest = -1.0e30f;

// keep the probability of (row of the [batch * heads * queries] list, key)?  The 64-bit element index is split: its low 32
// bits are hashed, the rest is mixed into the seed.
__device__ __forceinline__ bool sa_keep(uint32_t bh_row, uint32_t key, uint32_t nq, uint32_t threshold, uint32_t seed_lo,
                                        uint32_t seed_hi) {
  const uint64_t e = uint64_t(bh_row) * nq + key;
  return dropout_hash(uint32_t(e), seed_lo, seed_hi ^ (uint32_t(e >> 32) * 0x9E3779B1u)) >= threshold;
}

struct SaArgs {
  const float* qkv;      // [B * Q][ld]: q at column 0, k at C, v at 2 C (C = 32 H); the in-projection WITHOUT its bias
  const float* bias;     // [3 C] or null
  int B, Q, H, ld;
  float scale;           // 1 / sqrt(32)
  uint32_t threshold;    // keep iff hash >= threshold (0: no dropout)
  float inv_keep;        // 1 / (1 - p)
  uint32_t seed_lo, seed_hi;
  const unsigned long long* seed_device;
};

// 32 floats of one staged row
struct SaRow {
  sa_f4 v[8];
};
__device__ __forceinline__ SaRow sa_lds_row(const float* s, int r) {
  SaRow o;
  const sa_f4* p = reinterpret_cast<const sa_f4*>(s + r * kSaPad);
#pragma unroll
  for (int i = 0; i < 8; ++i) o.v[i] = p[i];
  return o;
}
__device__ __forceinline__ float sa_dot(const SaRow& a, const SaRow& b) {
  sa_f2 acc = {0.f, 0.f};
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    acc = sa_f2{a.v[i].x, a.v[i].y} * sa_f2{b.v[i].x, b.v[i].y} + acc;
    acc = sa_f2{a.v[i].z, a.v[i].w} * sa_f2{b.v[i].z, b.v[i].w} + acc;
  }
  return acc.x + acc.y;
}
__device__ __forceinline__ void sa_axpy(SaRow& y, float a, const SaRow& x) {
#pragma unroll
  for (int i = 0; i < 8; ++i) y.v[i] += a * x.v[i];
}
__device__ __forceinline__ void sa_zero(SaRow& y) {
#pragma unroll
  for (int i = 0; i < 8; ++i) y.v[i] = sa_f4{0.f, 0.f, 0.f, 0.f};
}
// the 32 channels of head `h` of row `row`, section `sec` (0 q, 1 k, 2 v), bias added
__device__ __forceinline__ SaRow sa_global_row(const SaArgs& a, int64_t row, int h, int sec) {
  SaRow o;
  const int C = a.H * kSaHd;
  const float* p = a.qkv + row * a.ld + sec * C + h * kSaHd;
  const float* bp = a.bias != nullptr ? a.bias + sec * C + h * kSaHd : nullptr;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    o.v[i] = *reinterpret_cast<const sa_f4*>(p + 4 * i);
    if (bp != nullptr) o.v[i] += *reinterpret_cast<const sa_f4*>(bp + 4 * i);
  }
  return o;
}
// sum of the 8 lanes' rows; lane `sub` of the group returns channels [4 sub, 4 sub + 4)  (reduce-scatter: 16 + 8 + 4 exchanges)
__device__ __forceinline__ sa_f4 sa_group_reduce(const SaRow& r, int sub) {
  sa_f4 a[4];
  {
    const bool up = (sub & 4) != 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const sa_f4 keep = up ? r.v[4 + i] : r.v[i], send = up ? r.v[i] : r.v[4 + i];
      a[i].x = keep.x + __shfl_xor(send.x, 4, 64); a[i].y = keep.y + __shfl_xor(send.y, 4, 64);
      a[i].z = keep.z + __shfl_xor(send.z, 4, 64); a[i].w = keep.w + __shfl_xor(send.w, 4, 64);
    }
  }
  sa_f4 b[2];
  {
    const bool up = (sub & 2) != 0;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const sa_f4 keep = up ? a[2 + i] : a[i], send = up ? a[i] : a[2 + i];
      b[i].x = keep.x + __shfl_xor(send.x, 2, 64); b[i].y = keep.y + __shfl_xor(send.y, 2, 64);
      b[i].z = keep.z + __shfl_xor(send.z, 2, 64); b[i].w = keep.w + __shfl_xor(send.w, 2, 64);
    }
  }
  const bool up = (sub & 1) != 0;
  const sa_f4 keep = up ? b[1] : b[0], send = up ? b[0] : b[1];
  sa_f4 c;
  c.x = keep.x + __shfl_xor(send.x, 1, 64); c.y = keep.y + __shfl_xor(send.y, 1, 64);
  c.z = keep.z + __shfl_xor(send.z, 1, 64); c.w = keep.w + __shfl_xor(send.w, 1, 64);
  return c;
}
__device__ __forceinline__ float sa_group_sum(float v) {
  v += __shfl_xor(v, 1, 64); v += __shfl_xor(v, 2, 64); v += __shfl_xor(v, 4, 64);
  return v;
}
__device__ __forceinline__ float sa_group_max(float v) {
  v = fmaxf(v, __shfl_xor(v, 1, 64)); v = fmaxf(v, __shfl_xor(v, 2, 64)); v = fmaxf(v, __shfl_xor(v, 4, 64));
  return v;
}

// stage rows [r0, r0 + 64) of one (batch, head) section into LDS (rows past the end: zeros); thread t -> rows t / 8 and
// t / 8 + 32, channels 4 (t % 8)
__device__ __forceinline__ void sa_stage(const SaArgs& a, float* dst, int b, int h, int sec, int r0, int tid, float mul) {
  const int C = a.H * kSaHd;
  const int c4 = (tid & 7) * 4;
  sa_f4 bias = {0.f, 0.f, 0.f, 0.f};
  if (a.bias != nullptr) bias = *reinterpret_cast<const sa_f4*>(a.bias + sec * C + h * kSaHd + c4);
#pragma unroll
  for (int it = 0; it < kSaChunk / kSaRows; ++it) {
    const int r = (tid >> 3) + it * kSaRows;
    sa_f4 v = {0.f, 0.f, 0.f, 0.f};
    if (r0 + r < a.Q) v = (*reinterpret_cast<const sa_f4*>(a.qkv + (int64_t(b) * a.Q + r0 + r) * a.ld + sec * C + h * kSaHd + c4) + bias) * mul;
    *reinterpret_cast<sa_f4*>(dst + r * kSaPad + c4) = v;
  }
}

// ---- forward --------------------------------------------------------------------------------------------------------------
template <bool DROP>
__global__ void __launch_bounds__(kSaThreads, 3)      // q, the context, eight scores and two staged rows at a time
query_self_attn_fwd_kernel(SaArgs a, float* __restrict__ out, float* __restrict__ lse, int tiles) {
  __shared__ __attribute__((aligned(16))) float s_k[kSaChunk * kSaPad];
  __shared__ __attribute__((aligned(16))) float s_v[kSaChunk * kSaPad];
  const int tid = threadIdx.x, sub = tid & 7, rl = tid >> 3;
  const int t = blockIdx.x % tiles, bh = blockIdx.x / tiles, h = bh % a.H, b = bh / a.H;
  const int row = t * kSaRows + rl;
  const bool live = row < a.Q;
  const int rowc = live ? row : a.Q - 1;
  uint32_t seed_lo = a.seed_lo, seed_hi = a.seed_hi;
  if (DROP) dropout_effective_seed(seed_lo, seed_hi, a.seed_device);

  SaRow q = sa_global_row(a, int64_t(b) * a.Q + rowc, h, 0);
#pragma unroll
  for (int i = 0; i < 8; ++i) q.v[i] *= a.scale;
  SaRow o;
  sa_zero(o);
  float m = kSaLowest, l = 0.f;      // a finite "no key yet": exp(lowest - x) = 0 without a special case
  const uint32_t bh_row = uint32_t(bh) * uint32_t(a.Q) + uint32_t(rowc);

  for (int k0 = 0; k0 < a.Q; k0 += kSaChunk) {
    __syncthreads();
    sa_stage(a, s_k, b, h, 1, k0, tid, 1.f);
    sa_stage(a, s_v, b, h, 2, k0, tid, 1.f);
    __syncthreads();
    float s[kSaPerLane];
    float cm = m;
#pragma unroll
    for (int j = 0; j < kSaPerLane; ++j) {
      const int kl = j * kSaLanes + sub;
      const float d = sa_dot(q, sa_lds_row(s_k, kl));      // (rows past the last key are staged as zeros)
      s[j] = k0 + kl < a.Q ? d : -INFINITY;
      cm = fmaxf(cm, s[j]);
      if (j & 1) __builtin_amdgcn_sched_barrier(0);      // two rows in flight at most: the scheduler would hoist all eight
    }
    const float alpha = __expf(m - cm);
    l *= alpha;
#pragma unroll
    for (int i = 0; i < 8; ++i) o.v[i] *= alpha;
    m = cm;
#pragma unroll
    for (int j = 0; j < kSaPerLane; ++j) {
      const int kl = j * kSaLanes + sub;
      const float p = __expf(s[j] - m);        // s = -inf: 0
      l += p;
      float pd = p;
      if (DROP) pd = sa_keep(bh_row, uint32_t(k0 + kl), uint32_t(a.Q), a.threshold, seed_lo, seed_hi) ? p * a.inv_keep : 0.f;
      sa_axpy(o, pd, sa_lds_row(s_v, kl));
      if (j & 1) __builtin_amdgcn_sched_barrier(0);
    }
  }
  // the 8 partial states of a row -> one
  const float mg = sa_group_max(m);
  const float f = __expf(m - mg);
  l = sa_group_sum(l * f);
#pragma unroll
  for (int i = 0; i < 8; ++i) o.v[i] *= f;
  const sa_f4 c = sa_group_reduce(o, sub);
  if (live) {
    const float inv = 1.f / l;
    *reinterpret_cast<sa_f4*>(out + (int64_t(b) * a.Q + row) * (a.H * kSaHd) + h * kSaHd + sub * 4) = c * inv;
    if (sub == 0) lse[int64_t(bh) * a.Q + row] = mg + __logf(l);
  }
}

// ---- backward -------------------------------------------------------------------------------------------------------------
// grad_qkv [B * Q][ld_g]: grad_q at column 0 (of the UNscaled q: x scale), grad_k at C, grad_v at 2 C.
// Workgroups [0, n) are query workgroups, [n, 2 n) key workgroups (n = B * H * tiles).
template <bool DROP>
__global__ void __launch_bounds__(kSaThreads, 2)      // a key workgroup holds k, v, grad_k, grad_v and one (query, grad_out) pair: ~200 VGPRs
query_self_attn_bwd_kernel(SaArgs a, const float* __restrict__ out, const float* __restrict__ lse,
                           const float* __restrict__ grad_out, float* __restrict__ grad_qkv, int ld_g, int tiles) {
  __shared__ __attribute__((aligned(16))) float s_a[kSaChunk * kSaPad];      // keys (query workgroups) / scaled queries (key workgroups)
  __shared__ __attribute__((aligned(16))) float s_b[kSaChunk * kSaPad];      // values / grad_out rows
  __shared__ float s_lse[kSaChunk], s_d[kSaChunk];
  const int tid = threadIdx.x, sub = tid & 7, rl = tid >> 3;
  const int n = a.B * a.H * tiles;
  const bool key_role = int(blockIdx.x) >= n;
  const int blk = key_role ? int(blockIdx.x) - n : int(blockIdx.x);
  const int t = blk % tiles, bh = blk / tiles, h = bh % a.H, b = bh / a.H;
  const int C = a.H * kSaHd;
  const int row = t * kSaRows + rl;
  const bool live = row < a.Q;
  const int rowc = live ? row : a.Q - 1;
  uint32_t seed_lo = a.seed_lo, seed_hi = a.seed_hi;
  if (DROP) dropout_effective_seed(seed_lo, seed_hi, a.seed_device);
  const float* go_head = grad_out + int64_t(b) * a.Q * C + h * kSaHd;
  const float* o_head = out + int64_t(b) * a.Q * C + h * kSaHd;

  if (!key_role) {
    // ---- grad_q of query row `row`: sum over keys of dS k, dS = a (dA~ keep / (1 - p) - D) ---------------------------------
    SaRow q = sa_global_row(a, int64_t(b) * a.Q + rowc, h, 0), go;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      q.v[i] *= a.scale;
      go.v[i] = *reinterpret_cast<const sa_f4*>(go_head + int64_t(rowc) * C + 4 * i);
    }
    float d_part;
    {      // (this lane's four channels of both rows, loaded again: go.v[sub] would index registers by a lane value)
      const sa_f4 ov = *reinterpret_cast<const sa_f4*>(o_head + int64_t(rowc) * C + 4 * sub);
      const sa_f4 gv = *reinterpret_cast<const sa_f4*>(go_head + int64_t(rowc) * C + 4 * sub);
      d_part = gv.x * ov.x + gv.y * ov.y + gv.z * ov.z + gv.w * ov.w;
    }
    const float D = sa_group_sum(d_part);
    const float L = lse[int64_t(bh) * a.Q + rowc];
    const uint32_t bh_row = uint32_t(bh) * uint32_t(a.Q) + uint32_t(rowc);
    SaRow dq;
    sa_zero(dq);
    for (int k0 = 0; k0 < a.Q; k0 += kSaChunk) {
      __syncthreads();
      sa_stage(a, s_a, b, h, 1, k0, tid, 1.f);
      sa_stage(a, s_b, b, h, 2, k0, tid, 1.f);
      __syncthreads();
#pragma unroll 1
      for (int j = 0; j < kSaPerLane; ++j) {
        const int kl = j * kSaLanes + sub;
        const SaRow kr = sa_lds_row(s_a, kl);
        const float p = k0 + kl < a.Q ? __expf(sa_dot(q, kr) - L) : 0.f;
        float da = sa_dot(go, sa_lds_row(s_b, kl));
        if (DROP) da = sa_keep(bh_row, uint32_t(k0 + kl), uint32_t(a.Q), a.threshold, seed_lo, seed_hi) ? da * a.inv_keep : 0.f;
        sa_axpy(dq, p * (da - D), kr);
      }
    }
    const sa_f4 c = sa_group_reduce(dq, sub);
    if (live) *reinterpret_cast<sa_f4*>(grad_qkv + (int64_t(b) * a.Q + row) * ld_g + h * kSaHd + sub * 4) = c * a.scale;
    return;
  }

  // ---- grad_k, grad_v of key row `row`: sums over the queries --------------------------------------------------------------
  const SaRow kr = sa_global_row(a, int64_t(b) * a.Q + rowc, h, 1), vr = sa_global_row(a, int64_t(b) * a.Q + rowc, h, 2);
  SaRow dk, dv;
  sa_zero(dk);
  sa_zero(dv);
  for (int q0 = 0; q0 < a.Q; q0 += kSaChunk) {
    __syncthreads();
    sa_stage(a, s_a, b, h, 0, q0, tid, a.scale);
    {      // grad_out rows, and D / lse of the chunk's queries (8 lanes per row)
      const int c4 = sub * 4;
#pragma unroll
      for (int it = 0; it < kSaChunk / kSaRows; ++it) {
        const int r = rl + it * kSaRows;
        sa_f4 g = {0.f, 0.f, 0.f, 0.f};
        float dp = 0.f;
        if (q0 + r < a.Q) {
          g = *reinterpret_cast<const sa_f4*>(go_head + int64_t(q0 + r) * C + c4);
          const sa_f4 ov = *reinterpret_cast<const sa_f4*>(o_head + int64_t(q0 + r) * C + c4);
          dp = g.x * ov.x + g.y * ov.y + g.z * ov.z + g.w * ov.w;
        }
        *reinterpret_cast<sa_f4*>(s_b + r * kSaPad + c4) = g;
        dp = sa_group_sum(dp);
        if (sub == 0) {
          s_d[r] = dp;
          s_lse[r] = q0 + r < a.Q ? lse[int64_t(bh) * a.Q + q0 + r] : 0.f;
        }
      }
    }
    __syncthreads();
#pragma unroll 1
    for (int j = 0; j < kSaPerLane; ++j) {
      const int ql = j * kSaLanes + sub;
      const SaRow qr = sa_lds_row(s_a, ql), gr = sa_lds_row(s_b, ql);
      const float p = q0 + ql < a.Q ? __expf(sa_dot(qr, kr) - s_lse[ql]) : 0.f;
      float da = sa_dot(gr, vr), pd = p;
      if (DROP) {
        const bool keep = sa_keep(uint32_t(bh) * uint32_t(a.Q) + uint32_t(q0 + ql), uint32_t(rowc), uint32_t(a.Q), a.threshold, seed_lo, seed_hi);
        da = keep ? da * a.inv_keep : 0.f;
        pd = keep ? p * a.inv_keep : 0.f;
      }
      sa_axpy(dv, pd, gr);
      sa_axpy(dk, p * (da - s_d[ql]), qr);      // qr is the SCALED query: d s / d k
    }
  }
  const sa_f4 ck = sa_group_reduce(dk, sub), cv = sa_group_reduce(dv, sub);
  if (live) {
    float* g = grad_qkv + (int64_t(b) * a.Q + row) * ld_g + h * kSaHd + sub * 4;
    *reinterpret_cast<sa_f4*>(g + C) = ck;
    *reinterpret_cast<sa_f4*>(g + 2 * C) = cv;
  }
}

static int sa_check(const char* fn, int dtype, int batch, int queries, int heads, int head_dim, int ld, float p) {
  if (dtype != VNX_F32) {
    set_error("%s: fp32 only (dtype %d)", fn, dtype);
    return VNX_ERR_UNSUPPORTED;
  }
  if (head_dim != kSaHd) {
    set_error("%s: built for heads of %d channels (head_dim %d)", fn, kSaHd, head_dim);
    return VNX_ERR_UNSUPPORTED;
  }
  if (batch < 0 || queries < 0 || heads <= 0 || ld < 3 * heads * kSaHd || (ld & 3) != 0 || !(p >= 0.f && p < 1.f)) {
    set_error("%s: bad sizes (batch %d, queries %d, heads %d, row stride %d, p %g)", fn, batch, queries, heads, ld, double(p));
    return VNX_ERR_INVALID_ARGUMENT;
  }
  if (int64_t(batch) * heads * ((queries + kSaRows - 1) / kSaRows) * 2 >= (int64_t(1) << 31)) {
    set_error("%s: too many workgroups", fn);
    return VNX_ERR_UNSUPPORTED;
  }
  return VNX_OK;
}

}  // namespace vnx

using namespace vnx;

extern "C" int vnx_query_self_attention_forward(int dtype, const void* qkv, const void* in_proj_bias, void* out, void* lse,
                                                int batch, int queries, int heads, int head_dim, int row_stride, float p,
                                                unsigned long long seed, const unsigned long long* seed_device,
                                                void* hip_stream) {
  if (int st = sa_check("vnx_query_self_attention_forward", dtype, batch, queries, heads, head_dim, row_stride, p)) return st;
  if (batch == 0 || queries == 0) return VNX_OK;
  if (!qkv || !out || !lse) {
    set_error("vnx_query_self_attention_forward: null pointer argument");
    return VNX_ERR_INVALID_ARGUMENT;
  }
  const int tiles = (queries + kSaRows - 1) / kSaRows;
  const SaArgs a{(const float*)qkv, (const float*)in_proj_bias, batch, queries, heads, row_stride, 1.f / sqrtf(float(kSaHd)),
                 dropout_threshold(p), 1.f / (1.f - p), uint32_t(seed), uint32_t(seed >> 32), seed_device};
  if (a.threshold != 0u)
    hipLaunchKernelGGL(query_self_attn_fwd_kernel<true>, dim3(uint32_t(batch * heads * tiles)), dim3(kSaThreads), 0,
                       (hipStream_t)hip_stream, a, (float*)out, (float*)lse, tiles);
  else
    hipLaunchKernelGGL(query_self_attn_fwd_kernel<false>, dim3(uint32_t(batch * heads * tiles)), dim3(kSaThreads), 0,
                       (hipStream_t)hip_stream, a, (float*)out, (float*)lse, tiles);
  return check_launch("query_self_attn_fwd");
}

extern "C" int vnx_query_self_attention_backward(int dtype, const void* qkv, const void* in_proj_bias, const void* out,
                                                 const void* lse, const void* grad_out, void* grad_qkv, int batch, int queries,
                                                 int heads, int head_dim, int row_stride, int grad_row_stride, float p,
                                                 unsigned long long seed, const unsigned long long* seed_device,
                                                 void* hip_stream) {
  if (int st = sa_check("vnx_query_self_attention_backward", dtype, batch, queries, heads, head_dim, row_stride, p)) return st;
  if (grad_row_stride < 3 * heads * kSaHd || (grad_row_stride & 3) != 0) {
    set_error("vnx_query_self_attention_backward: bad gradient row stride %d", grad_row_stride);
    return VNX_ERR_INVALID_ARGUMENT;
  }
  if (batch == 0 || queries == 0) return VNX_OK;
  if (!qkv || !out || !lse || !grad_out || !grad_qkv) {
    set_error("vnx_query_self_attention_backward: null pointer argument");
    return VNX_ERR_INVALID_ARGUMENT;
  }
  const int tiles = (queries + kSaRows - 1) / kSaRows;
  const SaArgs a{(const float*)qkv, (const float*)in_proj_bias, batch, queries, heads, row_stride, 1.f / sqrtf(float(kSaHd)),
                 dropout_threshold(p), 1.f / (1.f - p), uint32_t(seed), uint32_t(seed >> 32), seed_device};
  if (a.threshold != 0u)
    hipLaunchKernelGGL(query_self_attn_bwd_kernel<true>, dim3(uint32_t(2 * batch * heads * tiles)), dim3(kSaThreads), 0,
                       (hipStream_t)hip_stream, a, (const float*)out, (const float*)lse, (const float*)grad_out,
                       (float*)grad_qkv, grad_row_stride, tiles);
  else
    hipLaunchKernelGGL(query_self_attn_bwd_kernel<false>, dim3(uint32_t(2 * batch * heads * tiles)), dim3(kSaThreads), 0,
                       (hipStream_t)hip_stream, a, (const float*)out, (const float*)lse, (const float*)grad_out,
                       (float*)grad_qkv, grad_row_stride, tiles);
  return check_launch("query_self_attn_bwd");
}
