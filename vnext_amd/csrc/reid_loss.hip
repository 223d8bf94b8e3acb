// reid_loss.hip -- IDOL's two re-identification losses (the contrastive loss and the auxiliary cosine loss of
// deformable_detr.py:418-454, what vnext_amd.heads.loss_reid computes per image) for every instance of every image of a
// step at once: one launch forward, two backward.
//
// What it replaces (idol_criterion.reid_terms + heads.loss_reid, per image): four pageable uploads, an advanced-index gather of
// the key rows, two F.normalize chains, two similarity launches, two masked logsumexp, softplus and a dozen element-wise
// and reduction launches -- and autograd's replay of all of it, with four more GEMM launches behind .t().contiguous().
//
// Here: key fp32 [B][Q][C] and ref fp32 [B][R][C] (rows contiguous, any image stride: the two interleaved halves of one
// [2 B, Q, C] tensor are read in place), the instance list img / key_query int32 [J] (instance j compares row key_query[j] of
// key image img[j] with all R rows of reference image img[j]) and flags uint8 [J][R]: bit 0 positive, bit 1 negative, bit 2
// aux sample.  With k the key row, dot_r = <ref_r, k>, cos_r = dot_r / (max(|ref_r|, 1e-12) max(|k|, 1e-12)):
//   out[j][0] = softplus(logsumexp_{r in N} dot_r + logsumexp_{r in P} -dot_r),  exactly 0 when P or N is empty
//   out[j][1] = sum_{r in A} (cos_r - [r in P])^2 / max(|A|, 1)
// Both logsumexp are kept as (maximum, sum of exp(x - maximum)): the maximum is one of the dots, exact, and the backward's
// softmax is exp(x - maximum) / sum -- no fp32 rounding of a logsumexp of magnitude 100 inside an exponential.
// An instance whose img or key_query is out of range reads nothing, gets (0, 0) and contributes no gradient.
//
// Forward (reid_loss_fwd_kernel): one workgroup of four wave64 per instance.  A wave walks reference rows sixteen at a time
// (rows wave, wave + 4, ...), a lane holding V = 4 consecutive channels of the key row in registers (16-byte loads: a
// 256-channel row is one coalesced 1 KiB read; V = 1 where C % 4 != 0 or a pointer is not 16-byte aligned); one pass
// reduces dot and |ref_r|^2 together over a fixed exchange tree.  The R dots and norms are parked in LDS, then 256 lanes
// take the maxima, the sums of exponentials, the counts and the squared errors: lane sums, the tree, the four waves in
// order.  It saves dot [J][R], |ref_r| [J][R] and stats [J][8] = {|k|, max_N, sum_N, max_P, sum_P, |A|, P and N both
// non-empty, 0} for the backward: nothing of the embeddings' size.
//
// Backward, owner-computes: every element of grad_ref [B][R][C] and grad_key [B][Q][C] is written exactly once by the
// lane that owns it -- no memset, no scatter, no atomics, sums in list order: bit-identical run to run.
//   reid_loss_bwd_ref_kernel: a lane owns V channels of one row (b, r):
//     sum over the instances j of image b of  a_jr k_j + b_jr ref_r
//   reid_loss_bwd_key_kernel: a workgroup owns one row (b, q): zero unless an instance points at it, else
//     sum over those instances of  sum_r a_jr ref_r - (sum_r Gcos_jr cos_jr) k_j / |k_j|^2
//   a_jr = Gdot_jr + Gcos_jr / (m_r m_k),  b_jr = -Gcos_jr cos_jr / |ref_r|^2   (m = the clamped norm; the clamp is
//   differentiated as ATen's clamp_min: the norm's own term is dropped below 1e-12)
//   Gdot_jr = g[j][0] sigmoid(pair_j) ([r in N] softmax_N(dot)_r - [r in P] softmax_P(-dot)_r)
//   Gcos_jr = g[j][1] 2 (cos_r - [r in P]) [r in A] / max(|A|, 1)
// Accurate expf / logf / log1pf and true divisions throughout (no fast-math), as mask_loss.hip.
#include "vnx_common.h"

#include <math.h>

namespace vnx {
namespace {

constexpr int kRlThreads = 256;
constexpr int kRlWaves = kRlThreads / 64;
constexpr int kRlFwdRows = 16;                  // reference rows a wave of the forward has in flight
constexpr int kRlKeyRows = 8;                   // ... and a wave of the grad_key kernel
constexpr int kRlMaxRows = VNX_REID_LOSS_MAX_ROWS;
constexpr float kRlEps = 1e-12f;                 // F.normalize's clamp

struct RlIn {
  const float* key;
  const float* ref;
  int64_t key_stride, ref_stride;                // elements between two images
  const int32_t* img;
  const int32_t* kq;
  const uint8_t* flags;
  int B, Q, R, C, J;
};

template <int V> struct RlVec;
template <> struct RlVec<4> { using T = vnx_f4; };
template <> struct RlVec<1> { using T = float; };
template <int V> __device__ __forceinline__ typename RlVec<V>::T rl_load(const float* p) {
  return *reinterpret_cast<const typename RlVec<V>::T*>(p);
}
template <int V> __device__ __forceinline__ void rl_store(float* p, typename RlVec<V>::T v) {
  *reinterpret_cast<typename RlVec<V>::T*>(p) = v;
}
template <int V> __device__ __forceinline__ typename RlVec<V>::T rl_zero();
template <> __device__ __forceinline__ vnx_f4 rl_zero<4>() { return vnx_f4{0.f, 0.f, 0.f, 0.f}; }
template <> __device__ __forceinline__ float rl_zero<1>() { return 0.f; }
__device__ __forceinline__ float rl_dot(vnx_f4 a, vnx_f4 b) { return a.x * b.x + a.y * b.y + a.z * b.z + a.w * b.w; }
__device__ __forceinline__ float rl_dot(float a, float b) { return a * b; }

// N values at once over the workgroup, every lane gets the results: the exchange tree, then the four waves in order
template <int N, bool kMax>
__device__ __forceinline__ void rl_block_reduce(float (&v)[N], float (*s)[8]) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int i = 0; i < N; ++i) v[i] = kMax ? wave_max(v[i]) : wave_sum(v[i]);
  if (lane == 0) {
#pragma unroll
    for (int i = 0; i < N; ++i) s[wave][i] = v[i];
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < N; ++i) {
    float a = s[0][i];
#pragma unroll
    for (int w = 1; w < kRlWaves; ++w) a = kMax ? fmaxf(a, s[w][i]) : a + s[w][i];
    v[i] = a;
  }
  __syncthreads();
}

__device__ __forceinline__ bool rl_in_range(const RlIn& in, int b, int q) {
  return b >= 0 && b < in.B && q >= 0 && q < in.Q;
}

// pair = logsumexp_N(dot) + logsumexp_P(-dot): the two maxima meet first, in one rounding
__device__ __forceinline__ float rl_pair(float mN, float sN, float mP, float sP) { return (mN + mP) + (logf(sN) + logf(sP)); }

// what the backward knows of instance j
struct RlInst {
  bool ok, has;            // in range; P and N both non-empty
  const float* k;          // its key row
  float nk, mk;            // |k| and its clamped form
  float mN, sN, mP, sP;    // the two logsumexp as (maximum, sum)
  float gcs;               // g[j][0] * sigmoid(pair)
  float ga;                // g[j][1] * 2 / max(|A|, 1)
};
__device__ __forceinline__ RlInst rl_inst(const RlIn& in, const float* __restrict__ stats, const float* __restrict__ grad_out,
                                          int j) {
  RlInst I;
  const int b = in.img[j], q = in.kq[j];
  I.ok = rl_in_range(in, b, q);
  I.has = false;
  I.k = in.key;
  I.nk = I.mk = I.mN = I.sN = I.mP = I.sP = I.gcs = I.ga = 0.f;
  if (!I.ok) return I;
  const float* s = stats + 8 * int64_t(j);
  I.k = in.key + int64_t(b) * in.key_stride + int64_t(q) * in.C;
  I.nk = s[0];
  I.mk = fmaxf(I.nk, kRlEps);
  I.has = s[6] != 0.f;
  if (I.has) {
    I.mN = s[1]; I.sN = s[2]; I.mP = s[3]; I.sP = s[4];
    const float pair = rl_pair(I.mN, I.sN, I.mP, I.sP);
    const float e = expf(-fabsf(pair));
    I.gcs = grad_out[2 * int64_t(j)] * (pair >= 0.f ? 1.f / (1.f + e) : e / (1.f + e));
  }
  I.ga = grad_out[2 * int64_t(j) + 1] * 2.f / fmaxf(s[5], 1.f);
  return I;
}

// the coefficients of (instance, reference row): a and b above, and kc = Gcos * cos
struct RlCoef { float a, b, kc; };
__device__ __forceinline__ RlCoef rl_coef(const RlInst& I, float d, float nr, unsigned f) {
  const float denom = fmaxf(nr, kRlEps) * I.mk;
  const float cosv = d / denom;
  float gdot = 0.f;
  if (I.has) {
    if (f & 2u) gdot += expf(d - I.mN) / I.sN;
    if (f & 1u) gdot -= expf(-d - I.mP) / I.sP;
    gdot *= I.gcs;
  }
  const float gcos = (f & 4u) ? I.ga * (cosv - ((f & 1u) ? 1.f : 0.f)) : 0.f;
  RlCoef c;
  c.a = gdot + gcos / denom;
  c.b = nr >= kRlEps ? -gcos * cosv / (nr * nr) : 0.f;
  c.kc = gcos * cosv;
  return c;
}

}  // namespace

// grid: J workgroups.  out [J][2], dot [J][R], ref_norm [J][R], stats [J][8]
template <int V>
__global__ void __launch_bounds__(kRlThreads) reid_loss_fwd_kernel(const RlIn in, float* __restrict__ out,
                                                                   float* __restrict__ dot_out, float* __restrict__ rn_out,
                                                                   float* __restrict__ stats) {
  using Vec = typename RlVec<V>::T;
  __shared__ float s_dot[kRlMaxRows];
  __shared__ float s_rn[kRlMaxRows];
  __shared__ float s_red[kRlWaves][8];
  const int j = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = in.img[j], q = in.kq[j];
  const int R = in.R, C = in.C;
  if (!rl_in_range(in, b, q)) {                     // reads nothing, (0, 0), no gradient
    if (tid == 0) {
      out[2 * int64_t(j)] = 0.f;
      out[2 * int64_t(j) + 1] = 0.f;
    }
    if (tid < 8) stats[8 * int64_t(j) + tid] = 0.f;
    return;
  }
  const float* k = in.key + int64_t(b) * in.key_stride + int64_t(q) * C;
  const float* ref = in.ref + int64_t(b) * in.ref_stride;
  constexpr int kStep = 64 * V;                     // channels a wave covers per load
  const int c_first = lane * V;
  // the key row: its first kStep channels stay in registers, the rest (C > kStep) is re-read from the cache
  const Vec k0 = c_first < C ? rl_load<V>(k + c_first) : rl_zero<V>();
  float kk = rl_dot(k0, k0);
  for (int c = c_first + kStep; c < C; c += kStep) {
    const Vec kv = rl_load<V>(k + c);
    kk += rl_dot(kv, kv);
  }
  const float nk = sqrtf(wave_sum(kk));
  // kRlFwdRows rows per wave and round (rows r0, r0 + 4, ...): that many 16-byte loads in flight per lane -- with a
  // workgroup per instance the grid is a handful of workgroups, and a round's time is one load latency
  for (int r0 = wave; r0 < R; r0 += kRlFwdRows * kRlWaves) {
    float d[kRlFwdRows], n[kRlFwdRows];
#pragma unroll
    for (int u = 0; u < kRlFwdRows; ++u) d[u] = n[u] = 0.f;
    if (c_first < C) {
      Vec x[kRlFwdRows];
#pragma unroll
      for (int u = 0; u < kRlFwdRows; ++u) {
        const int r = min(r0 + u * kRlWaves, R - 1);      // past the end: the last row again, its result dropped below --
        x[u] = rl_load<V>(ref + int64_t(r) * C + c_first);      // a guarded load is a branch, and the loads go one by one
      }
      __builtin_amdgcn_sched_barrier(0);                  // every load of the round is issued before the first use
#pragma unroll
      for (int u = 0; u < kRlFwdRows; ++u) {
        d[u] = rl_dot(x[u], k0);
        n[u] = rl_dot(x[u], x[u]);
      }
    }
    for (int c = c_first + kStep; c < C; c += kStep) {
      const Vec kv = rl_load<V>(k + c);
      Vec x[kRlFwdRows];
#pragma unroll
      for (int u = 0; u < kRlFwdRows; ++u) {
        const int r = min(r0 + u * kRlWaves, R - 1);
        x[u] = rl_load<V>(ref + int64_t(r) * C + c);
      }
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int u = 0; u < kRlFwdRows; ++u) {
        d[u] += rl_dot(x[u], kv);
        n[u] += rl_dot(x[u], x[u]);
      }
    }
#pragma unroll
    for (int u = 0; u < kRlFwdRows; ++u) {
      d[u] = wave_sum(d[u]);
      n[u] = wave_sum(n[u]);
    }
    if (lane == 0) {
#pragma unroll
      for (int u = 0; u < kRlFwdRows; ++u) {
        const int r = r0 + u * kRlWaves;
        if (r < R) {
          s_dot[r] = d[u];
          s_rn[r] = sqrtf(n[u]);
        }
      }
    }
  }
  __syncthreads();
  const uint8_t* fl = in.flags + int64_t(j) * R;
  float m[2] = {-INFINITY, -INFINITY};              // max over N of dot, max over P of -dot
  for (int r = tid; r < R; r += kRlThreads) {
    const unsigned f = fl[r];
    const float dv = s_dot[r];
    if (f & 2u) m[0] = fmaxf(m[0], dv);
    if (f & 1u) m[1] = fmaxf(m[1], -dv);
  }
  rl_block_reduce<2, true>(m, s_red);
  const float mk = fmaxf(nk, kRlEps);
  float v[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};      // sum_N, sum_P, squared error over A, |A|, |N|, |P|
  for (int r = tid; r < R; r += kRlThreads) {
    const unsigned f = fl[r];
    const float dv = s_dot[r], nr = s_rn[r];
    if (f & 2u) { v[0] += expf(dv - m[0]); v[4] += 1.f; }
    if (f & 1u) { v[1] += expf(-dv - m[1]); v[5] += 1.f; }
    if (f & 4u) {
      const float e = dv / (fmaxf(nr, kRlEps) * mk) - ((f & 1u) ? 1.f : 0.f);
      v[2] += e * e;
      v[3] += 1.f;
    }
    dot_out[int64_t(j) * R + r] = dv;
    rn_out[int64_t(j) * R + r] = nr;
  }
  rl_block_reduce<6, false>(v, s_red);
  if (tid == 0) {
    const bool has = v[4] > 0.f && v[5] > 0.f;
    float contrast = 0.f;
    if (has) {
      const float pair = rl_pair(m[0], v[0], m[1], v[1]);
      contrast = fmaxf(pair, 0.f) + log1pf(expf(-fabsf(pair)));
    }
    out[2 * int64_t(j)] = contrast;
    out[2 * int64_t(j) + 1] = v[2] / fmaxf(v[3], 1.f);
    float* s = stats + 8 * int64_t(j);
    s[0] = nk;
    s[1] = has ? m[0] : 0.f;
    s[2] = has ? v[0] : 0.f;
    s[3] = has ? m[1] : 0.f;
    s[4] = has ? v[1] : 0.f;
    s[5] = v[3];
    s[6] = has ? 1.f : 0.f;
    s[7] = 0.f;
  }
}

// grid: ceil(B * R * ceil(C / V) / 256) workgroups; a lane owns V channels of one row of grad_ref [B][R][C]
template <int V>
__global__ void __launch_bounds__(kRlThreads) reid_loss_bwd_ref_kernel(const RlIn in, const float* __restrict__ dot,
                                                                       const float* __restrict__ rn,
                                                                       const float* __restrict__ stats,
                                                                       const float* __restrict__ grad_out,
                                                                       float* __restrict__ grad_ref) {
  using Vec = typename RlVec<V>::T;
  const int R = in.R, C = in.C;
  const int lanes_per_row = (C + V - 1) / V;
  const int64_t i = int64_t(blockIdx.x) * kRlThreads + threadIdx.x;
  if (i >= int64_t(in.B) * R * lanes_per_row) return;
  const int64_t row = i / lanes_per_row;
  const int c = int(i - row * lanes_per_row) * V;
  const int b = int(row / R), r = int(row - int64_t(b) * R);
  Vec acc = rl_zero<V>();
  float bsum = 0.f;
  for (int j = 0; j < in.J; ++j) {                  // the instances of image b, in list order
    if (in.img[j] != b) continue;
    const unsigned f = in.flags[int64_t(j) * R + r];
    if (f == 0u) continue;
    const RlInst I = rl_inst(in, stats, grad_out, j);
    if (!I.ok) continue;
    const RlCoef co = rl_coef(I, dot[int64_t(j) * R + r], rn[int64_t(j) * R + r], f);
    acc += co.a * rl_load<V>(I.k + c);
    bsum += co.b;
  }
  const Vec x = rl_load<V>(in.ref + int64_t(b) * in.ref_stride + int64_t(r) * C + c);
  rl_store<V>(grad_ref + row * C + c, acc + bsum * x);
}

// grid: B * Q workgroups; the workgroup owns row (b, q) of grad_key [B][Q][C]
template <int V>
__global__ void __launch_bounds__(kRlThreads) reid_loss_bwd_key_kernel(const RlIn in, const float* __restrict__ dot,
                                                                       const float* __restrict__ rn,
                                                                       const float* __restrict__ stats,
                                                                       const float* __restrict__ grad_out,
                                                                       float* __restrict__ grad_key) {
  using Vec = typename RlVec<V>::T;
  constexpr int kStep = 64 * V;                     // channels per pass: thread t < kStep owns channel c0 + t
  __shared__ float s_a[kRlMaxRows];
  __shared__ __attribute__((aligned(16))) float s_part[kRlWaves][kStep];
  __shared__ float s_red[kRlWaves][8];
  const int R = in.R, C = in.C;
  const int b = int(blockIdx.x) / in.Q, q = int(blockIdx.x) - b * in.Q;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float* ref = in.ref + int64_t(b) * in.ref_stride;
  float* o = grad_key + (int64_t(b) * in.Q + q) * C;
  for (int c0 = 0; c0 < C; c0 += kStep) {
    float acc = 0.f;
    for (int j = 0; j < in.J; ++j) {                // the instances that point at (b, q), in list order
      if (in.img[j] != b || in.kq[j] != q) continue;            // (the same answer in every lane)
      const RlInst I = rl_inst(in, stats, grad_out, j);
      float kc[1] = {0.f};
      for (int r = tid; r < R; r += kRlThreads) {
        const RlCoef co = rl_coef(I, dot[int64_t(j) * R + r], rn[int64_t(j) * R + r], in.flags[int64_t(j) * R + r]);
        s_a[r] = co.a;
        kc[0] += co.kc;
      }
      rl_block_reduce<1, false>(kc, s_red);          // (its barriers also publish s_a)
      Vec p = rl_zero<V>();
      const int c = c0 + lane * V;
      if (c < C) {
        for (int r0 = wave; r0 < R; r0 += kRlKeyRows * kRlWaves) {      // kRlKeyRows loads in flight, as in the forward
          Vec x[kRlKeyRows];
          float a[kRlKeyRows];
#pragma unroll
          for (int u = 0; u < kRlKeyRows; ++u) {
            const int r = r0 + u * kRlWaves, rr = min(r, R - 1);
            x[u] = rl_load<V>(ref + int64_t(rr) * C + c);
            a[u] = r < R ? s_a[rr] : 0.f;
          }
          __builtin_amdgcn_sched_barrier(0);
#pragma unroll
          for (int u = 0; u < kRlKeyRows; ++u) p += a[u] * x[u];
        }
      }
      rl_store<V>(&s_part[wave][lane * V], p);
      __syncthreads();
      if (tid < kStep && c0 + tid < C) {
        float tot = s_part[0][tid];
#pragma unroll
        for (int w = 1; w < kRlWaves; ++w) tot += s_part[w][tid];
        const float kterm = I.nk >= kRlEps ? kc[0] * I.k[c0 + tid] / (I.nk * I.nk) : 0.f;
        acc += tot - kterm;
      }
      __syncthreads();
    }
    if (tid < kStep && c0 + tid < C) o[c0 + tid] = acc;
  }
}

static int rl_check(const char* fn, const RlIn& in) {
  if (in.B < 0 || in.Q < 0 || in.R < 0 || in.C < 0 || in.J < 0 || in.key_stride < 0 || in.ref_stride < 0) {
    set_error("%s: bad sizes (images %d, key rows %d, reference rows %d, channels %d, instances %d)", fn, in.B, in.Q, in.R,
              in.C, in.J);
    return VNX_ERR_INVALID_ARGUMENT;
  }
  if (in.B < 1 || in.Q < 1 || in.C < 1 || in.R < 1 || in.R > kRlMaxRows) {
    set_error("%s: images %d, key rows %d, reference rows %d, channels %d: at least one of each and at most %d reference rows",
              fn, in.B, in.Q, in.R, in.C, kRlMaxRows);
    return VNX_ERR_UNSUPPORTED;
  }
  if ((in.B > 1 && (in.key_stride < int64_t(in.Q) * in.C || in.ref_stride < int64_t(in.R) * in.C))) {
    set_error("%s: image strides %lld / %lld are shorter than an image's rows", fn, (long long)in.key_stride,
              (long long)in.ref_stride);
    return VNX_ERR_INVALID_ARGUMENT;
  }
  const int64_t lanes = int64_t(in.B) * in.R * in.C;               // >= the grad_ref lanes
  if (int64_t(in.B) * in.Q >= (int64_t(1) << 31) || lanes / kRlThreads >= (int64_t(1) << 31) - 1) {
    set_error("%s: %d images of %d / %d rows x %d channels are outside what the kernels address", fn, in.B, in.Q, in.R, in.C);
    return VNX_ERR_UNSUPPORTED;
  }
  if (!in.key || !in.ref || (in.J > 0 && (!in.img || !in.kq || !in.flags))) {
    set_error("%s: null pointer argument", fn);
    return VNX_ERR_INVALID_ARGUMENT;
  }
  return VNX_OK;
}

static bool rl_vec(const RlIn& in) {
  return (in.C & 3) == 0 && (in.key_stride & 3) == 0 && (in.ref_stride & 3) == 0 &&
         (reinterpret_cast<uintptr_t>(in.key) & 15) == 0 && (reinterpret_cast<uintptr_t>(in.ref) & 15) == 0;
}

static RlIn rl_in(const void* key, long long key_image_stride, int key_rows, const void* ref, long long ref_image_stride,
                  int ref_rows, int channels, int images, const void* img, const void* key_query, const void* flags,
                  int instances) {
  return RlIn{(const float*)key, (const float*)ref, int64_t(key_image_stride), int64_t(ref_image_stride), (const int32_t*)img,
              (const int32_t*)key_query, (const uint8_t*)flags, images, key_rows, ref_rows, channels, instances};
}

}  // namespace vnx

using namespace vnx;

extern "C" int vnx_reid_loss_forward(const void* key, long long key_image_stride, int key_rows, const void* ref,
                                     long long ref_image_stride, int ref_rows, int channels, int images, const void* img,
                                     const void* key_query, const void* flags, int instances, void* out, void* dot,
                                     void* ref_norm, void* stats, void* hip_stream) {
  const char* fn = "vnx_reid_loss_forward";
  const RlIn in = rl_in(key, key_image_stride, key_rows, ref, ref_image_stride, ref_rows, channels, images, img, key_query,
                        flags, instances);
  if (int st = rl_check(fn, in)) return st;
  if (instances == 0) return VNX_OK;
  if (!out || !dot || !ref_norm || !stats) {
    set_error("%s: null pointer argument", fn);
    return VNX_ERR_INVALID_ARGUMENT;
  }
  hipStream_t stream = (hipStream_t)hip_stream;
  if (rl_vec(in))
    hipLaunchKernelGGL(reid_loss_fwd_kernel<4>, dim3(uint32_t(instances)), dim3(kRlThreads), 0, stream, in, (float*)out,
                       (float*)dot, (float*)ref_norm, (float*)stats);
  else
    hipLaunchKernelGGL(reid_loss_fwd_kernel<1>, dim3(uint32_t(instances)), dim3(kRlThreads), 0, stream, in, (float*)out,
                       (float*)dot, (float*)ref_norm, (float*)stats);
  return check_launch("reid_loss_fwd");
}

extern "C" int vnx_reid_loss_backward(const void* key, long long key_image_stride, int key_rows, const void* ref,
                                      long long ref_image_stride, int ref_rows, int channels, int images, const void* img,
                                      const void* key_query, const void* flags, int instances, const void* dot_v,
                                      const void* ref_norm_v, const void* stats_v, const void* grad_out_v, void* grad_key,
                                      void* grad_ref, void* hip_stream) {
  const char* fn = "vnx_reid_loss_backward";
  const RlIn in = rl_in(key, key_image_stride, key_rows, ref, ref_image_stride, ref_rows, channels, images, img, key_query,
                        flags, instances);
  const float *dot = (const float*)dot_v, *ref_norm = (const float*)ref_norm_v, *stats = (const float*)stats_v,
              *grad_out = (const float*)grad_out_v;
  hipStream_t stream = (hipStream_t)hip_stream;
  if (int st = rl_check(fn, in)) return st;
  if (!grad_key || !grad_ref || (instances > 0 && (!dot || !ref_norm || !stats || !grad_out))) {
    set_error("%s: null pointer argument", fn);
    return VNX_ERR_INVALID_ARGUMENT;
  }
  const bool vec = rl_vec(in) && (reinterpret_cast<uintptr_t>(grad_key) & 15) == 0 && (reinterpret_cast<uintptr_t>(grad_ref) & 15) == 0;
  const int64_t lanes = int64_t(images) * ref_rows * ((channels + (vec ? 3 : 0)) / (vec ? 4 : 1));
  const dim3 ref_grid(uint32_t((lanes + kRlThreads - 1) / kRlThreads)), key_grid(uint32_t(images) * uint32_t(key_rows));
  if (vec)
    hipLaunchKernelGGL(reid_loss_bwd_ref_kernel<4>, ref_grid, dim3(kRlThreads), 0, stream, in, dot, ref_norm, stats, grad_out, (float*)grad_ref);
  else
    hipLaunchKernelGGL(reid_loss_bwd_ref_kernel<1>, ref_grid, dim3(kRlThreads), 0, stream, in, dot, ref_norm, stats, grad_out, (float*)grad_ref);
  if (int st = check_launch("reid_loss_bwd_ref")) return st;
  if (vec)
    hipLaunchKernelGGL(reid_loss_bwd_key_kernel<4>, key_grid, dim3(kRlThreads), 0, stream, in, dot, ref_norm, stats, grad_out, (float*)grad_key);
  else
    hipLaunchKernelGGL(reid_loss_bwd_key_kernel<1>, key_grid, dim3(kRlThreads), 0, stream, in, dot, ref_norm, stats, grad_out, (float*)grad_key);
  return check_launch("reid_loss_bwd_key");
}
