// swin_glue.hip -- the element-wise glue of a Swin stage in one pass each way: stochastic depth, the residual add and the
// pre-norm LayerNorm of the NEXT branch, and PatchMerging's pad + 2x2 gather + LayerNorm.
//
// Reference (projects/SeqFormer/seqformer/backbone/swin.py; IDOL's Swin-L configs use the same file):
//   SwinTransformerBlock.forward   x = shortcut + drop_path(attn(norm1(x)));  x = x + drop_path(mlp(norm2(x)))
//   PatchMerging.forward           pad to even H, W; cat of the four 2x2 phases; norm over 4C; reduction
// Per residual site the library chain is rand / add / floor_ on the [B,1,1] mask, div and mul over the branch, the add,
// layer_norm (fp32 under autocast) and the cast the next Linear makes: eight launches.  Here:
//   y[r] = x[r] + scale[b] * a[r]                    (b = r / rows_per_sample; scale null: 1; a null: y = x, not written)
//   n[r] = LayerNorm(y[r]; gamma, beta, eps)          (gamma null: no n)          stats[r] = (mean, rstd)
// Swin is pre-norm: y stays the residual stream and n feeds the branch, so one entry point covers the in-block site
// (x, attn-out) -> (y, norm2(y)), the between-block site (y, mlp-out) -> (x', norm1_next(x')), the plain LayerNorm that
// opens a stage and the plain scaled add that closes it.
//
// Layout: a row is held in registers by a GROUP of G lanes (8, 16, 32 or 64: the smallest that covers C / 8, so a wave
// carries 64 / G rows), each lane NCH chunks of 8 consecutive channels -- 16 bytes of bf16, two 16-byte accesses of fp32.
// Chunk k of a row sits in lane k % G, slot k / G.  Mean and variance: two passes over the registers, xor-shuffles inside
// the group (fp32, as accurate as ATen's Welford).  No LDS and no barrier in the forward.
// Types: x / y, the branch a and n are (fp32, fp32, fp32), (fp32, bf16, bf16) or (bf16, bf16, bf16) -- what the eager chain
// produces without autocast, under bf16 autocast in stage 1 and in stages 2-4.  gamma, beta, stats and all arithmetic fp32.
// n is the LayerNorm of y AS STORED (the rounded y of a bf16 stream): the backward recomputes xhat from the saved y.
// A dropped sample (scale 0) never reads its branch: y = x bit for bit, grad_a = 0.
//
// Backward: g = grad_y + LayerNormBackward(grad_n); grad_x = g; grad_a = scale[b] * g.  Every element of both is written.
// grad_gamma / grad_beta: every lane keeps its columns' sums over the rows it walks, the lanes of a workgroup that hold the
// same columns meet in LDS in a fixed order, and the workgroup leaves one partial row pair; a finishing launch adds the
// partial rows in a fixed order.  No atomics: bit-identical run to run.  The partial buffer is sized by the launch.
//
// PatchMerging: output row (b, i, j) of 4C channels; chunk k lies in phase q = 8k / C -- source pixel (2i + (q & 1),
// 2j + (q >> 1)), the reference's cat order -- and a pixel outside the grid contributes zeros (the reference's pad), which
// count in the statistics.  Same kernels, MERGE = true: the row is gathered instead of streamed, there is no branch, and
// in the backward every element of grad_x is written by the one output row that owns it.
#include "vnx_common.h"

#include <algorithm>

namespace vnx {

namespace {

constexpr int kSgWaves = 4;                 // waves per workgroup
constexpr int kSgThreads = 64 * kSgWaves;
constexpr int kSgMaxBlocks = 1024;          // workgroups of a backward at most = partial row pairs at most
constexpr int kSgRowsPerBlock = 4;          // a backward workgroup walks at least this many passes (when there are rows)
constexpr int kSgFinCols = 16, kSgFinSlices = 16;      // the finishing launch: 16 columns x 16 slices per workgroup

struct f8 { vnx_f4 lo, hi; };

__device__ __forceinline__ f8 zero8() { return f8{vnx_f4{0.f, 0.f, 0.f, 0.f}, vnx_f4{0.f, 0.f, 0.f, 0.f}}; }

typedef uint32_t vnx_u4 __attribute__((ext_vector_type(4)));

template <typename T> __device__ __forceinline__ f8 load8(const T* p);
template <> __device__ __forceinline__ f8 load8<float>(const float* p) {
  return f8{*reinterpret_cast<const vnx_f4*>(p), *reinterpret_cast<const vnx_f4*>(p + 4)};
}
template <> __device__ __forceinline__ f8 load8<bf16_t>(const bf16_t* p) {
  const vnx_u4 r = *reinterpret_cast<const vnx_u4*>(p);
  return f8{vnx_f4{__uint_as_float(r.x << 16), __uint_as_float(r.x & 0xffff0000u), __uint_as_float(r.y << 16), __uint_as_float(r.y & 0xffff0000u)},
            vnx_f4{__uint_as_float(r.z << 16), __uint_as_float(r.z & 0xffff0000u), __uint_as_float(r.w << 16), __uint_as_float(r.w & 0xffff0000u)}};
}
template <typename T> __device__ __forceinline__ void store8(T* p, const f8& v);
template <> __device__ __forceinline__ void store8<float>(float* p, const f8& v) {
  *reinterpret_cast<vnx_f4*>(p) = v.lo;
  *reinterpret_cast<vnx_f4*>(p + 4) = v.hi;
}
template <> __device__ __forceinline__ void store8<bf16_t>(bf16_t* p, const f8& v) {
  *reinterpret_cast<vnx_u4*>(p) = vnx_u4{f32x2_to_bf16x2(v.lo.x, v.lo.y), f32x2_to_bf16x2(v.lo.z, v.lo.w),
                                         f32x2_to_bf16x2(v.hi.x, v.hi.y), f32x2_to_bf16x2(v.hi.z, v.hi.w)};
}
// the value as T stores it
template <typename T> __device__ __forceinline__ f8 rounded8(const f8& v);
template <> __device__ __forceinline__ f8 rounded8<float>(const f8& v) { return v; }
template <> __device__ __forceinline__ f8 rounded8<bf16_t>(const f8& v) {
  const uint32_t a = f32x2_to_bf16x2(v.lo.x, v.lo.y), b = f32x2_to_bf16x2(v.lo.z, v.lo.w);
  const uint32_t c = f32x2_to_bf16x2(v.hi.x, v.hi.y), d = f32x2_to_bf16x2(v.hi.z, v.hi.w);
  return f8{vnx_f4{__uint_as_float(a << 16), __uint_as_float(a & 0xffff0000u), __uint_as_float(b << 16), __uint_as_float(b & 0xffff0000u)},
            vnx_f4{__uint_as_float(c << 16), __uint_as_float(c & 0xffff0000u), __uint_as_float(d << 16), __uint_as_float(d & 0xffff0000u)}};
}

__device__ __forceinline__ float sum8(const f8& v) {
  return ((v.lo.x + v.lo.y) + (v.lo.z + v.lo.w)) + ((v.hi.x + v.hi.y) + (v.hi.z + v.hi.w));
}
__device__ __forceinline__ float dot8(const f8& a, const f8& b) {
  return ((a.lo.x * b.lo.x + a.lo.y * b.lo.y) + (a.lo.z * b.lo.z + a.lo.w * b.lo.w)) +
         ((a.hi.x * b.hi.x + a.hi.y * b.hi.y) + (a.hi.z * b.hi.z + a.hi.w * b.hi.w));
}

// the sum over the G lanes of a group, in every lane of the group
template <int G> __device__ __forceinline__ float group_sum(float v) {
#pragma unroll
  for (int off = G / 2; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// where the rows of a launch live: streamed rows of C channels, or (MERGE) rows gathered from x [B, H, W, C / 4]
struct SgShape {
  int64_t rows;               // rows of C channels
  int C;                      // channels of a row (MERGE: 4 x the input's)
  int64_t rows_per_sample;    // rows that share one scale (streamed rows)
  int H, W, H2, W2;           // MERGE: the input grid and the output grid (ceil of the halves)
};

// row / d (d >= 1): 32-bit arithmetic while the launch's rows fit (a 64-bit division is some forty instructions per row)
__device__ __forceinline__ int64_t sg_div(const SgShape& s, int64_t row, int64_t d) {
  return s.rows <= 0x7fffffffLL ? int64_t(uint32_t(row) / uint32_t(d < 0x7fffffffLL ? d : 0x7fffffffLL)) : row / d;
}

// MERGE: element offset of chunk k of output row (b, i, j) in x, or -1 for a pad pixel
__device__ __forceinline__ int64_t sg_merge_at(const SgShape& s, int64_t b, int i, int j, int k) {
  const int Cin = s.C >> 2, c8 = k << 3;
  const int q = (c8 >= Cin) + (c8 >= 2 * Cin) + (c8 >= 3 * Cin);
  const int h = 2 * i + (q & 1), w = 2 * j + (q >> 1);
  if (h >= s.H || w >= s.W) return -1;
  return ((b * s.H + h) * s.W + w) * Cin + (c8 - q * Cin);
}

template <int G, int NCH, typename TX, typename TA, typename TN, bool MERGE>
__global__ void __launch_bounds__(kSgThreads)
swin_glue_fwd_kernel(const TX* __restrict__ x, const TA* __restrict__ a, const float* __restrict__ scale,
                     const float* __restrict__ gamma, const float* __restrict__ beta, TX* __restrict__ y,
                     TN* __restrict__ n, float* __restrict__ stats, SgShape s, float eps) {
  constexpr int kRows = 64 / G;                              // rows per wave
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int l = lane % G, grp = lane / G;
  const int nchunks = s.C >> 3;
  const float inv_c = 1.f / float(s.C);
  const int64_t stride = int64_t(gridDim.x) * (kSgWaves * kRows);
  for (int64_t row = (int64_t(blockIdx.x) * kSgWaves + wave) * kRows + grp; row < s.rows; row += stride) {
    int64_t mb = 0;
    int mi = 0, mj = 0;
    float sc = 1.f;
    if (MERGE) {
      const int64_t per = int64_t(s.H2) * s.W2;
      mb = sg_div(s, row, per);
      const int rem = int(row - mb * per);
      mi = rem / s.W2;
      mj = rem - mi * s.W2;
    } else if (a != nullptr && scale != nullptr) {
      sc = scale[sg_div(s, row, s.rows_per_sample)];
    }
    f8 v[NCH];
    float sum = 0.f;
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      const int k = l + G * c;
      v[c] = zero8();
      if (k < nchunks) {
        if (MERGE) {
          const int64_t at = sg_merge_at(s, mb, mi, mj, k);
          if (at >= 0) v[c] = load8<TX>(x + at);
        } else {
          const int64_t at = row * s.C + (k << 3);
          v[c] = load8<TX>(x + at);
          if (a != nullptr) {
            if (sc != 0.f) {                                 // a dropped sample: y = x bit for bit, its branch is not read
              const f8 av = load8<TA>(a + at);
              v[c].lo = av.lo * sc + v[c].lo;
              v[c].hi = av.hi * sc + v[c].hi;
              v[c] = rounded8<TX>(v[c]);
            }
            store8<TX>(y + at, v[c]);
          }
        }
        sum += sum8(v[c]);
      }
    }
    if (gamma == nullptr) continue;                          // the plain scaled add
    const float mean = group_sum<G>(sum) * inv_c;
    float sq = 0.f;
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      if (l + G * c < nchunks) {
        v[c].lo -= mean;
        v[c].hi -= mean;
        sq += dot8(v[c], v[c]);
      }
    }
    const float rstd = rsqrtf(group_sum<G>(sq) * inv_c + eps);
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      const int k = l + G * c;
      if (k < nchunks) {
        const f8 g = load8<float>(gamma + (k << 3)), b = load8<float>(beta + (k << 3));
        f8 o;
        o.lo = v[c].lo * rstd * g.lo + b.lo;
        o.hi = v[c].hi * rstd * g.hi + b.hi;
        store8<TN>(n + row * s.C + (k << 3), o);
      }
    }
    if (l == 0) { stats[2 * row] = mean; stats[2 * row + 1] = rstd; }
  }
}

template <int G, int NCH, typename TX, typename TA, typename TN, bool MERGE>
__global__ void __launch_bounds__(kSgThreads)
swin_glue_bwd_kernel(const TX* __restrict__ grad_y, const TN* __restrict__ grad_n, const TX* __restrict__ y,
                     const float* __restrict__ stats, const float* __restrict__ gamma, const float* __restrict__ scale,
                     TX* __restrict__ grad_x, TA* __restrict__ grad_a, float* __restrict__ partial, SgShape s) {
  constexpr int kRows = 64 / G;
  __shared__ vnx_f4 red[4][kSgThreads];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int l = lane % G, grp = lane / G;
  const int nchunks = s.C >> 3;
  const float inv_c = 1.f / float(s.C);
  const int64_t stride = int64_t(gridDim.x) * (kSgWaves * kRows);
  f8 dg[NCH], db[NCH];
#pragma unroll
  for (int c = 0; c < NCH; ++c) dg[c] = db[c] = zero8();
  for (int64_t row = (int64_t(blockIdx.x) * kSgWaves + wave) * kRows + grp; row < s.rows; row += stride) {
    int64_t mb = 0;
    int mi = 0, mj = 0;
    float sc = 1.f;
    if (MERGE) {
      const int64_t per = int64_t(s.H2) * s.W2;
      mb = sg_div(s, row, per);
      const int rem = int(row - mb * per);
      mi = rem / s.W2;
      mj = rem - mi * s.W2;
    } else if (grad_a != nullptr && scale != nullptr) {
      sc = scale[sg_div(s, row, s.rows_per_sample)];
    }
    f8 g[NCH];                                               // the gradient of the row: LayerNorm's part first
#pragma unroll
    for (int c = 0; c < NCH; ++c) g[c] = zero8();
    if (grad_n != nullptr) {
      const float mean = stats[2 * row], rstd = stats[2 * row + 1];
      f8 xh[NCH];
      float m1 = 0.f, m2 = 0.f;
#pragma unroll
      for (int c = 0; c < NCH; ++c) {
        const int k = l + G * c;
        xh[c] = zero8();
        if (k < nchunks) {
          f8 yv = zero8();
          if (MERGE) {
            const int64_t at = sg_merge_at(s, mb, mi, mj, k);
            if (at >= 0) yv = load8<TX>(y + at);
          } else {
            yv = load8<TX>(y + row * s.C + (k << 3));
          }
          const f8 gn = load8<TN>(grad_n + row * s.C + (k << 3));
          const f8 gm = load8<float>(gamma + (k << 3));
          xh[c].lo = (yv.lo - mean) * rstd;
          xh[c].hi = (yv.hi - mean) * rstd;
          dg[c].lo += gn.lo * xh[c].lo;
          dg[c].hi += gn.hi * xh[c].hi;
          db[c].lo += gn.lo;
          db[c].hi += gn.hi;
          g[c].lo = gn.lo * gm.lo;
          g[c].hi = gn.hi * gm.hi;
          m1 += sum8(g[c]);
          m2 += dot8(g[c], xh[c]);
        }
      }
      m1 = group_sum<G>(m1) * inv_c;
      m2 = group_sum<G>(m2) * inv_c;
#pragma unroll
      for (int c = 0; c < NCH; ++c) {
        g[c].lo = (g[c].lo - m1 - xh[c].lo * m2) * rstd;
        g[c].hi = (g[c].hi - m1 - xh[c].hi * m2) * rstd;
      }
    }
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      const int k = l + G * c;
      if (k < nchunks) {
        if (MERGE) {
          const int64_t at = sg_merge_at(s, mb, mi, mj, k);
          if (at >= 0) store8<TX>(grad_x + at, g[c]);        // a pad pixel has no gradient
        } else {
          const int64_t at = row * s.C + (k << 3);
          if (grad_y != nullptr) {
            const f8 gy = load8<TX>(grad_y + at);
            g[c].lo += gy.lo;
            g[c].hi += gy.hi;
          }
          store8<TX>(grad_x + at, g[c]);
          if (grad_a != nullptr) {
            f8 ga = zero8();                                 // a dropped sample: exactly 0
            if (sc != 0.f) { ga.lo = g[c].lo * sc; ga.hi = g[c].hi * sc; }
            store8<TA>(grad_a + at, ga);
          }
        }
      }
    }
  }
  if (partial == nullptr) return;                            // no LayerNorm at this site (uniform over the launch)
  // the lanes l, l + G, l + 2 G, .. of the workgroup hold the same columns: thread l adds them in that order
  float* out = partial + int64_t(blockIdx.x) * 2 * s.C;
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    red[0][threadIdx.x] = dg[c].lo;
    red[1][threadIdx.x] = dg[c].hi;
    red[2][threadIdx.x] = db[c].lo;
    red[3][threadIdx.x] = db[c].hi;
    __syncthreads();
    const int k = int(threadIdx.x) + G * c;
    if (int(threadIdx.x) < G && k < nchunks) {
      vnx_f4 s0 = red[0][threadIdx.x], s1 = red[1][threadIdx.x], s2 = red[2][threadIdx.x], s3 = red[3][threadIdx.x];
      for (int t = int(threadIdx.x) + G; t < kSgThreads; t += G) {
        s0 += red[0][t]; s1 += red[1][t]; s2 += red[2][t]; s3 += red[3][t];
      }
      store8<float>(out + (k << 3), f8{s0, s1});
      store8<float>(out + s.C + (k << 3), f8{s2, s3});
    }
    __syncthreads();
  }
}

// grad_gamma[c] = sum_b partial[b][0][c], grad_beta[c] = sum_b partial[b][1][c]: thread (slice, column) adds the partial
// rows slice, slice + 16, .., and the slices meet in a fixed-order tree.  blocks == 0 writes zeros.
__global__ void __launch_bounds__(kSgFinCols * kSgFinSlices)
swin_glue_param_grad_kernel(const float* __restrict__ partial, float* __restrict__ grad_gamma,
                            float* __restrict__ grad_beta, int blocks, int C) {
  __shared__ float red[kSgFinSlices][kSgFinCols];
  const int c = threadIdx.x % kSgFinCols, slice = threadIdx.x / kSgFinCols;
  const int col = int(blockIdx.x) * kSgFinCols + c;          // 0 .. 2 C - 1: gamma | beta (2 C is a multiple of 16)
  float sum = 0.f;
  for (int b = slice; b < blocks; b += kSgFinSlices) sum += partial[int64_t(b) * 2 * C + col];
  red[slice][c] = sum;
  __syncthreads();
#pragma unroll
  for (int step = kSgFinSlices / 2; step > 0; step >>= 1) {
    if (slice < step) red[slice][c] += red[slice + step][c];
    __syncthreads();
  }
  if (slice == 0) {
    if (col < C) grad_gamma[col] = red[0][c];
    else grad_beta[col - C] = red[0][c];
  }
}

struct SgGeom { int G, NCH; };
// the smallest group that covers the row's chunks with one slot; above 64 chunks, whole waves with 2, 3 or 6 slots
SgGeom sg_geometry(int channels) {
  const int chunks = channels / 8;
  if (chunks <= 8) return {8, 1};
  if (chunks <= 16) return {16, 1};
  if (chunks <= 32) return {32, 1};
  if (chunks <= 64) return {64, 1};
  if (chunks <= 128) return {64, 2};
  if (chunks <= 192) return {64, 3};
  return {64, 6};
}

int64_t sg_passes(int64_t rows, int channels) {              // workgroup passes that cover the rows once
  const int per = kSgWaves * (64 / sg_geometry(channels).G);
  return (rows + per - 1) / per;
}

int sg_bwd_blocks(int64_t rows, int channels) {
  const int64_t passes = sg_passes(rows, channels);
  return int(std::min<int64_t>(kSgMaxBlocks, (passes + kSgRowsPerBlock - 1) / kSgRowsPerBlock));
}

bool sg_aligned(const void* p) { return (uintptr_t(p) & 15) == 0; }

int sg_check(const char* who, int x_dtype, int a_dtype, int n_dtype, int64_t rows, int channels) {
  const bool types = (x_dtype == VNX_F32 && a_dtype == VNX_F32 && n_dtype == VNX_F32) ||
                     (x_dtype == VNX_F32 && a_dtype == VNX_BF16 && n_dtype == VNX_BF16) ||
                     (x_dtype == VNX_BF16 && a_dtype == VNX_BF16 && n_dtype == VNX_BF16);
  if (!types) {
    set_error("%s: (stream, branch, norm) types are (f32, f32, f32), (f32, bf16, bf16) or (bf16, bf16, bf16) (got %d, %d, %d)",
              who, x_dtype, a_dtype, n_dtype);
    return VNX_ERR_UNSUPPORTED;
  }
  if (channels < 32 || channels > 3072 || channels % 8 != 0) {
    set_error("%s: rows of 32 .. 3072 channels, a multiple of 8 (got %d)", who, channels);
    return VNX_ERR_UNSUPPORTED;
  }
  if (rows < 0 || rows >= (int64_t(1) << 40)) {
    set_error("%s: bad row count %lld", who, (long long)rows);
    return VNX_ERR_INVALID_ARGUMENT;
  }
  return VNX_OK;
}

template <typename TX, typename TA, typename TN, bool MERGE>
void sg_launch_fwd(SgGeom geom, dim3 grid, hipStream_t stream, const void* x, const void* a, const void* scale,
                   const void* gamma, const void* beta, void* y, void* n, void* stats, const SgShape& s, float eps) {
#define VNX_SG_FWD(G, NCH)                                                                                              \
  hipLaunchKernelGGL((swin_glue_fwd_kernel<G, NCH, TX, TA, TN, MERGE>), grid, dim3(kSgThreads), 0, stream, (const TX*)x, \
                     (const TA*)a, (const float*)scale, (const float*)gamma, (const float*)beta, (TX*)y, (TN*)n,        \
                     (float*)stats, s, eps)
  if (geom.G == 8) VNX_SG_FWD(8, 1);
  else if (geom.G == 16) VNX_SG_FWD(16, 1);
  else if (geom.G == 32) VNX_SG_FWD(32, 1);
  else if (geom.NCH == 1) VNX_SG_FWD(64, 1);
  else if (geom.NCH == 2) VNX_SG_FWD(64, 2);
  else if (geom.NCH == 3) VNX_SG_FWD(64, 3);
  else VNX_SG_FWD(64, 6);
#undef VNX_SG_FWD
}

template <typename TX, typename TA, typename TN, bool MERGE>
void sg_launch_bwd(SgGeom geom, dim3 grid, hipStream_t stream, const void* grad_y, const void* grad_n, const void* y,
                   const void* stats, const void* gamma, const void* scale, void* grad_x, void* grad_a, void* partial,
                   const SgShape& s) {
#define VNX_SG_BWD(G, NCH)                                                                                              \
  hipLaunchKernelGGL((swin_glue_bwd_kernel<G, NCH, TX, TA, TN, MERGE>), grid, dim3(kSgThreads), 0, stream,               \
                     (const TX*)grad_y, (const TN*)grad_n, (const TX*)y, (const float*)stats, (const float*)gamma,      \
                     (const float*)scale, (TX*)grad_x, (TA*)grad_a, (float*)partial, s)
  if (geom.G == 8) VNX_SG_BWD(8, 1);
  else if (geom.G == 16) VNX_SG_BWD(16, 1);
  else if (geom.G == 32) VNX_SG_BWD(32, 1);
  else if (geom.NCH == 1) VNX_SG_BWD(64, 1);
  else if (geom.NCH == 2) VNX_SG_BWD(64, 2);
  else if (geom.NCH == 3) VNX_SG_BWD(64, 3);
  else VNX_SG_BWD(64, 6);
#undef VNX_SG_BWD
}

template <bool MERGE>
int sg_forward(const char* who, int x_dtype, int a_dtype, int n_dtype, const void* x, const void* a, const void* scale,
               const void* gamma, const void* beta, void* y, void* n, void* stats, const SgShape& s, float eps,
               void* hip_stream) {
  if (int st = sg_check(who, x_dtype, a_dtype, n_dtype, s.rows, s.C)) return st;
  if (s.rows == 0) return VNX_OK;
  if (!x || (a && !y) || (gamma && (!beta || !n || !stats)) || (!a && !gamma) || (!MERGE && s.rows_per_sample < 1)) {
    set_error("%s: null pointer argument, nothing to compute, or rows_per_sample < 1", who);
    return VNX_ERR_INVALID_ARGUMENT;
  }
  if (!sg_aligned(x) || !sg_aligned(a) || !sg_aligned(y) || !sg_aligned(n) || !sg_aligned(gamma) || !sg_aligned(beta)) {
    set_error("%s: rows and parameters must be 16-byte aligned", who);
    return VNX_ERR_UNSUPPORTED;
  }
  const SgGeom geom = sg_geometry(s.C);
  const dim3 grid(uint32_t(std::min<int64_t>(sg_passes(s.rows, s.C), int64_t(1) << 20)));
  hipStream_t stream = (hipStream_t)hip_stream;
  if (x_dtype == VNX_BF16) sg_launch_fwd<bf16_t, bf16_t, bf16_t, MERGE>(geom, grid, stream, x, a, scale, gamma, beta, y, n, stats, s, eps);
  else if (n_dtype == VNX_BF16) sg_launch_fwd<float, bf16_t, bf16_t, MERGE>(geom, grid, stream, x, a, scale, gamma, beta, y, n, stats, s, eps);
  else sg_launch_fwd<float, float, float, MERGE>(geom, grid, stream, x, a, scale, gamma, beta, y, n, stats, s, eps);
  return check_launch(who);
}

template <bool MERGE>
int sg_backward(const char* who, int x_dtype, int a_dtype, int n_dtype, const void* grad_y, const void* grad_n,
                const void* y, const void* stats, const void* gamma, const void* scale, void* grad_x, void* grad_a,
                void* grad_gamma, void* grad_beta, void* partial, size_t partial_bytes, const SgShape& s,
                void* hip_stream) {
  if (int st = sg_check(who, x_dtype, a_dtype, n_dtype, s.rows, s.C)) return st;
  const bool norm = gamma != nullptr;
  if ((norm && (!grad_gamma || !grad_beta || !partial)) || (!norm && grad_n) || (!MERGE && s.rows_per_sample < 1)) {
    set_error("%s: null pointer argument (a site with a LayerNorm takes gamma, both parameter gradients and the partial buffer; "
              "one without takes no grad_n), or rows_per_sample < 1", who);
    return VNX_ERR_INVALID_ARGUMENT;
  }
  const int blocks = s.rows > 0 ? sg_bwd_blocks(s.rows, s.C) : 0;
  if (norm && partial_bytes < size_t(blocks) * 2 * s.C * sizeof(float)) {
    set_error("%s: the partial buffer holds %zu bytes, the launch needs %zu", who, partial_bytes,
              size_t(blocks) * 2 * s.C * sizeof(float));
    return VNX_ERR_INVALID_ARGUMENT;
  }
  hipStream_t stream = (hipStream_t)hip_stream;
  if (s.rows > 0) {
    if (!grad_x || (grad_n && (!y || !stats))) {
      set_error("%s: null pointer argument", who);
      return VNX_ERR_INVALID_ARGUMENT;
    }
    if (!sg_aligned(grad_y) || !sg_aligned(grad_n) || !sg_aligned(y) || !sg_aligned(gamma) || !sg_aligned(grad_x) ||
        !sg_aligned(grad_a) || !sg_aligned(partial)) {
      set_error("%s: rows, parameters and the partial buffer must be 16-byte aligned", who);
      return VNX_ERR_UNSUPPORTED;
    }
    const SgGeom geom = sg_geometry(s.C);
    const dim3 grid{uint32_t(blocks)};
    void* part = norm ? partial : nullptr;
    if (x_dtype == VNX_BF16) sg_launch_bwd<bf16_t, bf16_t, bf16_t, MERGE>(geom, grid, stream, grad_y, grad_n, y, stats, gamma, scale, grad_x, grad_a, part, s);
    else if (n_dtype == VNX_BF16) sg_launch_bwd<float, bf16_t, bf16_t, MERGE>(geom, grid, stream, grad_y, grad_n, y, stats, gamma, scale, grad_x, grad_a, part, s);
    else sg_launch_bwd<float, float, float, MERGE>(geom, grid, stream, grad_y, grad_n, y, stats, gamma, scale, grad_x, grad_a, part, s);
  }
  if (norm)
    hipLaunchKernelGGL(swin_glue_param_grad_kernel, dim3(uint32_t(2 * s.C / kSgFinCols)), dim3(kSgFinCols * kSgFinSlices), 0,
                       stream, (const float*)partial, (float*)grad_gamma, (float*)grad_beta, grad_n ? blocks : 0, s.C);
  return check_launch(who);
}

int sg_merge_shape(const char* who, int batch, int height, int width, int channels, SgShape* s) {
  if (batch < 0 || height < 1 || width < 1 || channels < 8 || channels % 8 != 0 ||
      int64_t(batch) * height * width * channels >= (int64_t(1) << 46)) {
    set_error("%s: bad sizes batch=%d height=%d width=%d channels=%d (channels: a multiple of 8)", who, batch, height, width, channels);
    return channels > 0 && channels % 8 != 0 ? VNX_ERR_UNSUPPORTED : VNX_ERR_INVALID_ARGUMENT;
  }
  s->H = height; s->W = width; s->H2 = (height + 1) / 2; s->W2 = (width + 1) / 2;
  s->rows = int64_t(batch) * s->H2 * s->W2;
  s->C = 4 * std::min(channels, 1 << 20);                     // above 3072: sg_check refuses it
  s->rows_per_sample = 1;
  return VNX_OK;
}

}  // namespace

}  // namespace vnx

using namespace vnx;

extern "C" size_t vnx_swin_glue_partial_bytes(long long rows, int channels) {
  if (rows <= 0 || channels < 32 || channels > 3072 || channels % 8 != 0) return 16;
  return std::max<size_t>(16, size_t(sg_bwd_blocks(rows, channels)) * 2 * channels * sizeof(float));
}

extern "C" int vnx_swin_residual_norm_forward(int x_dtype, int a_dtype, int n_dtype, const void* x, const void* a,
                                              const void* scale, const void* gamma, const void* beta, void* y, void* n,
                                              void* stats, long long rows, int channels, long long rows_per_sample,
                                              float eps, void* hip_stream) {
  const SgShape s{rows, channels, rows_per_sample, 0, 0, 0, 0};
  return sg_forward<false>("vnx_swin_residual_norm_forward", x_dtype, a_dtype, n_dtype, x, a, scale, gamma, beta, y, n,
                           stats, s, eps, hip_stream);
}

extern "C" int vnx_swin_residual_norm_backward(int x_dtype, int a_dtype, int n_dtype, const void* grad_y,
                                               const void* grad_n, const void* y, const void* stats, const void* gamma,
                                               const void* scale, void* grad_x, void* grad_a, void* grad_gamma,
                                               void* grad_beta, void* partial, size_t partial_bytes, long long rows,
                                               int channels, long long rows_per_sample, void* hip_stream) {
  const SgShape s{rows, channels, rows_per_sample, 0, 0, 0, 0};
  return sg_backward<false>("vnx_swin_residual_norm_backward", x_dtype, a_dtype, n_dtype, grad_y, grad_n, y, stats, gamma,
                            scale, grad_x, grad_a, grad_gamma, grad_beta, partial, partial_bytes, s, hip_stream);
}

extern "C" int vnx_swin_merge_norm_forward(int x_dtype, int n_dtype, const void* x, const void* gamma, const void* beta,
                                           void* n, void* stats, int batch, int height, int width, int channels,
                                           float eps, void* hip_stream) {
  SgShape s{};
  if (int st = sg_merge_shape("vnx_swin_merge_norm_forward", batch, height, width, channels, &s)) return st;
  if (!gamma) { set_error("vnx_swin_merge_norm_forward: null pointer argument"); return VNX_ERR_INVALID_ARGUMENT; }
  return sg_forward<true>("vnx_swin_merge_norm_forward", x_dtype, n_dtype, n_dtype, x, nullptr, nullptr, gamma, beta,
                          nullptr, n, stats, s, eps, hip_stream);
}

extern "C" int vnx_swin_merge_norm_backward(int x_dtype, int n_dtype, const void* grad_n, const void* x, const void* stats,
                                            const void* gamma, void* grad_x, void* grad_gamma, void* grad_beta,
                                            void* partial, size_t partial_bytes, int batch, int height, int width,
                                            int channels, void* hip_stream) {
  SgShape s{};
  if (int st = sg_merge_shape("vnx_swin_merge_norm_backward", batch, height, width, channels, &s)) return st;
  if (!gamma || !grad_n) { set_error("vnx_swin_merge_norm_backward: null pointer argument"); return VNX_ERR_INVALID_ARGUMENT; }
  return sg_backward<true>("vnx_swin_merge_norm_backward", x_dtype, n_dtype, n_dtype, nullptr, grad_n, x,
                           stats, gamma, nullptr, grad_x, nullptr, grad_gamma, grad_beta, partial, partial_bytes, s,
                           hip_stream);
}
