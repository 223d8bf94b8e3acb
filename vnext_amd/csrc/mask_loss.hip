// mask_loss.hip -- the mask losses of both criteria (sigmoid focal + dice over the matched instances' mask logits) in one
// pass each way, the ground truth read IN PLACE at image resolution.
//
// What it replaces (criterion.py / idol_criterion.py, reference segmentation_condInst.py:680-723): per target dict a
// slice [s/2::s, s/2::s], a cast to float and a pad to the canvas, one cat, one gather with the matched target indices --
// a float copy of the ground truth as large as the logits -- and about twenty element-wise / reduction launches over
// [R, M] whose intermediates autograd keeps for a backward of as many launches again.
//
// Here: logits fp32 [R][F][h][w] (M = F h w per row), row_gt int64 [R] (the row's target, counted over the clips' targets
// laid back to back), and per clip a bool / uint8 tensor [n_i][F][H_i][W_i].  The target of logit (r, f, y, x) is
//   gt[row_gt[r]][f][y * stride + stride / 2][x * stride + stride / 2]     where that pixel exists, 0 where it does not
// (the reference's "slice, then zero-pad").  The per-clip base pointers, shapes and first-target offsets travel BY VALUE in
// the kernel arguments (vnx_mask_loss_clips, up to 16 clips): nothing is uploaded.  A row's clip is the same for every
// lane of a workgroup; its index goes through readfirstlane so that the table is read with scalar loads from the
// kernel-argument segment and is never copied to scratch.
//
// For a 0/1 target t the element reduces to   z = t ? x : -x,  ce = softplus(-z),  1 - p_t = s = sigmoid(-z):
//   focal = alpha_t * ce * s^gamma                               (alpha_t = t ? alpha : 1 - alpha; 1 when alpha < 0)
//   dfocal/dz = -alpha_t * s^gamma * (s + gamma * ce * (1 - s)),  dz/dx = t ? 1 : -1
//   dice = 1 - num / den,  num = 2 sum(p t) + 1,  den = sum(p) + sum(t) + 1,  ddice/dp = -(2 t den - num) / den^2
// with e = exp(-|x|) computed once: sigmoid = 1 / (1 + e) or e / (1 + e), softplus = log1p(e) + max(-z, 0).  Accurate expf /
// log1pf / division: this file is compiled without fast-math like the rest of the library.
//
// Forward, launch 1 (mask_loss_fwd_kernel): a workgroup of 256 lanes owns one PIECE of kMlPiece = 4096 consecutive logits of
// one row.  Where w is a multiple of 4 (and the logits are 16-byte aligned) a lane reads four logits with one 16-byte load
// -- they share (f, y) -- and, at stride 4 on a clip whose width is a multiple of 16, their four ground-truth bytes (columns
// 4x + 2, + 6, + 10, + 14) with one aligned 16-byte load; other strides and widths read the four bytes one by one, and
// other w take an element-per-lane path: any h, w, H_i, W_i works.  Four partial sums per piece (focal, p t, p, t): 16
// elements in the lane, lane exchange across the wave, LDS across the four waves, ONE 16-byte store per piece.
// Launch 2 (mask_loss_finish_kernel): one wave per row adds the row's pieces in a fixed order and writes focal[r] (the
// mean), dice[r] and the three row sums the backward needs.  No atomics anywhere: the result is a function of the input
// alone (bit-identical run to run).
// Backward (mask_loss_bwd_kernel): one element-wise launch over the same pieces; it recomputes e, s and p from the logits
// and the ground truth -- the forward saves nothing of [R, M] size -- and stores grad_logits 16 bytes per lane.
//
// A row whose row_gt is outside [0, total) has no ground truth: its target is 0 everywhere (the kernels never read
// outside a clip's tensor).
#include "vnx_common.h"

namespace vnx {
namespace {

constexpr int kMlThreads = 256;
constexpr int kMlPiece = VNX_MASK_LOSS_PIECE;                     // logits per workgroup
constexpr int kMlPerLane = kMlPiece / kMlThreads;                 // 16
static_assert(kMlPiece % (4 * kMlThreads) == 0, "a piece is whole 16-byte loads per lane");

struct MlDims {
  int R, F, h, w;        // logits [R][F][h][w]
  int M, hw, pieces;     // F h w, h w, ceil(M / kMlPiece)
  int stride, vec;       // vec: w % 4 == 0 and 16-byte aligned rows
  float alpha, gamma;
};

// the ground truth of one row: a clip's plane geometry and the row's first byte, all wave-uniform
struct MlRowGt {
  const unsigned char* base;      // frame 0 of the row's target; null = no ground truth (target 0)
  int H, W;
  int wide;                       // stride 4, W % 16 == 0, base 16-byte aligned: four targets from one 16-byte load
};

__device__ __forceinline__ MlRowGt ml_row_gt(const vnx_mask_loss_clips& clips, const int64_t* __restrict__ row_gt, int r,
                                             int F, int stride) {
  MlRowGt g{nullptr, 0, 0, 0};
  const int64_t t = row_gt[r];
  if (t < 0 || t >= int64_t(clips.total)) return g;
  int c = 0;                      // the last clip whose first target is <= t (clips without targets own nothing)
#pragma unroll
  for (int i = 1; i < VNX_MASK_LOSS_MAX_CLIPS; ++i)
    if (i < clips.count && int64_t(clips.first[i]) <= t) c = i;
  c = __builtin_amdgcn_readfirstlane(c);
  g.H = clips.height[c];
  g.W = clips.width[c];
  g.base = static_cast<const unsigned char*>(clips.masks[c]) + (t - clips.first[c]) * int64_t(F) * g.H * g.W;
  g.wide = stride == 4 && (g.W & 15) == 0 && (reinterpret_cast<uintptr_t>(clips.masks[c]) & 15) == 0;
  return g;
}

// targets of logits (f, y, x .. x + 3) as bits 0..3
__device__ __forceinline__ uint32_t ml_gt4(const MlRowGt& g, int f, int y, int x, int stride) {
  const int yy = y * stride + (stride >> 1);
  if (g.base == nullptr || yy >= g.H) return 0u;
  const unsigned char* row = g.base + (int64_t(f) * g.H + yy) * g.W;
  if (g.wide) {
    if (4 * x >= g.W) return 0u;                                  // W % 16 == 0 and x % 4 == 0: all four inside, or none
    typedef uint32_t u4 __attribute__((ext_vector_type(4)));
    const u4 v = *reinterpret_cast<const u4*>(row + 4 * x);       // byte 2 of each word: columns 4 (x + j) + 2
    return ((v.x & 0xff0000u) ? 1u : 0u) | ((v.y & 0xff0000u) ? 2u : 0u) | ((v.z & 0xff0000u) ? 4u : 0u) |
           ((v.w & 0xff0000u) ? 8u : 0u);
  }
  uint32_t bits = 0u;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int xx = (x + j) * stride + (stride >> 1);
    if (xx < g.W && row[xx] != 0) bits |= 1u << j;
  }
  return bits;
}

__device__ __forceinline__ bool ml_gt1(const MlRowGt& g, int f, int y, int x, int stride) {
  const int yy = y * stride + (stride >> 1), xx = x * stride + (stride >> 1);
  if (g.base == nullptr || yy >= g.H || xx >= g.W) return false;
  return g.base[(int64_t(f) * g.H + yy) * g.W + xx] != 0;
}

// what both directions need of one element
struct MlElem { float p, s, q, ce, at, sg; };      // sigmoid(x), sigmoid(-z), sigmoid(z), softplus(-z), alpha_t, s^gamma
__device__ __forceinline__ MlElem ml_elem(float x, bool t, float alpha, float gamma) {
  MlElem m;
  const float e = expf(-fabsf(x));
  const float inv = 1.f / (1.f + e);
  const float lo = e * inv;                        // the sigmoid of -|x|
  m.p = x >= 0.f ? inv : lo;
  const float z = t ? x : -x;
  m.s = z >= 0.f ? lo : inv;
  m.q = z >= 0.f ? inv : lo;
  m.ce = log1pf(e) + fmaxf(-z, 0.f);
  m.at = alpha >= 0.f ? (t ? alpha : 1.f - alpha) : 1.f;
  m.sg = gamma == 2.f ? m.s * m.s : powf(m.s, gamma);
  return m;
}

struct MlSums { float focal, pt, p, t; };
__device__ __forceinline__ void ml_accumulate(MlSums& a, float x, bool t, float alpha, float gamma) {
  const MlElem m = ml_elem(x, t, alpha, gamma);
  a.focal += m.at * m.ce * m.sg;
  a.pt += t ? m.p : 0.f;
  a.p += m.p;
  a.t += t ? 1.f : 0.f;
}

}  // namespace

// grid: R * pieces workgroups; partial [R][pieces][4] = {sum focal, sum p t, sum p, sum t} of the piece
__global__ void __launch_bounds__(kMlThreads) mask_loss_fwd_kernel(const float* __restrict__ logits,
                                                                   const vnx_mask_loss_clips clips,
                                                                   const int64_t* __restrict__ row_gt, const MlDims d,
                                                                   float* __restrict__ partial) {
  __shared__ float s_part[kMlThreads / 64][4];
  const int r = int(blockIdx.x) / d.pieces, piece = int(blockIdx.x) - r * d.pieces;
  const MlRowGt g = ml_row_gt(clips, row_gt, r, d.F, d.stride);
  const float* row = logits + int64_t(r) * d.M;
  const int e0 = piece * kMlPiece;
  MlSums a{0.f, 0.f, 0.f, 0.f};
  if (d.vec) {
#pragma unroll
    for (int i = 0; i < kMlPerLane / 4; ++i) {
      const int e = e0 + 4 * (i * kMlThreads + int(threadIdx.x));
      if (e < d.M) {                                              // M % 4 == 0: the whole group is inside
        const vnx_f4 v = *reinterpret_cast<const vnx_f4*>(row + e);
        const int f = e / d.hw, rem = e - f * d.hw, y = rem / d.w, x = rem - y * d.w;
        const uint32_t bits = ml_gt4(g, f, y, x, d.stride);
        ml_accumulate(a, v.x, bits & 1u, d.alpha, d.gamma);
        ml_accumulate(a, v.y, bits & 2u, d.alpha, d.gamma);
        ml_accumulate(a, v.z, bits & 4u, d.alpha, d.gamma);
        ml_accumulate(a, v.w, bits & 8u, d.alpha, d.gamma);
      }
    }
  } else {
#pragma unroll 4
    for (int i = 0; i < kMlPerLane; ++i) {
      const int e = e0 + i * kMlThreads + int(threadIdx.x);
      if (e < d.M) {
        const int f = e / d.hw, rem = e - f * d.hw, y = rem / d.w, x = rem - y * d.w;
        ml_accumulate(a, row[e], ml_gt1(g, f, y, x, d.stride), d.alpha, d.gamma);
      }
    }
  }
  a.focal = wave_sum(a.focal);
  a.pt = wave_sum(a.pt);
  a.p = wave_sum(a.p);
  a.t = wave_sum(a.t);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) {
    s_part[wave][0] = a.focal; s_part[wave][1] = a.pt; s_part[wave][2] = a.p; s_part[wave][3] = a.t;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    vnx_f4 o = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int k = 0; k < kMlThreads / 64; ++k) {                   // the waves in order
      o.x += s_part[k][0]; o.y += s_part[k][1]; o.z += s_part[k][2]; o.w += s_part[k][3];
    }
    *reinterpret_cast<vnx_f4*>(partial + 4 * int64_t(blockIdx.x)) = o;
  }
}

// grid: R workgroups of one wave.  Lane l adds pieces l, l + 64, ... in order, then the 64 lane sums meet in a fixed
// exchange tree.  focal [R] (the row's mean), dice [R], row_sums [R][3] = {sum p t, sum p, sum t}.
__global__ void __launch_bounds__(64) mask_loss_finish_kernel(const float* __restrict__ partial, int pieces, int M,
                                                              float* __restrict__ focal, float* __restrict__ dice,
                                                              float* __restrict__ row_sums) {
  const int r = blockIdx.x, lane = threadIdx.x;
  const vnx_f4* p = reinterpret_cast<const vnx_f4*>(partial) + int64_t(r) * pieces;
  vnx_f4 a = {0.f, 0.f, 0.f, 0.f};
  for (int k = lane; k < pieces; k += 64) a += p[k];
  a.x = wave_sum(a.x);
  a.y = wave_sum(a.y);
  a.z = wave_sum(a.z);
  a.w = wave_sum(a.w);
  if (lane == 0) {
    focal[r] = a.x / float(M);
    dice[r] = 1.f - (2.f * a.y + 1.f) / (a.z + a.w + 1.f);
    row_sums[3 * int64_t(r)] = a.y;
    row_sums[3 * int64_t(r) + 1] = a.z;
    row_sums[3 * int64_t(r) + 2] = a.w;
  }
}

// grid: R * pieces workgroups.  grad_x = g_focal[r] / M * dfocal/dx + g_dice[r] * ddice/dp * p (1 - p)
__global__ void __launch_bounds__(kMlThreads) mask_loss_bwd_kernel(const float* __restrict__ logits,
                                                                   const vnx_mask_loss_clips clips,
                                                                   const int64_t* __restrict__ row_gt, const MlDims d,
                                                                   const float* __restrict__ row_sums,
                                                                   const float* __restrict__ grad_focal,
                                                                   const float* __restrict__ grad_dice,
                                                                   float* __restrict__ grad_logits) {
  const int r = int(blockIdx.x) / d.pieces, piece = int(blockIdx.x) - r * d.pieces;
  const MlRowGt g = ml_row_gt(clips, row_gt, r, d.F, d.stride);
  const float* row = logits + int64_t(r) * d.M;
  float* out = grad_logits + int64_t(r) * d.M;
  const float num = 2.f * row_sums[3 * int64_t(r)] + 1.f;
  const float den = row_sums[3 * int64_t(r) + 1] + row_sums[3 * int64_t(r) + 2] + 1.f;
  const float gf = grad_focal[r] / float(d.M), gd = grad_dice[r];
  // g_dice * ddice/dp for a target of 1 and of 0
  const float k1 = -gd * (2.f * den - num) / (den * den), k0 = gd * num / (den * den);
  const float alpha = d.alpha, gamma = d.gamma;
  auto grad = [&](float x, bool t) {
    const MlElem m = ml_elem(x, t, alpha, gamma);
    const float dz = -m.at * m.sg * (m.s + gamma * m.ce * m.q);
    return gf * (t ? dz : -dz) + (t ? k1 : k0) * (m.s * m.q);      // p (1 - p) = s (1 - s)
  };
  const int e0 = piece * kMlPiece;
  if (d.vec) {
#pragma unroll
    for (int i = 0; i < kMlPerLane / 4; ++i) {
      const int e = e0 + 4 * (i * kMlThreads + int(threadIdx.x));
      if (e < d.M) {
        const vnx_f4 v = *reinterpret_cast<const vnx_f4*>(row + e);
        const int f = e / d.hw, rem = e - f * d.hw, y = rem / d.w, x = rem - y * d.w;
        const uint32_t bits = ml_gt4(g, f, y, x, d.stride);
        const vnx_f4 o = {grad(v.x, bits & 1u), grad(v.y, bits & 2u), grad(v.z, bits & 4u), grad(v.w, bits & 8u)};
        *reinterpret_cast<vnx_f4*>(out + e) = o;
      }
    }
  } else {
#pragma unroll 4
    for (int i = 0; i < kMlPerLane; ++i) {
      const int e = e0 + i * kMlThreads + int(threadIdx.x);
      if (e < d.M) {
        const int f = e / d.hw, rem = e - f * d.hw, y = rem / d.w, x = rem - y * d.w;
        out[e] = grad(row[e], ml_gt1(g, f, y, x, d.stride));
      }
    }
  }
}

static int ml_dims(const char* fn, const void* logits, const vnx_mask_loss_clips* clips, int rows, int frames, int height,
                   int width, int stride, float alpha, float gamma, MlDims* d) {
  if (rows < 0 || frames < 1 || height < 1 || width < 1 || stride < 1) {
    set_error("%s: bad sizes (rows %d, frames %d, %d x %d, stride %d)", fn, rows, frames, height, width, stride);
    return VNX_ERR_INVALID_ARGUMENT;
  }
  if (!(gamma >= 0.f)) {
    set_error("%s: gamma %g must not be negative", fn, double(gamma));
    return VNX_ERR_INVALID_ARGUMENT;
  }
  const int64_t M = int64_t(frames) * height * width;
  const int64_t pieces = (M + kMlPiece - 1) / kMlPiece;
  if (M >= (int64_t(1) << 31) - kMlPiece || int64_t(rows) * pieces >= (int64_t(1) << 31) ||
      int64_t(height) * stride >= (int64_t(1) << 30) || int64_t(width) * stride >= (int64_t(1) << 30)) {
    set_error("%s: %d rows of %lld logits are outside what the kernel addresses", fn, rows, (long long)M);
    return VNX_ERR_UNSUPPORTED;
  }
  if (rows == 0) return VNX_OK;
  if (!clips) {
    set_error("%s: null pointer argument", fn);
    return VNX_ERR_INVALID_ARGUMENT;
  }
  if (clips->count < 0 || clips->count > VNX_MASK_LOSS_MAX_CLIPS || clips->total < 0) {
    set_error("%s: %d clips (at most %d), %d targets", fn, clips->count, VNX_MASK_LOSS_MAX_CLIPS, clips->total);
    return VNX_ERR_INVALID_ARGUMENT;
  }
  for (int i = 0; i < clips->count; ++i) {
    const int next = i + 1 < clips->count ? clips->first[i + 1] : clips->total;
    const bool empty = next == clips->first[i];
    if (clips->first[i] < 0 || next < clips->first[i] || (i == 0 && clips->first[0] != 0) || clips->height[i] < 0 ||
        clips->width[i] < 0 || (!empty && (!clips->masks[i] || clips->height[i] < 1 || clips->width[i] < 1))) {
      set_error("%s: clip %d: targets %d..%d of %d x %d at %p", fn, i, clips->first[i], next, clips->height[i],
                clips->width[i], clips->masks[i]);
      return VNX_ERR_INVALID_ARGUMENT;
    }
  }
  d->R = rows; d->F = frames; d->h = height; d->w = width;
  d->M = int(M); d->hw = height * width; d->pieces = int(pieces);
  d->stride = stride;
  d->vec = (width & 3) == 0 && (reinterpret_cast<uintptr_t>(logits) & 15) == 0;
  d->alpha = alpha; d->gamma = gamma;
  return VNX_OK;
}

}  // namespace vnx

using namespace vnx;

extern "C" int vnx_mask_loss_forward(const void* logits, const vnx_mask_loss_clips* clips, const void* row_gt, int rows,
                                     int frames, int height, int width, int stride, float alpha, float gamma, void* partial,
                                     size_t partial_bytes, void* focal, void* dice, void* row_sums, void* hip_stream) {
  const char* fn = "vnx_mask_loss_forward";
  MlDims d;
  if (int st = ml_dims(fn, logits, clips, rows, frames, height, width, stride, alpha, gamma, &d)) return st;
  if (rows == 0) return VNX_OK;
  if (!logits || !row_gt || !partial || !focal || !dice || !row_sums) {
    set_error("%s: null pointer argument", fn);
    return VNX_ERR_INVALID_ARGUMENT;
  }
  const size_t need = size_t(rows) * size_t(d.pieces) * 4 * sizeof(float);
  if (partial_bytes < need || (reinterpret_cast<uintptr_t>(partial) & 15) != 0) {
    set_error("%s: partial buffer of %zu bytes, %zu needed (16-byte aligned)", fn, partial_bytes, need);
    return VNX_ERR_WORKSPACE;
  }
  hipStream_t stream = (hipStream_t)hip_stream;
  hipLaunchKernelGGL(mask_loss_fwd_kernel, dim3(uint32_t(rows) * uint32_t(d.pieces)), dim3(kMlThreads), 0, stream,
                     (const float*)logits, *clips, (const int64_t*)row_gt, d, (float*)partial);
  if (int st = check_launch("mask_loss_fwd")) return st;
  hipLaunchKernelGGL(mask_loss_finish_kernel, dim3(uint32_t(rows)), dim3(64), 0, stream, (const float*)partial, d.pieces,
                     d.M, (float*)focal, (float*)dice, (float*)row_sums);
  return check_launch("mask_loss_finish");
}

extern "C" int vnx_mask_loss_backward(const void* logits, const vnx_mask_loss_clips* clips, const void* row_gt, int rows,
                                      int frames, int height, int width, int stride, float alpha, float gamma,
                                      const void* row_sums, const void* grad_focal, const void* grad_dice,
                                      void* grad_logits, void* hip_stream) {
  const char* fn = "vnx_mask_loss_backward";
  MlDims d;
  if (int st = ml_dims(fn, logits, clips, rows, frames, height, width, stride, alpha, gamma, &d)) return st;
  if (rows == 0) return VNX_OK;
  if (!logits || !row_gt || !row_sums || !grad_focal || !grad_dice || !grad_logits) {
    set_error("%s: null pointer argument", fn);
    return VNX_ERR_INVALID_ARGUMENT;
  }
  d.vec = d.vec && (reinterpret_cast<uintptr_t>(grad_logits) & 15) == 0;
  hipLaunchKernelGGL(mask_loss_bwd_kernel, dim3(uint32_t(rows) * uint32_t(d.pieces)), dim3(kMlThreads), 0,
                     (hipStream_t)hip_stream, (const float*)logits, *clips, (const int64_t*)row_gt, d, (const float*)row_sums,
                     (const float*)grad_focal, (const float*)grad_dice, (float*)grad_logits);
  return check_launch("mask_loss_bwd");
}
