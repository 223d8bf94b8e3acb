// window_attn.hip -- the (shifted-)window multi-head self-attention of a Swin Transformer block, all windows, heads and
// images of one block in ONE launch forward and one (+ a small fixed-order reduction) backward.
//
// Reference: SwinTransformerBlock.forward / WindowAttention.forward / BasicLayer.forward (projects/SeqFormer/seqformer/
// backbone/swin.py:129-169, 233-293, 404-452).  Per block ATen runs: F.pad of the normalised tokens to a multiple of the
// window, torch.roll by -shift, the window partition (a permute + a copy), the qkv Linear, reshape / permute, the scale,
// q @ k^T, a gather + permute + copy of the relative-position bias and its add, the add of the [nW, N, N] shift mask,
// softmax, @ v, a transpose, window reverse, the inverse roll and the crop (another copy) -- and it materialises each
// [windows * heads, N, N] score tensor several times, forward and backward.
//
// Here the caller hands over qkv = norm1(x) Wqkv^T on the UNPADDED, UNROLLED tokens, [B * H * W][row_stride] in image-row
// order, WITHOUT the bias (the Linear acts on each token alone, so it commutes with pad / roll / partition).  Everything
// else is index arithmetic in the kernel:
//   * shifted-grid position (i, j) of the padded Hp x Wp grid holds original token ((i + s) mod Hp, (j + s) mod Wp);
//     window (wy, wx) holds the shifted positions [wy w, wy w + w) x [wx w, wx w + w), row-major (the partition order);
//   * a token outside H x W is padding: the reference pads AFTER norm1, so its q / k / v are the qkv bias.  Padded keys
//     take part in the softmax like any other; padded query rows produce nothing;
//   * relative-position bias: table[(ry_i - ry_j + w - 1) (2 w - 1) + (rx_i - rx_j + w - 1)][head];
//   * SW-MSA mask (s > 0): the reference's 3 x 3 region labels of the shifted grid (rows [0, Hp - w), [Hp - w, Hp - s),
//     [Hp - s, Hp), columns the same); -100.0 where the labels of query and key differ.
//
// Inner loop: one thread per window row (N = w^2 <= 144 rows, so a workgroup is one (image, window,
// head) and 1..3 waves), the key / value rows of the window staged in LDS and read as wave-wide broadcasts, fp32 vector FMAs
// and an online softmax.  The guide's v_mfma_f32_16x16x4_f32 runs at the fp32 vector rate (256 FLOP/clk/CU either way), so
// MFMA buys no arithmetic rate here; what the fused form saves is the score tensors and the copies, which it never writes.
//   * forward: out [B * H * W][C] (C = heads * 32) for the real tokens, in image-row order, and lse [B * H * W][heads];
//   * backward, per workgroup: phase 1 one thread per KEY row (recompute p from lse, grad_k, grad_v, dS kept in LDS),
//     phase 2 one thread per QUERY row (grad_q = scale sum_j dS_ij k_j), phase 3 one thread per table entry (the sum of dS
//     over the query rows at that relative offset, fixed order), and the k / v gradients of the padded tokens summed in row
//     order: [(2 w - 1)^2 + 64] partial floats per workgroup, reduced over the workgroups in a fixed order by a second
//     launch.  No atomics anywhere: the table and pad-bias gradients are bit-identical run to run.
//
// dtype VNX_BF16 at the two entry points below goes, after the same argument checks (row stride a multiple of 8 elements
// instead of 4), to the matrix-core kernels of window_attn_mfma.hip, which leave the same partials for the reduction here.
#include "window_attn.h"

namespace vnx {

typedef float wa_f4 __attribute__((ext_vector_type(4)));

constexpr int kWaThreads = 192;              // >= kWaMaxN, a multiple of 64
constexpr int kWaSPad = kWaMaxN + 1;         // floats per dS row in LDS (odd: thread i reading row i hits bank 17 i mod 64)
constexpr int kWaRedSlices = 16;             // workgroup slices of the partial reduction

// (WaArgs and the index helpers wa_token / wa_region / wa_rel: window_attn.h, shared with the bf16 matrix-core kernels)

struct WaRow {
  wa_f4 v[8];
};
__device__ __forceinline__ void wa_zero(WaRow& r) {
#pragma unroll
  for (int i = 0; i < 8; ++i) r.v[i] = wa_f4{0.f, 0.f, 0.f, 0.f};
}
__device__ __forceinline__ WaRow wa_lds(const float* base, int row) {
  WaRow o;
  const wa_f4* p = reinterpret_cast<const wa_f4*>(base + row * kWaHd);
#pragma unroll
  for (int i = 0; i < 8; ++i) o.v[i] = p[i];
  return o;
}
__device__ __forceinline__ void wa_store_lds(float* base, int row, const WaRow& r) {
  wa_f4* p = reinterpret_cast<wa_f4*>(base + row * kWaHd);
#pragma unroll
  for (int i = 0; i < 8; ++i) p[i] = r.v[i];
}
__device__ __forceinline__ float wa_dot(const WaRow& a, const WaRow& b) {
  float x = 0.f, y = 0.f, z = 0.f, u = 0.f;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    x = fmaf(a.v[i].x, b.v[i].x, x); y = fmaf(a.v[i].y, b.v[i].y, y);
    z = fmaf(a.v[i].z, b.v[i].z, z); u = fmaf(a.v[i].w, b.v[i].w, u);
  }
  return (x + y) + (z + u);
}
__device__ __forceinline__ void wa_axpy(WaRow& y, float a, const WaRow& x) {
#pragma unroll
  for (int i = 0; i < 8; ++i) y.v[i] += a * x.v[i];
}

// the 32 channels of head h, section sec (0 q, 1 k, 2 v) of a token (bias added); padding = the bias alone
__device__ __forceinline__ WaRow wa_global_row(const WaArgs& a, int64_t tok, int h, int sec) {
  WaRow o;
  const int C = a.heads * kWaHd;
  const int off = sec * C + h * kWaHd;
  if (tok >= 0) {
    const float* p = a.qkv + tok * a.ld + off;
#pragma unroll
    for (int i = 0; i < 8; ++i) o.v[i] = *reinterpret_cast<const wa_f4*>(p + 4 * i);
  } else {
    wa_zero(o);
  }
  if (a.bias != nullptr) {
#pragma unroll
    for (int i = 0; i < 8; ++i) o.v[i] += *reinterpret_cast<const wa_f4*>(a.bias + off + 4 * i);
  }
  return o;
}
// grid: B * nwin * heads workgroups (head fastest: the workgroups of one window read the same token rows)
__global__ void __launch_bounds__(kWaThreads) window_attn_fwd_kernel(WaArgs a, float* __restrict__ out,
                                                                     float* __restrict__ lse) {
  __shared__ __attribute__((aligned(16))) float s_k[kWaMaxN * kWaHd];
  __shared__ __attribute__((aligned(16))) float s_v[kWaMaxN * kWaHd];
  __shared__ float s_tab[kWaMaxT];
  __shared__ unsigned char s_reg[kWaMaxN];
  const int h = blockIdx.x % a.heads;
  const int bw = blockIdx.x / a.heads;
  const int b = bw / a.nwin, win = bw - b * a.nwin;
  const int N = a.w * a.w, T = (2 * a.w - 1) * (2 * a.w - 1);
  const int r = threadIdx.x;
  const bool live = r < N;
  int64_t tok = -1;
  WaRow q;
  if (live) {
    tok = wa_token(a, b, win, r);
    q = wa_global_row(a, tok, h, 0);
    wa_store_lds(s_k, r, wa_global_row(a, tok, h, 1));
    wa_store_lds(s_v, r, wa_global_row(a, tok, h, 2));
    if (a.s > 0) s_reg[r] = (unsigned char)wa_region(a, win, r);
#pragma unroll
    for (int i = 0; i < 8; ++i) q.v[i] *= a.scale;
  }
  for (int t = threadIdx.x; t < T; t += blockDim.x) s_tab[t] = a.table[t * a.heads + h];
  __syncthreads();
  if (!live || tok < 0) return;                     // padded query rows are computed by nobody: nothing reads them
  const int reg = a.s > 0 ? s_reg[r] : 0;
  float m = -3.0e38f, l = 0.f;
  WaRow acc;
  wa_zero(acc);
  for (int j = 0; j < N; ++j) {
    float sc = wa_dot(q, wa_lds(s_k, j)) + s_tab[wa_rel(r, j, a.w)];
    if (a.s > 0 && s_reg[j] != reg) sc += kWaMask;
    if (sc > m) {
      const float c = __expf(m - sc);
      l *= c;
#pragma unroll
      for (int i = 0; i < 8; ++i) acc.v[i] *= c;
      m = sc;
    }
    const float p = __expf(sc - m);
    l += p;
    wa_axpy(acc, p, wa_lds(s_v, j));
  }
  const float inv = 1.f / l;
  float* o = out + tok * (a.heads * kWaHd) + h * kWaHd;
#pragma unroll
  for (int i = 0; i < 8; ++i) *reinterpret_cast<wa_f4*>(o + 4 * i) = acc.v[i] * inv;
  lse[tok * a.heads + h] = m + __logf(l);
}

// grid: as the forward.  partial: per workgroup [T + 64] floats (table entries of head h, then the k and v gradient of the
// padded tokens of this window, 32 + 32)
__global__ void __launch_bounds__(kWaThreads) window_attn_bwd_kernel(WaArgs a, const float* __restrict__ out,
                                                                     const float* __restrict__ lse,
                                                                     const float* __restrict__ grad_out,
                                                                     float* __restrict__ grad_qkv,
                                                                     float* __restrict__ partial) {
  __shared__ __attribute__((aligned(16))) float s_q[kWaMaxN * kWaHd];      // phase 1: q (biased, unscaled); then grad_k rows
  __shared__ __attribute__((aligned(16))) float s_k[kWaMaxN * kWaHd];
  __shared__ __attribute__((aligned(16))) float s_do[kWaMaxN * kWaHd];     // phase 1: grad_out; then grad_v rows
  __shared__ float s_ds[kWaMaxN * kWaSPad];                                // dS[i][j] (the score gradient)
  __shared__ float s_lse[kWaMaxN], s_d[kWaMaxN];
  __shared__ float s_tab[kWaMaxT];
  __shared__ unsigned char s_reg[kWaMaxN], s_pad[kWaMaxN];
  const int h = blockIdx.x % a.heads;
  const int bw = blockIdx.x / a.heads;
  const int b = bw / a.nwin, win = bw - b * a.nwin;
  const int N = a.w * a.w, T = (2 * a.w - 1) * (2 * a.w - 1);
  const int C = a.heads * kWaHd;
  const int r = threadIdx.x;
  const bool live = r < N;
  int64_t tok = -1;
  WaRow kr, vr;
  if (live) {
    tok = wa_token(a, b, win, r);
    wa_store_lds(s_q, r, wa_global_row(a, tok, h, 0));
    kr = wa_global_row(a, tok, h, 1);
    vr = wa_global_row(a, tok, h, 2);
    wa_store_lds(s_k, r, kr);
    WaRow g;
    if (tok >= 0) {
      const float* gp = grad_out + tok * C + h * kWaHd;
      const float* op = out + tok * C + h * kWaHd;
      WaRow o;
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        g.v[i] = *reinterpret_cast<const wa_f4*>(gp + 4 * i);
        o.v[i] = *reinterpret_cast<const wa_f4*>(op + 4 * i);
      }
      s_d[r] = wa_dot(g, o);
      s_lse[r] = lse[tok * a.heads + h];
    } else {
      wa_zero(g);                                   // a padded query row: p = 0, so it contributes nothing
      s_d[r] = 0.f;
      s_lse[r] = __builtin_inff();
    }
    wa_store_lds(s_do, r, g);
    s_reg[r] = a.s > 0 ? (unsigned char)wa_region(a, win, r) : 0;
    s_pad[r] = tok < 0;
  }
  for (int t = threadIdx.x; t < T; t += blockDim.x) s_tab[t] = a.table[t * a.heads + h];
  __syncthreads();

  // phase 1: thread = key row r
  WaRow gk, gv;
  wa_zero(gk);
  wa_zero(gv);
  if (live) {
    const int reg = s_reg[r];
    for (int i = 0; i < N; ++i) {
      const WaRow qi = wa_lds(s_q, i);
      float sc = a.scale * wa_dot(qi, kr) + s_tab[wa_rel(i, r, a.w)];
      if (a.s > 0 && s_reg[i] != reg) sc += kWaMask;
      const float p = __expf(sc - s_lse[i]);
      const WaRow gi = wa_lds(s_do, i);
      const float ds = p * (wa_dot(gi, vr) - s_d[i]);
      s_ds[i * kWaSPad + r] = ds;
      wa_axpy(gv, p, gi);
      wa_axpy(gk, ds, qi);
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) gk.v[i] *= a.scale;
  }
  __syncthreads();                                  // s_q / s_do are free from here on
  if (live) {
    if (tok >= 0) {
      float* g = grad_qkv + tok * a.ld + h * kWaHd;
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        *reinterpret_cast<wa_f4*>(g + C + 4 * i) = gk.v[i];
        *reinterpret_cast<wa_f4*>(g + 2 * C + 4 * i) = gv.v[i];
      }
    }
    wa_store_lds(s_q, r, gk);
    wa_store_lds(s_do, r, gv);
  }
  __syncthreads();

  float* part = partial + int64_t(blockIdx.x) * (T + 64);
  // phase 2: thread = query row r
  if (live && tok >= 0) {
    WaRow gq;
    wa_zero(gq);
    const float* dsr = s_ds + r * kWaSPad;
    for (int j = 0; j < N; ++j) wa_axpy(gq, dsr[j], wa_lds(s_k, j));
    float* g = grad_qkv + tok * a.ld + h * kWaHd;
#pragma unroll
    for (int i = 0; i < 8; ++i) *reinterpret_cast<wa_f4*>(g + 4 * i) = gq.v[i] * a.scale;
  }
  // phase 3: thread = table entry t: the sum over the query rows of dS at relative offset t, in row order
  for (int t = threadIdx.x; t < T; t += blockDim.x) {
    const int dy = t / (2 * a.w - 1) - (a.w - 1), dx = t % (2 * a.w - 1) - (a.w - 1);
    float acc = 0.f;
    for (int yi = max(0, dy); yi < min(a.w, a.w + dy); ++yi)
      for (int xi = max(0, dx); xi < min(a.w, a.w + dx); ++xi) {
        const int i = yi * a.w + xi, j = (yi - dy) * a.w + (xi - dx);
        acc += s_ds[i * kWaSPad + j];
      }
    part[t] = acc;
  }
  // the k (channels 0..31) and v (32..63) gradients of the padded key rows, summed in row order
  if (threadIdx.x < 64) {
    const float* src = threadIdx.x < 32 ? s_q : s_do;
    const int c = threadIdx.x & 31;
    float acc = 0.f;
    for (int j = 0; j < N; ++j)
      if (s_pad[j]) acc += src[j * kWaHd + c];
    part[T + threadIdx.x] = acc;
  }
}

// grid: (ceil((T + 64) / 64), heads), kWaRedSlices * 64 threads: entry e of head h summed over the groups (image, window) --
// slice k takes groups k, k + 16, ... in order, then the 16 slice sums are added in slice order
__global__ void __launch_bounds__(kWaRedSlices * 64) window_attn_reduce_kernel(const float* __restrict__ partial, int groups,
                                                                               int heads, int T, int C,
                                                                               float* __restrict__ grad_table,
                                                                               float* __restrict__ grad_pad) {
  __shared__ float s_sum[kWaRedSlices][64];
  const int lane = threadIdx.x & 63, slice = threadIdx.x >> 6;
  const int e = blockIdx.x * 64 + lane, h = blockIdx.y;
  const int E = T + 64;
  float acc = 0.f;
  if (e < E) {
    const float* p = partial + int64_t(h) * E + e;
    const int64_t step = int64_t(heads) * E;
    for (int g = slice; g < groups; g += kWaRedSlices) acc += p[int64_t(g) * step];
  }
  s_sum[slice][lane] = acc;
  __syncthreads();
  if (slice != 0 || e >= E) return;
  float t = 0.f;
#pragma unroll
  for (int k = 0; k < kWaRedSlices; ++k) t += s_sum[k][lane];
  if (e < T) {
    grad_table[int64_t(e) * heads + h] = t;
  } else if (grad_pad != nullptr) {
    const int c = e - T;                            // 0..31: k channel, 32..63: v channel
    grad_pad[(c < 32 ? C : 2 * C) + h * kWaHd + (c & 31)] = t;
    if (c < 32) grad_pad[h * kWaHd + c] = 0.f;      // the q third: padded query rows are dropped
  }
}

static int wa_check(const char* fn, int dtype, int batch, int height, int width, int heads, int head_dim, int ld, int w,
                    int s) {
  if (dtype != VNX_F32 && dtype != VNX_BF16) {
    set_error("%s: fp32 or bf16 only (dtype %d)", fn, dtype);
    return VNX_ERR_UNSUPPORTED;
  }
  if (head_dim != kWaHd) {
    set_error("%s: built for heads of %d channels (head_dim %d)", fn, kWaHd, head_dim);
    return VNX_ERR_UNSUPPORTED;
  }
  if (w < 1 || w > kWaMaxWin || heads < 1 || heads > 48) {
    set_error("%s: window %d / heads %d outside 1..%d / 1..48", fn, w, heads, kWaMaxWin);
    return VNX_ERR_UNSUPPORTED;
  }
  if (batch < 0 || height < 1 || width < 1 || s < 0 || s >= w || ld < 3 * heads * kWaHd ||
      (ld & (dtype == VNX_BF16 ? 7 : 3)) != 0) {                 // rows 16-byte aligned: 4 fp32 or 8 bf16 elements
    set_error("%s: bad sizes (batch %d, %d x %d, shift %d, row stride %d)", fn, batch, height, width, s, ld);
    return VNX_ERR_INVALID_ARGUMENT;
  }
  const int64_t nwin = int64_t((height + w - 1) / w) * ((width + w - 1) / w);
  if (int64_t(batch) * nwin * heads >= (int64_t(1) << 31)) {
    set_error("%s: too many workgroups", fn);
    return VNX_ERR_UNSUPPORTED;
  }
  return VNX_OK;
}

static WaArgs wa_args(const void* qkv, const void* bias, const void* table, int batch, int height, int width, int heads,
                      int ld, int w, int s, float scale) {
  WaArgs a;
  a.qkv = (const float*)qkv;
  a.bias = (const float*)bias;
  a.table = (const float*)table;
  a.B = batch; a.H = height; a.W = width; a.heads = heads; a.ld = ld; a.w = w; a.s = s;
  a.Hp = (height + w - 1) / w * w;
  a.Wp = (width + w - 1) / w * w;
  a.nwx = a.Wp / w;
  a.nwin = (a.Hp / w) * a.nwx;
  a.scale = scale;
  return a;
}

static bool wa_aligned(const void* p) { return p == nullptr || (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace vnx

using namespace vnx;

extern "C" size_t vnx_window_attention_partial_bytes(int batch, int height, int width, int heads, int window) {
  if (batch < 0 || height < 1 || width < 1 || heads < 1 || window < 1 || window > kWaMaxWin) return 0;
  const int64_t nwin = int64_t((height + window - 1) / window) * ((width + window - 1) / window);
  const int64_t T = int64_t(2 * window - 1) * (2 * window - 1);
  return size_t(int64_t(batch) * nwin * heads * (T + 64) * int64_t(sizeof(float)));
}

extern "C" int vnx_window_attention_forward(int dtype, const void* qkv, const void* qkv_bias, const void* bias_table,
                                            void* out, void* lse, int batch, int height, int width, int heads, int head_dim,
                                            int row_stride, int window, int shift, float scale, void* hip_stream) {
  const char* fn = "vnx_window_attention_forward";
  if (int st = wa_check(fn, dtype, batch, height, width, heads, head_dim, row_stride, window, shift)) return st;
  if (batch == 0) return VNX_OK;
  if (!qkv || !bias_table || !out || !lse) {
    set_error("%s: null pointer argument", fn);
    return VNX_ERR_INVALID_ARGUMENT;
  }
  if (!wa_aligned(qkv) || !wa_aligned(qkv_bias) || !wa_aligned(out)) {
    set_error("%s: qkv, qkv_bias and out must be 16-byte aligned", fn);
    return VNX_ERR_INVALID_ARGUMENT;
  }
  const WaArgs a = wa_args(qkv, qkv_bias, bias_table, batch, height, width, heads, row_stride, window, shift, scale);
  if (dtype == VNX_BF16) return window_attention_mfma_forward(a, out, lse, (hipStream_t)hip_stream);
  const int threads = (window * window + 63) / 64 * 64;
  hipLaunchKernelGGL(window_attn_fwd_kernel, dim3(uint32_t(int64_t(batch) * a.nwin * heads)), dim3(threads), 0,
                     (hipStream_t)hip_stream, a, (float*)out, (float*)lse);
  return check_launch("window_attn_fwd");
}

extern "C" int vnx_window_attention_backward(int dtype, const void* qkv, const void* qkv_bias, const void* bias_table,
                                             const void* out, const void* lse, const void* grad_out, void* grad_qkv,
                                             void* grad_bias_table, void* grad_pad_bias, void* partial, size_t partial_bytes,
                                             int batch, int height, int width, int heads, int head_dim, int row_stride,
                                             int window, int shift, float scale, void* hip_stream) {
  const char* fn = "vnx_window_attention_backward";
  if (int st = wa_check(fn, dtype, batch, height, width, heads, head_dim, row_stride, window, shift)) return st;
  if (batch == 0) return VNX_OK;
  if (!qkv || !bias_table || !out || !lse || !grad_out || !grad_qkv || !grad_bias_table) {
    set_error("%s: null pointer argument", fn);
    return VNX_ERR_INVALID_ARGUMENT;
  }
  if (!wa_aligned(qkv) || !wa_aligned(qkv_bias) || !wa_aligned(out) || !wa_aligned(grad_out) || !wa_aligned(grad_qkv)) {
    set_error("%s: qkv, qkv_bias, out, grad_out and grad_qkv must be 16-byte aligned", fn);
    return VNX_ERR_INVALID_ARGUMENT;
  }
  const size_t need = vnx_window_attention_partial_bytes(batch, height, width, heads, window);
  if (partial == nullptr || partial_bytes < need) {
    set_error("%s: partial buffer of %zu bytes, %zu needed", fn, partial_bytes, need);
    return VNX_ERR_WORKSPACE;
  }
  const WaArgs a = wa_args(qkv, qkv_bias, bias_table, batch, height, width, heads, row_stride, window, shift, scale);
  const int threads = (window * window + 63) / 64 * 64;
  const int groups = batch * a.nwin;
  if (dtype == VNX_BF16) {                            // the matrix-core kernel leaves the same partials
    if (int st = window_attention_mfma_backward(a, out, lse, grad_out, grad_qkv, partial, (hipStream_t)hip_stream)) return st;
  } else {
    hipLaunchKernelGGL(window_attn_bwd_kernel, dim3(uint32_t(int64_t(groups) * heads)), dim3(threads), 0,
                       (hipStream_t)hip_stream, a, (const float*)out, (const float*)lse, (const float*)grad_out,
                       (float*)grad_qkv, (float*)partial);
    if (int st = check_launch("window_attn_bwd")) return st;
  }
  const int T = (2 * window - 1) * (2 * window - 1);
  hipLaunchKernelGGL(window_attn_reduce_kernel, dim3(uint32_t((T + 64 + 63) / 64), uint32_t(heads)),
                     dim3(kWaRedSlices * 64), 0, (hipStream_t)hip_stream, (const float*)partial, groups, heads, T,
                     heads * kWaHd, (float*)grad_bias_table, (float*)grad_pad_bias);
  return check_launch("window_attn_reduce");
}
