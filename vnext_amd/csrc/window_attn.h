// window_attn.h -- what the two instantiations of the Swin window attention share: the fp32 vector kernels of
// window_attn.hip and the bf16 matrix-core kernels of window_attn_mfma.hip.  The index arithmetic below (pad, cyclic shift,
// window partition, SW-MSA regions, relative-position offsets) is the specification of both.
#pragma once
#include "vnx_common.h"

namespace vnx {

constexpr int kWaHd = 32;                    // channels per head
constexpr int kWaMaxWin = 12;                // window sizes 1..12
constexpr int kWaMaxN = kWaMaxWin * kWaMaxWin;
constexpr int kWaMaxT = (2 * kWaMaxWin - 1) * (2 * kWaMaxWin - 1);
constexpr float kWaMask = -100.0f;

struct WaArgs {
  const float* qkv;      // [B * H * W][ld], q | k | v, no bias (bf16 instantiation: the same pointer, 16-bit elements)
  const float* bias;     // [3 C] or null
  const float* table;    // [(2 w - 1)^2][heads]
  int B, H, W, heads, ld, w, s, Hp, Wp, nwx, nwin;     // nwin = windows per image
  float scale;
};

// where window row `r` of window `win` (of image b) comes from: its token index in [B * H * W], or -1 for padding
__device__ __forceinline__ int64_t wa_token(const WaArgs& a, int b, int win, int r) {
  const int wy = win / a.nwx, wx = win - wy * a.nwx;
  const int ry = r / a.w, rx = r - ry * a.w;
  int pi = wy * a.w + ry + a.s, pj = wx * a.w + rx + a.s;
  if (pi >= a.Hp) pi -= a.Hp;
  if (pj >= a.Wp) pj -= a.Wp;
  if (pi >= a.H || pj >= a.W) return -1;
  return (int64_t(b) * a.H + pi) * a.W + pj;
}
// region label (0..8) of the shifted-grid position of window row `r` (only read when s > 0)
__device__ __forceinline__ int wa_region(const WaArgs& a, int win, int r) {
  const int wy = win / a.nwx, wx = win - wy * a.nwx;
  const int ry = r / a.w, rx = r - ry * a.w;
  const int i = wy * a.w + ry, j = wx * a.w + rx;
  const int li = i < a.Hp - a.w ? 0 : (i < a.Hp - a.s ? 1 : 2);
  const int lj = j < a.Wp - a.w ? 0 : (j < a.Wp - a.s ? 1 : 2);
  return li * 3 + lj;
}
// relative-position table index of (query row ri, key row rj)
__device__ __forceinline__ int wa_rel(int ri, int rj, int w) {
  const int yi = ri / w, xi = ri - yi * w, yj = rj / w, xj = rj - yj * w;
  return (yi - yj + w - 1) * (2 * w - 1) + (xi - xj + w - 1);
}

// window_attn_mfma.hip: the bf16 launches behind dtype == VNX_BF16 (arguments already checked by the entry points of
// window_attn.hip; `partial` as the fp32 backward lays it out, reduced by the same window_attn_reduce_kernel)
int window_attention_mfma_forward(const WaArgs& a, void* out, void* lse, hipStream_t stream);
int window_attention_mfma_backward(const WaArgs& a, const void* out, const void* lse, const void* grad_out, void* grad_qkv,
                                   void* partial, hipStream_t stream);

}  // namespace vnx
