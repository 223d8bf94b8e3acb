// window_attn_mfma.hip -- the bf16 instantiation of the Swin window attention (window_attn.hip has the function, the
// indexing and the fp32 vector kernels): bf16 qkv / out / grad_out / grad_qkv, every matrix product on the gfx950 matrix
// cores (v_mfma_f32_32x32x16_bf16), everything between the products in fp32.  Reached through the same two entry points
// with dtype == VNX_BF16.
//
// One workgroup per (image, window, head) as in the fp32 kernels, NT = ceil(N / 32) waves (N = w^2 window rows, padded to
// Np = 32 NT TILE rows: 49 -> 64, 144 -> 160).  Tile-padding rows are not image padding: they hold zeros, their
// probabilities are exactly 0 and nothing of them is stored; image-padded tokens are real keys / values equal to the bias.
//
// bf16 rounding happens at the MFMA operands -- q, k, v = bf16_rne(float(qkv) + bias), p for P V, dS for dQ; grad_out as
// it arrives -- and at the final stores of out and grad_qkv.  For dV = P^T dO and dK = dS^T Q the operand is p / dS as TWO
// bf16 terms, the rounded value and bf16(x - rounded) (two MFMAs): those products sum over the queries, padded query rows
// are dropped, and on a grid of one real token the single rounding of p_r / dS_rr moved the whole grad_k row by 3e-3 --
// with every rounding point single, a float64 evaluation of this arithmetic gives 9.57e-3 on grad_qkv there (5.4e-3 from the
// q / k / v rounding alone), the kernel the same number digit for digit, against a test bound of 2^-7.  The score (scale applied to the fp32
// accumulator, not to q), the table and mask adds, max / sum / lse, D, dS = p (dP - D), every accumulator and the table /
// pad-bias partials are fp32; the row sum l is taken from the fp32 p.
// D = rowsum(dO o O) is evaluated as rowsum(p o dP) from the kernel's own fp32 p and dP -- the same number for an unrounded
// O.  Taken from the bf16 `out` it carries dO . (O_bf16 - O), which every dS of the row inherits with the same sign: on a
// grid of one real token beside 48 / 143 padded keys that was 6e-2 / 9e-2 of the largest grad_qkv element (measured), against
// 1e-2 / 3e-3 for ATen.  With the kernel's own sum, sum_j dS_ij = D (1 - sum_j p_ij) = 0 to fp32 rounding.
//
// Forward, wave = one tile of 32 QUERIES: S^T = K Q^T (A = K rows from LDS, B = Q rows straight from global), so a lane
// holds one query column and 16 keys per tile in its accumulator registers, NT tiles = all keys of the window (<= 80
// registers).  Two-pass softmax in registers (max, then exp and sum; one exchange between the two lane halves each), no
// online rescaling.  P^T, rounded in place, is the B operand of O^T = V^T P^T (an accumulator tile as the next MFMA's
// operand: element j of lane half h of k-step s is tile row 16 s + 8 (j >> 2) + 4 h + (j & 3)); V^T comes from a transposed
// LDS image [channel][key] read in that same permuted k order (two 8-byte reads).
//
// Backward, phase A, wave = one tile of 32 KEYS (K and V rows in registers as B operands).  Pass 1 over the query tiles:
// S = Q K^T and dP = dO V^T (A = Q / dO rows from LDS), p = exp(scale S + bias + mask - lse), both kept in the accumulator
// registers (query on the register index, key on the lane; 2 x 16 NT registers), and the sums of p o dP over the wave's
// keys (a halving butterfly over the 32 key lanes), which meet in LDS in wave order: D.  Pass 2: dS = p (dP - D) in place,
// then dV^T += dO^T P and dK^T += Q^T dS with P / dS as B operands in place and dO^T / Q^T from transposed LDS images; dS
// also goes to LDS in BF16, [query][key] (the value the MFMAs consumed).  Phase B, wave = one tile of queries: dQ^T = K^T dS^T from the transposed K image and the dS rows.
// Phase C: the per-workgroup relative-offset sums of dS (fp32 accumulation over the bf16 dS in LDS, fixed order) and the
// k / v gradients of the image-padded keys (a fixed butterfly inside each wave, then the waves in order):
// [T + 64] fp32 partials per workgroup, reduced by window_attn_reduce_kernel unchanged.  No atomics: bit-identical run to run.
//
// Resources (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage; no scratch in any instantiation;
// VGPRs / AGPRs / LDS bytes per workgroup):
//   NT              1 (w <= 5)     2 (w 6, 7, 8)   3 (w 9)         4 (w 10, 11)    5 (w 12)
//   forward    37 / 16 / 7376   57 / 16 / 12112   68 / 48 / 16848   88 / 64 / 21584   114 / 0 / 26320
//   backward   83 / 32 / 18256  120 / 32 / 37200  152 / 32 / 60496  184 / 32 / 88144  236 / 0 / 120144
// The backward at w = 12 is ONE workgroup of 5 waves per CU (dS alone is 160 x 168 bf16 = 53.8 KB, the five operand images
// 57.9 KB); at w = 7 four workgroups fit.  Under 80 KB at w = 12 needs dS tiled by query block -- not built.
#include "window_attn.h"

namespace vnx {

typedef __bf16 wm_bf8 __attribute__((ext_vector_type(8)));
typedef float wm_f16 __attribute__((ext_vector_type(16)));
typedef uint32_t wm_u4 __attribute__((ext_vector_type(4)));
typedef uint32_t wm_u2 __attribute__((ext_vector_type(2)));
typedef float wm_f2 __attribute__((ext_vector_type(2)));

constexpr int kWmLd = 40;                    // bf16 per row of a row-major [row][32 channel] LDS image (80 B: 16-B aligned, rows 20 banks apart)
constexpr int kWmTilePad = -2;               // "token" of a tile-padding row (wa_token gives -1 for image padding)

__device__ __forceinline__ wm_f16 wm_mfma(wm_u4 a, wm_u4 b, wm_f16 c) {
  return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(wm_bf8, a), __builtin_bit_cast(wm_bf8, b), c, 0, 0, 0);
}
__device__ __forceinline__ float wm_lo(uint32_t x) { return __uint_as_float(x << 16); }
__device__ __forceinline__ float wm_hi(uint32_t x) { return __uint_as_float(x & 0xffff0000u); }
__device__ __forceinline__ wm_u4 wm_ld16(const void* p) { return *reinterpret_cast<const wm_u4*>(p); }

// 8 consecutive channels (from column `col`, a multiple of 8) of a token's qkv row as bf16_rne(float(qkv) + bias); an
// image-padded token (tok == -1) is the bias alone, a tile-padding row (kWmTilePad) zero
__device__ __forceinline__ wm_u4 wm_qkv8(const WaArgs& a, int64_t tok, int col) {
  if (tok == kWmTilePad) return wm_u4{0u, 0u, 0u, 0u};
  wm_u4 raw{0u, 0u, 0u, 0u};
  if (tok >= 0) raw = wm_ld16(reinterpret_cast<const uint16_t*>(a.qkv) + tok * a.ld + col);
  if (a.bias == nullptr) return raw;
  const vnx_f4 b0 = *reinterpret_cast<const vnx_f4*>(a.bias + col), b1 = *reinterpret_cast<const vnx_f4*>(a.bias + col + 4);
  return wm_u4{f32x2_to_bf16x2(wm_lo(raw.x) + b0.x, wm_hi(raw.x) + b0.y), f32x2_to_bf16x2(wm_lo(raw.y) + b0.z, wm_hi(raw.y) + b0.w),
               f32x2_to_bf16x2(wm_lo(raw.z) + b1.x, wm_hi(raw.z) + b1.y), f32x2_to_bf16x2(wm_lo(raw.w) + b1.z, wm_hi(raw.w) + b1.w)};
}
// the 8 channels of `v` to column `row` of a transposed image [channel][ld], channels c0 .. c0 + 7
__device__ __forceinline__ void wm_store_t(uint16_t* img, int ld, int c0, int row, wm_u4 v) {
  const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    img[(c0 + 2 * i) * ld + row] = uint16_t(w[i]);
    img[(c0 + 2 * i + 1) * ld + row] = uint16_t(w[i] >> 16);
  }
}
// accumulator registers 8 s .. 8 s + 7 as the bf16 fragment of k-step s
__device__ __forceinline__ wm_u4 wm_pack(const wm_f16& x, int s) {
  return wm_u4{f32x2_to_bf16x2(x[8 * s], x[8 * s + 1]), f32x2_to_bf16x2(x[8 * s + 2], x[8 * s + 3]),
               f32x2_to_bf16x2(x[8 * s + 4], x[8 * s + 5]), f32x2_to_bf16x2(x[8 * s + 6], x[8 * s + 7])};
}
// ... and what that rounding left behind, x - float(hi), as a second bf16 fragment (hi: the words of wm_pack(x, s))
__device__ __forceinline__ wm_u4 wm_pack_rest(const wm_f16& x, int s, wm_u4 hi) {
  return wm_u4{f32x2_to_bf16x2(x[8 * s] - wm_lo(hi.x), x[8 * s + 1] - wm_hi(hi.x)),
               f32x2_to_bf16x2(x[8 * s + 2] - wm_lo(hi.y), x[8 * s + 3] - wm_hi(hi.y)),
               f32x2_to_bf16x2(x[8 * s + 4] - wm_lo(hi.z), x[8 * s + 5] - wm_hi(hi.z)),
               f32x2_to_bf16x2(x[8 * s + 6] - wm_lo(hi.w), x[8 * s + 7] - wm_hi(hi.w))};
}
// the other operand of such a product: row `r` of a transposed image, the 8 columns in the accumulator's k order
// (base + 4 h + 0..3 and base + 8 + 4 h + 0..3; base = 32 tile + 16 s)
__device__ __forceinline__ wm_u4 wm_ld_perm(const uint16_t* img, int ld, int r, int base, int hh) {
  const wm_u2 lo = *reinterpret_cast<const wm_u2*>(img + r * ld + base + 4 * hh);
  const wm_u2 hi = *reinterpret_cast<const wm_u2*>(img + r * ld + base + 8 + 4 * hh);
  return wm_u4{lo.x, lo.y, hi.x, hi.y};
}
// tile row of accumulator register g in lane half hh
__device__ __forceinline__ int wm_row(int g, int hh) { return (g & 3) + 8 * (g >> 2) + 4 * hh; }

// sum of each of the 16 accumulator registers over the 32 lanes of a lane half, by a halving butterfly (a fixed tree: 16
// exchanges instead of 80): the lane keeps one half of its values and hands the other to its partner at every step.
// Returns the sum of register (lane & 31) >> 1 -- both lanes of a pair hold it.
__device__ __forceinline__ float wm_rowsum(const wm_f16& y, int r) {
  const bool b16 = r & 16, b8 = r & 8, b4 = r & 4, b2 = r & 2;
  float a8[8], a4[4], a2[2];
#pragma unroll
  for (int k = 0; k < 8; ++k) a8[k] = (b16 ? y[8 + k] : y[k]) + __shfl_xor(b16 ? y[k] : y[8 + k], 16);
#pragma unroll
  for (int k = 0; k < 4; ++k) a4[k] = (b8 ? a8[4 + k] : a8[k]) + __shfl_xor(b8 ? a8[k] : a8[4 + k], 8);
#pragma unroll
  for (int k = 0; k < 2; ++k) a2[k] = (b4 ? a4[2 + k] : a4[k]) + __shfl_xor(b4 ? a4[k] : a4[2 + k], 4);
  float u = (b2 ? a2[1] : a2[0]) + __shfl_xor(b2 ? a2[0] : a2[1], 2);
  u += __shfl_xor(u, 1);
  return u;
}

// per window row: y (2 w - 1) + x (the relative-position index of (i, j) is info_i - info_j + 2 w (w - 1)) in bits 0..9,
// the shift region in bits 10..13; tile-padding rows: 0 (any in-range table index; their p is forced to 0)
__device__ __forceinline__ int wm_info(const WaArgs& a, int win, int row, int N) {
  if (row >= N) return 0;
  const int ry = row / a.w, rx = row - ry * a.w;
  return (ry * (2 * a.w - 1) + rx) | ((a.s > 0 ? wa_region(a, win, row) : 0) << 10);
}

// grid: B * nwin * heads workgroups (head fastest), 64 NT threads
template <int NT>
__global__ void __launch_bounds__(64 * NT) window_attn_mfma_fwd_kernel(WaArgs a, uint16_t* __restrict__ out,
                                                                        float* __restrict__ lse) {
  constexpr int Np = 32 * NT, kLdT = Np + 8;
  __shared__ __attribute__((aligned(16))) uint16_t s_k[Np * kWmLd];          // K rows
  __shared__ __attribute__((aligned(16))) uint16_t s_vt[kWaHd * kLdT];       // V^T: [channel][key]
  __shared__ float s_tab[kWaMaxT];
  __shared__ int s_info[Np];
  const int h = blockIdx.x % a.heads;
  const int bw = blockIdx.x / a.heads;
  const int b = bw / a.nwin, win = bw - b * a.nwin;
  const int N = a.w * a.w, T = (2 * a.w - 1) * (2 * a.w - 1);
  const int C = a.heads * kWaHd;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, hh = lane >> 5;
  {                                                   // two threads per window row, 16 channels each
    const int row = tid >> 1, c0 = (tid & 1) * 16;
    const int64_t tok = row < N ? wa_token(a, b, win, row) : kWmTilePad;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      *reinterpret_cast<wm_u4*>(s_k + row * kWmLd + c0 + 8 * i) = wm_qkv8(a, tok, C + h * kWaHd + c0 + 8 * i);
      wm_store_t(s_vt, kLdT, c0 + 8 * i, row, wm_qkv8(a, tok, 2 * C + h * kWaHd + c0 + 8 * i));
    }
    if ((tid & 1) == 0) s_info[row] = wm_info(a, win, row, N);
  }
  for (int t = tid; t < T; t += 64 * NT) s_tab[t] = a.table[t * a.heads + h];
  const int query = wave * 32 + r;
  const int64_t qtok = query < N ? wa_token(a, b, win, query) : kWmTilePad;
  wm_u4 qf[2];
#pragma unroll
  for (int s = 0; s < 2; ++s) qf[s] = wm_qkv8(a, qtok, h * kWaHd + 16 * s + 8 * hh);
  __syncthreads();

  // S^T tiles: acc[kt][g] = S[query][key 32 kt + wm_row(g, hh)]
  wm_f16 acc[NT];
#pragma unroll
  for (int kt = 0; kt < NT; ++kt) {
#pragma unroll
    for (int g = 0; g < 16; ++g) acc[kt][g] = 0.f;
#pragma unroll
    for (int s = 0; s < 2; ++s)
      acc[kt] = wm_mfma(wm_ld16(s_k + (kt * 32 + r) * kWmLd + 16 * s + 8 * hh), qf[s], acc[kt]);
  }
  const int qinfo = s_info[query];
  const int qoff = (qinfo & 1023) + 2 * a.w * (a.w - 1), qreg = qinfo >> 10;
  float m = -3.0e38f;
#pragma unroll
  for (int kt = 0; kt < NT; ++kt) {
#pragma unroll
    for (int g = 0; g < 16; ++g) {
      const int key = kt * 32 + wm_row(g, hh);
      const int ki = s_info[key];
      float sc = a.scale * acc[kt][g] + s_tab[qoff - (ki & 1023)];
      if ((ki >> 10) != qreg) sc += kWaMask;
      sc = key < N ? sc : -__builtin_inff();          // tile padding: p = exp(-inf) = 0 exactly
      acc[kt][g] = sc;
      m = fmaxf(m, sc);
    }
  }
  m = fmaxf(m, __shfl_xor(m, 32));
  float l = 0.f;
#pragma unroll
  for (int kt = 0; kt < NT; ++kt) {
#pragma unroll
    for (int g = 0; g < 16; ++g) {
      const float p = __expf(acc[kt][g] - m);
      acc[kt][g] = p;
      l += p;
    }
  }
  l += __shfl_xor(l, 32);
  // O^T = V^T P^T: o[g] = O[query][channel wm_row(g, hh)]
  wm_f16 o;
#pragma unroll
  for (int g = 0; g < 16; ++g) o[g] = 0.f;
#pragma unroll
  for (int kt = 0; kt < NT; ++kt) {
#pragma unroll
    for (int s = 0; s < 2; ++s) o = wm_mfma(wm_ld_perm(s_vt, kLdT, r, kt * 32 + 16 * s, hh), wm_pack(acc[kt], s), o);
  }
  if (qtok < 0) return;                               // padded query rows are computed for nothing: nobody reads them
  const float inv = 1.f / l;
  uint16_t* op = out + qtok * C + h * kWaHd + 4 * hh;
#pragma unroll
  for (int q4 = 0; q4 < 4; ++q4)
    *reinterpret_cast<wm_u2*>(op + 8 * q4) = wm_u2{f32x2_to_bf16x2(o[4 * q4] * inv, o[4 * q4 + 1] * inv),
                                                   f32x2_to_bf16x2(o[4 * q4 + 2] * inv, o[4 * q4 + 3] * inv)};
  if (hh == 0) lse[qtok * a.heads + h] = m + __logf(l);
}

// grid and block: as the forward.  partial: per workgroup [T + 64] floats, as window_attn_bwd_kernel leaves them
template <int NT>
__global__ void __launch_bounds__(64 * NT) window_attn_mfma_bwd_kernel(WaArgs a, const float* __restrict__ lse,
                                                                        const uint16_t* __restrict__ grad_out,
                                                                        uint16_t* __restrict__ grad_qkv,
                                                                        float* __restrict__ partial) {
  constexpr int Np = 32 * NT, kLdT = Np + 8;
  __shared__ __attribute__((aligned(16))) uint16_t s_q[Np * kWmLd];          // Q rows, dO rows
  __shared__ __attribute__((aligned(16))) uint16_t s_do[Np * kWmLd];
  __shared__ __attribute__((aligned(16))) uint16_t s_qt[kWaHd * kLdT];       // Q^T, dO^T, K^T: [channel][row]
  __shared__ __attribute__((aligned(16))) uint16_t s_dot[kWaHd * kLdT];
  __shared__ __attribute__((aligned(16))) uint16_t s_kt[kWaHd * kLdT];
  __shared__ __attribute__((aligned(16))) uint16_t s_ds[Np * kLdT];          // dS [query][key], bf16
  __shared__ __attribute__((aligned(8))) wm_f2 s_row[Np];                    // per query row: lse, info (bits)
  __shared__ float s_dpart[NT][Np], s_d[Np];                                 // D = rowsum(p o dP): per key tile, then whole
  __shared__ float s_tab[kWaMaxT];
  __shared__ float s_pp[NT][64];                                             // per wave: k | v gradient of its padded keys
  const int h = blockIdx.x % a.heads;
  const int bw = blockIdx.x / a.heads;
  const int b = bw / a.nwin, win = bw - b * a.nwin;
  const int N = a.w * a.w, T = (2 * a.w - 1) * (2 * a.w - 1);
  const int C = a.heads * kWaHd;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, hh = lane >> 5;
  {                                                   // two threads per window row, 16 channels each
    const int row = tid >> 1, c0 = (tid & 1) * 16;
    const int64_t tok = row < N ? wa_token(a, b, win, row) : kWmTilePad;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const wm_u4 q = wm_qkv8(a, tok, h * kWaHd + c0 + 8 * i);
      *reinterpret_cast<wm_u4*>(s_q + row * kWmLd + c0 + 8 * i) = q;
      wm_store_t(s_qt, kLdT, c0 + 8 * i, row, q);
      wm_u4 g{0u, 0u, 0u, 0u};                        // a padded query row: no gradient arrives, p = 0
      if (tok >= 0) g = wm_ld16(grad_out + tok * C + h * kWaHd + c0 + 8 * i);
      *reinterpret_cast<wm_u4*>(s_do + row * kWmLd + c0 + 8 * i) = g;
      wm_store_t(s_dot, kLdT, c0 + 8 * i, row, g);
    }
    if ((tid & 1) == 0)
      s_row[row] = wm_f2{tok >= 0 ? lse[tok * a.heads + h] : __builtin_inff(), __int_as_float(wm_info(a, win, row, N))};
  }
  for (int t = tid; t < T; t += 64 * NT) s_tab[t] = a.table[t * a.heads + h];
  // this wave's key tile: K and V rows as B operands, and K^T for phase B
  const int key = wave * 32 + r;
  const int64_t ktok = key < N ? wa_token(a, b, win, key) : kWmTilePad;
  wm_u4 kf[2], vf[2];
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    kf[s] = wm_qkv8(a, ktok, C + h * kWaHd + 16 * s + 8 * hh);
    vf[s] = wm_qkv8(a, ktok, 2 * C + h * kWaHd + 16 * s + 8 * hh);
    wm_store_t(s_kt, kLdT, 16 * s + 8 * hh, key, kf[s]);
  }
  const int kinfo = wm_info(a, win, key, N);
  const int koff = 2 * a.w * (a.w - 1) - (kinfo & 1023), kreg = kinfo >> 10;
  const bool klive = key < N;
  __syncthreads();

  // phase A, pass 1: p and dP of every query tile against this wave's keys, kept in registers:
  // sa[qt][g] / pa[qt][g] = p / dP of [query 32 qt + wm_row(g, hh)][key]; the row sums of p o dP over these keys
  wm_f16 sa[NT], pa[NT];
#pragma unroll
  for (int qt = 0; qt < NT; ++qt) {
#pragma unroll
    for (int g = 0; g < 16; ++g) sa[qt][g] = pa[qt][g] = 0.f;
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      sa[qt] = wm_mfma(wm_ld16(s_q + (qt * 32 + r) * kWmLd + 16 * s + 8 * hh), kf[s], sa[qt]);
      pa[qt] = wm_mfma(wm_ld16(s_do + (qt * 32 + r) * kWmLd + 16 * s + 8 * hh), vf[s], pa[qt]);
    }
    wm_f16 y;
#pragma unroll
    for (int g = 0; g < 16; ++g) {
      const wm_f2 ri = s_row[qt * 32 + wm_row(g, hh)];
      const int qi = __float_as_int(ri.y);
      float sc = a.scale * sa[qt][g] + s_tab[(qi & 1023) + koff];
      if ((qi >> 10) != kreg) sc += kWaMask;
      const float p = klive ? __expf(sc - ri.x) : 0.f;      // lse = +inf on padded query rows: p = 0
      sa[qt][g] = p;
      y[g] = p * pa[qt][g];
    }
    const float u = wm_rowsum(y, r);
    if ((r & 1) == 0) s_dpart[wave][qt * 32 + wm_row(r >> 1, hh)] = u;
  }
  __syncthreads();
  if (tid < Np) {                                     // the key tiles in order
    float d = 0.f;
#pragma unroll
    for (int wv = 0; wv < NT; ++wv) d += s_dpart[wv][tid];
    s_d[tid] = d;
  }
  __syncthreads();
  // pass 2: dS = p (dP - D) in place, to LDS in bf16, and the two products that sum over the queries
  wm_f16 dk, dv;
#pragma unroll
  for (int g = 0; g < 16; ++g) dk[g] = dv[g] = 0.f;
#pragma unroll
  for (int qt = 0; qt < NT; ++qt) {
#pragma unroll
    for (int g = 0; g < 16; ++g) {
      const int qrow = qt * 32 + wm_row(g, hh);
      const float ds = sa[qt][g] * (pa[qt][g] - s_d[qrow]);
      pa[qt][g] = ds;
      s_ds[qrow * kLdT + key] = f32_to_bf16_bits(ds);
    }
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      // two bf16 terms each (the rounded value and what the rounding left): these two products sum over the QUERIES, and
      // padded query rows are dropped, so a window with few real tokens has few terms and a one-term rounding of p / dS
      // (up to 2^-8) does not average out -- see the header comment
      const wm_u4 ado = wm_ld_perm(s_dot, kLdT, r, qt * 32 + 16 * s, hh), aq = wm_ld_perm(s_qt, kLdT, r, qt * 32 + 16 * s, hh);
      const wm_u4 ph = wm_pack(sa[qt], s), dh = wm_pack(pa[qt], s);
      dv = wm_mfma(ado, ph, dv);
      dv = wm_mfma(ado, wm_pack_rest(sa[qt], s, ph), dv);
      dk = wm_mfma(aq, dh, dk);
      dk = wm_mfma(aq, wm_pack_rest(pa[qt], s, dh), dk);
    }
  }
  // dk[g] = dK[key][channel wm_row(g, hh)] (unscaled), dv the same
#pragma unroll
  for (int g = 0; g < 16; ++g) dk[g] *= a.scale;
  if (ktok >= 0) {
    uint16_t* gp = grad_qkv + ktok * a.ld + C + h * kWaHd + 4 * hh;
#pragma unroll
    for (int q4 = 0; q4 < 4; ++q4) {
      *reinterpret_cast<wm_u2*>(gp + 8 * q4) =
          wm_u2{f32x2_to_bf16x2(dk[4 * q4], dk[4 * q4 + 1]), f32x2_to_bf16x2(dk[4 * q4 + 2], dk[4 * q4 + 3])};
      *reinterpret_cast<wm_u2*>(gp + C + 8 * q4) =
          wm_u2{f32x2_to_bf16x2(dv[4 * q4], dv[4 * q4 + 1]), f32x2_to_bf16x2(dv[4 * q4 + 2], dv[4 * q4 + 3])};
    }
  }
  {                                                   // the image-padded keys of this wave: a fixed butterfly over the 32 key lanes
    const bool pad = ktok == -1;
    if (__any(pad)) {
#pragma unroll
      for (int g = 0; g < 16; ++g) {
        float xk = pad ? dk[g] : 0.f, xv = pad ? dv[g] : 0.f;
#pragma unroll
        for (int sh = 1; sh < 32; sh <<= 1) {
          xk += __shfl_xor(xk, sh);
          xv += __shfl_xor(xv, sh);
        }
        if (r == 0) {
          s_pp[wave][wm_row(g, hh)] = xk;
          s_pp[wave][32 + wm_row(g, hh)] = xv;
        }
      }
    } else {
      s_pp[wave][lane] = 0.f;
    }
  }
  __syncthreads();

  // phase B: this wave's query tile, dQ^T = K^T dS^T: dq[g] = dQ[query][channel wm_row(g, hh)]
  const int query = wave * 32 + r;
  const int64_t qtok = query < N ? wa_token(a, b, win, query) : kWmTilePad;
  wm_f16 dq;
#pragma unroll
  for (int g = 0; g < 16; ++g) dq[g] = 0.f;
#pragma unroll
  for (int kb = 0; kb < 2 * NT; ++kb)
    dq = wm_mfma(wm_ld16(s_kt + r * kLdT + kb * 16 + 8 * hh), wm_ld16(s_ds + query * kLdT + kb * 16 + 8 * hh), dq);
  if (qtok >= 0) {
    uint16_t* gp = grad_qkv + qtok * a.ld + h * kWaHd + 4 * hh;
#pragma unroll
    for (int q4 = 0; q4 < 4; ++q4)
      *reinterpret_cast<wm_u2*>(gp + 8 * q4) =
          wm_u2{f32x2_to_bf16x2(dq[4 * q4] * a.scale, dq[4 * q4 + 1] * a.scale),
                f32x2_to_bf16x2(dq[4 * q4 + 2] * a.scale, dq[4 * q4 + 3] * a.scale)};
  }
  // phase C: thread = table entry t: the sum over the query rows of dS at relative offset t, in row order
  float* part = partial + int64_t(blockIdx.x) * (T + 64);
  for (int t = tid; t < T; t += 64 * NT) {
    const int dy = t / (2 * a.w - 1) - (a.w - 1), dx = t % (2 * a.w - 1) - (a.w - 1);
    float acc = 0.f;
    for (int yi = max(0, dy); yi < min(a.w, a.w + dy); ++yi)
      for (int xi = max(0, dx); xi < min(a.w, a.w + dx); ++xi) {
        const int i = yi * a.w + xi, j = (yi - dy) * a.w + (xi - dx);
        acc += __uint_as_float(uint32_t(s_ds[i * kLdT + j]) << 16);
      }
    part[t] = acc;
  }
  if (tid < 64) {
    float acc = 0.f;
#pragma unroll
    for (int wv = 0; wv < NT; ++wv) acc += s_pp[wv][tid];
    part[T + tid] = acc;
  }
}

template <int NT>
static void wm_launch_fwd(const WaArgs& a, uint32_t grid, void* out, void* lse, hipStream_t stream) {
  hipLaunchKernelGGL(window_attn_mfma_fwd_kernel<NT>, dim3(grid), dim3(64 * NT), 0, stream, a, (uint16_t*)out, (float*)lse);
}
template <int NT>
static void wm_launch_bwd(const WaArgs& a, uint32_t grid, const void* lse, const void* grad_out, void* grad_qkv,
                          void* partial, hipStream_t stream) {
  hipLaunchKernelGGL(window_attn_mfma_bwd_kernel<NT>, dim3(grid), dim3(64 * NT), 0, stream, a, (const float*)lse,
                     (const uint16_t*)grad_out, (uint16_t*)grad_qkv, (float*)partial);
}

int window_attention_mfma_forward(const WaArgs& a, void* out, void* lse, hipStream_t stream) {
  const uint32_t grid = uint32_t(int64_t(a.B) * a.nwin * a.heads);
  switch ((a.w * a.w + 31) / 32) {                    // window 1..12: 1..5 tiles of 32 rows
    case 1: wm_launch_fwd<1>(a, grid, out, lse, stream); break;
    case 2: wm_launch_fwd<2>(a, grid, out, lse, stream); break;
    case 3: wm_launch_fwd<3>(a, grid, out, lse, stream); break;
    case 4: wm_launch_fwd<4>(a, grid, out, lse, stream); break;
    default: wm_launch_fwd<5>(a, grid, out, lse, stream); break;
  }
  return check_launch("window_attn_mfma_fwd");
}

// (`out` is not read: D comes from the kernel's own p and dP, see the header comment)
int window_attention_mfma_backward(const WaArgs& a, const void* /*out*/, const void* lse, const void* grad_out, void* grad_qkv,
                                   void* partial, hipStream_t stream) {
  const uint32_t grid = uint32_t(int64_t(a.B) * a.nwin * a.heads);
  switch ((a.w * a.w + 31) / 32) {
    case 1: wm_launch_bwd<1>(a, grid, lse, grad_out, grad_qkv, partial, stream); break;
    case 2: wm_launch_bwd<2>(a, grid, lse, grad_out, grad_qkv, partial, stream); break;
    case 3: wm_launch_bwd<3>(a, grid, lse, grad_out, grad_qkv, partial, stream); break;
    case 4: wm_launch_bwd<4>(a, grid, lse, grad_out, grad_qkv, partial, stream); break;
    default: wm_launch_bwd<5>(a, grid, lse, grad_out, grad_qkv, partial, stream); break;
  }
  return check_launch("window_attn_mfma_bwd");
}

}  // namespace vnx
