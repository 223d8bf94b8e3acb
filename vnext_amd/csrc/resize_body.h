// resize_body.h -- the one copy of the resize + ingest kernel (DESIGN sections 21, 24 and 30), instantiated three times:
//   resize.hip   kWindow = false  vnx_resize_ingest_frames: the whole frame, never flipped, a source row of 3 words and a
//                                 coefficient row of 6.  The window and the flip are compile-time constants there: the
//                                 instantiation holds none of their arithmetic.
//   augment.hip  kWindow = true   vnx_augment_frames: a crop window {x0, y0, cw, ch} inside the frame and a horizontal flip
//                                 flag, a source row of 8 words and a coefficient row of 8.
//   augment.hip  kBytes = true    vnx_resize_window_bytes: the WHOLE frame resized to (h1, w1), of which only the window
//                                 {x0, y0, cw, ch} of the RESULT is computed and stored -- as bytes, in the frame's own
//                                 layout, into the pixel buffer itself.  One row of 16 words per frame holds the geometry
//                                 and the two coefficient triples.  No normalisation, no padding mask, never flipped.
// The arithmetic, the tiling and the LDS layout are described at the head of resize.hip.  What the window changes: the
// coefficient tables are those of (cw -> nw) and (ch -> nh) and count from the window's origin, while the row pitch stays the
// frame's w and the CHW plane stride h * w.  What the flip changes: output column x takes resized column nw - 1 - x, an index
// where a tile's 32 horizontal bounds and weight rows are staged; the bytes written to LDS and phase V are the same code.
// What kBytes changes: the coefficient tables are those of (w -> w1) and (h -> h1) and output pixel (y, x) of the window
// takes their rows y0 + y and x0 + x -- again an index where the bounds and weights are staged.  Phase V's bytes go to a
// tile of LDS instead of through the normalisation, and from there to memory in 16-byte pieces (see the stores).
//
// kColor (augment.hip): detectron2's RandomBrightness / RandomContrast / RandomSaturation on the bytes
// phase V made, before the normalisation.  A colour row of 8 words per frame holds {flags, the brightness weight's fp32 bits,
// the contrast weight (a double: low word, high word), the saturation weight (likewise), 0, 0}.
//   kColor = 1  vnx_augment_frames_color without contrast: brightness and saturation are pointwise, so they sit between
//               phase V and the normalisation of the SAME launch.
//   kColor = 2  the first of two launches when contrast is on: contrast blends with the mean of the whole frame AFTER
//               brightness, so this pass stores the post-brightness bytes ([B][3][H][W], a word of 4 pixels per thread) and
//               each tile's integer sum (one uint32 per workgroup, every slot written) behind the frames in the pixel buffer;
//               augment.hip's second kernel folds the sums and finishes.
// The double expressions are the reference's numpy expressions, rounding for rounding: contraction is OFF for this whole
// file (the pragma below), so a product and the sum that takes it stay two roundings.
#pragma once

#include "vnx_common.h"

#pragma clang fp contract(off)

namespace vnx {
namespace {

constexpr int kResizeThreads = 256;
constexpr int kTile = 32;                  // output rows and columns of a workgroup
constexpr int kMaxKsize = 17;              // VNX_RESIZE_MAX_KSIZE
constexpr int kMaxRows = 272;              // staged source rows of a tile: (kTile + 1) * 8 + 1 at the limit, rounded up
constexpr int kAugSrcWords = 8;            // {byte offset, h, w, x0, y0, cw, ch, flip}
constexpr int kAugCoeffWords = 8;          // the two bilinear triples, then the offsets of the two nearest tables (augment.hip)
constexpr int kWinWords = 16;              // {src byte offset, h, w, h1, w1, x0, y0, cw, ch, dst byte offset, the two triples}

constexpr int kColorWords = 8;             // {flags, brightness fp32 bits, contrast lo, hi, saturation lo, hi, 0, 0}
constexpr int kBrightness = 1, kContrast = 2, kSaturation = 4;      // the flags

typedef uint32_t rsz_u4 __attribute__((ext_vector_type(4)));

struct ResizeArgs {
  const unsigned char* pixels;
  long long pixel_bytes;
  const int32_t* src_table;
  const int32_t* dst_table;
  const int32_t* coeffs;
  long long coeff_words;
  float* x;
  unsigned char* mask;                     // (kBytes: the pixel buffer again, writable: the windows are stored into it)
  int B, H, W, channels_last, interleaved;
  float mean[3], std[3];
  const int32_t* color;                    // kColor: [B][8]
  unsigned char* stage;                    // kColor = 2 and the second kernel: [B][3][H][W] post-brightness bytes
  uint32_t* sums;                          //   and [B][tiles] sums of them
};

struct AxisTab { int bounds, kk, ksize; };      // ksize 0: the pass is skipped

struct ResizeGeom {
  int off, h, w, nh, nw;      // nh == 0: the empty frame
  int x0, y0, cw, ch, flip;   // the window and the flip (kWindow false: 0, 0, w, h, 0)
  AxisTab hor, ver;
};

// kBytes only (beside ResizeGeom, whose nh x nw is then the window's size): the window's origin inside the resized h1 x w1
// image, and the byte offset of its slot inside the pixel buffer
struct WindowOut { int ox, oy, dst; };

// one axis of a frame's coefficient row: inside the buffer for n_out rows of bounds and weights, or a skipped pass
__device__ __forceinline__ bool axis_ok(const AxisTab t, int n_in, int n_out, long long words) {
  if (t.ksize == 0) return n_in == n_out;
  return t.ksize >= 1 && t.ksize <= kMaxKsize && t.bounds >= 0 && t.kk >= 0 && (long long)t.bounds + 2ll * n_out <= words &&
         (long long)t.kk + (long long)n_out * t.ksize <= words;
}

// frame `b` as the tables describe it, or the empty frame
template <bool kWindow>
__device__ __forceinline__ ResizeGeom resize_geom(const int32_t* __restrict__ src_table, const int32_t* __restrict__ dst_table,
                                                  const int32_t* __restrict__ coeffs, long long coeff_words,
                                                  long long pixel_bytes, int H, int W, int b) {
  ResizeGeom g;
  const int32_t* s = src_table + (kWindow ? kAugSrcWords : 3) * size_t(b);
  g.off = s[0]; g.h = s[1]; g.w = s[2];
  if constexpr (kWindow) {
    g.x0 = s[3]; g.y0 = s[4]; g.cw = s[5]; g.ch = s[6]; g.flip = s[7] != 0;
  } else {
    g.x0 = 0; g.y0 = 0; g.cw = g.w; g.ch = g.h; g.flip = 0;
  }
  const int zero = dst_table[3 * b];
  g.nh = dst_table[3 * b + 1]; g.nw = dst_table[3 * b + 2];
  const int32_t* row = coeffs + (kWindow ? kAugCoeffWords : 6) * size_t(b);      // (the host checked rows * B <= coeff_words)
  g.hor = AxisTab{row[0], row[1], row[2]};
  g.ver = AxisTab{row[3], row[4], row[5]};
  bool ok = g.off >= 0 && g.h >= 1 && g.w >= 1 && (long long)g.off + 3ll * g.h * g.w <= pixel_bytes && zero >= 0 &&
            g.nh >= 1 && g.nw >= 1 && g.nh <= H && g.nw <= W && axis_ok(g.hor, g.cw, g.nw, coeff_words) &&
            axis_ok(g.ver, g.ch, g.nh, coeff_words);
  if constexpr (kWindow)      // the window lies inside the frame (x0 + cw <= w <= 2^31 - 1: no overflow once the parts are in range)
    ok = ok && g.x0 >= 0 && g.y0 >= 0 && g.cw >= 1 && g.ch >= 1 && g.cw <= g.w && g.ch <= g.h && g.x0 <= g.w - g.cw &&
         g.y0 <= g.h - g.ch;
  if (!ok) g.nh = g.nw = 0;
  return g;
}

// frame `b` of vnx_resize_window_bytes as its row describes it, or the empty frame.  The source window is the whole frame;
// the "target" nh x nw is the window ch x cw of the resized image, which must lie inside (h1, w1) and inside H x W; its
// 3 * ch * cw bytes must lie inside the buffer and apart from the frame's own source bytes.
__device__ __forceinline__ ResizeGeom window_geom(const int32_t* __restrict__ win_table, long long coeff_words,
                                                  long long pixel_bytes, int H, int W, int b, WindowOut& o) {
  ResizeGeom g;
  const int32_t* s = win_table + kWinWords * size_t(b);
  g.off = s[0]; g.h = s[1]; g.w = s[2];
  const int h1 = s[3], w1 = s[4];
  o.ox = s[5]; o.oy = s[6]; g.nw = s[7]; g.nh = s[8]; o.dst = s[9];
  g.x0 = 0; g.y0 = 0; g.cw = g.w; g.ch = g.h; g.flip = 0;
  g.hor = AxisTab{s[10], s[11], s[12]};
  g.ver = AxisTab{s[13], s[14], s[15]};
  // pixel counts first (a product of two int32 fits 64 bits; three times one that is at most pixel_bytes < 2^31 does too)
  const long long src_px = (long long)g.h * g.w, dst_px = (long long)g.nh * g.nw;
  bool ok = g.off >= 0 && g.h >= 1 && g.w >= 1 && src_px <= pixel_bytes && h1 >= 1 && w1 >= 1 && g.nh >= 1 && g.nw >= 1 &&
            g.nh <= H && g.nw <= W && o.ox >= 0 && o.oy >= 0 && g.nw <= w1 && g.nh <= h1 && o.ox <= w1 - g.nw &&
            o.oy <= h1 - g.nh && o.dst >= 0 && dst_px <= pixel_bytes && axis_ok(g.hor, g.w, w1, coeff_words) &&
            axis_ok(g.ver, g.h, h1, coeff_words);
  if (ok) {
    const long long src_end = g.off + 3 * src_px, dst_end = o.dst + 3 * dst_px;
    ok = src_end <= pixel_bytes && dst_end <= pixel_bytes && (dst_end <= g.off || o.dst >= src_end);
  }
  if (!ok) g.nh = g.nw = 0;
  return g;
}

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// byte `at` (inside the buffer) through the aligned word around it; `cur` / `word` remember the last word fetched
__device__ __forceinline__ uint32_t source_byte(const unsigned char* __restrict__ pixels, long long pixel_bytes, long long at,
                                                long long& cur, uint32_t& word) {
  const long long lo = at & ~3ll;
  if (lo != cur) {
    cur = lo;
    if (lo + 4 <= pixel_bytes) {      // `pixels` is 4-byte aligned
      word = *reinterpret_cast<const uint32_t*>(pixels + lo);
    } else {                          // the buffer's last bytes
      word = 0;
      for (int j = 0; j < 4; ++j)
        if (lo + j < pixel_bytes) word |= uint32_t(pixels[lo + j]) << (8 * j);
    }
  }
  return (word >> (8 * int(at & 3))) & 0xffu;
}

// ---- colour (kColor) ----
struct ColorRow { int flags; float wb; double wc, ws; };

// frame `b`'s colour row; `allowed`: the flags this launch can honour.  A flag outside them, or a weight in use that is
// not finite, is a malformed row: -> false, and the frame is the empty frame
__device__ __forceinline__ bool color_row(const int32_t* __restrict__ color, int b, int allowed, ColorRow& r) {
  const int32_t* s = color + kColorWords * size_t(b);
  r.flags = s[0];
  r.wb = __int_as_float(s[1]);
  r.wc = __hiloint2double(s[3], s[2]);
  r.ws = __hiloint2double(s[5], s[4]);
  return (r.flags & ~allowed) == 0 && (!(r.flags & kBrightness) || __builtin_isfinite(r.wb)) &&
         (!(r.flags & kContrast) || __builtin_isfinite(r.wc)) && (!(r.flags & kSaturation) || __builtin_isfinite(r.ws));
}

// np.clip(x, 0, 255).astype(np.uint8): the conversion truncates
__device__ __forceinline__ uint32_t clip_byte(float x) { return uint32_t(x < 0.f ? 0.f : (x > 255.f ? 255.f : x)); }
__device__ __forceinline__ uint32_t clip_byte(double x) { return uint32_t(x < 0.0 ? 0.0 : (x > 255.0 ? 255.0 : x)); }

// BlendTransform in float64: src + w * float64(u), where src = (1 - w) * {mean, gray} is rounded already; the product is
// rounded, then the sum (no contraction in this file)
__device__ __forceinline__ uint32_t blend_byte(double src, double w, uint32_t u) { return clip_byte(src + w * double(u)); }

// px[c]: 4 pixels of channel c, a byte each.  Brightness: float32(w) * float32(u), one rounding
__device__ __forceinline__ void brighten_words(uint32_t (&px)[3], float w) {
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    uint32_t out = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) out |= clip_byte(w * float((px[c] >> (8 * j)) & 0xffu)) << (8 * j);
    px[c] = out;
  }
}

// Contrast: (1 - w) * mean + w * float64(u)
__device__ __forceinline__ void contrast_words(uint32_t (&px)[3], double w, double mean) {
  const double src = (1.0 - w) * mean;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    uint32_t out = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) out |= blend_byte(src, w, (px[c] >> (8 * j)) & 0xffu) << (8 * j);
    px[c] = out;
  }
}

// Saturation: gray = c0 * 0.299 + c1 * 0.587 + c2 * 0.114, three rounded products summed left to right, then
// (1 - w) * gray + w * float64(u_c) per channel
__device__ __forceinline__ void saturate_words(uint32_t (&px)[3], double w) {
  uint32_t out[3] = {0u, 0u, 0u};
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const uint32_t u0 = (px[0] >> (8 * j)) & 0xffu, u1 = (px[1] >> (8 * j)) & 0xffu, u2 = (px[2] >> (8 * j)) & 0xffu;
    const double gray = double(u0) * 0.299 + double(u1) * 0.587 + double(u2) * 0.114;
    const double src = (1.0 - w) * gray;
    out[0] |= blend_byte(src, w, u0) << (8 * j);
    out[1] |= blend_byte(src, w, u1) << (8 * j);
    out[2] |= blend_byte(src, w, u2) << (8 * j);
  }
  px[0] = out[0]; px[1] = out[1]; px[2] = out[2];
}

template <bool kWindow, bool kBytes>
__device__ __forceinline__ ResizeGeom frame_geom(const ResizeArgs& a, int b, WindowOut& wo) {
  if constexpr (kBytes) return window_geom(a.src_table, a.coeff_words, a.pixel_bytes, a.H, a.W, b, wo);
  else return resize_geom<kWindow>(a.src_table, a.dst_table, a.coeffs, a.coeff_words, a.pixel_bytes, a.H, a.W, b);
}

// frame `b` of a colour launch: the geometry of vnx_augment_frames, emptied where the colour row is malformed or, with two
// launches (kColor = 2, and the second kernel alike), where the frame's source bytes reach into the staging area
template <int kColor>
__device__ __forceinline__ ResizeGeom color_geom(const ResizeArgs& a, int b, ColorRow& cr) {
  ResizeGeom g = resize_geom<true>(a.src_table, a.dst_table, a.coeffs, a.coeff_words, a.pixel_bytes, a.H, a.W, b);
  bool ok = color_row(a.color, b, kColor == 2 ? (kBrightness | kContrast | kSaturation) : (kBrightness | kSaturation), cr);
  if constexpr (kColor == 2)      // (a live g: off + 3 h w <= pixel_bytes < 2^31)
    ok = ok && g.nh > 0 && (long long)g.off + 3ll * g.h * g.w <= (long long)(a.stage - a.pixels);
  if (!ok) g.nh = g.nw = 0;
  return g;
}

// x of 4 pixels of one output row, contiguous or channels-last
__device__ __forceinline__ void store_x(const ResizeArgs& a, int b, int y, int x0, const float (&val)[3][4]) {
  const int H = a.H, W = a.W;
  const size_t row = size_t(b) * H + y;
  if (a.channels_last) {
    float* out = a.x + (row * W + x0) * 3;
    *reinterpret_cast<vnx_f4*>(out) = vnx_f4{val[0][0], val[1][0], val[2][0], val[0][1]};
    *reinterpret_cast<vnx_f4*>(out + 4) = vnx_f4{val[1][1], val[2][1], val[0][2], val[1][2]};
    *reinterpret_cast<vnx_f4*>(out + 8) = vnx_f4{val[2][2], val[0][3], val[1][3], val[2][3]};
  } else {
#pragma unroll
    for (int c = 0; c < 3; ++c)
      *reinterpret_cast<vnx_f4*>(a.x + ((size_t(b) * 3 + c) * H + y) * W + x0) =
          vnx_f4{val[c][0], val[c][1], val[c][2], val[c][3]};
  }
}

// the padding mask of a tile: 16 pixels per thread, 64 threads
__device__ __forceinline__ void store_mask(const ResizeArgs& a, int b, int oy0, int ox0, int tid, int nh, int nw) {
  if (tid < 2 * kTile) {
    const int y = oy0 + (tid >> 1), x0 = ox0 + ((tid & 1) << 4);
    rsz_u4 v;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      uint32_t word = 0;
#pragma unroll
      for (int j = 0; j < 4; ++j) word |= uint32_t(y >= nh || x0 + 4 * k + j >= nw) << (8 * j);
      v[k] = word;
    }
    *reinterpret_cast<rsz_u4*>(a.mask + ((size_t(b) * a.H + y) * a.W + x0)) = v;
  }
}

template <bool kWindow, bool kBytes = false, int kColor = 0>
__global__ __launch_bounds__(kResizeThreads) void resize_ingest_kernel(ResizeArgs a) {
  static_assert(kColor == 0 || (kWindow && !kBytes), "colour rides on the augment instantiation");
  __shared__ __attribute__((aligned(16))) unsigned char rows[3][kMaxRows][kTile];
  __shared__ uint32_t kh[kTile][kMaxKsize], kv[kTile][kMaxKsize];
  __shared__ int bh[kTile][2], bv[kTile][2];      // {first source column, taps}; {first staged row, taps}
  __shared__ __attribute__((aligned(16))) unsigned char obuf[kBytes ? 3 * kTile * kTile : 16];      // kBytes: the tile's bytes
  __shared__ uint32_t wave_sum[kResizeThreads / 64];      // kColor = 2: the waves' sums of the tile's bytes

  const int H = a.H, W = a.W, tid = threadIdx.x;
  const int tiles_x = W / kTile, tiles_y = H / kTile;
  const int tx = blockIdx.x % tiles_x;
  const int rest = blockIdx.x / tiles_x;
  const int ty = rest % tiles_y, b = rest / tiles_y;
  const int ox0 = tx * kTile, oy0 = ty * kTile;
  WindowOut wo{};
  ColorRow cr{};
  const ResizeGeom g = [&] {                                    // workgroup-uniform
    if constexpr (kColor != 0) return color_geom<kColor>(a, b, cr);
    else return frame_geom<kWindow, kBytes>(a, b, wo);
  }();
  const bool live = oy0 < g.nh && ox0 < g.nw;              // the tile holds pixels of the frame

  if (live) {
    const int rows_out = min(kTile, g.nh - oy0), cols_out = min(kTile, g.nw - ox0);
    // the resized row an output row takes: itself, or (kBytes) the row of the window's origin further down
    auto resized_row = [&](int y) { return kBytes ? wo.oy + y : y; };
    // the window's rows this tile's output rows reach: [r0, r1)
    int r0, r1;
    if (g.ver.ksize == 0) {
      r0 = resized_row(oy0); r1 = r0 + rows_out;           // nh == ch
    } else {
      const int32_t* bnd = a.coeffs + g.ver.bounds;
      const int last = resized_row(oy0 + rows_out - 1);
      r0 = clampi(bnd[2 * resized_row(oy0)], 0, g.ch);
      r1 = clampi(clampi(bnd[2 * last], 0, g.ch) + clampi(bnd[2 * last + 1], 0, g.ver.ksize), r0, g.ch);
      if (r1 - r0 > kMaxRows) r1 = r0 + kMaxRows;
    }
    // ---- stage the tile's bounds and weights ----
    // the resized column an output column takes: itself, or with the flip its mirror (a tile at the frame's right edge then
    // holds the frame's FIRST resized columns)
    auto resized_col = [&](int x) { return kBytes ? wo.ox + x : (kWindow && g.flip ? g.nw - 1 - x : x); };
    if (tid < kTile) {
      int first = 0, cnt = 0;
      if (tid < cols_out) {
        const int xr = resized_col(ox0 + tid);
        if (g.hor.ksize == 0) { first = xr; cnt = 1; }
        else {
          const int32_t* bnd = a.coeffs + g.hor.bounds + 2 * xr;
          first = clampi(bnd[0], 0, g.cw);
          cnt = clampi(bnd[1], 0, min(g.hor.ksize, g.cw - first));
        }
      }
      bh[tid][0] = first; bh[tid][1] = cnt;
    } else if (tid < 2 * kTile) {
      const int r = tid - kTile;
      int first = 0, cnt = 0;
      if (r < rows_out) {
        if (g.ver.ksize == 0) { first = r; cnt = 1; }
        else {
          const int32_t* bnd = a.coeffs + g.ver.bounds + 2 * resized_row(oy0 + r);
          const int y = clampi(bnd[0], r0, r1);
          first = y - r0;
          cnt = clampi(bnd[1], 0, min(g.ver.ksize, r1 - y));
        }
      }
      bv[r][0] = first; bv[r][1] = cnt;
    }
    for (int i = tid; i < 2 * kTile * kMaxKsize; i += kResizeThreads) {
      const bool vert = i >= kTile * kMaxKsize;
      const int j = vert ? i - kTile * kMaxKsize : i;
      const int r = j / kMaxKsize, t = j - r * kMaxKsize;
      const AxisTab tab = vert ? g.ver : g.hor;
      const bool have = r < (vert ? rows_out : cols_out) && t < tab.ksize;
      const int idx = vert ? resized_row(oy0 + r) : resized_col(ox0 + r);      // (in range wherever `have` holds)
      const uint32_t k = have ? uint32_t(a.coeffs[tab.kk + (long long)idx * tab.ksize + t]) : 0u;
      (vert ? kv : kh)[r][t] = k;
    }
    __syncthreads();

    // ---- phase H: window rows [r0, r1) at the tile's columns -> bytes in LDS ----
    const int col = tid & (kTile - 1), sub = tid >> 5;      // 8 rows at a time
    const int first = bh[col][0], cnt = bh[col][1];
    const int n_rows = r1 - r0;
    const long long plane = (long long)g.h * g.w;
    const int step = a.interleaved ? 3 : 1;
    for (int c = 0; c < 3; ++c) {
      for (int r = sub; r < n_rows; r += kResizeThreads / kTile) {
        uint32_t u = 0;
        if (col < cols_out) {
          // pixel index of the first tap inside the frame: the row pitch is the FRAME's width
          const long long px = (long long)(g.y0 + r0 + r) * g.w + g.x0 + first;
          long long at = g.off + (a.interleaved ? px * 3 + c : c * plane + px);
          long long cur = -4;
          uint32_t word = 0;
          if (g.hor.ksize == 0) {
            u = source_byte(a.pixels, a.pixel_bytes, at, cur, word);
          } else {
            uint32_t acc = 1u << 21;
            for (int t = 0; t < cnt; ++t, at += step)
              acc += __umul24(kh[col][t], source_byte(a.pixels, a.pixel_bytes, at, cur, word));
            u = min(acc >> 22, 255u);
          }
        }
        rows[c][r][col] = (unsigned char)u;
      }
    }
    __syncthreads();
  }

  // ---- phase V and the stores: 4 pixels of one output row per thread ----
  {
    const int ly = tid >> 3, lx = (tid & 7) << 2;
    const int y = oy0 + ly, x0 = ox0 + lx;
    float val[3][4];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
#pragma unroll
      for (int j = 0; j < 4; ++j) val[c][j] = 0.f;
    }
    uint32_t px[3] = {0u, 0u, 0u};                           // the thread's 4 pixels, a word of bytes per channel
    const bool inside = live && y < g.nh && x0 < g.nw;
    if (inside) {
      const int first = bv[ly][0], cnt = bv[ly][1];
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        uint32_t bytes;
        if (g.ver.ksize == 0) {
          bytes = *reinterpret_cast<const uint32_t*>(&rows[c][first][lx]);
        } else {
          uint32_t acc[4] = {1u << 21, 1u << 21, 1u << 21, 1u << 21};
          for (int t = 0; t < cnt; ++t) {
            const uint32_t k = kv[ly][t];
            const uint32_t wd = *reinterpret_cast<const uint32_t*>(&rows[c][first + t][lx]);
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[j] += __umul24(k, (wd >> (8 * j)) & 0xffu);
          }
          bytes = 0;
#pragma unroll
          for (int j = 0; j < 4; ++j) bytes |= min(acc[j] >> 22, 255u) << (8 * j);
        }
        if constexpr (kBytes) {      // the tile as it will lie in memory: planes of 32 x 32, or rows of 32 pixels of 3 bytes
          if (a.interleaved) {
#pragma unroll
            for (int j = 0; j < 4; ++j) obuf[(ly * kTile + lx + j) * 3 + c] = (unsigned char)(bytes >> (8 * j));
          } else {
            *reinterpret_cast<uint32_t*>(&obuf[(c * kTile + ly) * kTile + lx]) = bytes;
          }
          continue;
        }
        px[c] = bytes;
      }
      if constexpr (kColor != 0) {                           // (the flags are workgroup-uniform)
        if (cr.flags & kBrightness) brighten_words(px, cr.wb);
        if constexpr (kColor == 1)
          if (cr.flags & kSaturation) saturate_words(px, cr.ws);
      }
      if constexpr (!kBytes && kColor != 2) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
#pragma unroll
          for (int j = 0; j < 4; ++j)
            if (x0 + j < g.nw) val[c][j] = (float((px[c] >> (8 * j)) & 0xffu) - a.mean[c]) / a.std[c];
        }
      }
    }
    if constexpr (kColor == 2) {
      // ---- the first of two launches: the post-brightness bytes and the tile's sum of them (pixels inside the frame only) ----
      uint32_t s = 0;
      if (inside) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          *reinterpret_cast<uint32_t*>(a.stage + ((size_t(b) * 3 + c) * H + y) * W + x0) = px[c];
#pragma unroll
          for (int j = 0; j < 4; ++j)
            if (x0 + j < g.nw) s += (px[c] >> (8 * j)) & 0xffu;
        }
      }
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) s += uint32_t(__shfl_xor(int(s), off, 64));
      if ((tid & 63) == 0) wave_sum[tid >> 6] = s;
      __syncthreads();
      if (tid == 0) {                                        // every slot is written, a dead tile's with 0: no memset
        for (int w = 1; w < kResizeThreads / 64; ++w) s += wave_sum[w];
        a.sums[blockIdx.x] = s;                              // (at most 32 * 32 * 3 * 255)
      }
      return;
    }
    if constexpr (kBytes) {
      // ---- the window's bytes: whole 16-byte pieces of memory where a tile row covers them, bytes at its two ends ----
      // A tile row is `len` bytes at `base` (any alignment; CHW: 3 * 32 rows of up to 32 bytes, HWC: 32 rows of up to 96).
      // Piece k of a row is the ALIGNED 16 bytes at (base & ~15) + 16 k: a piece that lies inside the row is one store, a
      // piece the row only touches is written byte by byte -- its other bytes belong to the neighbouring tile, row or slot.
      if (!live) return;                                     // (workgroup-uniform)
      __syncthreads();
      const int rows_out = min(kTile, g.nh - oy0), cols_out = min(kTile, g.nw - ox0);
      const int bpp = a.interleaved ? 3 : 1, lines = a.interleaved ? rows_out : 3 * rows_out;
      const int len = cols_out * bpp, pitch = kTile * bpp, pieces = pitch / 16 + 1;
      const long long plane = (long long)g.nh * g.nw;
      for (int item = tid; item < lines * pieces; item += kResizeThreads) {
        const int line = item / pieces, k = item - line * pieces;
        const int c = a.interleaved ? 0 : line / rows_out, r = a.interleaved ? line : line - c * rows_out;
        const long long px = (long long)(oy0 + r) * g.nw + ox0;
        unsigned char* base = a.mask + wo.dst + (a.interleaved ? px * 3 : c * plane + px);
        const unsigned char* from = obuf + (a.interleaved ? r : c * kTile + r) * pitch;
        const int lead = int(reinterpret_cast<uintptr_t>(base) & 15);
        const int lo = 16 * k - lead;                        // the piece is bytes [lo, lo + 16) of the row
        if (lo >= len) continue;
        if (lo >= 0 && lo + 16 <= len) {
          rsz_u4 v;
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            uint32_t word = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) word |= uint32_t(from[lo + 4 * q + j]) << (8 * j);
            v[q] = word;
          }
          *reinterpret_cast<rsz_u4*>(base + lo) = v;
        } else {
          for (int j = max(lo, 0); j < min(lo + 16, len); ++j) base[j] = from[j];
        }
      }
      return;
    }
    store_x(a, b, y, x0, val);
  }
  store_mask(a, b, oy0, ox0, tid, g.nh, g.nw);
}

// what the entry points check before they launch -> the kernel's arguments and its grid (blocks 0: nothing to launch)
template <bool kWindow>
inline int resize_ingest_args(const char* fn, const void* pixels, size_t pixel_bytes, const void* src_table,
                              const void* dst_table, const void* coeffs, size_t coeff_words, int batch, int height, int width,
                              const float* mean, const float* std, int channels_last, int interleaved, void* x, void* mask,
                              ResizeArgs& a, unsigned& grid) {
  constexpr int kRow = kWindow ? kAugCoeffWords : 6;
  grid = 0;
  if (batch < 0 || height < 32 || width < 32 || height % 32 != 0 || width % 32 != 0) {
    set_error("%s: bad sizes (batch %d, padded %d x %d: multiples of 32)", fn, batch, height, width);
    return VNX_ERR_INVALID_ARGUMENT;
  }
  if (batch == 0) return VNX_OK;
  if (!pixels || !src_table || !dst_table || !coeffs || !x || !mask) {
    set_error("%s: null pointer argument", fn);
    return VNX_ERR_INVALID_ARGUMENT;
  }
  if ((reinterpret_cast<uintptr_t>(pixels) & 3) != 0 || (reinterpret_cast<uintptr_t>(src_table) & 3) != 0 ||
      (reinterpret_cast<uintptr_t>(dst_table) & 3) != 0 || (reinterpret_cast<uintptr_t>(coeffs) & 3) != 0 ||
      (reinterpret_cast<uintptr_t>(x) & 15) != 0 || (reinterpret_cast<uintptr_t>(mask) & 15) != 0) {
    set_error("%s: pixels, the tables and coeffs must be 4-byte aligned, x and mask 16-byte aligned", fn);
    return VNX_ERR_INVALID_ARGUMENT;
  }
  if (coeff_words < kRow * size_t(batch)) {
    set_error("%s: coeffs holds %zu words: less than the %d frames' rows of %d", fn, coeff_words, batch, kRow);
    return VNX_ERR_INVALID_ARGUMENT;
  }
  if (pixel_bytes > size_t(0x7fffffff) || coeff_words > size_t(0x7fffffff)) {      // the tables' offsets are int32
    set_error("%s: %zu bytes of pixels, %zu words of coefficients: the tables address 2^31 - 1 at most", fn, pixel_bytes,
              coeff_words);
    return VNX_ERR_UNSUPPORTED;
  }
  const long long blocks = (long long)batch * (height / kTile) * (width / kTile);
  if (blocks > 0x7fffffffll) {
    set_error("%s: %d frames of %d x %d are more than one launch addresses", fn, batch, height, width);
    return VNX_ERR_UNSUPPORTED;
  }
  a = ResizeArgs{};
  a.pixels = (const unsigned char*)pixels;
  a.pixel_bytes = (long long)pixel_bytes;
  a.src_table = (const int32_t*)src_table;
  a.dst_table = (const int32_t*)dst_table;
  a.coeffs = (const int32_t*)coeffs;
  a.coeff_words = (long long)coeff_words;
  a.x = (float*)x;
  a.mask = (unsigned char*)mask;
  a.B = batch; a.H = height; a.W = width; a.channels_last = channels_last != 0; a.interleaved = interleaved != 0;
  for (int c = 0; c < 3; ++c) { a.mean[c] = mean[c]; a.std[c] = std[c]; }
  grid = unsigned(blocks);
  return VNX_OK;
}

// both plain entry points: the checks, and the launch
template <bool kWindow>
inline int launch_resize_ingest(const char* fn, const void* pixels, size_t pixel_bytes, const void* src_table,
                                const void* dst_table, const void* coeffs, size_t coeff_words, int batch, int height, int width,
                                const float* mean, const float* std, int channels_last, int interleaved, void* x, void* mask,
                                void* hip_stream) {
  ResizeArgs a;
  unsigned grid;
  const int rc = resize_ingest_args<kWindow>(fn, pixels, pixel_bytes, src_table, dst_table, coeffs, coeff_words, batch, height,
                                             width, mean, std, channels_last, interleaved, x, mask, a, grid);
  if (rc != VNX_OK || grid == 0) return rc;
  hipLaunchKernelGGL(resize_ingest_kernel<kWindow>, dim3(grid), dim3(kResizeThreads), 0, (hipStream_t)hip_stream, a);
  return check_launch(fn);
}

}  // namespace
}  // namespace vnx
