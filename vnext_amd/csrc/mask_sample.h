// mask_sample.h -- the one copy of the result masks' per-pixel sampling (mask_rle.hip and mask_dense.hip include it).
// The models form a result mask from stride-s logits as
//     m = F.interpolate(logits, size=(h * s, w * s), mode="bilinear", align_corners=False).sigmoid()
//     m = F.interpolate(m[:, :, :ih, :iw], size=(oh, ow), mode="nearest") > 0.5
// Output pixel (y, x) is therefore ONE bilinear sample: ATen's nearest index on the cropped grid, ATen's
// align_corners=False bilinear value of the upsampled map at that index, and the bit is value > 0 (= sigmoid > 0.5 apart
// from |value| within fp32 rounding of 0).
//
// The sample splits per axis: `mask_tap` is everything one output row (or column) contributes -- the first of its two
// source rows and the weight of the second -- and `mask_bit` combines a row's tap with a column's.  A kernel may compute a
// tap where it likes (per pixel, once per row, staged per workgroup): a tap is a function of its arguments alone, so the
// float operands of mask_bit's final expression are the same wherever they were formed, and that expression stands HERE
// only, in one source form.
//
// Contraction.  Under the build's default (-ffp-contract=fast) the back end fuses a product into a sum wherever it meets
// one AFTER the vectoriser has paired the multiplications of neighbouring pixels, so WHICH product of `a * b + c * d` is
// fused depends on the code around the call: inlined into mask_rle.hip's walk the expression below became
// fma(w1l, p1, w0l * p0) for the upper row, inlined into mask_dense.hip's it became fma(w0l, p0, w1l * p1) -- values one
// rounding apart, bits that differ where the sum nearly cancels.  Both functions therefore pin the rule with
// `#pragma clang fp contract(on)`: the front end fuses by the language's rule, per source expression (`a * b + c` and
// `c + a * b` become fma(a, b, c), the left product of a sum of two), before any other pass sees it, and nothing is
// fused beyond that.  The kernels that share this file agree bit for bit (tests/test_mask_dense.py holds them to it on
// inputs built to expose a difference).
#pragma once

#include "vnx_common.h"

namespace vnx {

struct MaskSample {
  int h, w;          // logit map
  int ih, iw;        // image size on the upsampled grid: the crop
  float ry, rx;      // bilinear scales h / (h s), w / (w s) (ATen area_pixel_compute_scale)
  float ny, nx;      // nearest scales ih / oh, iw / ow (ATen compute_scales_value)
};

inline MaskSample mask_sample(int height, int width, int stride, int image_height, int image_width, int out_height,
                              int out_width) {
  MaskSample s;
  s.h = height; s.w = width;
  s.ih = image_height; s.iw = image_width;
  s.ry = float(height) / float(int64_t(height) * stride);
  s.rx = float(width) / float(int64_t(width) * stride);
  s.ny = float(image_height) / float(out_height);
  s.nx = float(image_width) / float(out_width);
  return s;
}

struct MaskTap { int i0; float l1; };      // the first source row / column; the weight of the one after it

// output index `o` of one axis: `nearest` = n_image / n_out, `scale` = n / (n s)
__device__ __forceinline__ MaskTap mask_tap(int o, float nearest, int n_image, float scale) {
#pragma clang fp contract(on)
  const int i = min(int(floorf(float(o) * nearest)), n_image - 1);      // ATen nearest_neighbor_compute_source_index
  float s = scale * (float(i) + 0.5f) - 0.5f;                           // area_pixel_compute_source_index
  s = s < 0.f ? 0.f : s;
  const int i0 = int(s);
  return MaskTap{i0, s - float(i0)};
}

// ATen upsample_bilinear2d (align_corners=False) of the [h, w] map, read where the taps point
__device__ __forceinline__ bool mask_bit(const float* __restrict__ map, int h, int w, MaskTap ty, MaskTap tx) {
#pragma clang fp contract(on)
  const int h1 = ty.i0, w1 = tx.i0;
  const int h1p = h1 < h - 1 ? w : 0, w1p = w1 < w - 1 ? 1 : 0;
  const float h1l = ty.l1, h0l = 1.f - h1l;
  const float w1l = tx.l1, w0l = 1.f - w1l;
  const float* p = map + h1 * w + w1;
  const float v = h0l * (w0l * p[0] + w1l * p[w1p]) + h1l * (w0l * p[h1p] + w1l * p[h1p + w1p]);
  return v > 0.f;
}

__device__ __forceinline__ bool mask_logit_bit(const float* __restrict__ map, const MaskSample& a, int y, int x) {
  return mask_bit(map, a.h, a.w, mask_tap(y, a.ny, a.ih, a.ry), mask_tap(x, a.nx, a.iw, a.rx));
}

}  // namespace vnx
