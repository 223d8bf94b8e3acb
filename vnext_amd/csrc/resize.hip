// resize.hip -- Pillow's 8-bit bilinear resize of uint8 frames fused into the ingest: staged source frames to the network's
// (x, mask) in one launch (vnext_amd/ops/resize.py; include/vnext_hip.h).
//
// The arithmetic is Pillow's ImagingResample for 8 bits per channel, whose result the kernel reproduces byte for byte.  Per
// axis the host computes, in double, for every output index the first source index `xmin`, the tap count `cnt` and `cnt`
// non-negative weights in 22-bit fixed point; a pass is
//   out = min((2^21 + sum_t k[t] * src[xmin + t]) >> 22, 255)
// The horizontal pass runs first and its result is a BYTE; the vertical pass runs on those bytes.  A pass whose axis keeps
// its size is skipped (ksize 0 in the frame's coefficient row): the bytes pass through.  The kernel never evaluates the
// filter: bounds and weights are read from the `coeffs` buffer.  The resized byte u then goes through the ingest kernel's
// expression, (float(u) - mean[c]) / std[c] -- an IEEE subtract and a correctly rounded IEEE divide, contraction off -- so a
// frame whose target equals its source gives exactly what vnx_ingest_frames gives.
//
// Geometry is MEMORY, as in ingest.hip: a source table {byte offset, h, w}, a destination table {0, nh, nw} and, at the
// head of `coeffs`, a row {bounds offset, weights offset, ksize} x {horizontal, vertical} per frame (offsets in int32 words).
// A captured launch replays on new pixels.  A frame whose rows do not describe bytes inside `pixels`, a target inside the
// padded size and tables inside `coeffs` (negative values, nh > H, nw > W, a source end beyond pixel_bytes, ksize outside
// 1 .. 17, a skipped pass whose sizes differ, offsets outside the buffer) is an EMPTY frame: all padding.  The table entries
// themselves are clamped as they are staged -- first source index and tap count to the source row / the staged rows -- so
// no read leaves a buffer whatever the tables hold; on tables the host made the clamps change nothing.
//
// Tiling.  One workgroup of 256 threads per (frame, 32 x 32 tile of the padded output), all three channels.
//   stage:   the tile's 32 horizontal and 32 vertical bounds and weight rows go to LDS (clamped), 17 words per row.
//   phase H: the source rows the tile's output rows reach -- from the bounds of its first and last row, at most
//            kMaxRows = 272 (33 * 8 + 1 = 265 at the supported limit) -- are resampled horizontally at the tile's 32
//            columns and written to LDS as bytes: 3 x 272 x 32 = 26 112 B.  A thread owns one column and walks rows;
//            source bytes come from aligned 32-bit words (one load serves up to 4 taps of a CHW row), single bytes only
//            where the word would cross the buffer's end.  Source rows start at any byte, in planes or interleaved.
//   phase V: a thread owns 4 consecutive pixels of one output row: per tap one 32-bit LDS read per channel, four 24-bit
//            multiplies into uint32 accumulators (sum k <= 2^22 + 17, times 255, plus 2^21 < 2^31), shift, min, normalise,
//            16-byte stores (NCHW: one per plane; channels-last: three).  64 threads also write the tile's mask bytes.
// LDS per workgroup: 26 112 + 2 x 2 176 + 2 x 256 = 30 976 B: five workgroups per CU.  Tiles above one another recompute
// the horizontal pass of the rows they share: at 720 -> 360 a tile stages 66 source rows for 64 of its own, 3 % recomputed
// (99 for 96 at 3x); neighbouring columns share source bytes (through the caches) but no arithmetic.
// Every element of x and mask is written by exactly one thread: no memset, no atomics, plain vector stores.
// The kernel itself stands in resize_body.h, shared with augment.hip: this file instantiates it without
// a crop window and without a flip -- both compile-time constants, so the code below carries none of their arithmetic.
#include "resize_body.h"

using namespace vnx;

extern "C" int vnx_resize_ingest_frames(const void* pixels, size_t pixel_bytes, const void* src_table, const void* dst_table,
                                        const void* coeffs, size_t coeff_words, int batch, int height, int width,
                                        float mean0, float mean1, float mean2, float std0, float std1, float std2,
                                        int channels_last, int interleaved, void* x, void* mask, void* hip_stream) {
  const float mean[3] = {mean0, mean1, mean2}, std[3] = {std0, std1, std2};
  return launch_resize_ingest<false>("vnx_resize_ingest_frames", pixels, pixel_bytes, src_table, dst_table, coeffs, coeff_words,
                                     batch, height, width, mean, std, channels_last, interleaved, x, mask, hip_stream);
}
