// mask_dense.hip -- the thresholded result masks at the output size, formed from the fp32 mask logits in one launch (the
// dense route of `model(inputs)`; the RLE route is mask_rle.hip).  Host specification: vnext_amd/ops/mask_dense.py.
//
// A pixel's value is mask_sample.h's, the code mask_rle.hip runs: ATen's nearest index on the cropped grid, ONE
// align_corners=False bilinear sample of the logit map there, bit = value > 0.  Nothing between the logits and the bits is
// stored: no upsampled map, no sigmoid.  No atomics: the output is a function of the input alone.
//
// The walk is row-major over the M * oh output rows.  A task is kDenseRows consecutive rows x one tile of kDenseTile
// columns; a workgroup takes tasks in a grid-stride loop (64-bit counts: no grid dimension bounds M * oh), and per task
//   1. stages the tile's column taps {first source column, weight of the next} in LDS, once for all its rows;
//   2. gives each wave a row at a time.  The row's tap is wave-uniform and formed once per row; a lane then combines it
//      with the staged column taps of its pixels.
// VNX_MASK_DENSE_U8, [M][oh][ow] bytes of 0 / 1: a row segment starts at any byte address.  Piece k of a segment is the
//   ALIGNED 8 bytes at (address & ~7) + 8 k; a lane forms the 8 pixels of its piece and stores it whole where the piece
//   lies inside the segment, byte by byte where the segment only touches it -- the piece's other bytes belong to the
//   neighbouring tile, row or to memory that is not the output's (vnx_resize_window_bytes stores the same way).
// VNX_MASK_DENSE_BITS, [M][oh][pitch], pitch = 8 * ceil(ow / 64): pixel x is bit x & 7 of byte x >> 3.  One __ballot is
//   the word of 64 pixels (a pixel at or past ow votes 0: the padding is zero); lane j keeps word j of the tile and the
//   wave stores the row's words of the tile in one instruction, 8 bytes per lane.
// Every byte of the output is written, none outside it.
#include "mask_sample.h"

namespace vnx {

constexpr int kDenseThreads = 256;
constexpr int kDenseWaves = kDenseThreads / 64;
constexpr int kDenseTile = 2048;             // columns per task: 16 KiB of taps; 32 ballot words
constexpr int kDenseRows = 32;               // rows per task: 8 per wave
constexpr int64_t kDenseMaxBlocks = 1 << 20;

struct DenseArgs {
  const float* logits;
  unsigned char* out;
  MaskSample s;
  int oh, ow;
  int tiles;           // ceil(ow / kDenseTile)
  int64_t rows;        // M * oh
  int64_t tasks;       // tiles * ceil(rows / kDenseRows)
  int64_t pitch;       // bytes per output row: ow, or 8 * ceil(ow / 64)
};

template <int FORMAT>
__global__ void __launch_bounds__(kDenseThreads) mask_dense_kernel(DenseArgs a) {
  __shared__ MaskTap s_tap[kDenseTile];
  const int t = threadIdx.x, lane = t & 63;
  const int wv = __builtin_amdgcn_readfirstlane(t >> 6);
  const int h = a.s.h, w = a.s.w;
  for (int64_t task = blockIdx.x; task < a.tasks; task += gridDim.x) {
    const int tile = int(task % a.tiles);
    const int64_t row0 = task / a.tiles * kDenseRows;
    const int c0 = tile * kDenseTile, cols = min(kDenseTile, a.ow - c0);      // the tile's columns [c0, c0 + cols), cols >= 1
    for (int c = t; c < cols; c += kDenseThreads) {
      MaskTap tx = mask_tap(c0 + c, a.s.nx, a.s.iw, a.s.rx);
      tx.i0 = min(tx.i0, w - 1);             // (never past the map, whatever fp32 made of a huge width)
      s_tap[c] = tx;
    }
    __syncthreads();
    const int nrows = int(min(int64_t(kDenseRows), a.rows - row0));
    int64_t m = row0 / a.oh;
    const int y0 = int(row0 - m * a.oh);
    for (int i = wv; i < nrows; i += kDenseWaves) {
      int y = y0 + i;
      int64_t mi = m;
      while (y >= a.oh) { y -= a.oh; ++mi; }
      const float* map = a.logits + mi * h * w;
      MaskTap ty = mask_tap(y, a.s.ny, a.s.ih, a.s.ry);
      ty.i0 = min(ty.i0, h - 1);
      unsigned char* row = a.out + (row0 + i) * a.pitch;
      if constexpr (FORMAT == VNX_MASK_DENSE_U8) {
        unsigned char* seg = row + c0;
        const int lead = int(reinterpret_cast<uintptr_t>(seg) & 7);
        const int pieces = (lead + cols + 7) >> 3;
        for (int k = lane; k < pieces; k += 64) {
          const int lo = 8 * k - lead;                         // the piece is bytes [lo, lo + 8) of the segment
          uint64_t v = 0;
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            const int c = min(max(lo + j, 0), cols - 1);       // (a byte outside the segment is formed and not stored)
            v |= uint64_t(mask_bit(map, h, w, ty, s_tap[c])) << (8 * j);
          }
          if (lo >= 0 && lo + 8 <= cols) {
            *reinterpret_cast<uint64_t*>(seg + lo) = v;
          } else {
            for (int j = max(lo, 0); j < min(lo + 8, cols); ++j) seg[j] = (unsigned char)(v >> (8 * (j - lo)));
          }
        }
      } else {
        const int words = int(min(int64_t(kDenseTile / 64), a.pitch / 8 - tile * (kDenseTile / 64)));
        uint64_t mine = 0;
        for (int k = 0; k < words; ++k) {
          const int c = 64 * k + lane;
          const bool bit = mask_bit(map, h, w, ty, s_tap[min(c, cols - 1)]) && c < cols;
          const uint64_t word = __ballot(bit);
          if (lane == k) mine = word;
        }
        if (lane < words) reinterpret_cast<uint64_t*>(row)[tile * (kDenseTile / 64) + lane] = mine;
      }
    }
    __syncthreads();                                           // before the next task's taps overwrite these
  }
}

}  // namespace vnx

using namespace vnx;

extern "C" int vnx_mask_dense(int format, const void* logits, int masks, int height, int width, int stride,
                              int image_height, int image_width, int out_height, int out_width, void* out,
                              long long out_bytes, void* hip_stream) {
  const char* fn = "vnx_mask_dense";
  if (format != VNX_MASK_DENSE_U8 && format != VNX_MASK_DENSE_BITS) {
    set_error("%s: unknown format %d", fn, format);
    return VNX_ERR_INVALID_ARGUMENT;
  }
  if (masks < 0 || out_height < 1 || out_width < 1 || out_bytes < 0) {
    set_error("%s: bad sizes (masks %d, out %d x %d, out_bytes %lld)", fn, masks, out_height, out_width, out_bytes);
    return VNX_ERR_INVALID_ARGUMENT;
  }
  if (height < 1 || width < 1 || stride < 1 || image_height < 1 || image_width < 1 ||
      int64_t(image_height) > int64_t(height) * stride || int64_t(image_width) > int64_t(width) * stride) {
    set_error("%s: bad sizes (map %d x %d, stride %d, image %d x %d)", fn, height, width, stride, image_height,
              image_width);
    return VNX_ERR_INVALID_ARGUMENT;
  }
  if (int64_t(height) * width >= (int64_t(1) << 31)) {
    set_error("%s: map %d x %d has 2^31 elements or more", fn, height, width);
    return VNX_ERR_UNSUPPORTED;
  }
  if (masks == 0) return VNX_OK;
  if (!logits || !out) {
    set_error("%s: null pointer argument", fn);
    return VNX_ERR_INVALID_ARGUMENT;
  }
  if ((reinterpret_cast<uintptr_t>(logits) & 3) != 0) {
    set_error("%s: logits must be 4-byte aligned", fn);
    return VNX_ERR_INVALID_ARGUMENT;
  }
  if (format == VNX_MASK_DENSE_BITS && (reinterpret_cast<uintptr_t>(out) & 7) != 0) {
    set_error("%s: out must be 8-byte aligned for VNX_MASK_DENSE_BITS", fn);
    return VNX_ERR_INVALID_ARGUMENT;
  }
  DenseArgs a;
  a.logits = (const float*)logits;
  a.out = (unsigned char*)out;
  a.s = mask_sample(height, width, stride, image_height, image_width, out_height, out_width);
  a.oh = out_height; a.ow = out_width;
  a.tiles = (out_width + kDenseTile - 1) / kDenseTile;
  a.rows = int64_t(masks) * out_height;                          // < 2^62
  a.pitch = format == VNX_MASK_DENSE_U8 ? int64_t(out_width) : 8 * ((int64_t(out_width) + 63) / 64);
  if ((unsigned __int128)a.rows * (unsigned __int128)a.pitch > (unsigned __int128)out_bytes) {
    set_error("%s: out_bytes %lld: less than the %lld rows of %lld bytes", fn, out_bytes, (long long)a.rows,
              (long long)a.pitch);
    return VNX_ERR_INVALID_ARGUMENT;
  }
  a.tasks = a.tiles * ((a.rows + kDenseRows - 1) / kDenseRows);
  const dim3 grid{uint32_t(a.tasks < kDenseMaxBlocks ? a.tasks : kDenseMaxBlocks), 1, 1}, block{kDenseThreads, 1, 1};
  if (format == VNX_MASK_DENSE_U8)
    hipLaunchKernelGGL(mask_dense_kernel<VNX_MASK_DENSE_U8>, grid, block, 0, (hipStream_t)hip_stream, a);
  else
    hipLaunchKernelGGL(mask_dense_kernel<VNX_MASK_DENSE_BITS>, grid, block, 0, (hipStream_t)hip_stream, a);
  return check_launch(fn);
}
