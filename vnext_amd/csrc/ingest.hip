// ingest.hip -- uint8 frames to network inputs on the device: normalise + pad + padding mask in one launch, and the per-level
// padding masks and sine positions of a padded batch in one more (vnext_amd/ops/ingest.py; include/vnext_hip.h).
//
// Both kernels read the frames' geometry from MEMORY: an int32 table with one row {byte offset of the frame's first
// plane inside `pixels`, h, w} per frame.  A captured launch therefore bakes in the batch, the padded size, the layout, mean /
// std, the level sizes and the two position tables -- and nothing of the frames: a replay reads new pixels and new sizes.
// A row that does not describe planes inside `pixels` (negative values, h > H, w > W, an end beyond pixel_bytes) is taken as
// an EMPTY frame (all padding): no read leaves the buffer whatever the table holds.  Every element of every output is written
// by exactly one thread (no memset before, no atomics); all stores are plain vector stores.
//
// Pixel pass.  A thread owns 4 consecutive pixels of a padded row, all 3 channels: value = (float(u) - mean[c]) / std[c]
// inside the frame (one IEEE subtract, one correctly rounded IEEE divide: hipcc's default, which the build does not switch
// off; contraction is off for the file), 0 outside.  NCHW: one 16-byte store per channel plane; channels-last: the 12 floats
// are 48 contiguous bytes, three 16-byte stores.  Source bytes: a frame row starts at any byte, so the 4 bytes of a group are
// taken from the two aligned 32-bit words around them (v_alignbyte) wherever both words lie inside the buffer and the group
// lies inside the row; the groups at a row's ragged end and at the buffer's ends read single bytes.  The bool mask is written
// by further workgroups of the same launch, 16 pixels (one 16-byte store) per thread; it depends on the table alone.
//
// Level pass.  For each of up to 8 levels (h_l, w_l): the level mask is torch's nearest resize of the padding mask -- source
// index min(int(floorf(dst * scale)), in - 1), scale = float(in) / out, as ATen computes it -- and the position is
// models.seqformer.sine_position of that mask, in the memory order the eager function returns ([B][h_l][w_l][C], C = 2 *
// num_pos_feats, the y half first).  The padding mask of a frame is the complement of a top-left rectangle and the source
// index is monotone, so the level mask is one too: valid rows y < vh, valid columns x < vw (found by bisection on the source
// index), and the eager chain's two cumsums have the closed form
//   y_embed(y, x) = x < vw ? min(y + 1, vh) : 0      with the column's normaliser  x < vw ? vh : 0
//   x_embed(y, x) = y < vh ? min(x + 1, vw) : 0      with the row's normaliser     y < vh ? vw : 0
// from which the kernel follows the eager chain's fp32 operations in order: (e - 0.5) / (n + 1e-6) * 2pi, / dim_t, sin | cos.
// dim_t comes from the caller (no powf here).  Where the normaliser is 0 the argument is the constant -0.5 / 1e-6 * 2pi /
// dim_t ~ -3.1e6 / dim_t, far outside the range where two sine implementations agree: those values come from the caller's
// `degenerate` table, which holds what the eager chain itself produces there.  A thread owns 4 consecutive channels of one
// position (one 16-byte store; consecutive lanes, consecutive channel groups); the thread of channel group 0 writes the
// position's mask byte.
#include "vnx_common.h"

#pragma clang fp contract(off)

namespace vnx {
namespace {

constexpr int kIngestThreads = 256;
constexpr int kIngestMaxLevels = 8;         // VNX_INGEST_MAX_LEVELS
constexpr int kIngestMaxPosFeats = 128;     // VNX_INGEST_MAX_POS_FEATS

typedef uint32_t ing_u4 __attribute__((ext_vector_type(4)));

struct FrameGeom { long long off; int h, w; };

// row `b` of the table, or the empty frame when it does not describe planes inside the buffer
__device__ __forceinline__ FrameGeom frame_geom(const int32_t* __restrict__ table, int b, int H, int W, long long pixel_bytes) {
  const int off = table[3 * b], h = table[3 * b + 1], w = table[3 * b + 2];
  const bool ok = off >= 0 && h >= 1 && w >= 1 && h <= H && w <= W && (long long)off + 3ll * h * w <= pixel_bytes;
  return ok ? FrameGeom{off, h, w} : FrameGeom{0, 0, 0};
}

struct PixelArgs {
  const unsigned char* pixels;
  long long pixel_bytes;
  const int32_t* table;
  float* x;
  unsigned char* mask;
  int B, H, W, channels_last;
  float mean[3], std[3];
  unsigned pixel_blocks;      // workgroups of the pixel part; the rest write the mask
};

__global__ __launch_bounds__(kIngestThreads) void ingest_pixels_kernel(PixelArgs a) {
  const int H = a.H, W = a.W;
  if (blockIdx.x >= a.pixel_blocks) {      // ---- the mask: 16 pixels per thread ----
    const long long g = (long long)(blockIdx.x - a.pixel_blocks) * kIngestThreads + threadIdx.x;
    const int per_row = W >> 4;
    if (g >= (long long)a.B * H * per_row) return;
    const int xg = int(g % per_row);
    const long long row = g / per_row;
    const int y = int(row % H), b = int(row / H);
    const FrameGeom f = frame_geom(a.table, b, H, W, a.pixel_bytes);
    const int x0 = xg << 4;
    ing_u4 v;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      uint32_t word = 0;
#pragma unroll
      for (int j = 0; j < 4; ++j) word |= uint32_t(y >= f.h || x0 + 4 * k + j >= f.w) << (8 * j);
      v[k] = word;
    }
    *reinterpret_cast<ing_u4*>(a.mask + (size_t(row) * W + x0)) = v;
    return;
  }
  // ---- the pixels: 4 per thread, 3 channels ----
  const long long g = (long long)blockIdx.x * kIngestThreads + threadIdx.x;
  const int per_row = W >> 2;
  if (g >= (long long)a.B * H * per_row) return;
  const int xg = int(g % per_row);
  const long long row = g / per_row;
  const int y = int(row % H), b = int(row / H);
  const FrameGeom f = frame_geom(a.table, b, H, W, a.pixel_bytes);
  const int x0 = xg << 2;
  float val[3][4];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
#pragma unroll
    for (int j = 0; j < 4; ++j) val[c][j] = 0.f;
  }
  if (y < f.h && x0 < f.w) {
    const long long plane = (long long)f.h * f.w;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const long long at = f.off + c * plane + (long long)y * f.w + x0;      // first byte of the group, inside the buffer
      const long long lo = at & ~3ll;
      const int shift = int(at & 3);
      uint32_t bytes;
      if (x0 + 4 <= f.w && lo + 8 <= a.pixel_bytes) {      // both aligned words inside the buffer (`pixels` is 4-byte aligned)
        const uint32_t w0 = *reinterpret_cast<const uint32_t*>(a.pixels + lo);
        const uint32_t w1 = *reinterpret_cast<const uint32_t*>(a.pixels + lo + 4);
        bytes = __builtin_amdgcn_alignbyte(w1, w0, uint32_t(shift));
      } else {                                             // a row's ragged end, the buffer's last bytes
        bytes = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (x0 + j < f.w) bytes |= uint32_t(a.pixels[at + j]) << (8 * j);
      }
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (x0 + j < f.w) val[c][j] = (float((bytes >> (8 * j)) & 0xffu) - a.mean[c]) / a.std[c];
    }
  }
  if (a.channels_last) {
    float* out = a.x + (size_t(row) * W + x0) * 3;
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

struct LevelArgs {
  const int32_t* table;
  const float* dim_t;           // [npf]
  const float* degenerate;      // [npf]: sin (even) / cos (odd) where the normaliser is 0
  unsigned char* mask[kIngestMaxLevels];      // [B][h][w]
  float* pos[kIngestMaxLevels];               // [B][h][w][2 npf]
  int h[kIngestMaxLevels], w[kIngestMaxLevels];
  float scale_h[kIngestMaxLevels], scale_w[kIngestMaxLevels];      // float(H) / h, float(W) / w
  unsigned first_block[kIngestMaxLevels + 1];
  int levels, B, H, W, npf;
};

// ATen's nearest source index
__device__ __forceinline__ int nearest_src(int dst, float scale, int in) {
  const int s = int(floorf(float(dst) * scale));
  return s < in - 1 ? s : in - 1;
}

// destination indices whose source index lies below `valid`: the source index is monotone, so they are 0 .. count - 1
__device__ __forceinline__ int valid_count(int out, float scale, int in, int valid) {
  int lo = 0, hi = out;      // the count lies in [lo, hi]
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (nearest_src(mid, scale, in) < valid) lo = mid + 1; else hi = mid;
  }
  return lo;
}

__global__ __launch_bounds__(kIngestThreads) void ingest_levels_kernel(LevelArgs a) {
  int l = 0;
  while (l + 1 < a.levels && blockIdx.x >= a.first_block[l + 1]) ++l;      // workgroup-uniform
  const int h = a.h[l], w = a.w[l], npf = a.npf;
  const int groups = npf >> 1;                                             // 4-channel groups of a position (2 npf / 4)
  const long long g = (long long)(blockIdx.x - a.first_block[l]) * kIngestThreads + threadIdx.x;
  if (g >= (long long)a.B * h * w * groups) return;
  const int cg = int(g % groups);
  const long long p = g / groups;      // position (b, y, x)
  const int x = int(p % w);
  const long long r = p / w;
  const int y = int(r % h), b = int(r / h);
  const FrameGeom f = frame_geom(a.table, b, a.H, a.W, 0x7fffffffffffffffll);      // (the geometry alone: no pixel is read here)
  const int vh = valid_count(h, a.scale_h[l], a.H, f.h), vw = valid_count(w, a.scale_w[l], a.W, f.w);
  if (cg == 0) a.mask[l][p] = (unsigned char)(y >= vh || x >= vw);
  const int c0 = cg << 2;
  const bool x_half = c0 >= npf;      // channels [0, npf): pos_y, [npf, 2 npf): pos_x
  const int j0 = x_half ? c0 - npf : c0;
  // the coordinate of this half, and the normaliser of its column (pos_y) / row (pos_x)
  const int embed = x_half ? (y < vh ? (x + 1 < vw ? x + 1 : vw) : 0) : (x < vw ? (y + 1 < vh ? y + 1 : vh) : 0);
  const int norm = x_half ? (y < vh ? vw : 0) : (x < vw ? vh : 0);
  vnx_f4 out;
  if (norm == 0) {
    out = *reinterpret_cast<const vnx_f4*>(a.degenerate + j0);
  } else {
    const float e = (float(embed) - 0.5f) / (float(norm) + 1e-6f) * 6.283185307179586f;
    const vnx_f4 d = *reinterpret_cast<const vnx_f4*>(a.dim_t + j0);
    out = vnx_f4{sinf(e / d.x), cosf(e / d.y), sinf(e / d.z), cosf(e / d.w)};
  }
  *reinterpret_cast<vnx_f4*>(a.pos[l] + size_t(p) * (2 * npf) + c0) = out;
}

}  // namespace
}  // namespace vnx

using namespace vnx;

extern "C" int vnx_ingest_frames(const void* pixels, size_t pixel_bytes, const void* table, int batch, int height, int width,
                                 float mean0, float mean1, float mean2, float std0, float std1, float std2,
                                 int channels_last, void* x, void* mask, void* hip_stream) {
  const char* fn = "vnx_ingest_frames";
  if (batch < 0 || height < 32 || width < 32 || height % 32 != 0 || width % 32 != 0) {
    set_error("%s: bad sizes (batch %d, padded %d x %d: multiples of 32)", fn, batch, height, width);
    return VNX_ERR_INVALID_ARGUMENT;
  }
  if (batch == 0) return VNX_OK;
  if (!pixels || !table || !x || !mask) {
    set_error("%s: null pointer argument", fn);
    return VNX_ERR_INVALID_ARGUMENT;
  }
  if ((reinterpret_cast<uintptr_t>(pixels) & 3) != 0 || (reinterpret_cast<uintptr_t>(table) & 3) != 0 ||
      (reinterpret_cast<uintptr_t>(x) & 15) != 0 || (reinterpret_cast<uintptr_t>(mask) & 15) != 0) {
    set_error("%s: pixels and table must be 4-byte aligned, x and mask 16-byte aligned", fn);
    return VNX_ERR_INVALID_ARGUMENT;
  }
  if (pixel_bytes > size_t(0x7fffffff)) {      // the table's offsets are int32
    set_error("%s: %zu bytes of pixels: the table addresses 2^31 - 1 at most", fn, pixel_bytes);
    return VNX_ERR_UNSUPPORTED;
  }
  const long long groups = (long long)batch * height * (width / 4), mask_groups = (long long)batch * height * (width / 16);
  const long long pb = (groups + kIngestThreads - 1) / kIngestThreads, mb = (mask_groups + kIngestThreads - 1) / kIngestThreads;
  if (pb + mb > 0x7fffffffll) {
    set_error("%s: %d frames of %d x %d are more than one launch addresses", fn, batch, height, width);
    return VNX_ERR_UNSUPPORTED;
  }
  PixelArgs a;
  a.pixels = (const unsigned char*)pixels;
  a.pixel_bytes = (long long)pixel_bytes;
  a.table = (const int32_t*)table;
  a.x = (float*)x;
  a.mask = (unsigned char*)mask;
  a.B = batch; a.H = height; a.W = width; a.channels_last = channels_last != 0;
  a.mean[0] = mean0; a.mean[1] = mean1; a.mean[2] = mean2;
  a.std[0] = std0; a.std[1] = std1; a.std[2] = std2;
  a.pixel_blocks = unsigned(pb);
  hipLaunchKernelGGL(ingest_pixels_kernel, dim3(unsigned(pb + mb)), dim3(kIngestThreads), 0, (hipStream_t)hip_stream, a);
  return check_launch(fn);
}

extern "C" int vnx_ingest_levels(const void* table, int batch, int height, int width, int num_levels, const int* level_sizes,
                                 int num_pos_feats, const void* dim_t, const void* degenerate, void* const* masks,
                                 void* const* positions, void* hip_stream) {
  const char* fn = "vnx_ingest_levels";
  if (batch < 0 || height < 1 || width < 1 || num_levels < 0 || num_pos_feats < 1) {
    set_error("%s: bad sizes (batch %d, padded %d x %d, %d levels, %d position features)", fn, batch, height, width,
              num_levels, num_pos_feats);
    return VNX_ERR_INVALID_ARGUMENT;
  }
  if (num_levels > kIngestMaxLevels || num_pos_feats > kIngestMaxPosFeats || num_pos_feats % 4 != 0) {
    set_error("%s: %d levels, %d position features: at most %d levels, position features a multiple of 4 up to %d", fn,
              num_levels, num_pos_feats, kIngestMaxLevels, kIngestMaxPosFeats);
    return VNX_ERR_UNSUPPORTED;
  }
  if (batch == 0 || num_levels == 0) return VNX_OK;
  if (!table || !level_sizes || !dim_t || !degenerate || !masks || !positions) {
    set_error("%s: null pointer argument", fn);
    return VNX_ERR_INVALID_ARGUMENT;
  }
  if ((reinterpret_cast<uintptr_t>(table) & 3) != 0 || (reinterpret_cast<uintptr_t>(dim_t) & 15) != 0 ||
      (reinterpret_cast<uintptr_t>(degenerate) & 15) != 0) {
    set_error("%s: table must be 4-byte aligned, dim_t and degenerate 16-byte aligned", fn);
    return VNX_ERR_INVALID_ARGUMENT;
  }
  LevelArgs a;
  a.table = (const int32_t*)table;
  a.dim_t = (const float*)dim_t;
  a.degenerate = (const float*)degenerate;
  a.levels = num_levels; a.B = batch; a.H = height; a.W = width; a.npf = num_pos_feats;
  long long blocks = 0;
  for (int l = 0; l < kIngestMaxLevels; ++l) {
    a.first_block[l] = unsigned(blocks);
    if (l >= num_levels) {
      a.mask[l] = nullptr; a.pos[l] = nullptr; a.h[l] = a.w[l] = 0; a.scale_h[l] = a.scale_w[l] = 0.f;
      continue;
    }
    const int h = level_sizes[2 * l], w = level_sizes[2 * l + 1];
    if (h < 1 || w < 1 || h > height || w > width) {
      set_error("%s: level %d is %d x %d: inside 1 x 1 .. %d x %d", fn, l, h, w, height, width);
      return VNX_ERR_INVALID_ARGUMENT;
    }
    if (!masks[l] || !positions[l] || (reinterpret_cast<uintptr_t>(positions[l]) & 15) != 0) {
      set_error("%s: level %d: null mask or position pointer, or positions not 16-byte aligned", fn, l);
      return VNX_ERR_INVALID_ARGUMENT;
    }
    a.mask[l] = (unsigned char*)masks[l];
    a.pos[l] = (float*)positions[l];
    a.h[l] = h; a.w[l] = w;
    a.scale_h[l] = float(height) / float(h);      // compute_scales_value<float>: (float)input / output
    a.scale_w[l] = float(width) / float(w);
    const long long threads = (long long)batch * h * w * (num_pos_feats / 2);
    blocks += (threads + kIngestThreads - 1) / kIngestThreads;
    if (blocks > 0x7fffffffll) {
      set_error("%s: %d frames, level %d of %d x %d: more than one launch addresses", fn, batch, l, h, w);
      return VNX_ERR_UNSUPPORTED;
    }
  }
  a.first_block[kIngestMaxLevels] = unsigned(blocks);
  hipLaunchKernelGGL(ingest_levels_kernel, dim3(unsigned(blocks)), dim3(kIngestThreads), 0, (hipStream_t)hip_stream, a);
  return check_launch(fn);
}
