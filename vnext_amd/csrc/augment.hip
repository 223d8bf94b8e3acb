// augment.hip -- training-time augmentation on the device: crop, resize and horizontal flip of uint8 source frames into the
// network's (x, mask), and the same geometry applied to the ground-truth masks straight from their COCO run lengths, with
// the masks' boxes (vnext_amd/ops/augment.py; include/vnext_hip.h).
//
// vnx_augment_frames is the resize + ingest kernel of resize.hip instantiated WITH a crop window and a flip flag
// (resize_body.h: one copy of the device code).  A source row is {byte offset, h, w, x0, y0, cw, ch, flip}; the
// coefficient tables are those of (cw -> nw) and (ch -> nh); the row pitch stays w.  A row with the full window and no flip
// gives what vnx_resize_ingest_frames gives, bit for bit.
//
// vnx_resize_window_bytes is the third instantiation: the first resample of the COCO pre-training
// chain flip -> resize -> crop -> resize.  It resizes a frame to (h1, w1) but computes only the crop window of the result
// and stores it as bytes, in the frame's layout, into a slot of the SAME pixel buffer; vnx_augment_frames then reads that
// slot as a source frame.  A row is {src byte offset, h, w, h1, w1, x0, y0, cw, ch, dst byte offset, bounds / weights /
// ksize of (w -> w1), of (h -> h1)}.  A malformed row (the window outside (h1, w1) or the padded size, either byte range
// outside the buffer or the two overlapping, ksize beyond the limit) leaves its slot untouched.
//
// vnx_augment_frames_color is vnx_augment_frames with detectron2's RandomBrightness, RandomContrast and
// RandomSaturation on the resampled bytes, per frame, the weights read from a colour table in device memory.  Brightness and
// saturation are pointwise: the kColor = 1 instantiation applies them between phase V and the normalisation, in the one
// launch.  Contrast blends with the mean of the whole frame after brightness: the kColor = 2 instantiation stores the
// post-brightness bytes and every tile's integer sum behind the frames in the pixel buffer, and color_finish_kernel (below)
// folds a frame's sums, divides once in double and finishes: two launches, no atomics, no memset, bit-identical run to run.
// The float64 expressions are numpy's, rounding for rounding: resize_body.h switches contraction OFF for the whole file
// (`#pragma clang fp contract(off)`), this one included.
//
// vnx_augment_masks.  A ground-truth mask arrives as the END POSITIONS of its COCO runs (the cumulative sums of the counts;
// column-major, p = x * h + y; runs of zeros and ones alternate, zeros first).  The value of source pixel p is the parity of
// the number of ends <= p -- an upper bound by binary search; zero-length runs need no special case.  Output pixel (y, x) of
// a mask reads source pixel (y0 + ytab[y], x0 + xtab[flip ? nw - 1 - x : x]) with Pillow's NEAREST index tables of
// (ch -> nh) and (cw -> nw), made by the host (Pillow accumulates them in double; the closed form differs) and carried in
// `coeffs` behind the bilinear tables.  No mask exists at source resolution anywhere.
//   masks kernel: one workgroup of 256 threads per (mask, 32 x 32 tile of the padded size).  The tile's source columns
//     [xmin, xmax] bound the runs it can meet: ends in [xmin * h, (xmax + 1) * h).  Thread 0 finds that slice with two
//     searches; when it has at most kSlice ends it is copied to LDS and the per-pixel searches run there, otherwise they run
//     on the slice in memory.  A thread owns one column of the tile and 4 of its rows: byte stores, coalesced across lanes
//     (a mask's row pitch is nw: no alignment to build wider stores on).  The tile's box {min x, min y, max x, max y} is
//     reduced over the wave by shuffles, over the 4 waves through LDS, and written to the workspace: a slot per (mask, tile),
//     every slot written -- no memset, no atomics.
//   box kernel: one wave per mask folds its tiles' slots in a fixed order -> fp32 {min x, min y, max x + 1, max y + 1}
//     (BitMasks.get_bounding_boxes) and the `nonempty` byte; an empty mask gives zeros.  Bit-identical run to run.
// A mask row that names no frame, a frame whose geometry is malformed or an output range outside `masks` writes nothing and
// gives a zero box; runs outside `ends`, or whose last end is not h * w, are an EMPTY mask (zeros written).  End values are
// only compared, never used as addresses, and every table entry is clamped: no read leaves a buffer whatever they hold.
#include "resize_body.h"

namespace vnx {
namespace {

constexpr int kMaskThreads = 256;
constexpr int kSlice = 2048;               // ends of a tile's slice held in LDS (8 KiB)
constexpr int kMaskRowWords = 4;           // {ends offset, n_runs, frame index, byte offset of the output}
constexpr int kEmptyMin = 0x7fffffff;

struct MaskArgs {
  const int32_t* ends;
  long long n_ends;
  const int32_t* rows;
  const int32_t* src_table;
  const int32_t* dst_table;
  const int32_t* coeffs;
  long long coeff_words;
  unsigned char* out;
  long long out_bytes;
  int32_t* partial;                        // [n_masks][tiles_y * tiles_x][4]
  int n_masks, n_frames, H, W;
};

struct MaskGeom {
  int h, w, x0, y0, cw, ch, flip, nh, nw, xtab, ytab;      // nh == 0: nothing to write
};

// what the masks need of frame `f`: the frame's size, the window, the target and the two nearest tables inside `coeffs`
__device__ __forceinline__ MaskGeom mask_geom(const MaskArgs& a, int f) {
  MaskGeom g{};
  if (f < 0 || f >= a.n_frames) return g;
  const int32_t* s = a.src_table + kAugSrcWords * size_t(f);
  g.h = s[1]; g.w = s[2]; g.x0 = s[3]; g.y0 = s[4]; g.cw = s[5]; g.ch = s[6]; g.flip = s[7] != 0;
  g.nh = a.dst_table[3 * f + 1]; g.nw = a.dst_table[3 * f + 2];
  const int32_t* row = a.coeffs + kAugCoeffWords * size_t(f);
  g.xtab = row[6]; g.ytab = row[7];
  const bool ok = g.h >= 1 && g.w >= 1 && (long long)g.h * g.w <= 0x7fffffffll && g.x0 >= 0 && g.y0 >= 0 && g.cw >= 1 &&
                  g.ch >= 1 && g.cw <= g.w && g.ch <= g.h && g.x0 <= g.w - g.cw && g.y0 <= g.h - g.ch && g.nh >= 1 &&
                  g.nw >= 1 && g.nh <= a.H && g.nw <= a.W && g.xtab >= 0 && g.ytab >= 0 &&
                  (long long)g.xtab + g.nw <= a.coeff_words && (long long)g.ytab + g.nh <= a.coeff_words;
  if (!ok) g.nh = g.nw = 0;
  return g;
}

// the number of e[0 .. n) that are <= p (e ascending; on anything else still an index in [0, n])
template <typename Ptr>
__device__ __forceinline__ int upper_bound(Ptr e, int n, int p) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (e[mid] <= p) lo = mid + 1; else hi = mid;
  }
  return lo;
}

__device__ __forceinline__ int wave_min_i(int v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = min(v, __shfl_xor(v, off, 64));
  return v;
}
__device__ __forceinline__ int wave_max_i(int v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = max(v, __shfl_xor(v, off, 64));
  return v;
}

__global__ __launch_bounds__(kMaskThreads) void augment_masks_kernel(MaskArgs a) {
  __shared__ int32_t slice[kSlice];
  __shared__ int xs[kTile], ys[kTile];
  __shared__ int range[2];
  __shared__ int red[kMaskThreads / kWave][4];

  const int tid = threadIdx.x;
  const int tiles_x = a.W / kTile, tiles_y = a.H / kTile;
  const int tile = blockIdx.x % (tiles_x * tiles_y), m = blockIdx.x / (tiles_x * tiles_y);
  const int ox0 = (tile % tiles_x) * kTile, oy0 = (tile / tiles_x) * kTile;
  int32_t* slot = a.partial + 4 * size_t(blockIdx.x);

  // everything down to the searches is workgroup-uniform
  const int32_t* row = a.rows + kMaskRowWords * size_t(m);
  const int e_off = row[0], n_runs = row[1], out_off = row[3];
  const MaskGeom g = mask_geom(a, row[2]);
  const bool writes = g.nh > 0 && out_off >= 0 && (long long)out_off + (long long)g.nh * g.nw <= a.out_bytes;
  if (!writes || oy0 >= g.nh || ox0 >= g.nw) {      // no pixel of this mask in the tile: the empty box
    if (tid == 0) { slot[0] = kEmptyMin; slot[1] = kEmptyMin; slot[2] = -1; slot[3] = -1; }
    return;
  }
  const int rows_out = min(kTile, g.nh - oy0), cols_out = min(kTile, g.nw - ox0);
  const int32_t* e = a.ends + e_off;
  const bool runs_ok = e_off >= 0 && n_runs >= 1 && (long long)e_off + n_runs <= a.n_ends &&
                       e[n_runs - 1] == g.h * g.w;      // (h * w <= 2^31 - 1 was checked)

  // ---- the tile's source columns and rows ----
  if (tid < kTile) {
    int v = 0;
    if (tid < cols_out) {
      const int x = ox0 + tid;
      v = g.x0 + clampi(a.coeffs[g.xtab + (g.flip ? g.nw - 1 - x : x)], 0, g.cw - 1);
    }
    xs[tid] = v;
  } else if (tid < 2 * kTile) {
    const int r = tid - kTile;
    ys[r] = r < rows_out ? g.y0 + clampi(a.coeffs[g.ytab + oy0 + r], 0, g.ch - 1) : 0;
  }
  __syncthreads();
  // ---- the slice of ends the tile's columns can meet ----
  if (tid == 0) {
    int lo = 0, hi = 0;
    if (runs_ok) {
      int xmin = xs[0], xmax = xs[0];
      for (int i = 1; i < cols_out; ++i) { xmin = min(xmin, xs[i]); xmax = max(xmax, xs[i]); }
      lo = upper_bound(e, n_runs, xmin * g.h - 1);            // ends < the first position of column xmin
      hi = max(lo, upper_bound(e, n_runs, xmax * g.h + g.h - 1));
    }
    range[0] = lo; range[1] = hi;
  }
  __syncthreads();
  const int lo = range[0], n_slice = range[1] - lo;
  const bool in_lds = n_slice <= kSlice;
  if (in_lds) {
    for (int i = tid; i < n_slice; i += kMaskThreads) slice[i] = e[lo + i];
    __syncthreads();
  }

  // ---- the pixels: column tid % 32, rows tid / 32 + 8 k ----
  const int col = tid & (kTile - 1), sub = tid >> 5;
  int bx0 = kEmptyMin, by0 = kEmptyMin, bx1 = -1, by1 = -1;
  if (col < cols_out) {
    const int x = ox0 + col, base = xs[col] * g.h;
    unsigned char* out = a.out + out_off;
    for (int r = sub; r < rows_out; r += kMaskThreads / kTile) {
      const int y = oy0 + r;
      // ends <= p: the `lo` before the slice and those inside it (malformed runs: lo = 0 and an empty slice: the value 0)
      const int p = base + ys[r];
      const int v = (lo + (in_lds ? upper_bound(slice, n_slice, p) : upper_bound(e + lo, n_slice, p))) & 1;
      out[(long long)y * g.nw + x] = (unsigned char)v;
      if (v) { bx0 = min(bx0, x); bx1 = max(bx1, x); by0 = min(by0, y); by1 = max(by1, y); }
    }
  }
  // ---- the tile's box ----
  bx0 = wave_min_i(bx0); by0 = wave_min_i(by0); bx1 = wave_max_i(bx1); by1 = wave_max_i(by1);
  if ((tid & (kWave - 1)) == 0) {
    int* r = red[tid / kWave];
    r[0] = bx0; r[1] = by0; r[2] = bx1; r[3] = by1;
  }
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < kMaskThreads / kWave; ++w) {
      bx0 = min(bx0, red[w][0]); by0 = min(by0, red[w][1]); bx1 = max(bx1, red[w][2]); by1 = max(by1, red[w][3]);
    }
    slot[0] = bx0; slot[1] = by0; slot[2] = bx1; slot[3] = by1;
  }
}

// one wave per mask: fold the tiles' boxes
__global__ __launch_bounds__(kWave) void augment_boxes_kernel(const int32_t* __restrict__ partial, int tiles, float* boxes,
                                                              unsigned char* nonempty) {
  const int m = blockIdx.x, lane = threadIdx.x;
  int bx0 = kEmptyMin, by0 = kEmptyMin, bx1 = -1, by1 = -1;
  for (int t = lane; t < tiles; t += kWave) {
    const int32_t* s = partial + 4 * (size_t(m) * tiles + t);
    bx0 = min(bx0, s[0]); by0 = min(by0, s[1]); bx1 = max(bx1, s[2]); by1 = max(by1, s[3]);
  }
  bx0 = wave_min_i(bx0); by0 = wave_min_i(by0); bx1 = wave_max_i(bx1); by1 = wave_max_i(by1);
  if (lane == 0) {
    const bool any = bx1 >= 0;
    *reinterpret_cast<vnx_f4*>(boxes + 4 * size_t(m)) =
        any ? vnx_f4{float(bx0), float(by0), float(bx1 + 1), float(by1 + 1)} : vnx_f4{0.f, 0.f, 0.f, 0.f};
    nonempty[m] = any ? 1 : 0;
  }
}

// vnx_resize_window_bytes: what it checks before it launches, and the launch (the kBytes instantiation)
inline int launch_resize_window_bytes(const char* fn, void* pixels, size_t pixel_bytes, const void* win_table,
                                      const void* coeffs, size_t coeff_words, int batch, int height, int width,
                                      int interleaved, void* hip_stream) {
  if (batch < 0 || height < 32 || width < 32 || height % 32 != 0 || width % 32 != 0) {
    set_error("%s: bad sizes (batch %d, padded %d x %d: multiples of 32)", fn, batch, height, width);
    return VNX_ERR_INVALID_ARGUMENT;
  }
  if (batch == 0) return VNX_OK;
  if (!pixels || !win_table || !coeffs) {
    set_error("%s: null pointer argument", fn);
    return VNX_ERR_INVALID_ARGUMENT;
  }
  if (((reinterpret_cast<uintptr_t>(pixels) | reinterpret_cast<uintptr_t>(win_table) | reinterpret_cast<uintptr_t>(coeffs)) & 3) != 0) {
    set_error("%s: pixels, the table and coeffs must be 4-byte aligned", fn);
    return VNX_ERR_INVALID_ARGUMENT;
  }
  if (pixel_bytes > size_t(0x7fffffff) || coeff_words > size_t(0x7fffffff)) {      // the table's offsets are int32
    set_error("%s: %zu bytes of pixels, %zu words of coefficients: the table addresses 2^31 - 1 at most", fn, pixel_bytes,
              coeff_words);
    return VNX_ERR_UNSUPPORTED;
  }
  const long long blocks = (long long)batch * (height / kTile) * (width / kTile);
  if (blocks > 0x7fffffffll) {
    set_error("%s: %d frames of %d x %d are more than one launch addresses", fn, batch, height, width);
    return VNX_ERR_UNSUPPORTED;
  }
  ResizeArgs a{};
  a.pixels = (const unsigned char*)pixels;
  a.pixel_bytes = (long long)pixel_bytes;
  a.src_table = (const int32_t*)win_table;
  a.coeffs = (const int32_t*)coeffs;
  a.coeff_words = (long long)coeff_words;
  a.mask = (unsigned char*)pixels;      // the stores go into the pixel buffer
  a.B = batch; a.H = height; a.W = width; a.interleaved = interleaved != 0;
  hipLaunchKernelGGL((resize_ingest_kernel<false, true>), dim3(unsigned(blocks)), dim3(kResizeThreads), 0,
                     (hipStream_t)hip_stream, a);
  return check_launch(fn);
}

// ---- colour ----
// The second of two launches when contrast is on: the grid and the tiles of the frame kernel.  A workgroup folds ITS frame's
// tile sums (integers: any order gives the same total; the order here is fixed all the same) into the mean of the frame's
// own nh * nw * 3 bytes -- one division, in double -- then takes its tile's post-brightness bytes through contrast and
// saturation and on through the frame kernel's normalisation, padding and mask.
__global__ __launch_bounds__(kResizeThreads) void color_finish_kernel(ResizeArgs a) {
  __shared__ unsigned long long part[kResizeThreads / kWave];
  const int H = a.H, W = a.W, tid = threadIdx.x;
  const int tiles_x = W / kTile, tiles_y = H / kTile;
  const int tx = blockIdx.x % tiles_x;
  const int rest = blockIdx.x / tiles_x;
  const int ty = rest % tiles_y, b = rest / tiles_y;
  const int ox0 = tx * kTile, oy0 = ty * kTile;
  ColorRow cr{};
  const ResizeGeom g = color_geom<2>(a, b, cr);              // workgroup-uniform: what the first launch saw
  const bool live = oy0 < g.nh && ox0 < g.nw;

  double mean = 0.0;
  if (live && (cr.flags & kContrast)) {
    const int tiles = tiles_x * tiles_y;
    const uint32_t* sums = a.sums + size_t(b) * tiles;
    unsigned long long s = 0;
    for (int t = tid; t < tiles; t += kResizeThreads) s += sums[t];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const uint32_t lo = uint32_t(__shfl_xor(int(uint32_t(s)), off, 64)), hi = uint32_t(__shfl_xor(int(uint32_t(s >> 32)), off, 64));
      s += (unsigned long long)hi << 32 | lo;
    }
    if ((tid & (kWave - 1)) == 0) part[tid / kWave] = s;
    __syncthreads();
    s = part[0];
    for (int w = 1; w < kResizeThreads / kWave; ++w) s += part[w];
    mean = double(s) / double(3ll * g.nh * g.nw);            // (exact integers below 2^53; u.mean() divides once)
  }

  const int ly = tid >> 3, lx = (tid & 7) << 2;
  const int y = oy0 + ly, x0 = ox0 + lx;
  float val[3][4];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
#pragma unroll
    for (int j = 0; j < 4; ++j) val[c][j] = 0.f;
  }
  if (live && y < g.nh && x0 < g.nw) {
    uint32_t px[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) px[c] = *reinterpret_cast<const uint32_t*>(a.stage + ((size_t(b) * 3 + c) * H + y) * W + x0);
    if (cr.flags & kContrast) contrast_words(px, cr.wc, mean);
    if (cr.flags & kSaturation) saturate_words(px, cr.ws);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (x0 + j < g.nw) val[c][j] = (float((px[c] >> (8 * j)) & 0xffu) - a.mean[c]) / a.std[c];
    }
  }
  store_x(a, b, y, x0, val);
  store_mask(a, b, oy0, ox0, tid, g.nh, g.nw);
}

inline size_t color_stage_bytes(int batch, int height, int width) { return size_t(batch) * 3 * size_t(height) * size_t(width); }

}  // namespace
}  // namespace vnx

using namespace vnx;

extern "C" int vnx_augment_frames(const void* pixels, size_t pixel_bytes, const void* src_table, const void* dst_table,
                                  const void* coeffs, size_t coeff_words, int batch, int height, int width, float mean0,
                                  float mean1, float mean2, float std0, float std1, float std2, int channels_last,
                                  int interleaved, void* x, void* mask, void* hip_stream) {
  const float mean[3] = {mean0, mean1, mean2}, std[3] = {std0, std1, std2};
  return launch_resize_ingest<true>("vnx_augment_frames", pixels, pixel_bytes, src_table, dst_table, coeffs, coeff_words,
                                    batch, height, width, mean, std, channels_last, interleaved, x, mask, hip_stream);
}

extern "C" size_t vnx_augment_color_workspace(int batch, int height, int width) {
  if (batch <= 0 || height < 32 || width < 32) return 0;
  return color_stage_bytes(batch, height, width) + size_t(batch) * size_t(height / kTile) * size_t(width / kTile) * sizeof(uint32_t);
}

extern "C" int vnx_augment_frames_color(void* pixels, size_t pixel_bytes, const void* src_table, const void* dst_table,
                                        const void* coeffs, size_t coeff_words, const void* color_table, int batch, int height,
                                        int width, float mean0, float mean1, float mean2, float std0, float std1, float std2,
                                        int channels_last, int interleaved, int contrast, size_t workspace_offset, void* x,
                                        void* mask, void* hip_stream) {
  const char* fn = "vnx_augment_frames_color";
  const float mean[3] = {mean0, mean1, mean2}, std[3] = {std0, std1, std2};
  ResizeArgs a;
  unsigned grid;
  const int rc = resize_ingest_args<true>(fn, pixels, pixel_bytes, src_table, dst_table, coeffs, coeff_words, batch, height,
                                          width, mean, std, channels_last, interleaved, x, mask, a, grid);
  if (rc != VNX_OK || grid == 0) return rc;
  if (!color_table || (reinterpret_cast<uintptr_t>(color_table) & 3) != 0) {
    set_error("%s: the colour table is null or not 4-byte aligned", fn);
    return VNX_ERR_INVALID_ARGUMENT;
  }
  a.color = (const int32_t*)color_table;
  hipStream_t stream = (hipStream_t)hip_stream;
  if (!contrast) {      // pointwise steps only: inside the one frame launch
    hipLaunchKernelGGL((resize_ingest_kernel<true, false, 1>), dim3(grid), dim3(kResizeThreads), 0, stream, a);
    return check_launch(fn);
  }
  const size_t need = vnx_augment_color_workspace(batch, height, width);
  if ((workspace_offset & 15) != 0 || workspace_offset > pixel_bytes || need > pixel_bytes - workspace_offset) {
    set_error("%s: the workspace (%zu bytes at byte %zu, 16-byte aligned) does not lie inside the %zu bytes of pixels", fn, need,
              workspace_offset, pixel_bytes);
    return VNX_ERR_INVALID_ARGUMENT;
  }
  a.stage = (unsigned char*)pixels + workspace_offset;
  a.sums = reinterpret_cast<uint32_t*>(a.stage + color_stage_bytes(batch, height, width));      // (a multiple of 16 behind it)
  hipLaunchKernelGGL((resize_ingest_kernel<true, false, 2>), dim3(grid), dim3(kResizeThreads), 0, stream, a);
  const int rc1 = check_launch(fn);
  if (rc1 != VNX_OK) return rc1;
  hipLaunchKernelGGL(color_finish_kernel, dim3(grid), dim3(kResizeThreads), 0, stream, a);
  return check_launch(fn);
}

extern "C" int vnx_resize_window_bytes(void* pixels, size_t pixel_bytes, const void* win_table, const void* coeffs,
                                       size_t coeff_words, int batch, int height, int width, int interleaved,
                                       void* hip_stream) {
  return launch_resize_window_bytes("vnx_resize_window_bytes", pixels, pixel_bytes, win_table, coeffs, coeff_words, batch,
                                    height, width, interleaved, hip_stream);
}

extern "C" size_t vnx_augment_masks_workspace(int n_masks, int height, int width) {
  if (n_masks <= 0 || height < 32 || width < 32) return 0;
  return size_t(n_masks) * size_t(height / kTile) * size_t(width / kTile) * 4 * sizeof(int32_t);
}

extern "C" int vnx_augment_masks(const void* ends, size_t n_ends, const void* mask_rows, int n_masks, const void* src_table,
                                 const void* dst_table, const void* coeffs, size_t coeff_words, int n_frames, int height,
                                 int width, void* masks, size_t mask_bytes, void* boxes, void* nonempty, void* workspace,
                                 size_t workspace_bytes, void* hip_stream) {
  const char* fn = "vnx_augment_masks";
  if (n_masks < 0 || n_frames < 0 || height < 32 || width < 32 || height % 32 != 0 || width % 32 != 0) {
    set_error("%s: bad sizes (%d masks, %d frames, padded %d x %d: multiples of 32)", fn, n_masks, n_frames, height, width);
    return VNX_ERR_INVALID_ARGUMENT;
  }
  if (n_masks == 0) return VNX_OK;
  if (!ends || !mask_rows || !src_table || !dst_table || !coeffs || !masks || !boxes || !nonempty || !workspace) {
    set_error("%s: null pointer argument", fn);
    return VNX_ERR_INVALID_ARGUMENT;
  }
  if (((reinterpret_cast<uintptr_t>(ends) | reinterpret_cast<uintptr_t>(mask_rows) | reinterpret_cast<uintptr_t>(src_table) |
        reinterpret_cast<uintptr_t>(dst_table) | reinterpret_cast<uintptr_t>(coeffs)) & 3) != 0 ||
      ((reinterpret_cast<uintptr_t>(boxes) | reinterpret_cast<uintptr_t>(workspace)) & 15) != 0) {
    set_error("%s: ends, the tables and coeffs must be 4-byte aligned, boxes and the workspace 16-byte aligned", fn);
    return VNX_ERR_INVALID_ARGUMENT;
  }
  if (coeff_words < kAugCoeffWords * size_t(n_frames)) {
    set_error("%s: coeffs holds %zu words: less than the %d frames' rows of %d", fn, coeff_words, n_frames, kAugCoeffWords);
    return VNX_ERR_INVALID_ARGUMENT;
  }
  if (n_ends > size_t(0x7fffffff) || coeff_words > size_t(0x7fffffff) || mask_bytes > size_t(0x7fffffff)) {
    set_error("%s: %zu ends, %zu words of tables, %zu bytes of masks: the rows address 2^31 - 1 at most", fn, n_ends,
              coeff_words, mask_bytes);
    return VNX_ERR_UNSUPPORTED;
  }
  const long long tiles = (long long)(height / kTile) * (width / kTile);
  const long long blocks = tiles * n_masks;
  if (blocks > 0x7fffffffll) {
    set_error("%s: %d masks of %d x %d are more than one launch addresses", fn, n_masks, height, width);
    return VNX_ERR_UNSUPPORTED;
  }
  if (workspace_bytes < vnx_augment_masks_workspace(n_masks, height, width)) {
    set_error("%s: the workspace holds %zu bytes; vnx_augment_masks_workspace asks for %zu", fn, workspace_bytes,
              vnx_augment_masks_workspace(n_masks, height, width));
    return VNX_ERR_INVALID_ARGUMENT;
  }
  MaskArgs a;
  a.ends = (const int32_t*)ends;
  a.n_ends = (long long)n_ends;
  a.rows = (const int32_t*)mask_rows;
  a.src_table = (const int32_t*)src_table;
  a.dst_table = (const int32_t*)dst_table;
  a.coeffs = (const int32_t*)coeffs;
  a.coeff_words = (long long)coeff_words;
  a.out = (unsigned char*)masks;
  a.out_bytes = (long long)mask_bytes;
  a.partial = (int32_t*)workspace;
  a.n_masks = n_masks; a.n_frames = n_frames; a.H = height; a.W = width;
  hipStream_t stream = (hipStream_t)hip_stream;
  hipLaunchKernelGGL(augment_masks_kernel, dim3(unsigned(blocks)), dim3(kMaskThreads), 0, stream, a);
  const int rc = check_launch(fn);
  if (rc != VNX_OK) return rc;
  hipLaunchKernelGGL(augment_boxes_kernel, dim3(unsigned(n_masks)), dim3(kWave), 0, stream, (const int32_t*)workspace,
                     int(tiles), (float*)boxes, (unsigned char*)nonempty);
  return check_launch(fn);
}
