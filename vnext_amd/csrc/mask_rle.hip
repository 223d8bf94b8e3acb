// mask_rle.hip -- COCO compressed RLE strings of a batch of masks, encoded on the device (the YTVIS results file's
// `segmentations`; host specification: vnext_amd/utils/ytvis_json.py rle_counts + counts_to_string, i.e. pycocotools'
// rleEncode + rleToString).
//
// One workgroup per mask walks the mask's column-major (Fortran) order in chunks of 256 x 32 pixels:
//   1. pixel p = chunk + step * 256 + thread, 32 steps: the thread forms p's bit (logits mode: ATen's nearest index on
//      the cropped grid, then ATen's align_corners=False bilinear value of the stride-s upsampling at that index, bit =
//      value > 0; binary mode: the byte != 0) and the wave's __ballot packs 64 consecutive pixels into a word in LDS.
//      Consecutive lanes take consecutive rows of one column, so the logit loads of a wave touch a few cache lines.
//   2. Thread t then owns the 32 CONSECUTIVE pixels chunk + 32 t .. + 31 (half of word t / 2): run ends = bit changes
//      against the previous pixel (the pixel before p = 0 counts as 0, so the first run counts zeros and is 0 when
//      pixel 0 is set); a block scan of the popcounts places every run end's position in LDS.
//   3. Run end k closes count k = P[k] - P[k-1]; from the fourth count on, the string holds count[k] - count[k-2]
//      (P[-1] = 0).  Each thread turns its run ends into characters (5-bit groups + 48, 0x20 = more follows, sign
//      termination on 0x10: at most 7 for an int32), a second block scan of the character counts gives the offsets.
//   The walk carries the last pixel's bit, the number of run ends so far, their last three positions and the string
//   offset across chunks; the last count (N - last run end) is closed by thread 0 after the walk.
// The measure launch writes each mask's string length; the write launch repeats the walk and stores the characters at
// the caller's offsets.  Nothing at full resolution is stored: no upsampled map, no bool mask.  No atomics: the output
// is a function of the input alone.  Every character store is bounds-checked against the arena.
#include "mask_sample.h"

namespace vnx {

constexpr int kRleThreads = 256;
constexpr int kRleSteps = 32;                                // ballots per chunk
constexpr int kRleChunk = kRleThreads * kRleSteps;           // 8192 pixels
constexpr int kRleWords = kRleChunk / 64;

struct RleArgs {
  const void* in;
  MaskSample s;      // logits mode: the map, the crop and the scales (mask_sample.h)
  int oh, ow;        // output mask
  int n;             // oh * ow
  int dq, dr;        // 256 / oh, 256 % oh: the walk's step in (column, row)
};

// exclusive scan of one int per thread over the workgroup (4 waves); one barrier
__device__ __forceinline__ int rle_block_scan(int v, int* s, int* total) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  int inc = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int o = __shfl_up(inc, d, 64);
    inc += lane >= d ? o : 0;
  }
  if (lane == 63) s[wv] = inc;
  __syncthreads();
  int before = 0, tot = 0;
#pragma unroll
  for (int i = 0; i < kRleThreads / 64; ++i) {
    const int si = s[i];
    before += i < wv ? si : 0;
    tot += si;
  }
  *total = tot;
  return before + inc - v;
}

// the value the string holds for count k, whose run end is at s[j] (s[j - 1..j - 3]: the three run ends before it)
__device__ __forceinline__ int rle_value(const int* s, int j, int k) {
  int c = s[j] - (k >= 1 ? s[j - 1] : 0);
  if (k > 2) c -= s[j - 2] - s[j - 3];
  return c;
}

// characters rleToString emits for x: the fewest 5-bit groups that hold x as a signed number
__device__ __forceinline__ int rle_chars(int x) {
  const uint32_t u = uint32_t(x ^ (x >> 31));
  return (u == 0u ? 0 : 32 - __builtin_clz(u)) / 5 + 1;
}

__device__ __forceinline__ int rle_emit(char* __restrict__ arena, int64_t o, int64_t cap, int x) {
  int n = 0;
  bool more = true;
  while (more) {
    int c = x & 0x1f;
    x >>= 5;
    more = (c & 0x10) ? x != -1 : x != 0;
    if (more) c |= 0x20;
    if (uint64_t(o + n) < uint64_t(cap)) arena[o + n] = char(c + 48);      // never outside [0, cap)
    ++n;
  }
  return n;
}

template <bool WRITE, bool LOGITS>
__global__ void __launch_bounds__(kRleThreads) mask_rle_kernel(RleArgs a, int64_t* __restrict__ lengths,
                                                                const int64_t* __restrict__ offsets,
                                                                char* __restrict__ arena, int64_t arena_bytes) {
  __shared__ uint64_t s_words[kRleWords];
  __shared__ int s_pos[3 + kRleChunk];       // [0..2]: the last three run ends of the chunks before; then this chunk's
  __shared__ int s_scan[2][kRleThreads / 64];
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const int64_t m = blockIdx.x;
  const float* map = LOGITS ? (const float*)a.in + m * a.s.h * a.s.w : nullptr;
  const uint8_t* bin = LOGITS ? nullptr : (const uint8_t*)a.in + m * a.n;
  int y = t % a.oh, x = t / a.oh;            // this thread's pixel of the current step
  uint32_t last_bit = 0;
  int K = 0, P0 = 0, P1 = 0, P2 = 0;         // run ends so far; P[K-3], P[K-2], P[K-1]
  int64_t out = WRITE ? offsets[m] : 0;
  for (int64_t base = 0; base < a.n; base += kRleChunk) {
#pragma unroll 4
    for (int k = 0; k < kRleSteps; ++k) {
      const int64_t p = base + k * kRleThreads + t;
      bool bit = false;
      if (p < a.n) bit = LOGITS ? mask_logit_bit(map, a.s, y, x) : bin[int64_t(y) * a.ow + x] != 0;
      const uint64_t word = __ballot(bit);
      if (lane == 0) s_words[k * (kRleThreads / 64) + wv] = word;
      y += a.dr;
      x += a.dq;
      if (y >= a.oh) { y -= a.oh; ++x; }
    }
    if (t == 0) { s_pos[0] = P0; s_pos[1] = P1; s_pos[2] = P2; }
    __syncthreads();
    const uint64_t wd = s_words[t >> 1];
    const uint32_t seg = uint32_t(wd >> (32 * (t & 1)));
    uint32_t prev;
    if (t & 1) prev = uint32_t(wd >> 31) & 1u;
    else prev = t == 0 ? last_bit : uint32_t(s_words[(t >> 1) - 1] >> 63);
    uint32_t chg = seg ^ ((seg << 1) | prev);
    const int64_t first = base + 32 * t;
    const int64_t left = a.n - first;                    // pixels of this segment inside the mask
    if (left < 32) chg = left <= 0 ? 0u : chg & ((1u << left) - 1u);
    int nchg;
    const int nmine = __popc(chg);
    const int excl = rle_block_scan(nmine, s_scan[0], &nchg);
    {
      uint32_t c = chg;
      int j = 3 + excl;
      while (c) {
        s_pos[j++] = int(first) + __ffs(c) - 1;
        c &= c - 1u;
      }
    }
    __syncthreads();
    int len = 0;
    for (int i = 0; i < nmine; ++i) len += rle_chars(rle_value(s_pos, 3 + excl + i, K + excl + i));
    int ctot;
    const int cexcl = rle_block_scan(len, s_scan[1], &ctot);
    if (WRITE) {
      int64_t o = out + cexcl;
      for (int i = 0; i < nmine; ++i) o += rle_emit(arena, o, arena_bytes, rle_value(s_pos, 3 + excl + i, K + excl + i));
    }
    out += ctot;
    K += nchg;
    P0 = s_pos[nchg];
    P1 = s_pos[nchg + 1];
    P2 = s_pos[nchg + 2];
    last_bit = uint32_t(s_words[kRleWords - 1] >> 63);
    __syncthreads();                                     // before the next chunk overwrites s_words / s_pos / s_scan
  }
  if (t == 0) {                                          // the last run: N - P[K-1]
    int c = a.n - (K >= 1 ? P2 : 0);
    if (K > 2) c -= P1 - P0;
    if (WRITE) rle_emit(arena, out, arena_bytes, c);
    else lengths[m] = out + rle_chars(c);
  }
}

static int mask_rle_launch(bool write, int mode, const void* input, int masks, int height, int width, int stride,
                           int image_height, int image_width, int out_height, int out_width, int64_t* lengths,
                           const int64_t* offsets, void* arena, int64_t arena_bytes, hipStream_t stream) {
  RleArgs a;
  a.in = input;
  a.oh = out_height; a.ow = out_width;
  a.s = mode == VNX_MASK_RLE_LOGITS ? mask_sample(height, width, stride, image_height, image_width, out_height, out_width)
                                    : MaskSample{};
  a.n = out_height * out_width;
  a.dq = kRleThreads / out_height;
  a.dr = kRleThreads % out_height;
  const dim3 grid{uint32_t(masks), 1, 1}, block{kRleThreads, 1, 1};
  const bool logits = mode == VNX_MASK_RLE_LOGITS;
  if (write) {
    if (logits) hipLaunchKernelGGL((mask_rle_kernel<true, true>), grid, block, 0, stream, a, nullptr, offsets, (char*)arena, arena_bytes);
    else hipLaunchKernelGGL((mask_rle_kernel<true, false>), grid, block, 0, stream, a, nullptr, offsets, (char*)arena, arena_bytes);
    return check_launch("mask_rle_write");
  }
  if (logits) hipLaunchKernelGGL((mask_rle_kernel<false, true>), grid, block, 0, stream, a, lengths, nullptr, nullptr, int64_t(0));
  else hipLaunchKernelGGL((mask_rle_kernel<false, false>), grid, block, 0, stream, a, lengths, nullptr, nullptr, int64_t(0));
  return check_launch("mask_rle_measure");
}

}  // namespace vnx

using namespace vnx;

static int mask_rle_check(const char* fn, int mode, const void* input, int masks, int height, int width, int stride,
                          int image_height, int image_width, int out_height, int out_width) {
  if (mode != VNX_MASK_RLE_LOGITS && mode != VNX_MASK_RLE_BINARY) {
    set_error("%s: unknown mode %d", fn, mode);
    return VNX_ERR_INVALID_ARGUMENT;
  }
  if (masks < 0 || out_height < 1 || out_width < 1) {
    set_error("%s: bad sizes (masks %d, out %d x %d)", fn, masks, out_height, out_width);
    return VNX_ERR_INVALID_ARGUMENT;
  }
  if (int64_t(out_height) * out_width >= (int64_t(1) << 31)) {
    set_error("%s: out %d x %d has 2^31 pixels or more (int32 counts)", fn, out_height, out_width);
    return VNX_ERR_UNSUPPORTED;
  }
  if (mode == VNX_MASK_RLE_LOGITS) {
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
    if (masks > 0 && (reinterpret_cast<uintptr_t>(input) & 3) != 0) {
      set_error("%s: logits must be 4-byte aligned", fn);
      return VNX_ERR_INVALID_ARGUMENT;
    }
  }
  if (masks > 0 && !input) {
    set_error("%s: null pointer argument", fn);
    return VNX_ERR_INVALID_ARGUMENT;
  }
  return VNX_OK;
}

extern "C" int vnx_mask_rle_measure(int mode, const void* input, int masks, int height, int width, int stride,
                                    int image_height, int image_width, int out_height, int out_width, void* lengths,
                                    void* hip_stream) {
  const char* fn = "vnx_mask_rle_measure";
  if (int st = mask_rle_check(fn, mode, input, masks, height, width, stride, image_height, image_width, out_height,
                              out_width))
    return st;
  if (masks == 0) return VNX_OK;
  if (!lengths) {
    set_error("%s: null pointer argument", fn);
    return VNX_ERR_INVALID_ARGUMENT;
  }
  return mask_rle_launch(false, mode, input, masks, height, width, stride, image_height, image_width, out_height, out_width,
                         (int64_t*)lengths, nullptr, nullptr, 0, (hipStream_t)hip_stream);
}

extern "C" int vnx_mask_rle_write(int mode, const void* input, int masks, int height, int width, int stride,
                                  int image_height, int image_width, int out_height, int out_width, const void* offsets,
                                  void* arena, long long arena_bytes, void* hip_stream) {
  const char* fn = "vnx_mask_rle_write";
  if (int st = mask_rle_check(fn, mode, input, masks, height, width, stride, image_height, image_width, out_height,
                              out_width))
    return st;
  if (arena_bytes < 0) {
    set_error("%s: arena_bytes %lld < 0", fn, arena_bytes);
    return VNX_ERR_INVALID_ARGUMENT;
  }
  if (masks == 0) return VNX_OK;
  if (!offsets || !arena) {
    set_error("%s: null pointer argument", fn);
    return VNX_ERR_INVALID_ARGUMENT;
  }
  return mask_rle_launch(true, mode, input, masks, height, width, stride, image_height, image_width, out_height, out_width,
                         nullptr, (const int64_t*)offsets, arena, int64_t(arena_bytes), (hipStream_t)hip_stream);
}
