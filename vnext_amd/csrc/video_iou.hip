// video_iou.hip -- the video mask IoU of the YTVIS evaluator (YTVOSeval.computeIoU) as integer sums over run tables, and
// the decode of compressed COCO RLE strings into those tables (host specification: vnext_amd/ops/video_iou.py
// runs_from_counts / pair_sums_host; the string format: vnext_amd/utils/ytvis_json.py string_to_counts).
//
// A mask is a slice of two int32 arenas: ends[k] = the column-major pixel index at which run k ends (the cumulative sum
// of the COCO counts, run 0 counts zeros), ones[k] = the set pixels below ends[k].  A pixel's bit is the parity of the
// upper bound of its index in ends (the rule of augment.hip), so zero-length runs are harmless.  A row per mask holds
// {arena offset, runs, pixel count, area}.
//
// Decode (vnx_rle_runs_measure / _write), one wave per string, 64 bytes per step:
//   a byte closes a count when it lacks the continuation bit 0x20, so the ballot of those bytes gives every count's
//   index (the popcount below the lane + the carry) and start (the closing byte before it); the lane that holds the
//   closing byte reads its count's <= 7 bytes back.  From the fourth count on the string holds count[i] - count[i-2]:
//   count[i] is the sum of the stored values of i's parity class (the class of even indices without value 0), so two
//   wave scans undo the differences, a third gives the run ends and a fourth the set pixels below them; four int64
//   carries go from step to step.  The measure launch counts the closing bytes: that number sizes the slot, and the
//   write launch derives every index from the same ballots, so it cannot leave the slot by construction (it is checked
//   all the same).  Byte reads stay inside [offset, offset + length) of the byte arena.
// Sums (vnx_video_iou_sums), one wave per (detection track, ground-truth track) pair, four pairs per workgroup:
//   the wave loops over the frames; lanes stride over the set runs [s, e) of the frame's mask with fewer runs and add
//   F(e) - F(s), F(x) = the other mask's set pixels below x = one upper bound in its ends, its ones and the parity.
//   int64 registers, one wave reduction at the end.  No atomics, no workspace: the output is a function of the input.
#include "vnx_common.h"

namespace vnx {

constexpr int kIouWaves = 4;                       // strings / pairs per workgroup

__device__ __forceinline__ int64_t wave_scan_i64(int64_t v, int lane) {          // inclusive
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int64_t o = __shfl_up(v, d, 64);
    v += lane >= d ? o : 0;
  }
  return v;
}

__device__ __forceinline__ int64_t wave_last_i64(int64_t v) { return __shfl(v, 63, 64); }

// a string's slice of the byte arena, or an empty one when the slice does not lie inside the arena
__device__ __forceinline__ bool rle_slice(const int64_t* offsets, const int64_t* lengths, int m, int64_t arena_bytes,
                                          int64_t* o, int64_t* len) {
  *o = offsets[m];
  *len = lengths[m];
  const bool ok = *o >= 0 && *len >= 0 && *o <= arena_bytes && *len <= arena_bytes - *o;
  if (!ok) { *o = 0; *len = 0; }
  return ok;
}

__global__ void __launch_bounds__(kIouWaves * 64) rle_runs_measure_kernel(const uint8_t* __restrict__ bytes,
                                                                           int64_t arena_bytes,
                                                                           const int64_t* __restrict__ offsets,
                                                                           const int64_t* __restrict__ lengths, int masks,
                                                                           int32_t* __restrict__ runs) {
  const int lane = threadIdx.x & 63;
  const int m = blockIdx.x * kIouWaves + (threadIdx.x >> 6);
  if (m >= masks) return;
  int64_t o, len;
  rle_slice(offsets, lengths, m, arena_bytes, &o, &len);
  const uint8_t* s = bytes + o;
  int64_t n = 0;
  for (int64_t base = 0; base < len; base += 64) {
    const int64_t i = base + lane;
    const bool end = i < len && ((int(s[i]) - 48) & 0x20) == 0;
    n += __popcll(__ballot(end));
  }
  if (lane == 0) runs[m] = int32_t(n < 0x7fffffff ? n : 0x7fffffff);
}

__global__ void __launch_bounds__(kIouWaves * 64) rle_runs_write_kernel(
    const uint8_t* __restrict__ bytes, int64_t arena_bytes, const int64_t* __restrict__ offsets,
    const int64_t* __restrict__ lengths, const int32_t* __restrict__ pixels, const int32_t* __restrict__ run_offsets,
    const int32_t* __restrict__ runs, int masks, int32_t* __restrict__ ends, int32_t* __restrict__ ones,
    int64_t run_slots, int32_t* __restrict__ rows, int32_t* __restrict__ status) {
  const int lane = threadIdx.x & 63;
  const int m = blockIdx.x * kIouWaves + (threadIdx.x >> 6);
  if (m >= masks) return;
  int64_t o, len;
  uint32_t st = rle_slice(offsets, lengths, m, arena_bytes, &o, &len) ? 0u : uint32_t(VNX_RLE_RUNS_BAD_SLOT);
  const uint8_t* s = bytes + o;
  const int64_t roff = run_offsets[m];
  int64_t slot = runs[m];
  const int64_t npx = pixels[m];
  if (roff < 0 || slot < 0 || roff > run_slots || slot > run_slots - roff) {      // a slot outside the run arenas
    st |= VNX_RLE_RUNS_BAD_SLOT;
    slot = 0;
  }
  int64_t K = 0;                                   // counts closed so far
  int64_t carry_even = 0, carry_odd = 0;           // sums of the stored values per parity class (without value 0)
  int64_t carry_end = 0, carry_ones = 0;           // pixels, set pixels below the last closed run's end
  int64_t last_close = -1;                         // position of the last closing byte before this step
  bool bad_byte = false, negative = false;
  for (int64_t base = 0; base < len; base += 64) {
    const int64_t i = base + lane;
    const bool in = i < len;
    const int c = in ? int(s[i]) - 48 : 0;
    bad_byte |= in && (c < 0 || c > 63);
    const bool end = in && (c & 0x20) == 0;
    const uint64_t closes = __ballot(end);
    const uint64_t below = closes & ((uint64_t(1) << lane) - 1u);
    const int64_t k = K + __popcll(below);
    int64_t x = 0;
    if (end) {
      int64_t start = below ? base + (63 - __clzll(below)) + 1 : last_close + 1;
      int n = int(i - start) + 1;
      if (n > 7) {                                 // more than 35 bits: no int32 count is written that way
        negative = true;
        start = i - 6;
        n = 7;
      }
      for (int j = 0; j < n; ++j) x |= int64_t((int(s[start + j]) - 48) & 0x1f) << (5 * j);
      if (c & 0x10) x |= ~int64_t(0) << (5 * n);
    }
    const bool odd = (k & 1) != 0;
    const int64_t se = wave_scan_i64(end && !odd && k != 0 ? x : 0, lane);
    const int64_t so = wave_scan_i64(end && odd ? x : 0, lane);
    const int64_t count = !end ? 0 : k == 0 ? x : odd ? carry_odd + so : carry_even + se;
    negative |= count < 0;
    const int64_t e = carry_end + wave_scan_i64(count, lane);
    const int64_t n1 = carry_ones + wave_scan_i64(odd ? count : 0, lane);
    if (end && k < slot) {                         // roff + k < roff + slot <= run_slots
      ends[roff + k] = int32_t(e);
      ones[roff + k] = int32_t(n1);
    }
    carry_even += wave_last_i64(se);
    carry_odd += wave_last_i64(so);
    carry_end = wave_last_i64(e);
    carry_ones = wave_last_i64(n1);
    K += __popcll(closes);
    if (closes) last_close = base + (63 - __clzll(closes));
  }
  if (__ballot(bad_byte)) st |= VNX_RLE_RUNS_BAD_BYTE;
  if (__ballot(negative)) st |= VNX_RLE_RUNS_NEGATIVE;
  if (len > 0 && last_close != len - 1) st |= VNX_RLE_RUNS_TRUNCATED;
  if (npx < 1 || carry_end != npx) st |= VNX_RLE_RUNS_BAD_SUM;
  if (K != slot) st |= VNX_RLE_RUNS_BAD_SLOT;      // the slot was not sized by the measure launch
  if (lane == 0) {
    rows[4 * m + 0] = int32_t(roff);
    rows[4 * m + 1] = st ? 0 : int32_t(K);
    rows[4 * m + 2] = int32_t(npx);
    rows[4 * m + 3] = st ? 0 : int32_t(carry_ones);
    status[m] = int32_t(st);
  }
}

struct IouTable {
  const int32_t* ends;
  const int32_t* ones;
  int n;
};

// set pixels of the table's mask below pixel index x
__device__ __forceinline__ int64_t iou_below(const IouTable& t, int x) {
  int lo = 0, hi = t.n;
  while (lo < hi) {                                // upper bound: the run that holds x
    const int mid = (lo + hi) >> 1;
    if (t.ends[mid] <= x) lo = mid + 1;
    else hi = mid;
  }
  if (lo == 0) return 0;
  return int64_t(t.ones[lo - 1]) + ((lo & 1) ? int64_t(x) - t.ends[lo - 1] : 0);
}

// a mask's row -> its table; false when the row does not lie inside the run arenas
__device__ __forceinline__ bool iou_table(const int32_t* ends, const int32_t* ones, int64_t run_slots, const int4 row,
                                          IouTable* t) {
  if (row.x < 0 || row.y < 0 || int64_t(row.x) + row.y > run_slots) return false;
  t->ends = ends + row.x;
  t->ones = ones + row.x;
  t->n = row.y;
  return true;
}

__global__ void __launch_bounds__(kIouWaves * 64) video_iou_sums_kernel(
    const int32_t* __restrict__ ends, const int32_t* __restrict__ ones, int64_t run_slots,
    const int4* __restrict__ rows, int masks, const int32_t* __restrict__ frame_mask, int64_t frame_slots,
    const int2* __restrict__ tracks, int n_tracks, const int2* __restrict__ pairs, int64_t n_pairs,
    int64_t* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int64_t p = int64_t(blockIdx.x) * kIouWaves + (threadIdx.x >> 6);
  if (p >= n_pairs) return;
  const int2 pr = pairs[p];
  int64_t inter = 0, area_d = 0, area_g = 0;       // inter: this lane's share; the areas: the same in every lane
  int st = 0;
  if (pr.x < 0 || pr.x >= n_tracks || pr.y < 0 || pr.y >= n_tracks) {
    st = VNX_VIDEO_IOU_BAD_TABLE;
  } else {
    const int2 td = tracks[pr.x], tg = tracks[pr.y];                              // {first, frames}
    if (td.x < 0 || td.y < 0 || int64_t(td.x) + td.y > frame_slots || tg.x < 0 || tg.y < 0 ||
        int64_t(tg.x) + tg.y > frame_slots)
      st = VNX_VIDEO_IOU_BAD_TABLE;
    else if (td.y != tg.y)
      st = VNX_VIDEO_IOU_FRAMES;
    for (int f = 0; st == 0 && f < td.y; ++f) {
      const int md = frame_mask[td.x + f], mg = frame_mask[tg.x + f];
      if (md >= masks || mg >= masks) { st = VNX_VIDEO_IOU_BAD_TABLE; break; }
      int4 rd = make_int4(0, 0, 0, 0), rg = rd;
      IouTable a{nullptr, nullptr, 0}, b{nullptr, nullptr, 0};
      if (md >= 0) {
        rd = rows[md];
        if (!iou_table(ends, ones, run_slots, rd, &a)) { st = VNX_VIDEO_IOU_BAD_TABLE; break; }
      }
      if (mg >= 0) {
        rg = rows[mg];
        if (!iou_table(ends, ones, run_slots, rg, &b)) { st = VNX_VIDEO_IOU_BAD_TABLE; break; }
      }
      if (md >= 0 && mg >= 0) {
        if (rd.z != rg.z) { st = VNX_VIDEO_IOU_PIXELS; break; }
        if (b.n < a.n) { const IouTable t = a; a = b; b = t; }                   // walk the mask with fewer runs
        for (int64_t k = 1 + 2 * lane; k < a.n; k += 128) inter += iou_below(b, a.ends[k]) - iou_below(b, a.ends[k - 1]);
      }
      area_d += rd.w;
      area_g += rg.w;
    }
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) inter += __shfl_xor(inter, d, 64);
  if (lane == 0) {
    out[4 * p + 0] = st ? 0 : inter;
    out[4 * p + 1] = st ? 0 : area_d;
    out[4 * p + 2] = st ? 0 : area_g;
    out[4 * p + 3] = st;
  }
}

}  // namespace vnx

using namespace vnx;

static int rle_runs_check(const char* fn, const void* bytes, long long arena_bytes, const void* offsets,
                          const void* lengths, int masks) {
  if (masks < 0 || arena_bytes < 0) {
    set_error("%s: bad sizes (masks %d, arena_bytes %lld)", fn, masks, arena_bytes);
    return VNX_ERR_INVALID_ARGUMENT;
  }
  if (masks > 0 && (!offsets || !lengths || (arena_bytes > 0 && !bytes))) {
    set_error("%s: null pointer argument", fn);
    return VNX_ERR_INVALID_ARGUMENT;
  }
  return VNX_OK;
}

extern "C" int vnx_rle_runs_measure(const void* bytes, long long arena_bytes, const void* offsets, const void* lengths,
                                    int masks, void* runs, void* hip_stream) {
  const char* fn = "vnx_rle_runs_measure";
  if (int st = rle_runs_check(fn, bytes, arena_bytes, offsets, lengths, masks)) return st;
  if (masks == 0) return VNX_OK;
  if (!runs) {
    set_error("%s: null pointer argument", fn);
    return VNX_ERR_INVALID_ARGUMENT;
  }
  const dim3 grid{uint32_t((masks + kIouWaves - 1) / kIouWaves), 1, 1}, block{kIouWaves * 64, 1, 1};
  hipLaunchKernelGGL(rle_runs_measure_kernel, grid, block, 0, (hipStream_t)hip_stream, (const uint8_t*)bytes,
                     int64_t(arena_bytes), (const int64_t*)offsets, (const int64_t*)lengths, masks, (int32_t*)runs);
  return check_launch(fn);
}

extern "C" int vnx_rle_runs_write(const void* bytes, long long arena_bytes, const void* offsets, const void* lengths,
                                  const void* pixels, const void* run_offsets, const void* runs, int masks, void* ends,
                                  void* ones, long long run_slots, void* rows, void* status, void* hip_stream) {
  const char* fn = "vnx_rle_runs_write";
  if (int st = rle_runs_check(fn, bytes, arena_bytes, offsets, lengths, masks)) return st;
  if (run_slots < 0 || run_slots >= (1ll << 31)) {
    set_error("%s: run_slots %lld outside [0, 2^31) (int32 arena offsets)", fn, run_slots);
    return run_slots < 0 ? VNX_ERR_INVALID_ARGUMENT : VNX_ERR_UNSUPPORTED;
  }
  if (masks == 0) return VNX_OK;
  if (!pixels || !run_offsets || !runs || !rows || !status || (run_slots > 0 && (!ends || !ones))) {
    set_error("%s: null pointer argument", fn);
    return VNX_ERR_INVALID_ARGUMENT;
  }
  const dim3 grid{uint32_t((masks + kIouWaves - 1) / kIouWaves), 1, 1}, block{kIouWaves * 64, 1, 1};
  hipLaunchKernelGGL(rle_runs_write_kernel, grid, block, 0, (hipStream_t)hip_stream, (const uint8_t*)bytes,
                     int64_t(arena_bytes), (const int64_t*)offsets, (const int64_t*)lengths, (const int32_t*)pixels,
                     (const int32_t*)run_offsets, (const int32_t*)runs, masks, (int32_t*)ends, (int32_t*)ones,
                     int64_t(run_slots), (int32_t*)rows, (int32_t*)status);
  return check_launch(fn);
}

extern "C" int vnx_video_iou_sums(const void* ends, const void* ones, long long run_slots, const void* rows, int masks,
                                  const void* frame_mask, long long frame_slots, const void* tracks, int n_tracks,
                                  const void* pairs, long long n_pairs, void* sums, void* hip_stream) {
  const char* fn = "vnx_video_iou_sums";
  if (masks < 0 || n_tracks < 0 || n_pairs < 0 || run_slots < 0 || frame_slots < 0) {
    set_error("%s: bad sizes (masks %d, tracks %d, pairs %lld, run_slots %lld, frame_slots %lld)", fn, masks, n_tracks,
              n_pairs, run_slots, frame_slots);
    return VNX_ERR_INVALID_ARGUMENT;
  }
  if (run_slots >= (1ll << 31) || frame_slots >= (1ll << 31) || n_pairs > (1ll << 31) * kIouWaves - kIouWaves) {
    set_error("%s: run_slots %lld, frame_slots %lld or pairs %lld beyond the int32 offsets / the grid", fn, run_slots,
              frame_slots, n_pairs);
    return VNX_ERR_UNSUPPORTED;
  }
  if (n_pairs == 0) return VNX_OK;
  if (!pairs || !sums || (n_tracks > 0 && !tracks) || (frame_slots > 0 && !frame_mask) || (masks > 0 && !rows) ||
      (run_slots > 0 && (!ends || !ones))) {
    set_error("%s: null pointer argument", fn);
    return VNX_ERR_INVALID_ARGUMENT;
  }
  if ((reinterpret_cast<uintptr_t>(rows) & 15) != 0 || (reinterpret_cast<uintptr_t>(tracks) & 7) != 0 ||
      (reinterpret_cast<uintptr_t>(pairs) & 7) != 0) {
    set_error("%s: rows must be 16-byte aligned, tracks and pairs 8-byte aligned", fn);
    return VNX_ERR_INVALID_ARGUMENT;
  }
  const dim3 grid{uint32_t((n_pairs + kIouWaves - 1) / kIouWaves), 1, 1}, block{kIouWaves * 64, 1, 1};
  hipLaunchKernelGGL(video_iou_sums_kernel, grid, block, 0, (hipStream_t)hip_stream, (const int32_t*)ends,
                     (const int32_t*)ones, int64_t(run_slots), (const int4*)rows, masks, (const int32_t*)frame_mask,
                     int64_t(frame_slots), (const int2*)tracks, n_tracks, (const int2*)pairs, int64_t(n_pairs),
                     (int64_t*)sums);
  return check_launch(fn);
}
