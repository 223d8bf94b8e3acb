// clip_link.hip -- SeqFormer's clip matching (models/clip_matching.py: Videos) with the video's state in device memory:
// one call per clip, three launches, no host copy.  The statements are those of Videos.get_siou / update / get_result;
// what differs is where they run.
//
// State of one video (cl_views; zeroed by vnx_clip_link_reset):
//   counters int32 [4]                   tracks opened, instances that found no free track, clips taken, 0
//   ring_count int32 [R], ring_ids int32 [R][n_max]      instances of each stored clip and the track of each (-1: none)
//   in_clips f32 [cap], seen f32 [cap][L], cls f32 [cap][K], total f32 [cap][L][HW]      the accumulators of get_result
//   ring f32 [R][n_max][R][HW]           mask probabilities of the last R clips (a clip has at most R frames)
// The frame lists stay on the host, which owns them: vnx_clip_link_plan names, per stored clip that shares a frame with the
// incoming one, the shared (stored position, incoming position) pairs, and travels to the kernels BY VALUE.
//
// Launch 1, clip_link_siou_kernel: grid (shared pair x pixel chunk, stored clip), four waves.  All four walk the same
// pixels, 4 per lane and step; wave w owns stored rows 4w .. 4w + 3 against all 16 incoming rows -- 64 product
// accumulators and 8 row sums per lane, nothing spills -- and takes the sigmoid of incoming rows 4w .. 4w + 3, which the
// waves hand each other through LDS (one expf per incoming element and workgroup).  Rows past n_c / n_i are zeros.  Lanes
// meet in an xor butterfly; lane 0 of each wave stores its quarter of the workgroup's partial block (288 floats).
// Launch 2, clip_link_match_kernel: one workgroup.  Partials summed pair by pair, chunk by chunk; sIoU per stored clip;
// mean over the clips that hold a track; threshold; one wave solves the assignment; lane 0 opens the new tracks.
// Launch 3, clip_link_accumulate_kernel: grid (pixel chunk, frame, instance): total[id][frame] += logits, the ring slot
// receives sigmoid(logits); the first workgroup of an instance adds its class probabilities and counts.
// No atomics, every sum in a fixed order: the output is a function of the input alone.
#include "lsap_wave.h"

namespace vnx {
namespace {

constexpr int kClInst = VNX_CLIP_LINK_MAX_INSTANCES;      // instances of a clip at most
constexpr int kClFrames = VNX_CLIP_LINK_MAX_FRAMES;       // frames of a clip = ring slots at most
constexpr int kClRows = kClInst * kClFrames;              // (stored clip, instance) entries of one update at most
constexpr int kClThreads = 256;
constexpr int kClStep = 4 * kWave;                        // pixels of one step of a workgroup
constexpr int kClBlock = kClInst * kClInst + 2 * kClInst; // a partial block: products [16][16], stored sums [16], incoming sums [16]
constexpr int kClChunksMax = 16;                          // pixel chunks of a frame at most
constexpr float kClThreshold = 0.01f;                     // Videos.match_threshold
// the head of the workspace: what launch 2 matched on (vnx_debug_clip_link_score_layout), written on every call
constexpr size_t kClWsRows = 0, kClWsTracks = 16, kClWsScores = kClWsTracks + size_t(kClRows) * 4;
constexpr size_t kClWsPartial = (kClWsScores + size_t(kClRows) * kClInst * 4 + 255) & ~size_t(255);

struct ClState {
  int32_t* counters;
  int32_t* ring_count;
  int32_t* ring_ids;
  float* in_clips;
  float* seen;
  float* cls;
  float* total;
  float* ring;
  size_t bytes;
};

ClState cl_views(const vnx_clip_link_config& c, void* base) {
  size_t off = 0;      // base may be null: the sizing calls only want `bytes`
  auto take = [&](size_t bytes) {
    unsigned char* q = reinterpret_cast<unsigned char*>(uintptr_t(base) + off);
    off += (bytes + 255) & ~size_t(255);
    return q;
  };
  ClState s;
  const size_t cap = size_t(c.capacity), hw = size_t(c.pixels), R = size_t(c.ring), nm = size_t(c.max_instances);
  s.counters = reinterpret_cast<int32_t*>(take(16));
  s.ring_count = reinterpret_cast<int32_t*>(take(R * 4));
  s.ring_ids = reinterpret_cast<int32_t*>(take(R * nm * 4));
  s.in_clips = reinterpret_cast<float*>(take(cap * 4));
  s.seen = reinterpret_cast<float*>(take(cap * size_t(c.video_length) * 4));
  s.cls = reinterpret_cast<float*>(take(cap * size_t(c.classes) * 4));
  s.total = reinterpret_cast<float*>(take(cap * size_t(c.video_length) * hw * 4));
  s.ring = reinterpret_cast<float*>(take(R * nm * R * hw * 4));
  s.bytes = off;
  return s;
}

// pixels of a chunk: whole steps, at least 1024, at most kClChunksMax chunks per frame
int cl_chunk(int hw) {
  int c = (hw + kClChunksMax - 1) / kClChunksMax;
  c = (c + kClStep - 1) / kClStep * kClStep;
  return c < 1024 ? 1024 : c;
}
int cl_chunks(int hw) { const int c = cl_chunk(hw); return (hw + c - 1) / c; }

__device__ __forceinline__ float cl_sigmoid(float x) { return 1.f / (1.f + expf(-x)); }

// four pixels of a row from px on; past the row's end: zeros.  VEC: hw % 4 == 0 and 16-byte aligned rows
template <bool VEC> __device__ __forceinline__ vnx_f4 cl_load4(const float* row, int px, int hw) {
  vnx_f4 v = {0.f, 0.f, 0.f, 0.f};
  if (VEC) {
    if (px < hw) v = *reinterpret_cast<const vnx_f4*>(row + px);
  } else {
    if (px < hw) v.x = row[px];
    if (px + 1 < hw) v.y = row[px + 1];
    if (px + 2 < hw) v.z = row[px + 2];
    if (px + 3 < hw) v.w = row[px + 3];
  }
  return v;
}
template <bool VEC> __device__ __forceinline__ void cl_store4(float* row, int px, int hw, vnx_f4 v) {
  if (VEC) {
    if (px < hw) *reinterpret_cast<vnx_f4*>(row + px) = v;
  } else {
    if (px < hw) row[px] = v.x;
    if (px + 1 < hw) row[px + 1] = v.y;
    if (px + 2 < hw) row[px + 2] = v.z;
    if (px + 3 < hw) row[px + 3] = v.w;
  }
}

// ---- launch 1: products and row sums of one (stored clip, shared frame pair, pixel chunk) ---------------------------------
template <bool VEC>
__global__ __launch_bounds__(kClThreads) void clip_link_siou_kernel(
    const float* __restrict__ ring, const int32_t* __restrict__ ring_count, const float* __restrict__ logits,
    const vnx_clip_link_plan plan, int n_i, int n_max, int ring_frames, int hw, int chunk, int chunks,
    float* __restrict__ partial) {
  __shared__ vnx_f4 sb[kClInst][kWave];      // sigmoid of the step's incoming rows, 16 KB
  const int a = blockIdx.y;
  const int pair = blockIdx.x / chunks, ck = blockIdx.x - pair * chunks;
  if (pair >= plan.pairs[a]) return;
  const int slot = plan.slot[a];
  int n_c = ring_count[slot];
  n_c = n_c < n_max ? n_c : n_max;
  if (n_c <= 0) return;                      // an empty clip does not count (Videos.get_siou): launch 2 skips it too
  const int lane = threadIdx.x & (kWave - 1), wave = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
  const int ks = plan.stored_pos[a][pair], ki = plan.incoming_pos[a][pair], T = plan.frames;
  const float* a_row[4];
  const float* b_row[4];
  for (int r = 0; r < 4; ++r) {
    const int i = 4 * wave + r;
    a_row[r] = ring + ((size_t(slot) * n_max + (i < n_c ? i : 0)) * ring_frames + ks) * size_t(hw);
    b_row[r] = logits + (size_t(i < n_i ? i : 0) * T + ki) * size_t(hw);
  }
  float acc[4][kClInst];
  float asum[4], bsum[4];
  for (int r = 0; r < 4; ++r) {
    asum[r] = bsum[r] = 0.f;
    for (int j = 0; j < kClInst; ++j) acc[r][j] = 0.f;
  }
  const int begin = ck * chunk, end = begin + chunk < hw ? begin + chunk : hw;
  for (int p0 = begin; p0 < end; p0 += kClStep) {
    const int px = p0 + 4 * lane;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      vnx_f4 v = {0.f, 0.f, 0.f, 0.f};
      if (4 * wave + r < n_i) {
        const vnx_f4 x = cl_load4<VEC>(b_row[r], px, hw);
        v.x = px < hw ? cl_sigmoid(x.x) : 0.f;
        v.y = px + 1 < hw ? cl_sigmoid(x.y) : 0.f;
        v.z = px + 2 < hw ? cl_sigmoid(x.z) : 0.f;
        v.w = px + 3 < hw ? cl_sigmoid(x.w) : 0.f;
      }
      sb[4 * wave + r][lane] = v;
      bsum[r] += (v.x + v.y) + (v.z + v.w);
    }
    __syncthreads();
    vnx_f4 va[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      va[r] = vnx_f4{0.f, 0.f, 0.f, 0.f};
      if (4 * wave + r < n_c) va[r] = cl_load4<VEC>(a_row[r], px, hw);
      asum[r] += (va[r].x + va[r].y) + (va[r].z + va[r].w);
    }
#pragma unroll
    for (int j = 0; j < kClInst; ++j) {
      if (j < n_i) {
        const vnx_f4 vb = sb[j][lane];
#pragma unroll
        for (int r = 0; r < 4; ++r)
          acc[r][j] = fmaf(va[r].w, vb.w, fmaf(va[r].z, vb.z, fmaf(va[r].y, vb.y, fmaf(va[r].x, vb.x, acc[r][j]))));
      }
    }
    __syncthreads();
  }
  float* out = partial + ((size_t(a) * kClFrames + pair) * chunks + ck) * kClBlock;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
#pragma unroll
    for (int j = 0; j < kClInst; j += 4) {
      const vnx_f4 v = {wave_sum(acc[r][j]), wave_sum(acc[r][j + 1]), wave_sum(acc[r][j + 2]),
                        wave_sum(acc[r][j + 3])};
      if (lane == 0) *reinterpret_cast<vnx_f4*>(out + (4 * wave + r) * kClInst + j) = v;
    }
  }
  const vnx_f4 sa = {wave_sum(asum[0]), wave_sum(asum[1]), wave_sum(asum[2]), wave_sum(asum[3])};
  const vnx_f4 sbm = {wave_sum(bsum[0]), wave_sum(bsum[1]), wave_sum(bsum[2]), wave_sum(bsum[3])};
  if (lane == 0) {
    *reinterpret_cast<vnx_f4*>(out + kClInst * kClInst + 4 * wave) = sa;
    *reinterpret_cast<vnx_f4*>(out + kClInst * kClInst + kClInst + 4 * wave) = sbm;
  }
}

// ---- launch 2: scores, assignment, track ids ---------------------------------------------------------------------------------
__global__ __launch_bounds__(kClThreads) void clip_link_match_kernel(
    int32_t* __restrict__ counters, int32_t* __restrict__ ring_count, int32_t* __restrict__ ring_ids,
    const float* __restrict__ partial, const vnx_clip_link_plan plan, int n_i, int n_max, int cap, int chunks,
    int64_t* __restrict__ ids_out, int32_t* __restrict__ dbg_rows, int32_t* __restrict__ dbg_tracks,
    float* __restrict__ dbg_scores) {
  __shared__ float s_sum[kClFrames][kClBlock];            // per stored clip: the partial blocks summed
  __shared__ float s_siou[kClFrames][kClInst][kClInst];   // per stored clip: inter / (union + 1e-6)
  __shared__ float s_score[kClRows][kClInst];             // per row (a track some stored clip holds): the thresholded mean
  __shared__ int s_count[kClFrames];                      // instances of each stored clip
  __shared__ int s_id[kClRows];                           // track of entry (stored clip, instance); -1: none
  __shared__ int s_first[kClRows];                        // the entry is the first that names its track
  __shared__ int s_row_entry[kClRows];                    // row -> its first entry
  __shared__ int s_rows;
  __shared__ int s_track_of[kClInst];
  __shared__ __attribute__((aligned(16))) unsigned char s_lsap[(lsap_lds_bytes(kClInst, kClRows) + 15) & ~size_t(15)];
  const int tid = threadIdx.x;
  const int slots = n_i > 0 ? plan.slots : 0;             // an empty clip matches nothing (Videos.update)
  if (tid < kClFrames) {
    int c = 0;
    if (tid < slots) {
      c = ring_count[plan.slot[tid]];
      c = c < n_max ? c : n_max;
    }
    s_count[tid] = c < 0 ? 0 : c;
  }
  __syncthreads();
  // the blocks launch 1 wrote, added pair by pair, chunk by chunk
  for (int idx = tid; idx < slots * kClBlock; idx += kClThreads) {
    const int a = idx / kClBlock, c = idx - a * kClBlock;
    float sum = 0.f;
    if (s_count[a] > 0)
      for (int blk = 0; blk < plan.pairs[a] * chunks; ++blk) {
        const int pair = blk / chunks, ck = blk - pair * chunks;
        sum += partial[((size_t(a) * kClFrames + pair) * chunks + ck) * kClBlock + c];
      }
    s_sum[a][c] = sum;
  }
  if (tid < kClRows) {
    const int a = tid / kClInst, i = tid - a * kClInst;
    int id = -1;
    if (a < slots && i < s_count[a]) id = ring_ids[plan.slot[a] * n_max + i];
    s_id[tid] = id >= 0 && id < cap ? id : -1;            // an instance that found no track holds none
  }
  __syncthreads();
  for (int idx = tid; idx < slots * kClInst * kClInst; idx += kClThreads) {
    const int a = idx / (kClInst * kClInst), i = (idx / kClInst) % kClInst, j = idx % kClInst;
    const float inter = s_sum[a][i * kClInst + j];
    const float uni = s_sum[a][kClInst * kClInst + i] + s_sum[a][kClInst * kClInst + kClInst + j] - inter;
    s_siou[a][i][j] = inter / (uni + 1e-6f);
  }
  if (tid < kClRows) {
    int first = 0;
    const int id = s_id[tid];
    if (id >= 0) {
      first = 1;
      for (int e = 0; e < tid; ++e) first = s_id[e] == id ? 0 : first;
    }
    s_first[tid] = first;
  }
  __syncthreads();
  if (tid == 0) {
    int rows = 0;
    for (int e = 0; e < kClRows; ++e)
      if (s_first[e]) s_row_entry[rows++] = e;
    s_rows = rows;
    *dbg_rows = rows;
  }
  if (tid < kClInst) s_track_of[tid] = -1;
  __syncthreads();
  const int rows = s_rows;
  // siou[id] += ...; count[id] += 1 over the stored clips in their order, then siou / (count + 1e-6)
  for (int cell = tid; cell < rows * n_i; cell += kClThreads) {
    const int r = cell / n_i, j = cell - r * n_i;
    const int e0 = s_row_entry[r], id = s_id[e0];
    float sum = 0.f, count = 0.f;
    for (int e = e0; e < slots * kClInst; ++e)
      if (s_id[e] == id) {
        sum += s_siou[e / kClInst][e % kClInst][j];
        count += 1.f;
      }
    const float score = sum / (count + 1e-6f);
    dbg_scores[r * kClInst + j] = score;
    if (j == 0) dbg_tracks[r] = id;
    s_score[r][j] = score > kClThreshold ? score : 0.f;
  }
  __syncthreads();
  if (tid < kWave) {
    const int lane = tid;
    // Only these rows -- the tracks a stored clip of the window holds -- can have a non-zero score; the host form solves
    // over every track.  Dropping the all-zero rows changes nothing that is used: a complete assignment is worth the sum
    // of its positive pairs, which form a matching of the positive entries, and every such matching extends to a
    // complete assignment worth at least as much -- with or without the zero rows the optimum is the maximum-weight
    // matching of the positive entries, and where that is unique both problems return its pairs.  Pairs at zero are
    // discarded below, as `above[r, c]` discards them on the host.
    if (rows > 0 && n_i > 0) {
      const bool rows_short = rows <= n_i;
      const int ns = rows_short ? rows : n_i, nl = rows_short ? n_i : rows;
      const LsapLds s = carve(s_lsap, ns, nl);
      for (int c = lane; c < ns * nl; c += kWave) {
        const int si = c / nl, li = c - si * nl;
        s.cost[c] = -(rows_short ? s_score[si][li] : s_score[li][si]);      // maximise
      }
      wave_sync();
      if (lsap_solve_wave(s, ns, nl, lane)) {
        for (int si = lane; si < ns; si += kWave) {
          const int li = s.col_of_row[si];
          const int r = rows_short ? si : li, c = rows_short ? li : si;
          if (s_score[r][c] > 0.f) s_track_of[c] = s_id[s_row_entry[r]];
        }
      }
      wave_sync();
    }
    if (lane == 0) {      // unmatched instances open new tracks, in input order
      int opened = counters[0], lost = counters[1];
      const int slot = plan.write_slot;
      for (int c = 0; c < n_i; ++c) {
        int t = s_track_of[c];
        if (t < 0) {
          if (opened < cap) t = opened++; else ++lost;
        }
        ids_out[c] = t;
        ring_ids[slot * n_max + c] = t;
      }
      ring_count[slot] = n_i;
      counters[0] = opened;
      counters[1] = lost;
      counters[2] += 1;
    }
  }
}

// ---- launch 3: the clip joins its tracks and the ring -------------------------------------------------------------------------
template <bool VEC>
__global__ __launch_bounds__(kClThreads) void clip_link_accumulate_kernel(
    const float* __restrict__ logits, const float* __restrict__ cls_probs, const int64_t* __restrict__ ids,
    const vnx_clip_link_plan plan, int n_max, int ring_frames, int hw, int L, int K, int cap, float* __restrict__ total,
    float* __restrict__ seen, float* __restrict__ cls, float* __restrict__ in_clips, float* __restrict__ ring) {
  const int j = blockIdx.z, k = blockIdx.y, T = plan.frames;
  const int px = (blockIdx.x * kClThreads + threadIdx.x) * 4;
  const int64_t id = ids[j];
  const bool held = id >= 0 && id < cap;     // instances of one clip hold distinct tracks: every element has one owner
  const vnx_f4 x = cl_load4<VEC>(logits + (size_t(j) * T + k) * size_t(hw), px, hw);
  const vnx_f4 p = {cl_sigmoid(x.x), cl_sigmoid(x.y), cl_sigmoid(x.z), cl_sigmoid(x.w)};
  cl_store4<VEC>(ring + ((size_t(plan.write_slot) * n_max + j) * ring_frames + k) * size_t(hw), px, hw, p);
  if (!held) return;
  float* row = total + (size_t(id) * L + plan.frame_index[k]) * size_t(hw);
  const vnx_f4 t = cl_load4<VEC>(row, px, hw);
  cl_store4<VEC>(row, px, hw, vnx_f4{t.x + x.x, t.y + x.y, t.z + x.z, t.w + x.w});
  if (blockIdx.x == 0 && k == 0) {
    for (int c = threadIdx.x; c < K; c += kClThreads) cls[size_t(id) * K + c] += cls_probs[size_t(j) * K + c];
    if (threadIdx.x == 0) {
      in_clips[id] += 1.f;
      for (int f = 0; f < T; ++f) seen[size_t(id) * L + plan.frame_index[f]] += 1.f;
    }
  }
}

// ---- the result: cls / in_clips, total / seen ---------------------------------------------------------------------------------
template <bool VEC>
__global__ __launch_bounds__(kClThreads) void clip_link_result_kernel(
    const float* __restrict__ total, const float* __restrict__ seen, const float* __restrict__ cls,
    const float* __restrict__ in_clips, int hw, int L, int K, float* __restrict__ cls_out, float* __restrict__ logits_out) {
  const int t = blockIdx.z, f = blockIdx.y;
  const int px = (blockIdx.x * kClThreads + threadIdx.x) * 4;
  const size_t row = (size_t(t) * L + f) * size_t(hw);
  const float s = seen[size_t(t) * L + f];                // 0 where no clip of the track covers the frame: 0 / 0 = NaN
  const vnx_f4 v = cl_load4<VEC>(total + row, px, hw);
  cl_store4<VEC>(logits_out + row, px, hw, vnx_f4{v.x / s, v.y / s, v.z / s, v.w / s});
  if (blockIdx.x == 0 && f == 0) {
    const float n = in_clips[t];
    for (int c = threadIdx.x; c < K; c += kClThreads) cls_out[size_t(t) * K + c] = cls[size_t(t) * K + c] / n;
  }
}

int cl_check_config(const vnx_clip_link_config* c, const char* who) {
  if (!c) { set_error("%s: null config", who); return VNX_ERR_INVALID_ARGUMENT; }
  if (c->ring < 1 || c->max_instances < 1 || c->pixels < 1 || c->video_length < 1 || c->classes < 1 || c->capacity < 1) {
    set_error("%s: config out of range (ring %d, max_instances %d, pixels %d, video_length %d, classes %d, capacity %d: "
              "all at least 1)", who, c->ring, c->max_instances, c->pixels, c->video_length, c->classes, c->capacity);
    return VNX_ERR_INVALID_ARGUMENT;
  }
  if (c->ring > kClFrames || c->max_instances > kClInst) {
    set_error("%s: built for clips of up to %d frames and %d instances (got %d and %d)", who, kClFrames, kClInst, c->ring,
              c->max_instances);
    return VNX_ERR_UNSUPPORTED;
  }
  // a frame's pixels x 4 and the launch grids stay inside int; classes inside one workgroup's loop
  if (c->pixels > (1 << 28) || c->video_length > 65535 || c->capacity > (1 << 20) || c->classes > (1 << 20)) {
    set_error("%s: pixels %d, video_length %d, capacity %d or classes %d outside what the kernels address", who, c->pixels,
              c->video_length, c->capacity, c->classes);
    return VNX_ERR_UNSUPPORTED;
  }
  return VNX_OK;
}

size_t cl_workspace_bytes(const vnx_clip_link_config& c) {
  return kClWsPartial + size_t(kClFrames) * kClFrames * cl_chunks(c.pixels) * kClBlock * 4;
}

}  // namespace
}  // namespace vnx

using namespace vnx;

extern "C" size_t vnx_clip_link_state_bytes(const vnx_clip_link_config* cfg) {
  if (cl_check_config(cfg, "vnx_clip_link_state_bytes") != VNX_OK) return 0;
  return cl_views(*cfg, nullptr).bytes;
}

extern "C" size_t vnx_clip_link_workspace_bytes(const vnx_clip_link_config* cfg) {
  if (cl_check_config(cfg, "vnx_clip_link_workspace_bytes") != VNX_OK) return 0;
  return cl_workspace_bytes(*cfg);
}

extern "C" int vnx_clip_link_reset(const vnx_clip_link_config* cfg, void* state, void* hip_stream) {
  if (int st = cl_check_config(cfg, "vnx_clip_link_reset")) return st;
  if (!state || (uintptr_t(state) % 16)) {
    set_error("vnx_clip_link_reset: state must be a 16-byte aligned device pointer");
    return VNX_ERR_INVALID_ARGUMENT;
  }
  if (hipMemsetAsync(state, 0, cl_views(*cfg, state).bytes, (hipStream_t)hip_stream) != hipSuccess) {
    set_error("vnx_clip_link_reset: hipMemsetAsync failed");
    return VNX_ERR_LAUNCH;
  }
  return VNX_OK;
}

extern "C" int vnx_clip_link_update(const vnx_clip_link_config* cfg, void* state, const void* mask_logits,
                                    const void* cls_probs, const vnx_clip_link_plan* plan, int num_instances,
                                    void* ids_out, void* workspace, size_t workspace_bytes, void* hip_stream) {
  const char* fn = "vnx_clip_link_update";
  if (int st = cl_check_config(cfg, fn)) return st;
  if (!plan || num_instances < 0 || plan->frames < 1) {
    set_error("%s: null plan, negative instance count or a clip without frames", fn);
    return VNX_ERR_INVALID_ARGUMENT;
  }
  const int n = num_instances, T = plan->frames;
  if (n > cfg->max_instances || T > cfg->ring) {
    set_error("%s: a clip of %d instances x %d frames; this state takes up to %d x %d (the kernels: %d x %d)", fn, n, T,
              cfg->max_instances, cfg->ring, kClInst, kClFrames);
    return VNX_ERR_UNSUPPORTED;
  }
  bool ok = plan->slots >= 0 && plan->slots <= cfg->ring && plan->write_slot >= 0 && plan->write_slot < cfg->ring;
  for (int f = 0; ok && f < T; ++f) {
    ok = plan->frame_index[f] >= 0 && plan->frame_index[f] < cfg->video_length;
    for (int g = 0; g < f; ++g) ok = ok && plan->frame_index[g] != plan->frame_index[f];
  }
  for (int a = 0; ok && a < plan->slots; ++a) {
    ok = plan->slot[a] >= 0 && plan->slot[a] < cfg->ring && plan->pairs[a] >= 1 && plan->pairs[a] <= T;
    for (int p = 0; ok && p < plan->pairs[a]; ++p)
      ok = plan->stored_pos[a][p] < cfg->ring && plan->incoming_pos[a][p] < T;
  }
  if (!ok) {
    set_error("%s: plan outside the state (ring slots 0..%d, frame positions inside their clips, frames distinct and "
              "inside the video of %d)", fn, cfg->ring - 1, cfg->video_length);
    return VNX_ERR_INVALID_ARGUMENT;
  }
  if (!state || (uintptr_t(state) % 16) || !workspace || (uintptr_t(workspace) % 16) ||
      workspace_bytes < cl_workspace_bytes(*cfg) || (n > 0 && (!mask_logits || !cls_probs || !ids_out))) {
    set_error("%s: null pointer, state or workspace not 16-byte aligned, or workspace smaller than "
              "vnx_clip_link_workspace_bytes", fn);
    return VNX_ERR_INVALID_ARGUMENT;
  }
  hipStream_t stream = (hipStream_t)hip_stream;
  const ClState s = cl_views(*cfg, state);
  unsigned char* ws = static_cast<unsigned char*>(workspace);
  float* partial = reinterpret_cast<float*>(ws + kClWsPartial);
  const int hw = cfg->pixels, chunk = cl_chunk(hw), chunks = cl_chunks(hw);
  const bool vec = hw % 4 == 0 && uintptr_t(mask_logits) % 16 == 0;
  const float* logits = static_cast<const float*>(mask_logits);
  if (n > 0 && plan->slots > 0) {
    int pairs_max = 0;
    for (int a = 0; a < plan->slots; ++a) pairs_max = plan->pairs[a] > pairs_max ? plan->pairs[a] : pairs_max;
    const dim3 grid(pairs_max * chunks, plan->slots);
    if (vec)
      hipLaunchKernelGGL(clip_link_siou_kernel<true>, grid, dim3(kClThreads), 0, stream, s.ring, s.ring_count, logits, *plan,
                         n, cfg->max_instances, cfg->ring, hw, chunk, chunks, partial);
    else
      hipLaunchKernelGGL(clip_link_siou_kernel<false>, grid, dim3(kClThreads), 0, stream, s.ring, s.ring_count, logits,
                         *plan, n, cfg->max_instances, cfg->ring, hw, chunk, chunks, partial);
    if (int st = check_launch(fn)) return st;
  }
  hipLaunchKernelGGL(clip_link_match_kernel, dim3(1), dim3(kClThreads), 0, stream, s.counters, s.ring_count, s.ring_ids,
                     partial, *plan, n, cfg->max_instances, cfg->capacity, chunks, static_cast<int64_t*>(ids_out),
                     reinterpret_cast<int32_t*>(ws + kClWsRows), reinterpret_cast<int32_t*>(ws + kClWsTracks),
                     reinterpret_cast<float*>(ws + kClWsScores));
  if (int st = check_launch(fn)) return st;
  if (n > 0) {
    const dim3 grid((hw + 4 * kClThreads - 1) / (4 * kClThreads), T, n);
    if (vec)
      hipLaunchKernelGGL(clip_link_accumulate_kernel<true>, grid, dim3(kClThreads), 0, stream, logits,
                         static_cast<const float*>(cls_probs), static_cast<const int64_t*>(ids_out), *plan,
                         cfg->max_instances, cfg->ring, hw, cfg->video_length, cfg->classes, cfg->capacity, s.total, s.seen,
                         s.cls, s.in_clips, s.ring);
    else
      hipLaunchKernelGGL(clip_link_accumulate_kernel<false>, grid, dim3(kClThreads), 0, stream, logits,
                         static_cast<const float*>(cls_probs), static_cast<const int64_t*>(ids_out), *plan,
                         cfg->max_instances, cfg->ring, hw, cfg->video_length, cfg->classes, cfg->capacity, s.total, s.seen,
                         s.cls, s.in_clips, s.ring);
    if (int st = check_launch(fn)) return st;
  }
  return VNX_OK;
}

extern "C" int vnx_clip_link_result(const vnx_clip_link_config* cfg, const void* state, int num_tracks, void* cls_out,
                                    void* logits_out, void* hip_stream) {
  const char* fn = "vnx_clip_link_result";
  if (int st = cl_check_config(cfg, fn)) return st;
  if (num_tracks < 0 || num_tracks > cfg->capacity) {
    set_error("%s: %d tracks asked of a state of %d", fn, num_tracks, cfg->capacity);
    return VNX_ERR_INVALID_ARGUMENT;
  }
  if (num_tracks == 0) return VNX_OK;
  if (!state || (uintptr_t(state) % 16) || !cls_out || !logits_out) {
    set_error("%s: null pointer or state not 16-byte aligned", fn);
    return VNX_ERR_INVALID_ARGUMENT;
  }
  if (num_tracks > 65535) {
    set_error("%s: %d tracks are more than one launch grid takes", fn, num_tracks);
    return VNX_ERR_UNSUPPORTED;
  }
  const ClState s = cl_views(*cfg, const_cast<void*>(state));
  const int hw = cfg->pixels;
  const dim3 grid((hw + 4 * kClThreads - 1) / (4 * kClThreads), cfg->video_length, num_tracks);
  float* cls = static_cast<float*>(cls_out);
  float* out = static_cast<float*>(logits_out);
  if (hw % 4 == 0 && uintptr_t(logits_out) % 16 == 0)
    hipLaunchKernelGGL(clip_link_result_kernel<true>, grid, dim3(kClThreads), 0, (hipStream_t)hip_stream, s.total, s.seen,
                       s.cls, s.in_clips, hw, cfg->video_length, cfg->classes, cls, out);
  else
    hipLaunchKernelGGL(clip_link_result_kernel<false>, grid, dim3(kClThreads), 0, (hipStream_t)hip_stream, s.total, s.seen,
                       s.cls, s.in_clips, hw, cfg->video_length, cfg->classes, cls, out);
  return check_launch(fn);
}

extern "C" int vnx_debug_clip_link_score_layout(size_t* rows_offset, size_t* tracks_offset, size_t* scores_offset,
                                                int* rows_max, int* row_stride) {
  if (!rows_offset || !tracks_offset || !scores_offset || !rows_max || !row_stride) return VNX_ERR_INVALID_ARGUMENT;
  *rows_offset = kClWsRows;
  *tracks_offset = kClWsTracks;
  *scores_offset = kClWsScores;
  *rows_max = kClRows;
  *row_stride = kClInst;
  return VNX_OK;
}
