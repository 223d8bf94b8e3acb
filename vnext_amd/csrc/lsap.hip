// lsap.hip -- linear sum assignment on the device: SeqFormer's Hungarian matching without the host round trip.
//
// One launch solves every problem of a call, ONE WAVE64 PER PROBLEM (a workgroup is one wave): the problems are tiny (300
// queries x a handful of targets), the algorithm is a chain of dependent steps, and a single wave needs no workgroup
// barrier -- its lanes exchange values through __shfl_xor and through LDS in program order.  Every reduction has a fixed
// order and nothing is atomic, so the output is a function of the input alone (bit-identical run to run).
//
// Algorithm: shortest augmenting paths with dual variables (Crouse 2016, "On implementing 2D rectangular assignment
// algorithms" -- the algorithm of scipy's linear_sum_assignment).  The SHORT side (targets) is augmented one element at a
// time; the LONG side (queries) is spread over the lanes, column j on lane j % 64.  One Dijkstra step relaxes the lane's
// columns against the current row and takes one wave-wide arg-min (ties to the lower column); augmenting target number c
// takes at most c + 1 steps, n (n + 1) / 2 for a problem.  Duals, path costs and the running minimum are fp64 on fp32 cost
// entries, as scipy solves in double: on the same matrix the assignment is scipy's whenever the optimum is unique.
//
// LDS of a problem with ns short and nl long elements (lsap_lds_bytes): fp64 u[ns] v[nl] path_cost[nl], int32 path[nl]
// row_of_col[nl] done[nl] col_of_row[ns], then the cost block fp32 [ns][nl] (lane j reads bank j: conflict-free).
// Q = 300: 8.4 KB + n x 1212 B, n <= 128 in the 160 KB of a gfx950 CU.
//
// vnx_seqformer_match computes its cost block in the kernel (HungarianMatcher.cost, reference matcher.py:53-96);
// vnx_lsap_solve takes cost matrices from device memory through strides.
// The solver of one wave itself (LsapLds, carve, wave_sync, lsap_lds_bytes, lsap_solve_wave) lives in lsap_wave.h, which
// clip_link.hip includes too.
#include "lsap_wave.h"

namespace vnx {
namespace {

constexpr size_t kLdsBytes = 160 * 1024;      // LDS of a gfx950 CU = the most one workgroup can ask for

// pairs in ascending order of the long-side index (a counting rank over the ns <= nl assigned columns):
// long_out[rank] = long index, short_out[rank] = short index
__device__ void write_sorted_by_long(const LsapLds& s, int ns, int lane, int64_t* long_out, int64_t* short_out) {
  for (int i = lane; i < ns; i += kWave) {
    const int c = s.col_of_row[i];
    int rank = 0;
    for (int k = 0; k < ns; ++k) rank += s.col_of_row[k] < c;
    long_out[rank] = c;
    short_out[rank] = i;
  }
}

__device__ void write_unsolved(int n, int lane, int64_t* a, int64_t* b) {
  for (int r = lane; r < n; r += kWave) { a[r] = -1; b[r] = -1; }
}

// ---- SeqFormer: cost block + assignment of one (decoder layer, clip) per wave -----------------------------------------
__global__ __launch_bounds__(kWave) void seqformer_match_kernel(
    const float* __restrict__ logits, const float* __restrict__ boxes, const int64_t* __restrict__ labels,
    const float* __restrict__ tgt_boxes, const int32_t* __restrict__ offsets, int N, int T, int Q, int K, int n_tot,
    int n_cap, float w_class, float w_bbox, float w_giou, int64_t* __restrict__ qry, int64_t* __restrict__ tgt,
    float* __restrict__ cost_out) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int lane = threadIdx.x;
  const int l = blockIdx.x / N, b = blockIdx.x - l * N;
  const int off = offsets[b];
  const int n = offsets[b + 1] - off;
  if (n <= 0 || off < 0 || off + n > n_tot) return;       // an empty clip; offsets outside the arrays: nothing is addressed
  int64_t* q_out = qry + size_t(l) * n_tot + off;
  int64_t* t_out = tgt + size_t(l) * n_tot + off;
  if (n > n_cap || n > Q) {                               // more targets than the launch sized its LDS for
    write_unsolved(n, lane, q_out, t_out);
    return;
  }
  const LsapLds s = carve(smem, n, Q);
  const float* lg = logits + (size_t(l) * N + b) * size_t(Q) * K;
  const float* bx = boxes + (size_t(l) * N + b) * size_t(T) * Q * 4;
  float* c_out = cost_out ? cost_out + (size_t(l) * N + b) * size_t(Q) * n_tot + off : nullptr;
  const float frames = float(T);
  bool bad = false;
  for (int t = 0; t < n; ++t) {
    const int64_t label = labels[off + t];
    if (label < 0 || label >= K) { bad = true; continue; }
    const float* tb = tgt_boxes + size_t(off + t) * T * 4;
    for (int q = lane; q < Q; q += kWave) {
      // focal class cost, alpha 0.25, gamma 2 (matcher.py:75-80)
      const float prob = 1.f / (1.f + expf(-lg[size_t(q) * K + label]));
      const float neg = 0.75f * (prob * prob) * -logf(1.f - prob + 1e-8f);
      const float pos = 0.25f * ((1.f - prob) * (1.f - prob)) * -logf(prob + 1e-8f);
      float ssq = 0.f, giou_sum = 0.f;
      for (int f = 0; f < T; ++f) {
        const float* o = bx + (size_t(f) * Q + q) * 4;
        const float ox = o[0], oy = o[1], ow = o[2], oh = o[3];
        const float tx = tb[f * 4], ty = tb[f * 4 + 1], tw = tb[f * 4 + 2], th = tb[f * 4 + 3];
        // distance over the clip's T * 4 coordinates: the targets as they are
        const float dx = ox - tx, dy = oy - ty, dw = ow - tw, dh = oh - th;
        ssq += dx * dx; ssq += dy * dy; ssq += dw * dw; ssq += dh * dh;
        // GIoU: the targets clamped to [1e-7, 1] (matcher.py:68), eps on the hull only (box_ops.py:65-86)
        const float cx = fminf(fmaxf(tx, 1e-7f), 1.f), cy = fminf(fmaxf(ty, 1e-7f), 1.f);
        const float cw = fminf(fmaxf(tw, 1e-7f), 1.f), ch = fminf(fmaxf(th, 1e-7f), 1.f);
        const float ax0 = ox - 0.5f * ow, ay0 = oy - 0.5f * oh, ax1 = ox + 0.5f * ow, ay1 = oy + 0.5f * oh;
        const float bx0 = cx - 0.5f * cw, by0 = cy - 0.5f * ch, bx1 = cx + 0.5f * cw, by1 = cy + 0.5f * ch;
        const float iw = fmaxf(fminf(ax1, bx1) - fmaxf(ax0, bx0), 0.f), ih = fmaxf(fminf(ay1, by1) - fmaxf(ay0, by0), 0.f);
        const float inter = iw * ih;
        const float uni = (ax1 - ax0) * (ay1 - ay0) + (bx1 - bx0) * (by1 - by0) - inter;
        const float hw = fmaxf(fmaxf(ax1, bx1) - fminf(ax0, bx0), 0.f), hh = fmaxf(fmaxf(ay1, by1) - fminf(ay0, by0), 0.f);
        const float hull = hw * hh;
        giou_sum += inter / uni - (hull - uni) / (hull + 1e-7f);
      }
      const float c = w_bbox * sqrtf(ssq) + w_class * (pos - neg) + w_giou * -(giou_sum / frames);
      bad = bad || !isfinite(c);
      s.cost[size_t(t) * Q + q] = c;
      if (c_out) c_out[size_t(q) * n_tot + t] = c;
    }
  }
  if (__any(bad)) {                                       // scipy raises here; a kernel cannot: every target unmatched
    write_unsolved(n, lane, q_out, t_out);
    return;
  }
  if (!lsap_solve_wave(s, n, Q, lane)) {
    write_unsolved(n, lane, q_out, t_out);
    return;
  }
  write_sorted_by_long(s, n, lane, q_out, t_out);
}

// ---- the solver alone: cost matrices in device memory, any orientation through strides --------------------------------
__global__ __launch_bounds__(kWave) void lsap_solve_kernel(const float* __restrict__ cost, int rows, int cols,
                                                           int64_t batch_stride, int64_t row_stride, int64_t col_stride,
                                                           int maximize, int64_t* __restrict__ row_ind,
                                                           int64_t* __restrict__ col_ind) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int lane = threadIdx.x;
  const bool rows_short = rows <= cols;                   // scipy transposes when there are more rows than columns
  const int ns = rows_short ? rows : cols, nl = rows_short ? cols : rows;
  const int64_t ss = rows_short ? row_stride : col_stride, ls = rows_short ? col_stride : row_stride;
  const LsapLds s = carve(smem, ns, nl);
  const float* base = cost + int64_t(blockIdx.x) * batch_stride;
  int64_t* r_out = row_ind + size_t(blockIdx.x) * ns;
  int64_t* c_out = col_ind + size_t(blockIdx.x) * ns;
  bool bad = false;
  for (int i = 0; i < ns; ++i)
    for (int j = lane; j < nl; j += kWave) {
      const float c = base[i * ss + j * ls];
      bad = bad || !isfinite(c);
      s.cost[size_t(i) * nl + j] = maximize ? -c : c;
    }
  if (__any(bad) || !lsap_solve_wave(s, ns, nl, lane)) {
    write_unsolved(ns, lane, r_out, c_out);
    return;
  }
  if (rows_short) {
    for (int i = lane; i < ns; i += kWave) { r_out[i] = i; c_out[i] = s.col_of_row[i]; }
  } else {
    write_sorted_by_long(s, ns, lane, r_out, c_out);
  }
}

// more than 64 KB of dynamic LDS has to be asked for, once per kernel (asking twice is harmless)
template <typename Kernel> int allow_full_lds(Kernel kernel, std::atomic<bool>& asked) {
  if (asked.load(std::memory_order_acquire)) return VNX_OK;
  const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, int(kLdsBytes));
  if (e != hipSuccess) {
    set_error("lsap: hipFuncSetAttribute(max dynamic LDS) failed: %s", hipGetErrorString(e));
    return VNX_ERR_LAUNCH;
  }
  asked.store(true, std::memory_order_release);
  return VNX_OK;
}

// the problem's state fits the LDS of a CU
bool lsap_fits(int n_short, int n_long) { return lsap_lds_bytes(n_short, n_long) <= kLdsBytes; }

}  // namespace
}  // namespace vnx

using namespace vnx;

extern "C" int vnx_seqformer_match(const void* logits, const void* boxes, const void* labels, const void* target_boxes,
                                   const void* offsets, int layers, int clips, int frames, int queries, int classes,
                                   int targets_total, int targets_max, float cost_class, float cost_bbox, float cost_giou,
                                   void* query_index, void* target_index, void* cost_out, void* hip_stream) {
  const char* fn = "vnx_seqformer_match";
  if (layers < 0 || clips < 0 || frames < 1 || queries < 1 || classes < 1 || targets_total < 0 || targets_max < 0 ||
      targets_max > targets_total) {
    set_error("%s: bad sizes (layers %d, clips %d, frames %d, queries %d, classes %d, targets %d, largest clip %d)", fn,
              layers, clips, frames, queries, classes, targets_total, targets_max);
    return VNX_ERR_INVALID_ARGUMENT;
  }
  if (layers == 0 || clips == 0 || targets_total == 0) return VNX_OK;
  if (targets_max > queries || !lsap_fits(targets_max, queries)) {
    set_error("%s: %d targets of one clip against %d queries: more targets than queries, or more than the LDS of a "
              "CU holds", fn, targets_max, queries);
    return VNX_ERR_UNSUPPORTED;
  }
  if (int64_t(layers) * clips >= (int64_t(1) << 31) ||
      int64_t(layers) * clips * queries * (int64_t(classes) > int64_t(frames) * 4 ? classes : frames * 4) >= (int64_t(1) << 40)) {
    set_error("%s: %d x %d problems are outside what the kernel addresses", fn, layers, clips);
    return VNX_ERR_UNSUPPORTED;
  }
  if (!logits || !boxes || !labels || !target_boxes || !offsets || !query_index || !target_index) {
    set_error("%s: null pointer argument", fn);
    return VNX_ERR_INVALID_ARGUMENT;
  }
  hipStream_t stream = (hipStream_t)hip_stream;
  static std::atomic<bool> asked{false};
  const size_t lds = lsap_lds_bytes(targets_max, queries);
  if (lds > 64 * 1024)
    if (int st = allow_full_lds(seqformer_match_kernel, asked)) return st;
  hipLaunchKernelGGL(seqformer_match_kernel, dim3(layers * clips), dim3(kWave), lds, stream, (const float*)logits,
                     (const float*)boxes, (const int64_t*)labels, (const float*)target_boxes, (const int32_t*)offsets, clips,
                     frames, queries, classes, targets_total, targets_max, cost_class, cost_bbox, cost_giou,
                     (int64_t*)query_index, (int64_t*)target_index, (float*)cost_out);
  return check_launch(fn);
}

extern "C" int vnx_lsap_solve(const void* cost, int batch, int rows, int cols, long long batch_stride, long long row_stride,
                              long long col_stride, int maximize, void* row_index, void* col_index, void* hip_stream) {
  const char* fn = "vnx_lsap_solve";
  if (batch < 0 || rows < 0 || cols < 0) {
    set_error("%s: bad sizes (batch %d, %d x %d)", fn, batch, rows, cols);
    return VNX_ERR_INVALID_ARGUMENT;
  }
  if (batch == 0 || rows == 0 || cols == 0) return VNX_OK;
  if (!lsap_fits(rows < cols ? rows : cols, rows < cols ? cols : rows)) {
    set_error("%s: a %d x %d problem does not fit the LDS of a CU", fn, rows, cols);
    return VNX_ERR_UNSUPPORTED;
  }
  if (!cost || !row_index || !col_index) {
    set_error("%s: null pointer argument", fn);
    return VNX_ERR_INVALID_ARGUMENT;
  }
  hipStream_t stream = (hipStream_t)hip_stream;
  static std::atomic<bool> asked{false};
  const size_t lds = lsap_lds_bytes(rows < cols ? rows : cols, rows < cols ? cols : rows);
  if (lds > 64 * 1024)
    if (int st = allow_full_lds(lsap_solve_kernel, asked)) return st;
  hipLaunchKernelGGL(lsap_solve_kernel, dim3(batch), dim3(kWave), lds, stream, (const float*)cost, rows, cols,
                     int64_t(batch_stride), int64_t(row_stride), int64_t(col_stride), int(maximize != 0), (int64_t*)row_index,
                     (int64_t*)col_index);
  return check_launch(fn);
}
