// lsap_wave.h -- the assignment solver of one wave64 (shortest augmenting paths with fp64 duals: the algorithm, its tie
// rule and its LDS layout are described at the top of lsap.hip).  Shared by lsap.hip (one problem per workgroup of one
// wave) and clip_link.hip (one wave of a larger workgroup solves while the others wait at the next barrier).
#pragma once

#include <limits.h>

#include "vnx_common.h"

namespace vnx {

__host__ __device__ constexpr size_t lsap_lds_bytes(int ns, int nl) {
  return size_t(ns) * 12 + size_t(nl) * 28 + size_t(ns) * size_t(nl) * 4;
}

// Lanes of one wave hand values to each other through LDS: order the accesses for the compiler and the memory
// pipeline; the lanes themselves run in lockstep, so no s_barrier is involved.
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

struct LsapLds {
  double* u;          // [ns] dual of a short-side element
  double* v;          // [nl] dual of a long-side element
  double* path_cost;  // [nl] shortest path cost found so far in this augmentation
  int* path;          // [nl] predecessor (short side) on that path
  int* row_of_col;    // [nl] short element assigned to a long one, -1 = free
  int* done;          // [nl] column already scanned in this augmentation
  int* col_of_row;    // [ns] long element assigned to a short one
  float* cost;        // [ns][nl]
};

__device__ __forceinline__ LsapLds carve(unsigned char* smem, int ns, int nl) {
  LsapLds s;
  s.u = reinterpret_cast<double*>(smem);
  s.v = s.u + ns;
  s.path_cost = s.v + nl;
  s.path = reinterpret_cast<int*>(s.path_cost + nl);
  s.row_of_col = s.path + nl;
  s.done = s.row_of_col + nl;
  s.col_of_row = s.done + nl;
  s.cost = reinterpret_cast<float*>(s.col_of_row + ns);
  return s;
}

// s.cost holds the problem.  On return col_of_row / row_of_col hold the assignment.  false: no augmenting path (cannot
// happen with finite costs; the test is what bounds every loop).
__device__ inline bool lsap_solve_wave(const LsapLds& s, int ns, int nl, int lane) {
  const double inf = __builtin_huge_val();
  for (int j = lane; j < nl; j += kWave) { s.v[j] = 0.0; s.row_of_col[j] = -1; }
  for (int i = lane; i < ns; i += kWave) { s.u[i] = 0.0; s.col_of_row[i] = -1; }
  wave_sync();
  for (int cur = 0; cur < ns; ++cur) {
    for (int j = lane; j < nl; j += kWave) { s.path_cost[j] = inf; s.done[j] = 0; }
    double min_val = 0.0;
    int i = cur, sink = -1;
    // cur elements are assigned: the path visits at most cur + 1 columns
    for (int step = 0; step <= cur && sink < 0; ++step) {
      const double ui = s.u[i];
      const float* row = s.cost + size_t(i) * nl;
      double best = inf;
      int best_j = INT_MAX;
      for (int j = lane; j < nl; j += kWave) {
        if (s.done[j]) continue;
        const double r = min_val + double(row[j]) - ui - s.v[j];
        double p = s.path_cost[j];
        if (r < p) { s.path_cost[j] = p = r; s.path[j] = i; }
        if (p < best) { best = p; best_j = j; }          // ascending j: a tie keeps the lower column
      }
      for (int off = 32; off > 0; off >>= 1) {
        const double ov = __shfl_xor(best, off, kWave);
        const int oj = __shfl_xor(best_j, off, kWave);
        if (ov < best || (ov == best && oj < best_j)) { best = ov; best_j = oj; }
      }
      if (best_j == INT_MAX) return false;
      min_val = best;
      if ((best_j & (kWave - 1)) == lane) s.done[best_j] = 1;
      const int r = s.row_of_col[best_j];
      if (r < 0) sink = best_j; else i = r;
    }
    if (sink < 0) return false;
    // duals: every scanned column, and the short element it was assigned to (the sink's own difference is zero)
    for (int j = lane; j < nl; j += kWave) {
      if (!s.done[j]) continue;
      const double d = min_val - s.path_cost[j];
      s.v[j] -= d;
      const int r = s.row_of_col[j];
      if (r >= 0) s.u[r] += d;
    }
    if (lane == 0) s.u[cur] += min_val;
    wave_sync();
    if (lane == 0) {      // flip the path back from the sink
      int j = sink;
      for (int hop = 0; hop <= cur; ++hop) {
        const int r = s.path[j];
        s.row_of_col[j] = r;
        const int prev = s.col_of_row[r];
        s.col_of_row[r] = j;
        j = prev;
        if (r == cur) break;
      }
    }
    wave_sync();
  }
  return true;
}

}  // namespace vnx
