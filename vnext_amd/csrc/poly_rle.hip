// poly_rle.hip -- COCO polygons to run tables on the device: pycocotools' frPyObjects (rleFrPoly) + merge (the union) for
// one annotation per workgroup (host specification, step by step: vnext_amd/ops/poly_rle.py poly_counts_host /
// merge_counts_host / object_counts_host; the kernel is held to them count for count).
//
// Tables: coords double [n_coords], the polygons' x0, y0, x1, y1, ... back to back; poly_rows int32 [n_polys][4] =
// {coordinate offset, vertices, object, 0}; obj_rows int32 [n_objects][6] = {first polygon, polygons, run-slot offset, slot
// size, h, w} (the canvas lives in the object's row: an object may have no polygon, which is the empty mask).  Output: the
// run tables of video_iou.hip -- ends / ones slots, rows {offset, runs, pixels, area} -- and a status word per object.
//
// One wave64 (one workgroup of 64) per object; per polygon, in LDS:
//   1. vertices: X = (int)(5 x + 0.5), Y likewise (the cast truncates toward zero), the ring closed;
//   2. a wave scan of the per-edge dense point counts max(|dX|, |dY|) + 1 gives every edge's first point;
//   3. lanes stride over the dense points: a binary search finds point i's edge, the point is computed as the host does
//      (double; a product, then two additions -- contraction is OFF in this file; the division is IEEE), point i - 1
//      comes from the lane below; a change of u at an upsampled column 5 c + 2 with 0 <= c < w is a crossing at
//      c * h + clamp(ceil((min(v, v') - 2) / 5), 0, h)  (the integer form of the host's two tests);
//      crossings are compacted with __ballot + popcount;
//   4. a bitonic sort of the crossings, then positions of odd multiplicity below h * w stay (even-odd parity is per
//      polygon): the polygon's toggles.  They are appended to the object's event list as {position, start / end} keys; a
//      polygon with an odd number of toggles closes at h * w.
// Then the union: the events of all polygons sorted (starts before ends at one position), a wave scan of +1 / -1 gives the
// coverage, a start from coverage 0 or an end back to 0 toggles the union.  The toggles, then h * w, are the run ends; a
// slot longer than the runs is padded with ends = h * w and ones = the area (zero-length runs, legal for every consumer).
// No atomics, no workspace, no allocation, no synchronisation; every word is written by one lane: bit-identical run to run.
//
// Caps (vnext_hip.h), so that no table can make a wave loop for long: VNX_POLY_RLE_MAX_VERTICES per polygon,
// VNX_POLY_RLE_MAX_POINTS dense points and VNX_POLY_RLE_MAX_POLYGONS polygons per object, VNX_POLY_RLE_MAX_CROSSINGS
// crossings per polygon, events per object and (+ 1) words per run slot.  Beyond them: VNX_POLY_RLE_CAP, the empty table.
#include "vnx_common.h"

#pragma clang fp contract(off)

namespace vnx {

constexpr int kPolyVerts = VNX_POLY_RLE_MAX_VERTICES;
constexpr int kPolyCross = VNX_POLY_RLE_MAX_CROSSINGS;
constexpr int kPolyPoints = VNX_POLY_RLE_MAX_POINTS;
constexpr int kPolyPolys = VNX_POLY_RLE_MAX_POLYGONS;
constexpr double kPolyCoordLimit = 16777216.0;     // 2^24: 5 c + 0.5 and every difference of two of them stay in int32

struct PolyLds {
  int32_t X[kPolyVerts + 1], Y[kPolyVerts + 1], first[kPolyVerts + 1];
  int32_t cross[kPolyCross];                       // a polygon's crossings; at the end the union's toggles
  uint32_t events[kPolyCross];                     // the object's events: position * 2 + (1 for an end)
};

__device__ __forceinline__ int64_t poly_scan_i64(int64_t v, int lane) {           // inclusive
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int64_t o = __shfl_up(v, d, 64);
    v += lane >= d ? o : 0;
  }
  return v;
}

__device__ __forceinline__ int poly_scan_i32(int v, int lane) {                   // inclusive
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int o = __shfl_up(v, d, 64);
    v += lane >= d ? o : 0;
  }
  return v;
}

__device__ __forceinline__ uint64_t lanes_below(int lane) { return (uint64_t(1) << lane) - 1u; }

// ascending bitonic sort of s[0, n) by the one wave of the workgroup; s has room for the next power of two (<= kPolyCross)
template <typename T>
__device__ __forceinline__ void poly_sort(T* s, int n, T pad, int lane) {
  if (n < 2) return;                               // wave-uniform
  int n2 = 2;
  while (n2 < n) n2 <<= 1;
  for (int i = n + lane; i < n2; i += 64) s[i] = pad;
  __syncthreads();
  for (int k = 2; k <= n2; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int t = lane; t < (n2 >> 1); t += 64) {
        const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));                      // bit j clear
        const int p = i | j;
        const T a = s[i], b = s[p];
        if ((a > b) == ((i & k) == 0)) {
          s[i] = b;
          s[p] = a;
        }
      }
      __syncthreads();
    }
  }
}

__device__ __forceinline__ int ceil_div5(int a) { return a >= 0 ? (a + 4) / 5 : -((-a) / 5); }

__global__ void __launch_bounds__(64) poly_rle_kernel(const double* __restrict__ coords, int64_t n_coords,
                                                      const int4* __restrict__ poly_rows, int n_polys,
                                                      const int32_t* __restrict__ obj_rows, int n_objects,
                                                      int32_t* __restrict__ ends, int32_t* __restrict__ ones,
                                                      int64_t run_slots, int32_t* __restrict__ rows,
                                                      int32_t* __restrict__ status) {
  __shared__ PolyLds L;
  const int lane = threadIdx.x;
  const int m = blockIdx.x;
  if (m >= n_objects) return;
  const int32_t* orow = obj_rows + 6 * int64_t(m);
  const int first_poly = orow[0];
  int npoly = orow[1];
  int64_t roff = orow[2], slot = orow[3];
  const int h = orow[4], w = orow[5];
  uint32_t st = 0;
  int64_t hw = int64_t(h) * w;
  if (h < 1 || w < 1 || hw >= (int64_t(1) << 31)) {
    st |= VNX_POLY_RLE_BAD_SIZE;
    hw = 0;
  }
  if (roff < 0 || slot < 0 || roff > run_slots || slot > run_slots - roff) {     // a slot outside the run arenas
    st |= VNX_POLY_RLE_BAD_SLOT;
    roff = 0;
    slot = 0;
  }
  if (slot > kPolyCross + 1) {                     // no table of this kernel needs more; the words beyond stay unwritten
    st |= VNX_POLY_RLE_CAP;
    slot = kPolyCross + 1;
  }
  if (npoly < 0 || first_poly < 0 || first_poly > n_polys || npoly > n_polys - first_poly) {
    st |= VNX_POLY_RLE_BAD_SLOT;
    npoly = 0;
  }
  if (npoly > kPolyPolys) {
    st |= VNX_POLY_RLE_CAP;
    npoly = 0;
  }

  int n_events = 0;
  int64_t object_points = 0;
  // every condition below is wave-uniform, so the barriers inside are reached by all 64 lanes or by none
  for (int q = 0; q < npoly && st == 0; ++q) {
    const int4 pr = poly_rows[first_poly + q];     // {coordinate offset, vertices, object, 0}
    const int k = pr.y;
    if (pr.z != m || pr.x < 0 || k < 0 || pr.x > n_coords || 2 * int64_t(k) > n_coords - pr.x) {
      st |= VNX_POLY_RLE_BAD_SLOT;
      break;
    }
    if (k < 3) {
      st |= VNX_POLY_RLE_FEW_VERTICES;
      break;
    }
    if (k > kPolyVerts) {
      st |= VNX_POLY_RLE_CAP;
      break;
    }
    // 1. vertices
    const double* xy = coords + pr.x;
    bool bad = false;
    for (int j = lane; j < k; j += 64) {
      const double x = xy[2 * j], y = xy[2 * j + 1];
      const bool ok = fabs(x) <= kPolyCoordLimit && fabs(y) <= kPolyCoordLimit;  // false for a NaN
      bad |= !ok;
      L.X[j] = ok ? int(5.0 * x + 0.5) : 0;
      L.Y[j] = ok ? int(5.0 * y + 0.5) : 0;
    }
    if (__ballot(bad)) {
      st |= VNX_POLY_RLE_BAD_COORD;
      break;
    }
    __syncthreads();
    if (lane == 0) {
      L.X[k] = L.X[0];
      L.Y[k] = L.Y[0];
    }
    __syncthreads();
    // 2. the first dense point of every edge
    int64_t total = 0;
    for (int base = 0; base < k; base += 64) {
      const int j = base + lane;
      int64_t c = 0;
      if (j < k) {
        const int dx = abs(L.X[j + 1] - L.X[j]), dy = abs(L.Y[j + 1] - L.Y[j]);
        c = int64_t(dx > dy ? dx : dy) + 1;
      }
      const int64_t incl = poly_scan_i64(c, lane);
      // beyond the cap the stored value is not used: the polygon is flagged before the search reads it
      if (j < k) L.first[j] = int32_t(total + incl - c < kPolyPoints ? total + incl - c : kPolyPoints);
      total += __shfl(incl, 63, 64);
    }
    object_points += total;
    if (object_points > kPolyPoints) {
      st |= VNX_POLY_RLE_CAP;
      break;
    }
    __syncthreads();
    // 3. crossings
    int n_cross = 0, carry_u = 0, carry_v = 0;
    const int points = int(total);
    for (int base = 0; base < points; base += 64) {
      const int i = base + lane;
      const bool in = i < points;
      int u = 0, v = 0;
      if (in) {
        int lo = 0, hi = k - 1;                    // the last edge whose first point is <= i
        while (lo < hi) {
          const int mid = (lo + hi + 1) >> 1;
          if (L.first[mid] <= i) lo = mid;
          else hi = mid - 1;
        }
        const int d = i - L.first[lo];
        int xs = L.X[lo], ys = L.Y[lo], xe = L.X[lo + 1], ye = L.Y[lo + 1];
        const int dx = abs(xe - xs), dy = abs(ys - ye);
        const bool xmajor = dx >= dy;
        const bool flip = (xmajor && xs > xe) || (!xmajor && ys > ye);
        if (flip) {
          int t = xs; xs = xe; xe = t;
          t = ys; ys = ye; ye = t;
        }
        const int n = xmajor ? dx : dy;
        const int t = flip ? n - d : d;
        // a zero-length edge: 0 / 0 in the original; its one point's v is never read (u equals both neighbours')
        const double s = n == 0 ? 0.0 : xmajor ? double(ye - ys) / double(dx) : double(xe - xs) / double(dy);
        if (xmajor) {
          u = t + xs;
          const double p = s * double(t);
          const double a = double(ys) + p;
          v = int(a + 0.5);
        } else {
          v = t + ys;
          const double p = s * double(t);
          const double a = double(xs) + p;
          u = int(a + 0.5);
        }
      }
      int pu = __shfl_up(u, 1, 64), pv = __shfl_up(v, 1, 64);
      if (lane == 0) {
        pu = carry_u;
        pv = carry_v;
      }
      carry_u = __shfl(u, 63, 64);
      carry_v = __shfl(v, 63, 64);
      bool hit = in && i >= 1 && u != pu;
      int pos = 0;
      if (hit) {
        const int r = (u < pu ? u : u - 1) - 2;    // column c = r / 5 when r is a multiple of 5
        const int c = r / 5;
        hit = r % 5 == 0 && c >= 0 && c <= w - 1;
        int row = ceil_div5((v < pv ? v : pv) - 2);
        row = row < 0 ? 0 : row > h ? h : row;
        pos = hit ? c * h + row : 0;               // <= (w - 1) * h + h = h * w < 2^31
      }
      const uint64_t hits = __ballot(hit);
      const int rank = n_cross + __popcll(hits & lanes_below(lane));
      if (hit && rank < kPolyCross) L.cross[rank] = pos;
      n_cross += __popcll(hits);
    }
    if (n_cross > kPolyCross) {
      st |= VNX_POLY_RLE_CAP;
      break;
    }
    __syncthreads();
    // 4. sort; positions of odd multiplicity below h * w are this polygon's toggles
    poly_sort<int32_t>(L.cross, n_cross, 0x7fffffff, lane);
    int n_tog = 0, carry_g = 0;
    for (int base = 0; base < n_cross; base += 64) {
      const int i = base + lane;
      const bool in = i < n_cross;
      const int val = in ? L.cross[i] : 0;
      const bool is_first = in && (i == 0 || L.cross[i - 1] != val);
      const bool is_last = in && (i == n_cross - 1 || L.cross[i + 1] != val);
      const uint64_t firsts = __ballot(is_first);
      const uint64_t upto = firsts & (lanes_below(lane) | (uint64_t(1) << lane));
      const int g = upto ? base + (63 - __clzll(upto)) : carry_g;                // the first index of i's group
      if (firsts) carry_g = base + (63 - __clzll(firsts));
      const bool keep = is_last && ((i - g + 1) & 1) && val < hw;
      const uint64_t keeps = __ballot(keep);
      const int r = n_tog + __popcll(keeps & lanes_below(lane));
      if (keep && n_events + r < kPolyCross) L.events[n_events + r] = uint32_t(val) * 2u + uint32_t(r & 1);
      n_tog += __popcll(keeps);
    }
    if (n_tog & 1) {                               // the last set run reaches the end of the canvas
      if (lane == 0 && n_events + n_tog < kPolyCross) L.events[n_events + n_tog] = uint32_t(hw) * 2u + 1u;
      ++n_tog;
    }
    n_events += n_tog;
    if (n_events > kPolyCross) {
      st |= VNX_POLY_RLE_CAP;
      break;
    }
    __syncthreads();                               // X, Y, first and cross are rewritten by the next polygon
  }
  __syncthreads();

  // the union: coverage over the sorted events (one polygon's events are sorted as they stand)
  int n_union = 0;
  if (st == 0) {
    if (npoly > 1) poly_sort<uint32_t>(L.events, n_events, 0xffffffffu, lane);
    int cover = 0;
    for (int base = 0; base < n_events; base += 64) {
      const int i = base + lane;
      const bool in = i < n_events;
      const uint32_t key = in ? L.events[i] : 0u;
      const bool is_end = (key & 1u) != 0;
      const int delta = !in ? 0 : is_end ? -1 : 1;
      const int after = cover + poly_scan_i32(delta, lane);
      const int64_t pos = int64_t(key >> 1);
      const bool toggle = in && pos < hw && (is_end ? after == 0 : after - delta == 0);
      const uint64_t toggles = __ballot(toggle);
      const int r = n_union + __popcll(toggles & lanes_below(lane));
      if (toggle && r < kPolyCross) L.cross[r] = int32_t(pos);                   // r < n_events <= kPolyCross
      n_union += __popcll(toggles);
      cover = __shfl(after, 63, 64);
    }
    if (int64_t(n_union) + 1 > slot) st |= VNX_POLY_RLE_BAD_SLOT;                // the slot is too small: nothing of it is kept
  }
  __syncthreads();

  // the slot: ends = the toggles, h * w, then padding; ones = the set pixels below each end.  A flagged object: the empty mask
  const int runs = st ? 0 : n_union + 1;
  int64_t area = 0;
  for (int64_t base = 0; base < slot; base += 64) {
    const int64_t k = base + lane;
    int64_t e = hw, len = 0;
    if (k < runs) {
      const int64_t prev = k > 0 ? L.cross[k - 1] : 0;
      e = k < runs - 1 ? L.cross[k] : hw;
      len = (k & 1) ? e - prev : 0;
    }
    const int64_t below = area + poly_scan_i64(len, lane);
    if (k < slot) {                                // roff + k < roff + slot <= run_slots
      ends[roff + k] = int32_t(e);
      ones[roff + k] = int32_t(below);
    }
    area = __shfl(below, 63, 64);
  }
  if (lane == 0) {
    rows[4 * int64_t(m) + 0] = int32_t(roff);
    rows[4 * int64_t(m) + 1] = runs;
    rows[4 * int64_t(m) + 2] = int32_t(hw);
    rows[4 * int64_t(m) + 3] = st ? 0 : int32_t(area);
    status[m] = int32_t(st);
  }
}

}  // namespace vnx

using namespace vnx;

extern "C" int vnx_poly_rle(const void* coords, long long n_coords, const void* poly_rows, int n_polys,
                            const void* obj_rows, int n_objects, void* ends, void* ones, long long run_slots, void* rows,
                            void* status, void* hip_stream) {
  const char* fn = "vnx_poly_rle";
  if (n_coords < 0 || n_polys < 0 || n_objects < 0 || run_slots < 0) {
    set_error("%s: bad sizes (coords %lld, polygons %d, objects %d, run_slots %lld)", fn, n_coords, n_polys, n_objects,
              run_slots);
    return VNX_ERR_INVALID_ARGUMENT;
  }
  if (run_slots >= (1ll << 31) || n_coords >= (1ll << 31)) {
    set_error("%s: run_slots %lld or coords %lld beyond the int32 offsets", fn, run_slots, n_coords);
    return VNX_ERR_UNSUPPORTED;
  }
  if (n_objects == 0) return VNX_OK;
  if (!obj_rows || !rows || !status || (n_polys > 0 && !poly_rows) || (n_coords > 0 && !coords) ||
      (run_slots > 0 && (!ends || !ones))) {
    set_error("%s: null pointer argument", fn);
    return VNX_ERR_INVALID_ARGUMENT;
  }
  if ((reinterpret_cast<uintptr_t>(poly_rows) & 15) != 0 || (reinterpret_cast<uintptr_t>(coords) & 7) != 0) {
    set_error("%s: poly_rows must be 16-byte aligned, coords 8-byte aligned", fn);
    return VNX_ERR_INVALID_ARGUMENT;
  }
  const dim3 grid{uint32_t(n_objects), 1, 1}, block{64, 1, 1};
  hipLaunchKernelGGL(poly_rle_kernel, grid, block, 0, (hipStream_t)hip_stream, (const double*)coords, int64_t(n_coords),
                     (const int4*)poly_rows, n_polys, (const int32_t*)obj_rows, n_objects, (int32_t*)ends, (int32_t*)ones,
                     int64_t(run_slots), (int32_t*)rows, (int32_t*)status);
  return check_launch(fn);
}
