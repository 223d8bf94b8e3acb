// ap_match.hip -- the greedy detection / ground-truth matching of the COCO-style AP evaluators (COCOeval.evaluateImg,
// YTVOSeval.evaluateVid) for every (image, category) problem of an evaluation, all area ranges and all IoU thresholds
// in one launch (host specification: vnext_amd/ops/ap_match.py match_host).
//
// One wave64 per problem, four problems per workgroup; lane = area range * T + threshold (A * T <= 64 lanes work, the
// others leave).  A lane runs the reference's sequential loop on its own: detections in the given (score) order, each
// taking the ground truth of the highest IoU >= min(threshold, 1 - 1e-10) it may still take, the later one on a tie.
// The reference sorts the ground truths "ignored last, stable" per area range; no sort is made here: a lane walks the
// ground truths it does not ignore in their given order, then -- only when it holds no match yet, which is the
// reference's break -- the ignored ones.  A ground truth is ignored when it is a crowd or its area lies outside the
// lane's range; a matched ground truth is taken again only when it is a crowd.  A detection without a match is ignored
// when its area lies outside the range.
//
// Per lane two bit sets over the problem's ground truths live in LDS (ignored, matched), laid out [word][lane] so that
// the 64 lanes of a wave touch 64 consecutive dwords: no bank conflicts, no barrier (a lane reads only what it wrote).
// No atomics and no workspace: every output element is written by exactly one lane, so the result is a function of
// the input alone.  A row of the problem table that points outside an array writes nothing and sets the status word.
#include "vnx_common.h"

namespace vnx {

constexpr int kApWaves = 4;                                    // problems per workgroup
constexpr int kApWords = VNX_AP_MATCH_MAX_GT / 32;             // bit-set words per lane

__global__ void __launch_bounds__(kApWaves * 64) ap_match_kernel(
    const int64_t* __restrict__ table, int64_t problems, const double* __restrict__ ious, int64_t n_iou,
    const uint8_t* __restrict__ gt_crowd, const double* __restrict__ gt_area, int64_t n_gt,
    const double* __restrict__ dt_area, int64_t n_dt, const double* __restrict__ area_rng, int A,
    const double* __restrict__ thrs, int T, int32_t* __restrict__ dt_match, uint8_t* __restrict__ dt_ignore,
    int32_t* __restrict__ gt_match, uint8_t* __restrict__ gt_ignore, int32_t* __restrict__ status) {
  __shared__ uint32_t s_ign[kApWaves][kApWords][64];
  __shared__ uint32_t s_hit[kApWaves][kApWords][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t p = int64_t(blockIdx.x) * kApWaves + wave;
  if (p >= problems) return;
  const int64_t D = table[5 * p + 0], G = table[5 * p + 1];
  const int64_t dof = table[5 * p + 2], gof = table[5 * p + 3], iof = table[5 * p + 4];
  // each test keeps the next one's arithmetic inside int64: D <= n_dt and G <= VNX_AP_MATCH_MAX_GT bound D * G
  int st = 0;
  if (D < 0 || G < 0 || dof < 0 || gof < 0 || iof < 0 || dof > n_dt || D > n_dt - dof || gof > n_gt ||
      G > n_gt - gof || iof > n_iou)
    st = VNX_AP_MATCH_BAD_TABLE;
  else if (G > VNX_AP_MATCH_MAX_GT)
    st = VNX_AP_MATCH_GT_LIMIT;
  else if (D * G > n_iou - iof)
    st = VNX_AP_MATCH_BAD_TABLE;
  if (st) {
    if (lane == 0) *status = st;                   // several bad rows: one of their codes stays
    return;
  }
  if (lane >= A * T) return;
  const int a = lane / T;
  const double lo = area_rng[2 * a], hi = area_rng[2 * a + 1];
  const double thr = fmin(thrs[lane - a * T], 1 - 1e-10);
  const int g_n = int(G);
  int32_t* gtm = gt_match + int64_t(lane) * n_gt + gof;
  for (int w = 0; w * 32 < g_n; ++w) {
    uint32_t ign = 0;
    for (int g = w * 32; g < g_n && g < w * 32 + 32; ++g) {
      const double ga = gt_area[gof + g];
      ign |= uint32_t(gt_crowd[gof + g] != 0 || ga < lo || ga > hi) << (g & 31);
      gtm[g] = -1;
    }
    s_ign[wave][w][lane] = ign;
    s_hit[wave][w][lane] = 0;
    if (lane == a * T)                             // one lane per area range
      for (int g = w * 32; g < g_n && g < w * 32 + 32; ++g) gt_ignore[int64_t(a) * n_gt + gof + g] = (ign >> (g & 31)) & 1;
  }
  int32_t* dtm = dt_match + int64_t(lane) * n_dt + dof;
  uint8_t* dti = dt_ignore + int64_t(lane) * n_dt + dof;
  for (int64_t d = 0; d < D; ++d) {
    const double* row = ious + iof + d * G;
    double best = thr;
    int m = -1;
    uint32_t ign = 0, hit = 0;
    for (int g = 0; g < g_n; ++g) {                // the ground truths this lane does not ignore (none is a crowd)
      if ((g & 31) == 0) {
        ign = s_ign[wave][g >> 5][lane];
        hit = s_hit[wave][g >> 5][lane];
      }
      if (((ign | hit) >> (g & 31)) & 1) continue;
      const double v = row[g];
      if (v < best) continue;
      best = v;
      m = g;
    }
    int ig;
    if (m < 0) {                                   // no regular match: the ignored ones, crowds again and again
      for (int g = 0; g < g_n; ++g) {
        if ((g & 31) == 0) {
          ign = s_ign[wave][g >> 5][lane];
          hit = s_hit[wave][g >> 5][lane];
        }
        if (!((ign >> (g & 31)) & 1)) continue;
        if (((hit >> (g & 31)) & 1) && gt_crowd[gof + g] == 0) continue;
        const double v = row[g];
        if (v < best) continue;
        best = v;
        m = g;
      }
    }
    if (m >= 0) {
      ig = (s_ign[wave][m >> 5][lane] >> (m & 31)) & 1;
      s_hit[wave][m >> 5][lane] |= uint32_t(1) << (m & 31);
      gtm[m] = int32_t(d);
    } else {
      const double da = dt_area[dof + d];
      ig = da < lo || da > hi;
    }
    dtm[d] = m;
    dti[d] = uint8_t(ig);
  }
}

}  // namespace vnx

using namespace vnx;

extern "C" int vnx_ap_match(const void* table, long long problems, const void* ious, long long n_iou,
                            const void* gt_crowd, const void* gt_area, long long n_gt, const void* dt_area,
                            long long n_dt, const void* area_rng, int n_area, const void* thrs, int n_thrs,
                            void* dt_match, void* dt_ignore, void* gt_match, void* gt_ignore, void* status,
                            void* hip_stream) {
  const char* fn = "vnx_ap_match";
  if (problems < 0 || n_iou < 0 || n_gt < 0 || n_dt < 0 || n_area < 1 || n_thrs < 1) {
    set_error("%s: bad sizes (problems %lld, ious %lld, ground truths %lld, detections %lld, area ranges %d, thresholds %d)",
              fn, problems, n_iou, n_gt, n_dt, n_area, n_thrs);
    return VNX_ERR_INVALID_ARGUMENT;
  }
  if (int64_t(n_area) * n_thrs > VNX_AP_MATCH_MAX_LANES || problems > (1ll << 31) * kApWaves - kApWaves ||
      n_gt >= (1ll << 40) || n_dt >= (1ll << 40)) {
    set_error("%s: %d area ranges x %d thresholds (at most %d per wave), %lld problems, %lld ground truths or %lld "
              "detections beyond the kernel", fn, n_area, n_thrs, VNX_AP_MATCH_MAX_LANES, problems, n_gt, n_dt);
    return VNX_ERR_UNSUPPORTED;
  }
  if (problems == 0) return VNX_OK;
  if (!table || !area_rng || !thrs || !status || (n_iou > 0 && !ious) ||
      (n_gt > 0 && (!gt_crowd || !gt_area || !gt_match || !gt_ignore)) || (n_dt > 0 && (!dt_area || !dt_match || !dt_ignore))) {
    set_error("%s: null pointer argument", fn);
    return VNX_ERR_INVALID_ARGUMENT;
  }
  const dim3 grid{uint32_t((problems + kApWaves - 1) / kApWaves), 1, 1}, block{kApWaves * 64, 1, 1};
  hipLaunchKernelGGL(ap_match_kernel, grid, block, 0, (hipStream_t)hip_stream, (const int64_t*)table, int64_t(problems),
                     (const double*)ious, int64_t(n_iou), (const uint8_t*)gt_crowd, (const double*)gt_area, int64_t(n_gt),
                     (const double*)dt_area, int64_t(n_dt), (const double*)area_rng, n_area, (const double*)thrs, n_thrs,
                     (int32_t*)dt_match, (uint8_t*)dt_ignore, (int32_t*)gt_match, (uint8_t*)gt_ignore, (int32_t*)status);
  return check_launch(fn);
}
