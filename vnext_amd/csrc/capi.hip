// capi.hip -- the library-wide part of the extern "C" surface of libvnext_hip.so (include/vnext_hip.h: ABI version,
// status strings, last error, the development build's variant knob, stamps), the MSDA entry points and the vnx_debug_*
// MSDA aids.  MSDA argument validation, kernel selection (plan_backward) and error reporting live here; the MSDA kernels
// themselves are in msda_generic.hip / msda_d32*.hip.  Every other op defines its entry points beside its kernels.
#include <stdarg.h>
#include <stdio.h>

#include "msda_launchers.h"
#include "../../include/vnext_hip_debug.h"
#ifdef VNX_DEV_VARIANTS
#include "../../include/vnext_hip_dev.h"
#endif

namespace vnx {

static thread_local char t_error[512] = "";
#ifdef VNX_DEV_VARIANTS
std::atomic<int> g_kernel_variant{0};   // development build: A/B knob (vnx_set_kernel_variant); every entry point reads it once (vnx_common.h)
#endif

void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(t_error, sizeof t_error, fmt, ap);
  va_end(ap);
}

// The reference only printf()s a failed launch (ms_deform_im2col_cuda.cuh:948-952);
// here it becomes a status the caller must look at.
int check_launch(const char* what) {
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    set_error("%s: launch failed: %s", what, hipGetErrorString(e));
    return VNX_ERR_LAUNCH;
  }
  return VNX_OK;
}

static int check_common(const char* fn, int vdt, int ldt, const void* value,
                        const int64_t* shapes, const int64_t* lsi, const void* loc,
                        const void* attn, const MsdaDims& d) {
  if (elem_size(vdt) == 0) {
    set_error("%s: unknown value_dtype %d", fn, vdt);
    return VNX_ERR_INVALID_ARGUMENT;
  }
  const bool pair_ok = (ldt == vdt) || (ldt == VNX_F32 && (vdt == VNX_BF16 || vdt == VNX_F16));
  if (!pair_ok) {
    set_error("%s: loc_dtype %d must equal value_dtype %d, or be f32 with a 16-bit value", fn,
              ldt, vdt);
    return VNX_ERR_INVALID_ARGUMENT;
  }
  if (d.B < 0 || d.S < 0 || d.Lq < 0 || d.M <= 0 || d.D <= 0 || d.L <= 0 || d.P <= 0) {
    set_error("%s: bad sizes batch=%d spatial=%d heads=%d channels=%d levels=%d query=%d point=%d",
              fn, d.B, d.S, d.M, d.D, d.L, d.Lq, d.P);
    return VNX_ERR_INVALID_ARGUMENT;
  }
  const bool empty = (d.B == 0 || d.Lq == 0);
  if (!shapes || !lsi || (!empty && (!loc || !attn)) || (!empty && d.S > 0 && !value)) {
    set_error("%s: null pointer argument", fn);
    return VNX_ERR_INVALID_ARGUMENT;
  }
  // level-local pixel offsets and per-batch element offsets are 32-bit in the kernels
  if (int64_t(d.S) * d.M * d.D >= (int64_t(1) << 31)) {
    set_error("%s: spatial_size*heads*channels = %lld does not fit 31 bits", fn,
              (long long)(int64_t(d.S) * d.M * d.D));
    return VNX_ERR_UNSUPPORTED;
  }
  return VNX_OK;
}

}  // namespace vnx

using namespace vnx;

namespace vnx {
// Units per level at least, tile-fed path.  1 since round 4: a level that fits one unit (<= 256 pixels: the coarsest level of
// both pyramids, and the 240-pixel level of 360p) is ONE rectangle cut into query pieces, not two half-rectangles that each
// scan and decode every tile of the level -- with the pieces meeting in partial rows instead of atomics the second row-unit
// buys nothing and costs the level's reads twice: encoder backward 166.5 -> 163.2 us at 360p, 622 -> 611 us at 720p B = 5
// (720p B = 2: 271.4 / 272.1, unchanged).  (Round 3 measured 2 against 1 as 175.2 vs 176.4 us: then the pieces flushed
// through atomics.)  Also re-measured on the partial-row scheme: a piece per 5 chunks instead of 10 190 us, per 20 chunks
// 194 us (360p) / 265.6 us (720p B = 2, - 6); 4 pieces for the middle levels 171 / 293 us.
int gv_units_min(const MsdaDims& d, bool tiles, int forced) {
  if (forced) return forced;
  // Tried with per-unit selection: enough units that each expects about one selection window of
  // samples (10 per level at the encoder shape).  Slower on MI355X -- 353 vs 332 us per encoder-shape
  // backward -- because a unit's chunk count is set by its DISTINCT queries (128 staged rows per
  // chunk), and finer units multiply the (query, unit) incidences.
  (void)d;
  return tiles ? 1 : 2;
}
}  // namespace vnx

// ---- the side stream of the forked backward (include/vnext_hip.h: VNX_MSDA_FORK) -----------------------------------
// One lane per host thread and device, created on first use and kept: a non-blocking stream and two timing-less events.
// Creating them is not a stream operation, but a thread in a global-mode stream capture may not call "unsafe" runtime
// functions: the creation runs in relaxed mode.  No lane (creation failed) = the call stays on the caller's stream.
namespace vnx {
struct SideLane { int device; hipStream_t side; hipEvent_t fork, join; };
static SideLane* side_lane() {
  static thread_local SideLane lanes[16];
  static thread_local int n_lanes = 0;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return nullptr;
  for (int i = 0; i < n_lanes; ++i)
    if (lanes[i].device == dev) return lanes[i].side ? &lanes[i] : nullptr;
  if (n_lanes >= 16) return nullptr;
  SideLane& l = lanes[n_lanes++];
  l = SideLane{dev, nullptr, nullptr, nullptr};
  hipStreamCaptureMode mode = hipStreamCaptureModeRelaxed;
  const bool swapped = hipThreadExchangeStreamCaptureMode(&mode) == hipSuccess;
  bool ok = hipStreamCreateWithFlags(&l.side, hipStreamNonBlocking) == hipSuccess;
  ok = ok && hipEventCreateWithFlags(&l.fork, hipEventDisableTiming) == hipSuccess;
  ok = ok && hipEventCreateWithFlags(&l.join, hipEventDisableTiming) == hipSuccess;
  if (swapped) (void)hipThreadExchangeStreamCaptureMode(&mode);
  if (!ok) {
    (void)hipGetLastError();
    if (l.fork) (void)hipEventDestroy(l.fork);
    if (l.side) (void)hipStreamDestroy(l.side);
    l.side = nullptr;
    return nullptr;
  }
  return &l;
}
}  // namespace vnx

// ---- kernel-span stamps (development build only: include/vnext_hip_dev.h) ----------------------------------------
// The armed buffer is process-wide state, so it does not exist in the product library: there every launch passes a null
// stamp pointer and nothing outside a call's arguments can change what the call does or costs.
#ifdef VNX_DEV_VARIANTS
static unsigned long long* g_stamp_buf = nullptr;
static long long g_stamp_words = 0, g_stamp_used = 0;
static int g_stamp_n = 0;
static int g_stamp_kind[4096];
static long long g_stamp_off[4096], g_stamp_blocks[4096];
#endif
namespace vnx {
unsigned long long* take_stamp_region(int kernel, long long blocks) {
#ifdef VNX_DEV_VARIANTS
  if (!g_stamp_buf || g_stamp_n >= 4096 || g_stamp_used + 2 * blocks > g_stamp_words) return nullptr;
  g_stamp_kind[g_stamp_n] = kernel;
  g_stamp_off[g_stamp_n] = g_stamp_used;
  g_stamp_blocks[g_stamp_n] = blocks;
  ++g_stamp_n;
  unsigned long long* p = g_stamp_buf + g_stamp_used;
  g_stamp_used += 2 * blocks;
  return p;
#else
  (void)kernel; (void)blocks;
  return nullptr;
#endif
}
}  // namespace vnx

extern "C" {

int vnx_abi_version(void) { return VNX_ABI_VERSION; }

const char* vnx_status_string(int status) {
  switch (status) {
    case VNX_OK: return "ok";
    case VNX_ERR_INVALID_ARGUMENT: return "invalid argument";
    case VNX_ERR_UNSUPPORTED: return "unsupported shape";
    case VNX_ERR_WORKSPACE: return "workspace missing or too small";
    case VNX_ERR_LAUNCH: return "kernel launch failed";
    default: return "unknown status";
  }
}

const char* vnx_last_error(void) { return t_error; }

#ifdef VNX_DEV_VARIANTS
void vnx_set_kernel_variant(int variant) { g_kernel_variant.store(variant, std::memory_order_relaxed); }
int vnx_get_kernel_variant(void) { return g_kernel_variant.load(std::memory_order_relaxed); }
#endif

#ifdef VNX_DEV_VARIANTS
// buf: device memory of n_words 64-bit words, ZERO-filled by the caller before every measured run
// (slots of workgroups that never ran stay {0, 0} and are skipped); nullptr disarms
void vnx_debug_arm_stamps(void* buf, long long n_words) {
  g_stamp_buf = (unsigned long long*)buf;
  g_stamp_words = n_words;
  g_stamp_used = 0;
  g_stamp_n = 0;
}
// -> number of regions handed out since arming; per region: kernel kind (1 forward, 2
// grad_loc/attn, 3 grad_value), word offset into the buffer, number of workgroups
int vnx_debug_stamp_regions(int* kinds, long long* offsets, long long* blocks, int n) {
  for (int i = 0; i < n && i < g_stamp_n; ++i) {
    kinds[i] = g_stamp_kind[i];
    offsets[i] = g_stamp_off[i];
    blocks[i] = g_stamp_blocks[i];
  }
  return g_stamp_n;
}
#endif
int vnx_debug_wall_clock_khz(void) {
  int dev = 0, khz = 0;
  if (hipGetDevice(&dev) != hipSuccess) return 0;
  if (hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, dev) != hipSuccess) return 0;
  return khz;
}

// The LDS-staged forwards (north-star row n1; tools/experiments/msda_tile/) were measured over
// two rounds against the per-query L2-gather kernel -- 64-65 vs 55 us at encoder-360p, within 2 % at 720p -- and are retired
// from the product build: the development build keeps them reachable (KernelVariant::tile_fwd) with their parity tests.

int vnx_msda_forward(int value_dtype, int loc_dtype, const void* value,
                     const int64_t* spatial_shapes, const int64_t* level_start_index,
                     const void* sampling_loc, const void* attn_weight, void* output, int batch,
                     int spatial_size, int num_heads, int channels, int num_levels, int num_query,
                     int num_point, void* hip_stream) {
  const MsdaDims d{batch, spatial_size, num_heads, channels, num_levels, num_query, num_point};
  int st = check_common("vnx_msda_forward", value_dtype, loc_dtype, value, spatial_shapes,
                        level_start_index, sampling_loc, attn_weight, d);
  if (st != VNX_OK) return st;
  if (batch == 0 || num_query == 0) return VNX_OK;
  if (!output) {
    set_error("vnx_msda_forward: null output");
    return VNX_ERR_INVALID_ARGUMENT;
  }
  hipStream_t stream = (hipStream_t)hip_stream;
  const KernelVariant kv = kernel_variant();
#ifdef VNX_DEV_VARIANTS
  if (kv.tile_fwd == 2 && msda_tile2_fwd_supported(value_dtype, loc_dtype, d))
    return msda_forward_tile2(value, spatial_shapes, level_start_index, sampling_loc, attn_weight, output, d, stream);
  if (kv.tile_fwd == 1 && msda_tile_fwd_supported(value_dtype, loc_dtype, d))
    return msda_forward_tile(value, spatial_shapes, level_start_index, sampling_loc, attn_weight, output, d, nullptr,
                             kv.tile_fwd_debug, stream);
#endif
  if (!kv.generic && msda_d32_fwd_supported(value_dtype, loc_dtype, d))
    return msda_forward_d32(value_dtype, loc_dtype, value, spatial_shapes, level_start_index,
                            sampling_loc, attn_weight, output, d, kv, stream);
  return msda_forward_generic(value_dtype, loc_dtype, value, spatial_shapes, level_start_index,
                              sampling_loc, attn_weight, output, d, stream);
}

// ---- the backward's plan ------------------------------------------------------------------------------------------
// Which kernels a call runs and where each finds its piece of the workspace, decided ONCE per call by plan_backward(): the
// two size functions and the two backwards all ask it, so the size a caller is told and the pointers the kernels are handed
// come from the same numbers.
//   Generic  zero-filled fp32 image + hardware fp32 / fp64 atomics: the generic kernel (development build: or the tuned
//            one-kernel backward with atomics)
//   Pair     below 1 024 queries: both halves as ONE launch where the paired kernel is built for the call (msda_d32.hip:
//            msda_bwd_pair_kernel; fp32, L*P == 16, the one-wave grad_loc configuration -- the decoders' calls): the grad_value
//            units first, the grad_loc work in the remaining workgroups, sharing the GPU without a second queue
//   Direct   below 1 024 queries: grad_value by the self-decoding kernel (msda_d32_gvdirect.hip) -- no records, no tags, no
//            workspace, and no dependence on the grad_loc kernel, so the two may run concurrently (side_lane above)
//   Tiles    from 1 024 queries up (the encoders'): the grad_loc kernel leaves one word per (level, tile of queries),
//            grad_value from the op's inputs and those words (msda_d32_gvtiles.hip)
//   Records  the grad_loc kernel leaves one 16-B geometry record per sample, grad_value by owner-computes units fed by
//            those records with per-unit selection (msda_d32_gvrec.hip)
// Every fast path does nothing on the device unless the levels are packed; unless the caller promised packed levels the
// general path follows (unpacked_levels_tail), each kernel of which does nothing on the device when the levels ARE packed.
// No host sync either way.  (The record-less predecessor of Records -- every unit re-deriving its level's geometry -- and
// the side stream that overlapped it with the grad_loc kernel are archived under tools/experiments/msda_d32_gv.hip.)
enum class BwdPath { Generic, Pair, Direct, Tiles, Records };
// Workspace: [sample records (Records) or tile words (Tiles) | locations, weights | partial rows (Tiles) | fp32 image], every
// region a multiple of 256 B; a region a call does not need has no bytes.
struct MsdaBackwardPlan {
  BwdPath path;
  bool only_gl, only_gv;      // development build, timing ablations: one half of the backward alone
  bool fork, unpacked_tail;   // Direct: grad_value on the side stream between two events; the general path follows the fast one
  int tile_queries;           // Tiles: queries per tile word
  bool copy;                  // the locations / weights region exists (fp32, [batch][head][level][query][point], 12 B per sample)
  // the fp32 [B, S, M, D] image exists: the general path's accumulator for 16-bit values and / or (split_image) the target of
  // the query pieces' atomics (Records, 16-bit values)
  bool image, split_image;
  size_t off_loc, off_attn, off_partials, off_image, total;      // bytes; records / tile words at 0
};

static size_t align256(size_t n) { return (n + 255) & ~size_t(255); }

// fused: the fused prologue's backward (ldt VNX_F32: the decoded locations it leaves; flags VNX_MSDA_LEVELS_PACKED: it
// requires them).  It has its own support check (check_fused), always takes the automatic configuration of the grad_loc
// kernel, and has neither a generic form nor ablations.
static MsdaBackwardPlan plan_backward(int vdt, int ldt, const MsdaDims& d, int flags, const KernelVariant& kv, bool fused) {
  MsdaBackwardPlan p{};
  const bool sixteen = (vdt == VNX_BF16 || vdt == VNX_F16);
  const bool packed = (flags & VNX_MSDA_LEVELS_PACKED) != 0;
  const size_t image_bytes = sixteen ? sizeof(float) * size_t(d.B) * size_t(d.S) * size_t(d.M) * size_t(d.D) : 0;
  if (!fused && (kv.generic || kv.atomics_backward || !msda_d32_bwd_supported(vdt, ldt, d) ||
                 !msda_d32_gvrec_supported(vdt, ldt, d))) {
    p.path = BwdPath::Generic;
    p.image = sixteen;
    p.total = image_bytes;
    return p;
  }
  // Per-sample records (calls with few, scattered queries) or per-tile words (from 1 024 queries up)?  Measured on MI355X,
  // T = 5 encoder calls, model-like locations, cold: see DESIGN.md section 3.3b.  The development build forces records / tiles
  // for A/B runs (KernelVariant::gv_path; the variants that name a record-fed kernel keep it).
  // The self-decoding kernel is built for calls below 1 024 queries: beyond, every unit would re-stage all grad_out rows of
  // its head once per pass of kGvdQc queries, and 16-bit rows would be rounded once per pass -- such calls (L * P != 16 or
  // P != 4 at encoder sizes) keep the record-fed path, which accumulates in fp32.
  const bool records_forced = kv.gv_path == GvPath::Records;
  if (!records_forced && d.P == 4 && d.L * d.P == 16 && msda_d32_gvtiles_supported(vdt, ldt, d) &&
      (kv.gv_path == GvPath::Tiles || d.Lq >= 1024))
    p.path = BwdPath::Tiles;
  else if (!records_forced && d.Lq < 1024 && msda_d32_gvdirect_supported(vdt, ldt, d))
    p.path = BwdPath::Direct;
  else
    p.path = BwdPath::Records;

  size_t at = 0;
  if (p.path == BwdPath::Tiles) {
    p.tile_queries = msda_bwd_tile_queries(d, fused ? FwdCfg{0, 0} : kv.gl_cfg);
    at = align256(msda_gvtiles_summary_bytes(d, p.tile_queries));
  } else if (p.path == BwdPath::Records) {
    at = align256(msda_gvrec_record_bytes(d));
  }
  // Does the grad_loc kernel leave the locations / weights laid out for the grad_value kernel?  The fused backward always
  // does, for the tile-fed and the self-decoding kernel (it has to materialise them anyway -- the two tensors the fused prologue
  // otherwise never holds, 12 B per sample against the records' 16 + 4: 196.7 -> 194.9 us at encoder-360p against the op's own
  // layout), as two regions.  The plain backward does not: the 12 B per sample the grad_loc kernel then writes cost more than
  // the grad_value kernel's tidier reads save (encoder-360p 186 vs 175 us, 720p B = 2 337 vs 322 us, B = 5 664 vs 654 us --
  // although that kernel fetches 2 GB per 720p launch, PMC); the development build forces the copy on the tile path for A/B
  // runs (KernelVariant::tile_copy), as one region with the weights right behind the locations.
  const size_t samples = size_t(d.B) * d.Lq * d.M * d.L * d.P;
  p.copy = fused ? p.path != BwdPath::Records : (p.path == BwdPath::Tiles && kv.tile_copy);
  if (p.copy) {
    p.off_loc = at;
    p.off_attn = at + (fused ? align256(samples * 8) : samples * 8);
    at = fused ? p.off_attn + align256(samples * 4) : at + align256(samples * 12);
  }
  if (p.path == BwdPath::Tiles) {      // the partial rows of the query-split levels' pieces
    p.off_partials = at;
    at += align256(msda_gvtiles_partial_bytes(d));
  }
  // RECORD-fed path with 16-bit values and enough queries for the query split of the coarse levels (gv_query_splits): the
  // pieces of such a level meet through fp32 atomics, which need an fp32 target -- the same [B, S, M, 32] fp32 image the
  // general path of unpacked levels uses (the two never run on the same call: one needs packed levels, the other unpacked
  // ones).  The tile-fed path (every call the models make with >= 1 024 queries) needs none since round 4: its pieces store
  // fp32 partial rows (msda_gvtiles_partial_bytes) and a finishing kernel writes grad_value in its own dtype.
  p.split_image = sixteen && d.P == 4 && d.Lq >= 1024 && p.path == BwdPath::Records;
  // packed levels promised: the general path never runs, no fp32 image -- unless the query split needs it
  p.image = sixteen && (!packed || p.split_image);
  p.off_image = at;
  p.total = at + (p.image ? image_bytes : 0);

  // Development build: grad_loc / grad_attn alone, grad_value alone (timing), fork without the flag, the two launches where
  // the paired kernel would run.
  const bool direct = p.path == BwdPath::Direct;
  p.only_gl = !fused && kv.only_gl;
  p.only_gv = !fused && (direct ? kv.only_gv_direct : kv.only_gv);
  const bool whole = !p.only_gl && !p.only_gv;
  p.fork = direct && whole && ((flags & VNX_MSDA_FORK) || kv.fork);
  p.unpacked_tail = !packed && whole;
  if (direct && !fused && whole && !p.fork && !kv.no_pair && msda_backward_pair_supported(vdt, ldt, d) && (!sixteen || packed))
    p.path = BwdPath::Pair;
  return p;
}

size_t vnx_msda_backward_workspace_bytes(int value_dtype, int loc_dtype, int batch,
                                         int spatial_size, int num_heads, int channels,
                                         int num_levels, int num_query, int num_point, int flags) {
  const MsdaDims d{batch, spatial_size, num_heads, channels, num_levels, num_query, num_point};
  return plan_backward(value_dtype, loc_dtype, d, flags, kernel_variant(), false).total;
}

// The general path behind a fast one: every kernel of it does nothing on the device when the levels ARE packed.  acc: the fp32
// accumulator -- grad_value itself, or the workspace's image for 16-bit values, converted into grad_value at the end.
static int unpacked_levels_tail(int vdt, int ldt, const void* value, const int64_t* shapes, const int64_t* lsi, const void* loc,
                                const void* attn, const void* grad_out, void* acc, void* grad_value, void* grad_loc,
                                void* grad_attn, const MsdaDims& d, hipStream_t stream) {
  const size_t n_value = size_t(d.B) * size_t(d.S) * size_t(d.M) * size_t(d.D);
  const bool image = acc != grad_value;
  int st = zero_if_not_packed(shapes, lsi, d.L, d.S, acc, n_value * (image ? sizeof(float) : size_t(elem_size(vdt))), stream);
  if (st != VNX_OK) return st;
  st = msda_backward_generic(vdt, ldt, value, shapes, lsi, loc, attn, grad_out, acc, grad_loc, grad_attn, d,
                             /*only_if_not_packed=*/1, stream);
  if (st != VNX_OK) return st;
  if (image) return convert_f32_to(vdt, acc, grad_value, int64_t(n_value), shapes, lsi, d.L, d.S, stream);
  return VNX_OK;
}

int vnx_msda_backward(int value_dtype, int loc_dtype, const void* value,
                      const int64_t* spatial_shapes, const int64_t* level_start_index,
                      const void* sampling_loc, const void* attn_weight, const void* grad_output,
                      void* grad_value, void* grad_sampling_loc, void* grad_attn_weight, int batch,
                      int spatial_size, int num_heads, int channels, int num_levels, int num_query,
                      int num_point, int flags, void* workspace, size_t workspace_bytes,
                      void* hip_stream) {
  const MsdaDims d{batch, spatial_size, num_heads, channels, num_levels, num_query, num_point};
  int st = check_common("vnx_msda_backward", value_dtype, loc_dtype, value, spatial_shapes,
                        level_start_index, sampling_loc, attn_weight, d);
  if (st != VNX_OK) return st;
  hipStream_t stream = (hipStream_t)hip_stream;
  const KernelVariant kv = kernel_variant();
  const MsdaBackwardPlan plan = plan_backward(value_dtype, loc_dtype, d, flags, kv, false);
  const size_t n_value = size_t(batch) * size_t(spatial_size) * size_t(num_heads) * size_t(channels);
  if (n_value > 0 && !grad_value) {
    set_error("vnx_msda_backward: null grad_value");
    return VNX_ERR_INVALID_ARGUMENT;
  }
  const bool empty = (batch == 0 || num_query == 0);
  if (plan.total > 0 && !empty && (!workspace || workspace_bytes < plan.total)) {
    set_error("vnx_msda_backward: needs %zu workspace bytes (vnx_msda_backward_workspace_bytes), got %zu",
              plan.total, workspace_bytes);
    return VNX_ERR_WORKSPACE;
  }
  if (!empty && (!grad_output || !grad_sampling_loc || !grad_attn_weight)) {
    set_error("vnx_msda_backward: null gradient pointer");
    return VNX_ERR_INVALID_ARGUMENT;
  }
  if (empty) {  // no queries: the gradient of value is all zeros, the other two are empty
    if (n_value > 0 &&
        hipMemsetAsync(grad_value, 0, n_value * size_t(elem_size(value_dtype)), stream) != hipSuccess) {
      set_error("vnx_msda_backward: hipMemsetAsync failed");
      return VNX_ERR_LAUNCH;
    }
    return VNX_OK;
  }
  char* const ws = (char*)workspace;
  void* const image = plan.image ? (void*)(ws + plan.off_image) : nullptr;
  void* const gv_acc = plan.image ? image : grad_value;      // the generic kernels' fp32 accumulator

  if (plan.path == BwdPath::Generic) {
    // zero-filled image + hardware fp32/fp64 atomics
    const size_t acc_bytes = n_value * (plan.image ? sizeof(float) : size_t(elem_size(value_dtype)));
    if (acc_bytes > 0) {
      const hipError_t e = hipMemsetAsync(gv_acc, 0, acc_bytes, stream);
      if (e != hipSuccess) {
        set_error("vnx_msda_backward: hipMemsetAsync failed: %s", hipGetErrorString(e));
        return VNX_ERR_LAUNCH;
      }
    }
    if (kv.atomics_backward && msda_d32_bwd_supported(value_dtype, loc_dtype, d))
      st = msda_backward_d32(value_dtype, loc_dtype, value, spatial_shapes, level_start_index,
                             sampling_loc, attn_weight, grad_output, gv_acc, grad_sampling_loc,
                             grad_attn_weight, d, /*atomics=*/true, kv, nullptr, nullptr, nullptr, stream);
    else
      st = msda_backward_generic(value_dtype, loc_dtype, value, spatial_shapes, level_start_index,
                                 sampling_loc, attn_weight, grad_output, gv_acc, grad_sampling_loc,
                                 grad_attn_weight, d, /*only_if_not_packed=*/0, stream);
    if (st != VNX_OK) return st;
    if (plan.image)
      return convert_f32_to(value_dtype, image, grad_value, int64_t(n_value), nullptr, nullptr, 0, 0, stream);
    return VNX_OK;
  }

  if (plan.path == BwdPath::Pair) {
    st = msda_backward_pair_d32(value_dtype, value, spatial_shapes, level_start_index, sampling_loc, attn_weight, grad_output,
                                grad_value, grad_sampling_loc, grad_attn_weight, d,
                                kv.pair_order, stream);
    if (st != VNX_OK) return st;
  } else if (plan.path == BwdPath::Direct) {
    // (1) grad_value from the op's own inputs and (2) grad_loc / grad_attn: neither reads what the other writes.  One after
    // the other on the caller's stream -- or, with VNX_MSDA_FORK, (1) on the side stream between two events and (2) on the
    // caller's stream, which then waits for (1).
    // (Launching (2) without the packet's barrier bit -- hipExtAnyOrderLaunch, same stream, no events -- was tried: the flag is
    // not honoured on gfx9 parts (hip_ext.h says so; measured 23.70 vs 23.93 us eager, no overlap in the kernel trace).)
    SideLane* lane = plan.fork ? side_lane() : nullptr;
    if (lane) {
      if (hipEventRecord(lane->fork, stream) != hipSuccess || hipStreamWaitEvent(lane->side, lane->fork, 0) != hipSuccess) {
        (void)hipGetLastError();
        lane = nullptr;
      }
    }
    int st_gv = VNX_OK;
    if (!plan.only_gl)
      st_gv = msda_backward_gvdirect_d32(value_dtype, loc_dtype, spatial_shapes, level_start_index, sampling_loc, attn_weight,
                                         grad_output, grad_value, d, false, lane ? lane->side : stream);
    if (lane && hipEventRecord(lane->join, lane->side) != hipSuccess) {
      set_error("vnx_msda_backward: hipEventRecord on the side stream failed");
      st_gv = VNX_ERR_LAUNCH;
    }
    st = VNX_OK;
    if (!plan.only_gv)
      st = msda_backward_d32(value_dtype, loc_dtype, value, spatial_shapes, level_start_index, sampling_loc, attn_weight,
                             grad_output, nullptr, grad_sampling_loc, grad_attn_weight, d, /*atomics=*/false, kv, nullptr,
                             nullptr, nullptr, stream);
    if (lane && hipStreamWaitEvent(stream, lane->join, 0) != hipSuccess) {      // the join: always, once forked
      set_error("vnx_msda_backward: hipStreamWaitEvent on the caller's stream failed");
      return VNX_ERR_LAUNCH;
    }
    if (st_gv != VNX_OK) return st_gv;
    if (st != VNX_OK) return st;
  } else {
    const bool tiles = plan.path == BwdPath::Tiles;
    void* records = tiles ? nullptr : workspace;
    void* tile_words = tiles ? workspace : nullptr;
    float* tile_copy = plan.copy ? (float*)(ws + plan.off_loc) : nullptr;
    float* split_image = plan.split_image ? (float*)image : nullptr;
    float* partials = tiles ? (float*)(ws + plan.off_partials) : nullptr;
    // records mode: the accumulation-image argument carries the fp32 target of the query pieces' atomics (grad_value itself
    // or the split image), whose rows of the query-split levels the kernel zeroes (gv_query_splits); tile mode: nothing
    st = msda_backward_d32(value_dtype, loc_dtype, value, spatial_shapes, level_start_index,
                           sampling_loc, attn_weight, grad_output,
                           tiles ? nullptr : (value_dtype == VNX_F32 ? grad_value : (void*)split_image), grad_sampling_loc,
                           grad_attn_weight, d, /*atomics=*/false, kv, records, tile_words, tile_copy, stream);
    if (st != VNX_OK) return st;
    if (!plan.only_gl) {
      if (tiles)      // from the compact fp32 copy where the grad_loc kernel left one, from the op's own inputs otherwise
        st = msda_backward_gvtiles_d32(value_dtype, tile_copy ? VNX_F32 : loc_dtype, spatial_shapes, level_start_index,
                                       tile_copy ? (const void*)tile_copy : sampling_loc,
                                       tile_copy ? (const void*)(ws + plan.off_attn) : attn_weight, tile_words, grad_output,
                                       grad_value, d, plan.tile_queries, kv.gv_units, partials, plan.copy, stream);
      else
        st = msda_backward_gvrec_d32(value_dtype, spatial_shapes, level_start_index, records, grad_output,
                                     grad_value, d, kv, split_image, stream);
      if (st != VNX_OK) return st;
      if (split_image) {
        st = msda_split_levels_convert(value_dtype, spatial_shapes, level_start_index, split_image, grad_value, d,
                                       tiles, kv.gv_units, stream);
        if (st != VNX_OK) return st;
      }
    }
  }
  if (plan.unpacked_tail)
    return unpacked_levels_tail(value_dtype, loc_dtype, value, spatial_shapes, level_start_index, sampling_loc, attn_weight,
                                grad_output, gv_acc, grad_value, grad_sampling_loc, grad_attn_weight, d, stream);
  return VNX_OK;
}

// ---- fused prologue (include/vnext_hip.h) -----------------------------------------------------
static int check_fused(const char* fn, int value_dtype, int q_dtype, const MsdaDims& d, int ref_dim, int ref_div) {
  if (d.B < 0 || d.S < 0 || d.M <= 0 || d.D <= 0 || d.L <= 0 || d.Lq < 0 || d.P <= 0) {
    set_error("%s: bad sizes", fn);
    return VNX_ERR_INVALID_ARGUMENT;
  }
  if ((ref_dim != 2 && ref_dim != 4) || ref_div <= 0 || (d.B % ref_div) != 0) {
    set_error("%s: reference points must have 2 or 4 components and batch must be a multiple of "
              "reference_batch_div (got ref_dim=%d, batch=%d, div=%d)", fn, ref_dim, d.B, ref_div);
    return VNX_ERR_INVALID_ARGUMENT;
  }
  if (!msda_d32_fused_supported(value_dtype, q_dtype, d) || !msda_d32_gvrec_supported(value_dtype, q_dtype, d)) {
    set_error("%s: the fused prologue is built for 32-channel heads, levels*points == 16, fp32 or bf16 "
              "(got D=%d, L*P=%d, dtypes %d/%d); use vnx_msda_forward/backward", fn, d.D, d.L * d.P,
              value_dtype, q_dtype);
    return VNX_ERR_UNSUPPORTED;
  }
  return VNX_OK;
}

int vnx_msda_fused_forward(int value_dtype, int query_dtype, const void* value, const int64_t* spatial_shapes,
                           const int64_t* level_start_index, const void* sampling_offsets,
                           const void* attention_logits, const void* reference_points, void* output, int batch,
                           int spatial_size, int num_heads, int channels, int num_levels, int num_query,
                           int num_point, int ref_dim, int reference_batch_div, void* hip_stream) {
  const int ref_f32 = (ref_dim & VNX_MSDA_REF_F32) != 0;      // fp32 reference points beside 16-bit offsets / logits (ABI 14)
  ref_dim &= ~VNX_MSDA_REF_F32;
  const MsdaDims d{batch, spatial_size, num_heads, channels, num_levels, num_query, num_point};
  const int st = check_fused("vnx_msda_fused_forward", value_dtype, query_dtype, d, ref_dim, reference_batch_div);
  if (st != VNX_OK) return st;
  if (batch == 0 || num_query == 0) return VNX_OK;
  if (!value || !spatial_shapes || !level_start_index || !sampling_offsets || !attention_logits ||
      !reference_points || !output) {
    set_error("vnx_msda_fused_forward: null pointer argument");
    return VNX_ERR_INVALID_ARGUMENT;
  }
  const KernelVariant kv = kernel_variant();
#ifdef VNX_DEV_VARIANTS
  if (kv.tile_fwd == 1 && msda_tile_fwd_supported(value_dtype, query_dtype, d)) {
    const FusedArgs fa{reference_points, nullptr, ref_dim, reference_batch_div, nullptr};
    return msda_forward_tile(value, spatial_shapes, level_start_index, sampling_offsets, attention_logits, output, d, &fa, 0,
                             (hipStream_t)hip_stream);
  }
#endif
  return msda_fused_d32(false, value_dtype, query_dtype, value, spatial_shapes, level_start_index, sampling_offsets,
                        attention_logits, nullptr, output, nullptr, d, nullptr, reference_points, nullptr, ref_dim,
                        reference_batch_div, nullptr, nullptr, nullptr, nullptr, kv, (hipStream_t)hip_stream, ref_f32);
}

size_t vnx_msda_fused_backward_workspace_bytes(int value_dtype, int batch, int spatial_size, int num_heads, int num_levels,
                                               int num_query, int num_point) {
  const MsdaDims d{batch, spatial_size, num_heads, 32, num_levels, num_query, num_point};
  // the larger of the two layouts: the variant may change between this call and the backward (A/B runs); the record-fed
  // one needs the fp32 split image for 16-bit values
  KernelVariant records;
  records.gv_path = GvPath::Records;
  const size_t a = plan_backward(value_dtype, VNX_F32, d, VNX_MSDA_LEVELS_PACKED, records, true).total;
  const size_t b = plan_backward(value_dtype, VNX_F32, d, VNX_MSDA_LEVELS_PACKED, KernelVariant{}, true).total;
  return a > b ? a : b;
}

int vnx_msda_fused_backward(int value_dtype, int query_dtype, const void* value, const int64_t* spatial_shapes,
                            const int64_t* level_start_index, const void* sampling_offsets,
                            const void* attention_logits, const void* reference_points, const void* grad_output,
                            void* grad_value, void* grad_sampling_offsets, void* grad_attention_logits,
                            float* grad_reference_points, int batch, int spatial_size, int num_heads,
                            int channels, int num_levels, int num_query, int num_point, int ref_dim,
                            int reference_batch_div, void* workspace, size_t workspace_bytes, void* hip_stream) {
  const int ref_f32 = (ref_dim & VNX_MSDA_REF_F32) != 0;
  ref_dim &= ~VNX_MSDA_REF_F32;
  const MsdaDims d{batch, spatial_size, num_heads, channels, num_levels, num_query, num_point};
  int st = check_fused("vnx_msda_fused_backward", value_dtype, query_dtype, d, ref_dim, reference_batch_div);
  if (st != VNX_OK) return st;
  hipStream_t stream = (hipStream_t)hip_stream;
  if (grad_reference_points && (ref_dim != 2 || reference_batch_div != 1)) {
    set_error("vnx_msda_fused_backward: reference-point gradients are built for 2-d, per-batch references");
    return VNX_ERR_UNSUPPORTED;
  }
  if (grad_reference_points && batch > 0 && num_query > 0 &&
      hipMemsetAsync(grad_reference_points, 0, size_t(batch) * num_query * num_levels * 2 * sizeof(float), stream) !=
          hipSuccess)
    return check_launch("msda_fused_backward memset");
  if (batch == 0 || num_query == 0) {
    // no samples: grad_value is all zeros
    const size_t nbytes = size_t(batch) * spatial_size * num_heads * channels * size_t(elem_size(value_dtype));
    if (nbytes && hipMemsetAsync(grad_value, 0, nbytes, stream) != hipSuccess) return check_launch("memset");
    return VNX_OK;
  }
  if (!value || !spatial_shapes || !level_start_index || !sampling_offsets || !attention_logits ||
      !reference_points || !grad_output || !grad_value || !grad_sampling_offsets || !grad_attention_logits) {
    set_error("vnx_msda_fused_backward: null pointer argument");
    return VNX_ERR_INVALID_ARGUMENT;
  }
  const KernelVariant kv = kernel_variant();
  const MsdaBackwardPlan plan = plan_backward(value_dtype, VNX_F32, d, VNX_MSDA_LEVELS_PACKED, kv, true);
  if (!workspace || workspace_bytes < plan.total) {
    set_error("vnx_msda_fused_backward: workspace of %zu bytes needed (got %zu)", plan.total, workspace_bytes);
    return VNX_ERR_WORKSPACE;
  }
  char* const ws = (char*)workspace;
  const bool tiles = plan.path == BwdPath::Tiles, records = plan.path == BwdPath::Records;
  float* split_image = plan.split_image ? (float*)(ws + plan.off_image) : nullptr;
  float* d_loc = plan.copy ? (float*)(ws + plan.off_loc) : nullptr;
  float* d_attn = plan.copy ? (float*)(ws + plan.off_attn) : nullptr;
  // (1) grad of the Linear outputs (+ reference points), and what the grad_value kernel of the path reads:
  //   Direct   the decoded locations / softmax weights, laid out [batch][head][level][query][point] -- 12 B per sample where
  //            the record-fed kernel was left 16 + 4, no tags to select by, no chunk loop
  //   Tiles    one word per (level, tile of queries) and the decoded locations / weights
  //   Records  the sample records; the fp32 target of the query pieces' atomics is grad_value itself or the split image
  // (2) grad_value from those.  Packed levels are required (no-op on the device otherwise).
  st = msda_fused_d32(true, value_dtype, query_dtype, value, spatial_shapes, level_start_index, sampling_offsets,
                      attention_logits, grad_output, grad_sampling_offsets, grad_attention_logits, d,
                      records ? workspace : nullptr, reference_points, grad_reference_points, ref_dim, reference_batch_div,
                      records ? (value_dtype == VNX_F32 ? grad_value : (void*)split_image) : nullptr,
                      tiles ? workspace : nullptr, d_loc, d_attn, kv, stream, ref_f32);
  if (st != VNX_OK) return st;
  if (plan.path == BwdPath::Direct)
    return msda_backward_gvdirect_d32(value_dtype, VNX_F32, spatial_shapes, level_start_index, d_loc, d_attn, grad_output,
                                      grad_value, d, true, stream);
  if (tiles)
    st = msda_backward_gvtiles_d32(value_dtype, VNX_F32, spatial_shapes, level_start_index, d_loc, d_attn, workspace,
                                   grad_output, grad_value, d, plan.tile_queries, kv.gv_units, (float*)(ws + plan.off_partials),
                                   true, stream);
  else
    st = msda_backward_gvrec_d32(value_dtype, spatial_shapes, level_start_index, workspace, grad_output,
                                 grad_value, d, kv, split_image, stream);
  if (st != VNX_OK) return st;
  if (split_image)
    return msda_split_levels_convert(value_dtype, spatial_shapes, level_start_index, split_image, grad_value, d,
                                     tiles, kv.gv_units, stream);
  return VNX_OK;
}

}  // extern "C"

// ---- unit grid of the tile-fed grad_value kernel, seen from the host (include/vnext_hip_debug.h) -----------
namespace vnx { int msda_gvtiles_units_bound(const MsdaDims& d, int units_min); }
extern "C" int vnx_debug_gvtiles_units(const int64_t* host_shapes, int levels, int num_query, int batch, int heads,
                                       int units_min, int* units_used, int* units_bound, long long* partial_rows_used,
                                       long long* partial_rows_bound) {
  if (!host_shapes || levels <= 0 || !units_used || !units_bound) return VNX_ERR_INVALID_ARGUMENT;
  int64_t S = 0, rows = 0;
  int used = 0;
  for (int l = 0; l < levels; ++l) {
    const int H = int(host_shapes[2 * l]), W = int(host_shapes[2 * l + 1]);
    S += int64_t(H) * W;
    const int units = gv_level_units(H, W, units_min, true);
    const int qs = gv_query_splits(units, num_query, 4, true, batch * heads);      // the kernel's level table
    used += units * qs;
    if (qs > 1) rows += int64_t(qs) * H * W;      // the partial rows the level's query pieces store (gv_partial_rows_bound)
  }
  const MsdaDims d{batch, int(S), heads, 32, levels, num_query, 4};
  *units_used = used;
  *units_bound = vnx::msda_gvtiles_units_bound(d, units_min);
  if (partial_rows_used) *partial_rows_used = rows;
  if (partial_rows_bound) *partial_rows_bound = gv_partial_rows_bound(int(S), levels, batch * heads);
  return VNX_OK;
}

// ---- unit grid of the self-decoding grad_value kernel, seen from the host (include/vnext_hip_debug.h) -----------
namespace vnx { int msda_gvdirect_units_bound(const MsdaDims& d); }
extern "C" int vnx_debug_gvdirect_units(const int64_t* host_shapes, int levels, int num_query, int num_point, int batch_heads,
                                        int* units_used, int* units_bound, int* level_units, int* level_rows_per_unit,
                                        int* level_group_shift) {
  if (!host_shapes || levels <= 0 || num_point <= 0 || !units_used || !units_bound) return VNX_ERR_INVALID_ARGUMENT;
  int64_t S = 0;
  for (int l = 0; l < levels; ++l) S += host_shapes[2 * l] * host_shapes[2 * l + 1];
  const int rows = gvd_rows_max(int(S));
  const int ut = gvd_units_min(int(S), levels, batch_heads, rows);
  int used = 0;
  for (int l = 0; l < levels; ++l) {
    const int H = int(host_shapes[2 * l]), W = int(host_shapes[2 * l + 1]);
    const GvdSplit sp = gvd_level_split(H * W, ut, num_query, num_point, rows);      // the kernel's level table
    used += sp.units;
    if (level_units) level_units[l] = sp.units;
    if (level_rows_per_unit) level_rows_per_unit[l] = sp.rpu;
    if (level_group_shift) level_group_shift[l] = sp.gshift;
  }
  const MsdaDims d{batch_heads, int(S), 1, 32, levels, num_query, num_point};
  *units_used = used;
  *units_bound = vnx::msda_gvdirect_units_bound(d);
  return VNX_OK;
}

// ---- row-gather probe (include/vnext_hip_debug.h) ---------------------------------------------------
namespace vnx {
typedef float probe_f4 __attribute__((ext_vector_type(4)));
template <int NF>
__global__ void __launch_bounds__(256) row_gather_probe_kernel(const probe_f4* __restrict__ rows, const uint32_t* __restrict__ idx,
                                                                size_t n_idx, float* __restrict__ sink) {
  const size_t set = (blockIdx.x * size_t(blockDim.x) + threadIdx.x) >> 3, sets = (size_t(gridDim.x) * blockDim.x) >> 3;
  const int ch = threadIdx.x & 7;
  probe_f4 acc = {0.f, 0.f, 0.f, 0.f};
  for (size_t i = set * NF; i + NF <= n_idx; i += sets * NF) {
    probe_f4 v[NF];
#pragma unroll
    for (int j = 0; j < NF; ++j) v[j] = rows[size_t(idx[i + j]) * 8 + ch];
#pragma unroll
    for (int j = 0; j < NF; ++j) acc += v[j];
  }
  if (acc.x == 1.2345e-31f) { sink[0] = acc.x; sink[1] = acc.y; sink[2] = acc.z; sink[3] = acc.w; }
}
}  // namespace vnx

extern "C" int vnx_debug_row_gather_probe(const void* rows, size_t n_rows, const uint32_t* idx, size_t n_idx, int in_flight,
                                          float* sink, void* hip_stream) {
  if (!rows || !idx || !sink || n_rows == 0) {
    vnx::set_error("vnx_debug_row_gather_probe: null pointer argument");
    return VNX_ERR_INVALID_ARGUMENT;
  }
  hipStream_t st = (hipStream_t)hip_stream;
  const dim3 grid(8192), block(256);
#define VNX_PROBE(NF) hipLaunchKernelGGL((vnx::row_gather_probe_kernel<NF>), grid, block, 0, st, (const vnx::probe_f4*)rows, idx, n_idx, sink)
  if (in_flight >= 8) VNX_PROBE(8); else if (in_flight >= 4) VNX_PROBE(4); else if (in_flight >= 2) VNX_PROBE(2); else VNX_PROBE(1);
#undef VNX_PROBE
  return vnx::check_launch("row_gather_probe");
}
