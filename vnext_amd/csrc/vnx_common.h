// vnx_common.h -- shared device/host helpers for libvnext_hip.so (gfx950 only).
#pragma once

#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>
#include <hip/hip_fp16.h>
#include <stdint.h>

#include "../../include/vnext_hip.h"
#include <atomic>

namespace vnx {

constexpr int kWave = 64;  // CDNA wavefront

// ---- element types ---------------------------------------------------------
struct bf16_t { uint16_t bits; };
struct f16_t { _Float16 v; };

template <typename T> struct acc_of { using type = float; };
template <> struct acc_of<double> { using type = double; };
template <typename T> using acc_t = typename acc_of<T>::type;

__device__ __forceinline__ float to_acc(float x) { return x; }
__device__ __forceinline__ double to_acc(double x) { return x; }
__device__ __forceinline__ float to_acc(bf16_t x) { return __uint_as_float(uint32_t(x.bits) << 16); }
__device__ __forceinline__ float to_acc(f16_t x) { return float(x.v); }

// fp32 -> bf16, round to nearest even: gfx950 has the instruction (v_cvt_pk_bf16_f32, two values per issue; the compiler
// emits it for this vector conversion).  Until round 3 this was integer arithmetic -- ~6 instructions per value, a
// third more vector instructions in the bf16 grad_value kernel than in the fp32 one (PMC: 14.1 M vs 11.0 M per launch at
// decoder-720p), which is why 16-bit values were SLOWER there.
typedef __bf16 vnx_bf16x2_t __attribute__((ext_vector_type(2)));
typedef float vnx_f32x2_t __attribute__((ext_vector_type(2)));
__device__ __forceinline__ uint32_t f32x2_to_bf16x2(float lo, float hi) {       // lo in bits 0..15
  return __builtin_bit_cast(uint32_t, __builtin_convertvector(vnx_f32x2_t{lo, hi}, vnx_bf16x2_t));
}
__device__ __forceinline__ uint16_t f32_to_bf16_bits(float f) { return uint16_t(f32x2_to_bf16x2(f, 0.f)); }

// four consecutive channels of a row as fp32, whatever the storage type (fp32: 16 bytes, bf16 / f16: 8) -- the element-wise kernels
// of the layer stack (add_norm.hip, ffn_act.hip) compute in fp32 and round once on the way out
typedef float vnx_f4 __attribute__((ext_vector_type(4)));
typedef uint32_t vnx_u2 __attribute__((ext_vector_type(2)));
template <typename T> __device__ __forceinline__ vnx_f4 row4_load(const T* p);
template <> __device__ __forceinline__ vnx_f4 row4_load<float>(const float* p) { return *reinterpret_cast<const vnx_f4*>(p); }
template <> __device__ __forceinline__ vnx_f4 row4_load<bf16_t>(const bf16_t* p) {
  const vnx_u2 r = *reinterpret_cast<const vnx_u2*>(p);
  return vnx_f4{__uint_as_float(r.x << 16), __uint_as_float(r.x & 0xffff0000u), __uint_as_float(r.y << 16), __uint_as_float(r.y & 0xffff0000u)};
}
template <> __device__ __forceinline__ vnx_f4 row4_load<f16_t>(const f16_t* p) {
  typedef _Float16 h4 __attribute__((ext_vector_type(4)));
  const h4 r = *reinterpret_cast<const h4*>(p);
  return vnx_f4{float(r.x), float(r.y), float(r.z), float(r.w)};
}
template <typename T> __device__ __forceinline__ void row4_store(T* p, vnx_f4 v);
template <> __device__ __forceinline__ void row4_store<float>(float* p, vnx_f4 v) { *reinterpret_cast<vnx_f4*>(p) = v; }
template <typename T> __device__ __forceinline__ void row4_store_nt(T* p, vnx_f4 v);
template <> __device__ __forceinline__ void row4_store_nt<float>(float* p, vnx_f4 v) { __builtin_nontemporal_store(v, reinterpret_cast<vnx_f4*>(p)); }

template <typename T> __device__ __forceinline__ T from_acc(acc_t<T> x);
template <> __device__ __forceinline__ float from_acc<float>(float x) { return x; }
template <> __device__ __forceinline__ double from_acc<double>(double x) { return x; }
template <> __device__ __forceinline__ bf16_t from_acc<bf16_t>(float x) { return bf16_t{f32_to_bf16_bits(x)}; }
template <> __device__ __forceinline__ f16_t from_acc<f16_t>(float x) { return f16_t{_Float16(x)}; }
template <> __device__ __forceinline__ void row4_store<bf16_t>(bf16_t* p, vnx_f4 v) {
  *reinterpret_cast<vnx_u2*>(p) = vnx_u2{f32x2_to_bf16x2(v.x, v.y), f32x2_to_bf16x2(v.z, v.w)};
}
template <> __device__ __forceinline__ void row4_store<f16_t>(f16_t* p, vnx_f4 v) {
  typedef _Float16 h4 __attribute__((ext_vector_type(4)));
  *reinterpret_cast<h4*>(p) = h4{_Float16(v.x), _Float16(v.y), _Float16(v.z), _Float16(v.w)};
}
template <> __device__ __forceinline__ void row4_store_nt<f16_t>(f16_t* p, vnx_f4 v) {
  typedef _Float16 h4 __attribute__((ext_vector_type(4)));
  __builtin_nontemporal_store(h4{_Float16(v.x), _Float16(v.y), _Float16(v.z), _Float16(v.w)}, reinterpret_cast<h4*>(p));
}
template <> __device__ __forceinline__ void row4_store_nt<bf16_t>(bf16_t* p, vnx_f4 v) {
  __builtin_nontemporal_store(vnx_u2{f32x2_to_bf16x2(v.x, v.y), f32x2_to_bf16x2(v.z, v.w)}, reinterpret_cast<vnx_u2*>(p));
}

// hardware floating-point atomics (global_atomic_add_f32 / _f64), agent scope
__device__ __forceinline__ void atomic_add(float* p, float v) { unsafeAtomicAdd(p, v); }
__device__ __forceinline__ void atomic_add(double* p, double v) { unsafeAtomicAdd(p, v); }

// True when the levels tile [0, S) back to back in order (level_start_index[l] is the
// running sum of H*W and the total is spatial_size).
__device__ __forceinline__ bool levels_packed(const int64_t* shapes, const int64_t* lsi, int L, int S) {
  int64_t running = 0;
  bool ok = true;
  for (int l = 0; l < L; ++l) {
    ok = ok && (lsi[l] == running);
    running += shapes[2 * l] * shapes[2 * l + 1];
  }
  return ok && running == S;
}

__device__ __forceinline__ float floor_acc(float x) { return floorf(x); }
__device__ __forceinline__ double floor_acc(double x) { return floor(x); }

// ---- device helpers more than one op uses ------------------------------------------------------------------------
// sum / maximum over the 64 lanes of a wave, the same on every lane (a fixed exchange tree)
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, 64));
  return v;
}

// The dropout masks of add_norm.hip, ffn_act.hip and self_attn.hip are not stored: keep(element) = hash(seed, element
// index) >= threshold, recomputed by the backward from the same seed -- forward and backward must read ONE hash.
// murmur3-style mix of (element index, 64-bit seed) -> 32 uniform bits
__device__ __forceinline__ uint32_t dropout_hash(uint32_t idx, uint32_t seed_lo, uint32_t seed_hi) {
  uint32_t h = idx ^ seed_lo;
  h *= 0xcc9e2d51u; h = (h << 15) | (h >> 17); h *= 0x1b873593u;
  h ^= seed_hi;
  h ^= h >> 16; h *= 0x85ebca6bu; h ^= h >> 13; h *= 0xc2b2ae35u; h ^= h >> 16;
  return h;
}

// Effective seed of a launch: the host's 64 bits, mixed with a 64-bit word read from DEVICE memory when the caller
// passes one.  A host integer is baked into a captured hipGraph -- every replay of a captured training step would drop
// the same elements -- whereas a device word bumped once per step (by a captured `add_`) gives every replay
// fresh masks; forward and backward of one step read the same word, so the backward still recomputes the mask.
__device__ __forceinline__ void dropout_effective_seed(uint32_t& lo, uint32_t& hi, const unsigned long long* seed_device) {
  if (seed_device == nullptr) return;
  const unsigned long long s = *seed_device;                       // wave-uniform (scalar load)
  uint32_t a = uint32_t(s) * 0x9E3779B1u, b = (uint32_t(s >> 32) + 0x7F4A7C15u) * 0x85EBCA77u;
  a ^= a >> 15; b ^= b >> 13;
  lo ^= a * 0xC2B2AE3Du;
  hi ^= b * 0x27D4EB2Fu + a;
}

inline uint32_t dropout_threshold(float p) {      // host; keep iff hash >= threshold:  P(drop) = threshold / 2^32
  const double t = double(p) * 4294967296.0;
  return t <= 0.0 ? 0u : (t >= 4294967295.0 ? 0xffffffffu : uint32_t(t + 0.5));
}

// A float as an integer with the same order (x < y <=> key(x) < key(y), -0 = +0): with integer keys "before q in (value,
// index) order" is ONE comparison, key_j < key_q + (j < q), and rank counts need no second compare for the ties.  INT_MIN
// only for a NaN payload.  (One float add: a file-level `#pragma clang fp contract(off)` after this header changes nothing.)
__device__ __forceinline__ int order_key(float x) {
  const int b = __float_as_int(x + 0.f);
  return b ^ ((b >> 31) & 0x7fffffff);
}

// a row of n 4-byte items padded to whole 16-byte groups (the LDS layouts of ota_match.hip and det_select.hip)
__host__ __device__ inline int pad4(int n) { return (n + 3) & ~3; }

// ---- host side ---------------------------------------------------------------
void set_error(const char* fmt, ...);
int check_launch(const char* what);

// Kernel-span stamps (measurement aid behind bench.py's roofline).  While a stamp buffer is armed
// (vnx_debug_arm_stamps) every launch of a tuned MSDA kernel is handed a region of 2 x gridDim
// 64-bit slots; each workgroup leaves {its start, its last wave's end} there in constant-rate
// wall-clock ticks (s_memrealtime).  Host side: span = max(end) - min(start) = the kernel's own
// duration on the device, without the inter-kernel gap that event timing around back-to-back
// launches includes.  Per-workgroup slots: no same-address atomics across workgroups.
// nullptr (the normal case) = no stamps.
enum StampKernel { kStampFwd = 1, kStampGradLoc = 2, kStampGradValue = 3, kStampGradPair = 4 };
unsigned long long* take_stamp_region(int kernel, long long blocks);
__device__ __forceinline__ void stamp_begin(unsigned long long* s) {
  if (s && threadIdx.x == 0) s[2 * size_t(blockIdx.x)] = (unsigned long long)wall_clock64();
}
__device__ __forceinline__ void stamp_end(unsigned long long* s) {
  if (s && (threadIdx.x & 63) == 0) atomicMax(s + 2 * size_t(blockIdx.x) + 1, (unsigned long long)wall_clock64());
}
// ---- the kernel variant of a call ---------------------------------------------------------------------------------
// The PRODUCT library has one: every field at its default, the choice made from the call's own sizes.  The forced
// configurations, the archived kernels and the timing ablations (which return wrong results by construction) exist only in
// the development build (-DVNX_DEV_VARIANTS, libvnext_hip_dev.so, include/vnext_hip_dev.h), where vnx_set_kernel_variant
// sets a process-wide integer.  Each exported entry point reads it ONCE and hands the decoded struct, or
// the fields a callee needs, down: a value set while a call runs cannot give a call that is half one configuration and half
// another.  The numbers appear in decode_variant() and nowhere else.
struct FwdCfg { int qpw; int wpb; };      // queries per wave, waves per workgroup of the forward / grad_loc kernel; qpw 0 = by size (pick_fwd_cfg)
enum class GvPath { Auto, Records, Tiles };
struct KernelVariant {
  bool generic = false;              // the generic kernels, forward and backward
  // the tuned forward (msda_d32.hip: launch_fwd_cfg)
  FwdCfg fwd_cfg{0, 0};
  bool fwd_prefetch = false;         // its phase 0 (off since the measurement beside launch_fwd_cfg)
  int fwd_head_rot = 0;              // A/B record: which head runs on which XCD (the kernel's prefetch_rows >> 16)
  bool fwd_lpr8 = false;             // 16-bit rows as 8 lanes x 8 B instead of 4 x 16 B
  int slab_fwd = 0;                  // the slab forward (and the slab grad_loc kernel with it): +1 forced, -1 forbidden, 0 by size
  bool large_slab = false;           // 16-bit values: the large slab
  int tile_fwd = 0, tile_fwd_debug = 0;      // the archived LDS-staged forwards (tools/experiments/msda_tile/): 1 / 2, 0 = none; the first one's stamp mode
  // the backward (capi.hip: plan_backward)
  FwdCfg gl_cfg{0, 0};               // the grad_loc kernel's configuration
  bool atomics_backward = false;     // the one-kernel backward whose grad_value goes through global atomics
  // TIMING ABLATIONS: grad_loc / grad_attn alone; grad_value alone on the record- and tile-fed paths / on the self-decoding path
  bool only_gl = false, only_gv = false, only_gv_direct = false;
  int gv_units = 0;                  // grad_value units per level at least (gv_units_min); 0 = the path's own
  GvPath gv_path = GvPath::Auto;     // record- or tile-fed grad_value whatever the query count
  int rec_stamps = 0, rec_form = 0;  // the record-fed kernel's phase stamps (debug mode) and form (launch_gvrec's mode)
  bool tile_copy = false;            // tile path: the grad_loc kernel leaves a compact copy of the locations / weights
  bool fork = false, no_pair = false;      // self-decoding path: grad_value on the side stream, as VNX_MSDA_FORK asks; two launches where the paired kernel would run
  int pair_order = -1;               // the paired kernel's role order (msda_d32.hip); -1 = the launcher's choice
  // the gather form of the grad_loc kernel where the slab form would run; the slab form of the fused one (measured, not the product path)
  bool no_slab_backward = false, fused_slab_backward = false;
  // the mask head's forward (mask_head.hip)
  int mh_runs = 0;                   // runs per instance; 0 = by size (mask_head_runs)
  bool mh_strip = false;             // the strip kernel of rounds 1 - 3
};
#ifdef VNX_DEV_VARIANTS
extern std::atomic<int> g_kernel_variant;
inline KernelVariant decode_variant(int variant) {
  KernelVariant k;
  // configuration numbers c of the forward / grad_loc kernel: 2..5 = 8, 4, 2, 1 queries per wave with 4 waves per workgroup,
  // 12..15 the same with 1 wave; 20 + c / 40 + c wrap them (the forward's prefetch on / off); 60..68 take 13; others by size
  auto cfg = [](int c) {
    if (c >= 20 && c < 60) c = (c - 20) % 20;
    if (c >= 60 && c < 69) c = 13;
    if (c >= 2 && c <= 5) return FwdCfg{8 >> (c - 2), 4};
    if (c >= 12 && c <= 15) return FwdCfg{8 >> (c - 12), 1};
    return FwdCfg{0, 0};
  };
  k.generic = variant == 1;
  if (variant < 100) {                                   // 2..69: the forward's and the grad_loc kernel's shape
    k.fwd_cfg = cfg(variant);
    k.fwd_prefetch = variant >= 20 && variant < 40;      // (40..59: off, as by default)
    if (variant >= 60 && variant <= 68) k.fwd_head_rot = variant == 68 ? 14 : variant - 60;      // 14: the fixed head -> XCD map
    k.fwd_lpr8 = variant == 69;
  }
  k.only_gl = variant >= 100 && variant < 200;           // 100 + c
  k.atomics_backward = variant >= 300 && variant < 400;  // 300 + c
  // the configuration number the backward carries; the slab grad_loc kernel stands in for configuration 0 only
  const int c = variant < 100 ? variant : k.only_gl ? variant - 100 : 0;
  k.gl_cfg = cfg(k.atomics_backward ? variant - 300 : c);
  if (variant >= 200 && variant < 300)                   // 200 + units (1..16)
    k.gv_units = variant - 200 < 1 ? 1 : (variant - 200 > 16 ? 16 : variant - 200);
  k.only_gv = (variant >= 400 && variant < 430) || (variant > 431 && variant < 500);
  k.rec_stamps = variant == 408 ? 1 : variant == 412 ? 5 : 0;      // shader-clock / wall-clock ticks
  k.rec_form = variant == 420 ? 1 : variant == 425 ? 3 : 0;        // the LDS-slab form / the register slab without selection
  // 430 / 431 force records / tiles; the numbers that name a record-fed kernel keep it
  if (variant == 430 || k.rec_stamps || k.rec_form) k.gv_path = GvPath::Records;
  if (variant == 431) k.gv_path = GvPath::Tiles;
  k.fork = variant == 441;
  k.only_gv_direct = variant == 442;
  k.no_pair = variant == 444;
  if (variant >= 445 && variant <= 447) k.pair_order = variant - 445;      // grad_value groups first / grad_loc groups first / alternating
  k.tile_copy = variant == 510;
  // 700..702 and 720 select an archived MSDA forward, 701..798 the mask head's runs and 799 its strip kernel: the two
  // kernel families decode the same range, so 701 / 702 set a field of each (no test or tool runs both under one number)
  if (variant >= 700 && variant <= 702) { k.tile_fwd = 1; k.tile_fwd_debug = variant - 700; }
  if (variant == 720) k.tile_fwd = 2;
  if (variant > 700 && variant < 799) k.mh_runs = variant - 700;
  k.mh_strip = variant == 799;
  k.slab_fwd = variant == 730 ? 1 : variant == 731 ? -1 : 0;
  k.no_slab_backward = variant == 733 || c != 0;
  k.fused_slab_backward = variant == 734;
  k.large_slab = variant == 737;
  return k;
}
inline KernelVariant kernel_variant() { return decode_variant(g_kernel_variant.load(std::memory_order_relaxed)); }
#else
constexpr KernelVariant kernel_variant() { return KernelVariant{}; }
#endif

// ---- buffer descriptors ---------------------------------------------------------------------
__device__ __forceinline__ __amdgpu_buffer_rsrc_t make_rsrc(const void* base, uint32_t bytes) {
  // wave-uniform inputs only (callers pass readfirstlane'd values)
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), 0, int(bytes), 0x00020000);
}

// Descriptor over [base, base+bytes) whose words the compiler can prove wave-uniform
// (readfirstlane of both pointer halves; through uint32_t so nothing sign-extends).
__device__ __forceinline__ __amdgpu_buffer_rsrc_t uniform_rsrc(const void* base, uint32_t bytes) {
  const uint32_t lo = uint32_t(__builtin_amdgcn_readfirstlane(int(uint32_t(uintptr_t(base)))));
  const uint32_t hi = uint32_t(__builtin_amdgcn_readfirstlane(int(uint32_t(uintptr_t(base) >> 32))));
  const uint32_t n = uint32_t(__builtin_amdgcn_readfirstlane(int(bytes)));
  return make_rsrc(reinterpret_cast<const void*>(uintptr_t(lo) | (uintptr_t(hi) << 32)), n);
}

inline int elem_size(int dtype) {
  switch (dtype) {
    case VNX_F32: return 4;
    case VNX_F64: return 8;
    case VNX_BF16: return 2;
    case VNX_F16: return 2;
    default: return 0;
  }
}

}  // namespace vnx
