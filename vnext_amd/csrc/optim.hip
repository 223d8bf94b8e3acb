// optim.hip -- the tail of a training step: full-model gradient norm, clip_grad_norm_'s coefficient and the decoupled AdamW
// update of every parameter tensor, in three launches whatever the number of tensors (vnext_amd/ops/optim.py;
// include/vnext_hip.h).
//
// Everything about the tensors is read from MEMORY: a table of vnx_adamw_tensor rows (pointers, element count, group, flags,
// the step's two bias corrections), a table of vnx_adamw_group rows, and a list of chunks {tensor index, element offset} that
// cuts the tensors into pieces of kOptChunk elements.  One workgroup of kOptThreads threads handles one chunk; all of a
// workgroup's table reads are workgroup-uniform.
//
//   1. adamw_norm_kernel: the chunk's sum of g^2 in fp32 -- each thread a fixed set of elements in a fixed order, the lanes by
//      a fixed exchange tree, the four waves in a fixed order -- into the chunk's own slot of `partials`.  Every slot is written
//      (a skipped tensor's, a malformed chunk's: 0), so there is no memset.
//   2. adamw_fold_kernel: ONE workgroup adds the slots in double -- thread t the slots t, t + 256, ... in order, then a fixed
//      tree over the threads -- and leaves total_norm and coef in `norm`: as floats, and coef once more as the double it was
//      computed in.
//   3. adamw_update_kernel: reads coef from `norm` and updates p, m, v.  The clipped gradient exists in registers only.
// No atomics: the result does not depend on the order in which workgroups run, and two runs are bit-identical.
//
// Sizing.  The update pass streams 16 B in and 12 B out per element and does ~15 multiply-adds, a square root and two divisions on them: the questions are bytes in
// flight and occupancy, not arithmetic.  A thread owns kOptVec 16-byte groups of each of g, p, m, v = 256 B of loads, 16 KB
// per wave, none of which depends on another.  The correctly rounded divide and square root cost registers: left alone the
// compiler takes 164 of them (two waves per SIMD); the kernel asks for four waves per SIMD (121 registers, no spill), and
// the compiler then issues a thread's loads in batches of four between the arithmetic rather than all at once -- 16 waves
// per CU with 4 to 16 KB outstanding each, still several times the ~32 KB per CU of outstanding loads that saturate
// HBM.  kOptChunk = 4096 elements keeps the chunk list of a 49 M-parameter
// model at ~12 k workgroups (47 rounds of 256 CUs: the tail round is ~2 % of the pass) while a tensor of a few hundred
// elements (norms and biases) still costs one short workgroup, not a slot in a padded stream.
// The norm pass reads 4 B per element with the same shape (64 B per thread in flight, more waves resident).
//
// Access.  A tensor whose four pointers are 16-byte aligned (the row's flag says so; chunk offsets are multiples of kOptChunk)
// is walked with 16-byte loads and stores, lane l of step k on group k * 256 + l of the chunk, and its last numel % 4 elements
// one per thread; any other tensor one element per thread per step.  No access lies outside [0, numel).
#include "vnx_common.h"

#pragma clang fp contract(off)

namespace vnx {
namespace {

constexpr int kOptThreads = 256;
constexpr int kOptChunk = VNX_ADAMW_CHUNK;
constexpr int kOptVec = kOptChunk / (4 * kOptThreads);      // 16-byte groups per thread and stream
// The tensors' pointers come out of a table, so the compiler cannot see their address space and would emit FLAT accesses;
// they are device memory by contract: say so, and the loads and stores are global_load / global_store_dwordx4.
typedef __attribute__((address_space(1))) float gfloat;
typedef __attribute__((address_space(1))) vnx_f4 gfloat4;
__device__ __forceinline__ gfloat* as_global(const void* p, long long off) {
  return (gfloat*)(static_cast<const float*>(p) + off);
}
static_assert(kOptVec * 4 * kOptThreads == kOptChunk, "a chunk is a whole number of 16-byte groups per thread");
static_assert(sizeof(vnx_adamw_tensor) == 64 && sizeof(vnx_adamw_group) == 64, "table rows: include/vnext_hip.h");

// the piece of a tensor a workgroup owns: n == 0 when the chunk names no tensor or lies outside it
struct Piece {
  vnx_adamw_tensor row;
  long long off;
  int n;
};

__device__ __forceinline__ Piece piece_of(const vnx_adamw_tensor* __restrict__ tensors, int n_tensors,
                                          const long long* __restrict__ chunks) {
  Piece pc;
  const long long t = chunks[2 * size_t(blockIdx.x)], off = chunks[2 * size_t(blockIdx.x) + 1];
  pc.off = off;
  pc.n = 0;
  if (t < 0 || t >= n_tensors) {
    pc.row = vnx_adamw_tensor{};
    return pc;
  }
  pc.row = tensors[t];
  if (off < 0 || off >= pc.row.numel) return pc;
  const long long left = pc.row.numel - off;
  pc.n = left < kOptChunk ? int(left) : kOptChunk;
  return pc;
}

__global__ __launch_bounds__(kOptThreads) void adamw_norm_kernel(const vnx_adamw_tensor* __restrict__ tensors, int n_tensors,
                                                                 const long long* __restrict__ chunks,
                                                                 float* __restrict__ partials) {
  __shared__ float wave_part[kOptThreads / kWave];
  const Piece pc = piece_of(tensors, n_tensors, chunks);
  const int tid = threadIdx.x;
  float acc = 0.f;
  if (pc.n > 0 && pc.row.g != nullptr) {
    const gfloat* __restrict__ g = as_global(pc.row.g, pc.off);
    if (!(pc.row.flags & VNX_ADAMW_UNALIGNED)) {
      const int n4 = pc.n >> 2;
      vnx_f4 x[kOptVec];
#pragma unroll
      for (int k = 0; k < kOptVec; ++k) {
        const int i4 = k * kOptThreads + tid;
        x[k] = i4 < n4 ? *reinterpret_cast<const gfloat4*>(g + 4 * i4) : vnx_f4{0.f, 0.f, 0.f, 0.f};
      }
#pragma unroll
      for (int k = 0; k < kOptVec; ++k) acc += (x[k].x * x[k].x + x[k].y * x[k].y) + (x[k].z * x[k].z + x[k].w * x[k].w);
      const int i = (n4 << 2) + tid;      // the last numel % 4 elements
      if (i < pc.n) acc += g[i] * g[i];
    } else {
      for (int i = tid; i < pc.n; i += kOptThreads) acc += g[i] * g[i];
    }
  }
  acc = wave_sum(acc);
  if ((tid & (kWave - 1)) == 0) wave_part[tid / kWave] = acc;
  __syncthreads();
  if (tid == 0) partials[blockIdx.x] = (wave_part[0] + wave_part[1]) + (wave_part[2] + wave_part[3]);
}

__global__ __launch_bounds__(kOptThreads) void adamw_fold_kernel(const float* __restrict__ partials, long long n_chunks,
                                                                 double max_norm, float* __restrict__ norm) {
  __shared__ double part[kOptThreads];
  const int tid = threadIdx.x;
  double acc = 0.0;
  for (long long i = tid; i < n_chunks; i += kOptThreads) acc += double(partials[i]);
  part[tid] = acc;
  __syncthreads();
  for (int s = kOptThreads / 2; s > 0; s >>= 1) {
    if (tid < s) part[tid] += part[tid + s];
    __syncthreads();
  }
  if (tid == 0) {
    const double total = sqrt(part[0]);
    const double c = max_norm / (total + 1e-6);
    const double coef = c > 1.0 ? 1.0 : c;      // clamp(max=1): a NaN stays a NaN
    norm[0] = float(total);
    norm[1] = float(coef);
    *reinterpret_cast<double*>(norm + 2) = coef;
  }
}

struct StepConsts {
  double coef, decay, omb1, beta2, omb2, step;
  float bc2s, eps;
};

// torch.optim.AdamW's single-tensor expression on the clipped gradient.  The three state updates are a handful of multiply-adds
// whose fp32 roundings (the clipped gradient's, the coefficient's, the products') would add up to a few ulp of m and v, shared
// by every element through the coefficient; fp64 multiply-adds run at half the fp32 rate here and the pass waits for memory,
// so they are done in double on the fp32 inputs and rounded ONCE.  The denominator -- a square root and two divisions, the
// expensive part -- stays fp32, correctly rounded: its error reaches p scaled by the step size.
__device__ __forceinline__ void adamw_element(float& p, float g, float& m, float& v, const StepConsts& c) {
  const double gd = double(g) * c.coef;
  m = float(fma(c.omb1, gd - double(m), double(m)));
  v = float(fma(c.omb2 * gd, gd, c.beta2 * double(v)));
  const float denom = sqrtf(v) / c.bc2s + c.eps;
  p = float(fma(-c.step, double(m / denom), double(p) * c.decay));
}

// the 16-byte groups of an aligned chunk: n4 of them (Full: all kOptChunk / 4, and no lane tests a bound -- the common case,
// where no branch stands between a thread's loads)
template <bool Full>
__device__ __forceinline__ void adamw_groups(const gfloat* __restrict__ g, gfloat* __restrict__ p, gfloat* __restrict__ m,
                                             gfloat* __restrict__ v, int n4, int tid, const StepConsts& c) {
  vnx_f4 xg[kOptVec], xp[kOptVec], xm[kOptVec], xv[kOptVec];
#pragma unroll
  for (int k = 0; k < kOptVec; ++k) {
    const int i4 = k * kOptThreads + tid;
    if (Full || i4 < n4) {
      xg[k] = *reinterpret_cast<const gfloat4*>(g + 4 * i4);
      xp[k] = *reinterpret_cast<const gfloat4*>(p + 4 * i4);
      xm[k] = *reinterpret_cast<const gfloat4*>(m + 4 * i4);
      xv[k] = *reinterpret_cast<const gfloat4*>(v + 4 * i4);
    }
  }
#pragma unroll
  for (int k = 0; k < kOptVec; ++k) {
    const int i4 = k * kOptThreads + tid;
    if (Full || i4 < n4) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        float pj = xp[k][j], mj = xm[k][j], vj = xv[k][j];
        adamw_element(pj, xg[k][j], mj, vj, c);
        xp[k][j] = pj; xm[k][j] = mj; xv[k][j] = vj;
      }
      *reinterpret_cast<gfloat4*>(p + 4 * i4) = xp[k];
      *reinterpret_cast<gfloat4*>(m + 4 * i4) = xm[k];
      *reinterpret_cast<gfloat4*>(v + 4 * i4) = xv[k];
    }
  }
}

__global__ __launch_bounds__(kOptThreads) __attribute__((amdgpu_waves_per_eu(4, 8)))
void adamw_update_kernel(const vnx_adamw_tensor* __restrict__ tensors, int n_tensors,
                         const vnx_adamw_group* __restrict__ groups, int n_groups, const long long* __restrict__ chunks,
                         const float* __restrict__ norm) {
  const Piece pc = piece_of(tensors, n_tensors, chunks);
  if (pc.n == 0 || pc.row.g == nullptr || pc.row.p == nullptr || pc.row.m == nullptr || pc.row.v == nullptr) return;
  if (pc.row.group < 0 || pc.row.group >= n_groups) return;
  const vnx_adamw_group grp = groups[pc.row.group];
  StepConsts c;
  c.coef = *reinterpret_cast<const double*>(norm + 2);
  c.decay = grp.decay;
  c.omb1 = grp.one_minus_beta1;
  c.beta2 = grp.beta2;
  c.omb2 = grp.one_minus_beta2;
  c.step = grp.lr / double(pc.row.bias_correction1);
  c.bc2s = pc.row.bias_correction2_sqrt;
  c.eps = float(grp.eps);
  const int tid = threadIdx.x;
  const gfloat* __restrict__ g = as_global(pc.row.g, pc.off);
  gfloat* __restrict__ p = as_global(pc.row.p, pc.off);
  gfloat* __restrict__ m = as_global(pc.row.m, pc.off);
  gfloat* __restrict__ v = as_global(pc.row.v, pc.off);
  if (!(pc.row.flags & VNX_ADAMW_UNALIGNED)) {
    if (pc.n == kOptChunk) {
      adamw_groups<true>(g, p, m, v, kOptChunk / 4, tid, c);
      return;
    }
    const int n4 = pc.n >> 2;
    adamw_groups<false>(g, p, m, v, n4, tid, c);
    const int i = (n4 << 2) + tid;      // the last numel % 4 elements
    if (i < pc.n) {
      float pi = p[i], mi = m[i], vi = v[i];
      adamw_element(pi, g[i], mi, vi, c);
      p[i] = pi; m[i] = mi; v[i] = vi;
    }
  } else {
    for (int i = tid; i < pc.n; i += kOptThreads) {
      float pi = p[i], mi = m[i], vi = v[i];
      adamw_element(pi, g[i], mi, vi, c);
      p[i] = pi; m[i] = mi; v[i] = vi;
    }
  }
}

int check_tables(const char* fn, const void* tensors, int n_tensors, const void* chunks, long long n_chunks) {
  if (n_tensors < 0 || n_chunks < 0) {
    set_error("%s: bad sizes (%d tensors, %lld chunks)", fn, n_tensors, n_chunks);
    return VNX_ERR_INVALID_ARGUMENT;
  }
  if (n_chunks > 0x7fffffffll) {
    set_error("%s: %lld chunks are more than one launch addresses", fn, n_chunks);
    return VNX_ERR_UNSUPPORTED;
  }
  if (n_chunks > 0 && (!tensors || !chunks || n_tensors == 0)) {
    set_error("%s: %lld chunks without a tensor table or a chunk list", fn, n_chunks);
    return VNX_ERR_INVALID_ARGUMENT;
  }
  if ((reinterpret_cast<uintptr_t>(tensors) & 15) != 0 || (reinterpret_cast<uintptr_t>(chunks) & 15) != 0) {
    set_error("%s: tensors and chunks must be 16-byte aligned", fn);
    return VNX_ERR_INVALID_ARGUMENT;
  }
  return VNX_OK;
}

}  // namespace
}  // namespace vnx

using namespace vnx;

extern "C" int vnx_adamw_grad_norm(const void* tensors, int n_tensors, const void* chunks, long long n_chunks, double max_norm,
                                   void* partials, void* norm, void* hip_stream) {
  const char* fn = "vnx_adamw_grad_norm";
  const int st = check_tables(fn, tensors, n_tensors, chunks, n_chunks);
  if (st != VNX_OK) return st;
  if (!norm || (n_chunks > 0 && !partials) || (reinterpret_cast<uintptr_t>(partials) & 3) != 0 ||
      (reinterpret_cast<uintptr_t>(norm) & 7) != 0) {
    set_error("%s: partials (4-byte aligned) and norm (8-byte aligned) must be non-null", fn);
    return VNX_ERR_INVALID_ARGUMENT;
  }
  hipStream_t stream = (hipStream_t)hip_stream;
  if (n_chunks > 0) {
    hipLaunchKernelGGL(adamw_norm_kernel, dim3(unsigned(n_chunks)), dim3(kOptThreads), 0, stream,
                       (const vnx_adamw_tensor*)tensors, n_tensors, (const long long*)chunks, (float*)partials);
    const int launched = check_launch(fn);
    if (launched != VNX_OK) return launched;
  }
  hipLaunchKernelGGL(adamw_fold_kernel, dim3(1), dim3(kOptThreads), 0, stream, (const float*)partials, n_chunks, max_norm,
                     (float*)norm);
  return check_launch(fn);
}

extern "C" int vnx_adamw_clipped_step(const void* tensors, int n_tensors, const void* groups, int n_groups, const void* chunks,
                                      long long n_chunks, const void* norm, void* hip_stream) {
  const char* fn = "vnx_adamw_clipped_step";
  const int st = check_tables(fn, tensors, n_tensors, chunks, n_chunks);
  if (st != VNX_OK) return st;
  if (n_chunks == 0) return VNX_OK;
  if (!groups || n_groups < 1 || !norm || (reinterpret_cast<uintptr_t>(groups) & 15) != 0 ||
      (reinterpret_cast<uintptr_t>(norm) & 7) != 0) {
    set_error("%s: groups (16-byte aligned, at least one row) and norm (8-byte aligned) must be non-null", fn);
    return VNX_ERR_INVALID_ARGUMENT;
  }
  hipLaunchKernelGGL(adamw_update_kernel, dim3(unsigned(n_chunks)), dim3(kOptThreads), 0, (hipStream_t)hip_stream,
                     (const vnx_adamw_tensor*)tensors, n_tensors, (const vnx_adamw_group*)groups, n_groups,
                     (const long long*)chunks, (const float*)norm);
  return check_launch(fn);
}
