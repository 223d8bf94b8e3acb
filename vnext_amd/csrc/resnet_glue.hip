// resnet_glue.hip -- the element-wise glue of the ResNet trunk in one pass per site: what follows a convolution whose frozen
// batch norm is folded into its filters (models/resnet.py).
//
// Per bottleneck the library chain is a bias add after each convolution (three, four with a projection shortcut), three
// ReLUs and the residual add, each a launch over a full activation; the stem adds a bias, a ReLU and a 3 x 3 max-pool.  Here
// the convolutions run without a bias and
//   conv_epilogue_fwd   y <- relu((y + bias[ch]) + (res + res_bias[ch]))     in place; res, res_bias optional
//   conv_epilogue_bwd   grad_in = y > 0 ? grad_y : 0                        one tensor: the gradient of y AND of res
//   stem_pool_fwd       out = max_pool2d(relu(x + bias[ch]), 3, 2, 1)       x read once, only the pooled map written
// These are streaming kernels: the design point is bytes moved and launches.  Every thread owns whole 16-byte chunks
// (4 fp32 / 8 bf16 / 8 f16 elements) of the flat array; a chunk is one 16-byte access per operand when the pointers are
// 16-byte aligned and the chunk is whole, element accesses otherwise (the array's tail, unaligned views).
//
// The channel of flat element i is (i / inner) % c with inner = h * w (NCHW) or 1 (NHWC).  Three forms, picked per launch:
//   kUniform  inner is a multiple of the chunk: a chunk lies in one plane, one bias per chunk
//   kRow      NHWC and c is a multiple of the chunk: a chunk is 16 bytes of one pixel's channels, the bias a 16-byte load
//   kWalk     anything else (plane heads and tails of an odd h * w, an odd NHWC c): the chunk is still ONE access of the
//             activation, the bias is looked up element by element, walking (offset in plane, channel) without a division
// fp32: the additions run in exactly the order written above (no multiply, so nothing contracts): bit-identical to the eager
// chain.  16-bit: operands widened, the sum formed in fp32, rounded once.  NaN and +-inf propagate as in clamp_min (a NaN is
// not less than 0).  All index arithmetic is 64-bit.
#include "vnx_common.h"

#include <algorithm>

namespace vnx {

namespace {

constexpr int kRgThreads = 256;
constexpr long long kRgMaxBlocks = 1 << 16;      // beyond: grid-stride
constexpr long long kRgMaxElems = 1LL << 46;      // elements of a call at most
constexpr long long kRgMaxDim = 1LL << 31;        // each size at most: the products below stay inside 64 bits

enum RgForm { kUniform = 0, kRow = 1, kWalk = 2 };

template <typename T> struct alignas(16) Chunk {
  static constexpr int N = 16 / int(sizeof(T));
  T e[N];
};

template <typename T> __device__ __forceinline__ void chunk_load(const T* p, bool vec, int valid, float* out) {
  constexpr int N = Chunk<T>::N;
  if (vec) {
    const Chunk<T> v = *reinterpret_cast<const Chunk<T>*>(p);
#pragma unroll
    for (int j = 0; j < N; ++j) out[j] = to_acc(v.e[j]);
  } else {
#pragma unroll
    for (int j = 0; j < N; ++j) out[j] = j < valid ? to_acc(p[j]) : 0.f;
  }
}

template <typename T> __device__ __forceinline__ void chunk_store(T* p, bool vec, int valid, const float* in) {
  constexpr int N = Chunk<T>::N;
  if (vec) {
    Chunk<T> v;
#pragma unroll
    for (int j = 0; j < N; ++j) v.e[j] = from_acc<T>(in[j]);
    *reinterpret_cast<Chunk<T>*>(p) = v;
  } else {
#pragma unroll
    for (int j = 0; j < N; ++j)
      if (j < valid) p[j] = from_acc<T>(in[j]);
  }
}

__device__ __forceinline__ float relu_keep_nan(float v) { return v < 0.f ? 0.f : v; }

template <typename T, int FORM>
__global__ void __launch_bounds__(kRgThreads)
conv_epilogue_fwd_kernel(T* __restrict__ y, const T* __restrict__ bias, const T* __restrict__ res,
                         const T* __restrict__ res_bias, long long total, long long inner, long long c, bool aligned) {
  constexpr int N = Chunk<T>::N;
  const long long chunks = (total + N - 1) / N;
  const long long stride = (long long)gridDim.x * kRgThreads;
  for (long long k = (long long)blockIdx.x * kRgThreads + threadIdx.x; k < chunks; k += stride) {
    const long long i0 = k * N;
    const long long left = total - i0;
    const int valid = left < N ? int(left) : N;
    const bool vec = aligned && valid == N;
    float a[N], r[N], b[N], rb[N];
    chunk_load<T>(y + i0, vec, valid, a);
    if (res != nullptr) chunk_load<T>(res + i0, vec, valid, r);
    if (FORM == kUniform) {
      const long long ch = (i0 / inner) % c;
      const float bv = to_acc(bias[ch]);
      const float rbv = res_bias != nullptr ? to_acc(res_bias[ch]) : 0.f;
#pragma unroll
      for (int j = 0; j < N; ++j) { b[j] = bv; rb[j] = rbv; }
    } else if (FORM == kRow) {
      const long long c0 = i0 % c;                           // a multiple of N; c0 + N <= c
      chunk_load<T>(bias + c0, aligned, N, b);
      if (res_bias != nullptr) chunk_load<T>(res_bias + c0, aligned, N, rb);
    } else {
      const long long plane = i0 / inner;
      long long off = i0 - plane * inner, ch = plane % c;
#pragma unroll
      for (int j = 0; j < N; ++j) {
        b[j] = to_acc(bias[ch]);
        rb[j] = res_bias != nullptr ? to_acc(res_bias[ch]) : 0.f;
        if (++off == inner) { off = 0; if (++ch == c) ch = 0; }
      }
    }
#pragma unroll
    for (int j = 0; j < N; ++j) {
      float v = a[j] + b[j];
      if (res != nullptr) {
        float s = r[j];
        if (res_bias != nullptr) s = s + rb[j];
        v = v + s;
      }
      a[j] = relu_keep_nan(v);
    }
    chunk_store<T>(y + i0, vec, valid, a);
  }
}

template <typename T>
__global__ void __launch_bounds__(kRgThreads)
conv_epilogue_bwd_kernel(const T* __restrict__ grad_y, const T* __restrict__ y, T* __restrict__ grad_in, long long total,
                         bool aligned) {
  constexpr int N = Chunk<T>::N;
  const long long chunks = (total + N - 1) / N;
  const long long stride = (long long)gridDim.x * kRgThreads;
  for (long long k = (long long)blockIdx.x * kRgThreads + threadIdx.x; k < chunks; k += stride) {
    const long long i0 = k * N;
    const long long left = total - i0;
    const int valid = left < N ? int(left) : N;
    const bool vec = aligned && valid == N;
    float g[N], v[N];
    chunk_load<T>(grad_y + i0, vec, valid, g);
    chunk_load<T>(y + i0, vec, valid, v);
#pragma unroll
    for (int j = 0; j < N; ++j) g[j] = v[j] > 0.f ? g[j] : 0.f;
    chunk_store<T>(grad_in + i0, vec, valid, g);
  }
}

// ATen's max_pool2d: `val > max || isnan(val)` replaces the maximum, so a NaN in the window is the result
__device__ __forceinline__ float pool_take(float m, float v) { return (v > m || v != v) ? v : m; }

// One thread per output element (VEC = 1), or per 16 bytes of one output pixel's channels (NHWC, VEC = Chunk<T>::N).
template <typename T, bool NHWC, int VEC>
__global__ void __launch_bounds__(kRgThreads)
stem_pool_fwd_kernel(const T* __restrict__ x, const T* __restrict__ bias, T* __restrict__ out, long long n, long long c,
                     long long h, long long w, long long oh, long long ow) {
  const long long cg = c / VEC;                              // channel groups (VEC > 1: c is a multiple of VEC)
  const long long items = n * cg * oh * ow;
  const long long stride = (long long)gridDim.x * kRgThreads;
  for (long long it = (long long)blockIdx.x * kRgThreads + threadIdx.x; it < items; it += stride) {
    long long img, ch, oy, ox;
    if (NHWC) {
      ch = (it % cg) * VEC;
      long long t = it / cg;
      ox = t % ow; t /= ow;
      oy = t % oh;
      img = t / oh;
    } else {
      ox = it % ow;
      long long t = it / ow;
      oy = t % oh; t /= oh;
      ch = t % c;
      img = t / c;
    }
    float b[VEC], m[VEC];
    if constexpr (VEC > 1) chunk_load<T>(bias + ch, true, VEC, b);
    else b[0] = to_acc(bias[ch]);
#pragma unroll
    for (int j = 0; j < VEC; ++j) m[j] = -INFINITY;
    for (int dy = 0; dy < 3; ++dy) {
      const long long iy = 2 * oy - 1 + dy;
      if (iy < 0 || iy >= h) continue;
      for (int dx = 0; dx < 3; ++dx) {
        const long long ix = 2 * ox - 1 + dx;
        if (ix < 0 || ix >= w) continue;
        const long long at = NHWC ? ((img * h + iy) * w + ix) * c + ch : ((img * c + ch) * h + iy) * w + ix;
        float v[VEC];
        if constexpr (VEC > 1) chunk_load<T>(x + at, true, VEC, v);
        else v[0] = to_acc(x[at]);
#pragma unroll
        for (int j = 0; j < VEC; ++j) m[j] = pool_take(m[j], relu_keep_nan(v[j] + b[j]));
      }
    }
    const long long to = NHWC ? ((img * oh + oy) * ow + ox) * c + ch : ((img * c + ch) * oh + oy) * ow + ox;
    if constexpr (VEC > 1) chunk_store<T>(out + to, true, VEC, m);
    else out[to] = from_acc<T>(m[0]);
  }
}

bool rg_aligned(const void* p) { return (uintptr_t(p) & 15) == 0; }

dim3 rg_grid(long long items) {
  const long long blocks = (items + kRgThreads - 1) / kRgThreads;
  return dim3(uint32_t(std::max<long long>(1, std::min<long long>(blocks, kRgMaxBlocks))));
}

int rg_check(const char* who, int dtype, int layout) {
  if (dtype != VNX_F32 && dtype != VNX_BF16 && dtype != VNX_F16) {
    set_error("%s: dtype is VNX_F32, VNX_BF16 or VNX_F16 (got %d)", who, dtype);
    return VNX_ERR_UNSUPPORTED;
  }
  if (layout != VNX_LAYOUT_NCHW && layout != VNX_LAYOUT_NHWC) {
    set_error("%s: layout is VNX_LAYOUT_NCHW or VNX_LAYOUT_NHWC (got %d)", who, layout);
    return VNX_ERR_UNSUPPORTED;
  }
  return VNX_OK;
}

template <typename T>
void epilogue_fwd_launch(void* y, const void* bias, const void* res, const void* res_bias, long long total, long long inner,
                         long long c, bool nhwc, hipStream_t stream) {
  constexpr int N = Chunk<T>::N;
  const bool aligned = rg_aligned(y) && rg_aligned(bias) && rg_aligned(res) && rg_aligned(res_bias);
  const dim3 grid = rg_grid((total + N - 1) / N);
#define VNX_RG_FWD(FORM)                                                                                             \
  hipLaunchKernelGGL((conv_epilogue_fwd_kernel<T, FORM>), grid, dim3(kRgThreads), 0, stream, (T*)y, (const T*)bias, \
                     (const T*)res, (const T*)res_bias, total, inner, c, aligned)
  if (!nhwc && inner % N == 0) VNX_RG_FWD(kUniform);
  else if (nhwc && c % N == 0) VNX_RG_FWD(kRow);
  else VNX_RG_FWD(kWalk);
#undef VNX_RG_FWD
}

template <typename T>
void epilogue_bwd_launch(const void* grad_y, const void* y, void* grad_in, long long total, hipStream_t stream) {
  constexpr int N = Chunk<T>::N;
  const bool aligned = rg_aligned(grad_y) && rg_aligned(y) && rg_aligned(grad_in);
  hipLaunchKernelGGL((conv_epilogue_bwd_kernel<T>), rg_grid((total + N - 1) / N), dim3(kRgThreads), 0, stream,
                     (const T*)grad_y, (const T*)y, (T*)grad_in, total, aligned);
}

template <typename T>
void stem_pool_launch(const void* x, const void* bias, void* out, long long n, long long c, long long h, long long w,
                      long long oh, long long ow, bool nhwc, hipStream_t stream) {
  constexpr int N = Chunk<T>::N;
  const long long outs = n * c * oh * ow;
#define VNX_RG_POOL(NHWC, VEC, ITEMS)                                                                               \
  hipLaunchKernelGGL((stem_pool_fwd_kernel<T, NHWC, VEC>), rg_grid(ITEMS), dim3(kRgThreads), 0, stream, (const T*)x, \
                     (const T*)bias, (T*)out, n, c, h, w, oh, ow)
  if (nhwc && c % N == 0 && rg_aligned(x) && rg_aligned(bias) && rg_aligned(out)) VNX_RG_POOL(true, N, outs / N);
  else if (nhwc) VNX_RG_POOL(true, 1, outs);
  else VNX_RG_POOL(false, 1, outs);
#undef VNX_RG_POOL
}

}  // namespace

}  // namespace vnx

using namespace vnx;

extern "C" int vnx_conv_epilogue_forward(int dtype, int layout, void* y, const void* bias, const void* res,
                                         const void* res_bias, long long n, long long c, long long hw, void* hip_stream) {
  const char* who = "vnx_conv_epilogue_forward";
  if (int st = rg_check(who, dtype, layout)) return st;
  if (n < 0 || n > kRgMaxDim || c < 1 || c > kRgMaxDim || hw < 0 || (hw > 0 && n * c > kRgMaxElems / hw)) {
    set_error("%s: bad sizes n=%lld c=%lld hw=%lld", who, n, c, hw);
    return VNX_ERR_INVALID_ARGUMENT;
  }
  const long long total = n * c * hw;
  if (total == 0) return VNX_OK;
  if (!y || !bias || (res_bias && !res)) {
    set_error("%s: null pointer argument (y and bias are required; res_bias goes with res)", who);
    return VNX_ERR_INVALID_ARGUMENT;
  }
  hipStream_t stream = (hipStream_t)hip_stream;
  const bool nhwc = layout == VNX_LAYOUT_NHWC;
  const long long inner = nhwc ? 1 : hw;
  if (dtype == VNX_F32) epilogue_fwd_launch<float>(y, bias, res, res_bias, total, inner, c, nhwc, stream);
  else if (dtype == VNX_BF16) epilogue_fwd_launch<bf16_t>(y, bias, res, res_bias, total, inner, c, nhwc, stream);
  else epilogue_fwd_launch<f16_t>(y, bias, res, res_bias, total, inner, c, nhwc, stream);
  return check_launch(who);
}

extern "C" int vnx_conv_epilogue_backward(int dtype, const void* grad_y, const void* y, void* grad_in, long long count,
                                          void* hip_stream) {
  const char* who = "vnx_conv_epilogue_backward";
  if (int st = rg_check(who, dtype, VNX_LAYOUT_NCHW)) return st;
  if (count < 0 || count > kRgMaxElems) {
    set_error("%s: bad count %lld", who, count);
    return VNX_ERR_INVALID_ARGUMENT;
  }
  if (count == 0) return VNX_OK;
  if (!grad_y || !y || !grad_in) {
    set_error("%s: null pointer argument", who);
    return VNX_ERR_INVALID_ARGUMENT;
  }
  hipStream_t stream = (hipStream_t)hip_stream;
  if (dtype == VNX_F32) epilogue_bwd_launch<float>(grad_y, y, grad_in, count, stream);
  else if (dtype == VNX_BF16) epilogue_bwd_launch<bf16_t>(grad_y, y, grad_in, count, stream);
  else epilogue_bwd_launch<f16_t>(grad_y, y, grad_in, count, stream);
  return check_launch(who);
}

extern "C" int vnx_stem_pool_forward(int dtype, int layout, const void* conv_out, const void* bias, void* out, long long n,
                                     long long c, long long h, long long w, void* hip_stream) {
  const char* who = "vnx_stem_pool_forward";
  if (int st = rg_check(who, dtype, layout)) return st;
  if (n < 0 || n > kRgMaxDim || c < 1 || c > kRgMaxDim || h < 1 || h > kRgMaxDim || w < 1 || w > kRgMaxDim ||
      n * c > kRgMaxElems / h / w) {
    set_error("%s: bad sizes n=%lld c=%lld h=%lld w=%lld", who, n, c, h, w);
    return VNX_ERR_INVALID_ARGUMENT;
  }
  if (n == 0) return VNX_OK;
  if (!conv_out || !bias || !out) {
    set_error("%s: null pointer argument", who);
    return VNX_ERR_INVALID_ARGUMENT;
  }
  const long long oh = (h - 1) / 2 + 1, ow = (w - 1) / 2 + 1;      // floor((h + 2 * 1 - 3) / 2) + 1
  hipStream_t stream = (hipStream_t)hip_stream;
  const bool nhwc = layout == VNX_LAYOUT_NHWC;
  if (dtype == VNX_F32) stem_pool_launch<float>(conv_out, bias, out, n, c, h, w, oh, ow, nhwc, stream);
  else if (dtype == VNX_BF16) stem_pool_launch<bf16_t>(conv_out, bias, out, n, c, h, w, oh, ow, nhwc, stream);
  else stem_pool_launch<f16_t>(conv_out, bias, out, n, c, h, w, oh, ow, nhwc, stream);
  return check_launch(who);
}
