// set_loss.hip -- the class and box losses of both criteria (sigmoid focal over all logits against the implied one-hot
// target, L1 and GIoU of the matched boxes, the count of matched queries whose argmax is their label) for every decoder
// layer at once: two launches forward, one backward.
//
// What it replaces (criterion.py / idol_criterion.py `forward_all_layers`): zeros_like + index_put + a label gather for the
// one-hot target, sigmoid, BCE and about ten element-wise passes over [Ld, N, Q, K], two reductions, a transposed
// advanced-index gather of the predicted boxes, cat + gather of the targets, two cxcywh -> xyxy conversions, `giou_loss`
// (some twenty-five launches), the per-layer sums (index_add_ in IDOL) -- and autograd's replay of all of it, with a dense
// index_put backward into the boxes.
//
// Here: logits fp32 [Ld][N][Q][K], boxes fp32 [Ld][N][T][Q][4] (cx, cy, w, h; IDOL: T = 1), the pair list lay / clip / qry /
// tgt int64 [R] (`DeviceMatch`'s layout: pair r says that query qry[r] of (layer lay[r], clip clip[r]) is matched to target
// tgt[r] of the batch's targets laid back to back), labels int64 [n_tot], target boxes fp32 [n_tot][T][4].
//   out [Ld][4] = { sum over (n, q, k) of the focal term, target 1 at (n, qry, labels[tgt]) of the layer's pairs, else 0;
//                   sum over the layer's pairs, frames and coordinates of |pred - want|;
//                   sum over the layer's pairs and frames of 1 - GIoU (criterion.giou_loss: eps 1e-7 on union and hull,
//                   the (hi > lo).all overlap gate, hull extents not clamped);
//                   the number of the layer's pairs whose argmax over K is the label (first maximum, as torch.argmax) }
// PRECONDITIONS: a (lay, clip, qry) triple appears at most once in the list (Hungarian pairs are one-to-one; simOTA returns
// each selected query once) -- with a duplicate, which of the two pairs a query keeps is not defined.  A pair with a
// negative qry or tgt (the device matcher's answer for a clip whose cost is not finite), or with any index outside its
// array, contributes nothing; a label outside [0, K) sets no target and scores no hit, the pair's boxes still count.
//
// The focal element is mask_loss.hip's: for a 0/1 target t, z = t ? x : -x, ce = softplus(-z), s = sigmoid(-z) = 1 - p_t,
//   focal = alpha_t * ce * s^2 (gamma = 2; alpha_t = t ? alpha : 1 - alpha, 1 when alpha < 0),
//   dfocal/dz = -alpha_t * s^2 * (s + 2 ce (1 - s)),  dz/dx = t ? 1 : -1,   e = exp(-|x|) computed once.
//
// Forward, launch 1 (set_loss_fwd_kernel): a workgroup of 256 lanes owns one PIECE of one (layer, clip): a run of
// rows_per_piece = clamp(4096 / K, 1, 1024) consecutive queries, i.e. about 4 096 consecutive logits -- any K works, the
// row of an element is one division of its index (one per 16-byte load where K % 4 == 0).  The one-hot target is never
// materialised: the workgroup first scans the pair list (a few hundred entries at most, cheaper than a sorted index) and
// leaves, per query of its piece, the label and the pair's index in LDS.  It then streams its logits, 16 per lane, walks
// its matched queries' boxes (one lane per (query, frame)), takes the argmax of each matched row, and stores ONE 16-byte
// partial {focal, l1, giou, hits}: lane sums, a fixed exchange tree across the wave, the four waves in order.
// Launch 2 (set_loss_finish_kernel): one wave per layer adds the layer's N x pieces partials in a fixed order.
// No atomics anywhere: the result is a function of the input alone (bit-identical run to run).
//
// Backward (set_loss_bwd_kernel): one launch over the same pieces.  It rebuilds the LDS map, recomputes every term from
// the inputs -- the forward keeps nothing -- and writes EVERY element of grad_logits and of grad_boxes (zeros at
// unmatched queries): no memset, no scatter.  grad of column 3 (the hit count) is ignored: it is not differentiable.
// Gradient conventions are ATen's: sign(pred - want) for the L1 term, sign(0) = 0; maximum / minimum hand the gradient to
// the selected operand, and at an exact tie split it evenly between the two (the target's half goes nowhere); the
// intersection is differentiated only where the overlap gate is open.
#include "vnx_common.h"

namespace vnx {
namespace {

constexpr int kSlThreads = 256;
constexpr int kSlPiece = VNX_SET_LOSS_PIECE;            // logits per workgroup, about
constexpr int kSlMaxRows = VNX_SET_LOSS_MAX_ROWS;       // queries per workgroup at most (the LDS map)
constexpr float kSlEps = 1e-7f;

struct SlDims {
  int Ld, N, T, Q, K, R, n_tot;
  int rows, pieces;      // queries per piece, pieces per (layer, clip)
  int vec;               // K % 4 == 0 and 16-byte aligned logits (and grad_logits): four logits of one row per load
  float alpha;
};

struct SlIn {
  const float* logits;
  const float* boxes;
  const int64_t* lay;
  const int64_t* clip;
  const int64_t* qry;
  const int64_t* tgt;
  const int64_t* labels;
  const float* tgt_boxes;
};

// which piece this workgroup owns
struct SlPiece { int l, n, q0, nq; };
__device__ __forceinline__ SlPiece sl_piece(const SlDims& d) {
  SlPiece p;
  const int ln = int(blockIdx.x) / d.pieces, piece = int(blockIdx.x) - ln * d.pieces;
  p.l = ln / d.N;
  p.n = ln - p.l * d.N;
  p.q0 = piece * d.rows;
  p.nq = min(d.rows, d.Q - p.q0);
  return p;
}

// per query of the piece: the label of its target (-1: unmatched, or a label outside [0, K)) and its pair (-1: unmatched)
__device__ __forceinline__ void sl_build_map(const SlIn& in, const SlDims& d, const SlPiece& p, int* s_label, int* s_pair) {
  for (int i = threadIdx.x; i < p.nq; i += kSlThreads) {
    s_label[i] = -1;
    s_pair[i] = -1;
  }
  __syncthreads();
  for (int r = threadIdx.x; r < d.R; r += kSlThreads) {
    if (in.lay[r] != int64_t(p.l) || in.clip[r] != int64_t(p.n)) continue;
    const int64_t q = in.qry[r], t = in.tgt[r];
    if (q < int64_t(p.q0) || q >= int64_t(p.q0 + p.nq) || t < 0 || t >= int64_t(d.n_tot)) continue;
    const int64_t c = in.labels[t];
    s_label[int(q) - p.q0] = c >= 0 && c < int64_t(d.K) ? int(c) : -1;
    s_pair[int(q) - p.q0] = r;
  }
  __syncthreads();
}

struct SlElem { float s, q, ce, at; };      // sigmoid(-z), sigmoid(z), softplus(-z), alpha_t
__device__ __forceinline__ SlElem sl_elem(float x, bool t, float alpha) {
  SlElem m;
  const float e = expf(-fabsf(x));
  const float inv = 1.f / (1.f + e);
  const float lo = e * inv;                        // the sigmoid of -|x|
  const float z = t ? x : -x;
  m.s = z >= 0.f ? lo : inv;
  m.q = z >= 0.f ? inv : lo;
  m.ce = log1pf(e) + fmaxf(-z, 0.f);
  m.at = alpha >= 0.f ? (t ? alpha : 1.f - alpha) : 1.f;
  return m;
}
__device__ __forceinline__ float sl_focal(float x, bool t, float alpha) {
  const SlElem m = sl_elem(x, t, alpha);
  return m.at * m.ce * (m.s * m.s);
}
__device__ __forceinline__ float sl_focal_grad(float x, bool t, float alpha) {      // dfocal/dx
  const SlElem m = sl_elem(x, t, alpha);
  const float dz = -m.at * (m.s * m.s) * (m.s + 2.f * m.ce * m.q);
  return t ? dz : -dz;
}

struct SlBox { float cx, cy, w, h; };
__device__ __forceinline__ SlBox sl_load_box(const float* p) { return SlBox{p[0], p[1], p[2], p[3]}; }

// 1 - GIoU of two cxcywh boxes, criterion.giou_loss on their xyxy forms
struct SlGiou {
  float ax1, ay1, ax2, ay2, bx1, by1, bx2, by2;
  float iw, ih, inter, uni, hw, hh, hull;
  bool overlap;
};
__device__ __forceinline__ SlGiou sl_giou_terms(const SlBox& a, const SlBox& b) {
  SlGiou g;
  g.ax1 = a.cx - 0.5f * a.w; g.ay1 = a.cy - 0.5f * a.h; g.ax2 = a.cx + 0.5f * a.w; g.ay2 = a.cy + 0.5f * a.h;
  g.bx1 = b.cx - 0.5f * b.w; g.by1 = b.cy - 0.5f * b.h; g.bx2 = b.cx + 0.5f * b.w; g.by2 = b.cy + 0.5f * b.h;
  g.iw = fminf(g.ax2, g.bx2) - fmaxf(g.ax1, g.bx1);
  g.ih = fminf(g.ay2, g.by2) - fmaxf(g.ay1, g.by1);
  g.overlap = g.iw > 0.f && g.ih > 0.f;
  g.inter = g.overlap ? g.iw * g.ih : 0.f;
  g.uni = (g.ax2 - g.ax1) * (g.ay2 - g.ay1) + (g.bx2 - g.bx1) * (g.by2 - g.by1) - g.inter;
  g.hw = fmaxf(g.ax2, g.bx2) - fminf(g.ax1, g.bx1);
  g.hh = fmaxf(g.ay2, g.by2) - fminf(g.ay1, g.by1);
  g.hull = g.hw * g.hh;
  return g;
}
__device__ __forceinline__ float sl_giou_loss(const SlGiou& g) {
  return 1.f - (g.inter / (g.uni + kSlEps) - (g.hull - g.uni) / (g.hull + kSlEps));
}
// the share of a maximum's / minimum's gradient that goes to its first operand
__device__ __forceinline__ float sl_max_share(float a, float b) { return a > b ? 1.f : (a == b ? 0.5f : 0.f); }
__device__ __forceinline__ float sl_min_share(float a, float b) { return a < b ? 1.f : (a == b ? 0.5f : 0.f); }

// the pair's address pieces: element (l, n, t, q) of the boxes, frame t of target j
__device__ __forceinline__ int64_t sl_box_at(const SlDims& d, const SlPiece& p, int t, int q) {
  return (((int64_t(p.l) * d.N + p.n) * d.T + t) * d.Q + q) * 4;
}

}  // namespace

// grid: Ld * N * pieces workgroups; partial [Ld][N * pieces][4] = {focal, l1, giou, hits} of the piece
__global__ void __launch_bounds__(kSlThreads) set_loss_fwd_kernel(const SlIn in, const SlDims d, float* __restrict__ partial) {
  __shared__ int s_label[kSlMaxRows];
  __shared__ int s_pair[kSlMaxRows];
  __shared__ float s_part[kSlThreads / 64][4];
  const SlPiece p = sl_piece(d);
  sl_build_map(in, d, p, s_label, s_pair);
  const float* row0 = in.logits + ((int64_t(p.l) * d.N + p.n) * d.Q + p.q0) * d.K;
  const int count = p.nq * d.K;                                   // <= max(kSlPiece, K) logits
  float focal = 0.f, l1 = 0.f, giou = 0.f, hits = 0.f;
  if (d.vec) {
    for (int e = 4 * int(threadIdx.x); e < count; e += 4 * kSlThreads) {      // K % 4 == 0: the four share a row
      const vnx_f4 v = *reinterpret_cast<const vnx_f4*>(row0 + e);
      const int i = e / d.K, k = e - i * d.K, c = s_label[i] - k;             // c in 0..3: that one is the target
      focal += sl_focal(v.x, c == 0, d.alpha);
      focal += sl_focal(v.y, c == 1, d.alpha);
      focal += sl_focal(v.z, c == 2, d.alpha);
      focal += sl_focal(v.w, c == 3, d.alpha);
    }
  } else {
    for (int e = threadIdx.x; e < count; e += kSlThreads) {
      const int i = e / d.K, k = e - i * d.K;
      focal += sl_focal(row0[e], s_label[i] == k, d.alpha);
    }
  }
  // the matched queries' boxes: one lane per (frame, query of the piece); the argmax with frame 0
  for (int idx = threadIdx.x; idx < p.nq * d.T; idx += kSlThreads) {
    const int t = idx / p.nq, i = idx - t * p.nq;
    const int r = s_pair[i];
    if (r < 0) continue;
    const SlBox a = sl_load_box(in.boxes + sl_box_at(d, p, t, p.q0 + i));
    const SlBox b = sl_load_box(in.tgt_boxes + (in.tgt[r] * d.T + t) * 4);
    l1 += fabsf(a.cx - b.cx) + fabsf(a.cy - b.cy) + fabsf(a.w - b.w) + fabsf(a.h - b.h);
    giou += sl_giou_loss(sl_giou_terms(a, b));
    if (t == 0) {
      const float* x = row0 + int64_t(i) * d.K;
      float best = x[0];
      int arg = 0;
      for (int k = 1; k < d.K; ++k) {
        const float v = x[k];
        if (v > best) { best = v; arg = k; }
      }
      hits += arg == s_label[i] ? 1.f : 0.f;
    }
  }
  focal = wave_sum(focal);
  l1 = wave_sum(l1);
  giou = wave_sum(giou);
  hits = wave_sum(hits);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) {
    s_part[wave][0] = focal; s_part[wave][1] = l1; s_part[wave][2] = giou; s_part[wave][3] = hits;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    vnx_f4 o = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int k = 0; k < kSlThreads / 64; ++k) {                   // the waves in order
      o.x += s_part[k][0]; o.y += s_part[k][1]; o.z += s_part[k][2]; o.w += s_part[k][3];
    }
    *reinterpret_cast<vnx_f4*>(partial + 4 * int64_t(blockIdx.x)) = o;
  }
}

// grid: Ld workgroups of one wave.  Lane j adds the layer's partials j, j + 64, ... in order, then the 64 lane sums meet
// in a fixed exchange tree.  out [Ld][4]
__global__ void __launch_bounds__(64) set_loss_finish_kernel(const float* __restrict__ partial, int per_layer,
                                                             float* __restrict__ out) {
  const int l = blockIdx.x, lane = threadIdx.x;
  const vnx_f4* p = reinterpret_cast<const vnx_f4*>(partial) + int64_t(l) * per_layer;
  vnx_f4 a = {0.f, 0.f, 0.f, 0.f};
  for (int k = lane; k < per_layer; k += 64) a += p[k];
  a.x = wave_sum(a.x);
  a.y = wave_sum(a.y);
  a.z = wave_sum(a.z);
  a.w = wave_sum(a.w);
  if (lane == 0) *reinterpret_cast<vnx_f4*>(out + 4 * int64_t(l)) = a;
}

// grid: Ld * N * pieces workgroups.  grad_logits = g[l][0] * dfocal/dx everywhere; grad_boxes = g[l][1] * dL1 + g[l][2] *
// d(1 - GIoU) at the matched (l, n, t, q), 0 elsewhere
__global__ void __launch_bounds__(kSlThreads) set_loss_bwd_kernel(const SlIn in, const SlDims d,
                                                                  const float* __restrict__ grad_out,
                                                                  float* __restrict__ grad_logits,
                                                                  float* __restrict__ grad_boxes) {
  __shared__ int s_label[kSlMaxRows];
  __shared__ int s_pair[kSlMaxRows];
  const SlPiece p = sl_piece(d);
  sl_build_map(in, d, p, s_label, s_pair);
  const float g_focal = grad_out[4 * p.l], g_l1 = grad_out[4 * p.l + 1], g_giou = grad_out[4 * p.l + 2];
  const int64_t base = ((int64_t(p.l) * d.N + p.n) * d.Q + p.q0) * d.K;
  const float* row0 = in.logits + base;
  float* out0 = grad_logits + base;
  const int count = p.nq * d.K;
  if (d.vec) {
    for (int e = 4 * int(threadIdx.x); e < count; e += 4 * kSlThreads) {
      const vnx_f4 v = *reinterpret_cast<const vnx_f4*>(row0 + e);
      const int i = e / d.K, k = e - i * d.K, c = s_label[i] - k;
      const vnx_f4 o = {g_focal * sl_focal_grad(v.x, c == 0, d.alpha), g_focal * sl_focal_grad(v.y, c == 1, d.alpha),
                        g_focal * sl_focal_grad(v.z, c == 2, d.alpha), g_focal * sl_focal_grad(v.w, c == 3, d.alpha)};
      *reinterpret_cast<vnx_f4*>(out0 + e) = o;
    }
  } else {
    for (int e = threadIdx.x; e < count; e += kSlThreads) {
      const int i = e / d.K, k = e - i * d.K;
      out0[e] = g_focal * sl_focal_grad(row0[e], s_label[i] == k, d.alpha);
    }
  }
  for (int idx = threadIdx.x; idx < p.nq * d.T; idx += kSlThreads) {
    const int t = idx / p.nq, i = idx - t * p.nq;
    const int r = s_pair[i];
    const int64_t at = sl_box_at(d, p, t, p.q0 + i);
    float dcx = 0.f, dcy = 0.f, dw = 0.f, dh = 0.f;
    if (r >= 0) {
      const SlBox a = sl_load_box(in.boxes + at);
      const SlBox b = sl_load_box(in.tgt_boxes + (in.tgt[r] * d.T + t) * 4);
      auto sign = [](float v) { return v > 0.f ? 1.f : (v < 0.f ? -1.f : 0.f); };
      dcx = g_l1 * sign(a.cx - b.cx);
      dcy = g_l1 * sign(a.cy - b.cy);
      dw = g_l1 * sign(a.w - b.w);
      dh = g_l1 * sign(a.h - b.h);
      const SlGiou g = sl_giou_terms(a, b);
      // loss = 1 - I / (U + eps) + (H - U) / (H + eps),  U = area_a + area_b - I
      const float ue = g.uni + kSlEps, he = g.hull + kSlEps;
      const float dU = g_giou * (g.inter / (ue * ue) - 1.f / he);           // through U, the direct dependence
      const float dI = g.overlap ? g_giou * (-1.f / ue) - dU : 0.f;         // through I, directly and as part of U
      const float dH = g_giou * (ue / (he * he));
      const float aw = g.ax2 - g.ax1, ah = g.ay2 - g.ay1;
      // gradients of the four xyxy coordinates of the prediction: its area, the intersection, the hull
      const float diw = dI * g.ih, dih = dI * g.iw, dhw = dH * g.hh, dhh = dH * g.hw;
      const float dx1 = -dU * ah - diw * sl_max_share(g.ax1, g.bx1) - dhw * sl_min_share(g.ax1, g.bx1);
      const float dy1 = -dU * aw - dih * sl_max_share(g.ay1, g.by1) - dhh * sl_min_share(g.ay1, g.by1);
      const float dx2 = dU * ah + diw * sl_min_share(g.ax2, g.bx2) + dhw * sl_max_share(g.ax2, g.bx2);
      const float dy2 = dU * aw + dih * sl_min_share(g.ay2, g.by2) + dhh * sl_max_share(g.ay2, g.by2);
      dcx += dx1 + dx2;
      dcy += dy1 + dy2;
      dw += 0.5f * (dx2 - dx1);
      dh += 0.5f * (dy2 - dy1);
    }
    float* o = grad_boxes + at;
    o[0] = dcx; o[1] = dcy; o[2] = dw; o[3] = dh;
  }
}

static int sl_dims(const char* fn, const SlIn& in, int layers, int clips, int frames, int queries, int classes, int pairs,
                   int targets_total, float alpha, SlDims* d) {
  if (layers < 1 || clips < 1 || frames < 1 || queries < 1 || classes < 1 || pairs < 0 || targets_total < 0) {
    set_error("%s: bad sizes (layers %d, clips %d, frames %d, queries %d, classes %d, pairs %d, targets %d)", fn, layers,
              clips, frames, queries, classes, pairs, targets_total);
    return VNX_ERR_INVALID_ARGUMENT;
  }
  if (!(alpha <= 1.f)) {
    set_error("%s: alpha %g (at most 1; negative: no class weighting)", fn, double(alpha));
    return VNX_ERR_INVALID_ARGUMENT;
  }
  const int rows = classes >= kSlPiece ? 1 : (kSlPiece / classes > kSlMaxRows ? kSlMaxRows : kSlPiece / classes);
  const int64_t pieces = (int64_t(queries) + rows - 1) / rows;
  if (int64_t(rows) * classes >= (int64_t(1) << 30) || int64_t(layers) * clips * pieces >= (int64_t(1) << 31) ||
      int64_t(rows) * frames >= (int64_t(1) << 30)) {
    set_error("%s: %d x %d x %d x %d logits are outside what the kernel addresses", fn, layers, clips, queries, classes);
    return VNX_ERR_UNSUPPORTED;
  }
  if (!in.logits || !in.boxes || (pairs > 0 && (!in.lay || !in.clip || !in.qry || !in.tgt)) ||
      (targets_total > 0 && (!in.labels || !in.tgt_boxes))) {
    set_error("%s: null pointer argument", fn);
    return VNX_ERR_INVALID_ARGUMENT;
  }
  d->Ld = layers; d->N = clips; d->T = frames; d->Q = queries; d->K = classes; d->R = pairs; d->n_tot = targets_total;
  d->rows = rows; d->pieces = int(pieces);
  d->vec = (classes & 3) == 0 && (reinterpret_cast<uintptr_t>(in.logits) & 15) == 0;
  d->alpha = alpha;
  return VNX_OK;
}

static SlIn sl_in(const void* logits, const void* boxes, const void* lay, const void* clip, const void* qry, const void* tgt,
                  const void* labels, const void* target_boxes) {
  return SlIn{(const float*)logits, (const float*)boxes, (const int64_t*)lay, (const int64_t*)clip, (const int64_t*)qry,
              (const int64_t*)tgt, (const int64_t*)labels, (const float*)target_boxes};
}

}  // namespace vnx

using namespace vnx;

extern "C" int vnx_set_loss_forward(const void* logits, const void* boxes, const void* lay, const void* clip, const void* qry,
                                    const void* tgt, const void* labels, const void* target_boxes, int layers, int clips,
                                    int frames, int queries, int classes, int pairs, int targets_total, float alpha,
                                    void* partial, size_t partial_bytes, void* out, void* hip_stream) {
  const char* fn = "vnx_set_loss_forward";
  const SlIn in = sl_in(logits, boxes, lay, clip, qry, tgt, labels, target_boxes);
  SlDims d;
  if (int st = sl_dims(fn, in, layers, clips, frames, queries, classes, pairs, targets_total, alpha, &d)) return st;
  if (!partial || !out) {
    set_error("%s: null pointer argument", fn);
    return VNX_ERR_INVALID_ARGUMENT;
  }
  const size_t need = size_t(layers) * size_t(clips) * size_t(d.pieces) * 4 * sizeof(float);
  if (partial_bytes < need || (reinterpret_cast<uintptr_t>(partial) & 15) != 0 || (reinterpret_cast<uintptr_t>(out) & 15) != 0) {
    set_error("%s: partial buffer of %zu bytes, %zu needed (partial and out 16-byte aligned)", fn, partial_bytes, need);
    return VNX_ERR_WORKSPACE;
  }
  hipStream_t stream = (hipStream_t)hip_stream;
  hipLaunchKernelGGL(set_loss_fwd_kernel, dim3(uint32_t(layers) * uint32_t(clips) * uint32_t(d.pieces)), dim3(kSlThreads), 0,
                     stream, in, d, (float*)partial);
  if (int st = check_launch("set_loss_fwd")) return st;
  hipLaunchKernelGGL(set_loss_finish_kernel, dim3(uint32_t(layers)), dim3(64), 0, stream, (const float*)partial,
                     clips * d.pieces, (float*)out);
  return check_launch("set_loss_finish");
}

extern "C" int vnx_set_loss_backward(const void* logits, const void* boxes, const void* lay, const void* clip, const void* qry,
                                     const void* tgt, const void* labels, const void* target_boxes, int layers, int clips,
                                     int frames, int queries, int classes, int pairs, int targets_total, float alpha,
                                     const void* grad_out, void* grad_logits, void* grad_boxes, void* hip_stream) {
  const char* fn = "vnx_set_loss_backward";
  const SlIn in = sl_in(logits, boxes, lay, clip, qry, tgt, labels, target_boxes);
  SlDims d;
  if (int st = sl_dims(fn, in, layers, clips, frames, queries, classes, pairs, targets_total, alpha, &d)) return st;
  if (!grad_out || !grad_logits || !grad_boxes) {
    set_error("%s: null pointer argument", fn);
    return VNX_ERR_INVALID_ARGUMENT;
  }
  d.vec = d.vec && (reinterpret_cast<uintptr_t>(grad_logits) & 15) == 0;
  hipLaunchKernelGGL(set_loss_bwd_kernel, dim3(uint32_t(layers) * uint32_t(clips) * uint32_t(d.pieces)), dim3(kSlThreads), 0,
                     (hipStream_t)hip_stream, in, d, (const float*)grad_out, (float*)grad_logits, (float*)grad_boxes);
  return check_launch("set_loss_bwd");
}
