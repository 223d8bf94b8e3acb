// msda_units.h -- the MSDA kernels' shared host/device definitions: the call's sizes, the grad_value unit geometry with its
// tuning constants, and the fused prologue's arguments.  Included by msda_launchers.h and msda_gv_common.h; nothing outside the
// MSDA files needs it.
#pragma once
#include "vnx_common.h"

namespace vnx {

struct MsdaDims {
  int B, S, M, D, L, Lq, P;
};

// grad_value units: every level is split into at least this many.  Shared by the grad_loc kernel
// (which tags every sample with the units it touches) and the grad_value kernels.  `forced`:
// KernelVariant::gv_units of the variant the entry point read (0 = 2, or the tile-fed path's own).
int gv_units_min(const MsdaDims& d, bool tiles, int forced);
// Backward workspace of the record-fed path: [16-B sample records | 256-B aligned | 4-B unit ranges]
inline size_t gv_unit_ids_offset(const MsdaDims& d) {
  const size_t n = size_t(d.B) * d.M * d.L * d.Lq * d.P;
  return (16 * n + 255) & ~size_t(255);
}

// The fused prologue's extra arguments (msda_d32.hip, msda_d32_tile.hip)
struct FusedArgs {
  const void* reference;   // [B / ref_div, Lq, L, ref_dim], same element type as the offsets
  float* grad_reference;   // [B, Lq, L, 2] fp32, zero-filled, accumulated over heads; or null
  int ref_dim;             // 2 or 4
  int ref_div;             // consecutive batch elements sharing one reference row (frames of a clip)
  float* qsplit_zero;      // backward, fp32 grad_value: rows of the query-split levels are zeroed here (or null)
  float* tile_loc;         // backward, tile mode of grad_value (msda_d32_gvtiles.hip): the decoded locations [B,Lq,M,L,P,2]
  float* tile_attn;        //   and softmax weights [B,Lq,M,L,P] are left here in fp32 for that kernel (or null)
  int ref_f32;             // the reference points are fp32 whatever the offsets' type (round 6: under autocast the Linears emit
                           // 16-bit offsets / logits while the reference points stay fp32 -- VNX_MSDA_REF_F32 of the C ABI)
};
// element i of the reference points as fp32
template <typename TL>
__device__ __forceinline__ float fused_ref(const FusedArgs& fa, int64_t i) {
  return fa.ref_f32 ? static_cast<const float*>(fa.reference)[i] : to_acc(static_cast<const TL*>(fa.reference)[i]);
}

// Query split of the grad_value units (msda_d32_gvrec.hip).  A level of at most two row-units (the coarse
// levels: 240 and 60 pixels at 360p) receives taps from EVERY query, so each of its units sorts one chunk
// per 128 queries -- forty at the encoder shape (Lq = 5100), against a dozen for a fine-level unit: the
// kernel's critical path (a level-3 unit ran ~100 us of the 190).  From 1024 queries up such a level is
// therefore also split by query range into pieces of about ten chunks, each its own workgroup, and the
// pieces meet in grad_value through fp32 atomics (1.5 M dwords per 360p encoder call) on rows the
// grad_loc kernel zeroed.  NOT at the decoder shape: there the kernel lasts 15 us, the contended,
// L2-bypassing atomics cost each piece 12-25 us, and the backward went from 32 to 49 us.
// fp32 grad_value and 4 points per level only (the selection kernel); 1 = no split.
constexpr int kQsCoarse = 4;        // query pieces of a coarse level (<= 2 row-units) at most, from 32 (batch, head) pairs up
constexpr int kQsCoarseSmall = 16;  // ... with fewer pairs (the grid does not fill the chip: more, shorter pieces)
constexpr int kQsMid = 2;
constexpr int kQsChunks = 10;       // a piece is given about this many chunks of 128 queries
// batch_heads = B x M: with fewer than 32 (batch, head) pairs the grid leaves workgroup slots empty, and the middle
// levels are split further: 8 pieces instead of 2 (round 2: 4 -- encoder backward at B = 2 123 -> 109 us at 360p, 450 ->
// 412 us at 720p; round 3, tile-fed path: 8 pieces 322 -> 288 us at 720p B = 2, 234 -> 192 us at B = 1, 360p unchanged; 16
// pieces 326 us); at B = 5 (a full grid) 4 pieces measured slower than 2 (168.8 -> 191.7 us at 360p, 625 -> 637 us at 720p).
// The unit split of a level of n pixels, the ONE definition shared by the grad_loc kernel (which zeroes the rows of
// query-split levels and tags every sample with the units it touches), the grad_value kernels' level tables and the
// launcher's grid bound: at most rows_max rows per unit (kGvRowsMax / kGvTileRowsMax by grad_value path), at least units_min units, then normalised so that no unit is
// empty (units = ceil(n / rows_per_unit)).  (Round 2 had the zeroing phase use the count BEFORE normalisation: with
// units_min = 5 a 16-pixel level gave 5 there and 4 in the grad_value kernel -- different sides of the query-split
// threshold, atomics onto rows nobody had zeroed.  Latent at the default units_min = 2)
// The corner (h0, w0) of a sample's 2 x 2 footprint, h0 in [-1, H - 1], w0 in [-1, W - 1], in one word of the 16-byte
// sample record (grad_loc kernel -> record-fed grad_value kernel): two 16-bit fields while both sides of the level are
// below 65 535 pixels, the flat index over a (H + 1) x (W + 1) grid otherwise (one integer division per sample to
// unpack -- levels that large do not occur in the models, but a 1 x 70 000 level used to come back silently wrong).
// 0xffffffff = sample outside the map (never produced by either form).
__device__ __forceinline__ bool gv_corner_is_flat(int H, int W) { return H >= 0xffff || W >= 0xffff; }
__device__ __forceinline__ uint32_t gv_pack_corner(int h0, int w0, int H, int W) {
  return gv_corner_is_flat(H, W) ? uint32_t(h0 + 1) * uint32_t(W + 1) + uint32_t(w0 + 1)
                                 : (uint32_t(h0 + 1) << 16) | uint32_t(w0 + 1);
}
__device__ __forceinline__ void gv_unpack_corner(uint32_t v, int H, int W, int& h0, int& w0) {
  if (gv_corner_is_flat(H, W)) {
    const uint32_t h1 = v / uint32_t(W + 1);
    h0 = int(h1) - 1; w0 = int(v - h1 * uint32_t(W + 1)) - 1;
  } else {
    h0 = int(v >> 16) - 1; w0 = int(v & 0xffffu) - 1;
  }
}

// Rows per unit: 320 for the record-fed kernel (5 rows per 8-lane group, 72 VGPRs, 3 units per CU; 19 units per (batch,
// head) at 360p = 760 workgroups, one round of the 768 resident), 256 for the tile-fed kernel (4 rows per group: 62 VGPRs
// and 39 KB of LDS, FOUR units per CU -- encoder-360p backward 190.5 -> 176.8 us, 720p B = 2 341 -> 325 us; at 720p B = 5
// the thinner strips cost 2 %: 718 -> 732 us).
constexpr int kGvRowsMax = 320;
constexpr int kGvTileRowsMax = 256;
struct GvSplit { int units, rpu; };
__host__ __device__ inline GvSplit gv_level_split(int n, int units_min, int rows_max) {
  GvSplit s{0, 1};
  if (n > 0) {
    int units = (n + rows_max - 1) / rows_max;
    if (units < units_min) units = units_min;
    if (units > n) units = n;
    s.rpu = (n + units - 1) / units;
    s.units = (n + s.rpu - 1) / s.rpu;
  }
  return s;
}

// Units of the self-decoding grad_value kernel (msda_d32_gvdirect.hip; calls below 1 024 queries -- the decoders').  A unit is
// a pixel range of one level and reads + decodes the level's samples of ALL queries itself, so what the kernel fetches grows
// with the number of units (every one of them stages all grad_out rows of its head): units are LARGE -- up to kGvdRows
// rows, 10 per (batch, head) at 360p -- and hold no rows in registers: after one sort an 8-lane group walks its rows one
// after the other and stores each at once.  Every level receives the same number of taps (4 x points x queries) whatever
// its size, so a row of a coarse level (80 taps at the 60-pixel level of a 300-query call) is spread over 1 << gshift
// adjacent groups whose partial sums meet in registers; `ut` (gvd_units_min) cuts such a level in two when the grid has room.
constexpr int kGvdQc = 304;         // queries staged per pass (all 300 of a decoder call): 19 KiB of grad_out row halves in LDS
constexpr int kGvdRows = 768;       // rows of a unit at most (what the kernel's LDS holds); the launchers choose <= this per call (gvd_rows_max)
constexpr int kGvdRowsLarge = 640;  // ... for pyramids above kGvdSmallS pixels
constexpr int kGvdSmallS = 8192;
constexpr int kGvdOneRound = 832;   // workgroups resident at once -- 3 per CU x 256 CUs = 768 -- plus a twelfth: the T = 5 decoder call with
                                  // its small levels cut in two is 440 + 375 = 815 workgroups, and in the bench's fwd + bwd step that
                                  // is the best split measured (round 6, the product library built each way, same box: 7.73-7.76
                                  // Gpoints/s against 7.45-7.47 uncut -- the uncut call's longest units, whole coarse levels, end the
                                  // launch alone on their CUs and hold the next launch back -- 6.80 with three units per level, 6.45
                                  // with four; backward-only sequences prefer the uncut call, 19.5 against 21.5 us)
struct GvdSplit { int units, rpu, gshift; };
// Units per level at least.  A level that fits one unit (the 240- and 60-pixel levels at 360p) receives as many taps as a
// whole fine level, so its unit is the call's longest: when the grid has room for it in ONE round of resident workgroups such
// a level is cut in two (T = 5 decoder call: 10 -> 12 units per (batch, head), 480 workgroups, kernel 14.8 -> 13.6 us; at
// B = 10 the grid takes two rounds either way and the extra units cost 0.6 us: there 1).
// Rows per unit at most, chosen per call (round 6; measured with three workgroups per CU, paired backward, cold): 768 rows at
// the 360p pyramid (S = 5 100: 9 units per (batch, head) instead of 10 -- T = 5 call 21.9 -> 20.8 us with the grad_loc groups
// first, 19.5 with the grad_value groups first once everything is resident in one round; B = 10 35.4 -> 33.1), 640 at the
// 720p pyramid (S = 19 560: 35.1 against 40.3 us with 768 -- there a unit's time is its rows' stores).
__host__ __device__ inline int gvd_rows_max(int S) {
  const int r = S <= kGvdSmallS ? kGvdRows : kGvdRowsLarge;
  return r < kGvdRows ? r : kGvdRows;
}
// Units per (batch, head) the launchers expect (an estimate for tuning choices: the host knows S and L, not the level sizes;
// pyramids whose levels shrink four-fold need S / rows + L - 1)
__host__ __device__ inline int gvd_units_estimate(int S, int L, int rows) { return S / rows + (L > 1 ? L - 1 : 1); }
__host__ __device__ inline int gvd_units_min(int S, int L, int batch_heads, int rows, int64_t other_workgroups = 0) {
  // (the host knows S and L, not the level sizes: S / ROWS + L bounds the units of the 640-row split; the levels that gain a
  //  unit are the one or two smallest -- a heuristic for a tuning choice, any value is correct)
  //  `other_workgroups`: what shares the round with the units -- the grad_loc workgroups of the paired kernel, msda_d32.hip)
  return int64_t(batch_heads) * (gvd_units_estimate(S, L, rows) + 2) + other_workgroups <= kGvdOneRound ? 2 : 1;
}
__host__ __device__ inline GvdSplit gvd_level_split(int n, int ut, int Lq, int P, int rows_max) {
  GvdSplit s{0, 1, 0};
  if (n <= 0) return s;
  int units = (n + rows_max - 1) / rows_max;
  if (units < ut) units = ut;
  if (units > n) units = n;
  s.rpu = (n + units - 1) / units;
  s.units = (n + s.rpu - 1) / s.rpu;
  // taps a row expects: 4 x points x (queries of a pass) / pixels of the level; from 16 up a row takes 2 groups, 32: 4, 64: 8.
  // A pass stages min(kGvdQc, 4 * kGvdQc / P) queries (the kernel's qc), so taps <= 16 * kGvdQc = kGvdCap; a
  // gshift g >= 1 means taps >= (8 << g) * n, so rpu << g <= n << g <= kGvdCap / 8 -- inside the walk's kIters rounds.  (Taken
  // over the whole call, 4 x P x min(Lq, kGvdQc), it overcounted a pass from 5 points up: rows past slot 768 were lost.)
  const int qc = kGvdQc < 4 * kGvdQc / P ? kGvdQc : 4 * kGvdQc / P;
  const int64_t taps = int64_t(4) * P * (Lq < qc ? Lq : qc);
  while (s.gshift < 3 && taps >= (int64_t(16) << s.gshift) * n) ++s.gshift;
  // the walk covers kGvdRows slots of a unit (rows << gshift): fewer groups on a row is always correct, a row past the
  // last slot is never stored
  while (s.gshift > 0 && (s.rpu << s.gshift) > kGvdRows) --s.gshift;
  return s;
}

// Units of the tile-fed grad_value kernel (msda_d32_gvtiles.hip): RECTANGLES of a level, at most rows_max pixels each.
// A narrow level (W < 32) is cut into bands of whole image rows; a wider one also into columns of about 32 pixels --
// blocks of 32 x 8: a band of a 160-pixel-wide level would be 1.6 image rows thin while samples reach +-6 rows, i.e.
// 8.5 bands' worth of query tiles would hit every band of the 720p level 0 where a block sees 4.7.  Measured (encoder
// backward, B = 5, cold): round 3 -- blocks from 128 pixels of width up 732 -> 691 us at 720p, from 64 pixels up 651 us and
// 176.7 -> 174.6 us at 360p; block width 16 instead of 32: 699 us.  Round 4 (pieces meeting in partial rows): blocks from
// 32 pixels of width up -- the 40-pixel levels (24 x 40 at 360p, 23 x 40 at 720p) become four 20 x 12 blocks instead of four
// 40 x 6 bands -- 163.5 -> 153.4 us at 360p, 611 -> 594 us at 720p B = 5, 272.7 -> 266.7 us at B = 2; from 16 pixels up:
// the same (a 20-pixel level fits one unit either way); block width 24: 154.8 / 590 / 262.5 us, 16: 162 / 617 / 412 us.
// Very flat levels (H < 8) get wider blocks so that the unit count stays ~ n / rows_max.  At least units_min units per
// level when it has the rows.
// Unit u of a level: block (u % nbx, u / nbx), pixels [bx * bw, ..) x [by * bh, ..), clipped to the level.
constexpr int kGvBlockMinW = 32;
constexpr int kGvBlockW = 32;
struct GvGrid { int nbx, nby, bw, bh; };
__host__ __device__ inline GvGrid gv_level_grid(int H, int W, int units_min, int rows_max) {
  GvGrid g{1, 1, 1, 1};
  if (H <= 0 || W <= 0) { g.nbx = g.nby = 0; return g; }
  if (W < kGvBlockMinW && W <= rows_max) {
    g.nbx = 1; g.bw = W;
  } else {
    const int target = H >= rows_max / kGvBlockW ? kGvBlockW : rows_max / H;       // flat levels: wider blocks
    g.nbx = (W + target - 1) / target;
    g.bw = (W + g.nbx - 1) / g.nbx;
    g.nbx = (W + g.bw - 1) / g.bw;
  }
  g.bh = rows_max / g.bw;
  if (g.bh < 1) g.bh = 1;
  if (g.bh > H) g.bh = H;
  g.nby = (H + g.bh - 1) / g.bh;
  if (g.nbx * g.nby < units_min && g.nby < H) {           // small levels: at least units_min bands
    int want = (units_min + g.nbx - 1) / g.nbx;
    if (want > H) want = H;
    g.bh = (H + want - 1) / want;
    g.nby = (H + g.bh - 1) / g.bh;
  }
  return g;
}

// units of one level on either grad_value path: what decides its query split (gv_query_splits) -- shared by the grad_loc
// kernel (zeroing), the grad_value kernels and the 16-bit convert pass
__host__ __device__ inline int gv_level_units(int H, int W, int units_min, bool tiles) {
  if (tiles) {
    const GvGrid g = gv_level_grid(H, W, units_min, kGvTileRowsMax);
    return g.nbx * g.nby;
  }
  return gv_level_split(H * W, units_min, kGvRowsMax).units;
}

__host__ __device__ inline int gv_query_splits(int row_units, int Lq, int P, bool f32, int batch_heads) {
  if (!f32 || P != 4 || row_units > 4 || Lq < 1024) return 1;
  const int chunks = (Lq + 127) / 128;
  const int qs = (chunks + kQsChunks - 1) / kQsChunks;
  // round 4, pieces meeting in partial rows (no atomics): coarse cap 8 -> 4 from 32 pairs up (encoder-720p B = 5 611 -> 600 us;
  // 360p has 4 pieces either way), 8 -> 16 below (720p B = 2 272.7 -> 263.9 us; 16 at B = 5: 628 us, 4 at B = 2: 332 us)
  const int mid = batch_heads < 32 ? 4 * kQsMid : kQsMid;
  const int coarse = batch_heads < 32 ? kQsCoarseSmall : kQsCoarse;
  const int cap = row_units > 2 ? mid : coarse;          // middle levels: 3-4 row-units (960 pixels at 360p)
  return qs < 1 ? 1 : (qs > cap ? cap : qs);
}

// Tile-fed grad_value path: the query pieces of a split level do NOT meet through atomics (rounds 2-3 did: 4 M fp32 atomics
// per T=5 360p encoder call, issued 8 lanes x 16-B stride per row = the slow address pattern of tools/atomic_bench.hip,
// 80 G dwords/s: 44 us of the 87-us kernel, plus 7 us in the grad_loc kernel to zero the rows first -- found by timing
// ablations in round 4).  Every piece stores its rows, plain 16-B stores, into its own slab of fp32 PARTIAL rows in the
// workspace, and a small finishing kernel adds the pieces of each row in a fixed order and writes grad_value once (in its
// own dtype: the fp32 "split image" + convert pass of 16-bit values is gone too).  Layout per (batch, head): for every
// split level l in order, qs_l pieces x n_l pixels x 32 floats, starting at row  sum_{l' < l} qs_l' n_l'.
// A split level has at most 4 units of at most kGvTileRowsMax pixels (gv_query_splits), at most this many pieces:
__host__ __device__ inline int gv_split_pieces_max(int batch_heads) {          // = the caps of gv_query_splits
  const int mid = batch_heads < 32 ? 4 * kQsMid : kQsMid;
  const int coarse = batch_heads < 32 ? kQsCoarseSmall : kQsCoarse;
  return mid > coarse ? mid : coarse;
}
// A split level is either coarse (<= 2 units: <= 2 x 256 pixels, `coarse` pieces) or middle (3-4 units: <= 4 x 256 pixels,
// `mid` pieces), never both: a level contributes at most max(512 coarse, 1024 mid) rows, and all of them at most S x the
// larger piece count.  (Until round 4 the bound was min(S, 1024 L) x max(mid, coarse): twice this, 134 MB at B = 2 for the
// ~25 MB the pieces write, allocated by every backward call -- ADVICE r4.)
static_assert(kQsMid <= kQsCoarse && 4 * kQsMid <= kQsCoarseSmall,
              "msda_gvtiles_units_bound counts the extra workgroups of the split levels with the COARSE cap");
__host__ __device__ inline int64_t gv_partial_rows_bound(int S, int L, int batch_heads) {      // partial rows per (batch, head), an upper bound
  const int64_t mid = batch_heads < 32 ? 4 * kQsMid : kQsMid;
  const int64_t coarse = batch_heads < 32 ? kQsCoarseSmall : kQsCoarse;
  const int64_t per_level_c = int64_t(2) * kGvTileRowsMax * coarse, per_level_m = int64_t(4) * kGvTileRowsMax * mid;
  const int64_t by_levels = int64_t(L) * (per_level_c > per_level_m ? per_level_c : per_level_m);
  const int64_t by_pixels = int64_t(S) * (coarse > mid ? coarse : mid);
  return by_levels < by_pixels ? by_levels : by_pixels;
}

}  // namespace vnx
