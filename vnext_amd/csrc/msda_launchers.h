// msda_launchers.h -- the host-side launchers of the MSDA kernels, one per source file, as capi.hip calls them.
// Included by capi.hip and by every file that defines one of them.
#pragma once
#include "msda_units.h"

namespace vnx {

// msda_generic.hip
int msda_forward_generic(int, int, const void*, const int64_t*, const int64_t*, const void*, const void*, void*, MsdaDims, hipStream_t);
int msda_backward_generic(int, int, const void*, const int64_t*, const int64_t*, const void*,
                          const void*, const void*, void*, void*, void*, MsdaDims,
                          int only_if_not_packed, hipStream_t);
int convert_f32_to(int, const void*, void*, int64_t, const int64_t*, const int64_t*, int, int, hipStream_t);
int zero_if_not_packed(const int64_t*, const int64_t*, int, int, void*, size_t, hipStream_t);

// msda_d32.hip.  `kv`: the variant the entry point read.
bool msda_d32_fwd_supported(int vdt, int ldt, const MsdaDims& d);
bool msda_d32_bwd_supported(int vdt, int ldt, const MsdaDims& d);
int msda_forward_d32(int, int, const void*, const int64_t*, const int64_t*, const void*,
                     const void*, void*, MsdaDims, const KernelVariant& kv, hipStream_t);
// atomics: grad_value through global atomics into `gv` by the same kernel; otherwise grad_loc / grad_attn only, leaving
// sample records or tile words for a grad_value kernel (gv: the fp32 rows of the query-split levels to zero, or null)
int msda_backward_d32(int, int, const void*, const int64_t*, const int64_t*, const void*,
                      const void*, const void*, void* gv, void*, void*, MsdaDims, bool atomics, const KernelVariant& kv,
                      void* records, void* tile_summary, float* tile_copy, hipStream_t);
int msda_bwd_tile_queries(const MsdaDims& d, FwdCfg forced);      // queries per tile word of the grad_loc kernel
bool msda_d32_fused_supported(int vdt, int ldt, const MsdaDims& d);
int msda_fused_d32(bool backward, int vdt, int ldt, const void* value, const int64_t* shapes, const int64_t* lsi,
                   const void* raw_off, const void* raw_logit, const void* grad_out, void* out_or_grad_off,
                   void* grad_logit, MsdaDims d, void* records, const void* reference, float* grad_reference,
                   int ref_dim, int ref_div, void* grad_value_f32, void* tile_summary, float* tile_loc, float* tile_attn,
                   const KernelVariant& kv, hipStream_t stream, int ref_f32);
bool msda_backward_pair_supported(int vdt, int ldt, const MsdaDims& d);
int msda_backward_pair_d32(int vdt, const void* value, const int64_t*, const int64_t*, const void* loc, const void* attn,
                           const void* grad_out, void* grad_value, void* grad_loc, void* grad_attn, MsdaDims, int order,
                           hipStream_t);

// msda_d32_gvtiles.hip
bool msda_d32_gvtiles_supported(int vdt, int ldt, const MsdaDims& d);
size_t msda_gvtiles_summary_bytes(const MsdaDims& d, int tile_queries);
size_t msda_gvtiles_partial_bytes(const MsdaDims& d);
int msda_backward_gvtiles_d32(int vdt, int ldt, const int64_t*, const int64_t*, const void* loc, const void* attn,
                              const void* summaries, const void* grad_out, void* grad_value, MsdaDims,
                              int tile_queries, int gv_units, float* partials, bool compact, hipStream_t);

// msda_d32_gvrec.hip
bool msda_d32_gvrec_supported(int vdt, int ldt, const MsdaDims& d);
size_t msda_gvrec_record_bytes(const MsdaDims& d);
int msda_backward_gvrec_d32(int vdt, const int64_t*, const int64_t*, const void* records, const void*,
                            void*, MsdaDims, const KernelVariant& kv, float* split_image, hipStream_t);
int msda_split_levels_convert(int vdt, const int64_t*, const int64_t*, const float* image, void* grad_value, MsdaDims, bool tiles,
                              int gv_units, hipStream_t);

// msda_d32_gvdirect.hip
bool msda_d32_gvdirect_supported(int vdt, int ldt, const MsdaDims& d);
int msda_gvdirect_units_bound(const MsdaDims& d, int ut, int rows);
int msda_backward_gvdirect_d32(int vdt, int ldt, const int64_t*, const int64_t*, const void* loc, const void* attn,
                               const void* grad_out, void* grad_value, MsdaDims, bool compact, hipStream_t);

#ifdef VNX_DEV_VARIANTS      // the LDS-staged forwards: tools/experiments/msda_tile/ (development build only)
bool msda_tile_fwd_supported(int vdt, int ldt, const MsdaDims& d);
int msda_forward_tile(const void*, const int64_t*, const int64_t*, const void*, const void*, void*, MsdaDims,
                      const FusedArgs*, int debug, hipStream_t);
bool msda_tile2_fwd_supported(int vdt, int ldt, const MsdaDims& d);
int msda_forward_tile2(const void*, const int64_t*, const int64_t*, const void*, const void*, void*, MsdaDims, hipStream_t);
#endif

}  // namespace vnx
