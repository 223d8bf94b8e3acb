/*
 * include/vnext_hip_dev.h -- what the DEVELOPMENT build (vnext_amd/lib/libvnext_hip_dev.so: the product sources
 * compiled with -DVNX_DEV_VARIANTS plus the archived kernels of tools/experiments/msda_tile/) exports on top of
 * vnext_hip.h and vnext_hip_debug.h.  The product library (libvnext_hip.so) exports NONE of this: there a call
 * selects its kernels from its own arguments and nothing process-wide can change what it computes.
 *
 * Used by tests/ (parity of every kernel form, not only the automatically selected one), tools/kbench.hip and
 * the python tools (A/B timing).
 */
#ifndef VNEXT_HIP_DEV_H_
#define VNEXT_HIP_DEV_H_

#ifdef __cplusplus
extern "C" {
#endif

/*
 * Kernel selection override (process-wide, development build only).  Every exported entry point reads it once per call and
 * decodes it in ONE place -- decode_variant(), vnext_amd/csrc/vnx_common.h -- from which this list is written:
 *   0          automatic: what the product library always does.  Any number not named below: the same
 *   1          the generic kernels, forward and backward
 *   c = 2..5   tuned forward and grad_loc kernel: 8, 4, 2, 1 queries per wave, 4 waves per workgroup
 *   c = 12..15 the same with 1 wave per workgroup
 *   20..39     configuration c = variant - 20 (0 = by size) with the forward's prefetch phase on; 40..59: variant - 40, off
 *   60..67     configuration 13 with heads rotated over the XCDs by variant - 60; 68 the fixed head -> XCD map
 *   69         automatic configuration, 16-bit rows of the forward as 8 lanes x 8 B
 *              (below 100 any number but 0 also keeps the gather form of the grad_loc kernel where the slab form would run)
 *   100 + c    TIMING ABLATION: grad_loc / grad_attn alone, configuration c as above
 *   200 + u    grad_value units per level at least (u = 1..16)
 *   300 + c    the one-kernel backward whose grad_value goes through global atomics, configuration c
 *   400..429, 432..499  TIMING ABLATION: grad_value alone on the record- and tile-fed paths, of which
 *     408 / 412  record-fed kernel with phase stamps in shader-clock / wall-clock ticks (vnx_debug_read_rec_stamps)
 *     420 / 425  record-fed kernel in its LDS-slab form / its register-slab form without selection
 *                (these four force the record-fed path)
 *     441        whole backward, grad_value on the side stream as VNX_MSDA_FORK asks (self-decoding path)
 *     442        TIMING ABLATION: grad_value alone on the self-decoding path too
 *     444        whole backward, two launches where the paired kernel would run
 *     445..447   whole backward, paired kernel with the grad_value groups first / the grad_loc groups first / alternating
 *                (441 and 444..447 are whole backwards on the self-decoding path only: a call that takes the record- or
 *                tile-fed path under them is the ablation of their range)
 *   430 / 431  force the record-fed / the tile-fed grad_value path (whole backward)
 *   510        tile-fed path: the grad_loc kernel leaves a compact copy of the locations / weights
 *   700..702   the LDS-staged forward of tools/experiments/msda_tile/ (DESIGN.md section 3.1c/d); 701 / 702 with stamps of the
 *              first / second item of every workgroup (vnx_debug_read_tile_stamps); 720 the second LDS-staged forward
 *   701..798   ALSO, in the mask head's forward: variant - 700 runs per instance; 799 its strip kernel
 *   730 / 731  force / forbid the slab forward (and with it the slab form of the grad_loc kernel)
 *   733        the gather form of the grad_loc kernel where the slab form would run (the forward keeps its slab)
 *   734        the slab form of the fused grad_loc kernel; 737 the large slab for 16-bit values
 * The TIMING ABLATIONS skip one of the two backward kernels: wrong results by construction.
 */
void vnx_set_kernel_variant(int variant);
int vnx_get_kernel_variant(void);

/*
 * Kernel-span stamps (process-wide state, hence development build only).  While a buffer is armed every launch of a tuned
 * MSDA kernel takes a region of 2 x gridDim 64-bit words and each workgroup leaves {its start, its last wave's end} there in
 * constant-rate wall-clock ticks (vnx_debug_wall_clock_khz, vnext_hip_debug.h).  buf: n_words zero-filled 64-bit words;
 * nullptr disarms.  vnx_debug_stamp_regions -> number of regions handed out since arming; per region the kernel kind
 * (1 forward, 2 grad_loc / grad_attn, 3 grad_value, 4 the paired backward kernel), word offset, workgroups.
 */
void vnx_debug_arm_stamps(void* buf, long long n_words);
int vnx_debug_stamp_regions(int* kinds, long long* offsets, long long* blocks, int n);

/* phase stamps of the record-fed grad_value kernel (variants 408 / 412) and of the tiled forward (701 / 702): copies
 * n 64-bit words of the kernel's fixed device array to `host`; returns a hipError_t as int */
int vnx_debug_read_rec_stamps(unsigned long long* host, int n);
int vnx_debug_read_tile_stamps(unsigned long long* host, int n);
/* the same for the self-decoding grad_value kernel (msda_d32_gvdirect.hip), 8 stamps per workgroup, of a library built with
 * -DVNX_GVD_STAMPS (zeros otherwise) */
int vnx_debug_read_gvd_stamps(unsigned long long* host, int n);

#ifdef __cplusplus
}
#endif
#endif /* VNEXT_HIP_DEV_H_ */
