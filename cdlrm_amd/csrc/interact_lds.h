// The pair layout and the LDS footprints of the interaction kernels, shared by dense.hip (k_interact_*) and
// bag_interact.hip (k_bag_interact_*).
#pragma once
#include "common.h"

__device__ __forceinline__ int pair_base(int i, int itself) { return itself ? i * (i + 1) / 2 : i * (i - 1) / 2; }

// ---- LDS footprints of the interaction kernels, floats per wave (a workgroup is four waves, each with a slice of its own) ----
// Written down ONCE: the kernels carve their slices with these and interact_plan() sizes the launch's dynamic LDS from them.
// Generic pair (any D): the feature tile [32][D + 1] + 32; the backward stages the pair gradients (padded to 4) behind it.
__host__ __device__ constexpr int ia_generic_tile(int D) { return 32 * (D + 1) + 32; }
__host__ __device__ constexpr int ia_generic_bwd_floats(int D, int npairs) { return ia_generic_tile(D) + ((npairs + 3) & ~3); }
// Pipelined kernels (D = 4 D4 in 32 / 64 / 128 / 256).  A whole-row tile is [32][D + 4], a column slab's slice [32][D / NS + 4];
// a staged dR row is the dense part + up to 32 * 33 / 2 pair gradients, a staged output row that + the pad word.
__host__ __device__ constexpr int ia_row_tile(int D4) { return 32 * (4 * D4 + 4); }
__host__ __device__ constexpr int ia_slab_slice(int D4, int NS) { return 32 * (4 * D4 / NS + 4); }
__host__ __device__ constexpr int ia_grad_row(int D4) { return 4 * D4 + 528; }
__host__ __device__ constexpr int ia_out_row(int D4) { return 4 * D4 + 532; }
__host__ __device__ constexpr int ia_fwd_p_floats(int D4) { return ia_row_tile(D4); }
__host__ __device__ constexpr int ia_bwd_p_floats(int D4) { return ia_row_tile(D4) + ia_grad_row(D4); }
__host__ __device__ constexpr int ia_fwd_s_slices(int D4, int NS, bool DB) { return (DB ? 2 : 1) * ia_slab_slice(D4, NS); }
__host__ __device__ constexpr int ia_fwd_s_floats(int D4, int NS, bool DB) { return ia_fwd_s_slices(D4, NS, DB) + ia_out_row(D4); }
__host__ __device__ constexpr int ia_bwd_s_floats(int D4, int NS) { return ia_slab_slice(D4, NS) + ia_grad_row(D4); }
// Wide kernels (interact_wide.hip, 32 < F <= 64): the Gram matrix is 64 x 64.  Pipelined pair (D = 4 D4 in 32 / 64 / 128 / 256):
// a slab's slice is [64][32 + 4]; a staged dR row is the dense part + up to 64 * 65 / 2 pair gradients, a staged output row
// that + the pad word.  Whole-row pair (any D): the feature tile [64][D + 1] + 32; the backward stages the pair gradients
// (padded to 4) behind it.
__host__ __device__ constexpr int iw_slab_slice() { return 64 * 36; }
__host__ __device__ constexpr int iw_grad_row(int D4) { return 4 * D4 + 2080; }
__host__ __device__ constexpr int iw_out_row(int D4) { return 4 * D4 + 2084; }
__host__ __device__ constexpr int iw_fwd_floats(int D4) { return iw_slab_slice() + iw_out_row(D4); }
__host__ __device__ constexpr int iw_bwd_floats(int D4) { return iw_slab_slice() + iw_grad_row(D4); }
// The gather variants of the pipelined pair keep the row offsets of one sample (64 words) behind the wave's slice.
__host__ __device__ constexpr int iw_gather_table() { return 64; }
__host__ __device__ constexpr int iw_row_tile(int D) { return 64 * (D + 1) + 32; }
__host__ __device__ constexpr int iw_row_bwd_floats(int D, int npairs) { return iw_row_tile(D) + ((npairs + 3) & ~3); }
// Extra-wide kernels (interact_xwide.hip, 64 < F <= 128): the four waves of a workgroup share ONE sample, so these are floats per
// workgroup.  FP is F rounded up to 32.  Two [FP][32 + 4] slices (double-buffered slabs); the forward stages the pair row (pairs
// padded to 4) behind them, the backward the whole dR row [D | pairs padded to 4] and a [32][36] output tile per wave.
#define IX_PITCH 36
__host__ __device__ constexpr int ix_slice(int FP) { return FP * IX_PITCH; }
__host__ __device__ constexpr int ix_pair_row(int npairs) { return (npairs + 3) & ~3; }
__host__ __device__ constexpr int ix_out_tile() { return 32 * IX_PITCH; }
__host__ __device__ constexpr int ix_fwd_floats(int FP, int npairs) { return 2 * ix_slice(FP) + ix_pair_row(npairs); }
__host__ __device__ constexpr int ix_bwd_floats(int FP, int D, int npairs) {
    return 2 * ix_slice(FP) + D + ix_pair_row(npairs) + 4 * ix_out_tile();
}
// bf16 / bf16x3 extra-wide kernels (interact_xwide_b16.hip): the slices hold PL bf16 planes (1: hi, 2: hi and lo)
// instead of fp32 words; footprints still in floats per workgroup.  Forward: a plane is [FP][32 + 8] bf16, contraction (column)
// contiguous -- an 80-byte pitch, an odd multiple of 16 B.  Backward: a plane is the TRANSPOSE [32][FP + 8] bf16, contraction
// (feature) contiguous -- 208 / 272 bytes, odd multiples of 16 B too -- and row 0 of the slab stays fp32 beside each slice (32
// words: act' needs the bottom MLP's output unrounded).  Pair row, dR row and output tiles are those of the fp32 kernels.
#define IXB_FWD_PITCH 40
__host__ __device__ constexpr int ixb_bwd_pitch(int FP) { return FP + 8; }
__host__ __device__ constexpr int ixb_fwd_slice(int FP, int PL) { return PL * FP * IXB_FWD_PITCH / 2; }
__host__ __device__ constexpr int ixb_bwd_slice(int FP, int PL) { return PL * 32 * ixb_bwd_pitch(FP) / 2; }
__host__ __device__ constexpr int ixb_row0() { return 32; }
__host__ __device__ constexpr int ixb_fwd_floats(int FP, int PL, int npairs) { return 2 * ixb_fwd_slice(FP, PL) + ix_pair_row(npairs); }
__host__ __device__ constexpr int ixb_bwd_floats(int FP, int PL, int D, int npairs) {
    return 2 * ixb_bwd_slice(FP, PL) + 2 * ixb_row0() + D + ix_pair_row(npairs) + 4 * ix_out_tile();
}

// ---- host helpers of the entry points in dense.hip and interact_wide.hip --------------------------------------------------------
// run-time D4 of the pipelined kernels -> compile-time: fn(std::integral_constant<int, D4>{})
template <typename Fn>
static int ia_with_d4(int d4, Fn&& fn) {
    switch (d4) {
        case 8: return fn(std::integral_constant<int, 8>{});
        case 16: return fn(std::integral_constant<int, 16>{});
        case 32: return fn(std::integral_constant<int, 32>{});
        case 64: return fn(std::integral_constant<int, 64>{});
    }
    cdlrm_set_error("interaction: no pipelined kernel at D = %d", 4 * d4);
    return CDLRM_EINVAL;
}

// One launch of a plan (its .grid workgroups of 256 lanes, its .lds bytes of dynamic LDS).
// carry: an attached completion event (CdlrmStopScope of the entry point) rides on the launch as its stop event
template <auto Kernel, typename Plan, typename... Args>
static int ia_launch(const Plan& p, void* stream, bool carry, Args... args) {
    const int rc = cdlrm_grant_dynamic_lds<Kernel>(p.lds);
    if (rc) return rc;
    const dim3 grid((unsigned)p.grid), block(256);
    if (carry) CDLRM_LAUNCH_EV(Kernel, grid, block, p.lds, (hipStream_t)stream, args...);
    else hipLaunchKernelGGL(Kernel, grid, block, p.lds, (hipStream_t)stream, args...);
    CDLRM_LAUNCH_CHECK();
    return 0;
}
