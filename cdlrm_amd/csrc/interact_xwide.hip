// The pairwise-dot interaction for 65 to 128 features (cdlrm_interact_xwide_fwd / _bwd): interact_features "dot"
// (model_no_ddp.py:272-293) where one sample's Gram matrix is 3 x 3 or 4 x 4 blocks of 32 x 32 and no longer fits one wave's
// registers.  Same operands and layouts as cdlrm_interact_wide_fwd / _bwd: feat [B, F, D], R[b] = [feature 0 (D) | pairs at
// pair_base(i) + j | pad], dfeat [B, F, D] with the direct path and act'(feature 0) applied to row 0.
//
// Work split: a 256-lane workgroup owns one sample at a time and strides over the batch; its four waves share the sample's block
// in LDS.  FP = 32 NB is F rounded up to 32 (NB = 3 or 4, a template argument); rows F .. FP - 1 are staged as zeros and their
// products are never stored.  One family for every D % 4 == 0: the block is staged 32 columns at a time into [FP][36] slices, a
// last slab narrower than 32 columns zero-filled.
//
// Staging: two slices.  While slab s feeds the MFMAs out of one, every lane holds its NB float4 of the NEXT step -- slab s + 1, or
// slab 0 of the workgroup's next sample -- in registers and writes them into the other slice behind the MFMAs; one workgroup
// barrier per slab closes the step.  No wave ever waits for a load it issued in the same step.
//
// Forward: wave w owns the diagonal block (w, w) and the blocks (w + 1, w), (w + 2, w) with the block rows taken modulo NB --
// stored transposed where the row wraps below the column: 3 / 3 / 2 / 2 blocks at NB = 4, 2 / 2 / 2 / 0 at NB = 3.  It reads the
// (up to) three row fragments of its blocks once per k-group and uses fragment 0 as the B operand of all of them.  The
// accumulators run across all slabs and are scattered into ONE staged pair row in LDS, which leaves as float4 stores by all 256
// lanes, pad words as 0.  The dense part R[b, :D] never passes LDS: the lanes that loaded row 0 store it from their registers.
//
// Backward: the dR row is staged once per sample (prefetched a sample ahead in registers).  Wave w owns row block w of
// S = G + G^T: it builds its A fragments (FP / 2 values per lane) once per sample and per slab runs one f32x16 accumulator over
// FP / 2 k-steps, the B operand read from the shared slice.  At NB = 3 wave 3 owns no row block: it loads, stages and waits at
// the barriers only -- splitting three row blocks over four waves by k-range would cost an LDS add and a second barrier per
// slab for kernels that the matrix pipe does not limit.  Tiles leave through a private [32][36] tile per wave as float4 rows.
//
// Scalar tiers on workgroup-uniform branches: an R / dR that is not 16-byte aligned or has a pitch without whole float4 words,
// an unaligned dfeat.
#include "interact_lds.h"

typedef float v4f __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
static inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// accumulator register r of lane half lk: row of its 32x32 block
__device__ __forceinline__ int ix_acc_row(int r, int lk) { return (r & 3) + 8 * (r >> 2) + 4 * lk; }

// A lane's share of one slab: word lane % 8 of rows lane / 8 + 32 i.  Rows >= F and columns >= D are zeros.
template <int NB>
struct IxLoader {
    v4f v[NB];
    const v4f* feat4;
    int F, D4, row, word;

    __device__ __forceinline__ void init(const float* feat, int F_, int D4_) {
        feat4 = reinterpret_cast<const v4f*>(feat);
        F = F_;
        D4 = D4_;
        row = threadIdx.x >> 3;
        word = threadIdx.x & 7;
    }
    __device__ __forceinline__ void load(int64_t b, int s) {
        // every load is issued, from a clamped address inside the sample's block; what lies outside it becomes zeros
        const int c4 = 8 * s + word;
        const v4f* src = feat4 + b * F * D4 + min(c4, D4 - 1);
#pragma unroll
        for (int i = 0; i < NB; ++i) {
            const v4f x = src[min(row + 32 * i, F - 1) * D4], z = {0.f, 0.f, 0.f, 0.f};
            v[i] = row + 32 * i < F && c4 < D4 ? x : z;
        }
    }
    __device__ __forceinline__ void stage(float* __restrict__ Ts) const {
#pragma unroll
        for (int i = 0; i < NB; ++i) *reinterpret_cast<v4f*>(Ts + (row + 32 * i) * IX_PITCH + 4 * word) = v[i];
    }
};

// the (sample, slab) behind (b, s) in a workgroup's walk; false behind its last one
__device__ __forceinline__ bool ix_next(int64_t b, int s, int NS, int64_t B, int64_t& bn, int& sn) {
    sn = s + 1;
    bn = b;
    if (sn == NS) {
        sn = 0;
        bn = b + gridDim.x;
    }
    return bn < B;
}

template <int NB>
__global__ void __launch_bounds__(256, 2) k_interact_xwide_fwd(const float* __restrict__ feat, int64_t B, int F, int D, int itself,
                                                               float* __restrict__ R, int64_t ld_r, int vec) {
    constexpr int FP = 32 * NB;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* Os = smem + 2 * ix_slice(FP);        // the pair row [pairs | pad words]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int lr = lane & 31, lk = lane >> 5;
    const int NS = (D + 31) >> 5;
    const int npairs = pair_base(F, itself), P4 = (npairs + 3) >> 2;
    int64_t b = blockIdx.x;
    if (b >= B) return;                         // (the whole workgroup)
    // blocks (f[q], f[0]), q < nblk
    const int nblk = wave >= NB ? 0 : (NB == 4 && wave < 2 ? 3 : 2);
    int f[3];
#pragma unroll
    for (int q = 0; q < 3; ++q) f[q] = (wave + q) % NB;
    IxLoader<NB> ld;
    ld.init(feat, F, D >> 2);
    // the staging of step (b, s) into a slice; row 0 is the dense part of R[b]
    auto stage = [&](float* Ts, int64_t b, int s) __attribute__((always_inline)) {
        ld.stage(Ts);
        const int col = 32 * s + 4 * ld.word;
        if (ld.row == 0 && col < D) {
            float* out = R + b * ld_r + col;
            if (vec) *reinterpret_cast<v4f*>(out) = ld.v[0];
            else { out[0] = ld.v[0][0]; out[1] = ld.v[0][1]; out[2] = ld.v[0][2]; out[3] = ld.v[0][3]; }
        }
    };
    if ((int)threadIdx.x < 4 * P4 - npairs) Os[npairs + threadIdx.x] = 0.f;     // the pad words: written once, no pair lands there
    ld.load(b, 0);
    stage(smem, b, 0);
    __syncthreads();
    f32x16 a0, a1, a2;
    int s = 0, cur = 0;
    for (;;) {
        int64_t bn;
        int sn;
        const bool more = ix_next(b, s, NS, B, bn, sn);
        if (more) ld.load(bn, sn);
        __builtin_amdgcn_sched_barrier(0);
        if (s == 0) {
#pragma unroll
            for (int r = 0; r < 16; ++r) a0[r] = a1[r] = a2[r] = 0.f;
        }
        const float* Ts = smem + cur * ix_slice(FP);
        const float* tp = Ts + lr * IX_PITCH + 4 * lk;      // lane half lk: contraction indices 8 g + 4 lk .. + 3 of a group
        const int ng = min(4, (D - 32 * s + 7) >> 3);       // k-groups of 8 columns that hold any
        if (nblk) {
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                if (g >= ng) break;
                const v4f x0 = *reinterpret_cast<const v4f*>(tp + 32 * f[0] * IX_PITCH + 8 * g);
                const v4f x1 = *reinterpret_cast<const v4f*>(tp + 32 * f[1] * IX_PITCH + 8 * g);
                if (nblk == 3) {
                    const v4f x2 = *reinterpret_cast<const v4f*>(tp + 32 * f[2] * IX_PITCH + 8 * g);
#pragma unroll
                    for (int c = 0; c < 4; ++c) {
                        a0 = __builtin_amdgcn_mfma_f32_32x32x2f32(x0[c], x0[c], a0, 0, 0, 0);
                        a1 = __builtin_amdgcn_mfma_f32_32x32x2f32(x1[c], x0[c], a1, 0, 0, 0);
                        a2 = __builtin_amdgcn_mfma_f32_32x32x2f32(x2[c], x0[c], a2, 0, 0, 0);
                    }
                } else {
#pragma unroll
                    for (int c = 0; c < 4; ++c) {
                        a0 = __builtin_amdgcn_mfma_f32_32x32x2f32(x0[c], x0[c], a0, 0, 0, 0);
                        a1 = __builtin_amdgcn_mfma_f32_32x32x2f32(x1[c], x0[c], a1, 0, 0, 0);
                    }
                }
            }
        }
        __builtin_amdgcn_sched_barrier(0);
        const bool last = s == NS - 1;
        if (last) {
            // One slab per sample: the previous sample's row may still be leaving (its stores follow the barrier of its last
            // slab, which is the one in front of this step).  With more slabs a slab barrier lies in between.
            if (NS == 1) __syncthreads();
            if (nblk) {
                const int j = 32 * f[0] + lr;
#pragma unroll
                for (int q = 0; q < 3; ++q) {
                    if (q >= nblk) break;
                    const f32x16& a = q == 0 ? a0 : q == 1 ? a1 : a2;
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int i = 32 * f[q] + ix_acc_row(r, lk);
                        const int hi = max(i, j), lo = min(i, j);
                        // the diagonal block holds every pair twice: its lower triangle only
                        const bool ok = hi < F && (q ? true : i > j || (i == j && itself));
                        if (ok) Os[pair_base(hi, itself) + lo] = a[r];
                    }
                }
            }
        }
        if (more) stage(smem + (cur ^ 1) * ix_slice(FP), bn, sn);
        __syncthreads();
        if (last) {
            float* out = R + b * ld_r + D;
            if (vec) {
                for (int e = threadIdx.x; e < P4; e += 256)
                    *reinterpret_cast<v4f*>(out + 4 * e) = *reinterpret_cast<const v4f*>(Os + 4 * e);
            } else {
                for (int e = threadIdx.x; e < npairs; e += 256) out[e] = Os[e];
            }
        }
        if (!more) break;
        b = bn;
        s = sn;
        cur ^= 1;
    }
}

// One wave per SIMD: bounded to two, the NB = 4 instance spills (172 to 232 bytes per lane in every arrangement tried); unbounded,
// what does not fit 256 VGPRs is parked in AGPRs and there is no scratch.
template <int NB>
__global__ void __launch_bounds__(256) k_interact_xwide_bwd(const float* __restrict__ feat, const float* __restrict__ dR,
                                                               int64_t ld_r, int64_t B, int F, int D, int itself, int x_act,
                                                               float* __restrict__ dfeat, int vec_r, int vec_df) {
    constexpr int FP = 32 * NB;
    constexpr int NG = (512 + ix_pair_row(FP * (FP + 1) / 2) + 1023) / 1024;    // float4 per lane of the longest dR row
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int lr = lane & 31, lk = lane >> 5;
    const int NS = (D + 31) >> 5;
    const int npairs = pair_base(F, itself);
    const int G4 = (D + ix_pair_row(npairs)) >> 2;      // float4 words of one dR row (the pad words lie inside the pitch)
    float* Gs = smem + 2 * ix_slice(FP);                // the dR row [dense D | pairs | pad words]
    float* Os = Gs + D + ix_pair_row(npairs) + wave * ix_out_tile();
    const bool active = wave < NB;                      // owns row block `wave` of S
    int64_t b = blockIdx.x;
    if (b >= B) return;                                 // (the whole workgroup)
    IxLoader<NB> ld;
    ld.init(feat, F, D >> 2);
    v4f gn[NG];
    auto fetch_grad = [&](int64_t b) __attribute__((always_inline)) {
        if (!vec_r) return;
        const v4f* src = reinterpret_cast<const v4f*>(dR + b * ld_r);
#pragma unroll
        for (int i = 0; i < NG; ++i) gn[i] = src[min((int)threadIdx.x + 256 * i, G4 - 1)];      // (past the row: its last word again)
    };
    float sreg[FP / 2];
    // head of sample b: its dR row into LDS, the A fragments of S = G + G^T out of it (lane holds S[32 wave + lr][lk + 2 m]);
    // off the diagonal exactly one of G_ij, G_ji exists
    auto head = [&](int64_t b) __attribute__((always_inline)) {
        if (vec_r) {
#pragma unroll
            for (int i = 0; i < NG; ++i) *reinterpret_cast<v4f*>(Gs + 4 * min((int)threadIdx.x + 256 * i, G4 - 1)) = gn[i];
        } else {
            const float* src = dR + b * ld_r;
            for (int e = threadIdx.x; e < D + npairs; e += 256) Gs[e] = src[e];
        }
        __syncthreads();
        if (b + gridDim.x < B) fetch_grad(b + gridDim.x);
        if (active) {
            // the row is made opaque per sample: otherwise the FP / 2 addresses and masks below, which depend on the lane alone,
            // are hoisted out of the sample loop and live in registers beside the fragments (spills)
            int i = 32 * wave + lr;
            asm volatile("" : "+v"(i));
#pragma unroll
            for (int m = 0; m < FP / 2; ++m) {
                const int j = lk + 2 * m;
                const int hi = max(i, j), lo = min(i, j);
                const bool valid = hi < F && (hi != lo || itself);
                float v = Gs[valid ? D + pair_base(hi, itself) + lo : 0];
                v = valid ? v : 0.f;
                sreg[m] = hi == lo ? v + v : v;
                if (m % 8 == 7) __builtin_amdgcn_sched_barrier(0);      // eight reads in flight: their addresses and masks die here
            }
        }
    };
    fetch_grad(b);
    ld.load(b, 0);
    ld.stage(smem);
    head(b);                // (its barrier also publishes the first slice)
    int s = 0, cur = 0;
    for (;;) {
        int64_t bn;
        int sn;
        const bool more = ix_next(b, s, NS, B, bn, sn);
        if (more) ld.load(bn, sn);
        __builtin_amdgcn_sched_barrier(0);
        if (active) {
            const float* Ts = smem + cur * ix_slice(FP);
            const float* tp = Ts + lk * IX_PITCH + lr;
            f32x16 acc;
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[r] = 0.f;
            // k-step m: rows lk + 2 m of T.  Eight B operands are read while the eight before them feed the MFMAs: left to itself
            // the scheduler reads all FP / 2 first, which does not fit beside the fragments.
            float t[2][8];
#pragma unroll
            for (int u = 0; u < 8; ++u) t[0][u] = tp[2 * u * IX_PITCH];
#pragma unroll
            for (int c = 0; c < FP / 16; ++c) {
                if (c + 1 < FP / 16) {
#pragma unroll
                    for (int u = 0; u < 8; ++u) t[(c + 1) & 1][u] = tp[2 * (8 * (c + 1) + u) * IX_PITCH];
                }
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int u = 0; u < 8; ++u) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(sreg[8 * c + u], t[c & 1][u], acc, 0, 0, 0);
                __builtin_amdgcn_sched_barrier(0);
            }
            if (wave == 0) {    // row 0 (register 0 of the lanes lk = 0): the dense feature: + direct path, * act'(bottom-MLP output)
                float v = acc[0] + Gs[32 * s + lr];
                const float y = Ts[lr];
                if (x_act == 1) v = y > 0.f ? v : 0.f;
                else if (x_act == 2) v = v * ((1.0f - y) * y);
                acc[0] = lk == 0 ? v : acc[0];
            }
            float* out = dfeat + (b * F + 32 * wave) * D + 32 * s;
            if (vec_df) {
#pragma unroll
                for (int r = 0; r < 16; ++r) Os[ix_acc_row(r, lk) * IX_PITCH + lr] = acc[r];
#pragma unroll
                for (int k = 0; k < 4; ++k) {       // whole float4 words of rows < F and columns < D only
                    const int row = 8 * k + (lane >> 3), c4 = lane & 7;
                    if (32 * wave + row < F && 32 * s + 4 * c4 < D)
                        *reinterpret_cast<v4f*>(out + (int64_t)row * D + 4 * c4) = *reinterpret_cast<const v4f*>(Os + row * IX_PITCH + 4 * c4);
                }
            } else if (32 * s + lr < D) {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int row = ix_acc_row(r, lk);
                    if (32 * wave + row < F) out[(int64_t)row * D + lr] = acc[r];
                }
            }
        }
        __builtin_amdgcn_sched_barrier(0);
        if (more) ld.stage(smem + (cur ^ 1) * ix_slice(FP));
        __syncthreads();
        if (!more) break;
        b = bn;
        s = sn;
        cur ^= 1;
        if (s == 0) head(b);
    }
}

// ---- the host side: one plan, two entry points, one query ----------------------------------------------------------------------
struct IxPlan {
    int nb;             // 32-row blocks of the Gram matrix: 3 (F <= 96) or 4
    int ns;             // 32-column slabs of a sample
    bool vec_r;         // R / dR rows are whole aligned float4 words
    bool vec_df;        // dfeat is 16-byte aligned
    int64_t grid;       // workgroups of 256 lanes: a sample per workgroup, striding
    size_t lds;         // dynamic LDS bytes of the launch
};

// The whole LDS budget of both kernels.  aligned_r: R (forward) / dR (backward) is 16-byte aligned; aligned_dfeat: dfeat is.
static IxPlan xwide_plan(int op, int64_t B, int F, int D, int itself, int64_t ld_r, bool aligned_r, bool aligned_dfeat) {
    IxPlan p{};
    const int npairs = itself ? F * (F + 1) / 2 : F * (F - 1) / 2, width = D + npairs;
    p.nb = F <= 96 ? 3 : 4;
    p.ns = (D + 31) / 32;
    p.vec_r = ld_r % 4 == 0 && aligned_r && ld_r >= ((width + 3) & ~3);
    p.vec_df = aligned_dfeat;
    const int floats = op == CDLRM_IA_OP_FWD ? ix_fwd_floats(32 * p.nb, npairs) : ix_bwd_floats(32 * p.nb, D, npairs);
    p.lds = (size_t)floats * sizeof(float);
    // forward: two workgroups per CU (256 CUs) -- half a register file each, and 2 x 69 KB of LDS at the most.  Backward: one.
    const int64_t cap = op == CDLRM_IA_OP_FWD ? 512 : 256;
    p.grid = B < cap ? B : cap;
    return p;
}

#define IX_SHAPE_OK(F, D) ((F) > 64 && (F) <= 128 && (D) >= 4 && (D) % 4 == 0 && (D) <= 512)
#define IX_SHAPE_MSG "unsupported shape (64<F<=128, D%4==0, D<=512)"
#define IX_WIDTH(F, D, itself) ((D) + ((itself) ? (F) * ((F) + 1) / 2 : (F) * ((F) - 1) / 2))

extern "C" int cdlrm_interact_xwide_fwd(const float* feat, int64_t B, int32_t F, int32_t D, int32_t itself, float* R,
                                        int64_t ld_r, void* stream) {
    CDLRM_REQUIRE(feat && R && B >= 0 && IX_SHAPE_OK(F, D), IX_SHAPE_MSG);
    CDLRM_REQUIRE(aligned16(feat) && ld_r >= IX_WIDTH(F, D, itself), "alignment / ld_r");
    const IxPlan p = xwide_plan(CDLRM_IA_OP_FWD, B, F, D, itself, ld_r, aligned16(R), false);
    CDLRM_REQUIRE(p.lds <= 160 * 1024, "LDS budget");
    if (B == 0) return 0;
    if (p.nb == 3) return ia_launch<k_interact_xwide_fwd<3>>(p, stream, false, feat, B, F, D, itself, R, ld_r, (int)p.vec_r);
    return ia_launch<k_interact_xwide_fwd<4>>(p, stream, false, feat, B, F, D, itself, R, ld_r, (int)p.vec_r);
}

extern "C" int cdlrm_interact_xwide_bwd(const float* feat, const float* dR, int64_t ld_r, int64_t B, int32_t F, int32_t D,
                                        int32_t itself, int32_t x_act, float* dfeat, void* stream) {
    CdlrmStopScope stop_scope;          // (first: every exit below flushes an attached completion event)
    CDLRM_REQUIRE(feat && dR && dfeat && B >= 0 && IX_SHAPE_OK(F, D), IX_SHAPE_MSG);
    CDLRM_REQUIRE(aligned16(feat) && ld_r >= IX_WIDTH(F, D, itself), "alignment / ld_r");
    const IxPlan p = xwide_plan(CDLRM_IA_OP_BWD, B, F, D, itself, ld_r, aligned16(dR), aligned16(dfeat));
    CDLRM_REQUIRE(p.lds <= 160 * 1024, "LDS budget");
    if (B == 0) return 0;
    if (p.nb == 3)
        return ia_launch<k_interact_xwide_bwd<3>>(p, stream, true, feat, dR, ld_r, B, F, D, itself, x_act, dfeat, (int)p.vec_r, (int)p.vec_df);
    return ia_launch<k_interact_xwide_bwd<4>>(p, stream, true, feat, dR, ld_r, B, F, D, itself, x_act, dfeat, (int)p.vec_r, (int)p.vec_df);
}

extern "C" int cdlrm_interact_xwide_route(int32_t op, int64_t B, int32_t F, int32_t D, int32_t itself, int64_t ld_r,
                                          int32_t aligned, struct cdlrm_interact_route* out) {
    CDLRM_REQUIRE(out && (op == CDLRM_IA_OP_FWD || op == CDLRM_IA_OP_BWD) && B >= 0, "bad argument");
    CDLRM_REQUIRE(IX_SHAPE_OK(F, D), IX_SHAPE_MSG);
    CDLRM_REQUIRE(ld_r >= IX_WIDTH(F, D, itself), "alignment / ld_r");
    const IxPlan p = xwide_plan(op, B, F, D, itself, ld_r, aligned & 1, aligned & 2);
    CDLRM_REQUIRE(p.lds <= 160 * 1024, "LDS budget");
    out->family = CDLRM_IA_XWIDE; out->d4 = D / 4; out->ns = p.ns; out->reserved = 0;
    out->grid = p.grid; out->lds_bytes = (int64_t)p.lds;
    return 0;
}
