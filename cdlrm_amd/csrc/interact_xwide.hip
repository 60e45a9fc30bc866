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
//
// The pair also runs as the fused gather (cdlrm_gather_interact_xwide_fwd / _bwd): the same kernels with the
// loader's source switched (IxLoader<NB, G>), the rows read from the cache by slot id; the float4 tiers only.
#include "interact_lds.h"

typedef float v4f __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
static inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// accumulator register r of lane half lk: row of its 32x32 block
__device__ __forceinline__ int ix_acc_row(int r, int lk) { return (r & 3) + 8 * (r >> 2) + 4 * lk; }

// G (the fused gather, cdlrm_gather_interact_xwide_fwd / _bwd): row 0 of a sample's block is the dense feature
// x[b] (pitch ldx4 words), rows 1 .. F - 1 are the cache rows weight[tab[t].row_base + slots[t * n + b]], t = row - 1 -- the
// [B, T, D] block cdlrm_embbag_fwd would write and the kernels below read back never exists.  Same operands in the same lanes,
// same MFMA order: bit-identical to gather + interaction.
struct IxGather {
    const TableDesc* tab;       // row_base of every table's cache rows
    const v4f* weight;          // cache rows (and the auxiliary rows behind them), D4 float4 words each; fewer than 2^31 words
    const int32_t* slots;       // [T, n] slot ids of the batch (T * n < 2^31, checked by the host)
    int n;
    int64_t ldx4;               // pitch of the dense-feature rows, float4 words
};

// A lane's share of one slab: word lane % 8 of rows tid / 8 + 32 i.  Rows >= F and columns >= D are zeros.
//
// G: the rows come by slot id, and slot id -> address -> row is a dependent chain of two memory round trips.  It is taken apart
// over three samples of the workgroup's walk, in registers: at the top of a sample's FIRST step a lane requests the NB slot ids of
// its rows for the sample two ahead (idb; the eight lanes of a row read the same word) after moving the ids that request brought
// a sample ago into ida; at the top of the sample's LAST step ida becomes off[] -- 32-bit float4-word offsets from `weight` -- right
// in front of load(bn, 0), and off[] then serves slabs 1 .. NS - 1 of that sample.  A request is at least a whole step old when
// its ids are touched (NS = 1: exactly one step; the stage() of that step has waited for younger loads already), so no lane waits
// for a slot id inside the step that asked for it.  Row 0 comes from x by a select on register 0 of lanes 0 .. 7; the row slot
// of rows 0 and >= F is clamped into 1 .. F - 1, so every id and row load is issued and the spare ones are replaced by zeros.
template <int NB, bool G = false>
struct IxLoader {
    v4f v[NB];
    const v4f* feat4;           // G: x
    int F, D4, row, word;
    const v4f* w4;              // G: the cache rows
    int64_t ldx4;
    const int32_t* slots;
    int srow[NB], rbase[NB];    // where the row's table keeps its slot ids; row_base * D4 of that table
    int ida[NB], idb[NB];       // slot ids of the sample one / two ahead of the one whose first step has begun
    int off[NB];                // float4 words from `weight` to the rows of the sample that load() reads

    __device__ __forceinline__ void init(const float* feat, int F_, int D4_) {
        feat4 = reinterpret_cast<const v4f*>(feat);
        F = F_;
        D4 = D4_;
        row = threadIdx.x >> 3;
        word = threadIdx.x & 7;
    }
    __device__ __forceinline__ void init(const float* x, const IxGather& ga, int F_, int D4_) {
        init(x, F_, D4_);
        w4 = ga.weight;
        ldx4 = ga.ldx4;
        slots = ga.slots;
#pragma unroll
        for (int i = 0; i < NB; ++i) {
            const int t = min(max(row + 32 * i, 1), F - 1) - 1;
            srow[i] = t * ga.n;
            rbase[i] = (int)ga.tab[t].row_base * D4;
        }
    }
    __device__ __forceinline__ void fetch_ids(int64_t b) {
#pragma unroll
        for (int i = 0; i < NB; ++i) idb[i] = slots[srow[i] + b];
    }
    __device__ __forceinline__ void offsets(const int (&id)[NB]) {
#pragma unroll
        for (int i = 0; i < NB; ++i) off[i] = rbase[i] + id[i] * D4;
    }
    __device__ __forceinline__ void load(int64_t b, int s) {
        // every load is issued, from a clamped address inside the sample's block; what lies outside it becomes zeros
        const int c4 = 8 * s + word;
        const v4f z = {0.f, 0.f, 0.f, 0.f};
        if constexpr (G) {      // (off[] must be sample b's)
            const int c = min(c4, D4 - 1);
#pragma unroll
            for (int i = 0; i < NB; ++i) {
                const v4f* src = w4 + (uint32_t)off[i];
                if (i == 0) src = row == 0 ? feat4 + b * ldx4 : src;
                const v4f x = src[c];
                v[i] = row + 32 * i < F && c4 < D4 ? x : z;
            }
            return;
        }
        const v4f* src = feat4 + b * F * D4 + min(c4, D4 - 1);
#pragma unroll
        for (int i = 0; i < NB; ++i) {
            const v4f x = src[min(row + 32 * i, F - 1) * D4];
            v[i] = row + 32 * i < F && c4 < D4 ? x : z;
        }
    }
    // the first sample's slab 0.  G: its chain and the ids of the sample behind it, exposed once per workgroup
    __device__ __forceinline__ void prime(int64_t b, int64_t B) {
        if constexpr (G) {
            fetch_ids(b);
            offsets(idb);
        }
        load(b, 0);
        if constexpr (G) {
            if (b + gridDim.x < B) fetch_ids(b + gridDim.x);
        }
    }
    // top of step (b, s): the loads of the step behind it, (bn, sn) if there is one (`more`)
    __device__ __forceinline__ void ahead(int64_t b, int s, int64_t bn, int sn, bool more, int64_t B) {
        if constexpr (G) {
            if (s == 0) {
#pragma unroll
                for (int i = 0; i < NB; ++i) ida[i] = idb[i];
                const int64_t b2 = b + 2 * (int64_t)gridDim.x;
                if (b2 < B) fetch_ids(b2);      // (ids of samples past B are not loaded)
            }
            if (more && sn == 0) offsets(ida);
        }
        if (more) load(bn, sn);
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

// G = false: feat is the [B, F, D] block, ga is not read.  G (cdlrm_gather_interact_xwide_fwd): feat is x, the rows come through
// ga.  One body; the loader alone knows the difference.
template <int NB, bool G = false>
__global__ void __launch_bounds__(256, 2) k_interact_xwide_fwd(const float* __restrict__ feat, IxGather ga, int64_t B, int F, int D,
                                                               int itself, float* __restrict__ R, int64_t ld_r, int vec) {
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
    IxLoader<NB, G> ld;
    if constexpr (G) ld.init(feat, ga, F, D >> 2);
    else ld.init(feat, F, D >> 2);
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
    ld.prime(b, B);
    stage(smem, b, 0);
    __syncthreads();
    f32x16 a0, a1, a2;
    int s = 0, cur = 0;
    for (;;) {
        int64_t bn;
        int sn;
        const bool more = ix_next(b, s, NS, B, bn, sn);
        ld.ahead(b, s, bn, sn, more, B);
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
// G (cdlrm_gather_interact_xwide_bwd): as in the forward kernel; the rows are read again from the cache, so the launch goes in
// front of the batch's embedding update.
template <int NB, bool G = false>
__global__ void __launch_bounds__(256) k_interact_xwide_bwd(const float* __restrict__ feat, IxGather ga, const float* __restrict__ dR,
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
    IxLoader<NB, G> ld;
    if constexpr (G) ld.init(feat, ga, F, D >> 2);
    else ld.init(feat, F, D >> 2);
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
    ld.prime(b, B);
    ld.stage(smem);
    head(b);                // (its barrier also publishes the first slice)
    int s = 0, cur = 0;
    for (;;) {
        int64_t bn;
        int sn;
        const bool more = ix_next(b, s, NS, B, bn, sn);
        ld.ahead(b, s, bn, sn, more, B);
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
    if (p.nb == 3) return ia_launch<k_interact_xwide_fwd<3>>(p, stream, false, feat, IxGather{}, B, F, D, itself, R, ld_r, (int)p.vec_r);
    return ia_launch<k_interact_xwide_fwd<4>>(p, stream, false, feat, IxGather{}, B, F, D, itself, R, ld_r, (int)p.vec_r);
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
        return ia_launch<k_interact_xwide_bwd<3>>(p, stream, true, feat, IxGather{}, dR, ld_r, B, F, D, itself, x_act, dfeat, (int)p.vec_r, (int)p.vec_df);
    return ia_launch<k_interact_xwide_bwd<4>>(p, stream, true, feat, IxGather{}, dR, ld_r, B, F, D, itself, x_act, dfeat, (int)p.vec_r, (int)p.vec_df);
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

// ---- fused gather + interaction at 65 to 128 features (Criteo layout: one index per bag, so a bag's sum-pool is its cache row) ----
// cached EmbeddingBag forward (model_no_ddp.py:200-203) + interact_features "dot" (:272-293) in one launch, and the interaction
// backward reading the same rows again.  The float4 tiers only: whole-float4 R / dR rows, aligned dfeat.
// The plan of both launches and of the query: xwide_plan's answer for an aligned call (the loader's chain lives in registers, so
// there is no LDS beside it).  nb 0: no kernel -- F outside 65 .. 128, D not a multiple of 4 or above 512, a cache whose rows a
// 32-bit float4-word offset cannot name, or more LDS than a workgroup gets.
static IxPlan gather_xwide_plan(int op, int64_t B, const cdlrm_ctx* ctx) {
    const int F = ctx->T + 1, D = ctx->D;
    if (!(IX_SHAPE_OK(F, D) && ctx->total_rows * (D / 4) < INT32_MAX)) return IxPlan{};
    const IxPlan p = xwide_plan(op, B, F, D, 1, (IX_WIDTH(F, D, 1) + 3) & ~3, true, true);
    return p.lds <= 160 * 1024 ? p : IxPlan{};
}

#define IXG_SHAPE_MSG "unsupported shape (64 < T + 1 <= 128, D % 4 == 0, D <= 512, cache rows * D / 4 < 2^31)"

extern "C" int cdlrm_gather_interact_xwide_supported(cdlrm_ctx* ctx) {
    return ctx && gather_xwide_plan(CDLRM_IA_OP_FWD, 1, ctx).nb ? 1 : 0;
}

extern "C" int cdlrm_gather_interact_xwide_grid(cdlrm_ctx* ctx, int32_t op, int64_t B, int64_t* grid, int64_t* lds_bytes) {
    CDLRM_REQUIRE(ctx && grid && lds_bytes && (op == CDLRM_IA_OP_FWD || op == CDLRM_IA_OP_BWD) && B >= 0, "bad argument");
    const IxPlan p = gather_xwide_plan(op, B, ctx);
    CDLRM_REQUIRE(p.nb, IXG_SHAPE_MSG);
    *grid = p.grid;
    *lds_bytes = (int64_t)p.lds;
    return 0;
}

// what both entry points ask of the slots, the dense feature and the R / dR rows (the checks of cdlrm_gather_interact_fwd / _bwd)
static int gather_xwide_check(const cdlrm_ctx* ctx, const IxPlan& p, int64_t n, const float* x, int64_t ld_x, const float* r,
                              int64_t ld_r, int64_t B, int32_t itself) {
    CDLRM_REQUIRE(p.nb, IXG_SHAPE_MSG ": gather + interaction as two calls");
    CDLRM_REQUIRE(B >= 0 && n >= B && (int64_t)ctx->T * n < INT32_MAX && aligned16(x) && ld_x % 4 == 0 && ld_x >= ctx->D,
                  "slot pitch / dense-feature rows");
    const int width = IX_WIDTH(ctx->T + 1, ctx->D, itself);
    CDLRM_REQUIRE(ld_r % 4 == 0 && aligned16(r) && ld_r >= ((width + 3) & ~3), "whole-float4 rows of R / dR (ld_r)");
    return 0;
}

// one launch of the plan between a start and a stop event (either may be null)
template <auto Kernel, typename... Args>
static int ix_launch_between(const IxPlan& p, void* stream, hipEvent_t ev0, hipEvent_t ev1, Args... args) {
    const int rc = cdlrm_grant_dynamic_lds<Kernel>(p.lds);
    if (rc) return rc;
    hipExtLaunchKernelGGL(Kernel, dim3((unsigned)p.grid), dim3(256), p.lds, (hipStream_t)stream, ev0, ev1, 0, args...);
    return 0;
}

extern "C" int cdlrm_gather_interact_xwide_fwd(cdlrm_ctx* ctx, const int32_t* slots, int64_t n, const float* x, int64_t ld_x,
                                               int64_t B, int32_t itself, float* R, int64_t ld_r, void* stream) {
    CdlrmStopScope stop_scope;          // (first: every exit below flushes an attached completion event)
    CDLRM_CLEAR_STALE();
    CDLRM_REQUIRE(ctx && slots && x && R, "null argument");
    CDLRM_REQUIRE(ctx->weight, "cdlrm_ctx_bind_cache first");
    const IxPlan p = gather_xwide_plan(CDLRM_IA_OP_FWD, B, ctx);
    const int rc = gather_xwide_check(ctx, p, n, x, ld_x, R, ld_r, B, itself);
    if (rc) return rc;
    if (B == 0) return 0;       // (an armed event pair stays armed for the next launch that can carry it)
    // a timed pair (cdlrm_ctx_time_next_gather) and an attached completion event, as cdlrm_gather_interact_fwd carries them
    hipEvent_t ev0 = (hipEvent_t)ctx->ev_start, ev1 = (hipEvent_t)ctx->ev_stop;
    ctx->ev_start = ctx->ev_stop = nullptr;
    hipEvent_t se = cdlrm_take_stop_event((hipStream_t)stream);
    if (!ev1 && se) { ev1 = se; se = nullptr; }
    const IxGather ga{ctx->d_tab, reinterpret_cast<const v4f*>(ctx->weight), slots, (int)n, ld_x / 4};
    const int F = ctx->T + 1, D = ctx->D;
    const int rl = p.nb == 3 ? ix_launch_between<k_interact_xwide_fwd<3, true>>(p, stream, ev0, ev1, x, ga, B, F, D, itself, R, ld_r, 1)
                             : ix_launch_between<k_interact_xwide_fwd<4, true>>(p, stream, ev0, ev1, x, ga, B, F, D, itself, R, ld_r, 1);
    if (rl) return rl;
    if (se) CDLRM_HIP_CHECK(hipEventRecord(se, (hipStream_t)stream));
    CDLRM_LAUNCH_CHECK();
    return 0;
}

extern "C" int cdlrm_gather_interact_xwide_bwd(cdlrm_ctx* ctx, const int32_t* slots, int64_t n, const float* x, int64_t ld_x,
                                               const float* dR, int64_t ld_r, int64_t B, int32_t itself, int32_t x_act,
                                               float* dfeat, void* stream) {
    CdlrmStopScope stop_scope;          // (first: every exit below flushes an attached completion event)
    CDLRM_REQUIRE(ctx && slots && x && dR && dfeat, "null argument");
    CDLRM_REQUIRE(ctx->weight, "cdlrm_ctx_bind_cache first");
    const IxPlan p = gather_xwide_plan(CDLRM_IA_OP_BWD, B, ctx);
    const int rc = gather_xwide_check(ctx, p, n, x, ld_x, dR, ld_r, B, itself);
    if (rc) return rc;
    CDLRM_REQUIRE(aligned16(dfeat), "whole-float4 gradient rows (dfeat)");
    if (B == 0) return 0;
    const IxGather ga{ctx->d_tab, reinterpret_cast<const v4f*>(ctx->weight), slots, (int)n, ld_x / 4};
    const int F = ctx->T + 1, D = ctx->D;
    if (p.nb == 3)
        return ia_launch<k_interact_xwide_bwd<3, true>>(p, stream, true, x, ga, dR, ld_r, B, F, D, itself, x_act, dfeat, 1, 1);
    return ia_launch<k_interact_xwide_bwd<4, true>>(p, stream, true, x, ga, dR, ld_r, B, F, D, itself, x_act, dfeat, 1, 1);
}
