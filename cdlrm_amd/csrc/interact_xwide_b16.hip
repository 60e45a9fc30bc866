// The pairwise-dot interaction for 65 to 128 features on the bf16 matrix pipe (cdlrm_interact_xwide_b16_fwd / _bwd, DESIGN.md
// 4.14): the operands, layouts, results, work split and grids of cdlrm_interact_xwide_fwd / _bwd (interact_xwide.hip, DESIGN.md
// 4.12), contracted on v_mfma_f32_32x32x16_bf16 instead of v_mfma_f32_32x32x2_f32.  PL = 1 ("bf16"): every operand element of
// the two contractions is rounded once to bf16.  PL = 2 ("bf16x3"): every element is split into two bf16 planes, x ~ h + l, and a
// product is al*bh + ah*bl + ah*bh -- the split and the order of gemm_bf16.h, near-fp32 error.  Accumulation is
// fp32; the dense part of R and the direct path of dfeat row 0 never touch bf16.
//
// Conversion happens once per element, on the way into LDS: the loader still brings fp32 float4 words into registers one step
// ahead of the MFMAs; the staging step writes PL bf16 images instead of an fp32 slice.
//
// Forward: an image is [FP][40] bf16, column-contiguous (the contraction runs over columns): a lane's float4 becomes one 8-byte
// write per plane, a fragment (row lr, columns 16 ks + 8 lk .. + 7) one ds_read_b128.  Wave w owns the blocks (w, w), (w + 1, w),
// (w + 2, w) modulo NB as in 4.12 and reads fragment 0 as the B operand of all of them; a slab is two 16-deep k-steps, a k-step
// that holds no column is skipped.
//
// Backward: dT[:, slab] = S T[:, slab] contracts over the FEATURE index, so the B fragment of a lane is 8 consecutive features of
// one column -- the transpose of how rows arrive.  The loader is dealt differently instead of transposing in LDS: a lane holds the
// same float4 word of FOUR CONSECUTIVE rows (rows 4 (tid / 8) .. + 3, word tid % 8: the global loads stay 128 contiguous bytes per
// 8 lanes), so each of its four columns is four consecutive features -- one 8-byte write per column and plane into the image
// [32 columns][FP + 8] bf16.  Per slab and lane: 4 PL ds_write_b64 (+ one b128 of the fp32 row 0 by 8 lanes) and, in the
// waves that own a row block, PL FP / 16 ds_read_b128 for FP / 16 (PL = 1) or 3 FP / 16 (PL = 2) MFMAs.  At NB = 3 the lanes of
// wave 3 hold rows >= 96: they load and stage nothing.  S = G + G^T is exact in fp32 (off the diagonal one of G_ij, G_ji exists,
// the diagonal is 2 G_ii) and is rounded / split once per sample into the A fragments, 8 consecutive k per lane and MFMA.
#include "b16.h"
#include "interact_lds.h"

typedef float v4f __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
static inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// accumulator register r of lane half lk: row of its 32x32 block
__device__ __forceinline__ int ixb_acc_row(int r, int lk) { return (r & 3) + 8 * (r >> 2) + 4 * lk; }

// A lane's share of one slab, zeros at rows >= F and columns >= D.  TR = false (forward): word tid % 8 of rows tid / 8 + 32 i,
// i < NB.  TR (backward): word tid % 8 of rows 4 (tid / 8) + i, i < 4; lanes whose rows lie at or past FP hold nothing.
template <int NB, bool TR>
struct IxbLoader {
    static constexpr int NV = TR ? 4 : NB;
    v4f v[NV];
    const v4f* feat4;
    int F, D4, rg, word;
    bool idle;

    __device__ __forceinline__ void init(const float* feat, int F_, int D4_) {
        feat4 = reinterpret_cast<const v4f*>(feat);
        F = F_;
        D4 = D4_;
        rg = threadIdx.x >> 3;
        word = threadIdx.x & 7;
        idle = TR && 4 * rg >= 32 * NB;         // (wave 3 at NB = 3: wave-uniform)
    }
    __device__ __forceinline__ int row(int i) const { return TR ? 4 * rg + i : rg + 32 * i; }
    __device__ __forceinline__ void load(int64_t b, int s) {
        if (idle) return;
        // every load is issued, from a clamped address inside the sample's block; what lies outside it becomes zeros
        const int c4 = 8 * s + word;
        const v4f z = {0.f, 0.f, 0.f, 0.f};
        const v4f* src = feat4 + b * F * D4 + min(c4, D4 - 1);
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const v4f x = src[min(row(i), F - 1) * D4];
            v[i] = row(i) < F && c4 < D4 ? x : z;
        }
    }
};

// the (sample, slab) behind (b, s) in a workgroup's walk; false behind its last one
__device__ __forceinline__ bool ixb_next(int64_t b, int s, int NS, int64_t B, int64_t& bn, int& sn) {
    sn = s + 1;
    bn = b;
    if (sn == NS) {
        sn = 0;
        bn = b + gridDim.x;
    }
    return bn < B;
}

// four consecutive contraction indices -> 8 bytes of the hi image at S (PL = 2: and of the lo image `plane` elements behind it)
template <int PL>
__device__ __forceinline__ void ixb_write4(unsigned short* __restrict__ S, int plane, float e0, float e1, float e2, float e3) {
    uint2 h;
    if constexpr (PL == 2) {
        uint2 l;
        b16_split(e0, e1, h.x, l.x);
        b16_split(e2, e3, h.y, l.y);
        *reinterpret_cast<uint2*>(S + plane) = l;
    } else {
        h.x = b16_pack(e0, e1);
        h.y = b16_pack(e2, e3);
    }
    *reinterpret_cast<uint2*>(S) = h;
}

// one 16-deep k-step of one accumulator.  PL = 2: lo*hi, hi*lo, then hi*hi, the small terms first; lo*lo is dropped
template <int PL>
__device__ __forceinline__ f32x16 ixb_mfma(const b16x8 (&a)[PL], const b16x8 (&b)[PL], f32x16 acc) {
    if constexpr (PL == 2) {
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[1], b[0], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[0], b[1], acc, 0, 0, 0);
    }
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[0], b[0], acc, 0, 0, 0);
}

template <int NB, int PL>
__global__ void __launch_bounds__(256, 2) k_interact_xwide_b16_fwd(const float* __restrict__ feat, int64_t B, int F, int D, int itself,
                                                                   float* __restrict__ R, int64_t ld_r, int vec) {
    constexpr int FP = 32 * NB, KP = IXB_FWD_PITCH, PLANE = FP * KP;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* Os = smem + 2 * ixb_fwd_slice(FP, PL);       // the pair row [pairs | pad words]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int lr = lane & 31, lk = lane >> 5;
    const int NS = (D + 31) >> 5;
    const int npairs = pair_base(F, itself), P4 = (npairs + 3) >> 2;
    int64_t b = blockIdx.x;
    if (b >= B) return;                                 // (the whole workgroup)
    // blocks (f[q], f[0]), q < nblk
    const int nblk = wave >= NB ? 0 : (NB == 4 && wave < 2 ? 3 : 2);
    int f[3];
#pragma unroll
    for (int q = 0; q < 3; ++q) f[q] = (wave + q) % NB;
    IxbLoader<NB, false> ld;
    ld.init(feat, F, D >> 2);
    // the staging of step (b, s) into a slice: the bf16 images; row 0 is the dense part of R[b] and leaves as it was loaded
    auto stage = [&](float* slice, int64_t b, int s) __attribute__((always_inline)) {
        unsigned short* S = reinterpret_cast<unsigned short*>(slice) + 4 * ld.word;
#pragma unroll
        for (int i = 0; i < NB; ++i) ixb_write4<PL>(S + ld.row(i) * KP, PLANE, ld.v[i][0], ld.v[i][1], ld.v[i][2], ld.v[i][3]);
        const int col = 32 * s + 4 * ld.word;
        if (ld.rg == 0 && col < D) {
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
        const bool more = ixb_next(b, s, NS, B, bn, sn);
        if (more) ld.load(bn, sn);
        __builtin_amdgcn_sched_barrier(0);
        if (s == 0) {
#pragma unroll
            for (int r = 0; r < 16; ++r) a0[r] = a1[r] = a2[r] = 0.f;
        }
        // lane half lk: contraction indices 16 ks + 8 lk .. + 7 of a k-step
        const unsigned short* tp = reinterpret_cast<const unsigned short*>(smem + cur * ixb_fwd_slice(FP, PL)) + lr * KP + 8 * lk;
        const int nk = min(2, (D - 32 * s + 15) >> 4);      // k-steps of 16 columns that hold any
        if (nblk) {
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                if (ks >= nk) break;
                b16x8 x0[PL], x1[PL], x2[PL];
#pragma unroll
                for (int p = 0; p < PL; ++p) {
                    x0[p] = __builtin_bit_cast(b16x8, *reinterpret_cast<const uint4*>(tp + p * PLANE + 32 * f[0] * KP + 16 * ks));
                    x1[p] = __builtin_bit_cast(b16x8, *reinterpret_cast<const uint4*>(tp + p * PLANE + 32 * f[1] * KP + 16 * ks));
                }
                if (nblk == 3) {
#pragma unroll
                    for (int p = 0; p < PL; ++p)
                        x2[p] = __builtin_bit_cast(b16x8, *reinterpret_cast<const uint4*>(tp + p * PLANE + 32 * f[2] * KP + 16 * ks));
                    a2 = ixb_mfma<PL>(x2, x0, a2);
                }
                a0 = ixb_mfma<PL>(x0, x0, a0);
                a1 = ixb_mfma<PL>(x1, x0, a1);
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
                        const int i = 32 * f[q] + ixb_acc_row(r, lk);
                        const int hi = max(i, j), lo = min(i, j);
                        // the diagonal block holds every pair twice: its lower triangle only
                        const bool ok = hi < F && (q ? true : i > j || (i == j && itself));
                        if (ok) Os[pair_base(hi, itself) + lo] = a[r];
                    }
                }
            }
        }
        if (more) stage(smem + (cur ^ 1) * ixb_fwd_slice(FP, PL), bn, sn);
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

// Registers: the A fragments of S are FP / 4 registers per plane where the fp32 kernel keeps FP / 2 words.  Bounded to two waves per
// SIMD the NB = 3 instances fit without scratch; the NB = 4 instances spill (112 bytes per lane at PL = 1, 216 at PL = 2), so they
// run unbounded like the fp32 kernel (DESIGN.md 4.14 has the table).  No instance uses scratch.
template <int NB, int PL>
__global__ void __launch_bounds__(256, NB == 3 ? 2 : 1) k_interact_xwide_b16_bwd(const float* __restrict__ feat, const float* __restrict__ dR,
                                                                   int64_t ld_r, int64_t B, int F, int D, int itself, int x_act,
                                                                   float* __restrict__ dfeat, int vec_r, int vec_df) {
    constexpr int FP = 32 * NB, KP = ixb_bwd_pitch(FP), PLANE = 32 * KP, NM = FP / 16;
    constexpr int NG = (512 + ix_pair_row(FP * (FP + 1) / 2) + 1023) / 1024;    // float4 per lane of the longest dR row
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int lr = lane & 31, lk = lane >> 5;
    const int NS = (D + 31) >> 5;
    const int npairs = pair_base(F, itself);
    const int G4 = (D + ix_pair_row(npairs)) >> 2;      // float4 words of one dR row (the pad words lie inside the pitch)
    float* Ys = smem + 2 * ixb_bwd_slice(FP, PL);       // row 0 of the two staged slabs, fp32
    float* Gs = Ys + 2 * ixb_row0();                    // the dR row [dense D | pairs | pad words]
    float* Os = Gs + D + ix_pair_row(npairs) + wave * ix_out_tile();
    const bool active = wave < NB;                      // owns row block `wave` of S
    int64_t b = blockIdx.x;
    if (b >= B) return;                                 // (the whole workgroup)
    IxbLoader<NB, true> ld;
    ld.init(feat, F, D >> 2);
    // the staging of a loaded slab into slice k: column 4 word + u of the lane's four rows is four consecutive features
    auto stage = [&](int k) __attribute__((always_inline)) {
        if (ld.idle) return;
        unsigned short* S = reinterpret_cast<unsigned short*>(smem + k * ixb_bwd_slice(FP, PL)) + 4 * ld.word * KP + 4 * ld.rg;
#pragma unroll
        for (int u = 0; u < 4; ++u) ixb_write4<PL>(S + u * KP, PLANE, ld.v[0][u], ld.v[1][u], ld.v[2][u], ld.v[3][u]);
        if (ld.rg == 0) *reinterpret_cast<v4f*>(Ys + k * ixb_row0() + 4 * ld.word) = ld.v[0];
    };
    v4f gn[NG];
    auto fetch_grad = [&](int64_t b) __attribute__((always_inline)) {
        if (!vec_r) return;
        const v4f* src = reinterpret_cast<const v4f*>(dR + b * ld_r);
#pragma unroll
        for (int i = 0; i < NG; ++i) gn[i] = src[min((int)threadIdx.x + 256 * i, G4 - 1)];      // (past the row: its last word again)
    };
    unsigned sa[PL][NM][4];
    // head of sample b: its dR row into LDS, the A fragments of S = G + G^T out of it (lane holds S[32 wave + lr][16 m + 8 lk + e],
    // e < 8, as four bf16 pairs per plane); off the diagonal exactly one of G_ij, G_ji exists
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
            // the row is made opaque per sample: otherwise the addresses and masks below, which depend on the lane alone, are
            // hoisted out of the sample loop and live in registers beside the fragments
            int i = 32 * wave + lr;
            asm volatile("" : "+v"(i));
#pragma unroll
            for (int m = 0; m < NM; ++m) {
                float sv[8];
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const int j = 16 * m + 8 * lk + e;
                    const int hi = max(i, j), lo = min(i, j);
                    const bool valid = hi < F && (hi != lo || itself);
                    float v = Gs[valid ? D + pair_base(hi, itself) + lo : 0];
                    v = valid ? v : 0.f;
                    sv[e] = hi == lo ? v + v : v;
                }
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    if constexpr (PL == 2) b16_split(sv[2 * e], sv[2 * e + 1], sa[0][m][e], sa[1][m][e]);
                    else sa[0][m][e] = b16_pack(sv[2 * e], sv[2 * e + 1]);
                }
                __builtin_amdgcn_sched_barrier(0);      // eight reads in flight: their addresses and masks die here
            }
        }
    };
    fetch_grad(b);
    ld.load(b, 0);
    stage(0);
    head(b);                // (its barrier also publishes the first slice)
    int s = 0, cur = 0;
    for (;;) {
        int64_t bn;
        int sn;
        const bool more = ixb_next(b, s, NS, B, bn, sn);
        if (more) ld.load(bn, sn);
        __builtin_amdgcn_sched_barrier(0);
        if (active) {
            // lane: column lr of the slab, features 16 m + 8 lk .. + 7 of k-step m
            const unsigned short* tp = reinterpret_cast<const unsigned short*>(smem + cur * ixb_bwd_slice(FP, PL)) + lr * KP + 8 * lk;
            f32x16 acc;
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
            for (int m = 0; m < NM; ++m) {
                b16x8 a[PL], t[PL];
#pragma unroll
                for (int p = 0; p < PL; ++p) {
                    a[p] = __builtin_bit_cast(b16x8, (uint4){sa[p][m][0], sa[p][m][1], sa[p][m][2], sa[p][m][3]});
                    t[p] = __builtin_bit_cast(b16x8, *reinterpret_cast<const uint4*>(tp + p * PLANE + 16 * m));
                }
                acc = ixb_mfma<PL>(a, t, acc);
            }
            if (wave == 0) {    // row 0 (register 0 of the lanes lk = 0): the dense feature: + direct path, * act'(bottom-MLP output)
                float v = acc[0] + Gs[32 * s + lr];
                const float y = Ys[cur * ixb_row0() + lr];
                if (x_act == 1) v = y > 0.f ? v : 0.f;
                else if (x_act == 2) v = v * ((1.0f - y) * y);
                acc[0] = lk == 0 ? v : acc[0];
            }
            float* out = dfeat + (b * F + 32 * wave) * D + 32 * s;
            if (vec_df) {
#pragma unroll
                for (int r = 0; r < 16; ++r) Os[ixb_acc_row(r, lk) * IX_PITCH + lr] = acc[r];
#pragma unroll
                for (int k = 0; k < 4; ++k) {       // whole float4 words of rows < F and columns < D only
                    const int row = 8 * k + (lane >> 3), c4 = lane & 7;
                    if (32 * wave + row < F && 32 * s + 4 * c4 < D)
                        *reinterpret_cast<v4f*>(out + (int64_t)row * D + 4 * c4) = *reinterpret_cast<const v4f*>(Os + row * IX_PITCH + 4 * c4);
                }
            } else if (32 * s + lr < D) {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int row = ixb_acc_row(r, lk);
                    if (32 * wave + row < F) out[(int64_t)row * D + lr] = acc[r];
                }
            }
        }
        __builtin_amdgcn_sched_barrier(0);
        if (more) stage(cur ^ 1);
        __syncthreads();
        if (!more) break;
        b = bn;
        s = sn;
        cur ^= 1;
        if (s == 0) head(b);
    }
}

// ---- the host side: one plan, two entry points, one query ----------------------------------------------------------------------
struct IxbPlan {
    int nb;             // 32-row blocks of the Gram matrix: 3 (F <= 96) or 4
    int ns;             // 32-column slabs of a sample
    bool vec_r;         // R / dR rows are whole aligned float4 words
    bool vec_df;        // dfeat is 16-byte aligned
    int64_t grid;       // workgroups of 256 lanes: a sample per workgroup, striding
    size_t lds;         // dynamic LDS bytes of the launch
};

// The whole LDS budget of both kernels; the tiers and grids of the fp32 pair (xwide_plan in interact_xwide.hip).
static IxbPlan xwide_b16_plan(int op, int64_t B, int F, int D, int itself, int planes, int64_t ld_r, bool aligned_r, bool aligned_dfeat) {
    IxbPlan p{};
    const int npairs = itself ? F * (F + 1) / 2 : F * (F - 1) / 2, width = D + npairs;
    p.nb = F <= 96 ? 3 : 4;
    p.ns = (D + 31) / 32;
    p.vec_r = ld_r % 4 == 0 && aligned_r && ld_r >= ((width + 3) & ~3);
    p.vec_df = aligned_dfeat;
    const int floats = op == CDLRM_IA_OP_FWD ? ixb_fwd_floats(32 * p.nb, planes, npairs) : ixb_bwd_floats(32 * p.nb, planes, D, npairs);
    p.lds = (size_t)floats * sizeof(float);
    const int64_t cap = op == CDLRM_IA_OP_FWD ? 512 : 256;
    p.grid = B < cap ? B : cap;
    return p;
}

#define IXB_SHAPE_OK(F, D) ((F) > 64 && (F) <= 128 && (D) >= 4 && (D) % 4 == 0 && (D) <= 512)
#define IXB_SHAPE_MSG "unsupported shape (64<F<=128, D%4==0, D<=512)"
#define IXB_PLANES_MSG "planes: 1 (bf16) or 2 (bf16x3)"
#define IXB_WIDTH(F, D, itself) ((D) + ((itself) ? (F) * ((F) + 1) / 2 : (F) * ((F) - 1) / 2))

template <int PL>
static int ixb_launch_fwd(const IxbPlan& p, void* stream, const float* feat, int64_t B, int F, int D, int itself, float* R, int64_t ld_r) {
    if (p.nb == 3) return ia_launch<k_interact_xwide_b16_fwd<3, PL>>(p, stream, false, feat, B, F, D, itself, R, ld_r, (int)p.vec_r);
    return ia_launch<k_interact_xwide_b16_fwd<4, PL>>(p, stream, false, feat, B, F, D, itself, R, ld_r, (int)p.vec_r);
}

template <int PL>
static int ixb_launch_bwd(const IxbPlan& p, void* stream, const float* feat, const float* dR, int64_t ld_r, int64_t B, int F, int D,
                          int itself, int x_act, float* dfeat) {
    if (p.nb == 3)
        return ia_launch<k_interact_xwide_b16_bwd<3, PL>>(p, stream, true, feat, dR, ld_r, B, F, D, itself, x_act, dfeat, (int)p.vec_r, (int)p.vec_df);
    return ia_launch<k_interact_xwide_b16_bwd<4, PL>>(p, stream, true, feat, dR, ld_r, B, F, D, itself, x_act, dfeat, (int)p.vec_r, (int)p.vec_df);
}

extern "C" int cdlrm_interact_xwide_b16_fwd(const float* feat, int64_t B, int32_t F, int32_t D, int32_t itself, int32_t planes,
                                            float* R, int64_t ld_r, void* stream) {
    CDLRM_REQUIRE(feat && R && B >= 0 && IXB_SHAPE_OK(F, D), IXB_SHAPE_MSG);
    CDLRM_REQUIRE(planes == 1 || planes == 2, IXB_PLANES_MSG);
    CDLRM_REQUIRE(aligned16(feat) && ld_r >= IXB_WIDTH(F, D, itself), "alignment / ld_r");
    const IxbPlan p = xwide_b16_plan(CDLRM_IA_OP_FWD, B, F, D, itself, planes, ld_r, aligned16(R), false);
    CDLRM_REQUIRE(p.lds <= 160 * 1024, "LDS budget");
    if (B == 0) return 0;
    return planes == 2 ? ixb_launch_fwd<2>(p, stream, feat, B, F, D, itself, R, ld_r) : ixb_launch_fwd<1>(p, stream, feat, B, F, D, itself, R, ld_r);
}

extern "C" int cdlrm_interact_xwide_b16_bwd(const float* feat, const float* dR, int64_t ld_r, int64_t B, int32_t F, int32_t D,
                                            int32_t itself, int32_t x_act, int32_t planes, float* dfeat, void* stream) {
    CdlrmStopScope stop_scope;          // (first: every exit below flushes an attached completion event)
    CDLRM_REQUIRE(feat && dR && dfeat && B >= 0 && IXB_SHAPE_OK(F, D), IXB_SHAPE_MSG);
    CDLRM_REQUIRE(planes == 1 || planes == 2, IXB_PLANES_MSG);
    CDLRM_REQUIRE(aligned16(feat) && ld_r >= IXB_WIDTH(F, D, itself), "alignment / ld_r");
    const IxbPlan p = xwide_b16_plan(CDLRM_IA_OP_BWD, B, F, D, itself, planes, ld_r, aligned16(dR), aligned16(dfeat));
    CDLRM_REQUIRE(p.lds <= 160 * 1024, "LDS budget");
    if (B == 0) return 0;
    return planes == 2 ? ixb_launch_bwd<2>(p, stream, feat, dR, ld_r, B, F, D, itself, x_act, dfeat)
                       : ixb_launch_bwd<1>(p, stream, feat, dR, ld_r, B, F, D, itself, x_act, dfeat);
}

extern "C" int cdlrm_interact_xwide_b16_route(int32_t op, int64_t B, int32_t F, int32_t D, int32_t itself, int32_t planes,
                                              int64_t ld_r, int32_t aligned, struct cdlrm_interact_route* out) {
    CDLRM_REQUIRE(out && (op == CDLRM_IA_OP_FWD || op == CDLRM_IA_OP_BWD) && B >= 0, "bad argument");
    CDLRM_REQUIRE(IXB_SHAPE_OK(F, D), IXB_SHAPE_MSG);
    CDLRM_REQUIRE(planes == 1 || planes == 2, IXB_PLANES_MSG);
    CDLRM_REQUIRE(ld_r >= IXB_WIDTH(F, D, itself), "alignment / ld_r");
    const IxbPlan p = xwide_b16_plan(op, B, F, D, itself, planes, ld_r, aligned & 1, aligned & 2);
    CDLRM_REQUIRE(p.lds <= 160 * 1024, "LDS budget");
    out->family = CDLRM_IA_XWIDE_B16; out->d4 = D / 4; out->ns = p.ns; out->reserved = 0;
    out->grid = p.grid; out->lds_bytes = (int64_t)p.lds;
    return 0;
}
