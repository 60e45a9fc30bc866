// Multi-hot bags pooled INSIDE the dot interaction (cdlrm_bag_interact_fwd / _bwd): the cached EmbeddingBag forward with
// offsets (model_no_ddp.py:200-203, mode "sum") + interact_features "dot" (:272-293) in one launch, and the interaction
// backward pooling the same bags again -- the [B, T, D] block between the two operators is never written or read back.
//
// Work split, LDS layout and MFMA order are those of the column-slab kernels of dense.hip (k_interact_fwd_s / k_interact_bwd_s,
// single slice): 256-lane workgroups, a wave per sample, striding; the sample's [F, D] block staged 32 columns at a time into the
// wave's own slice [32][36]; forward Z = P P^T as the tiles (0,0), (1,0), (1,1) on the 16x16x4 fp32 MFMA, backward
// dP[:, slab] = (G + G^T) P[:, slab] on the 32x32x2 one; output rows leave through a staging row as whole float4 words.  Same
// operands in the same lanes in the same order: bit-identical to cdlrm_embbag_fwd + cdlrm_interact_fwd / cdlrm_interact_bwd.
//
// What is new is the operand producer (BagPool).  Register i of a lane covers 16 bytes -- chunk c = lane % 8 of every slab -- of
// row lane / 8 + 8 i; row r >= 1 is the sum-pool of bag b of table r - 1, from +0 in lookup order, exactly k_embbag_fwd_bags'
// (embbag.hip).  That kernel pools a bag as a serial chain: one dependent load per lookup.  Here the lookups of a bag are
// independent loads: U of them per row, for RI rows and all NS slabs, are issued back to back -- RI * U * NS 16-byte loads in
// flight per lane --, the slot ids of the next U are requested right behind them, and the rows are added in order as they land.
// The rows of a wave have bags of different lengths: the trip count is the wave's longest, a lane past its bag's end loads the
// row of a clamped -- valid -- lookup and does not add it.  offsets -> slot ids -> rows is a dependent chain, so the chain is
// started early: the offsets of a sample are requested one sample ahead, and its first U slot ids and the first group of row
// loads are issued in FRONT of the current sample's MFMAs and land under them.  Row 0 is the dense feature: a "bag" of one
// row read from x (assigned, not added: its bits pass through).  Rows F .. 31 repeat row F - 1, as in the slab kernels.
// Only bags b < B are pooled: the scratch bag of squared-off inputs (n_bags == B + 1) and its padding lookups are never read.
#include "interact_lds.h"

typedef float v4f __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
static inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

struct BagSrc {
    const TableDesc* tab;       // row_base of every table's cache rows
    const v4f* weight;          // cache rows (and the auxiliary rows behind them), D4 float4 words each
    const int32_t* slots;       // [T, n] slot ids of the batch's lookups
    const int64_t* offsets;     // [T, ld_off]: bag b of table t is lookups offsets[t, b] .. offsets[t, b + 1] (the last one: .. n)
    int n, n_bags, ld_off;      // (T * n and T * ld_off < 2^31, checked by the host)
    int64_t ldx4;               // pitch of the dense-feature rows, float4 words
};

template <int D4, int RI, int U>
struct BagPool {
    static constexpr int NS = D4 / 8, CS = 8, NR = 4;
    static_assert(NR % RI == 0, "the lane's four rows are pooled RI at a time");
    BagSrc ga;
    const v4f* x4;              // the dense feature's rows
    int srow[NR], orow[NR];     // where the row's table starts in `slots` / `offsets`
    const v4f* wbase[NR];       // this lane's 16 bytes of slot 0 of the row's table
    bool dense;                 // register 0 of this lane is row 0
    int c0;
    int lo[NR], len[NR];        // first lookup and length of the bags pooled next
    int64_t oa[NR], ob[NR];     // the offsets of the sample after that, in flight
    int32_t sl[NR][U];          // slot ids of the group of lookups whose rows are loaded next

    __device__ __forceinline__ void init(const BagSrc& g, const float* x, int lane, int F) {
        ga = g;
        x4 = reinterpret_cast<const v4f*>(x);
        dense = lane < CS;
        c0 = lane % CS;
#pragma unroll
        for (int i = 0; i < NR; ++i) {
            const int row = (lane + 64 * i) / CS;
            const int t = max(min(row, F - 1) - 1, 0);
            srow[i] = t * ga.n;
            orow[i] = t * ga.ld_off;
            wbase[i] = ga.weight + (ga.tab[t].row_base * D4 + c0);
        }
    }
    __device__ __forceinline__ int lookup(int k) const { return min(max(k, 0), ga.n - 1); }    // clamped: always a valid lookup
    // offsets of sample bb's bags: requested a sample ahead of take()
    __device__ __forceinline__ void request(int64_t bb) {
#pragma unroll
        for (int i = 0; i < NR; ++i) {
            oa[i] = ga.offsets[orow[i] + bb];
            ob[i] = ga.offsets[orow[i] + min(bb + 1, (int64_t)ga.n_bags - 1)];
        }
    }
    __device__ __forceinline__ void take(int64_t bb) {
#pragma unroll
        for (int i = 0; i < NR; ++i) {
            lo[i] = (int)oa[i];
            len[i] = (bb + 1 < ga.n_bags ? (int)ob[i] : ga.n) - lo[i];
        }
        if (dense) { lo[0] = 0; len[0] = 1; }
    }
    // slot ids of the first U lookups of every row
    __device__ __forceinline__ void first() {
#pragma unroll
        for (int i = 0; i < NR; ++i)
#pragma unroll
            for (int u = 0; u < U; ++u) sl[i][u] = ga.slots[srow[i] + lookup(lo[i] + u)];
    }
    // rows of lookups k0 .. k0 + U - 1 of rows rg .. rg + RI - 1, all slabs; behind them the slot ids of the next U lookups
    __device__ __forceinline__ void issue(int64_t bb, int rg, int k0, v4f (&v)[RI][U][NS]) {
#pragma unroll
        for (int r = 0; r < RI; ++r) {
            const int i = rg + r;
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const v4f* p = wbase[i] + (int64_t)sl[i][u] * D4;
                if (i == 0 && dense) p = x4 + bb * ga.ldx4 + c0;
#pragma unroll
                for (int s = 0; s < NS; ++s) v[r][u][s] = p[s * CS];
            }
        }
#pragma unroll
        for (int r = 0; r < RI; ++r)
#pragma unroll
            for (int u = 0; u < U; ++u) sl[rg + r][u] = ga.slots[srow[rg + r] + lookup(lo[rg + r] + k0 + U + u)];
    }
    // ... added in lookup order; a lookup past the bag's end is not added
    __device__ __forceinline__ void fold(int rg, int k0, const v4f (&v)[RI][U][NS], v4f (&acc)[NS][NR]) const {
#pragma unroll
        for (int r = 0; r < RI; ++r) {
            const int i = rg + r;
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const bool live = k0 + u < len[i];
#pragma unroll
                for (int s = 0; s < NS; ++s) {
                    const v4f a = acc[s][i];
                    acc[s][i] = live ? ((i == 0 && dense) ? v[r][u][s] : a + v[r][u][s]) : a;
                }
            }
        }
    }
    // acc = the pooled rows of sample bb.  early: group 0 of rows 0 .. RI - 1 is in v0 already (issue(bb, 0, 0, v0))
    __device__ __forceinline__ void pool(int64_t bb, v4f (&acc)[NS][NR], bool early, v4f (&v0)[RI][U][NS]) {
#pragma unroll
        for (int rg = 0; rg < NR; rg += RI) {
#pragma unroll
            for (int r = 0; r < RI; ++r)
#pragma unroll
                for (int s = 0; s < NS; ++s) acc[s][rg + r] = v4f{0.f, 0.f, 0.f, 0.f};
            int k0 = 0;
            if (rg == 0 && early) {
                fold(0, 0, v0, acc);
                k0 = U;
            }
            for (;; k0 += U) {
                bool more = false;
#pragma unroll
                for (int r = 0; r < RI; ++r) more |= k0 < len[rg + r];
                if (__builtin_amdgcn_ballot_w64(more) == 0) break;      // the wave's longest bag of these rows is done
                issue(bb, rg, k0, v0);
                fold(rg, k0, v0, acc);
            }
        }
    }
};

// per instance: rows pooled at a time (RI * U * NS float4 loads in flight per lane; DESIGN.md 4.8 has the registers)
constexpr int bag_ri(int d4) { return d4 == 8 ? 4 : d4 == 16 ? 2 : 1; }
// ... and lookups per row: CDLRM_BAG_INTERACT_U, but for D = 256 (half of it: with more the kernels spill)
constexpr int bag_u(int d4) { return d4 == 64 ? CDLRM_BAG_INTERACT_U / 2 : CDLRM_BAG_INTERACT_U; }

template <int D4>
__global__ void __launch_bounds__(256) k_bag_interact_fwd(const float* __restrict__ x, BagSrc ga, int64_t B, int F, int itself,
                                                          float* __restrict__ R, int64_t ld_r) {
    constexpr int D = 4 * D4, NS = D4 / 8, CS = 8, DS = 32, PITCH = DS + 4, NR = 4, RI = bag_ri(D4), U = bag_u(D4);
    static_assert(32 * PITCH == ia_slab_slice(D4, NS), "the slice the kernel walks is the slice the launch is sized for");
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float* Ts = smem + wave * ia_fwd_s_floats(D4, NS, false);
    float* Os = Ts + ia_slab_slice(D4, NS);
    const int64_t nw = (int64_t)gridDim.x * 4;
    int64_t b = (int64_t)blockIdx.x * 4 + wave;
    if (b >= B) return;
    const int l16 = lane & 15, g4 = lane >> 4;
    const int off = itself ? 1 : 0;
    int doff[NR];
#pragma unroll
    for (int i = 0; i < NR; ++i) doff[i] = ((lane + 64 * i) / CS) * PITCH + 4 * (lane % CS);
    BagPool<D4, RI, U> P;
    P.init(ga, x, lane, F);
    v4f nxt[NS][NR];            // the pooled rows of the sample computed next
    v4f v0[RI][U][NS];          // rows in flight
    P.request(b);
    P.take(b);
    P.first();
    P.request(min(b + nw, B - 1));
    P.pool(b, nxt, false, v0);
    auto one = [&](int64_t b) __attribute__((always_inline)) {
        const bool more = b + nw < B;
        const int64_t bn = min(b + nw, B - 1);
        // the next sample's chain, in front of this sample's MFMAs: its offsets were requested a sample ago
        P.take(bn);
        P.request(min(bn + nw, B - 1));
        P.first();
        if (more) P.issue(bn, 0, 0, v0);
        __builtin_amdgcn_sched_barrier(0);
        v4f acc00 = {0.f, 0.f, 0.f, 0.f}, acc10 = acc00, acc11 = acc00;
        const float* tp = Ts + l16 * PITCH + 4 * g4;
#pragma unroll
        for (int s = 0; s < NS; ++s) {
#pragma unroll
            for (int i = 0; i < NR; ++i) *reinterpret_cast<v4f*>(Ts + doff[i]) = nxt[s][i];
            if (lane < CS) *reinterpret_cast<v4f*>(Os + s * DS + 4 * lane) = nxt[s][0];      // row 0: the dense part of the output
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll 2
            for (int g = 0; g < DS / 16; ++g) {
                const float4 a0 = *reinterpret_cast<const float4*>(tp + 16 * g);                  // rows 0..15
                const float4 a1 = *reinterpret_cast<const float4*>(tp + 16 * PITCH + 16 * g);     // rows 16..31
                acc00 = __builtin_amdgcn_mfma_f32_16x16x4f32(a0.x, a0.x, acc00, 0, 0, 0);
                acc10 = __builtin_amdgcn_mfma_f32_16x16x4f32(a1.x, a0.x, acc10, 0, 0, 0);
                acc11 = __builtin_amdgcn_mfma_f32_16x16x4f32(a1.x, a1.x, acc11, 0, 0, 0);
                acc00 = __builtin_amdgcn_mfma_f32_16x16x4f32(a0.y, a0.y, acc00, 0, 0, 0);
                acc10 = __builtin_amdgcn_mfma_f32_16x16x4f32(a1.y, a0.y, acc10, 0, 0, 0);
                acc11 = __builtin_amdgcn_mfma_f32_16x16x4f32(a1.y, a1.y, acc11, 0, 0, 0);
                acc00 = __builtin_amdgcn_mfma_f32_16x16x4f32(a0.z, a0.z, acc00, 0, 0, 0);
                acc10 = __builtin_amdgcn_mfma_f32_16x16x4f32(a1.z, a0.z, acc10, 0, 0, 0);
                acc11 = __builtin_amdgcn_mfma_f32_16x16x4f32(a1.z, a1.z, acc11, 0, 0, 0);
                acc00 = __builtin_amdgcn_mfma_f32_16x16x4f32(a0.w, a0.w, acc00, 0, 0, 0);
                acc10 = __builtin_amdgcn_mfma_f32_16x16x4f32(a1.w, a0.w, acc10, 0, 0, 0);
                acc11 = __builtin_amdgcn_mfma_f32_16x16x4f32(a1.w, a1.w, acc11, 0, 0, 0);
            }
            __builtin_amdgcn_sched_barrier(0);
        }
        float* out = R + b * ld_r;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            // accumulator register r of lane l: tile row 4 (l / 16) + r, tile column l % 16
            const int i0 = 4 * g4 + r, i1 = 16 + 4 * g4 + r;
            if (i0 < F && l16 < i0 + off) Os[D + pair_base(i0, itself) + l16] = acc00[r];
            if (i1 < F) Os[D + pair_base(i1, itself) + l16] = acc10[r];
            if (i1 < F && 16 + l16 < i1 + off) Os[D + pair_base(i1, itself) + 16 + l16] = acc11[r];
        }
        const int width = D + pair_base(F, itself);
        if (lane < 4) Os[width + lane] = 0.f;       // the row pitch's pad columns (ld_r >= width rounded up to 4)
        const int W4 = (width + 3) >> 2;
        constexpr int NST = (D4 + 132 + 63) / 64;   // covers F = 32 with `itself`; a compile-time count
#pragma unroll
        for (int k = 0; k < NST; ++k) {
            const int e = min(64 * k + lane, W4 - 1);
            *reinterpret_cast<v4f*>(out + 4 * e) = *reinterpret_cast<const v4f*>(Os + 4 * e);
        }
        __builtin_amdgcn_sched_barrier(0);
        if (more) P.pool(bn, nxt, true, v0);
    };
    for (; b < B; b += nw) one(b);
}

template <int D4>
__global__ void __launch_bounds__(256) k_bag_interact_bwd(const float* __restrict__ x, BagSrc ga, const float* __restrict__ dR,
                                                          int64_t ld_r, int64_t B, int F, int itself, int x_act,
                                                          float* __restrict__ dfeat) {
    constexpr int D = 4 * D4, NS = D4 / 8, CS = 8, DS = 32, PITCH = DS + 4, NR = 4, RI = bag_ri(D4), U = bag_u(D4);
    constexpr int GMAX = ia_grad_row(D4);       // dense part + up to 32*33/2 pair gradients
    constexpr int NG = (GMAX / 4 + 63) / 64;
    static_assert(32 * PITCH == ia_slab_slice(D4, NS), "the slice the kernel walks is the slice the launch is sized for");
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int lr = lane & 31, lk = lane >> 5;
    float* Ts = smem + wave * ia_bwd_s_floats(D4, NS);
    float* Gs = Ts + 32 * PITCH;
    float* Os = Gs + D;                         // [16][32] output staging: the pair part of the dR row, dead once S is built
    const int off = itself ? 1 : 0;
    const int npairs = pair_base(F, itself);
    const int G4 = (D + npairs + 3) / 4;        // float4 words of one dR row (the pad word lies inside the pitch)
    const int64_t nw = (int64_t)gridDim.x * 4;
    int64_t b = (int64_t)blockIdx.x * 4 + wave;
    if (b >= B) return;
    int doff[NR];
#pragma unroll
    for (int i = 0; i < NR; ++i) doff[i] = ((lane + 64 * i) / CS) * PITCH + 4 * (lane % CS);
    BagPool<D4, RI, U> P;
    P.init(ga, x, lane, F);
    v4f nxt[NS][NR], gn[NG];
    v4f v0[RI][U][NS];
    P.request(b);
#pragma unroll
    for (int i = 0; i < NG; ++i) gn[i] = reinterpret_cast<const v4f*>(dR + b * ld_r)[min(lane + 64 * i, G4 - 1)];
    P.take(b);
    P.first();
    P.request(min(b + nw, B - 1));
    P.pool(b, nxt, false, v0);
    auto one = [&](int64_t b) __attribute__((always_inline)) {
        const bool more = b + nw < B;
        const int64_t bn = min(b + nw, B - 1);
        P.take(bn);
        P.request(min(bn + nw, B - 1));
        P.first();
#pragma unroll
        for (int i = 0; i < NG; ++i) *reinterpret_cast<v4f*>(Gs + 4 * min(lane + 64 * i, GMAX / 4 - 1)) = gn[i];
#pragma unroll
        for (int i = 0; i < NG; ++i) gn[i] = reinterpret_cast<const v4f*>(dR + bn * ld_r)[min(lane + 64 * i, G4 - 1)];
        if (more) P.issue(bn, 0, 0, v0);
        __builtin_amdgcn_sched_barrier(0);
        // A fragments of S = G + G^T: lane holds S[lr][lk + 2m], m = 0..15
        float sreg[16];
#pragma unroll
        for (int m = 0; m < 16; ++m) {
            const int j = lk + 2 * m;
            float v = 0.f;
            if (lr < F && j < F) {
                if (j < lr + off) v += Gs[D + pair_base(lr, itself) + j];
                if (lr < j + off) v += Gs[D + pair_base(j, itself) + lr];
            }
            sreg[m] = v;
        }
        float* out = dfeat + b * F * D;
#pragma unroll
        for (int s = 0; s < NS; ++s) {
#pragma unroll
            for (int i = 0; i < NR; ++i) *reinterpret_cast<v4f*>(Ts + doff[i]) = nxt[s][i];
            __builtin_amdgcn_sched_barrier(0);
            const int n0 = s * DS;
            f32x16 acc;
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[r] = 0.f;
            const float* tp = Ts + lk * PITCH + lr;
#pragma unroll
            for (int m = 0; m < 16; ++m) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(sreg[m], tp[2 * m * PITCH], acc, 0, 0, 0);
            {   // row 0 (register 0 of the lanes lk = 0): the dense feature: + direct path, * act'(bottom-MLP output)
                float v = acc[0] + Gs[n0 + lr];
                const float y = Ts[lr];
                if (x_act == 1) v = y > 0.f ? v : 0.f;
                else if (x_act == 2) v = v * ((1.0f - y) * y);
                acc[0] = lk == 0 ? v : acc[0];
            }
#pragma unroll
            for (int h = 0; h < 2; ++h) {
#pragma unroll
                for (int rr = 0; rr < 8; ++rr)      // accumulator register 8h + rr: row 16h + (rr&3) + 8 (rr>>2) + 4 lk
                    Os[((rr & 3) + 8 * (rr >> 2) + 4 * lk) * 32 + lr] = acc[8 * h + rr];
                const int nvalid = min(F - 16 * h, 16) * 8;     // float4 words of valid rows (F > 16: >= 8)
#pragma unroll
                for (int k = 0; k < 2; ++k) {
                    const int idx = min(64 * k + lane, nvalid - 1);     // clamped: spare lanes repeat the last word
                    const int row = idx >> 3, c4 = idx & 7;
                    const v4f gv = *reinterpret_cast<const v4f*>(Os + row * 32 + 4 * c4);
                    *reinterpret_cast<v4f*>(out + (16 * h + row) * D + n0 + 4 * c4) = gv;
                }
            }
            __builtin_amdgcn_sched_barrier(0);
        }
        if (more) P.pool(bn, nxt, true, v0);
    };
    for (; b < B; b += nw) one(b);
}

// ---- host side ----------------------------------------------------------------------------------------------------------
// One workgroup per CU, as the fused one-index forward: a wave has the whole register file for the rows it keeps in flight.
static inline bool bag_interact_dim(int D) { return D == 32 || D == 64 || D == 128 || D == 256; }
static inline int64_t bag_interact_grid(int64_t B) { return cdiv(B, 4) < 256 ? cdiv(B, 4) : 256; }
static inline size_t bag_interact_lds(int op, int d4) {
    return (size_t)4 * (op ? ia_bwd_s_floats(d4, d4 / 8) : ia_fwd_s_floats(d4, d4 / 8, false)) * sizeof(float);
}

template <typename Fn>
static int bag_with_d4(int d4, Fn&& fn) {
    switch (d4) {
        case 8: return fn(std::integral_constant<int, 8>{});
        case 16: return fn(std::integral_constant<int, 16>{});
        case 32: return fn(std::integral_constant<int, 32>{});
        default: return fn(std::integral_constant<int, 64>{});
    }
}

extern "C" int cdlrm_bag_interact_supported(cdlrm_ctx* ctx) {
    return ctx && bag_interact_dim(ctx->D) && ctx->T + 1 > 16 && ctx->T + 1 <= 32 ? 1 : 0;
}

extern "C" int cdlrm_bag_interact_grid(int32_t op, int64_t B, int32_t D, int64_t* grid, int64_t* lds_bytes) {
    CDLRM_REQUIRE(grid && lds_bytes && (op == 0 || op == 1) && B >= 0, "bad argument");
    CDLRM_REQUIRE(bag_interact_dim(D), "unsupported D (32 / 64 / 128 / 256)");
    *grid = bag_interact_grid(B);
    *lds_bytes = (int64_t)bag_interact_lds(op, D / 4);
    return 0;
}

// what both entry points ask of the bags, the dense feature and the R / dR rows
static int bag_interact_check(cdlrm_ctx* ctx, const int32_t* slots, int64_t n, const int64_t* offsets, int64_t n_bags,
                              int64_t ld_off, const float* x, int64_t ld_x, const float* r, int64_t ld_r, int64_t B,
                              int32_t itself) {
    CDLRM_REQUIRE(ctx && slots && offsets && x && r, "null argument");
    CDLRM_REQUIRE(ctx->weight, "cdlrm_ctx_bind_cache first");
    const int D = ctx->D, T = ctx->T, F = T + 1;
    CDLRM_REQUIRE(bag_interact_dim(D), "unsupported D (32 / 64 / 128 / 256): pool and interact as two calls");
    CDLRM_REQUIRE(T + 1 > 16 && T + 1 <= 32, "unsupported T (16 < T + 1 <= 32): pool and interact as two calls");
    CDLRM_REQUIRE(B >= 0 && (n_bags == B || n_bags == B + 1), "n_bags is B, or B + 1 for squared-off bags");
    CDLRM_REQUIRE(n >= 1 && ld_off >= n_bags && (int64_t)T * n < INT32_MAX && (int64_t)T * ld_off < INT32_MAX,
                  "n lookups / offset pitch ld_off");
    CDLRM_REQUIRE(aligned16(x) && ld_x % 4 == 0 && ld_x >= D, "dense-feature rows x / ld_x");
    const int width = D + (itself ? F * (F + 1) / 2 : F * (F - 1) / 2);
    CDLRM_REQUIRE(ld_r % 4 == 0 && aligned16(r) && ld_r >= ((width + 3) & ~3), "whole-float4 rows of R / dR (ld_r)");
    return 0;
}

extern "C" int cdlrm_bag_interact_fwd(cdlrm_ctx* ctx, const int32_t* slots, int64_t n, const int64_t* offsets, int64_t n_bags,
                                      int64_t ld_off, const float* x, int64_t ld_x, int64_t B, int32_t itself, float* R,
                                      int64_t ld_r, void* stream) {
    CdlrmStopScope stop_scope;          // (first: every exit below flushes an attached completion event)
    CDLRM_CLEAR_STALE();
    const int rc = bag_interact_check(ctx, slots, n, offsets, n_bags, ld_off, x, ld_x, R, ld_r, B, itself);
    if (rc) return rc;
    if (B == 0) return 0;       // (an armed event pair stays armed for the next launch that can carry it)
    // a timed pair (cdlrm_ctx_time_next_gather) and an attached completion event, as cdlrm_gather_interact_fwd carries them
    hipEvent_t ev0 = (hipEvent_t)ctx->ev_start, ev1 = (hipEvent_t)ctx->ev_stop;
    ctx->ev_start = ctx->ev_stop = nullptr;
    hipEvent_t se = cdlrm_take_stop_event((hipStream_t)stream);
    if (!ev1 && se) { ev1 = se; se = nullptr; }
    const BagSrc ga{ctx->d_tab, reinterpret_cast<const v4f*>(ctx->weight), slots, offsets, (int)n, (int)n_bags, (int)ld_off, ld_x / 4};
    const int F = ctx->T + 1;
    const size_t lds = bag_interact_lds(0, ctx->D / 4);
    const int rl = bag_with_d4(ctx->D / 4, [&](auto d4) {
        constexpr auto kernel = k_bag_interact_fwd<decltype(d4)::value>;
        const int rg = cdlrm_grant_dynamic_lds<kernel>(lds);
        if (rg) return rg;
        hipExtLaunchKernelGGL(kernel, dim3((unsigned)bag_interact_grid(B)), dim3(256), lds, (hipStream_t)stream, ev0, ev1, 0, x, ga,
                              B, F, itself, R, ld_r);
        return 0;
    });
    if (rl) return rl;
    if (se) CDLRM_HIP_CHECK(hipEventRecord(se, (hipStream_t)stream));
    CDLRM_LAUNCH_CHECK();
    return 0;
}

extern "C" int cdlrm_bag_interact_bwd(cdlrm_ctx* ctx, const int32_t* slots, int64_t n, const int64_t* offsets, int64_t n_bags,
                                      int64_t ld_off, const float* x, int64_t ld_x, const float* dR, int64_t ld_r, int64_t B,
                                      int32_t itself, int32_t x_act, float* dfeat, void* stream) {
    CdlrmStopScope stop_scope;          // (first: every exit below flushes an attached completion event)
    const int rc = bag_interact_check(ctx, slots, n, offsets, n_bags, ld_off, x, ld_x, dR, ld_r, B, itself);
    if (rc) return rc;
    CDLRM_REQUIRE(dfeat && aligned16(dfeat), "whole-float4 gradient rows (dfeat)");
    if (B == 0) return 0;
    const BagSrc ga{ctx->d_tab, reinterpret_cast<const v4f*>(ctx->weight), slots, offsets, (int)n, (int)n_bags, (int)ld_off, ld_x / 4};
    const int F = ctx->T + 1;
    const size_t lds = bag_interact_lds(1, ctx->D / 4);
    return bag_with_d4(ctx->D / 4, [&](auto d4) {
        constexpr auto kernel = k_bag_interact_bwd<decltype(d4)::value>;
        const int rg = cdlrm_grant_dynamic_lds<kernel>(lds);
        if (rg) return rg;
        CDLRM_LAUNCH_EV(kernel, dim3((unsigned)bag_interact_grid(B)), dim3(256), lds, (hipStream_t)stream, x, ga, dR, ld_r, B, F,
                        itself, x_act, dfeat);
        CDLRM_LAUNCH_CHECK();
        return 0;
    });
}
