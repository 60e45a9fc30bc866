// The pairwise-dot interaction for 33 to 64 features (cdlrm_interact_wide_fwd / _bwd): interact_features "dot"
// (model_no_ddp.py:272-293) where one sample's Gram matrix no longer fits the single 32x32 tile of the kernels in dense.hip.
// Same operands and layouts as cdlrm_interact_fwd / _bwd: feat [B, F, D], R[b] = [feature 0 (D) | pairs at pair_base(i) + j | pad],
// dfeat [B, F, D] with the direct path and act'(feature 0) applied to row 0.
//
// Work split: 256-lane workgroups, a wave per sample, striding over the batch; every wave owns its LDS slice, so there is no
// workgroup barrier anywhere.  Two families:
//
//   pipelined (D in 32 / 64 / 128 / 256, whole-float4 R / dR rows, 16-byte aligned dfeat): the sample's 64-row block -- rows
//   F .. 63 repeat row F - 1, finite values whose products are never stored -- is staged 32 columns at a time into a [64][36]
//   slice.  Forward: the lower triangle of the 64x64 Gram matrix is the 32x32 blocks (0,0), (1,0), (1,1); three f32x16
//   accumulators on the 32x32x2 fp32 MFMA run on across the slabs, and one ds_read_b128 from row lane % 32 plus one from row
//   32 + lane % 32 feed four k-steps of all three blocks: two LDS reads per twelve MFMAs.  Backward: the A fragments of
//   S = G + G^T (64x64: 2 row blocks x 32 values per lane) are built once per sample from the staged dR row, and per slab
//   dT[:, slab] = S T[:, slab] is two f32x16 accumulators x 32 k-steps that share one B operand read.
//
//   The prefetch.  The narrow slab kernels keep the NEXT sample's whole block in registers (NS * NR float4 per lane); over 64
//   rows that is 256 registers at D = 256 and does not fit beside 48 accumulator registers (forward) or 96 of fragments and
//   accumulators (backward).  Here the loads run a FIXED distance ahead instead: a ring of RD slabs (8 float4 per lane each).
//   When slab s has been staged its ring slot is refilled with slab s + RD -- of this sample, or, behind the sample's last
//   slabs, slab s + RD - NS of the wave's next sample: the ring walks across the sample boundary and the register cost does not
//   depend on D.  NS is a multiple of RD, so a slab's slot is a compile-time number.
//
//   whole-row (any D % 4 == 0 that fits the LDS budget; unaligned R / dR / dfeat, a pitch without whole words): the [64][D + 1]
//   form of k_interact_fwd / k_interact_bwd, scalar LDS reads, outputs stored straight from the accumulator lanes.
//
// The pipelined pair also runs as the fused gather (cdlrm_gather_interact_wide_fwd / _bwd): the same kernels with
// the ring's source switched (IwRing<D4, G>), the rows read from the cache by slot id.
#include "interact_lds.h"

typedef float v4f __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef int v4i __attribute__((ext_vector_type(4)));
static inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

#define IW_PITCH 36         // floats per slice row: 32 columns + 4 (an odd multiple of 16 B: conflict-free b128 writes and reads)
#define IW_NR 8             // float4 per lane and slab: 64 rows x 8 words over 64 lanes

// accumulator register r of lane half lk: row of its 32x32 block
__device__ __forceinline__ int iw_acc_row(int r, int lk) { return (r & 3) + 8 * (r >> 2) + 4 * lk; }

// fn(integral_constant<int, S>) for S = 0 .. NS - 1, in order: the slab number is a compile-time value in the body
template <int... S, typename Fn>
__device__ __forceinline__ void iw_each_slab(std::integer_sequence<int, S...>, Fn&& fn) {
    (fn(std::integral_constant<int, S>{}), ...);
}

// G (the fused gather, cdlrm_gather_interact_wide_fwd / _bwd): row 0 of a sample's block is the dense feature
// x[b] (pitch ldx4 words), rows 1 .. F - 1 are the cache rows weight[tab[t].row_base + slots[t * n + b]], t = row - 1 -- the
// [B, T, D] block cdlrm_embbag_fwd would write and the kernels above read back never exists.  Same operands in the same lanes,
// same MFMA order: bit-identical to gather + interaction.
struct IwGather {
    const TableDesc* tab;       // row_base of every table's cache rows
    const v4f* weight;          // cache rows (and the auxiliary rows behind them), D4 float4 words each; fewer than 2^31 words
    const int32_t* slots;       // [T, n] slot ids of the batch (T * n < 2^31, checked by the host)
    int n;
    int64_t ldx4;               // pitch of the dense-feature rows, float4 words
};

// the register ring of both pipelined kernels: lane = (row lane / 8 + 8 i, word lane % 8) of a slab, i < 8
//
// G: soff[] holds, per register, the float4 words from `weight` to the row's start -- of ONE sample at a time.  The ring walks
// across the sample boundary, so the addresses of the wave's next sample must be in registers before this sample's last refills
// (NS <= RD: before its first), and slot id -> address -> row is a dependent chain of two memory round trips.  It is taken apart
// over three samples: lane r loads the slot id of row r (clamped to 1 .. F - 1) of the sample a whole sample before it is
// needed (fetch_ids, one register), turns it into a word offset and posts it into the wave's 64-word LDS table at the head of
// the next sample (post_ids), and behind the last refill that still needs the old addresses every lane takes the offsets of its
// eight rows out of the table with two ds_read_b128 (take_offsets; the table is ordered [lane / 8][i]) -- in front of a slab's
// MFMAs, which hide the LDS round trip.  No load ever waits for an address.  The table needs no second buffer (the register
// holds the sample in between) and no barrier (each wave owns its table; a wave's LDS operations complete in order).
template <int D4, bool G = false>
struct IwRing {
    static constexpr int NS = D4 / 8, RD = NS >= 2 ? 2 : 1;
    // G: at the head of the wave's k-th sample soff[] holds the offsets of sample k + LA - 1 and `sid` the slot ids of sample
    // k + LA.  NS > RD: the first NS - RD refills still read this sample, the offsets of the next are taken behind the last of
    // them.  NS <= RD: every refill reads the next sample, the offsets of the one after it are taken behind the last refill.
    static constexpr int LA = NS > RD ? 1 : 2, TAKE = NS > RD ? NS - RD - 1 : NS - 1;
    v4f v[RD][IW_NR];
    int soff[IW_NR];        // float4 words from the sample's start to this lane's word of slab 0; the row clamped to F - 1
    int doff;               // where register 0 goes in the slice; register i is 8 rows further down
    const v4f* feat4;       // G: word lane % 8 of x[0]
    int FD4;
    const v4f* w4;          // G: word lane % 8 of weight[0]
    int64_t ldx4;
    const int32_t* slots;
    int srow, rbase, sid;   // lane r: where its table's slot ids start, row_base * D4 of that table, the id in flight
    int* tpost;             // this lane's word of the table (row r at [r % 8][r / 8])
    const v4i* ttake;       // the eight offsets of rows lane / 8 + 8 i
    bool row0;              // register 0 of this lane is the dense feature

    __device__ __forceinline__ void init(const float* feat, int F, int lane) {
        feat4 = reinterpret_cast<const v4f*>(feat);
        FD4 = F * D4;
#pragma unroll
        for (int i = 0; i < IW_NR; ++i) soff[i] = min((lane >> 3) + 8 * i, F - 1) * D4 + (lane & 7);
        doff = (lane >> 3) * IW_PITCH + 4 * (lane & 7);
    }
    __device__ __forceinline__ void init(const float* x, const IwGather& ga, int F, int lane, float* table) {
        feat4 = reinterpret_cast<const v4f*>(x) + (lane & 7);
        w4 = ga.weight + (lane & 7);
        ldx4 = ga.ldx4;
        slots = ga.slots;
        const int t = min(max(lane, 1), F - 1) - 1;        // rows F .. 63 repeat row F - 1; row 0's word is never used
        srow = t * ga.n;
        rbase = (int)ga.tab[t].row_base * D4;
        tpost = reinterpret_cast<int*>(table) + (lane & 7) * 8 + (lane >> 3);
        ttake = reinterpret_cast<const v4i*>(table) + (lane >> 3) * 2;
        row0 = lane < 8;
        doff = (lane >> 3) * IW_PITCH + 4 * (lane & 7);
    }
    __device__ __forceinline__ void fetch_ids(int64_t b) { sid = slots[srow + b]; }
    __device__ __forceinline__ void post_ids() { *tpost = rbase + sid * D4; }
    __device__ __forceinline__ void take_offsets() {
        const v4i lo = ttake[0], hi = ttake[1];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            soff[i] = lo[i];
            soff[4 + i] = hi[i];
        }
    }
    template <int SLOT>
    __device__ __forceinline__ void load(int s, int64_t b) {
        if constexpr (G) {      // (soff[] must be sample b's)
#pragma unroll
            for (int i = 0; i < IW_NR; ++i) {
                const v4f* src = w4 + (uint32_t)soff[i];
                if (i == 0) src = row0 ? feat4 + b * ldx4 : src;
                v[SLOT][i] = src[s * 8];
            }
            return;
        }
        const v4f* src = feat4 + b * FD4 + s * 8;
#pragma unroll
        for (int i = 0; i < IW_NR; ++i) v[SLOT][i] = src[soff[i]];
    }
    // G: the first sample's addresses and rows, the chain exposed once; leaves the registers as the head of a sample finds them
    __device__ __forceinline__ void prime(int64_t b, int64_t nw, int64_t B) {
        fetch_ids(b);
        post_ids();
        take_offsets();
        load<0>(0, b);
        if constexpr (RD == 2) load<1>(1, b);
        if constexpr (LA == 2) {
            fetch_ids(min(b + nw, B - 1));
            post_ids();
            take_offsets();
        }
        fetch_ids(min(b + LA * nw, B - 1));
    }
    // G, at the head of sample b: the ids fetched a sample ago become offsets in the table, the ids of the sample after go out
    __device__ __forceinline__ void advance(int64_t b, int64_t nw, int64_t B) {
        post_ids();
        fetch_ids(min(b + (LA + 1) * nw, B - 1));
    }
    template <int SLOT>
    __device__ __forceinline__ void stage(float* __restrict__ Ts) const {
#pragma unroll
        for (int i = 0; i < IW_NR; ++i) *reinterpret_cast<v4f*>(Ts + doff + 8 * i * IW_PITCH) = v[SLOT][i];
    }
    // behind the staging of slab S of sample b: its slot takes slab S + RD, which lies in the next sample bn behind slab NS - RD
    template <int S>
    __device__ __forceinline__ void refill(int64_t b, int64_t bn) {
        if constexpr (S + RD < NS) load<S % RD>(S + RD, b);
        else load<S % RD>(S + RD - NS, bn);
        if constexpr (G && S == TAKE) take_offsets();       // (the refills behind slab TAKE read another sample than this one)
    }
};

// G = false: feat is the [B, F, D] block, ga is not read.  G (cdlrm_gather_interact_wide_fwd): feat is x, the rows come through
// ga.  One body; the ring alone knows the difference.
template <int D4, bool G = false>
__global__ void __launch_bounds__(256, 2) k_interact_wide_fwd(const float* __restrict__ feat, IwGather ga, int64_t B, int F,
                                                              int itself, float* __restrict__ R, int64_t ld_r) {
    using Ring = IwRing<D4, G>;
    constexpr int D = 4 * D4, NS = Ring::NS, RD = Ring::RD;
    constexpr int WF = iw_fwd_floats(D4) + (G ? iw_gather_table() : 0);
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float* Ts = smem + wave * WF;
    float* Os = Ts + iw_slab_slice();           // the output row [dense D | pairs | pad word]
    const int64_t nw = (int64_t)gridDim.x * 4;
    int64_t b = (int64_t)blockIdx.x * 4 + wave;
    if (b >= B) return;
    const int lr = lane & 31, lk = lane >> 5;
    const int off = itself ? 1 : 0;
    const int width = D + pair_base(F, itself), W4 = (width + 3) >> 2;
    Ring ring;
    if constexpr (G) {
        ring.init(feat, ga, F, lane, Ts + iw_fwd_floats(D4));
        ring.prime(b, nw, B);
    } else {
        ring.init(feat, F, lane);
        ring.template load<0>(0, b);
        if constexpr (RD == 2) ring.template load<1>(1, b);
    }
    const float* tp = Ts + lr * IW_PITCH + 4 * lk;      // lane half lk: contraction indices 8 g + 4 lk .. + 3 of a group
    auto slab = [&](auto s_, int64_t b, int64_t bn, f32x16& a00, f32x16& a10, f32x16& a11) __attribute__((always_inline)) {
        constexpr int S = decltype(s_)::value;
        ring.template stage<S % RD>(Ts);
        if (lane < 8) *reinterpret_cast<v4f*>(Os + S * 32 + 4 * lane) = ring.v[S % RD][0];       // row 0: the dense part of the output
        ring.template refill<S>(b, bn);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const v4f x0 = *reinterpret_cast<const v4f*>(tp + 8 * g);                       // rows 0..31
            const v4f x1 = *reinterpret_cast<const v4f*>(tp + 32 * IW_PITCH + 8 * g);       // rows 32..63
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                a00 = __builtin_amdgcn_mfma_f32_32x32x2f32(x0[c], x0[c], a00, 0, 0, 0);
                a10 = __builtin_amdgcn_mfma_f32_32x32x2f32(x1[c], x0[c], a10, 0, 0, 0);
                a11 = __builtin_amdgcn_mfma_f32_32x32x2f32(x1[c], x1[c], a11, 0, 0, 0);
            }
        }
        __builtin_amdgcn_sched_barrier(0);
    };
    // NK unconditional float4 stores of the staged row; lanes past its last word repeat that word
    auto store_row = [&](auto nk_, float* out) __attribute__((always_inline)) {
#pragma unroll
        for (int k = 0; k < decltype(nk_)::value; ++k) {
            const int e = min(64 * k + lane, W4 - 1);
            *reinterpret_cast<v4f*>(out + 4 * e) = *reinterpret_cast<const v4f*>(Os + 4 * e);
        }
    };
    auto one = [&](int64_t b) __attribute__((always_inline)) {
        const int64_t bn = min(b + nw, B - 1);
        if constexpr (G) ring.advance(b, nw, B);
        f32x16 a00, a10, a11;
#pragma unroll
        for (int r = 0; r < 16; ++r) a00[r] = a10[r] = a11[r] = 0.f;
        iw_each_slab(std::make_integer_sequence<int, NS>{}, [&](auto s_) __attribute__((always_inline)) { slab(s_, b, bn, a00, a10, a11); });
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int i0 = iw_acc_row(r, lk), i1 = 32 + i0;
            if (lr < i0 + off) Os[D + pair_base(i0, itself) + lr] = a00[r];
            if (i1 < F) {
                Os[D + pair_base(i1, itself) + lr] = a10[r];
                if (32 + lr < i1 + off) Os[D + pair_base(i1, itself) + 32 + lr] = a11[r];
            }
        }
        if (lane < 4) Os[width + lane] = 0.f;       // the row pitch's pad columns (ld_r >= width rounded up to 4)
        // a compile-time number of stores on either side of a wave-uniform branch: the waits in front of the next staging
        // still count loads, not store acknowledgements (see k_interact_fwd_s).  NLO covers F = 48 with `itself`.
        constexpr int NHI = (D4 + 521 + 63) / 64, NLO = (D4 + 295 + 63) / 64;
        float* out = R + b * ld_r;
        if (W4 <= 64 * NLO) store_row(std::integral_constant<int, NLO>{}, out);
        else store_row(std::integral_constant<int, NHI>{}, out);
        __builtin_amdgcn_sched_barrier(0);
    };
    one(b);                 // first sample peeled: see k_interact_fwd_s
    for (b += nw; b < B; b += nw) one(b);
}

// One wave per SIMD: beside 64 fragment and 32 accumulator registers the ring and the next sample's dR row (NG float4) do not fit
// a half register file -- bounded to two waves per SIMD every instance spills (124 to 632 bytes per lane).
// G (cdlrm_gather_interact_wide_bwd): as in the forward kernel; the rows are read again from the cache, so the launch goes in
// front of the batch's embedding update.
template <int D4, bool G = false>
__global__ void __launch_bounds__(256, 1) k_interact_wide_bwd(const float* __restrict__ feat, IwGather ga,
                                                        const float* __restrict__ dR, int64_t ld_r, int64_t B, int F,
                                                        int itself, int x_act, float* __restrict__ dfeat) {
    using Ring = IwRing<D4, G>;
    constexpr int D = 4 * D4, NS = Ring::NS, RD = Ring::RD;
    constexpr int GMAX = iw_grad_row(D4);       // dense part + up to 64 * 65 / 2 pair gradients
    constexpr int NG = (GMAX / 4 + 63) / 64;
    constexpr int WF = iw_bwd_floats(D4) + (G ? iw_gather_table() : 0);
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int lr = lane & 31, lk = lane >> 5;
    float* Ts = smem + wave * WF;
    float* Gs = Ts + iw_slab_slice();
    float* Os = Gs + D;                         // [16][32] output staging: the pair part of the dR row (>= 528 floats), dead once S is built
    const int npairs = pair_base(F, itself);
    const int G4 = (D + npairs + 3) / 4;        // float4 words of one dR row (the pad word lies inside the pitch)
    const int64_t nw = (int64_t)gridDim.x * 4;
    int64_t b = (int64_t)blockIdx.x * 4 + wave;
    if (b >= B) return;
    Ring ring;
    if constexpr (G) ring.init(feat, ga, F, lane, Ts + iw_bwd_floats(D4));
    else ring.init(feat, F, lane);
    v4f gn[NG];
#pragma unroll
    for (int i = 0; i < NG; ++i) gn[i] = reinterpret_cast<const v4f*>(dR + b * ld_r)[min(lane + 64 * i, G4 - 1)];
    if constexpr (G) {
        ring.prime(b, nw, B);
    } else {
        ring.template load<0>(0, b);
        if constexpr (RD == 2) ring.template load<1>(1, b);
    }
    const float* tp = Ts + lk * IW_PITCH + lr;
    auto slab = [&](auto s_, int64_t b, int64_t bn, const float (&sreg)[2][32]) __attribute__((always_inline)) {
        constexpr int S = decltype(s_)::value;
        ring.template stage<S % RD>(Ts);
        ring.template refill<S>(b, bn);
        __builtin_amdgcn_sched_barrier(0);
        f32x16 acc0, acc1;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc0[r] = acc1[r] = 0.f;
#pragma unroll
        for (int m = 0; m < 32; ++m) {          // k-step m: rows lk + 2 m of T, one read for both row blocks of S
            const float t = tp[2 * m * IW_PITCH];
            acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(sreg[0][m], t, acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(sreg[1][m], t, acc1, 0, 0, 0);
        }
        {   // row 0 (register 0 of the lanes lk = 0): the dense feature: + direct path, * act'(bottom-MLP output)
            float v = acc0[0] + Gs[S * 32 + lr];
            const float y = Ts[lr];
            if (x_act == 1) v = y > 0.f ? v : 0.f;
            else if (x_act == 2) v = v * ((1.0f - y) * y);
            acc0[0] = lk == 0 ? v : acc0[0];
        }
        float* out = dfeat + b * F * D + S * 32;
#pragma unroll
        for (int h = 0; h < 4; ++h) {           // 16 rows at a time through LDS, whole float4 words of rows < F only
            if (h == 3 && F <= 48) break;       // (wave-uniform)
#pragma unroll
            for (int rr = 0; rr < 8; ++rr) Os[iw_acc_row(rr, lk) * 32 + lr] = (h < 2 ? acc0 : acc1)[8 * (h & 1) + rr];
            const int nvalid = min(F - 16 * h, 16) * 8;
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                const int idx = min(64 * k + lane, nvalid - 1);     // clamped: spare lanes repeat the last word
                const int row = idx >> 3, c4 = idx & 7;
                *reinterpret_cast<v4f*>(out + (16 * h + row) * D + 4 * c4) = *reinterpret_cast<const v4f*>(Os + row * 32 + 4 * c4);
            }
        }
        __builtin_amdgcn_sched_barrier(0);
    };
    auto one = [&](int64_t b) __attribute__((always_inline)) {
        const int64_t bn = min(b + nw, B - 1);
        if constexpr (G) ring.advance(b, nw, B);
#pragma unroll
        for (int i = 0; i < NG; ++i) *reinterpret_cast<v4f*>(Gs + 4 * min(lane + 64 * i, GMAX / 4 - 1)) = gn[i];
#pragma unroll
        for (int i = 0; i < NG; ++i) gn[i] = reinterpret_cast<const v4f*>(dR + bn * ld_r)[min(lane + 64 * i, G4 - 1)];
        __builtin_amdgcn_sched_barrier(0);
        // A fragments of S = G + G^T: lane holds S[32 rb + lr][lk + 2 m].  Off the diagonal exactly one of G_ij, G_ji exists.
        float sreg[2][32];
#pragma unroll
        for (int rb = 0; rb < 2; ++rb) {
#pragma unroll
            for (int m = 0; m < 32; ++m) {
                const int i = 32 * rb + lr, j = lk + 2 * m;
                const int hi = max(i, j), lo = min(i, j);
                const bool valid = hi < F && (hi != lo || itself);
                float v = Gs[valid ? D + pair_base(hi, itself) + lo : 0];
                v = valid ? v : 0.f;
                sreg[rb][m] = hi == lo ? v + v : v;
            }
        }
        iw_each_slab(std::make_integer_sequence<int, NS>{}, [&](auto s_) __attribute__((always_inline)) { slab(s_, b, bn, sreg); });
    };
    one(b);                 // first sample peeled: see k_interact_fwd_s
    for (b += nw; b < B; b += nw) one(b);
}

// ---- the whole-row pair: any D, no alignment asked of R / dR / dfeat ----------------------------------------------------------
__global__ void __launch_bounds__(256) k_interact_wide_fwd_row(const float* __restrict__ feat, int64_t B, int F, int D, int itself,
                                                               float* __restrict__ R, int64_t ld_r) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int lr = lane & 31, lk = lane >> 5;
    const int ldt = D + 1, D4 = D >> 2;
    const int off = itself ? 1 : 0;
    float* Ts = smem + wave * iw_row_tile(D);
    for (int e = lane; e < iw_row_tile(D); e += 64) Ts[e] = 0.f;       // rows F..63 stay zero
    const int64_t nw = (int64_t)gridDim.x * 4;
    for (int64_t b = (int64_t)blockIdx.x * 4 + wave; b < B; b += nw) {
        const float4* src = reinterpret_cast<const float4*>(feat + b * F * D);
        for (int e = lane; e < F * D4; e += 64) {
            const float4 v = src[e];
            float* d = Ts + (e / D4) * ldt + (e % D4) * 4;
            d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
        }
        f32x16 a00, a10, a11;
#pragma unroll
        for (int r = 0; r < 16; ++r) a00[r] = a10[r] = a11[r] = 0.f;
        const float* tp = Ts + lr * ldt + lk;
        for (int k0 = 0; k0 < D; k0 += 2) {
            const float x0 = tp[k0], x1 = tp[32 * ldt + k0];
            a00 = __builtin_amdgcn_mfma_f32_32x32x2f32(x0, x0, a00, 0, 0, 0);
            a10 = __builtin_amdgcn_mfma_f32_32x32x2f32(x1, x0, a10, 0, 0, 0);
            a11 = __builtin_amdgcn_mfma_f32_32x32x2f32(x1, x1, a11, 0, 0, 0);
        }
        float* out = R + b * ld_r;
        for (int c = lane; c < D; c += 64) out[c] = Ts[c];
        float* pr = out + D;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int i0 = iw_acc_row(r, lk), i1 = 32 + i0;
            if (lr < i0 + off) pr[pair_base(i0, itself) + lr] = a00[r];
            if (i1 < F) {
                pr[pair_base(i1, itself) + lr] = a10[r];
                if (32 + lr < i1 + off) pr[pair_base(i1, itself) + 32 + lr] = a11[r];
            }
        }
    }
}

__global__ void __launch_bounds__(256) k_interact_wide_bwd_row(const float* __restrict__ feat, const float* __restrict__ dR,
                                                               int64_t ld_r, int64_t B, int F, int D, int itself, int x_act,
                                                               float* __restrict__ dfeat) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int lr = lane & 31, lk = lane >> 5;
    const int ldt = D + 1, D4 = D >> 2;
    const int npairs = pair_base(F, itself);
    float* Ts = smem + wave * iw_row_bwd_floats(D, npairs);
    float* Gs = Ts + iw_row_tile(D);
    for (int e = lane; e < iw_row_tile(D); e += 64) Ts[e] = 0.f;       // rows F..63 and the tail behind row 63 stay zero
    const int64_t nw = (int64_t)gridDim.x * 4;
    for (int64_t b = (int64_t)blockIdx.x * 4 + wave; b < B; b += nw) {
        const float4* src = reinterpret_cast<const float4*>(feat + b * F * D);
        for (int e = lane; e < F * D4; e += 64) {
            const float4 v = src[e];
            float* d = Ts + (e / D4) * ldt + (e % D4) * 4;
            d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
        }
        const float* gx = dR + b * ld_r;
        for (int e = lane; e < npairs; e += 64) Gs[e] = gx[D + e];
        float sreg[2][32];
#pragma unroll
        for (int rb = 0; rb < 2; ++rb) {
#pragma unroll
            for (int m = 0; m < 32; ++m) {
                const int i = 32 * rb + lr, j = lk + 2 * m;
                const int hi = max(i, j), lo = min(i, j);
                const bool valid = hi < F && (hi != lo || itself);
                float v = Gs[valid ? pair_base(hi, itself) + lo : 0];
                v = valid ? v : 0.f;
                sreg[rb][m] = hi == lo ? v + v : v;
            }
        }
        float* out = dfeat + b * F * D;
        for (int n0 = 0; n0 < D; n0 += 32) {
            f32x16 acc[2];
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[0][r] = acc[1][r] = 0.f;
            const float* tp = Ts + lk * ldt + n0 + lr;      // (columns >= D of the last block: the next row's, or the zero tail)
#pragma unroll
            for (int m = 0; m < 32; ++m) {
                const float t = tp[2 * m * ldt];
                acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(sreg[0][m], t, acc[0], 0, 0, 0);
                acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(sreg[1][m], t, acc[1], 0, 0, 0);
            }
            const int col = n0 + lr;
            if (col < D) {
#pragma unroll
                for (int rb = 0; rb < 2; ++rb) {
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int i = 32 * rb + iw_acc_row(r, lk);
                        if (i < F) {
                            float v = acc[rb][r];
                            if (i == 0) {       // the dense feature: + direct path, * act'(bottom-MLP output) if asked
                                v += gx[col];
                                const float y = Ts[col];
                                if (x_act == 1) v = y > 0.f ? v : 0.f;
                                else if (x_act == 2) v = v * ((1.0f - y) * y);
                            }
                            out[i * D + col] = v;
                        }
                    }
                }
            }
        }
    }
}

// ---- the host side: one plan, two entry points, one query ----------------------------------------------------------------------
struct IwPlan {
    int family;         // CDLRM_IA_WIDE_SLAB / CDLRM_IA_WIDE_ROW
    int d4, ns;
    int64_t grid;       // workgroups of 256 lanes: a wave per sample, striding
    size_t lds;         // dynamic LDS bytes of the launch
};

// aligned_r: R (forward) / dR (backward) is 16-byte aligned; aligned_dfeat: dfeat is
static IwPlan wide_plan(int op, int64_t B, int F, int D, int itself, int64_t ld_r, bool aligned_r, bool aligned_dfeat) {
    IwPlan p{};
    const int npairs = itself ? F * (F + 1) / 2 : F * (F - 1) / 2, width = D + npairs;
    const bool piped = D == 32 || D == 64 || D == 128 || D == 256;
    const bool vec = ld_r % 4 == 0 && aligned_r && ld_r >= ((width + 3) & ~3);       // whole-float4 rows of R / dR
    const bool fwd = op == CDLRM_IA_OP_FWD;
    int floats;         // per wave
    int64_t cap;        // workgroups (256 CUs)
    p.d4 = D / 4;
    if (piped && vec && (fwd || aligned_dfeat)) {
        // Forward: two workgroups per CU -- the slice is single-buffered, so the second wave of a SIMD is what issues MFMAs while
        // the first waits out its staging round trip (LDS: 2 x 74 KB at D = 256).  Backward: one, its kernels hold more than half
        // a register file.  Development key 4 (cdlrm_debug_set) overrides the forward's workgroups per CU.
        p.family = CDLRM_IA_WIDE_SLAB;
        p.ns = p.d4 / 8;
        floats = fwd ? iw_fwd_floats(p.d4) : iw_bwd_floats(p.d4);
        cap = 256 * (!fwd ? 1 : g_cdlrm_debug[4] > 0 ? g_cdlrm_debug[4] : 2);
    } else {
        p.family = CDLRM_IA_WIDE_ROW;
        floats = fwd ? iw_row_tile(D) : iw_row_bwd_floats(D, npairs);
        cap = 1024;
    }
    p.grid = cdiv(B, 4) < cap ? cdiv(B, 4) : cap;
    p.lds = (size_t)4 * floats * sizeof(float);
    return p;
}

#define IW_SHAPE_OK(F, D) ((F) > 32 && (F) <= 64 && (D) >= 4 && (D) % 4 == 0 && (D) <= 512)
#define IW_WIDTH(F, D, itself) ((D) + ((itself) ? (F) * ((F) + 1) / 2 : (F) * ((F) - 1) / 2))

extern "C" int cdlrm_interact_wide_fwd(const float* feat, int64_t B, int32_t F, int32_t D, int32_t itself, float* R,
                                       int64_t ld_r, void* stream) {
    CDLRM_REQUIRE(feat && R && B >= 0 && IW_SHAPE_OK(F, D), "unsupported shape (32<F<=64, D%4==0)");
    CDLRM_REQUIRE(aligned16(feat) && ld_r >= IW_WIDTH(F, D, itself), "alignment / ld_r");
    const IwPlan p = wide_plan(CDLRM_IA_OP_FWD, B, F, D, itself, ld_r, aligned16(R), false);
    CDLRM_REQUIRE(p.lds <= 160 * 1024, "LDS budget");
    if (B == 0) return 0;
    if (p.family == CDLRM_IA_WIDE_SLAB)
        return ia_with_d4(p.d4, [&](auto d4) {
            return ia_launch<k_interact_wide_fwd<decltype(d4)::value>>(p, stream, false, feat, IwGather{}, B, F, itself, R, ld_r);
        });
    return ia_launch<k_interact_wide_fwd_row>(p, stream, false, feat, B, F, D, itself, R, ld_r);
}

extern "C" int cdlrm_interact_wide_bwd(const float* feat, const float* dR, int64_t ld_r, int64_t B, int32_t F, int32_t D,
                                       int32_t itself, int32_t x_act, float* dfeat, void* stream) {
    CdlrmStopScope stop_scope;          // (first: every exit below flushes an attached completion event)
    CDLRM_REQUIRE(feat && dR && dfeat && B >= 0 && IW_SHAPE_OK(F, D), "unsupported shape (32<F<=64, D%4==0)");
    CDLRM_REQUIRE(aligned16(feat) && ld_r >= IW_WIDTH(F, D, itself), "alignment / ld_r");
    const IwPlan p = wide_plan(CDLRM_IA_OP_BWD, B, F, D, itself, ld_r, aligned16(dR), aligned16(dfeat));
    CDLRM_REQUIRE(p.lds <= 160 * 1024, "LDS budget");
    if (B == 0) return 0;
    if (p.family == CDLRM_IA_WIDE_SLAB)
        return ia_with_d4(p.d4, [&](auto d4) {
            return ia_launch<k_interact_wide_bwd<decltype(d4)::value>>(p, stream, true, feat, IwGather{}, dR, ld_r, B, F, itself, x_act, dfeat);
        });
    return ia_launch<k_interact_wide_bwd_row>(p, stream, true, feat, dR, ld_r, B, F, D, itself, x_act, dfeat);
}

extern "C" int cdlrm_interact_wide_route(int32_t op, int64_t B, int32_t F, int32_t D, int32_t itself, int64_t ld_r,
                                         int32_t aligned, struct cdlrm_interact_route* out) {
    CDLRM_REQUIRE(out && (op == CDLRM_IA_OP_FWD || op == CDLRM_IA_OP_BWD) && B >= 0, "bad argument");
    CDLRM_REQUIRE(IW_SHAPE_OK(F, D), "unsupported shape (32<F<=64, D%4==0)");
    CDLRM_REQUIRE(ld_r >= IW_WIDTH(F, D, itself), "alignment / ld_r");
    const IwPlan p = wide_plan(op, B, F, D, itself, ld_r, aligned & 1, aligned & 2);
    CDLRM_REQUIRE(p.lds <= 160 * 1024, "LDS budget");
    out->family = p.family; out->d4 = p.d4; out->ns = p.ns; out->reserved = 0;
    out->grid = p.grid; out->lds_bytes = (int64_t)p.lds;
    return 0;
}

// ---- fused gather + interaction at 33 to 64 features (Criteo layout: one index per bag, so a bag's sum-pool is its cache row) ----
// cached EmbeddingBag forward (model_no_ddp.py:200-203) + interact_features "dot" (:272-293) in one launch, and the interaction
// backward reading the same rows again.  The pipelined family only: D in 32 / 64 / 128 / 256, whole-float4 R / dR rows, aligned dfeat.
// The plan of both launches and of the query: wide_plan's grid for an aligned call, the offset table behind every wave's slice.
// family 0: no kernel -- F outside 33 .. 64, another D, or a cache whose rows a 32-bit float4-word offset cannot name.
static IwPlan gather_wide_plan(int op, int64_t B, const cdlrm_ctx* ctx) {
    const int F = ctx->T + 1, D = ctx->D;
    if (!(F > 32 && F <= 64 && (D == 32 || D == 64 || D == 128 || D == 256) && ctx->total_rows * (D / 4) < INT32_MAX)) return IwPlan{};
    IwPlan p = wide_plan(op, B, F, D, 1, (IW_WIDTH(F, D, 1) + 3) & ~3, true, true);     // (whole-float4 rows: the pipelined family)
    p.lds += (size_t)4 * iw_gather_table() * sizeof(float);
    return p;
}

extern "C" int cdlrm_gather_interact_wide_supported(cdlrm_ctx* ctx) {
    return ctx && gather_wide_plan(CDLRM_IA_OP_FWD, 1, ctx).family ? 1 : 0;
}

extern "C" int cdlrm_gather_interact_wide_grid(cdlrm_ctx* ctx, int32_t op, int64_t B, int64_t* grid, int64_t* lds_bytes) {
    CDLRM_REQUIRE(ctx && grid && lds_bytes && (op == CDLRM_IA_OP_FWD || op == CDLRM_IA_OP_BWD) && B >= 0, "bad argument");
    const IwPlan p = gather_wide_plan(op, B, ctx);
    CDLRM_REQUIRE(p.family, "unsupported shape (D in 32/64/128/256, 32 < T + 1 <= 64, cache rows * D / 4 < 2^31)");
    *grid = p.grid;
    *lds_bytes = (int64_t)p.lds;
    return 0;
}

// what both entry points ask of the slots, the dense feature and the R / dR rows (the checks of cdlrm_gather_interact_fwd / _bwd)
static int gather_wide_check(const cdlrm_ctx* ctx, const IwPlan& p, const int32_t* slots, int64_t n, const float* x, int64_t ld_x,
                             const float* r, int64_t ld_r, int64_t B, int32_t itself) {
    CDLRM_REQUIRE(p.family, "unsupported shape (D in 32/64/128/256, 32 < T + 1 <= 64, cache rows * D / 4 < 2^31): gather + interaction as two calls");
    CDLRM_REQUIRE(B >= 0 && n >= B && (int64_t)ctx->T * n < INT32_MAX && aligned16(x) && ld_x % 4 == 0 && ld_x >= ctx->D,
                  "slot pitch / dense-feature rows");
    const int width = IW_WIDTH(ctx->T + 1, ctx->D, itself);
    CDLRM_REQUIRE(ld_r % 4 == 0 && aligned16(r) && ld_r >= ((width + 3) & ~3), "whole-float4 rows of R / dR (ld_r)");
    return 0;
}

extern "C" int cdlrm_gather_interact_wide_fwd(cdlrm_ctx* ctx, const int32_t* slots, int64_t n, const float* x, int64_t ld_x,
                                              int64_t B, int32_t itself, float* R, int64_t ld_r, void* stream) {
    CdlrmStopScope stop_scope;          // (first: every exit below flushes an attached completion event)
    CDLRM_CLEAR_STALE();
    CDLRM_REQUIRE(ctx && slots && x && R, "null argument");
    CDLRM_REQUIRE(ctx->weight, "cdlrm_ctx_bind_cache first");
    const IwPlan p = gather_wide_plan(CDLRM_IA_OP_FWD, B, ctx);
    const int rc = gather_wide_check(ctx, p, slots, n, x, ld_x, R, ld_r, B, itself);
    if (rc) return rc;
    if (B == 0) return 0;       // (an armed event pair stays armed for the next launch that can carry it)
    // a timed pair (cdlrm_ctx_time_next_gather) and an attached completion event, as cdlrm_gather_interact_fwd carries them
    hipEvent_t ev0 = (hipEvent_t)ctx->ev_start, ev1 = (hipEvent_t)ctx->ev_stop;
    ctx->ev_start = ctx->ev_stop = nullptr;
    hipEvent_t se = cdlrm_take_stop_event((hipStream_t)stream);
    if (!ev1 && se) { ev1 = se; se = nullptr; }
    const IwGather ga{ctx->d_tab, reinterpret_cast<const v4f*>(ctx->weight), slots, (int)n, ld_x / 4};
    const int F = ctx->T + 1;
    const int rl = ia_with_d4(p.d4, [&](auto d4) {
        constexpr auto kernel = k_interact_wide_fwd<decltype(d4)::value, true>;
        const int rg = cdlrm_grant_dynamic_lds<kernel>(p.lds);
        if (rg) return rg;
        hipExtLaunchKernelGGL(kernel, dim3((unsigned)p.grid), dim3(256), p.lds, (hipStream_t)stream, ev0, ev1, 0, x, ga, B, F, itself,
                              R, ld_r);
        return 0;
    });
    if (rl) return rl;
    if (se) CDLRM_HIP_CHECK(hipEventRecord(se, (hipStream_t)stream));
    CDLRM_LAUNCH_CHECK();
    return 0;
}

extern "C" int cdlrm_gather_interact_wide_bwd(cdlrm_ctx* ctx, const int32_t* slots, int64_t n, const float* x, int64_t ld_x,
                                              const float* dR, int64_t ld_r, int64_t B, int32_t itself, int32_t x_act,
                                              float* dfeat, void* stream) {
    CdlrmStopScope stop_scope;          // (first: every exit below flushes an attached completion event)
    CDLRM_REQUIRE(ctx && slots && x && dR && dfeat, "null argument");
    CDLRM_REQUIRE(ctx->weight, "cdlrm_ctx_bind_cache first");
    const IwPlan p = gather_wide_plan(CDLRM_IA_OP_BWD, B, ctx);
    const int rc = gather_wide_check(ctx, p, slots, n, x, ld_x, dR, ld_r, B, itself);
    if (rc) return rc;
    CDLRM_REQUIRE(aligned16(dfeat), "whole-float4 gradient rows (dfeat)");
    if (B == 0) return 0;
    const IwGather ga{ctx->d_tab, reinterpret_cast<const v4f*>(ctx->weight), slots, (int)n, ld_x / 4};
    const int F = ctx->T + 1;
    return ia_with_d4(p.d4, [&](auto d4) {
        return ia_launch<k_interact_wide_bwd<decltype(d4)::value, true>>(p, stream, true, x, ga, dR, ld_r, B, F, itself, x_act, dfeat);
    });
}
