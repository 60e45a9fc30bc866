// The quotient-remainder compose INSIDE the dot interaction (cdlrm_qr_interact_fwd / _bwd): cdlrm_qr_cached_fwd
// (qr_cached.hip: E[b, t] = row(slot[t, b]) (*|+) Wr[t][r[t, b]]) + interact_features "dot" in one launch, and the interaction
// backward composing the same rows again -- the [B, T, D] block of composed rows between the two operators is never written
// or read back.  Both kernels are single-pass and read-only on the cache rows and on Wr.
//
// Work split, LDS layout and MFMA order are those of the column-slab kernels of dense.hip (k_interact_fwd_s / k_interact_bwd_s):
// 256-lane workgroups, a wave per sample, striding, one workgroup per CU; the sample's [F, D] block staged 32 columns at a time
// into the wave's slice(s) [32][36]; forward Z = P P^T as the tiles (0,0), (1,0), (1,1) on the 16x16x4 fp32 MFMA -- double-
// buffered slices with the fragment reads a group ahead wherever the plain fused forward is (qr_fwd_db) --, backward
// dP[:, slab] = (G + G^T) P[:, slab] on the 32x32x2 one; output rows leave through a staging row as whole float4 words.  The
// operands are the values qrc_compose makes (one fp32 operation per element), in the same lanes, in the same MFMA order:
// bit-identical to cdlrm_qr_cached_fwd + cdlrm_interact_fwd and to cdlrm_interact_bwd on that block.
//
// What is new is the operand producer (QrRows).  Register i of a lane covers 16 bytes -- chunk lane % 8 of every slab -- of row
// lane / 8 + 8 i.  Row 0 is the dense feature (assigned: its bits pass through), row t + 1 the cache row of slot[t, b] composed
// with Wr[t][min(r[t, b], c - 1)]; a plain table (collisions[t] == 0) passes its row through: its lanes load a valid Wr word
// and never use it.  Rows F .. 31 repeat row F - 1, compose included.
//   slot id + remainder -> row address + Wr address -> two loads  is a dependent chain: a sample's slot ids and remainder bytes
// are requested TWO samples ahead, its cache rows are loaded ONE sample ahead (all NS slabs: NS * NR float4 per lane), as in the
// plain fused kernels.  The Wr operand (T * c * D floats, L2-resident) is NOT held beside them: only the fragment of the slab
// staged next is live (NR float4), loaded when its predecessor has been consumed, and the compose happens at the staging write.
// The memory counter retires loads in order, so a Wr fragment is issued IN FRONT of the row loads of the same slot: waiting
// for it then waits for the rows issued a slab earlier, not for the ones issued with it.
#include "interact_lds.h"

typedef float v4f __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
static inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

#define QRI_MAX_C 16        // (QRC_MAX_C of qr_cached.hip)

struct QrSrc {
    const TableDesc* tab;       // row_base of every table's cache rows
    const v4f* weight;          // cache rows (and the auxiliary rows behind them), D4 float4 words each
    const int32_t* slots;       // [T, n] slot ids of the batch's lookups
    const uint8_t* rem;         // [T, ld_rem] remainders (cdlrm_qr_split)
    const v4f* Wr;              // [T, cmax, D4] remainder tables
    const int32_t* collisions;  // [T]; 0: a plain table
    int n, ld_rem, cmax, op;    // (T * n and T * ld_rem < 2^31, checked by the host); op 0: mult, else add
    int64_t ldx4;               // pitch of the dense-feature rows, float4 words
};

template <int D4>
struct QrRows {
    static constexpr int NS = D4 / 8, CS = 8, NR = 4;
    QrSrc ga;
    const v4f* x4;              // the dense feature's rows
    int srow[NR], rrow[NR];     // where the row's table starts in `slots` / `rem`
    const v4f* wbase[NR];       // this lane's 16 bytes of slot 0 of the row's table
    int wtab[NR];               // ... and of remainder 0 of the row's table, float4 words into Wr
    bool qr[NR];                // the row is composed (not the dense feature, not a plain table's)
    bool dense;                 // register 0 of this lane is row 0
    int c0;
    int32_t sl[NR];             // slot ids and remainders of the sample TWO ahead, in flight
    int rm[NR];
    const v4f* pn[NR];          // the sources of the sample whose rows are fetched next
    int wc[NR], wn[NR];         // Wr words of the sample being staged / of the next one

    __device__ __forceinline__ void init(const QrSrc& g, const float* x, int lane, int F) {
        ga = g;
        x4 = reinterpret_cast<const v4f*>(x);
        dense = lane < CS;
        c0 = lane % CS;
#pragma unroll
        for (int i = 0; i < NR; ++i) {
            const int row = (lane + 64 * i) / CS;
            const int t = max(min(row, F - 1) - 1, 0);
            srow[i] = t * ga.n;
            rrow[i] = t * ga.ld_rem;
            wbase[i] = ga.weight + (ga.tab[t].row_base * D4 + c0);
            wtab[i] = t * ga.cmax * D4 + c0;
            qr[i] = ga.collisions[t] > 0 && !(i == 0 && dense);
            wn[i] = wtab[i];
        }
    }
    __device__ __forceinline__ void request(int64_t bb) {
#pragma unroll
        for (int i = 0; i < NR; ++i) {
            sl[i] = ga.slots[srow[i] + bb];
            rm[i] = ga.rem[rrow[i] + bb];
        }
    }
    // sample bb (requested a sample ago) becomes the one fetched next; the one before it the one being staged
    __device__ __forceinline__ void point(int64_t bb) {
#pragma unroll
        for (int i = 0; i < NR; ++i) {
            wc[i] = wn[i];
            wn[i] = wtab[i] + min(rm[i], ga.cmax - 1) * D4;      // (never outside the remainder table)
            const v4f* p = wbase[i] + (int64_t)sl[i] * D4;
            if (i == 0 && dense) p = x4 + bb * ga.ldx4 + c0;
            pn[i] = p;
        }
    }
    __device__ __forceinline__ void rows(int s, v4f (&v)[NR]) const {
#pragma unroll
        for (int i = 0; i < NR; ++i) v[i] = pn[i][s * CS];
    }
    __device__ __forceinline__ void frag(const int (&w)[NR], int s, v4f (&y)[NR]) const {
#pragma unroll
        for (int i = 0; i < NR; ++i) y[i] = ga.Wr[w[i] + s * CS];
    }
    // the Wr fragment of slab s of the sample being staged; s >= NS: of slab s - NS of the sample behind it
    __device__ __forceinline__ void frag_ahead(int s, v4f (&y)[NR]) const {
        if (s < NS) frag(wc, s, y);
        else frag(wn, s - NS, y);
    }
    // qrc_compose (qr_cached.hip): one fp32 operation per element
    __device__ __forceinline__ v4f compose(int i, v4f v, v4f y) const {
        const v4f z = ga.op == 0 ? v * y : v + y;
        return qr[i] ? z : v;
    }
};

// the forward is double-buffered wherever the plain fused forward is (ia_gather_fwd_db of dense.hip): D >= 64
constexpr bool qr_fwd_db(int d4) { return d4 > 8; }

template <int D4>
__global__ void __launch_bounds__(256) k_qr_interact_fwd(const float* __restrict__ x, QrSrc ga, int64_t B, int F, int itself,
                                                         float* __restrict__ R, int64_t ld_r) {
    constexpr int D = 4 * D4, NS = D4 / 8, CS = 8, DS = 32, PITCH = DS + 4, NR = 4;
    constexpr bool DB = qr_fwd_db(D4);
    static_assert(32 * PITCH == ia_slab_slice(D4, NS), "the slice the kernel walks is the slice the launch is sized for");
    static_assert(!DB || NS % 2 == 0, "double buffering alternates two slices over an even number of slabs");
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float* Ts = smem + wave * ia_fwd_s_floats(D4, NS, DB);
    float* Os = Ts + ia_fwd_s_slices(D4, NS, DB);
    const int64_t nw = (int64_t)gridDim.x * 4;
    int64_t b = (int64_t)blockIdx.x * 4 + wave;
    if (b >= B) return;
    const int l16 = lane & 15, g4 = lane >> 4;
    const int off = itself ? 1 : 0;
    int doff[NR];
#pragma unroll
    for (int i = 0; i < NR; ++i) doff[i] = ((lane + 64 * i) / CS) * PITCH + 4 * (lane % CS);
    QrRows<D4> P;
    P.init(ga, x, lane, F);
    v4f nxt[NS][NR];            // the raw rows of the sample staged next
    v4f wr[NR];                 // the Wr fragment of the slab staged next
    P.request(b);
    P.point(b);
    P.frag(P.wn, 0, wr);
#pragma unroll
    for (int s = 0; s < NS; ++s) P.rows(s, nxt[s]);
    P.request(min(b + nw, B - 1));
    // accumulators -> staging row -> whole 16-byte words
    auto emit = [&](int64_t b, const v4f& acc00, const v4f& acc10, const v4f& acc11) __attribute__((always_inline)) {
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
    };
    if constexpr (DB) {
        // ---- double-buffered: slices T0 (even slabs) and T1 (odd slabs); slab s + 1 (the NEXT sample's slab 0 behind the last one)
        // is composed and staged into the other slice in the shadows of slab s's first MFMAs; behind it, one instruction group per
        // MFMA slot, the Wr fragment of the slab staged after that, the dense part of the output row and the row refill.
        float* const T0 = Ts;
        float* const T1 = Ts + 32 * PITCH;
        constexpr int NG = DS / 16;                 // 16-deep groups per slab
        static_assert(NG >= 2 && NR + 2 < 12 * (NG - 1), "the slab's side work ends before its last group reads the other slice");
#pragma unroll
        for (int i = 0; i < NR; ++i) *reinterpret_cast<v4f*>(T0 + doff[i]) = P.compose(i, nxt[0][i], wr[i]);   // the first sample's slab 0
        P.frag(P.wn, 1, wr);
        const int toff = l16 * PITCH + 4 * g4;
        float4 fa0 = *reinterpret_cast<const float4*>(T0 + toff);                              // fragments of (slab 0, group 0)
        float4 fa1 = *reinterpret_cast<const float4*>(T0 + toff + 16 * PITCH);
        auto one_db = [&](int64_t b) __attribute__((always_inline)) {
            const int64_t bn = min(b + nw, B - 1);
            P.point(bn);
            P.request(min(bn + nw, B - 1));
            P.rows(0, nxt[0]);                          // nxt[0] is free: this sample's slab 0 is staged
            if (lane < CS) *reinterpret_cast<v4f*>(Os + 4 * lane) = *reinterpret_cast<const v4f*>(T0 + 4 * lane);    // row 0 of slab 0
            v4f acc00 = {0.f, 0.f, 0.f, 0.f}, acc10 = acc00, acc11 = acc00;
            auto mf = [&](int j, const float4& a0, const float4& a1) __attribute__((always_inline)) {
                const int c = j / 3, w = j % 3;
                const float x0 = c == 0 ? a0.x : c == 1 ? a0.y : c == 2 ? a0.z : a0.w;
                const float x1 = c == 0 ? a1.x : c == 1 ? a1.y : c == 2 ? a1.z : a1.w;
                if (w == 0) acc00 = __builtin_amdgcn_mfma_f32_16x16x4f32(x0, x0, acc00, 0, 0, 0);
                else if (w == 1) acc10 = __builtin_amdgcn_mfma_f32_16x16x4f32(x1, x0, acc10, 0, 0, 0);
                else acc11 = __builtin_amdgcn_mfma_f32_16x16x4f32(x1, x1, acc11, 0, 0, 0);
            };
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                const float* cur = (s & 1) ? T1 : T0;
                float* oth = (s & 1) ? T0 : T1;
#pragma unroll
                for (int g = 0; g < NG; ++g) {
                    const float4 a0 = fa0, a1 = fa1;
                    const float* np_ = (g + 1 < NG) ? cur + toff + 16 * (g + 1) : oth + toff;
#pragma unroll
                    for (int j = 0; j < 12; ++j) {
                        mf(j, a0, a1);
                        const int k = g * 12 + j;           // slot inside the slab
                        if (k < NR) {
                            const int sn = s + 1 < NS ? s + 1 : 0;       // the slab being staged (the NEXT sample's slab 0 behind the last)
                            *reinterpret_cast<v4f*>(oth + doff[k]) = P.compose(k, nxt[sn][k], wr[k]);
                        }
                        if (k == NR) P.frag_ahead(s + 2, wr);           // in FRONT of the row refill (see the head of the file)
                        if (k == NR + 1 && s + 1 < NS && lane < CS) *reinterpret_cast<v4f*>(Os + (s + 1) * DS + 4 * lane) = nxt[s + 1][0];
                        if (k == NR + 2 && s + 1 < NS) P.rows(s + 1, nxt[s + 1]);
                        if (j == 0) {                       // the next group's fragments (last group: the next slab's first)
                            fa0 = *reinterpret_cast<const float4*>(np_);
                            fa1 = *reinterpret_cast<const float4*>(np_ + 16 * PITCH);
                        }
                        __builtin_amdgcn_sched_barrier(0);
                    }
                }
            }
            emit(b, acc00, acc10, acc11);
        };
        one_db(b);              // first sample peeled: see k_interact_fwd_s
        for (b += nw; b < B; b += nw) one_db(b);
        return;
    }
    auto one = [&](int64_t b) __attribute__((always_inline)) {
        const int64_t bn = min(b + nw, B - 1);
        P.point(bn);
        P.request(min(bn + nw, B - 1));
        v4f acc00 = {0.f, 0.f, 0.f, 0.f}, acc10 = acc00, acc11 = acc00;
        const float* tp = Ts + l16 * PITCH + 4 * g4;
#pragma unroll
        for (int s = 0; s < NS; ++s) {
#pragma unroll
            for (int i = 0; i < NR; ++i) *reinterpret_cast<v4f*>(Ts + doff[i]) = P.compose(i, nxt[s][i], wr[i]);
            if (lane < CS) *reinterpret_cast<v4f*>(Os + s * DS + 4 * lane) = nxt[s][0];      // row 0: the dense part of the output
            P.frag_ahead(s + 1, wr);
            P.rows(s, nxt[s]);
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
        emit(b, acc00, acc10, acc11);
    };
    one(b);
    for (b += nw; b < B; b += nw) one(b);
}

template <int D4>
__global__ void __launch_bounds__(256) k_qr_interact_bwd(const float* __restrict__ x, QrSrc ga, const float* __restrict__ dR,
                                                         int64_t ld_r, int64_t B, int F, int itself, int x_act,
                                                         float* __restrict__ dfeat) {
    constexpr int D = 4 * D4, NS = D4 / 8, CS = 8, DS = 32, PITCH = DS + 4, NR = 4;
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
    QrRows<D4> P;
    P.init(ga, x, lane, F);
    v4f nxt[NS][NR], wr[NR], gn[NG];
    P.request(b);
    P.point(b);
    P.frag(P.wn, 0, wr);
#pragma unroll
    for (int i = 0; i < NG; ++i) gn[i] = reinterpret_cast<const v4f*>(dR + b * ld_r)[min(lane + 64 * i, G4 - 1)];
#pragma unroll
    for (int s = 0; s < NS; ++s) P.rows(s, nxt[s]);
    P.request(min(b + nw, B - 1));
    auto one = [&](int64_t b) __attribute__((always_inline)) {
        const int64_t bn = min(b + nw, B - 1);
        P.point(bn);
        P.request(min(bn + nw, B - 1));
#pragma unroll
        for (int i = 0; i < NG; ++i) *reinterpret_cast<v4f*>(Gs + 4 * min(lane + 64 * i, GMAX / 4 - 1)) = gn[i];
#pragma unroll
        for (int i = 0; i < NG; ++i) gn[i] = reinterpret_cast<const v4f*>(dR + bn * ld_r)[min(lane + 64 * i, G4 - 1)];
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
            for (int i = 0; i < NR; ++i) *reinterpret_cast<v4f*>(Ts + doff[i]) = P.compose(i, nxt[s][i], wr[i]);
            P.frag_ahead(s + 1, wr);            // in FRONT of the row refill (see the head of the file)
            P.rows(s, nxt[s]);
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
    };
    one(b);                 // first sample peeled: see k_interact_fwd_s
    for (b += nw; b < B; b += nw) one(b);
}

// ---- host side ----------------------------------------------------------------------------------------------------------
// One workgroup per CU, forward and backward: a wave has the whole register file for the rows it keeps in flight.
static inline bool qr_interact_dim(int D) { return D == 32 || D == 64 || D == 128 || D == 256; }
static inline int64_t qr_interact_grid(int64_t B) { return cdiv(B, 4) < 256 ? cdiv(B, 4) : 256; }
static inline size_t qr_interact_lds(int op, int d4) {
    return (size_t)4 * (op ? ia_bwd_s_floats(d4, d4 / 8) : ia_fwd_s_floats(d4, d4 / 8, qr_fwd_db(d4))) * sizeof(float);
}

template <typename Fn>
static int qr_with_d4(int d4, Fn&& fn) {
    switch (d4) {
        case 8: return fn(std::integral_constant<int, 8>{});
        case 16: return fn(std::integral_constant<int, 16>{});
        case 32: return fn(std::integral_constant<int, 32>{});
        default: return fn(std::integral_constant<int, 64>{});
    }
}

extern "C" int cdlrm_qr_interact_supported(cdlrm_ctx* ctx) {
    return ctx && qr_interact_dim(ctx->D) && ctx->T + 1 > 16 && ctx->T + 1 <= 32 ? 1 : 0;
}

extern "C" int cdlrm_qr_interact_grid(int32_t op, int64_t B, int32_t D, int64_t* grid, int64_t* lds_bytes) {
    CDLRM_REQUIRE(grid && lds_bytes && (op == 0 || op == 1) && B >= 0, "bad argument");
    CDLRM_REQUIRE(qr_interact_dim(D), "unsupported D (32 / 64 / 128 / 256)");
    *grid = qr_interact_grid(B);
    *lds_bytes = (int64_t)qr_interact_lds(op, D / 4);
    return 0;
}

// what both entry points ask of the lookups, the remainder operands, the dense feature and the R / dR rows
static int qr_interact_check(cdlrm_ctx* ctx, const int32_t* slots, int64_t n, const uint8_t* r, int64_t ld_r, const float* Wr,
                             const int32_t* collisions, int32_t c, int32_t op, const float* x, int64_t ld_x, const float* R,
                             int64_t ld_R, int64_t B, int32_t itself) {
    CDLRM_REQUIRE(ctx && slots && x && R, "null argument");
    CDLRM_REQUIRE(r && Wr && collisions, "null r / Wr / collisions");
    CDLRM_REQUIRE(ctx->weight, "cdlrm_ctx_bind_cache first");
    const int D = ctx->D, T = ctx->T, F = T + 1;
    CDLRM_REQUIRE(qr_interact_dim(D), "unsupported D (32 / 64 / 128 / 256): compose and interact as two calls");
    CDLRM_REQUIRE(T + 1 > 16 && T + 1 <= 32, "unsupported T (16 < T + 1 <= 32): compose and interact as two calls");
    CDLRM_REQUIRE(B >= 0 && n == B, "n lookups per table: one per sample (n == B)");
    CDLRM_REQUIRE(c >= 2 && c <= QRI_MAX_C, "collisions c: 2 .. 16");
    CDLRM_REQUIRE(op == 0 || op == 1, "operation op: 0 = mult, 1 = add (concat changes the row width)");
    CDLRM_REQUIRE((int64_t)T * n < INT32_MAX, "T * n lookups beyond 2^31");
    CDLRM_REQUIRE(ld_r >= n && (int64_t)T * ld_r < INT32_MAX, "remainder pitch ld_r");
    CDLRM_REQUIRE(aligned16(Wr), "16-byte aligned remainder tables Wr");
    CDLRM_REQUIRE(aligned16(x) && ld_x % 4 == 0 && ld_x >= D, "dense-feature rows x / ld_x");
    const int width = D + (itself ? F * (F + 1) / 2 : F * (F - 1) / 2);
    CDLRM_REQUIRE(ld_R % 4 == 0 && aligned16(R) && ld_R >= ((width + 3) & ~3), "whole-float4 rows of R / dR (ld_R / ld_dR)");
    return 0;
}

static inline QrSrc qr_src(cdlrm_ctx* ctx, const int32_t* slots, int64_t n, const uint8_t* r, int64_t ld_r, const float* Wr,
                           const int32_t* collisions, int32_t c, int32_t op, int64_t ld_x) {
    return QrSrc{ctx->d_tab, reinterpret_cast<const v4f*>(ctx->weight), slots, r, reinterpret_cast<const v4f*>(Wr), collisions,
                 (int)n, (int)ld_r, (int)c, (int)op, ld_x / 4};
}

extern "C" int cdlrm_qr_interact_fwd(cdlrm_ctx* ctx, const int32_t* slots, int64_t n, const uint8_t* r, int64_t ld_r,
                                     const float* Wr, const int32_t* collisions, int32_t c, int32_t op, const float* x,
                                     int64_t ld_x, int64_t B, int32_t itself, float* R, int64_t ld_R, void* stream) {
    CdlrmStopScope stop_scope;          // (first: every exit below flushes an attached completion event)
    CDLRM_CLEAR_STALE();
    const int rc = qr_interact_check(ctx, slots, n, r, ld_r, Wr, collisions, c, op, x, ld_x, R, ld_R, B, itself);
    if (rc) return rc;
    if (B == 0) return 0;       // (an armed event pair stays armed for the next launch that can carry it)
    // a timed pair (cdlrm_ctx_time_next_gather) and an attached completion event, as cdlrm_gather_interact_fwd carries them
    hipEvent_t ev0 = (hipEvent_t)ctx->ev_start, ev1 = (hipEvent_t)ctx->ev_stop;
    ctx->ev_start = ctx->ev_stop = nullptr;
    hipEvent_t se = cdlrm_take_stop_event((hipStream_t)stream);
    if (!ev1 && se) { ev1 = se; se = nullptr; }
    const QrSrc ga = qr_src(ctx, slots, n, r, ld_r, Wr, collisions, c, op, ld_x);
    const int F = ctx->T + 1;
    const size_t lds = qr_interact_lds(0, ctx->D / 4);
    const int rl = qr_with_d4(ctx->D / 4, [&](auto d4) {
        constexpr auto kernel = k_qr_interact_fwd<decltype(d4)::value>;
        const int rg = cdlrm_grant_dynamic_lds<kernel>(lds);
        if (rg) return rg;
        hipExtLaunchKernelGGL(kernel, dim3((unsigned)qr_interact_grid(B)), dim3(256), lds, (hipStream_t)stream, ev0, ev1, 0, x, ga,
                              B, F, itself, R, ld_R);
        return 0;
    });
    if (rl) return rl;
    if (se) CDLRM_HIP_CHECK(hipEventRecord(se, (hipStream_t)stream));
    CDLRM_LAUNCH_CHECK();
    return 0;
}

extern "C" int cdlrm_qr_interact_bwd(cdlrm_ctx* ctx, const int32_t* slots, int64_t n, const uint8_t* r, int64_t ld_r,
                                     const float* Wr, const int32_t* collisions, int32_t c, int32_t op, const float* x,
                                     int64_t ld_x, const float* dR, int64_t ld_dR, int64_t B, int32_t itself, int32_t x_act,
                                     float* dfeat, void* stream) {
    CdlrmStopScope stop_scope;          // (first: every exit below flushes an attached completion event)
    const int rc = qr_interact_check(ctx, slots, n, r, ld_r, Wr, collisions, c, op, x, ld_x, dR, ld_dR, B, itself);
    if (rc) return rc;
    CDLRM_REQUIRE(dfeat && aligned16(dfeat), "whole-float4 gradient rows (dfeat)");
    if (B == 0) return 0;
    const QrSrc ga = qr_src(ctx, slots, n, r, ld_r, Wr, collisions, c, op, ld_x);
    const int F = ctx->T + 1;
    const size_t lds = qr_interact_lds(1, ctx->D / 4);
    return qr_with_d4(ctx->D / 4, [&](auto d4) {
        constexpr auto kernel = k_qr_interact_bwd<decltype(d4)::value>;
        const int rg = cdlrm_grant_dynamic_lds<kernel>(lds);
        if (rg) return rg;
        CDLRM_LAUNCH_EV(kernel, dim3((unsigned)qr_interact_grid(B)), dim3(256), lds, (hipStream_t)stream, x, ga, dR, ld_dR, B, F,
                        itself, x_act, dfeat);
        CDLRM_LAUNCH_CHECK();
        return 0;
    });
}
