// K8: EmbeddingBag backward + sparse SGD on the cache rows, fused and atomics-free (gfx950).
// Reference: nn.EmbeddingBag(sparse=True) backward + optim.SGD step, main_no_ddp.py:376, 409, 413.
//
//   prepare (depends only on the slot ids, so it runs right after the probe, under the MLPs):
//     1. sort (slot, position) keys per table: LDS bitonic chunks (+ rank-merge passes when a table has
//        more than SORT_CHUNK lookups)
//     2. meta[p] = distance of sorted position p from the start of its run of equal slots
//   apply:
//     3. one LPR-lane group (16 B per lane) per sorted position; only chunk heads (meta % SEG_CH == 0) work:
//        they add <= SEG_CH gradient rows in position order; a run that fits one chunk updates its row at
//        once (W[slot] += -lr * sum), longer runs leave per-chunk partial sums
//     4. heads of long runs add their partials in chunk order and update the row.
// Repeated slots therefore accumulate in a fixed order: bitwise reproducible, no float atomics
// (cdna_hip_programming.md Guideline 12 / Appendix B "store pass + per-destination sum pass").
// HBM-bound: algorithmic bytes per lookup 4D (grad) + 2*4D (row read-modify-write) + 8.
#include "common.h"

#define SORT_CHUNK 8192          // most keys one workgroup sorts (64 KiB of LDS)
#define SORT_THREADS 1024
#define SEG_CH 32

__device__ __forceinline__ uint64_t shfl_xor_u64(uint64_t v, int lane_mask) {
    const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, lane_mask, 64);
    const uint32_t hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), lane_mask, 64);
    return ((uint64_t)hi << 32) | lo;
}

// Sort of one chunk of (slot, position) keys by ONE workgroup of 1024 threads, E keys per thread (chunk padded to
// 1024 * E with ~0 keys):
//   1. every wave sorts its 64 * E keys in REGISTERS -- a bitonic network whose exchanges at distance < E stay inside a
//      thread and at distance >= E are lane shuffles: no LDS, no barrier;
//   2. the 16 sorted runs meet in LDS and are merged pairwise by RANK: a key's place in the merged run is its place in
//      its own run plus the number of smaller keys in the sibling run (a binary search in LDS): log2(16) = 4 passes with
//      two barriers each.
// The all-LDS bitonic network this replaces took 91 compare-exchange stages with a 1024-thread barrier after each
// (91-113 us for 26 tables x 8192 lookups, profiles/r01_v7_c3_n1_kernel_stats.csv).
template <int E>
__global__ void __launch_bounds__(SORT_THREADS) k_sort_chunks(const int32_t* __restrict__ slots, int64_t n,
                                                              uint64_t* __restrict__ keys, int32_t* __restrict__ meta,
                                                              int npow2, int write_meta, int32_t* __restrict__ longcount,
                                                              uint8_t* __restrict__ once, int nb, int64_t ld_in,
                                                              int64_t batch_len, int nbt, int j0) {
    extern __shared__ __attribute__((aligned(16))) uint64_t sk[];
    __shared__ int wmax[16];
    const int t = blockIdx.y;
    // output list of input list t: a SLICE of a window chunk (nb of its nbt batches, from batch j0 on) lands in the chunk's
    // [T, nbt] lists; a batch's own sort and a whole chunk: ol == t
    const int ol = (t / nb) * nbt + j0 + t % nb;
    // the long-run list of THIS work buffer starts empty: cleared here, by the first kernel of every prepare (an apply always
    // follows a prepare on the same buffer, in stream order), so no clearing launch sits on the queue (a 4-byte hipMemsetAsync
    // is a 5.4 us kernel of its own) and two backward passes in flight on different work buffers share nothing
    if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) { longcount[0] = 0; longcount[2] = 0; }
    const int chunk = SORT_THREADS * E;       // == sort_chunk(n): whole chunks, a shorter last one
    const int64_t base = (int64_t)blockIdx.x * chunk;
    const int cnt = (int)min((int64_t)chunk, n - base);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    constexpr int WK = 64 * E;              // keys per wave
    constexpr int NT = SORT_THREADS * E;    // keys per workgroup (>= npow2)
    uint64_t k[E];
    int pos[E];
#pragma unroll
    for (int e = 0; e < E; ++e) {
        // coalesced load: element e of lane l is chunk index wave*WK + e*64 + l (which key a thread starts with is irrelevant)
        const int i = wave * WK + e * 64 + lane;
        k[e] = ~0ull;
        if (i < cnt) {
            const int64_t p = base + i;
            // (window form, cdlrm_embbag_bwd_prepare_window: list t = batch t % nb of table t / nb, read out of the resolver's
            //  [T, ld_in] slot ids; one batch: nb = 1, ld_in = n)
            k[e] = ((uint64_t)(uint32_t)slots[(int64_t)(t / nb) * ld_in + (int64_t)(t % nb) * batch_len + p] << 32) | (uint64_t)p;
        }
    }
    // 1. wave-local bitonic sort; the key with wave-local index g = lane * E + e lives in register e of lane `lane`
#pragma unroll
    for (int size = 2; size <= WK; size <<= 1) {
#pragma unroll
        for (int j = size >> 1; j >= 1; j >>= 1) {
            if (j >= E) {
                const int lm = j / E;
#pragma unroll
                for (int e = 0; e < E; ++e) {
                    const uint64_t o = shfl_xor_u64(k[e], lm);
                    const int g = lane * E + e;
                    const bool up = (g & size) == 0, lower = (g & j) == 0;
                    const uint64_t mn = k[e] < o ? k[e] : o, mx = k[e] < o ? o : k[e];
                    k[e] = (lower == up) ? mn : mx;
                }
            } else {
#pragma unroll
                for (int e = 0; e < E; ++e) {
                    const int p = e ^ j;
                    if (p > e) {
                        const int g = lane * E + e;
                        const bool up = (g & size) == 0;
                        const uint64_t a = k[e], b = k[p];
                        const bool sw = (a > b) == up;
                        k[e] = sw ? b : a;
                        k[p] = sw ? a : b;
                    }
                }
            }
        }
    }
#pragma unroll
    for (int e = 0; e < E; ++e) {
        pos[e] = wave * WK + lane * E + e;
        sk[pos[e]] = k[e];
    }
    __syncthreads();
    // 2. rank-merge the 16 runs pairwise; ties (only the ~0 pad keys repeat) go left run first.  Branch-free binary
    //    searches with a fixed step count, the E searches of a thread interleaved (E independent LDS reads in flight per
    //    step instead of one dependent read at a time)
    for (int run = WK; run < NT; run <<= 1) {
        int sib[E], cntl[E];
        bool left[E];
#pragma unroll
        for (int e = 0; e < E; ++e) {
            const int s0 = pos[e] & ~(2 * run - 1);
            left[e] = (pos[e] & run) == 0;
            sib[e] = left[e] ? s0 + run : s0;       // first key of the sibling run
            cntl[e] = 0;                            // sibling keys that sort in front of k[e], so far
        }
        for (int st = run >> 1; st > 0; st >>= 1) {
            uint64_t v[E];
#pragma unroll
            for (int e = 0; e < E; ++e) v[e] = sk[sib[e] + cntl[e] + st - 1];
#pragma unroll
            for (int e = 0; e < E; ++e) cntl[e] += (left[e] ? (v[e] < k[e]) : (v[e] <= k[e])) ? st : 0;
        }
        {
            uint64_t v[E];
#pragma unroll
            for (int e = 0; e < E; ++e) v[e] = sk[sib[e] + cntl[e]];        // cntl <= run - 1 here: in range
#pragma unroll
            for (int e = 0; e < E; ++e) cntl[e] += (left[e] ? (v[e] < k[e]) : (v[e] <= k[e])) ? 1 : 0;
        }
#pragma unroll
        for (int e = 0; e < E; ++e) {
            const int s0 = pos[e] & ~(2 * run - 1);
            pos[e] = s0 + (pos[e] - (left[e] ? s0 : s0 + run)) + cntl[e];
        }
        __syncthreads();                    // every search of this pass has read the old layout
#pragma unroll
        for (int e = 0; e < E; ++e) sk[pos[e]] = k[e];
        __syncthreads();
    }
    for (int i = threadIdx.x; i < cnt; i += blockDim.x) keys[(int64_t)ol * n + base + i] = sk[i];
    if (!write_meta) return;
    // run starts by an inclusive max-scan of head positions: thread owns E consecutive sorted keys
    const int i0 = threadIdx.x * E;
    int local = -1;     // last head position inside my range
    for (int e = 0; e < E; ++e) {
        const int i = i0 + e;
        if (i < cnt && (i == 0 || (uint32_t)(sk[i] >> 32) != (uint32_t)(sk[i - 1] >> 32))) local = i;
    }
    int inc = local;
    const int wid = wave;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int o = __shfl_up(inc, d, 64);
        if (lane >= d) inc = max(inc, o);
    }
    if (lane == 63) wmax[wid] = inc;
    __syncthreads();
    int pre = -1;       // max over all previous threads
    for (int w = 0; w < wid; ++w) pre = max(pre, wmax[w]);
    const int up = __shfl_up(inc, 1, 64);
    if (lane > 0) pre = max(pre, up);
    int run = pre;
    for (int e = 0; e < E; ++e) {
        const int i = i0 + e;
        if (i >= cnt) break;
        if (i == 0 || (uint32_t)(sk[i] >> 32) != (uint32_t)(sk[i - 1] >> 32)) run = i;
        meta[(int64_t)ol * n + base + i] = i - run;
        // a slot this batch reads ONCE (a run of one lookup), flagged at the lookup's position in the batch
        const bool last = i + 1 >= cnt || (uint32_t)(sk[i + 1] >> 32) != (uint32_t)(sk[i] >> 32);
        once[(int64_t)ol * n + (uint32_t)sk[i]] = (run == i && last) ? 1 : 0;
    }
}

// merge sorted runs of length `run` pairwise by ranking (keys are unique: position is part of the key)
__global__ void __launch_bounds__(256) k_merge_pass(const uint64_t* __restrict__ in, uint64_t* __restrict__ out,
                                                    int64_t n, int64_t run, int nb, int nbt, int j0) {
    const int t = blockIdx.y;
    const int ol = (t / nb) * nbt + j0 + t % nb;
    const uint64_t* a = in + (int64_t)ol * n;
    uint64_t* o = out + (int64_t)ol * n;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t pair = i / (2 * run);
        const int64_t s0 = pair * 2 * run;
        const int64_t s1 = min(s0 + run, n), s2 = min(s0 + 2 * run, n);
        const uint64_t key = a[i];
        int64_t pos;
        if (i < s1) pos = i + (lower_bound_u64(a, s1, s2, key) - s1);
        else pos = (i - s1) + lower_bound_u64(a, s0, s1, key);
        o[pos] = key;
    }
}

// meta for tables sorted in several chunks: distance to the run start by binary search
__global__ void __launch_bounds__(256) k_seg_meta(const uint64_t* __restrict__ keys, int64_t n, int32_t* __restrict__ meta,
                                                  uint8_t* __restrict__ once, int nb, int nbt, int j0) {
    // A tile of 256 consecutive sorted positions per pass: the run start of a position is the LAST run start at or in front of
    // it -- an inclusive max-scan inside the tile (wave shuffles + one LDS hop) -- and only the run that reaches into the tile
    // from the left needs a search over the keys, ONE per tile instead of one per position (round 6: a tiny table's run is
    // thousands of positions, each of which walked 13 dependent loads; 12-31 us beside the step for 2 x 26 lists).
    __shared__ int wlast[4];
    __shared__ int64_t left_start;
    const int t = blockIdx.y;
    const int ol = (t / nb) * nbt + j0 + t % nb;
    const uint64_t* kt = keys + (int64_t)ol * n;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int64_t p0 = (int64_t)blockIdx.x * 256; p0 < n; p0 += (int64_t)gridDim.x * 256) {
        const int64_t p = p0 + threadIdx.x;
        const bool in = p < n;
        const uint64_t key = in ? kt[p] : 0ull;
        const uint64_t s = key >> 32;
        const bool start = in && (p == 0 || (kt[p - 1] >> 32) != s);
        if (threadIdx.x == 0) left_start = -1;
        // last run start at or in front of this thread, inside the tile (-1: none)
        int v = start ? (int)threadIdx.x : -1;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int o = __shfl_up(v, d, 64);
            if (lane >= d) v = max(v, o);
        }
        if (lane == 63) wlast[wave] = v;
        __syncthreads();
        for (int w = 0; w < wave; ++w) v = max(v, wlast[w]);
        if (in && v < 0 && threadIdx.x == 0) left_start = lower_bound_u64(kt, 0, p0, s << 32);      // the run of the tile's first key
        __syncthreads();
        if (in) {
            const int64_t st = v >= 0 ? p0 + v : left_start;
            const int32_t r = (int32_t)(p - st);
            meta[(int64_t)ol * n + p] = r;
            // a slot this batch reads ONCE, flagged at the lookup's position in the batch (see k_sort_chunks)
            const bool last = p + 1 >= n || (kt[p + 1] >> 32) != s;
            once[(int64_t)ol * n + (uint32_t)key] = (r == 0 && last) ? 1 : 0;
        }
        __syncthreads();
    }
}

// ---------------------------------------------------------------------------------------------
// The row update: a compile-time policy (`Row`) of the three apply kernels k_bwd_chunks / k_bwd_blocks / k_bwd_long.  The kernels
// own the run search, the gradient-row sums (their loads in flight and their order of additions: the bit-exactness contract), the
// partial sums and the long-run list; a Row says what happens to the row of a run whose whole sum G one lane group holds:
//   SgdRow       W[slot] = fma(-lr, G, W[slot]), column chunk by column chunk: stored as soon as the chunk's sum is known, any D.
//   AdaRow       row-wise Adagrad (opt-in: cdlrm_embbag_bwd_apply_opt / _apply_sorted_opt, CDLRM_EMB_OPT_ROWWISE_ADAGRAD; DESIGN.md
//                4.5), per run of a CACHE-PROPER slot s of table t:
//                    i = tags[s];  S[i] += (1/D) sum_d G_d^2;  W[s] -= lr * G / (sqrt(S[i]) + eps)
//                S: one fp32 per TABLE row (state + state_base[t] + i), indexed by the tag of the slot, so it never moves with a
//                row.  A slot is one run and a run has one owning lane group: S[i] is read and written once per launch, without
//                atomics.  Aux slots (misses: transient copies, rewritten by the next forward) are skipped -- no row write, no state
//                update.  A lane keeps the NCH = ceil(D4 / LPR) column chunks it owns in registers until the row's sum of squares
//                is known (NCH > 1 only at LPR = 64, D > 256); the sum is reduced over the lane group by a fixed xor butterfly:
//                every lane ends with the same bits.
// (Only k_bwd_chunks takes both: k_bwd_blocks and k_bwd_long take AdaRow, and the SGD update has k_bwd_blocks_sgd and
//  k_bwd_long_sgd, texts of their own that held their measured speed where the shared bodies did not -- see there.)
// A kernel's use of a Row r, per run:  r.find, r.read_state;  per column chunk the lane owns (Row::for_chunks): r.load, the sum,
// r.chunk;  then r.finish and r.flag (the touched rule).
struct AdaArgs {
    const int64_t* tags;
    float* state;
    const int64_t* state_base;      // device [T]: first accumulator of table t
    float eps;
};

// what a row update sees of its table and its lane
struct RowCtx {
    const TableDesc* tab;
    int t, ways, D4, c;
    uint32_t aux0;                  // first aux slot
    // aux rows (transient copies of host rows, rewritten by every forward) are never flagged: the cross-rank row merge
    // leaves them alone, so it cannot collide with the NEXT batch's aux fill running ahead in the other aux region
    uint32_t first_aux;
    float lr;
    AdaArgs o;
};

template <int LPR_>
struct SgdRow {
    static constexpr int LPR = LPR_;
    static constexpr bool SGD = true;
    bool upd = false;               // this lane group updates the run's row (the run fits one chunk; k_bwd_long: always)
    float4 w;
    __device__ __forceinline__ void find(const RowCtx&, uint32_t, bool single) { upd = single; }
    __device__ __forceinline__ void read_state(const RowCtx&) {}
    template <class F>
    static __device__ __forceinline__ void for_chunks(int c, int D4, F f) {
        for (int cc = c; cc < D4; cc += LPR) f(0, cc);
    }
    __device__ __forceinline__ void load(int, const float4* wp) {
        if (upd) w = *wp;           // issued early, consumed after the sums
    }
    __device__ __forceinline__ void chunk(int, float4* wp, const float4& g, float lr) {
        if (upd) {
            w.x = fmaf(-lr, g.x, w.x); w.y = fmaf(-lr, g.y, w.y);
            w.z = fmaf(-lr, g.z, w.z); w.w = fmaf(-lr, g.w, w.w);
            *wp = w;
        }
    }
    __device__ __forceinline__ void finish(const RowCtx&, float4*) {}
    __device__ __forceinline__ bool flag(const RowCtx& x, uint32_t slot) const { return upd && slot < x.first_aux; }
};

// the accumulator cell of slot `slot` of table t; -1: an aux slot, or a tag that names no row of the table (an empty way: nothing
// the batch can have looked up) -- the run is then left alone
__device__ __forceinline__ int64_t ada_cell(const TableDesc* __restrict__ tab, int t, const AdaArgs& o, uint32_t slot,
                                            uint32_t aux0, int ways) {
    if (slot >= aux0) return -1;
    const uint32_t P = (uint32_t)tab[t].P;          // slot = P * way + set; tags are [P, ways]
    const uint32_t way = slot / P, set = slot - way * P;
    const int64_t i = o.tags[tab[t].tag_base + (int64_t)set * ways + way];
    return (uint64_t)i < (uint64_t)tab[t].n_rows ? o.state_base[t] + i : -1;
}

// S_new and the rows' step from the run sums g (zero in chunks past D4) -- called by ALL lanes of the group
template <int LPR, int NCH>
__device__ __forceinline__ float ada_step(float4 (&w)[NCH], const float4 (&g)[NCH], float s_old, float lr, float eps, int D4) {
    float ss = 0.f;
#pragma unroll
    for (int k = 0; k < NCH; ++k) {
        ss = fmaf(g[k].x, g[k].x, ss); ss = fmaf(g[k].y, g[k].y, ss);
        ss = fmaf(g[k].z, g[k].z, ss); ss = fmaf(g[k].w, g[k].w, ss);
    }
#pragma unroll
    for (int m = LPR >> 1; m >= 1; m >>= 1) ss += __shfl_xor(ss, m, 64);
    const float s_new = s_old + ss / (float)(4 * D4);
    const float scale = lr / (sqrtf(s_new) + eps);
#pragma unroll
    for (int k = 0; k < NCH; ++k) {
        w[k].x = fmaf(-scale, g[k].x, w[k].x); w[k].y = fmaf(-scale, g[k].y, w[k].y);
        w[k].z = fmaf(-scale, g[k].z, w[k].z); w[k].w = fmaf(-scale, g[k].w, w[k].w);
    }
    return s_new;
}

template <int LPR_, int NCH>
struct AdaRow {
    static constexpr int LPR = LPR_;
    static constexpr bool SGD = false;
    bool upd = false;               // a cache-proper slot with a valid tag whose run fits one chunk (uniform over the lane group)
    int64_t cell = -1;
    float s_old = 0.f;
    float4 w[NCH], g[NCH];
    // tag -> accumulator -> row: issued early, consumed after the sums
    __device__ __forceinline__ void find(const RowCtx& x, uint32_t slot, bool single) {
        cell = single ? ada_cell(x.tab, x.t, x.o, slot, x.aux0, x.ways) : -1;
        upd = cell >= 0;
#pragma unroll
        for (int k = 0; k < NCH; ++k) w[k] = g[k] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    __device__ __forceinline__ void read_state(const RowCtx& x) { s_old = upd ? x.o.state[cell] : 0.f; }
    template <class F>
    static __device__ __forceinline__ void for_chunks(int c, int D4, F f) {
#pragma unroll
        for (int k = 0; k < NCH; ++k)
            if (c + k * LPR < D4) f(k, c + k * LPR);
    }
    __device__ __forceinline__ void load(int k, const float4* wp) {
        if (upd) w[k] = *wp;
    }
    __device__ __forceinline__ void chunk(int k, float4*, const float4& sum, float) { g[k] = sum; }
    __device__ __forceinline__ void finish(const RowCtx& x, float4* wrow) {
        if (!upd) return;
        const float s_new = ada_step<LPR, NCH>(w, g, s_old, x.lr, x.o.eps, x.D4);
#pragma unroll
        for (int k = 0; k < NCH; ++k)
            if (x.c + k * LPR < x.D4) wrow[x.c + k * LPR] = w[k];
        if (x.c == 0) x.o.state[cell] = s_new;
    }
    __device__ __forceinline__ bool flag(const RowCtx&, uint32_t) const { return upd; }
};

// ---- the pieces the apply kernels are made of ----------------------------------------------------------------------------------
// a ballot over the lanes of one lane group
template <int LPR>
__device__ __forceinline__ unsigned long long group_ballot(bool pred, int gshift) {
    const unsigned long long b = __ballot(pred);
    return LPR == 64 ? b : ((b >> gshift) & ((1ull << LPR) - 1));
}

// k_bwd_chunks: the first position after p (within the chunk window) that starts another run, found by the group at once;
// SEG_CH: the run continues past this chunk
template <int LPR>
__device__ __forceinline__ int chunk_extent(const int32_t* __restrict__ mt, int64_t p, int64_t n, int c, int gshift) {
    constexpr int KM = (SEG_CH + LPR - 1) / LPR;
    int jstop = SEG_CH;
#pragma unroll
    for (int m = KM - 1; m >= 0; --m) {
        const int j = c + m * LPR;
        const int64_t q = p + 1 + j;
        const bool stop = (j < SEG_CH) && (q >= n || mt[q] == 0);
        const unsigned long long bits = group_ballot<LPR>(stop, gshift);
        if (bits) jstop = m * LPR + (__ffsll((long long)bits) - 1);
    }
    return jstop;
}

__device__ __forceinline__ void add4(float4& acc, const float4& v) { acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w; }

// gradient row of the lookup at batch position pos, this lane's column chunk (gc: the table's gradient + 4 * chunk)
template <bool ARANGE>
__device__ __forceinline__ float4 grad_row(const float* __restrict__ gc, int64_t ld_bag, const int64_t* __restrict__ off,
                                           int64_t n_bags, int64_t pos) {
    const int64_t bag = ARANGE ? pos : bag_of(off, n_bags, pos);
    return *reinterpret_cast<const float4*>(gc + bag * ld_bag);
}

// k_bwd_chunks' sum: the rows of the len sorted keys at kp, in position order, four loads in flight
template <bool ARANGE>
__device__ __forceinline__ float4 sum_rows_keys(const uint64_t* __restrict__ kp, int len, const float* __restrict__ gc,
                                                int64_t ld_bag, const int64_t* __restrict__ off, int64_t n_bags) {
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    int q = 0;
    for (; q + 4 <= len; q += 4) {
        int64_t bag[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int64_t pos = (int64_t)(kp[q + u] & 0xffffffffull);
            bag[u] = ARANGE ? pos : bag_of(off, n_bags, pos);
        }
        float4 v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) v[u] = *reinterpret_cast<const float4*>(gc + bag[u] * ld_bag);
#pragma unroll
        for (int u = 0; u < 4; ++u) add4(acc, v[u]);
    }
    for (; q < len; ++q) add4(acc, grad_row<ARANGE>(gc, ld_bag, off, n_bags, (int64_t)(kp[q] & 0xffffffffull)));
    return acc;
}

// k_bwd_blocks, one head in the block: the rows of the len positions at sp (LDS), RA loads in flight
template <bool ARANGE, int RA>
__device__ __forceinline__ float4 sum_rows_lone(const uint32_t* sp, int len, const float* __restrict__ gc, int64_t ld_bag,
                                                const int64_t* __restrict__ off, int64_t n_bags) {
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int q = 0; q < len; q += RA) {
        float4 v[RA];
#pragma unroll
        for (int u = 0; u < RA; ++u)
            if (q + u < len) v[u] = grad_row<ARANGE>(gc, ld_bag, off, n_bags, sp[q + u]);
#pragma unroll
        for (int u = 0; u < RA; ++u)
            if (q + u < len) add4(acc, v[u]);
    }
    return acc;
}

// a chunk head of a block (k_bwd_blocks): position j of the block, len positions of its run inside this chunk
struct Head {
    int j, len;                     // len == 0: no head
    bool head, single, more;        // the chunk starts its run / is the whole run / is not the run's last
    uint32_t slot;
};
__device__ __forceinline__ Head decode_head(uint64_t S, int j, const uint32_t* s_slot) {
    Head h;
    const uint64_t rest = S >> (j + 1);
    const int nxt = rest ? (__ffsll((long long)rest) - 1) : 64;
    h.more = nxt >= SEG_CH;
    h.len = h.more ? SEG_CH : nxt + 1;
    h.head = (S >> j) & 1;
    h.single = h.head && !h.more;
    h.j = j;
    h.slot = s_slot[j];
    return h;
}

// k_bwd_blocks, up to HU heads: four rows of each in flight
template <bool ARANGE, int HU>
__device__ __forceinline__ void sum_rows_heads(float4 (&acc)[HU], const Head (&h)[HU], int maxlen, const uint32_t* s_pos,
                                               const float* __restrict__ gc, int64_t ld_bag, const int64_t* __restrict__ off,
                                               int64_t n_bags) {
#pragma unroll
    for (int u = 0; u < HU; ++u) acc[u] = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int q = 0; q < maxlen; q += 4) {
        float4 v[HU][4];
#pragma unroll
        for (int u = 0; u < HU; ++u)
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (q + k < h[u].len) v[u][k] = grad_row<ARANGE>(gc, ld_bag, off, n_bags, s_pos[h[u].j + q + k]);
#pragma unroll
        for (int u = 0; u < HU; ++u)
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (q + k < h[u].len) add4(acc[u], v[u][k]);
    }
}

// what lane 0 of the group leaves behind for a chunk at sorted position p (r0 positions into its run): the row's touched flag,
// or the run's entry in the long-run list (its first chunk) and its end (its last chunk)
__device__ __forceinline__ void book_chunk(int t, int64_t p, const int32_t& r0, int len, bool head, bool single, bool more,
                                           bool flag, int64_t row, int64_t n, uint8_t* __restrict__ touched,
                                           int64_t* __restrict__ longlist, int32_t* __restrict__ longcount,
                                           int32_t* __restrict__ runend) {
    if (single) {
        if (touched && flag) touched[row] = 1;
    } else if (head) {
        const int li = atomicAdd(longcount, 1);
        longlist[li] = ((int64_t)t << 40) | p;
    }
    // the LAST chunk of a long run knows where the run ends: leave it at the run's head for k_bwd_long (which
    // would otherwise find it by a 13-step binary search over the keys, one dependent global read per step)
    if (!single && !more) runend[(int64_t)t * n + (p - r0)] = (int32_t)(p + len);
}

// k_bwd_long's sum: the chunk partials of the run [p0, end) in chunk order (a fixed order: reproducible), sixteen then four loads
// in flight (a tiny table's run is thousands of lookups = a hundred partials behind ONE lane group: at four in flight the kernel
// was its latency chain).  pc: the table's partials + this lane's column chunk
__device__ __forceinline__ float4 fold_partials(const float4* __restrict__ pc, int D4, int64_t p0, int64_t end) {
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    // at most two chunk heads of long runs share one SEG_CH-aligned bucket of positions: the run's first chunk is the odd one
    auto partial = [&](int64_t q) { return pc[(2 * (q / SEG_CH) + (q == p0 ? 1 : 0)) * D4]; };
    int64_t p = p0;
    for (; p + 15 * SEG_CH < end; p += 16 * SEG_CH) {
        float4 v[16];
#pragma unroll
        for (int u = 0; u < 16; ++u) v[u] = partial(p + u * SEG_CH);
#pragma unroll
        for (int u = 0; u < 16; ++u) add4(acc, v[u]);
    }
    for (; p + 3 * SEG_CH < end; p += 4 * SEG_CH) {
        float4 v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) v[u] = partial(p + u * SEG_CH);
#pragma unroll
        for (int u = 0; u < 4; ++u) add4(acc, v[u]);
    }
    for (; p < end; p += SEG_CH) add4(acc, partial(p));
    return acc;
}

// ---- the apply kernels ---------------------------------------------------------------------------------------------------------
// A lane group per sorted position; only chunk heads work.
// (kstride: elements between two tables' sorted lists -- n, or nb * n inside a window's sorted chunk; aux_add: the sorted
//  chunk holds phase-0 aux slots, the batch trains on aux region aux_add / aux)
template <class Row, bool ARANGE>
__global__ void __launch_bounds__(256) k_bwd_chunks(const TableDesc* __restrict__ tab, int D4,
                                                    float4* __restrict__ weight, const uint64_t* __restrict__ keys,
                                                    const int32_t* __restrict__ meta,
                                                    const int64_t* __restrict__ offsets, int64_t n, int64_t n_bags,
                                                    int64_t ld_off, const float* __restrict__ grad, int64_t ld_bag,
                                                    int64_t ld_table, float lr, float4* __restrict__ partials,
                                                    int64_t pstride, int64_t* __restrict__ longlist,
                                                    int32_t* __restrict__ longcount, uint8_t* __restrict__ touched,
                                                    int64_t aux_total, int32_t* __restrict__ runend, int64_t kstride,
                                                    int ways, int aux_add, AdaArgs o) {
    constexpr int LPR = Row::LPR;
    const int t = blockIdx.y;
    const int64_t row_base = tab[t].row_base;
    const int c = threadIdx.x % LPR;
    const int gpb = blockDim.x / LPR;
    const int gid = threadIdx.x / LPR;
    const int gshift = ((threadIdx.x & 63) / LPR) * LPR;
    const uint64_t* kt = keys + (int64_t)t * kstride;
    const int32_t* mt = meta + (int64_t)t * kstride;
    const uint32_t aux0 = (uint32_t)(tab[t].P * ways);
    const float* g = grad + (int64_t)t * ld_table;
    const int64_t* off = ARANGE ? nullptr : offsets + (int64_t)t * ld_off;
    const RowCtx x = {tab, t, ways, D4, c, aux0, (uint32_t)(tab[t].rows - aux_total), lr, o};
    for (int64_t p = (int64_t)blockIdx.x * gpb + gid; p < n; p += (int64_t)gridDim.x * gpb) {
        const int r0 = mt[p];
        if (r0 % SEG_CH) continue;               // chunk interior: some other group owns this position
        const bool head = r0 == 0;
        uint32_t slot = (uint32_t)(kt[p] >> 32);
        if (slot >= aux0) slot += aux_add;
        const int jstop = chunk_extent<LPR>(mt, p, n, c, gshift);
        const bool more = jstop == SEG_CH;
        const int len = more ? SEG_CH : jstop + 1;
        const bool single = head && !more;
        Row r;
        r.find(x, slot, single);
        r.read_state(x);
        float4* wrow = weight + (row_base + slot) * D4;
        // at most two chunk heads of long runs share one SEG_CH-aligned bucket of positions
        float4* prow = partials + ((int64_t)t * pstride + 2 * (p / SEG_CH) + (head ? 1 : 0)) * D4;
        Row::for_chunks(c, D4, [&](int k, int cc) __attribute__((always_inline)) {
            r.load(k, wrow + cc);
            const float4 acc = sum_rows_keys<ARANGE>(kt + p, len, g + cc * 4, ld_bag, off, n_bags);
            r.chunk(k, wrow + cc, acc, lr);
            if (!single) prow[cc] = acc;
        });
        r.finish(x, wrow);
        if (c == 0)
            book_chunk(t, p, r0, len, head, single, more, r.flag(x, slot), row_base + slot, n, touched, longlist, longcount, runend);
    }
}

// The same sums in the same order (bit-identical to k_bwd_chunks), laid out for memory-level parallelism.  k_bwd_chunks gives a
// lane group ONE sorted position per trip: meta -> look-ahead meta -> key -> gradient / row loads are four dependent global
// reads, and a group makes ~9 such trips at c3 -- the kernel is a chain of latencies (52 us alone for 166 MB of traffic).
// Here a lane group owns a BLOCK of SEG_CH consecutive sorted positions: one coalesced read brings the keys and run distances of
// the block and of the SEG_CH positions behind it (a chunk that starts in the block ends at most there), run starts and chunk
// heads become two bit masks (a ballot), and the heads of the block are worked HU AT A TIME with four gradient rows each in
// flight (RA rows when the block holds one head: the inside of a long run).  Two dependent reads per block instead of four per
// position.  Instantiated for AdaRow (skip_once, the `rest` entries' switch, is an SGD matter -- k_bwd_blocks_sgd below --; the
// parameter and aux_total are not read here: launch_blocks passes one argument list to either kernel).
template <class Row, bool ARANGE, int HU = 4, int RA = 16>
__global__ void __launch_bounds__(256) k_bwd_blocks(const TableDesc* __restrict__ tab, int D4,
                                                    float4* __restrict__ weight, const uint64_t* __restrict__ keys,
                                                    const int32_t* __restrict__ meta,
                                                    const int64_t* __restrict__ offsets, int64_t n, int64_t n_bags,
                                                    int64_t ld_off, const float* __restrict__ grad, int64_t ld_bag,
                                                    int64_t ld_table, float lr, float4* __restrict__ partials,
                                                    int64_t pstride, int64_t* __restrict__ longlist,
                                                    int32_t* __restrict__ longcount, uint8_t* __restrict__ touched,
                                                    int64_t aux_total, int32_t* __restrict__ runend, int skip_once,
                                                    int64_t kstride, int ways, int aux_add, AdaArgs o) {
    constexpr int LPR = Row::LPR;
    constexpr int GPB = 256 / LPR;
    constexpr int SPAN = 2 * SEG_CH;                // positions a block's chunks can reach
    constexpr int NL = SPAN / LPR;                  // span positions per lane
    static_assert(SEG_CH == 32 && SPAN % LPR == 0, "masks below are 32 / 64 bits wide");
    __shared__ uint32_t s_pos[GPB][SPAN];           // low half of the key: the lookup's position in the batch
    __shared__ uint32_t s_slot[GPB][SEG_CH];
    __shared__ int32_t s_r0[GPB][SEG_CH];
    const int t = blockIdx.y;
    const int64_t row_base = tab[t].row_base;
    const int c = threadIdx.x % LPR;
    const int gid = threadIdx.x / LPR;
    const int gshift = ((threadIdx.x & 63) / LPR) * LPR;
    const uint64_t* kt = keys + (int64_t)t * kstride;
    const int32_t* mt = meta + (int64_t)t * kstride;
    const uint32_t aux0 = (uint32_t)(tab[t].P * ways);
    const float* g = grad + (int64_t)t * ld_table;
    const int64_t* off = ARANGE ? nullptr : offsets + (int64_t)t * ld_off;
    const RowCtx x = {tab, t, ways, D4, c, aux0, (uint32_t)(tab[t].rows - aux_total), lr, o};
    const int64_t nblk = (n + SEG_CH - 1) / SEG_CH;
    for (int64_t blk = (int64_t)blockIdx.x * GPB + gid; blk < nblk; blk += (int64_t)gridDim.x * GPB) {
        const int64_t p0 = blk * SEG_CH;
        uint64_t S = 0;                              // bit j: position p0 + j starts a run (or lies past the end)
        uint32_t H = 0;                              // bit j < SEG_CH: position p0 + j is a chunk head
        __builtin_amdgcn_wave_barrier();             // the previous block's LDS reads are issued before these writes
#pragma unroll
        for (int m = 0; m < NL; ++m) {
            const int j = c + m * LPR;
            const int64_t q = p0 + j;
            const bool in = q < n;
            const uint64_t key = in ? kt[q] : 0ull;
            const int32_t r = in ? mt[q] : 0;
            s_pos[gid][j] = (uint32_t)key;
            if (j < SEG_CH) {
                uint32_t slot = (uint32_t)(key >> 32);
                if (slot >= aux0) slot += aux_add;
                s_slot[gid][j] = slot;
                s_r0[gid][j] = r;
            }
            S |= group_ballot<LPR>(r == 0, gshift) << (m * LPR);
            if (m * LPR < SEG_CH) H |= (uint32_t)(group_ballot<LPR>(in && j < SEG_CH && (r % SEG_CH) == 0, gshift) << (m * LPR));
        }
        __builtin_amdgcn_wave_barrier();
        float4* pbucket = partials + ((int64_t)t * pstride + 2 * blk) * D4;
        while (H) {
            const bool alone = (H & (H - 1)) == 0;
            if (alone) {
                // one head: RA gradient rows in flight
                const Head h = decode_head(S, __ffs((int)H) - 1, s_slot[gid]);
                H = 0;
                Row r;
                r.find(x, h.slot, h.single);
                r.read_state(x);
                float4* wrow = weight + (row_base + h.slot) * D4;
                Row::for_chunks(c, D4, [&](int k, int cc) __attribute__((always_inline)) {
                    r.load(k, wrow + cc);
                    const float4 acc = sum_rows_lone<ARANGE, RA>(s_pos[gid] + h.j, h.len, g + cc * 4, ld_bag, off, n_bags);
                    r.chunk(k, wrow + cc, acc, lr);
                    if (!h.single) pbucket[(h.head ? 1 : 0) * D4 + cc] = acc;
                });
                r.finish(x, wrow);
                if (c == 0)
                    book_chunk(t, p0 + h.j, s_r0[gid][h.j], h.len, h.head, h.single, h.more, r.flag(x, h.slot), row_base + h.slot, n,
                               touched, longlist, longcount, runend);
                continue;
            }
            // up to HU heads, four gradient rows of each in flight
            Head h[HU];
            Row r[HU];
            int maxlen = 0;
#pragma unroll
            for (int u = 0; u < HU; ++u) {
                h[u] = Head{0, 0, false, false, false, 0};
                if (H) {
                    h[u] = decode_head(S, __ffs((int)H) - 1, s_slot[gid]);
                    H &= H - 1;
                    maxlen = max(maxlen, h[u].len);
                    r[u].find(x, h[u].slot, h[u].single);
                }
            }
#pragma unroll
            for (int u = 0; u < HU; ++u) r[u].read_state(x);
            Row::for_chunks(c, D4, [&](int k, int cc) __attribute__((always_inline)) {
                float4 acc[HU];
#pragma unroll
                for (int u = 0; u < HU; ++u) r[u].load(k, weight + (row_base + h[u].slot) * D4 + cc);
                sum_rows_heads<ARANGE, HU>(acc, h, maxlen, s_pos[gid], g + cc * 4, ld_bag, off, n_bags);
#pragma unroll
                for (int u = 0; u < HU; ++u) {
                    if (h[u].len == 0) continue;
                    r[u].chunk(k, weight + (row_base + h[u].slot) * D4 + cc, acc[u], lr);
                    if (!h[u].single) pbucket[(h[u].head ? 1 : 0) * D4 + cc] = acc[u];
                }
            });
#pragma unroll
            for (int u = 0; u < HU; ++u) r[u].finish(x, weight + (row_base + h[u].slot) * D4);
            if (c == 0) {
#pragma unroll
                for (int u = 0; u < HU; ++u) {
                    if (h[u].len == 0) continue;
                    book_chunk(t, p0 + h[u].j, s_r0[gid][h[u].j], h[u].len, h[u].head, h[u].single, h[u].more, r[u].flag(x, h[u].slot),
                               row_base + h[u].slot, n, touched, longlist, longcount, runend);
                }
            }
        }
    }
}

// k_bwd_blocks with the SGD update, in its own text: the shared body above with SgdRow ran the lean <.., true, 1, 8> form 15 %
// slower alone (47.4 against 41.3 us, profiles/emb_apply_refactor_times.txt), so the SGD kernel keeps the text it was measured
// and tuned with (bwd_apply_plan) and k_bwd_blocks above is instantiated for AdaRow only.  The same sums in the same order:
// tests/test_emb_apply_digests.py and test_embbag_bwd_routes.py ("same bits across kernels") hold the two texts together.
// skip_once: runs of ONE lookup were updated by the interaction backward itself (cdlrm_gather_interact_bwd_sgd).  (The unnamed
// AdaArgs: launch_blocks' one argument list; not read.)
template <int LPR, bool ARANGE, int HU = 4, int RA = 16>
__global__ void __launch_bounds__(256) k_bwd_blocks_sgd(const TableDesc* __restrict__ tab, int D4,
                                                    float4* __restrict__ weight, const uint64_t* __restrict__ keys,
                                                    const int32_t* __restrict__ meta,
                                                    const int64_t* __restrict__ offsets, int64_t n, int64_t n_bags,
                                                    int64_t ld_off, const float* __restrict__ grad, int64_t ld_bag,
                                                    int64_t ld_table, float lr, float4* __restrict__ partials,
                                                    int64_t pstride, int64_t* __restrict__ longlist,
                                                    int32_t* __restrict__ longcount, uint8_t* __restrict__ touched,
                                                    int64_t aux_total, int32_t* __restrict__ runend, int skip_once,
                                                    int64_t kstride, int ways, int aux_add, AdaArgs) {
    constexpr int GPB = 256 / LPR;
    constexpr int SPAN = 2 * SEG_CH;                // positions a block's chunks can reach
    constexpr int NL = SPAN / LPR;                  // span positions per lane
    static_assert(SEG_CH == 32 && SPAN % LPR == 0, "masks below are 32 / 64 bits wide");
    __shared__ uint32_t s_pos[GPB][SPAN];           // low half of the key: the lookup's position in the batch
    __shared__ uint32_t s_slot[GPB][SEG_CH];
    __shared__ int32_t s_r0[GPB][SEG_CH];
    const int t = blockIdx.y;
    const int64_t row_base = tab[t].row_base;
    const uint32_t first_aux = (uint32_t)(tab[t].rows - aux_total);
    const int c = threadIdx.x % LPR;
    const int gid = threadIdx.x / LPR;
    const int gshift = ((threadIdx.x & 63) / LPR) * LPR;
    const uint64_t* kt = keys + (int64_t)t * kstride;
    const int32_t* mt = meta + (int64_t)t * kstride;
    const uint32_t aux0 = (uint32_t)(tab[t].P * ways);
    const float* g = grad + (int64_t)t * ld_table;
    const int64_t* off = ARANGE ? nullptr : offsets + (int64_t)t * ld_off;
    const int64_t nblk = (n + SEG_CH - 1) / SEG_CH;
    for (int64_t blk = (int64_t)blockIdx.x * GPB + gid; blk < nblk; blk += (int64_t)gridDim.x * GPB) {
        const int64_t p0 = blk * SEG_CH;
        uint64_t S = 0;                              // bit j: position p0 + j starts a run (or lies past the end)
        uint32_t H = 0;                              // bit j < SEG_CH: position p0 + j is a chunk head
        __builtin_amdgcn_wave_barrier();             // the previous block's LDS reads are issued before these writes
#pragma unroll
        for (int m = 0; m < NL; ++m) {
            const int j = c + m * LPR;
            const int64_t q = p0 + j;
            const bool in = q < n;
            const uint64_t key = in ? kt[q] : 0ull;
            const int32_t r = in ? mt[q] : 0;
            s_pos[gid][j] = (uint32_t)key;
            if (j < SEG_CH) {
                uint32_t slot = (uint32_t)(key >> 32);
                if (slot >= aux0) slot += aux_add;
                s_slot[gid][j] = slot;
                s_r0[gid][j] = r;
            }
            const unsigned long long b = __ballot(r == 0);
            const unsigned long long bits = LPR == 64 ? b : ((b >> gshift) & ((1ull << LPR) - 1));
            S |= bits << (m * LPR);
            if (m * LPR < SEG_CH) {
                const unsigned long long hb = __ballot(in && j < SEG_CH && (r % SEG_CH) == 0);
                const unsigned long long hbits = LPR == 64 ? hb : ((hb >> gshift) & ((1ull << LPR) - 1));
                H |= (uint32_t)(hbits << (m * LPR));
            }
        }
        __builtin_amdgcn_wave_barrier();
        if (skip_once) {
            // runs of ONE lookup were updated by the interaction backward itself (cdlrm_gather_interact_bwd_sgd): a start
            // followed by a start.  Only their touched flags are left to set.
            const uint32_t one = (uint32_t)(S & (S >> 1)) & H;
            H &= ~one;
            if (touched) {
#pragma unroll
                for (int m = 0; m * LPR < SEG_CH; ++m) {
                    const int j = c + m * LPR;
                    if (j < SEG_CH && ((one >> j) & 1)) {
                        const uint32_t slot = s_slot[gid][j];
                        if (slot < first_aux) touched[row_base + slot] = 1;
                    }
                }
            }
        }
        const int64_t pbucket = (int64_t)t * pstride + 2 * blk;
        while (H) {
            const bool alone = (H & (H - 1)) == 0;
            if (alone) {
                // one head: 16 gradient rows in flight
                const int j = __ffs((int)H) - 1;
                H = 0;
                const uint64_t rest = S >> (j + 1);
                const int nxt = rest ? (__ffsll((long long)rest) - 1) : 64;
                const bool more = nxt >= SEG_CH;
                const int len = more ? SEG_CH : nxt + 1;
                const bool head = (S >> j) & 1;
                const bool single = head && !more;
                const uint32_t slot = s_slot[gid][j];
                for (int cc = c; cc < D4; cc += LPR) {
                    float4 w;
                    if (single) w = weight[(row_base + slot) * D4 + cc];
                    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
                    for (int q = 0; q < len; q += RA) {
                        float4 v[RA];
#pragma unroll
                        for (int u = 0; u < RA; ++u)
                            if (q + u < len) {
                                const int64_t pos = s_pos[gid][j + q + u];
                                const int64_t bag = ARANGE ? pos : bag_of(off, n_bags, pos);
                                v[u] = *reinterpret_cast<const float4*>(g + bag * ld_bag + cc * 4);
                            }
#pragma unroll
                        for (int u = 0; u < RA; ++u)
                            if (q + u < len) { acc.x += v[u].x; acc.y += v[u].y; acc.z += v[u].z; acc.w += v[u].w; }
                    }
                    if (single) {
                        w.x = fmaf(-lr, acc.x, w.x); w.y = fmaf(-lr, acc.y, w.y);
                        w.z = fmaf(-lr, acc.z, w.z); w.w = fmaf(-lr, acc.w, w.w);
                        weight[(row_base + slot) * D4 + cc] = w;
                    } else {
                        partials[(pbucket + (head ? 1 : 0)) * D4 + cc] = acc;
                    }
                }
                if (c == 0) {
                    const int64_t p = p0 + j;
                    if (single) {
                        if (touched && slot < first_aux) touched[row_base + slot] = 1;
                    } else if (head) {
                        const int li = atomicAdd(longcount, 1);
                        longlist[li] = ((int64_t)t << 40) | p;
                    }
                    if (!single && !more) runend[(int64_t)t * n + (p - s_r0[gid][j])] = (int32_t)(p + len);
                }
                continue;
            }
            // up to four heads, four gradient rows of each in flight
            int hj[HU], hlen[HU];
            bool hhead[HU], hsingle[HU], hmore[HU];
            uint32_t hslot[HU];
            int maxlen = 0;
#pragma unroll
            for (int u = 0; u < HU; ++u) {
                hlen[u] = 0; hj[u] = 0; hhead[u] = false; hsingle[u] = false; hmore[u] = false; hslot[u] = 0;
                if (H) {
                    const int j = __ffs((int)H) - 1;
                    H &= H - 1;
                    const uint64_t rest = S >> (j + 1);
                    const int nxt = rest ? (__ffsll((long long)rest) - 1) : 64;
                    hmore[u] = nxt >= SEG_CH;
                    hlen[u] = hmore[u] ? SEG_CH : nxt + 1;
                    hhead[u] = (S >> j) & 1;
                    hsingle[u] = hhead[u] && !hmore[u];
                    hj[u] = j;
                    hslot[u] = s_slot[gid][j];
                    maxlen = max(maxlen, hlen[u]);
                }
            }
            for (int cc = c; cc < D4; cc += LPR) {
                float4 w[HU], acc[HU];
#pragma unroll
                for (int u = 0; u < HU; ++u) {
                    acc[u] = make_float4(0.f, 0.f, 0.f, 0.f);
                    if (hsingle[u]) w[u] = weight[(row_base + hslot[u]) * D4 + cc];
                }
                for (int q = 0; q < maxlen; q += 4) {
                    float4 v[HU][4];
#pragma unroll
                    for (int u = 0; u < HU; ++u)
#pragma unroll
                        for (int k = 0; k < 4; ++k)
                            if (q + k < hlen[u]) {
                                const int64_t pos = s_pos[gid][hj[u] + q + k];
                                const int64_t bag = ARANGE ? pos : bag_of(off, n_bags, pos);
                                v[u][k] = *reinterpret_cast<const float4*>(g + bag * ld_bag + cc * 4);
                            }
#pragma unroll
                    for (int u = 0; u < HU; ++u)
#pragma unroll
                        for (int k = 0; k < 4; ++k)
                            if (q + k < hlen[u]) {
                                acc[u].x += v[u][k].x; acc[u].y += v[u][k].y; acc[u].z += v[u][k].z; acc[u].w += v[u][k].w;
                            }
                }
#pragma unroll
                for (int u = 0; u < HU; ++u) {
                    if (hlen[u] == 0) continue;
                    if (hsingle[u]) {
                        w[u].x = fmaf(-lr, acc[u].x, w[u].x); w[u].y = fmaf(-lr, acc[u].y, w[u].y);
                        w[u].z = fmaf(-lr, acc[u].z, w[u].z); w[u].w = fmaf(-lr, acc[u].w, w[u].w);
                        weight[(row_base + hslot[u]) * D4 + cc] = w[u];
                    } else {
                        partials[(pbucket + (hhead[u] ? 1 : 0)) * D4 + cc] = acc[u];
                    }
                }
            }
            if (c == 0) {
#pragma unroll
                for (int u = 0; u < HU; ++u) {
                    if (hlen[u] == 0) continue;
                    const int64_t p = p0 + hj[u];
                    if (hsingle[u]) {
                        if (touched && hslot[u] < first_aux) touched[row_base + hslot[u]] = 1;
                    } else if (hhead[u]) {
                        const int li = atomicAdd(longcount, 1);
                        longlist[li] = ((int64_t)t << 40) | p;
                    }
                    if (!hsingle[u] && !hmore[u]) runend[(int64_t)t * n + (p - s_r0[gid][hj[u]])] = (int32_t)(p + hlen[u]);
                }
            }
        }
    }
}

// k_bwd_long with the SGD update, in its own text like k_bwd_blocks_sgd and for the same reason: with SgdRow the shared body below
// compiled to 152 registers against this text's 202 (3 waves per SIMD against 2) and the SGD applies that end in it ran 1 to
// 1.5 us over the parent's slowest round (profiles/emb_apply_refactor_times.txt, section B); k_bwd_long below is instantiated for
// AdaRow only.  (The unnamed AdaArgs: launch_long passes one argument list to either kernel; this one does not read it.)
template <int LPR>
__global__ void __launch_bounds__(256) k_bwd_long_sgd(const TableDesc* __restrict__ tab, int D4,
                                                  float4* __restrict__ weight, const uint64_t* __restrict__ keys,
                                                  int64_t n, float lr, const float4* __restrict__ partials,
                                                  int64_t pstride, const int64_t* __restrict__ longlist,
                                                  int32_t* __restrict__ longcount, uint8_t* __restrict__ touched,
                                                  int64_t aux_total, const int32_t* __restrict__ runend, int64_t kstride,
                                                  int ways, int aux_add, AdaArgs) {
    const int c = threadIdx.x % LPR;
    const int gpb = blockDim.x / LPR;
    const int gid = threadIdx.x / LPR;
    const int cnt = *longcount;
    // The list counter lives in the work buffer: cleared by the first kernel of every prepare (k_sort_chunks) AND left zero by
    // the last workgroup of this kernel to finish -- every workgroup has read it by then --, so a second apply on one prepare
    // (a benchmark loop) starts from an empty list too.  longcount[2] counts the workgroups that are through.
    __syncthreads();
    if (threadIdx.x == 0) {
        const int through = atomicAdd(longcount + 2, 1);
        if (through == (int)gridDim.x - 1) {
            atomicExch(longcount, 0);
            atomicExch(longcount + 2, 0);
        }
    }
    for (int li = blockIdx.x * gpb + gid; li < cnt; li += gridDim.x * gpb) {
        const int64_t e = longlist[li];
        const int t = (int)(e >> 40);
        const int64_t p0 = e & (((int64_t)1 << 40) - 1);
        const uint64_t* kt = keys + (int64_t)t * kstride;
        uint32_t slot = (uint32_t)(kt[p0] >> 32);
        if (slot >= (uint32_t)(tab[t].P * ways)) slot += aux_add;
        const int64_t end = runend[(int64_t)t * n + p0];
        const int64_t row = tab[t].row_base + slot;
        for (int cc = c; cc < D4; cc += LPR) {
            float4 w = weight[row * D4 + cc];
            float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
            // chunk partials in chunk order (a fixed order: reproducible), sixteen then four loads in flight (a tiny table's run is
            // thousands of lookups = a hundred partials behind ONE lane group: at four in flight the kernel was its latency chain)
            int64_t p = p0;
            for (; p + 15 * SEG_CH < end; p += 16 * SEG_CH) {
                float4 v[16];
#pragma unroll
                for (int u = 0; u < 16; ++u) {
                    const int64_t q = p + u * SEG_CH;
                    const int64_t pi = 2 * (q / SEG_CH) + (q == p0 ? 1 : 0);
                    v[u] = partials[((int64_t)t * pstride + pi) * D4 + cc];
                }
#pragma unroll
                for (int u = 0; u < 16; ++u) { acc.x += v[u].x; acc.y += v[u].y; acc.z += v[u].z; acc.w += v[u].w; }
            }
            for (; p + 3 * SEG_CH < end; p += 4 * SEG_CH) {
                float4 v[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int64_t q = p + u * SEG_CH;
                    const int64_t pi = 2 * (q / SEG_CH) + (q == p0 ? 1 : 0);
                    v[u] = partials[((int64_t)t * pstride + pi) * D4 + cc];
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) { acc.x += v[u].x; acc.y += v[u].y; acc.z += v[u].z; acc.w += v[u].w; }
            }
            for (; p < end; p += SEG_CH) {
                const int64_t pi = 2 * (p / SEG_CH) + (p == p0 ? 1 : 0);
                const float4 v = partials[((int64_t)t * pstride + pi) * D4 + cc];
                acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
            }
            w.x = fmaf(-lr, acc.x, w.x); w.y = fmaf(-lr, acc.y, w.y);
            w.z = fmaf(-lr, acc.z, w.z); w.w = fmaf(-lr, acc.w, w.w);
            weight[row * D4 + cc] = w;
        }
        if (c == 0 && touched && (int64_t)slot < tab[t].rows - aux_total) touched[row] = 1;
    }
}

// heads of long runs add their chunks' partial sums and update the row.  Instantiated for AdaRow (SGD: k_bwd_long_sgd above);
// aux_total is the SGD touched rule's and is not read here (one argument list for launch_long)
template <class Row>
__global__ void __launch_bounds__(256) k_bwd_long(const TableDesc* __restrict__ tab, int D4,
                                                  float4* __restrict__ weight, const uint64_t* __restrict__ keys,
                                                  int64_t n, float lr, const float4* __restrict__ partials,
                                                  int64_t pstride, const int64_t* __restrict__ longlist,
                                                  int32_t* __restrict__ longcount, uint8_t* __restrict__ touched,
                                                  int64_t aux_total, const int32_t* __restrict__ runend, int64_t kstride,
                                                  int ways, int aux_add, AdaArgs o) {
    constexpr int LPR = Row::LPR;
    const int c = threadIdx.x % LPR;
    const int gpb = blockDim.x / LPR;
    const int gid = threadIdx.x / LPR;
    const int cnt = *longcount;
    // The list counter lives in the work buffer: cleared by the first kernel of every prepare (k_sort_chunks) AND left zero by
    // the last workgroup of this kernel to finish -- every workgroup has read it by then --, so a second apply on one prepare
    // (a benchmark loop) starts from an empty list too.  longcount[2] counts the workgroups that are through.
    __syncthreads();
    if (threadIdx.x == 0) {
        const int through = atomicAdd(longcount + 2, 1);
        if (through == (int)gridDim.x - 1) {
            atomicExch(longcount, 0);
            atomicExch(longcount + 2, 0);
        }
    }
    for (int li = blockIdx.x * gpb + gid; li < cnt; li += gridDim.x * gpb) {
        const int64_t e = longlist[li];
        const int t = (int)(e >> 40);
        const int64_t p0 = e & (((int64_t)1 << 40) - 1);
        const uint64_t* kt = keys + (int64_t)t * kstride;
        uint32_t slot = (uint32_t)(kt[p0] >> 32);
        const uint32_t aux0 = (uint32_t)(tab[t].P * ways);
        if (slot >= aux0) slot += aux_add;
        const RowCtx x = {tab, t, ways, D4, c, aux0, 0 /* first_aux: SgdRow's */, lr, o};
        Row r;
        r.find(x, slot, true);
        if (!r.upd) continue;               // (AdaRow) an aux slot's run: its partial sums are dropped
        r.read_state(x);
        const int64_t end = runend[(int64_t)t * n + p0];
        const int64_t row = tab[t].row_base + slot;
        float4* wrow = weight + row * D4;
        Row::for_chunks(c, D4, [&](int k, int cc) __attribute__((always_inline)) {
            r.load(k, wrow + cc);
            const float4 acc = fold_partials(partials + (int64_t)t * pstride * D4 + cc, D4, p0, end);
            r.chunk(k, wrow + cc, acc, lr);
        });
        r.finish(x, wrow);
        if (c == 0 && touched && r.flag(x, slot)) touched[row] = 1;
    }
}

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
static uint64_t align256(uint64_t v) { return (v + 255) & ~(uint64_t)255; }
template <typename P> static P* at(const void* base, uint64_t off) { return (P*)((char*)base + off); }

// ---- buffer layouts: byte offsets of every region and the byte count ------------------------------------------------------------
// work layout: keys A [T*n] u64 | keys B [T*n] u64 | meta [T*n] i32 | partials [T*pstride*D] f32 |
//              longlist [T*(n/SEG_CH+2)] i64 | long-run counter | runend [T*n] i32 (end of a long run, at its head) |
//              once [T*n] u8 (by position in the batch: the lookup's slot occurs once in the batch)
struct BwdLayout {
    uint64_t keysA, keysB, meta, partials, longlist, longcount, runend, once, bytes;
    int64_t pstride;
};
static BwdLayout bwd_layout(int32_t T, int64_t n, int32_t D) {
    BwdLayout l;
    uint64_t o = 0;
    l.keysA = o; o += align256((uint64_t)T * n * 8);
    l.keysB = o; o += align256((uint64_t)T * n * 8);
    l.meta = o; o += align256((uint64_t)T * n * 4);
    l.pstride = 2 * (cdiv(n, SEG_CH) + 1);
    l.partials = o; o += align256((uint64_t)T * l.pstride * D * 4);
    l.longlist = o; o += align256((uint64_t)T * (n / SEG_CH + 2) * 8);
    l.longcount = o; o += 256;
    l.runend = o; o += align256((uint64_t)T * n * 4);
    l.once = o; o += align256((uint64_t)T * n);
    l.bytes = o;
    return l;
}

// ---- a window chunk's batches sorted at once (the look-ahead resolver's slot ids: cdlrm_window_resolve) ----------------------
// sorted layout: keys A [T*nb*n] u64 | keys B | meta [T*nb*n] i32 | once [T*nb*n] u8 | 256 B; list t * nb + j = table t, batch j
// (the 256 B: the counter words the sort kernel clears -- `longcount` of a buffer no apply reads)
struct SortedLayout {
    uint64_t keysA, keysB, meta, once, longcount, bytes;
};
static SortedLayout sorted_layout(int32_t T, int32_t nb, int64_t n) {
    SortedLayout l;
    const uint64_t e = (uint64_t)T * nb * n;
    uint64_t o = 0;
    l.keysA = o; o += align256(e * 8);
    l.keysB = o; o += align256(e * 8);
    l.meta = o; o += align256(e * 4);
    l.once = o; o += align256(e);
    l.longcount = o; o += 256;
    l.bytes = o;
    return l;
}

extern "C" uint64_t cdlrm_embbag_bwd_work_bytes(int32_t T, int64_t n, int32_t dim) { return bwd_layout(T, n, dim).bytes; }
extern "C" uint64_t cdlrm_embbag_bwd_sorted_bytes(int32_t num_tables, int32_t nb, int64_t n) {
    return sorted_layout(num_tables, nb, n).bytes;
}

// ---- the sort ------------------------------------------------------------------------------------------------------------------
// Keys per sorting workgroup.  The in-LDS sort is bound by vector-instruction issue on ONE CU (measured: 9 / 16 / 33 / 83 us
// for 1024 / 2048 / 4096 / 8192 keys per workgroup, tools/sort_scale.py), so mid-sized inputs are cut into 2048-key
// chunks that sort on different CUs and meet in global rank-merge passes (k_merge_pass, ~8 us each at 26 x 8192 keys);
// very long inputs (config c5: 65536 lookups per table) keep 8192-key chunks: there the merge passes dominate.
static int64_t sort_chunk(int64_t n) {
    if (n <= 2048) return n <= 1024 ? 1024 : 2048;
    return n <= 16384 ? 2048 : SORT_CHUNK;
}

// the sort of `lists` lists of n slot ids each (a batch: one list per table; a window chunk: one per table and batch)
// (Measured for the look-ahead slices, which have a whole step of slack, and not taken: ONE workgroup per list of 8192 keys -- 83
//  us on 52 CUs, no merge passes, one launch instead of four -- 0.5401 against 0.5363 ms per c3 step; a tie at a batch of 2048.)
struct BwdSortPlan {
    int chunk, E, nchunks;      // keys per sorting workgroup / per thread (the chunk spread over the 1024 threads), workgroups per list
    int passes;                 // rank-merge passes: k_merge_pass launches, keys A -> B -> A ...
    bool keys_in_b;             // ... so an odd number of them leaves the sorted keys in keys B
    bool seg_meta;              // several chunks per list: k_seg_meta writes the run distances and once-only flags, not the sort kernel
    dim3 sort_grid, merge_grid, meta_grid;
    size_t lds;                 // k_sort_chunks' dynamic LDS
};
static BwdSortPlan bwd_sort_plan(int lists, int64_t n) {
    BwdSortPlan p;
    const int64_t chunk = sort_chunk(n), nchunks = cdiv(n, chunk);
    p.chunk = (int)chunk;
    p.E = (int)(chunk / SORT_THREADS);
    p.nchunks = (int)nchunks;
    p.passes = 0;
    for (int64_t run = chunk; run < n; run *= 2) ++p.passes;
    p.keys_in_b = p.passes & 1;
    p.seg_meta = nchunks > 1;
    int64_t gx = cdiv(n, 256);
    if (gx > 4096) gx = 4096;
    p.sort_grid = dim3((unsigned)nchunks, (unsigned)lists);
    p.merge_grid = p.meta_grid = dim3((unsigned)gx, (unsigned)lists);
    p.lds = (size_t)SORT_THREADS * p.E * 8;
    return p;
}

// what the sort writes, in `work` or in a window chunk's `sorted`
struct SortBufs {
    uint64_t *keysA, *keysB;
    int32_t* meta;
    uint8_t* once;
    int32_t* longcount;
};
template <typename Layout>
static SortBufs sort_bufs(void* base, const Layout& l) {
    return {at<uint64_t>(base, l.keysA), at<uint64_t>(base, l.keysB), at<int32_t>(base, l.meta), at<uint8_t>(base, l.once),
            at<int32_t>(base, l.longcount)};
}

// byte offsets of the sorted keys / run distances / once-only flags of list j (table 0; a batch's own sort: j = 0): what
// _sorted_views, the per-batch apply and the route query all read
struct SortedOffs {
    uint64_t keys, meta, once;
};
template <typename Layout>
static SortedOffs sorted_offs(const Layout& l, const BwdSortPlan& p, int64_t n, int64_t j) {
    return {(p.keys_in_b ? l.keysB : l.keysA) + (uint64_t)(j * n) * 8, l.meta + (uint64_t)(j * n) * 4, l.once + (uint64_t)(j * n)};
}

// slots: list t = batch t % nb of table t / nb, at slots[(t / nb) * ld_in + (t % nb) * batch_len ..]; its output list:
// (t / nb) * nbt + j0 + t % nb (k_sort_chunks)
static int bwd_sort_launch(const BwdSortPlan& p, const SortBufs& b, const int32_t* slots, int64_t n, int nb, int64_t ld_in,
                           int64_t batch_len, int nbt, int j0, hipStream_t s) {
    const int wm = p.seg_meta ? 0 : 1;
#define SORT_CALL(E_)                                                                                                      \
    hipLaunchKernelGGL(k_sort_chunks<E_>, p.sort_grid, dim3(SORT_THREADS), p.lds, s, slots, n, b.keysA, b.meta, p.chunk, wm, \
                       b.longcount, b.once, nb, ld_in, batch_len, nbt, j0)
    switch (p.E) {
        case 1: SORT_CALL(1); break;
        case 2: SORT_CALL(2); break;
        case 4: SORT_CALL(4); break;
        default: {
            const int rc = cdlrm_grant_dynamic_lds<k_sort_chunks<8>>(p.lds);
            if (rc) return rc;
            SORT_CALL(8);
        }
    }
#undef SORT_CALL
    int64_t run = p.chunk;
    for (int i = 0; i < p.passes; ++i, run *= 2)
        hipLaunchKernelGGL(k_merge_pass, p.merge_grid, dim3(256), 0, s, (i & 1) ? b.keysB : b.keysA, (i & 1) ? b.keysA : b.keysB, n,
                           run, nb, nbt, j0);
    if (p.seg_meta)
        hipLaunchKernelGGL(k_seg_meta, p.meta_grid, dim3(256), 0, s, p.keys_in_b ? b.keysB : b.keysA, n, b.meta, b.once, nb, nbt, j0);
    CDLRM_LAUNCH_CHECK();
    return 0;
}

// ---- the apply -----------------------------------------------------------------------------------------------------------------
struct BwdApplyPlan {
    int kernel;                 // CDLRM_BWD_APPLY_*
    int arange, lpr;            // one lookup per bag (no offsets); lanes per row
    int64_t grid_x, grid_y;     // the apply kernel's grid
    int64_t long_grid;          // k_bwd_long's
};
static BwdApplyPlan bwd_apply_plan(int T, int D, int64_t n, bool has_offsets, bool skip_once) {
    BwdApplyPlan p;
    p.arange = !has_offsets;
    p.lpr = lanes_per_row(D / 4);
    const int gpb = 256 / p.lpr;
    // a lane group per block of SEG_CH sorted positions (k_bwd_blocks): the form for the runs of >= 2 lookups that
    // cdlrm_embbag_bwd_apply_rest is left with (few heads per block).  With every run of one lookup in the list it is slower
    // than a lane group per position (c3: 48.8 against 44.0 us alone, 144 against 105 us inside the step: a block of a large
    // table holds 30 heads = 8 trips); cdlrm_debug_set(6, 64) selects it there too
    const bool blocks = skip_once || (g_cdlrm_debug[6] & 64);
    // The lean form: the runs of >= 2 lookups, one lookup per bag: ONE head at a time with four rows in flight (eight when the block
    // holds one head) -- 4 x 4 / 16 rows in flight need 239 registers, and beside the weight-gradient GEMMs it is the kernel's
    // footprint on a SIMD, not its own latency chain, that the step pays for (alone it finishes in 30 us either way).  c3,
    // tools/ab_step.py, one box, 4 rounds: heads x rows / lone-head rows 4x4/16: 0.5393 ms, 2x4/8: 0.5357, 1x4/8: 0.5332,
    // 2x4/4: 0.5362, 1x4/4: 0.5350.  cdlrm_debug_set(6, 128): the 4x4/16 form.
    const bool lean = blocks && !has_offsets && skip_once && !(g_cdlrm_debug[6] & 128);
    p.kernel = !blocks ? CDLRM_BWD_APPLY_CHUNKS : lean ? CDLRM_BWD_APPLY_BLOCKS_LEAN : CDLRM_BWD_APPLY_BLOCKS;
    int64_t gx = blocks ? cdiv(cdiv(n, SEG_CH), gpb) : cdiv(n, gpb);
    if (!blocks && gx > 65535) gx = 65535;
    // at most 12 workgroups per CU (the position loop strides): the kernel runs on a side queue beside the weight-gradient and
    // bottom-MLP GEMMs, and an unbounded grid (26 624 workgroups at c3, 213 k at c5) takes every free wave slot between their
    // launches.  Same box, same process, 6 x 90 steps each (tools/ab_step.py --attr debug:1): uncapped / 12 / 8 / 6 / 4 per CU
    // -> 0.5804 / 0.5754 / 0.5762 / 0.5977 / 0.6386 ms at c3 (10 .. 24: the same as 12), 3.762 / 3.722 ms at c5, nothing at a
    // per-rank batch of 1024 (3328 workgroups to begin with).  Results do not depend on the grid (a position is owned by
    // one lane group).  cdlrm_debug_set(1, n): n per CU, -1 uncapped
    const int per_cu = g_cdlrm_debug[1] > 0 ? g_cdlrm_debug[1] : 12;
    const int64_t cap = cdiv((int64_t)256 * per_cu, T);
    if (g_cdlrm_debug[1] >= 0 && gx > cap) gx = cap;
    p.grid_x = gx;
    p.grid_y = T;
    p.long_grid = cdiv((int64_t)T * (n / SEG_CH + 1), gpb);
    if (p.long_grid > 1024) p.long_grid = 1024;
    return p;
}

// what k_bwd_chunks, k_bwd_blocks and k_bwd_long take.  keys / meta: table 0's sorted list, table t's lies kstride elements further
// (a batch's own sort: n; a window chunk's: nb * n); aux_add: the sorted slots are phase-0 aux slots, the batch trains on aux region
// aux_add / aux (0 for a batch's own sort: k_take has added the phase); partials .. runend: the scratch of `work`
struct BwdApplyArgs {
    const TableDesc* tab;
    int D4;
    float4* weight;
    const uint64_t* keys;
    const int32_t* meta;
    int64_t kstride;
    const int64_t* offsets;
    int64_t n, n_bags, ld_off;
    const float* grad;
    int64_t ld_bag, ld_table;
    float lr;
    float4* partials;
    int64_t pstride;
    int64_t* longlist;
    int32_t *longcount, *runend;
    uint8_t* touched;
    int64_t aux_total;
    int skip_once, ways, aux_add;
    int opt;                    // CDLRM_EMB_OPT_*: SgdRow / AdaRow
    AdaArgs ada;                // (read by the AdaRow kernels only)
};

template <auto Kernel>
static void launch_chunks(dim3 grid, const BwdApplyArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(Kernel, grid, dim3(256), 0, s, a.tab, a.D4, a.weight, a.keys, a.meta, a.offsets, a.n, a.n_bags, a.ld_off,
                       a.grad, a.ld_bag, a.ld_table, a.lr, a.partials, a.pstride, a.longlist, a.longcount, a.touched, a.aux_total,
                       a.runend, a.kstride, a.ways, a.aux_add, a.ada);
}
template <auto Kernel>
static void launch_blocks(dim3 grid, const BwdApplyArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(Kernel, grid, dim3(256), 0, s, a.tab, a.D4, a.weight, a.keys, a.meta, a.offsets, a.n, a.n_bags, a.ld_off,
                       a.grad, a.ld_bag, a.ld_table, a.lr, a.partials, a.pstride, a.longlist, a.longcount, a.touched, a.aux_total,
                       a.runend, a.skip_once, a.kstride, a.ways, a.aux_add, a.ada);
}
template <auto Kernel>
static void launch_long(dim3 grid, const BwdApplyArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(Kernel, grid, dim3(256), 0, s, a.tab, a.D4, a.weight, a.keys, a.n, a.lr, a.partials, a.pstride, a.longlist,
                       a.longcount, a.touched, a.aux_total, a.runend, a.kstride, a.ways, a.aux_add, a.ada);
}

// sums + row updates (the plan's apply kernel), then the long runs
template <class Row>
static void bwd_apply_launch_row(const BwdApplyPlan& p, const BwdApplyArgs& a, hipStream_t s) {
    const dim3 grid((unsigned)p.grid_x, (unsigned)p.grid_y);
    if (p.kernel == CDLRM_BWD_APPLY_CHUNKS) {
        if (p.arange) launch_chunks<k_bwd_chunks<Row, true>>(grid, a, s);
        else launch_chunks<k_bwd_chunks<Row, false>>(grid, a, s);
    } else if constexpr (Row::SGD) {
        // (the SGD update's blocks kernel has its own text; the lean form belongs to the `rest` entries, which take no optimizer)
        constexpr int L = Row::LPR;
        if (p.kernel == CDLRM_BWD_APPLY_BLOCKS_LEAN) launch_blocks<k_bwd_blocks_sgd<L, true, 1, 8>>(grid, a, s);
        else if (p.arange) launch_blocks<k_bwd_blocks_sgd<L, true>>(grid, a, s);
        else launch_blocks<k_bwd_blocks_sgd<L, false>>(grid, a, s);
    } else {
        if (p.arange) launch_blocks<k_bwd_blocks<Row, true>>(grid, a, s);
        else launch_blocks<k_bwd_blocks<Row, false>>(grid, a, s);
    }
    if constexpr (Row::SGD) launch_long<k_bwd_long_sgd<Row::LPR>>(dim3((unsigned)p.long_grid), a, s);
    else launch_long<k_bwd_long<Row>>(dim3((unsigned)p.long_grid), a, s);
}
template <int L>
static void bwd_apply_launch_lpr(const BwdApplyPlan& p, const BwdApplyArgs& a, hipStream_t s) {
    if (a.opt != CDLRM_EMB_OPT_ROWWISE_ADAGRAD) return bwd_apply_launch_row<SgdRow<L>>(p, a, s);
    // column chunks per lane: 1 up to D = 256 (LPR >= D4); 2 / 4 at LPR = 64 (bwd_apply has checked D <= 1024)
    if constexpr (L == 64) {
        const int nch = (int)cdiv(a.D4, L);
        if (nch > 2) return bwd_apply_launch_row<AdaRow<L, 4>>(p, a, s);
        if (nch == 2) return bwd_apply_launch_row<AdaRow<L, 2>>(p, a, s);
    }
    bwd_apply_launch_row<AdaRow<L, 1>>(p, a, s);
}
static int bwd_apply_launch(const BwdApplyPlan& p, const BwdApplyArgs& a, hipStream_t s) {
#define APPLY_CALL(L) bwd_apply_launch_lpr<L>(p, a, s)
    DISPATCH_LPR(p.lpr, APPLY_CALL)
#undef APPLY_CALL
    CDLRM_LAUNCH_CHECK();
    return 0;
}

// ---- argument checks shared by the launching calls and the route query (pointer and alignment checks: the launching calls' own) --
static int bwd_check_batch(int T, int64_t n) {
    CDLRM_REQUIRE(n < ((int64_t)1 << 31) && T < (1 << 20), "n < 2^31");
    return 0;
}
static int bwd_check_window(int T, int32_t nb, int64_t n, int32_t j0, int32_t count, int64_t batch_len, int64_t ld_w) {
    CDLRM_REQUIRE(nb >= 1 && n >= 1 && n < ((int64_t)1 << 31) && (int64_t)T * nb < 65536, "1 <= nb, T * nb < 65536, n < 2^31");
    CDLRM_REQUIRE(j0 >= 0 && count >= 1 && j0 + count <= nb, "0 <= j0, 1 <= count, j0 + count <= nb");
    CDLRM_REQUIRE(batch_len >= n && ld_w >= (int64_t)(nb - 1) * batch_len + n, "a batch's n slot ids lie inside its batch_len columns");
    return 0;
}

// ---- entry points: check, plan, launch -------------------------------------------------------------------------------------------
extern "C" int cdlrm_embbag_bwd_prepare(cdlrm_ctx* ctx, const int32_t* slots, int64_t n, void* work, void* stream) {
    CDLRM_REQUIRE(ctx && slots && work, "null argument");
    CDLRM_REQUIRE(((uintptr_t)work & 255) == 0, "work must be 256-byte aligned");
    const int rc = bwd_check_batch(ctx->T, n);
    if (rc) return rc;
    if (n == 0) return 0;
#ifdef CDLRM_DEV
    if (g_cdlrm_debug[6] & 2) return 0;     // development build (tools/ab_step.py --attr debug:6): what the step costs WITHOUT the slot sort
#endif
    return bwd_sort_launch(bwd_sort_plan(ctx->T, n), sort_bufs(work, bwd_layout(ctx->T, n, ctx->D)), slots, n, 1, n, 0, 1, 0,
                           (hipStream_t)stream);
}

extern "C" int cdlrm_embbag_bwd_prepare_window(cdlrm_ctx* ctx, const int32_t* wslots, int64_t ld_w, int64_t batch_len,
                                               int32_t nb, int64_t n, int32_t j0, int32_t count, void* sorted, void* stream) {
    CDLRM_REQUIRE(ctx && wslots && sorted, "null argument");
    CDLRM_REQUIRE(((uintptr_t)sorted & 255) == 0, "sorted must be 256-byte aligned");
    const int rc = bwd_check_window(ctx->T, nb, n, j0, count, batch_len, ld_w);
    if (rc) return rc;
    return bwd_sort_launch(bwd_sort_plan(ctx->T * count, n), sort_bufs(sorted, sorted_layout(ctx->T, nb, n)),
                           wslots + (int64_t)j0 * batch_len, n, count, ld_w, batch_len, nb, j0, (hipStream_t)stream);
}

extern "C" int cdlrm_embbag_bwd_sorted_views(cdlrm_ctx* ctx, void* sorted, int32_t nb, int64_t n, int32_t j,
                                             const uint64_t** keys, const int32_t** meta, const uint8_t** once) {
    CDLRM_REQUIRE(ctx && sorted && keys && meta && once && nb >= 1 && j >= 0 && j < nb && n >= 1, "bad argument");
    const SortedOffs v = sorted_offs(sorted_layout(ctx->T, nb, n), bwd_sort_plan(ctx->T, n), n, j);
    *keys = at<const uint64_t>(sorted, v.keys);
    *meta = at<const int32_t>(sorted, v.meta);
    *once = at<const uint8_t>(sorted, v.once);
    return 0;
}

extern "C" int cdlrm_embbag_bwd_once_flags(cdlrm_ctx* ctx, void* work, int64_t n, const uint8_t** once) {
    CDLRM_REQUIRE(ctx && work && once && n >= 1, "bad argument");
    *once = at<const uint8_t>(work, bwd_layout(ctx->T, n, ctx->D).once);
    return 0;
}

// sums + row updates over sorted lists: keys / meta / kstride / aux_phase as BwdApplyArgs has them, or keys == nullptr: the sort
// that cdlrm_embbag_bwd_prepare left in `work` itself; the scratch is `work`'s either way
static int bwd_apply(cdlrm_ctx* ctx, const int64_t* offsets, int64_t n, int64_t n_bags, int64_t ld_off, const float* grad,
                     int64_t ld_bag, int64_t ld_table, float lr, void* work, const uint64_t* keys, const int32_t* meta,
                     int64_t kstride, int aux_phase, uint8_t* touched, void* stream, int skip_once, int opt = CDLRM_EMB_OPT_SGD,
                     float eps = 0.f, float* state = nullptr, const int64_t* state_base = nullptr) {
    CDLRM_REQUIRE(ctx && grad && work, "null argument");
    CDLRM_REQUIRE(opt == CDLRM_EMB_OPT_SGD || opt == CDLRM_EMB_OPT_ROWWISE_ADAGRAD, "opt: CDLRM_EMB_OPT_*");
    if (opt != CDLRM_EMB_OPT_SGD) {
        CDLRM_REQUIRE(!skip_once, "the `rest` apply follows an SGD step of the once-only slots: it takes no optimizer");
        CDLRM_REQUIRE(state && state_base && eps > 0.f, "row-wise Adagrad needs its state, state_base and eps > 0");
        CDLRM_REQUIRE(ctx->tags, "cdlrm_ctx_bind_cache first");
        CDLRM_REQUIRE(ctx->D <= 1024, "row-wise Adagrad: dim <= 1024 (a lane holds its row's column chunks in registers)");
    }
    CDLRM_REQUIRE(ctx->weight, "cdlrm_ctx_bind_cache first");
    CDLRM_REQUIRE(((uintptr_t)grad & 15) == 0 && ld_bag % 4 == 0 && ld_table % 4 == 0 && ((uintptr_t)work & 255) == 0,
                  "aligned grad rows / work");
    CDLRM_REQUIRE(offsets != nullptr || n_bags == n, "Criteo layout needs n_bags == n");
    if (n == 0) return 0;
#ifdef CDLRM_DEV
    if (g_cdlrm_debug[6] & 1) return 0;     // development build: ... without the embedding update (an upper bound on what moving it buys)
#endif
    const BwdLayout l = bwd_layout(ctx->T, n, ctx->D);
    if (!keys) {
        const SortedOffs v = sorted_offs(l, bwd_sort_plan(ctx->T, n), n, 0);
        keys = at<const uint64_t>(work, v.keys);
        meta = at<const int32_t>(work, v.meta);
        kstride = n;
    }
    const BwdApplyArgs a = {ctx->d_tab, ctx->D / 4, reinterpret_cast<float4*>(ctx->weight), keys, meta, kstride, offsets, n, n_bags,
                            ld_off, grad, ld_bag, ld_table, lr, at<float4>(work, l.partials), l.pstride,
                            at<int64_t>(work, l.longlist), at<int32_t>(work, l.longcount), at<int32_t>(work, l.runend), touched,
                            (int64_t)ctx->aux * ctx->aux_phases, skip_once, ctx->ways, aux_phase * ctx->aux, opt,
                            {ctx->tags, state, state_base, eps}};
    return bwd_apply_launch(bwd_apply_plan(ctx->T, ctx->D, n, offsets != nullptr, skip_once != 0), a, (hipStream_t)stream);
}

extern "C" int cdlrm_embbag_bwd_apply(cdlrm_ctx* ctx, const int64_t* offsets, int64_t n, int64_t n_bags, int64_t ld_off,
                                      const float* grad, int64_t ld_bag, int64_t ld_table, float lr, void* work,
                                      uint8_t* touched, void* stream) {
    return bwd_apply(ctx, offsets, n, n_bags, ld_off, grad, ld_bag, ld_table, lr, work, nullptr, nullptr, 0, 0, touched, stream, 0);
}

// The apply behind cdlrm_gather_interact_bwd_sgd: slots the batch reads once were updated there (their gradient rows were
// never written); what is left are the runs of two and more lookups.
extern "C" int cdlrm_embbag_bwd_apply_rest(cdlrm_ctx* ctx, const int64_t* offsets, int64_t n, int64_t n_bags, int64_t ld_off,
                                           const float* grad, int64_t ld_bag, int64_t ld_table, float lr, void* work,
                                           uint8_t* touched, void* stream) {
    return bwd_apply(ctx, offsets, n, n_bags, ld_off, grad, ld_bag, ld_table, lr, work, nullptr, nullptr, 0, 0, touched, stream, 1);
}

// The apply over a window chunk's sorted lists (cdlrm_embbag_bwd_prepare_window; keys / meta: batch j's views, tstride = nb * n):
// no per-batch sort.  `work` only lends its scratch (partial sums, long-run list); its long-run counter must be zero -- every
// apply leaves it zero, a fresh buffer is zero-filled by the caller.  One lookup per bag (the Criteo layout).
extern "C" int cdlrm_embbag_bwd_apply_sorted(cdlrm_ctx* ctx, int64_t n, const float* grad, int64_t ld_bag, int64_t ld_table,
                                             float lr, void* work, const uint64_t* keys, const int32_t* meta, int64_t tstride,
                                             int32_t aux_phase, int32_t rest, uint8_t* touched, void* stream) {
    CDLRM_REQUIRE(ctx && keys && meta && tstride >= n, "null argument / tstride");
    CDLRM_REQUIRE(aux_phase >= 0 && aux_phase < (ctx->aux_phases > 0 ? ctx->aux_phases : 1), "aux_phase outside the geometry's aux_phases");
    return bwd_apply(ctx, nullptr, n, n, 0, grad, ld_bag, ld_table, lr, work, keys, meta, tstride, aux_phase, touched, stream,
                     rest ? 1 : 0);
}

// The two applies that take an optimizer: opt = CDLRM_EMB_OPT_SGD launches exactly the sibling's plan (state unused);
// CDLRM_EMB_OPT_ROWWISE_ADAGRAD the same plan's kernels with the AdaRow update.
extern "C" int cdlrm_embbag_bwd_apply_opt(cdlrm_ctx* ctx, const int64_t* offsets, int64_t n, int64_t n_bags, int64_t ld_off,
                                          const float* grad, int64_t ld_bag, int64_t ld_table, float lr, void* work,
                                          uint8_t* touched, int32_t opt, float eps, float* state, const int64_t* state_base,
                                          void* stream) {
    return bwd_apply(ctx, offsets, n, n_bags, ld_off, grad, ld_bag, ld_table, lr, work, nullptr, nullptr, 0, 0, touched, stream, 0,
                     opt, eps, state, state_base);
}
extern "C" int cdlrm_embbag_bwd_apply_sorted_opt(cdlrm_ctx* ctx, int64_t n, const float* grad, int64_t ld_bag, int64_t ld_table,
                                                 float lr, void* work, const uint64_t* keys, const int32_t* meta, int64_t tstride,
                                                 int32_t aux_phase, int32_t rest, uint8_t* touched, int32_t opt, float eps,
                                                 float* state, const int64_t* state_base, void* stream) {
    CDLRM_REQUIRE(ctx && keys && meta && tstride >= n, "null argument / tstride");
    CDLRM_REQUIRE(aux_phase >= 0 && aux_phase < (ctx->aux_phases > 0 ? ctx->aux_phases : 1), "aux_phase outside the geometry's aux_phases");
    return bwd_apply(ctx, nullptr, n, n, 0, grad, ld_bag, ld_table, lr, work, keys, meta, tstride, aux_phase, touched, stream,
                     rest ? 1 : 0, opt, eps, state, state_base);
}

extern "C" int cdlrm_embbag_bwd_sgd(cdlrm_ctx* ctx, const int32_t* slots, const int64_t* offsets, int64_t n,
                                    int64_t n_bags, int64_t ld_off, const float* grad, int64_t ld_bag,
                                    int64_t ld_table, float lr, void* work, uint8_t* touched, void* stream) {
    int rc = cdlrm_embbag_bwd_prepare(ctx, slots, n, work, stream);
    if (rc) return rc;
    return cdlrm_embbag_bwd_apply(ctx, offsets, n, n_bags, ld_off, grad, ld_bag, ld_table, lr, work, touched, stream);
}

// The route query: the checks, plans and layouts of the calls above on a geometry of num_tables x dim, copied out.  No context,
// device or buffer exists; the offsets are relative to the start of `work` (window entries: of `sorted`).
extern "C" int cdlrm_embbag_bwd_route(int32_t num_tables, int32_t dim, int64_t n, int32_t has_offsets, int32_t entry, int32_t nb,
                                      int32_t j0, int32_t count, cdlrm_emb_bwd_route* out) {
    CDLRM_REQUIRE(out && num_tables >= 1 && dim >= 4 && dim % 4 == 0, "bad argument");
    CDLRM_REQUIRE(entry >= CDLRM_BWD_ENTRY_APPLY && entry <= CDLRM_BWD_ENTRY_SORTED_REST, "entry: CDLRM_BWD_ENTRY_*");
    const bool window = entry >= CDLRM_BWD_ENTRY_SORTED;
    CDLRM_REQUIRE(!window || !has_offsets, "the window-sorted path has one lookup per bag");     // (_apply_sorted takes no offsets)
    memset(out, 0, sizeof(*out));
    const int rc = window ? bwd_check_window(num_tables, nb, n, j0, count, n, (int64_t)nb * n) : bwd_check_batch(num_tables, n);
    if (rc || n == 0) return rc;
    const BwdSortPlan sp = bwd_sort_plan(window ? num_tables * count : num_tables, n);
    const BwdApplyPlan ap = bwd_apply_plan(num_tables, dim, n, has_offsets != 0,
                                           entry == CDLRM_BWD_ENTRY_REST || entry == CDLRM_BWD_ENTRY_SORTED_REST);
    // (the window entries: batch j0's lists, as _sorted_views gives them and _apply_sorted is handed them)
    const SortedOffs v = window ? sorted_offs(sorted_layout(num_tables, nb, n), sp, n, j0)
                                : sorted_offs(bwd_layout(num_tables, n, dim), sp, n, 0);
    out->sort_chunk = sp.chunk; out->sort_e = sp.E; out->sort_chunks = sp.nchunks; out->merge_passes = sp.passes;
    out->seg_meta = sp.seg_meta; out->keys_in_b = sp.keys_in_b;
    out->apply = ap.kernel; out->arange = ap.arange; out->lpr = ap.lpr;
    out->apply_grid_x = ap.grid_x; out->apply_grid_y = ap.grid_y; out->long_grid = ap.long_grid;
    out->keys_off = (int64_t)v.keys; out->meta_off = (int64_t)v.meta; out->once_off = (int64_t)v.once;
    out->apply_keys_off = (int64_t)v.keys;
    return 0;
}
