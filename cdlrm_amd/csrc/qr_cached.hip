// K16: the quotient-remainder trick ON the cached training step.
// The cache holds QUOTIENT rows keyed by q; the remainder tables Wr [T, c, D] live whole in HBM (104 KB at c4's shape: they
// stay in L2).  One lookup per bag (the Criteo layout):
//   split     idx -> q = (int64)((float)idx / (float)c) clamped to rows_q - 1 for an in-range idx, r = idx % c
//   forward   E[b, k] = row(slot[b, k]) (*|+) Wr[k][r[b, k]], straight into the interaction's feature rows
//   backward  dfeat[b, 1 + k] <- g * Wr[k][r] (mult; add: left alone) -- what the sparse-SGD path then applies to the cache
//             rows -- and gWr[k][r] = sum_b g * row (mult) / sum_b g (add), WITHOUT float atomics: a workgroup owns a fixed
//             range of bags of one table, its lane groups add in ascending bag order into LDS, the groups are added in
//             ascending order into one [c, D] partial in caller-owned scratch; `finish` adds the partials in ascending order
//             and applies Wr -= lr * gWr.  The partition depends on (T, n, D, c) only: two calls give the same bits.
// HBM-bound, 16 B per lane.
#include "common.h"

#define QRC_MAX_C 16
#define QRC_BAGS 128        // bags of one table a backward workgroup owns

__device__ __forceinline__ int64_t qrc_quotient(int64_t idx, int c) {
    // torch: int64 tensor / python int -> true_divide in float32, then .long() (tricks/qr_embedding_bag.py; kept on purpose)
    return (int64_t)((float)idx / (float)c);
}

// q may alias idx: every thread reads its own element before it writes it (no __restrict__ on the two)
__global__ void __launch_bounds__(256) k_qr_split(const int64_t* idx, int64_t n, int64_t ld_idx,
                                                  const int32_t* __restrict__ collisions,
                                                  const int64_t* __restrict__ table_rows, int64_t* q, int64_t ld_q,
                                                  uint8_t* __restrict__ r, int64_t ld_r, int* err) {
    const int k = blockIdx.y;
    const int c = collisions[k];
    const int64_t rows = table_rows[k];
    const int64_t rows_q = c > 0 ? (rows + c - 1) / c : rows;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t v = idx[(int64_t)k * ld_idx + i];
        int64_t qq = 0;
        int rr = 0;
        if (v < 0 || v >= rows) {
            atomicOr(err, 1);
        } else if (c == 0) {
            qq = v;
        } else {
            qq = qrc_quotient(v, c);
            if (qq >= rows_q) qq = rows_q - 1;      // float32 quotient of an in-range id above 2^24: at most one row too far
            rr = (int)(v % c);
        }
        q[(int64_t)k * ld_q + i] = qq;
        r[(int64_t)k * ld_r + i] = (uint8_t)rr;
    }
}

__device__ __forceinline__ float4 qrc_compose(float4 x, float4 y, int op) {
    return op == 0 ? make_float4(x.x * y.x, x.y * y.y, x.z * y.z, x.w * y.w)
                   : make_float4(x.x + y.x, x.y + y.y, x.z + y.z, x.w + y.w);
}

// forward: a lane group (LPR lanes x 16 B) per bag, U bags in flight per group; a persistent grid walks (table, bag chunk)
// items and loads the NEXT item's slot ids and remainders before the current item's rows (as k_embbag_fwd_arange_p does: one
// memory latency per item instead of two).  Loads are unpredicated (tail bags clamp to the last bag), only the stores are masked.
template <int LPR, int U>
__global__ void __launch_bounds__(256) k_qr_cached_fwd(const TableDesc* __restrict__ tab, int T, int D4,
                                                       const float4* __restrict__ weight,
                                                       const int32_t* __restrict__ slots, const uint8_t* __restrict__ rem,
                                                       int64_t ld_r, const float4* __restrict__ Wr,
                                                       const int32_t* __restrict__ collisions, int cmax, int op, int64_t n,
                                                       float* __restrict__ out, int64_t ld_bag, int64_t ld_table) {
    const int cl = threadIdx.x % LPR;
    const int gpb = blockDim.x / LPR;
    const int gid = threadIdx.x / LPR;
    const int64_t chunks = cdiv_dev(n, (int64_t)gpb * U);
    const int64_t total = chunks * T;
    int64_t w = blockIdx.x;
    if (w >= total) return;
    int32_t s[U];
    int rr[U];
    {
        const int t = (int)(w / chunks);
        const int64_t b0 = ((w % chunks) * gpb + gid) * U;
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t b = min(b0 + u, n - 1);
            s[u] = slots[(int64_t)t * n + b];
            rr[u] = rem[(int64_t)t * ld_r + b];
        }
    }
    while (true) {
        const int t = (int)(w / chunks);
        const int64_t b0 = ((w % chunks) * gpb + gid) * U;
        const int64_t wn = w + gridDim.x;
        int32_t sn[U] = {};
        int rn[U] = {};
        if (wn < total) {
            const int tn = (int)(wn / chunks);
            const int64_t bn = ((wn % chunks) * gpb + gid) * U;
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int64_t b = min(bn + u, n - 1);
                sn[u] = slots[(int64_t)tn * n + b];
                rn[u] = rem[(int64_t)tn * ld_r + b];
            }
        }
        const int c = collisions[t];
        const int64_t row_base = tab[t].row_base;
        const float4* wr = Wr + (int64_t)t * cmax * D4;
        float* o = out + (int64_t)t * ld_table;
#pragma unroll
        for (int u = 0; u < U; ++u) rr[u] = min(rr[u], cmax - 1);        // (never outside the remainder table)
        for (int cc = cl; cc < D4; cc += LPR) {
            float4 v[U], y[U];
#pragma unroll
            for (int u = 0; u < U; ++u) v[u] = weight[(row_base + s[u]) * D4 + cc];
            if (c > 0) {
#pragma unroll
                for (int u = 0; u < U; ++u) y[u] = wr[(int64_t)rr[u] * D4 + cc];
#pragma unroll
                for (int u = 0; u < U; ++u) v[u] = qrc_compose(v[u], y[u], op);
            }
#pragma unroll
            for (int u = 0; u < U; ++u)
                if (b0 + u < n) *reinterpret_cast<float4*>(o + (b0 + u) * ld_bag + cc * 4) = v[u];
        }
        if (wn >= total) break;
        w = wn;
        for (int u = 0; u < U; ++u) { s[u] = sn[u]; rr[u] = rn[u]; }
    }
}

// backward: grid (chunks of QRC_BAGS bags, T).  LDS: [gpb][c][D4] float4 accumulators, one column of it per thread.
template <int LPR, int U>
__global__ void __launch_bounds__(256) k_qr_cached_bwd(const TableDesc* __restrict__ tab, int D4,
                                                       const float4* __restrict__ weight,
                                                       const int32_t* __restrict__ slots, const uint8_t* __restrict__ rem,
                                                       int64_t ld_r, const float4* __restrict__ Wr,
                                                       const int32_t* __restrict__ collisions, int cmax, int op, int64_t n,
                                                       float* __restrict__ grad, int64_t ld_bag, int64_t ld_table,
                                                       float4* __restrict__ partial) {
    extern __shared__ float4 qrc_acc[];
    const int t = blockIdx.y;
    const int c = collisions[t];
    if (c == 0) return;          // a plain table: its gradient rows are the cache rows' already (block-uniform exit)
    const int cl = threadIdx.x % LPR;
    const int gpb = blockDim.x / LPR;
    const int gid = threadIdx.x / LPR;
    const int64_t row_base = tab[t].row_base;
    float4* mine = qrc_acc + (int64_t)gid * cmax * D4;
    for (int k = 0; k < cmax; ++k)
        for (int cc = cl; cc < D4; cc += LPR) mine[k * D4 + cc] = make_float4(0.f, 0.f, 0.f, 0.f);
    const int64_t lo = (int64_t)blockIdx.x * QRC_BAGS;
    const int64_t hi = min(lo + QRC_BAGS, n);
    const float4* wr = Wr + (int64_t)t * cmax * D4;
    float* gt = grad + (int64_t)t * ld_table;
    // group gid owns bags lo + gid, lo + gid + gpb, ...: ascending, U of them in flight
    for (int64_t b0 = lo + gid; b0 < hi; b0 += (int64_t)gpb * U) {
        int32_t s[U];
        int rr[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t b = min(b0 + (int64_t)u * gpb, hi - 1);
            s[u] = slots[(int64_t)t * n + b];
            rr[u] = min((int)rem[(int64_t)t * ld_r + b], cmax - 1);
        }
        for (int cc = cl; cc < D4; cc += LPR) {
            float4 g[U], x[U], y[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int64_t b = min(b0 + (int64_t)u * gpb, hi - 1);
                g[u] = *reinterpret_cast<const float4*>(gt + b * ld_bag + cc * 4);
            }
            if (op == 0) {
#pragma unroll
                for (int u = 0; u < U; ++u) x[u] = weight[(row_base + s[u]) * D4 + cc];
#pragma unroll
                for (int u = 0; u < U; ++u) y[u] = wr[(int64_t)rr[u] * D4 + cc];
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int64_t b = b0 + (int64_t)u * gpb;
                if (b < hi) {
                    float4 d = g[u];
                    if (op == 0) {
                        d = make_float4(g[u].x * x[u].x, g[u].y * x[u].y, g[u].z * x[u].z, g[u].w * x[u].w);
                        *reinterpret_cast<float4*>(gt + b * ld_bag + cc * 4) =
                            make_float4(g[u].x * y[u].x, g[u].y * y[u].y, g[u].z * y[u].z, g[u].w * y[u].w);
                    }
                    float4 a = mine[rr[u] * D4 + cc];
                    a.x += d.x; a.y += d.y; a.z += d.z; a.w += d.w;
                    mine[rr[u] * D4 + cc] = a;
                }
            }
        }
    }
    __syncthreads();
    // the groups' sums in ascending group order -> this workgroup's [c, D4] partial
    float4* p = partial + ((int64_t)t * gridDim.x + blockIdx.x) * cmax * D4;
    for (int e = threadIdx.x; e < c * D4; e += blockDim.x) {
        float4 a = qrc_acc[e];
        for (int g2 = 1; g2 < gpb; ++g2) {
            const float4 v = qrc_acc[(int64_t)g2 * cmax * D4 + e];
            a.x += v.x; a.y += v.y; a.z += v.z; a.w += v.w;
        }
        p[e] = a;
    }
}

// finish: gWr[t][k] = the partials in ascending chunk order; Wr -= lr * gWr
__global__ void __launch_bounds__(256) k_qr_cached_finish(const int32_t* __restrict__ collisions, int T, int cmax, int D4,
                                                          int64_t chunks, const float4* __restrict__ partial, float lr,
                                                          float4* __restrict__ Wr, float4* __restrict__ gWr) {
    const int64_t per = (int64_t)cmax * D4;
    const int64_t total = (int64_t)T * per;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
        const int t = (int)(e / per);
        const int64_t i = e % per;
        if (i >= (int64_t)collisions[t] * D4) continue;
        const float4* p = partial + (int64_t)t * chunks * per + i;
        float4 a = p[0];
#pragma unroll 8
        for (int64_t ch = 1; ch < chunks; ++ch) {       // (the loads are independent: several in flight, the adds in order)
            const float4 v = p[ch * per];
            a.x += v.x; a.y += v.y; a.z += v.z; a.w += v.w;
        }
        if (gWr) gWr[e] = a;
        float4 w = Wr[e];
        w.x -= lr * a.x; w.y -= lr * a.y; w.z -= lr * a.z; w.w -= lr * a.w;
        Wr[e] = w;
    }
}

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
extern "C" int cdlrm_qr_split(cdlrm_ctx* ctx, const int64_t* idx, int64_t n, int64_t ld_idx, const int32_t* collisions,
                              const int64_t* table_rows, int64_t* q, int64_t ld_q, uint8_t* r, int64_t ld_r, void* stream) {
    CDLRM_CLEAR_STALE();
    CDLRM_REQUIRE(ctx && idx && collisions && table_rows && q && r, "null argument");
    CDLRM_REQUIRE(n >= 0 && ld_idx >= n && ld_q >= n && ld_r >= n, "bad n / pitch");
    if (n == 0) return 0;
    int64_t gx = cdiv(n, 256);
    if (gx > 4096) gx = 4096;
    hipLaunchKernelGGL(k_qr_split, dim3((unsigned)gx, (unsigned)ctx->T), dim3(256), 0, (hipStream_t)stream, idx, n, ld_idx,
                       collisions, table_rows, q, ld_q, r, ld_r, ctx->d_err);
    CDLRM_LAUNCH_CHECK();
    return 0;
}

static int qrc_check(cdlrm_ctx* ctx, int32_t c, int32_t op, int64_t n, int64_t ld_r, const void* rows, int64_t ld_bag,
                     int64_t ld_table) {
    CDLRM_REQUIRE(ctx->weight, "cdlrm_ctx_bind_cache first");
    CDLRM_REQUIRE(c >= 2 && c <= QRC_MAX_C, "collisions: 2 .. 16");
    CDLRM_REQUIRE(op == 0 || op == 1, "operation: 0 = mult, 1 = add (concat changes the row width)");
    CDLRM_REQUIRE(n >= 0 && ld_r >= n, "bad n / remainder pitch");
    CDLRM_REQUIRE(((uintptr_t)rows & 15) == 0 && ld_bag % 4 == 0 && ld_table % 4 == 0, "16-byte aligned feature rows");
    return 0;
}

extern "C" int cdlrm_qr_cached_fwd(cdlrm_ctx* ctx, const int32_t* slots, const uint8_t* r, int64_t ld_r, const float* Wr,
                                   const int32_t* collisions, int32_t c, int32_t op, int64_t n, float* out, int64_t ld_bag,
                                   int64_t ld_table, void* stream) {
    CDLRM_CLEAR_STALE();
    CDLRM_REQUIRE(ctx && slots && r && Wr && collisions && out, "null argument");
    CDLRM_REQUIRE(((uintptr_t)Wr & 15) == 0, "16-byte aligned remainder tables");
    if (int rc = qrc_check(ctx, c, op, n, ld_r, out, ld_bag, ld_table)) return rc;
    if (n == 0) return 0;
    const int D4 = ctx->D / 4;
    const int lpr = lanes_per_row(D4);
    const int gpb = 256 / lpr;
    constexpr int U = 4;
    int64_t gx = cdiv(n, (int64_t)gpb * U) * ctx->T;
    if (gx > 4096) gx = 4096;
#define QRCF(L)                                                                                                           \
    hipLaunchKernelGGL((k_qr_cached_fwd<L, U>), dim3((unsigned)gx), dim3(256), 0, (hipStream_t)stream, ctx->d_tab, ctx->T, D4, \
                       reinterpret_cast<const float4*>(ctx->weight), slots, r, ld_r, reinterpret_cast<const float4*>(Wr),  \
                       collisions, (int)c, (int)op, n, out, ld_bag, ld_table)
    DISPATCH_LPR(lpr, QRCF)
#undef QRCF
    CDLRM_LAUNCH_CHECK();
    return 0;
}

extern "C" uint64_t cdlrm_qr_cached_bwd_work_bytes(int32_t num_tables, int64_t n, int32_t dim, int32_t c) {
    if (num_tables <= 0 || n <= 0 || dim <= 0 || c <= 0) return 0;
    return (uint64_t)num_tables * (uint64_t)cdiv(n, QRC_BAGS) * (uint64_t)c * (uint64_t)dim * sizeof(float);
}

extern "C" int cdlrm_qr_cached_bwd(cdlrm_ctx* ctx, const int32_t* slots, const uint8_t* r, int64_t ld_r, const float* Wr,
                                   const int32_t* collisions, int32_t c, int32_t op, int64_t n, float* grad, int64_t ld_bag,
                                   int64_t ld_table, void* work, void* stream) {
    CDLRM_CLEAR_STALE();
    CDLRM_REQUIRE(ctx && slots && r && Wr && collisions && grad && work, "null argument");
    CDLRM_REQUIRE((((uintptr_t)Wr | (uintptr_t)work) & 15) == 0, "16-byte aligned remainder tables / scratch");
    if (int rc = qrc_check(ctx, c, op, n, ld_r, grad, ld_bag, ld_table)) return rc;
    if (n == 0) return 0;
    const int D4 = ctx->D / 4;
    const int lpr = lanes_per_row(D4);
    const int gpb = 256 / lpr;
    const size_t lds = (size_t)gpb * c * D4 * sizeof(float4);
    CDLRM_REQUIRE(lds <= 65536, "remainder accumulators beyond 64 KB of LDS (dim * collisions too large)");
    constexpr int U = 4;
    const dim3 grid((unsigned)cdiv(n, QRC_BAGS), (unsigned)ctx->T);
#define QRCB(L)                                                                                                          \
    hipLaunchKernelGGL((k_qr_cached_bwd<L, U>), grid, dim3(256), lds, (hipStream_t)stream, ctx->d_tab, D4,                  \
                       reinterpret_cast<const float4*>(ctx->weight), slots, r, ld_r, reinterpret_cast<const float4*>(Wr), \
                       collisions, (int)c, (int)op, n, grad, ld_bag, ld_table, reinterpret_cast<float4*>(work))
    DISPATCH_LPR(lpr, QRCB)
#undef QRCB
    CDLRM_LAUNCH_CHECK();
    return 0;
}

extern "C" int cdlrm_qr_cached_bwd_finish(cdlrm_ctx* ctx, const int32_t* collisions, int32_t c, int64_t n, const void* work,
                                          float lr, float* Wr, float* gWr, void* stream) {
    CDLRM_CLEAR_STALE();
    CDLRM_REQUIRE(ctx && collisions && work && Wr, "null argument");
    CDLRM_REQUIRE(c >= 2 && c <= QRC_MAX_C && n >= 0, "collisions: 2 .. 16");
    CDLRM_REQUIRE((((uintptr_t)Wr | (uintptr_t)work | (uintptr_t)gWr) & 15) == 0, "16-byte aligned remainder tables / scratch");
    if (n == 0) return 0;
    const int D4 = ctx->D / 4;
    const int64_t total = (int64_t)ctx->T * c * D4;
    hipLaunchKernelGGL(k_qr_cached_finish, dim3((unsigned)cdiv(total, 256)), dim3(256), 0, (hipStream_t)stream, collisions,
                       ctx->T, (int)c, D4, cdiv(n, QRC_BAGS), reinterpret_cast<const float4*>(work), lr,
                       reinterpret_cast<float4*>(Wr), reinterpret_cast<float4*>(gWr));
    CDLRM_LAUNCH_CHECK();
    return 0;
}
