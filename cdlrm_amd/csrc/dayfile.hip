// Batches of the pre-processed Criteo day files, cut on the device a look-ahead window per launch
// (cdlrm_amd/data_loader_terabyte.py: DeviceDayLoader).
//
// The reference transforms every batch on one host thread (data_loader_terabyte.py:68-87: `x_cat % max_ind_range`, int32 ->
// float, + 1, torch.log, int32 -> int64, X_cat^T as a strided view) and the trainer uploads the result step by step
// (main_no_ddp.py:388-391).  Here the RAW rows of a window go to HBM once and one launch per file segment writes the window's
// (X, lS_i, T) in the layout the synthetic front end hands out: lS_i as columns of an int64 [n_cat, L * B] rectangle, X and T
// as rows of [L * B, n_dense] / [L * B, 1].
//
// X and T keep the day file's row-major order: they are flat elementwise passes.  lS_i is a transpose with a widening store:
// a workgroup reads its tile of samples flat and coalesced (16-byte loads between a scalar head and tail), stages it in LDS at
// a sample stride padded to an ODD number of dwords (26 dwords per sample would put lanes t and t + 16 of a ds_read_b32 on
// one bank: gcd(26, 32) = 2), and every wave then stores 64 consecutive int64 (512 B) of one table's row.  160 B read and
// 264 B written per sample at 13 / 26 features: the yardstick is HBM bandwidth.
//
// k_rows_window (below) is the same cut for rows picked by an order from arrays that stay in HBM (the processed Criteo file,
// cdlrm_amd/data_loader_processed.py: DeviceProcessedLoader); both kernels share dayfile_index / dayfile_dense.
#include "common.h"

#define DAYFILE_TILE 256          // samples per workgroup = threads per workgroup
#define DAYFILE_MAX_CAT 60        // (n_cat | 1) * DAYFILE_TILE dwords of LDS <= 64 KiB

// numpy's floor-mod (`x_cat % max_ind_range`, data_loader_terabyte.py:70-71): the result has the divisor's sign
__device__ __forceinline__ int64_t dayfile_index(int32_t v, int64_t m) {
    if (m <= 0) return (int64_t)v;
    if (m > 0x7fffffffll)               // wider than any int32: only a negative entry changes
        return v < 0 ? (int64_t)v + m : (int64_t)v;
    int32_t r = v % (int32_t)m;
    if (r < 0) r += (int32_t)m;
    return (int64_t)r;
}

// The reference's order of operations (data_loader_terabyte.py:73: torch.log(torch.tensor(x_int, dtype=torch.float) + 1)):
// int32 -> fp32 rounds first (values above 2^24), the + 1 is an fp32 add.  The logarithm itself is taken in double and rounded
// once: at most half an fp32 ulp (and a double's rounding) from the true value, whatever the toolchain's logf keeps.
__device__ __forceinline__ float dayfile_dense(int32_t v) {
    const float f = (float)v + 1.0f;
    return (float)log((double)f);
}

// NC_T > 0: the number of categorical features at compile time (division by it folds to a multiply); 0: nc at run time
template <int NC_T>
__global__ void __launch_bounds__(DAYFILE_TILE) k_dayfile_window(const int32_t* __restrict__ x_int, const int32_t* __restrict__ x_cat,
                                                                 const int32_t* __restrict__ y, int64_t n, int nd, int nc_rt,
                                                                 int64_t max_ind_range, float* __restrict__ X,
                                                                 int64_t* __restrict__ lS_i, int64_t pitch, int64_t col0,
                                                                 float* __restrict__ T) {
    extern __shared__ __attribute__((aligned(16))) int32_t tile[];
    const int nc = NC_T ? NC_T : nc_rt;
    const int S = nc | 1;                                        // odd sample stride, in dwords
    const int tid = threadIdx.x;
    const int64_t t0 = (int64_t)blockIdx.x * DAYFILE_TILE;       // first sample of this tile
    const int nt = (int)((n - t0) < DAYFILE_TILE ? (n - t0) : DAYFILE_TILE);

    // ---- categorical features: flat read -> LDS
    {
        const int32_t* src = x_cat + t0 * nc;
        const int total = nt * nc;
        int head = (int)(((16 - ((uintptr_t)src & 15)) & 15) >> 2);      // dwords up to the first 16-byte boundary
        if (head > total) head = total;
        const int nvec = (total - head) >> 2;
        const int tail0 = head + (nvec << 2);
        if (tid < head) tile[tid + (tid / nc) * (S - nc)] = src[tid];
        for (int v = tid; v < nvec; v += DAYFILE_TILE) {
            const int f = head + (v << 2);
            const int4 q = *reinterpret_cast<const int4*>(src + f);
            int s = f / nc, k = f - s * nc;
            const int32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                tile[s * S + k] = w[e];
                if (++k == nc) { k = 0; ++s; }
            }
        }
        if (tid < total - tail0) {
            const int f = tail0 + tid;
            tile[f + (f / nc) * (S - nc)] = src[f];
        }
    }
    __syncthreads();
    // ---- LDS -> one table row at a time: lane t holds sample t0 + t, a wave stores 64 consecutive int64
    if (tid < nt) {
        const int32_t* mine = tile + tid * S;
        int64_t* dst = lS_i + col0 + t0 + tid;
        if (NC_T) {
#pragma unroll
            for (int k = 0; k < (NC_T ? NC_T : 1); ++k) dst[(int64_t)k * pitch] = dayfile_index(mine[k], max_ind_range);
        } else {
            for (int k = 0; k < nc; ++k) dst[(int64_t)k * pitch] = dayfile_index(mine[k], max_ind_range);
        }
        T[col0 + t0 + tid] = (float)y[t0 + tid];
    }
    // ---- dense features: source and destination are both row-major, a flat elementwise pass over the tile's nt * nd values
    {
        const int32_t* src = x_int + t0 * nd;
        float* dst = X + (col0 + t0) * nd;
        const int total = nt * nd;
        if ((((uintptr_t)src ^ (uintptr_t)dst) & 15) == 0) {     // both reach a 16-byte boundary together: vector body
            int head = (int)(((16 - ((uintptr_t)src & 15)) & 15) >> 2);
            if (head > total) head = total;
            const int nvec = (total - head) >> 2;
            const int tail0 = head + (nvec << 2);
            if (tid < head) dst[tid] = dayfile_dense(src[tid]);
            for (int v = tid; v < nvec; v += DAYFILE_TILE) {
                const int f = head + (v << 2);
                const int4 q = *reinterpret_cast<const int4*>(src + f);
                float4 o;
                o.x = dayfile_dense(q.x); o.y = dayfile_dense(q.y); o.z = dayfile_dense(q.z); o.w = dayfile_dense(q.w);
                *reinterpret_cast<float4*>(dst + f) = o;
            }
            if (tid < total - tail0) dst[tail0 + tid] = dayfile_dense(src[tail0 + tid]);
        } else {
            for (int f = tid; f < total; f += DAYFILE_TILE) dst[f] = dayfile_dense(src[f]);
        }
    }
}

extern "C" int cdlrm_dayfile_tile(void) { return DAYFILE_TILE; }

extern "C" int cdlrm_dayfile_window(const int32_t* x_int, const int32_t* x_cat, const int32_t* y, int64_t n, int32_t n_dense,
                                    int32_t n_cat, int64_t max_ind_range, float* X, int64_t* lS_i, int64_t lS_i_pitch,
                                    int64_t col0, float* T, void* stream) {
    CDLRM_REQUIRE(n >= 0 && col0 >= 0 && lS_i_pitch >= col0 + n, "the segment must lie inside the window rectangle's row");
    CDLRM_REQUIRE(n_dense >= 1 && n_cat >= 1 && n_cat <= DAYFILE_MAX_CAT, "1 .. 60 categorical features (a tile's LDS image)");
    if (n == 0) return 0;
    CDLRM_REQUIRE(x_int && x_cat && y && X && lS_i && T, "null buffer");
    CDLRM_REQUIRE(((uintptr_t)x_int & 3) == 0 && ((uintptr_t)x_cat & 3) == 0 && ((uintptr_t)y & 3) == 0 &&
                  ((uintptr_t)X & 3) == 0 && ((uintptr_t)T & 3) == 0 && ((uintptr_t)lS_i & 7) == 0, "misaligned buffer");
    const dim3 grid((unsigned)cdiv(n, DAYFILE_TILE)), block(DAYFILE_TILE);
    const size_t lds = (size_t)(n_cat | 1) * DAYFILE_TILE * sizeof(int32_t);
    if (n_cat == 26)
        hipLaunchKernelGGL(k_dayfile_window<26>, grid, block, lds, (hipStream_t)stream, x_int, x_cat, y, n, (int)n_dense, 26,
                           max_ind_range, X, lS_i, lS_i_pitch, col0, T);
    else
        hipLaunchKernelGGL(k_dayfile_window<0>, grid, block, lds, (hipStream_t)stream, x_int, x_cat, y, n, (int)n_dense,
                           (int)n_cat, max_ind_range, X, lS_i, lS_i_pitch, col0, T);
    CDLRM_LAUNCH_CHECK();
    return 0;
}

// ---- the permuted cut: rows of the processed Criteo file, resident in HBM, picked by an order (DeviceProcessedLoader)
//
// Sample i of the piece is row order[i] of x_int / x_cat / y.  The outputs, the LDS image and the store phase are
// k_dayfile_window's; only the reads differ.  A row is short and lies anywhere (104 B of x_cat, 52 B of x_int, in arrays of
// several GB), so lanes SHARE a row's loads: the tile's nt * U load units are dealt to the threads flat, unit f = (sample f / U,
// piece f % U) -- at 26 features 13 lanes read the 13 8-byte halves of one row's two lines, 64 lanes cover five rows, and no
// lane walks a row.  8-byte units when every row starts on an 8-byte boundary (an even feature count and an 8-byte aligned
// array), dwords otherwise.  The tile's slice of the order is staged in LDS first (one coalesced 2 KiB read per workgroup).
// Every row address is formed in 64 bits: row * 104 B passes 2^32 at 41.3 M rows.
template <int NC_T>
__global__ void __launch_bounds__(DAYFILE_TILE) k_rows_window(const int32_t* __restrict__ x_int, const int32_t* __restrict__ x_cat,
                                                              const int32_t* __restrict__ y, const int64_t* __restrict__ order,
                                                              int64_t n, int nd, int nc_rt, int pairs, int64_t max_ind_range,
                                                              float* __restrict__ X, int64_t* __restrict__ lS_i, int64_t pitch,
                                                              int64_t col0, float* __restrict__ T) {
    extern __shared__ __attribute__((aligned(16))) int32_t tile[];
    const int nc = NC_T ? NC_T : nc_rt;
    const int S = nc | 1;                                        // odd sample stride, in dwords
    int64_t* rows = reinterpret_cast<int64_t*>(tile + S * DAYFILE_TILE);        // behind the image: S KiB, 8-byte aligned
    const int tid = threadIdx.x;
    const int64_t t0 = (int64_t)blockIdx.x * DAYFILE_TILE;       // first sample of this tile
    const int nt = (int)((n - t0) < DAYFILE_TILE ? (n - t0) : DAYFILE_TILE);

    if (tid < nt) rows[tid] = order[t0 + tid];
    __syncthreads();
    // ---- categorical features: shared row reads -> LDS
    if (pairs) {
        const int U = nc >> 1;                                   // 8-byte units per row
        const int total = nt * U;
        for (int f = tid; f < total; f += DAYFILE_TILE) {
            const int s = f / U, u = f - s * U;
            const int2 q = *reinterpret_cast<const int2*>(x_cat + rows[s] * (int64_t)nc + 2 * u);
            tile[s * S + 2 * u] = q.x;
            tile[s * S + 2 * u + 1] = q.y;
        }
    } else {
        const int total = nt * nc;
        for (int f = tid; f < total; f += DAYFILE_TILE) {
            const int s = f / nc, k = f - s * nc;
            tile[s * S + k] = x_cat[rows[s] * (int64_t)nc + k];
        }
    }
    __syncthreads();
    // ---- LDS -> one table row at a time: lane t holds sample t0 + t, a wave stores 64 consecutive int64
    if (tid < nt) {
        const int32_t* mine = tile + tid * S;
        int64_t* dst = lS_i + col0 + t0 + tid;
        if (NC_T) {
#pragma unroll
            for (int k = 0; k < (NC_T ? NC_T : 1); ++k) dst[(int64_t)k * pitch] = dayfile_index(mine[k], max_ind_range);
        } else {
            for (int k = 0; k < nc; ++k) dst[(int64_t)k * pitch] = dayfile_index(mine[k], max_ind_range);
        }
        T[col0 + t0 + tid] = (float)y[rows[tid]];
    }
    // ---- dense features: the destination is flat (the tile's nt * nd values in a row), a source row is shared by nd lanes
    {
        float* dst = X + (col0 + t0) * nd;
        const int total = nt * nd;
        for (int f = tid; f < total; f += DAYFILE_TILE) {
            const int s = f / nd, k = f - s * nd;
            dst[f] = dayfile_dense(x_int[rows[s] * (int64_t)nd + k]);
        }
    }
}

extern "C" int cdlrm_rows_tile(void) { return DAYFILE_TILE; }

extern "C" int cdlrm_rows_window(const int32_t* x_int, const int32_t* x_cat, const int32_t* y, int64_t n_rows,
                                 const int64_t* order, int64_t n, int32_t n_dense, int32_t n_cat, int64_t max_ind_range, float* X,
                                 int64_t* lS_i, int64_t lS_i_pitch, int64_t col0, float* T, void* stream) {
    CDLRM_REQUIRE(n >= 0 && col0 >= 0 && lS_i_pitch >= col0 + n, "the piece must lie inside the window rectangle's row");
    CDLRM_REQUIRE(n_dense >= 1 && n_cat >= 1 && n_cat <= DAYFILE_MAX_CAT, "1 .. 60 categorical features (a tile's LDS image)");
    CDLRM_REQUIRE(n_rows >= 1, "no resident rows to pick from");
    if (n == 0) return 0;
    CDLRM_REQUIRE(x_int && x_cat && y && order && X && lS_i && T, "null buffer");
    CDLRM_REQUIRE(((uintptr_t)x_int & 3) == 0 && ((uintptr_t)x_cat & 3) == 0 && ((uintptr_t)y & 3) == 0 &&
                  ((uintptr_t)X & 3) == 0 && ((uintptr_t)T & 3) == 0 && ((uintptr_t)lS_i & 7) == 0 &&
                  ((uintptr_t)order & 7) == 0, "misaligned buffer");
    const dim3 grid((unsigned)cdiv(n, DAYFILE_TILE)), block(DAYFILE_TILE);
    // the tile's image and the tile's 256 entries of the order: (60 | 1) KiB + 2 KiB < 64 KiB
    const size_t lds = (size_t)(n_cat | 1) * DAYFILE_TILE * sizeof(int32_t) + DAYFILE_TILE * sizeof(int64_t);
    const int pairs = (n_cat % 2 == 0 && ((uintptr_t)x_cat & 7) == 0) ? 1 : 0;
    if (n_cat == 26)
        hipLaunchKernelGGL(k_rows_window<26>, grid, block, lds, (hipStream_t)stream, x_int, x_cat, y, order, n, (int)n_dense, 26,
                           pairs, max_ind_range, X, lS_i, lS_i_pitch, col0, T);
    else
        hipLaunchKernelGGL(k_rows_window<0>, grid, block, lds, (hipStream_t)stream, x_int, x_cat, y, order, n, (int)n_dense,
                           (int)n_cat, pairs, max_ind_range, X, lS_i, lS_i_pitch, col0, T);
    CDLRM_LAUNCH_CHECK();
    return 0;
}
