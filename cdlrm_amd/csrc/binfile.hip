// Batches of the MLPerf binary Criteo files, cut on the device a look-ahead window per launch
// (cdlrm_amd/data_loader_terabyte.py: DeviceBinLoader).
//
// The binary file stores one record per sample, [y | n_dense | n_cat] int32 (data_loader_terabyte.py:238-275: 40 dwords,
// 160 B at 13 / 26 features), and the reference cuts a batch out of it with one seek + read and transforms it on the host
// (:225-235 -> _transform_features, :68-87).  Here the RAW records of a window go to HBM once and one launch per piece writes
// the window's (X, lS_i, T) exactly as csrc/dayfile.hip does for the three arrays of a day file -- same arithmetic
// (dayfile_index / dayfile_dense restated below, word for word), same outputs, same bytes per sample (160 read, 264 written),
// ONE input stream instead of three.
//
// A workgroup reads its tile of 256 records as a flat dword stream, coalesced 16-byte loads between a scalar head and tail (a
// record of 40 dwords is 16-byte aligned only when the buffer is; a record of 1 + n_dense + n_cat dwords in general is not),
// and keeps the tile in LDS at a record stride S = R | 1 dwords, R = 1 + n_dense + n_cat.  S is odd, so the column reads that
// follow -- lane t reads dword c of record t: bank (t * S + c) mod 32 (ds_read_b32 banks over 32 dwords, the two 32-lane
// halves of a wave do not conflict with each other) -- touch 32 different banks per half: gcd(S, 32) = 1.  For the Criteo
// record R = 40 would put lanes t and t + 4 on one bank (gcd(40, 32) = 8, 8-way); S = 41 is free of conflicts.  When R is
// odd already the LDS image IS the flat stream, shifted so that the 16-byte global loads become 16-byte LDS stores.
// Out of LDS: every wave stores 64 consecutive int64 (512 B) of one table's row per instruction, T is a flat fp32 store of
// one dword per lane, and X -- row-major on both sides once y and the categorical dwords are skipped -- is a flat pass over
// the tile's nt * n_dense values with 16-byte stores between the destination's own head and tail.
#include "common.h"

#define BINFILE_TILE 256          // samples per workgroup = threads per workgroup
#define BINFILE_MAX_CAT 60        // as cdlrm_dayfile_window
#define BINFILE_MAX_LDS (160 * 1024)

// numpy's floor-mod (`x_cat % max_ind_range`, data_loader_terabyte.py:70-71): the result has the divisor's sign
__device__ __forceinline__ int64_t binfile_index(int32_t v, int64_t m) {
    if (m <= 0) return (int64_t)v;
    if (m > 0x7fffffffll)               // wider than any int32: only a negative entry changes
        return v < 0 ? (int64_t)v + m : (int64_t)v;
    int32_t r = v % (int32_t)m;
    if (r < 0) r += (int32_t)m;
    return (int64_t)r;
}

// data_loader_terabyte.py:73: torch.log(x_int.to(torch.float) + 1) -- int32 -> fp32 rounds first, the + 1 is an fp32 add; the
// logarithm is taken in double and rounded once (csrc/dayfile.hip: dayfile_dense)
__device__ __forceinline__ float binfile_dense(int32_t v) {
    const float f = (float)v + 1.0f;
    return (float)log((double)f);
}

// ND_T / NC_T > 0: the record's shape at compile time (the divisions fold to multiplies); 0: at run time
template <int ND_T, int NC_T>
__global__ void __launch_bounds__(BINFILE_TILE) k_binfile_window(const int32_t* __restrict__ rec, int64_t n, int nd_rt, int nc_rt,
                                                                 int64_t max_ind_range, float* __restrict__ X,
                                                                 int64_t* __restrict__ lS_i, int64_t pitch, int64_t col0,
                                                                 float* __restrict__ T) {
    extern __shared__ __attribute__((aligned(16))) int32_t lds[];
    const int nd = ND_T ? ND_T : nd_rt;
    const int nc = NC_T ? NC_T : nc_rt;
    const int R = 1 + nd + nc;                                   // dwords per record
    const int S = R | 1;                                         // odd record stride in LDS
    const int tid = threadIdx.x;
    const int64_t t0 = (int64_t)blockIdx.x * BINFILE_TILE;       // first sample of this tile
    const int nt = (int)((n - t0) < BINFILE_TILE ? (n - t0) : BINFILE_TILE);

    // ---- the tile's records: flat read -> LDS
    const int32_t* src = rec + t0 * R;
    const int total = nt * R;
    int head = (int)(((16 - ((uintptr_t)src & 15)) & 15) >> 2);  // dwords up to the first 16-byte boundary
    if (head > total) head = total;
    const int nvec = (total - head) >> 2;
    const int tail0 = head + (nvec << 2);
    // S == R: dword f of the stream lies at tile[f], and tile is shifted so that tile + head is 16-byte aligned
    int32_t* tile = lds + (S == R ? ((4 - head) & 3) : 0);
    if (S == R) {
        if (tid < head) tile[tid] = src[tid];
        for (int v = tid; v < nvec; v += BINFILE_TILE) {
            const int f = head + (v << 2);
            *reinterpret_cast<int4*>(tile + f) = *reinterpret_cast<const int4*>(src + f);
        }
        if (tid < total - tail0) tile[tail0 + tid] = src[tail0 + tid];
    } else {
        if (tid < head) tile[tid + (tid / R) * (S - R)] = src[tid];
        for (int v = tid; v < nvec; v += BINFILE_TILE) {
            const int f = head + (v << 2);
            const int4 q = *reinterpret_cast<const int4*>(src + f);
            int s = f / R, k = f - s * R;
            const int32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                tile[s * S + k] = w[e];
                if (++k == R) { k = 0; ++s; }
            }
        }
        if (tid < total - tail0) {
            const int f = tail0 + tid;
            tile[f + (f / R) * (S - R)] = src[f];
        }
    }
    __syncthreads();
    // ---- LDS -> one table row at a time: lane t holds sample t0 + t, a wave stores 64 consecutive int64; T beside it
    if (tid < nt) {
        const int32_t* mine = tile + tid * S;
        const int32_t* cat = mine + 1 + nd;
        int64_t* dst = lS_i + col0 + t0 + tid;
        if (NC_T) {
#pragma unroll
            for (int k = 0; k < (NC_T ? NC_T : 1); ++k) dst[(int64_t)k * pitch] = binfile_index(cat[k], max_ind_range);
        } else {
            for (int k = 0; k < nc; ++k) dst[(int64_t)k * pitch] = binfile_index(cat[k], max_ind_range);
        }
        T[col0 + t0 + tid] = (float)mine[0];
    }
    // ---- dense features: the destination is row-major, a flat pass over the tile's nt * nd values out of LDS
    {
        float* dst = X + (col0 + t0) * nd;
        const int totd = nt * nd;
        int dhead = (int)(((16 - ((uintptr_t)dst & 15)) & 15) >> 2);
        if (dhead > totd) dhead = totd;
        const int dvec = (totd - dhead) >> 2;
        const int dtail0 = dhead + (dvec << 2);
        if (tid < dhead) dst[tid] = binfile_dense(tile[(tid / nd) * S + 1 + tid % nd]);
        for (int v = tid; v < dvec; v += BINFILE_TILE) {
            const int f = dhead + (v << 2);
            int s = f / nd, k = f - s * nd;
            float o[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                o[e] = binfile_dense(tile[s * S + 1 + k]);
                if (++k == nd) { k = 0; ++s; }
            }
            *reinterpret_cast<float4*>(dst + f) = make_float4(o[0], o[1], o[2], o[3]);
        }
        if (tid < totd - dtail0) {
            const int f = dtail0 + tid;
            dst[f] = binfile_dense(tile[(f / nd) * S + 1 + f % nd]);
        }
    }
}

extern "C" int cdlrm_binfile_tile(void) { return BINFILE_TILE; }

extern "C" int cdlrm_binfile_window(const int32_t* rec, int64_t n, int32_t n_dense, int32_t n_cat, int64_t max_ind_range, float* X,
                                    int64_t* lS_i, int64_t lS_i_pitch, int64_t col0, float* T, void* stream) {
    CDLRM_REQUIRE(n >= 0 && col0 >= 0 && lS_i_pitch >= col0 + n, "the piece must lie inside the window rectangle's row");
    CDLRM_REQUIRE(n_dense >= 1 && n_cat >= 1 && n_cat <= BINFILE_MAX_CAT, "1 .. 60 categorical features");
    // (+ 4 dwords: the shift that lines the LDS image up with the 16-byte loads)
    const size_t lds = ((size_t)((1 + n_dense + n_cat) | 1) * BINFILE_TILE + 4) * sizeof(int32_t);
    CDLRM_REQUIRE(lds <= BINFILE_MAX_LDS, "a tile of 256 records must fit the 160 KiB of LDS");
    if (n == 0) return 0;
    CDLRM_REQUIRE(rec && X && lS_i && T, "null buffer");
    CDLRM_REQUIRE(((uintptr_t)rec & 3) == 0 && ((uintptr_t)X & 3) == 0 && ((uintptr_t)T & 3) == 0 && ((uintptr_t)lS_i & 7) == 0,
                  "misaligned buffer");
    const dim3 grid((unsigned)cdiv(n, BINFILE_TILE)), block(BINFILE_TILE);
    if (n_dense == 13 && n_cat == 26) {         // (41 KiB)
        hipLaunchKernelGGL((k_binfile_window<13, 26>), grid, block, lds, (hipStream_t)stream, rec, n, 13, 26, max_ind_range, X, lS_i,
                           lS_i_pitch, col0, T);
    } else {
        // (64 KiB: what a kernel may ask for without the attribute)
        const int rc = cdlrm_grant_dynamic_lds<k_binfile_window<0, 0>, 64 * 1024>(lds);
        if (rc) return rc;
        hipLaunchKernelGGL((k_binfile_window<0, 0>), grid, block, lds, (hipStream_t)stream, rec, n, (int)n_dense, (int)n_cat,
                           max_ind_range, X, lS_i, lS_i_pitch, col0, T);
    }
    CDLRM_LAUNCH_CHECK();
    return 0;
}
