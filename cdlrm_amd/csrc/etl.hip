// Raw Criteo text on the device (cdlrm_amd/data_utils.py: getCriteoAdData): the reference's ETL walks the text one line and
// one field at a time in Python (data_utils.py:966-1044: process_one_file, :111-169: processCriteoAdData).  Here a chunk of the
// text lies in HBM and four small kernels do the per-line work:
//
//   cdlrm_etl_line_index   mark '\n', scan -> the start offset of every line that ends inside the chunk
//   cdlrm_etl_parse        one lane per line through etl_parse_line (etl_parse.h: the ONE parser, host and device)
//   cdlrm_etl_subsample    keep flag from (y, rand_u, rate), scan, stable scatter of the three arrays
//   cdlrm_etl_encode       a column of X_cat, value -> id, by binary search in that column's sorted keys
//
// No kernel here loops without a bound known at launch, none uses a floating-point atomic, none runs on the training queue.
// Malformed text is DATA: it is reported through the error word (64 bits, the smallest (line << 8 | code) wins by an integer
// atomicMin) and the line's outputs are zero.
#include "common.h"
#include "etl_parse.h"
#include "scan.h"

#define ETL_THREADS 256
#define ETL_BYTES_PER_THREAD 16
#define ETL_BYTES_PER_BLOCK (ETL_THREADS * ETL_BYTES_PER_THREAD)

typedef unsigned long long etl_err_t;

__device__ __forceinline__ void etl_report(etl_err_t* err, int64_t line1, int code) {
    atomicMin(err, ((etl_err_t)line1 << 8) | (etl_err_t)code);
}

// ---- line index -------------------------------------------------------------------------------------------------------------

// bit i of the result: byte base + i is a '\n' (bytes at or beyond len are not)
__device__ __forceinline__ unsigned etl_newline_mask(const uint8_t* text, int64_t base, int64_t len) {
    unsigned m = 0;
    if (base + ETL_BYTES_PER_THREAD <= len) {
        const uint4 v = *reinterpret_cast<const uint4*>(text + base);      // text is 16-byte aligned, base a multiple of 16
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int i = 0; i < 16; ++i) m |= (unsigned)(((w[i >> 2] >> ((i & 3) * 8)) & 0xff) == '\n') << i;
    } else {
#pragma unroll
        for (int i = 0; i < 16; ++i)
            if (base + i < len) m |= (unsigned)(text[base + i] == '\n') << i;
    }
    return m;
}

__global__ void __launch_bounds__(ETL_THREADS) k_etl_nl_count(const uint8_t* __restrict__ text, int64_t len,
                                                              int64_t* __restrict__ sums) {
    __shared__ int smem[32];
    const int64_t base = ((int64_t)blockIdx.x * ETL_THREADS + threadIdx.x) * ETL_BYTES_PER_THREAD;
    const int cnt = base < len ? __popc(etl_newline_mask(text, base, len)) : 0;
    int total;
    block_excl_scan(cnt, smem, &total);
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

__global__ void __launch_bounds__(ETL_THREADS) k_etl_nl_emit(const uint8_t* __restrict__ text, int64_t len,
                                                             const int64_t* __restrict__ sums, int64_t* __restrict__ starts,
                                                             int64_t cap) {
    __shared__ int smem[32];
    const int64_t base = ((int64_t)blockIdx.x * ETL_THREADS + threadIdx.x) * ETL_BYTES_PER_THREAD;
    const unsigned m = base < len ? etl_newline_mask(text, base, len) : 0u;
    int total;
    const int ex = block_excl_scan(__popc(m), smem, &total);
    int64_t rank = sums[blockIdx.x] + ex;              // newlines in front of this lane's first one
    if (blockIdx.x == 0 && threadIdx.x == 0) starts[0] = 0;
#pragma unroll
    for (int i = 0; i < ETL_BYTES_PER_THREAD; ++i)
        if (m & (1u << i)) {
            ++rank;
            if (rank <= cap) starts[rank] = base + i + 1;
        }
}

extern "C" int64_t cdlrm_etl_line_index_work_bytes(int64_t len) {
    if (len < 0) return -1;
    return (int64_t)sizeof(int64_t) * (cdiv(len, ETL_BYTES_PER_BLOCK) + 2);
}

extern "C" int cdlrm_etl_line_index(const uint8_t* text, int64_t len, int64_t* starts, int64_t cap, int64_t* d_count,
                                    void* work, int64_t work_bytes, void* stream) {
    CDLRM_REQUIRE(len >= 0 && cap >= 0, "negative size");
    CDLRM_REQUIRE(starts && d_count, "null buffer");
    CDLRM_REQUIRE(((uintptr_t)starts & 7) == 0 && ((uintptr_t)d_count & 7) == 0, "misaligned buffer");
    hipStream_t s = (hipStream_t)stream;
    if (len == 0) {
        CDLRM_HIP_CHECK(hipMemsetAsync(starts, 0, sizeof(int64_t), s));
        CDLRM_HIP_CHECK(hipMemsetAsync(d_count, 0, sizeof(int64_t), s));
        return 0;
    }
    CDLRM_REQUIRE(text && work, "null buffer");
    CDLRM_REQUIRE(((uintptr_t)text & 15) == 0 && ((uintptr_t)work & 7) == 0, "text must be 16-byte aligned");
    CDLRM_REQUIRE(work_bytes >= cdlrm_etl_line_index_work_bytes(len), "work buffer too small (cdlrm_etl_line_index_work_bytes)");
    const int64_t nblocks = cdiv(len, ETL_BYTES_PER_BLOCK);
    CDLRM_REQUIRE(nblocks <= 0x7fffffffll, "chunk too long for one launch");
    int64_t* sums = (int64_t*)work;
    CDLRM_CLEAR_STALE();
    hipLaunchKernelGGL(k_etl_nl_count, dim3((unsigned)nblocks), dim3(ETL_THREADS), 0, s, text, len, sums);
    hipLaunchKernelGGL(k_scan_tops, dim3(1), dim3(1024), 0, s, sums, nblocks, d_count);
    hipLaunchKernelGGL(k_etl_nl_emit, dim3((unsigned)nblocks), dim3(ETL_THREADS), 0, s, text, len, sums, starts, cap);
    CDLRM_LAUNCH_CHECK();
    return 0;
}

// ---- parse ------------------------------------------------------------------------------------------------------------------

// One lane per line: consecutive lines are contiguous, so a wave reads one contiguous span of the text.
__global__ void __launch_bounds__(ETL_THREADS) k_etl_parse(const uint8_t* __restrict__ text, int64_t len,
                                                           const int64_t* __restrict__ starts, int64_t n, int64_t line0,
                                                           int64_t max_ind_range, int32_t* __restrict__ y,
                                                           int32_t* __restrict__ x_int, int32_t* __restrict__ x_cat,
                                                           etl_err_t* err) {
    const int64_t i = (int64_t)blockIdx.x * ETL_THREADS + threadIdx.x;
    if (i >= n) return;
    const int64_t begin = starts[i], end = starts[i + 1] - 1;        // without the '\n'
    int32_t out[ETL_N_FIELDS];
    int code;
    if (begin < 0 || begin > end || end >= len) {                    // not a line index of this text: read nothing
        code = ETL_ERR_SPAN;
#pragma unroll
        for (int k = 0; k < ETL_N_FIELDS; ++k) out[k] = 0;
    } else {
        code = etl_parse_line(text, begin, end, max_ind_range, out, out + 1, out + 1 + ETL_N_DENSE);
    }
    y[i] = out[0];
#pragma unroll
    for (int k = 0; k < ETL_N_DENSE; ++k) x_int[i * ETL_N_DENSE + k] = out[1 + k];
#pragma unroll
    for (int k = 0; k < ETL_N_CAT; ++k) x_cat[i * ETL_N_CAT + k] = out[1 + ETL_N_DENSE + k];
    if (code) etl_report(err, line0 + i + 1, code);
}

extern "C" int cdlrm_etl_parse(const uint8_t* text, int64_t len, const int64_t* starts, int64_t n, int64_t line0,
                               int64_t max_ind_range, int32_t* y, int32_t* x_int, int32_t* x_cat, void* err, void* stream) {
    CDLRM_REQUIRE(len >= 0 && n >= 0 && line0 >= 0, "negative size");
    CDLRM_REQUIRE(n <= len, "every line ends with a byte of the text");
    CDLRM_REQUIRE(line0 + n < (1ll << 55), "line number too large for the error word");
    if (n == 0) return 0;
    CDLRM_REQUIRE(text && starts && y && x_int && x_cat && err, "null buffer");
    CDLRM_REQUIRE(((uintptr_t)starts & 7) == 0 && ((uintptr_t)err & 7) == 0 && (((uintptr_t)y | (uintptr_t)x_int | (uintptr_t)x_cat) & 3) == 0,
                  "misaligned buffer");
    const int64_t nblocks = cdiv(n, ETL_THREADS);
    CDLRM_REQUIRE(nblocks <= 0x7fffffffll, "too many lines for one launch");
    CDLRM_CLEAR_STALE();
    hipLaunchKernelGGL(k_etl_parse, dim3((unsigned)nblocks), dim3(ETL_THREADS), 0, (hipStream_t)stream, text, len, starts, n, line0,
                       max_ind_range, y, x_int, x_cat, (etl_err_t*)err);
    CDLRM_LAUNCH_CHECK();
    return 0;
}

// ---- sub-sample -------------------------------------------------------------------------------------------------------------

// data_utils.py:991-993: a line is dropped iff target == 0 and rand_u[k] < rate, k the line's number in its file; in float64
__device__ __forceinline__ int etl_keep(const int32_t* y, const double* rand_u, int64_t line0, double rate, int64_t i) {
    return !(y[i] == 0 && rand_u[line0 + i] < rate);
}

__global__ void __launch_bounds__(ETL_THREADS) k_etl_keep_count(const int32_t* __restrict__ y, const double* __restrict__ rand_u,
                                                                int64_t line0, double rate, int64_t n, int64_t* __restrict__ sums) {
    __shared__ int smem[32];
    const int64_t i = (int64_t)blockIdx.x * ETL_THREADS + threadIdx.x;
    const int keep = i < n ? etl_keep(y, rand_u, line0, rate, i) : 0;
    int total;
    block_excl_scan(keep, smem, &total);
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

// behind k_scan_tops: rows_out = rows_in + kept (two different words: the scatter below still reads rows_in)
__global__ void k_etl_advance(const int64_t* rows_in, const int64_t* kept, int64_t* rows_out) {
    if (threadIdx.x == 0 && blockIdx.x == 0) *rows_out = *rows_in + *kept;
}

__global__ void __launch_bounds__(ETL_THREADS) k_etl_keep_scatter(const int32_t* __restrict__ y, const int32_t* __restrict__ x_int,
                                                                  const int32_t* __restrict__ x_cat,
                                                                  const double* __restrict__ rand_u, int64_t line0, double rate,
                                                                  int64_t n, const int64_t* __restrict__ sums,
                                                                  const int64_t* __restrict__ rows_in, int64_t out_cap,
                                                                  int32_t* __restrict__ out_y, int32_t* __restrict__ out_x_int,
                                                                  int32_t* __restrict__ out_x_cat) {
    __shared__ int smem[32];
    const int64_t i = (int64_t)blockIdx.x * ETL_THREADS + threadIdx.x;
    const int keep = i < n ? etl_keep(y, rand_u, line0, rate, i) : 0;
    int total;
    const int ex = block_excl_scan(keep, smem, &total);
    if (!keep) return;
    const int64_t o = *rows_in + sums[blockIdx.x] + ex;
    if (o < 0 || o >= out_cap) return;                  // (cannot happen with out_cap >= rows kept so far + n; never write outside)
    out_y[o] = y[i];
#pragma unroll
    for (int k = 0; k < ETL_N_DENSE; ++k) out_x_int[o * ETL_N_DENSE + k] = x_int[i * ETL_N_DENSE + k];
#pragma unroll
    for (int k = 0; k < ETL_N_CAT; ++k) out_x_cat[o * ETL_N_CAT + k] = x_cat[i * ETL_N_CAT + k];
}

extern "C" int64_t cdlrm_etl_subsample_work_bytes(int64_t n) {
    if (n < 0) return -1;
    return (int64_t)sizeof(int64_t) * (cdiv(n, ETL_THREADS) + 2);
}

extern "C" int cdlrm_etl_subsample(const int32_t* y, const int32_t* x_int, const int32_t* x_cat, int64_t n, const double* rand_u,
                                   int64_t n_rand, int64_t line0, double rate, int32_t* out_y, int32_t* out_x_int,
                                   int32_t* out_x_cat, int64_t out_cap, const int64_t* rows_in, int64_t* rows_out, void* work,
                                   int64_t work_bytes, void* stream) {
    CDLRM_REQUIRE(n >= 0 && line0 >= 0 && out_cap >= 0, "negative size");
    CDLRM_REQUIRE(line0 + n <= n_rand, "rand_u must hold a draw for every line of the file");
    CDLRM_REQUIRE(rate > 0.0, "not launched at rate 0: the rows are kept as they are");
    CDLRM_REQUIRE(rows_in && rows_out && rows_in != rows_out, "rows_in and rows_out are two different words");
    hipStream_t s = (hipStream_t)stream;
    if (n == 0) {
        CDLRM_HIP_CHECK(hipMemcpyAsync(rows_out, rows_in, sizeof(int64_t), hipMemcpyDeviceToDevice, s));
        return 0;
    }
    CDLRM_REQUIRE(y && x_int && x_cat && rand_u && out_y && out_x_int && out_x_cat && work, "null buffer");
    CDLRM_REQUIRE(((uintptr_t)rand_u & 7) == 0 && ((uintptr_t)work & 7) == 0 && ((uintptr_t)rows_in & 7) == 0 && ((uintptr_t)rows_out & 7) == 0,
                  "misaligned buffer");
    CDLRM_REQUIRE(work_bytes >= cdlrm_etl_subsample_work_bytes(n), "work buffer too small (cdlrm_etl_subsample_work_bytes)");
    const int64_t nblocks = cdiv(n, ETL_THREADS);
    CDLRM_REQUIRE(nblocks <= 0x7fffffffll, "too many rows for one launch");
    int64_t* sums = (int64_t*)work;
    int64_t* kept = sums + nblocks;                      // the chunk's kept rows, behind the block sums
    CDLRM_CLEAR_STALE();
    hipLaunchKernelGGL(k_etl_keep_count, dim3((unsigned)nblocks), dim3(ETL_THREADS), 0, s, y, rand_u, line0, rate, n, sums);
    hipLaunchKernelGGL(k_scan_tops, dim3(1), dim3(1024), 0, s, sums, nblocks, kept);
    hipLaunchKernelGGL(k_etl_advance, dim3(1), dim3(64), 0, s, rows_in, (const int64_t*)kept, rows_out);
    hipLaunchKernelGGL(k_etl_keep_scatter, dim3((unsigned)nblocks), dim3(ETL_THREADS), 0, s, y, x_int, x_cat, rand_u, line0, rate, n,
                       (const int64_t*)sums, rows_in, out_cap, out_y, out_x_int, out_x_cat);
    CDLRM_LAUNCH_CHECK();
    return 0;
}

// ---- encode -----------------------------------------------------------------------------------------------------------------

// x_cat[r, col] = ids[k] with keys[k] == x_cat[r, col]; keys ascending (signed), m < 2^31: at most 32 halvings
__global__ void __launch_bounds__(ETL_THREADS) k_etl_encode(int32_t* __restrict__ x_cat, int64_t n, int n_cols, int col,
                                                            const int32_t* __restrict__ keys, const int32_t* __restrict__ ids,
                                                            int64_t m, int64_t row0, etl_err_t* err) {
    const int64_t r = (int64_t)blockIdx.x * ETL_THREADS + threadIdx.x;
    if (r >= n) return;
    int32_t* cell = x_cat + r * n_cols + col;
    const int32_t v = *cell;
    int64_t lo = 0, hi = m;
#pragma unroll 1
    for (int step = 0; step < 32 && lo < hi; ++step) {
        const int64_t mid = (lo + hi) >> 1;
        if (keys[mid] < v) lo = mid + 1; else hi = mid;
    }
    if (lo < m && keys[lo] == v) {
        *cell = ids[lo];
    } else {
        *cell = 0;
        etl_report(err, row0 + r + 1, ETL_ERR_NOT_IN_DICT);
    }
}

extern "C" int cdlrm_etl_encode(int32_t* x_cat, int64_t n, int32_t n_cols, int32_t col, const int32_t* keys, const int32_t* ids,
                                int64_t m, int64_t row0, void* err, void* stream) {
    CDLRM_REQUIRE(n >= 0 && m >= 0 && row0 >= 0, "negative size");
    CDLRM_REQUIRE(n_cols >= 1 && col >= 0 && col < n_cols, "column outside the row");
    CDLRM_REQUIRE(m <= 0x7fffffffll, "a dictionary holds fewer than 2^31 keys (32 search steps)");
    CDLRM_REQUIRE(row0 + n < (1ll << 55), "row number too large for the error word");
    if (n == 0) return 0;
    CDLRM_REQUIRE(x_cat && err && (m == 0 || (keys && ids)), "null buffer");
    CDLRM_REQUIRE(((uintptr_t)err & 7) == 0 && (((uintptr_t)x_cat | (uintptr_t)keys | (uintptr_t)ids) & 3) == 0, "misaligned buffer");
    const int64_t nblocks = cdiv(n, ETL_THREADS);
    CDLRM_REQUIRE(nblocks <= 0x7fffffffll, "too many rows for one launch");
    CDLRM_CLEAR_STALE();
    hipLaunchKernelGGL(k_etl_encode, dim3((unsigned)nblocks), dim3(ETL_THREADS), 0, (hipStream_t)stream, x_cat, n, (int)n_cols, (int)col,
                       keys, ids, m, row0, (etl_err_t*)err);
    CDLRM_LAUNCH_CHECK();
    return 0;
}
