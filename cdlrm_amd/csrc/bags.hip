// Ragged multi-hot bags on the device (engine.BagWindows): a look-ahead window's global per-table index lists live in
// HBM as ONE int64 buffer, and the two layouts the training path reads are cut from it by copy-and-rebase kernels --
//   cdlrm_bags_window:     the window plan's rectangle [T, n_win] (engine.pad_window's contract)
//   cdlrm_bags_rank_slice: one batch's squared lists for a rank's samples [s0, s1) (engine.square_bags's contract on the
//                          rank's sub-batch, offsets rebased to 0)
// The host used to build both with a Python loop over the tables per step / per window, on the GLOBAL batch at every rank.
//
// Buffer layout: table k's list is the concatenation of the window's batches' table-k lists.  bpos [(L + 1) * T]:
// bpos[b * T + k] = position in buf of batch b's table-k list, bpos[L * T + k] = the end of table k's list, so batch b's
// table-k list is buf[bpos[b * T + k], bpos[(b + 1) * T + k]).  Both kernels are HBM-bound copies: one launch covers every
// table (grid.y), the index rows are written two lookups per lane with 16-byte vector stores.
#include "common.h"

// out[k, i] = list_k[i] for i < len_k, else list_k[0]  (len_k >= 1: the host refuses an empty table list)
__global__ void __launch_bounds__(256) k_bags_window(const int64_t* __restrict__ buf, const int64_t* __restrict__ bpos,
                                                     int32_t L, int32_t T, int64_t total, int64_t n_win,
                                                     int64_t* __restrict__ out) {
    const int k = blockIdx.y;
    const int64_t start = bpos[k];
    const int64_t len = bpos[(int64_t)L * T + k] - start;
    int64_t* row = out + (int64_t)k * n_win;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_win; i += (int64_t)gridDim.x * blockDim.x) {
        int64_t p = start + (i < len ? i : 0);
        p = p < 0 ? 0 : (p >= total ? total - 1 : p);          // (bounds: a malformed bpos reads inside buf, never past it)
        row[i] = buf[p];
    }
}

// One batch b (global offsets off [T, nbag], nbag = the batch's sample count), a rank's samples [s0, s1):
//   a_k = off[k, s0],  e_k = s1 < nbag ? off[k, s1] : len_k,  m_k = e_k - a_k  (the rank's lookups of table k)
//   idx[k, i]      = list_k[a_k + i] for i < m_k, else list_k[a_k]     (i < n; n even, rows 16-byte aligned)
//   off_out[k, i]  = off[k, s0 + i] - a_k for i < nb = s1 - s0;  off_out[k, nb] = m_k
__global__ void __launch_bounds__(256) k_bags_rank_slice(const int64_t* __restrict__ buf, const int64_t* __restrict__ bpos,
                                                         int32_t b, int32_t T, int64_t total, const int64_t* __restrict__ off,
                                                         int64_t nbag, int64_t s0, int64_t s1, int64_t n,
                                                         int64_t* __restrict__ idx, int64_t* __restrict__ off_out) {
    const int k = blockIdx.y;
    const int64_t start = bpos[(int64_t)b * T + k];
    const int64_t len = bpos[(int64_t)(b + 1) * T + k] - start;
    const int64_t* o = off + (int64_t)k * nbag;
    const int64_t a = o[s0];
    const int64_t e = s1 < nbag ? o[s1] : len;
    const int64_t m = e - a;
    const int64_t nb = s1 - s0;
    const int64_t half = n >> 1;
    const int64_t src0 = start + a;
    longlong2* row = reinterpret_cast<longlong2*>(idx + (int64_t)k * n);
    int64_t* orow = off_out + (int64_t)k * (nb + 1);
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < half + nb + 1; t += (int64_t)gridDim.x * blockDim.x) {
        if (t < half) {
            const int64_t i = 2 * t;
            int64_t p0 = src0 + (i < m ? i : 0), p1 = src0 + (i + 1 < m ? i + 1 : 0);
            p0 = p0 < 0 ? 0 : (p0 >= total ? total - 1 : p0);
            p1 = p1 < 0 ? 0 : (p1 >= total ? total - 1 : p1);
            longlong2 v;
            v.x = buf[p0];
            v.y = buf[p1];
            row[t] = v;
        } else {
            const int64_t i = t - half;
            orow[i] = i < nb ? o[s0 + i] - a : m;
        }
    }
}

extern "C" int cdlrm_bags_window(const int64_t* buf, int64_t total, const int64_t* bpos, int32_t L, int32_t T, int64_t n_win,
                                 int64_t* out, void* stream) {
    CDLRM_REQUIRE(buf && bpos && out && total >= 1 && L >= 1 && T >= 1 && T <= 65535 && n_win >= 1, "bad argument");
    int64_t gx = cdiv(n_win, 256 * 4);
    if (gx > 1024) gx = 1024;
    hipLaunchKernelGGL(k_bags_window, dim3((unsigned)gx, (unsigned)T), dim3(256), 0, (hipStream_t)stream, buf, bpos, L, T,
                       total, n_win, out);
    CDLRM_LAUNCH_CHECK();
    return 0;
}

extern "C" int cdlrm_bags_rank_slice(const int64_t* buf, int64_t total, const int64_t* bpos, int32_t L, int32_t b, int32_t T,
                                     const int64_t* off, int64_t nbag, int64_t s0, int64_t s1, int64_t n, int64_t* idx,
                                     int64_t* off_out, void* stream) {
    CDLRM_REQUIRE(buf && bpos && off && idx && off_out && total >= 1 && 0 <= b && b < L && T >= 1 && T <= 65535,
                  "bad argument");
    CDLRM_REQUIRE(0 <= s0 && s0 < s1 && s1 <= nbag, "the rank's sample range must be a non-empty part of the batch");
    CDLRM_REQUIRE(n >= 2 && n % 2 == 0, "the squared width must be even (engine: a multiple of 256)");
    CDLRM_REQUIRE(((uintptr_t)idx & 15) == 0, "idx must be 16-byte aligned");
    const int64_t work = n / 2 + (s1 - s0) + 1;
    int64_t gx = cdiv(work, 256 * 4);
    if (gx > 1024) gx = 1024;
    hipLaunchKernelGGL(k_bags_rank_slice, dim3((unsigned)gx, (unsigned)T), dim3(256), 0, (hipStream_t)stream, buf, bpos, b, T,
                       total, off, nbag, s0, s1, n, idx, off_out);
    CDLRM_LAUNCH_CHECK();
    return 0;
}
