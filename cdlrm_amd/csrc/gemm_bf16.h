// bf16 matrix-core GEMM for gfx950: the opt-in `CDLRM_GEMM_BF16` mode of the MLP layers ("bf16 mode").
//
//   C[m,n] = sum_k bf16(A(m,k)) * bf16(B(k,n))     fp32 operands in HBM, fp32 accumulation, fp32 epilogue
//
// Same structure as the register-staged k_gemm of gemm.h -- block tile (64*TM) x (64*TN), 4 waves as 2x2, global -> register
// prefetch of the next K tile under the current tile's MFMAs, one barrier pair per K tile -- with the operand conversion on the
// way INTO LDS: each fp32 element is rounded ONCE to bf16 (v_cvt_pk_bf16_f32: round-to-nearest-even, a NaN stays a NaN) and the
// LDS images hold bf16, half the bytes and half the reads of an fp32 image.  The K tile is 64 deep: four
// v_mfma_f32_32x32x16_bf16 steps per accumulator.  A bf16 x bf16 product is exact in fp32 (8 + 8 significand bits), so the only
// roundings are the operand casts and the fp32 accumulation, in an order fixed by the tile shape: no atomics, two launches give
// the same bits.
//
// LDS images: both operands contraction-contiguous, [rows][B16_KP] bf16, B16_KP = 64 + 8 (144-byte pitch: an odd multiple of
// 16 B, so the ds_read_b128 fragment reads of 16 consecutive rows hit disjoint banks).  Operand lane map of the 32x32x16 bf16
// MFMA (cdna_hip_programming.md): lane l holds A[row l & 31][k = 8 (l >> 5) + j] and B[k = 8 (l >> 5) + j][col l & 31], j = 0..7;
// the C/D layout is that of the fp32 32x32 MFMA, so the epilogue is gemm.h's.
//
// Staging pieces (what one thread loads and converts for one operand):
//   contraction-contiguous (A_KC / B_KC): a row's 8 consecutive k -- two float4 loads, one 16-byte LDS write;
//   contraction-strided: 4 consecutive k x 4 consecutive rows -- four float4 loads, four 8-byte LDS writes (the transpose
//   happens in the write pass).
// Rows past the matrix edge are clamped to valid addresses (their products land in outputs that are never stored), contraction
// indices past the split's end are zero-filled at LDS-write time -- the K tails (479, 480 not a multiple of 64) included.
//
// PL = 2: the opt-in `CDLRM_GEMM_BF16X3` mode, the same kernels with two bf16 PLANES per operand:
//
//   x ~ h + l,   h = bf16(x),   l = bf16(x - float(h))   (the subtraction is exact in fp32; l = 0 where h is not finite)
//   C[m,n] = sum_k  al*bh + ah*bl + ah*bh                 (al*bl, ~2^-16 of the product, is dropped)
//
// Loads, staging registers, K tails and epilogue are those of PL = 1; b16_store writes a hi image and, ROWS * B16_KP elements
// behind it, a lo image of the same pitch (two planes = the LDS bytes of one fp32 image), and each 16-deep step issues three
// MFMAs per accumulator -- lo*hi, hi*lo, hi*hi, the small terms first -- into the one fp32 accumulator.  |x - h - l| <= 2^-16 |x|,
// so a product is off by ~3 * 2^-16 of its magnitude at most: near fp32, not fp32.  Tiles: 64x64 and 64x128 only (a 128x128
// tile's four images are 73.7 KB, past the 64 KB a workgroup may declare statically).
#pragma once
#include "gemm.h"

#define B16_BK 64
#define B16_KP (B16_BK + 8)

typedef __bf16 b16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 b16x2 __attribute__((ext_vector_type(2)));
typedef float f32x2v __attribute__((ext_vector_type(2)));

// two fp32 -> packed bf16 pair (lo in bits 0-15): the plain cast, v_cvt_pk_bf16_f32 (round-to-nearest-even, NaN-preserving)
__device__ __forceinline__ unsigned b16_pack(float lo, float hi) {
    const b16x2 v = __builtin_convertvector((f32x2v){lo, hi}, b16x2);
    return __builtin_bit_cast(unsigned, v);
}

// the two planes of a pair: hi = the plain cast, lo = the cast of the (exact) remainder, 0 where hi is Inf or NaN -- a NaN or an
// overflow then lives in the hi plane alone and reaches the outputs of its own row / column only
__device__ __forceinline__ void b16_split(float x0, float x1, unsigned& hi, unsigned& lo) {
    hi = b16_pack(x0, x1);
    const float r0 = x0 - __uint_as_float(hi << 16), r1 = x1 - __uint_as_float(hi & 0xffff0000u);
    lo = b16_pack((hi & 0x7f80u) != 0x7f80u ? r0 : 0.f, (hi & 0x7f800000u) != 0x7f800000u ? r1 : 0.f);
}

// float4s one thread holds for one operand tile of ROWS rows x 64 contraction indices (both staging forms: ROWS / 16)
template <int ROWS>
struct B16Stage {
    float4 v[ROWS / 16];
};

template <bool KC, int ROWS, bool VEC>
__device__ __forceinline__ void b16_load(const float* __restrict__ P, int64_t ld, int64_t r0, int64_t rmax, int64_t k0,
                                         int64_t kmax, B16Stage<ROWS>& st) {
    // straight-line code (see tile_load in gemm.h: a branch around the loads would drain the prefetch)
    if (KC) {
#pragma unroll
        for (int i = 0; i < ROWS / 32; ++i) {
            const int f = threadIdx.x + i * 256;
            const int64_t r = f / 8, c = (f % 8) * 8;
            const int64_t rr = min(r0 + r, rmax - 1);
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                if (VEC) {
                    st.v[2 * i + h] = *reinterpret_cast<const float4*>(P + rr * ld + min(k0 + c + 4 * h, kmax - 4));
                } else {
                    float e[4];
#pragma unroll
                    for (int u = 0; u < 4; ++u) e[u] = P[rr * ld + min(k0 + c + 4 * h + u, kmax - 1)];
                    st.v[2 * i + h] = make_float4(e[0], e[1], e[2], e[3]);
                }
            }
        }
    } else {
#pragma unroll
        for (int i = 0; i < ROWS / 64; ++i) {
            const int f = threadIdx.x + i * 256;
            const int64_t kg = f / (ROWS / 4), r = (f % (ROWS / 4)) * 4;
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int64_t kk = min(k0 + 4 * kg + u, kmax - 1);
                if (VEC) {
                    st.v[4 * i + u] = *reinterpret_cast<const float4*>(P + kk * ld + min(r0 + r, rmax - 4));
                } else {
                    float e[4];
#pragma unroll
                    for (int q = 0; q < 4; ++q) e[q] = P[kk * ld + min(r0 + r + q, rmax - 1)];
                    st.v[4 * i + u] = make_float4(e[0], e[1], e[2], e[3]);
                }
            }
        }
    }
}

// convert + write one staged tile into its bf16 LDS image (PL = 2: the hi image at S, the lo image ROWS * B16_KP behind it),
// zero-filling contraction indices >= kmax
template <bool KC, int ROWS, int PL>
__device__ __forceinline__ void b16_store(unsigned short* __restrict__ S, const B16Stage<ROWS>& st, int64_t k0, int64_t kmax) {
    unsigned short* __restrict__ SL = (PL == 2) ? S + ROWS * B16_KP : S;     // PL = 1: the one image only, SL unused
    if (KC) {
#pragma unroll
        for (int i = 0; i < ROWS / 32; ++i) {
            const int f = threadIdx.x + i * 256;
            const int r = f / 8, c = (f % 8) * 8;
            float e[8] = {st.v[2 * i].x, st.v[2 * i].y, st.v[2 * i].z, st.v[2 * i].w,
                          st.v[2 * i + 1].x, st.v[2 * i + 1].y, st.v[2 * i + 1].z, st.v[2 * i + 1].w};
#pragma unroll
            for (int u = 0; u < 8; ++u) e[u] = (k0 + c + u < kmax) ? e[u] : 0.f;     // selects, not branches
            uint4 w;
            if (PL == 2) {
                uint4 wl;
                b16_split(e[0], e[1], w.x, wl.x); b16_split(e[2], e[3], w.y, wl.y);
                b16_split(e[4], e[5], w.z, wl.z); b16_split(e[6], e[7], w.w, wl.w);
                *reinterpret_cast<uint4*>(SL + r * B16_KP + c) = wl;
            } else {
                w.x = b16_pack(e[0], e[1]); w.y = b16_pack(e[2], e[3]); w.z = b16_pack(e[4], e[5]); w.w = b16_pack(e[6], e[7]);
            }
            *reinterpret_cast<uint4*>(S + r * B16_KP + c) = w;
        }
    } else {
#pragma unroll
        for (int i = 0; i < ROWS / 64; ++i) {
            const int f = threadIdx.x + i * 256;
            const int kg = f / (ROWS / 4), r = (f % (ROWS / 4)) * 4;
            float4 x[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const bool ok = k0 + 4 * kg + u < kmax;
                x[u] = st.v[4 * i + u];
                x[u].x = ok ? x[u].x : 0.f; x[u].y = ok ? x[u].y : 0.f; x[u].z = ok ? x[u].z : 0.f; x[u].w = ok ? x[u].w : 0.f;
            }
            uint2 w0, w1, w2, w3;       // row r + q: its 4 consecutive contraction indices 4 kg .. 4 kg + 3
            if (PL == 2) {
                uint2 l0, l1, l2, l3;
                b16_split(x[0].x, x[1].x, w0.x, l0.x); b16_split(x[2].x, x[3].x, w0.y, l0.y);
                b16_split(x[0].y, x[1].y, w1.x, l1.x); b16_split(x[2].y, x[3].y, w1.y, l1.y);
                b16_split(x[0].z, x[1].z, w2.x, l2.x); b16_split(x[2].z, x[3].z, w2.y, l2.y);
                b16_split(x[0].w, x[1].w, w3.x, l3.x); b16_split(x[2].w, x[3].w, w3.y, l3.y);
                *reinterpret_cast<uint2*>(SL + (r + 0) * B16_KP + 4 * kg) = l0;
                *reinterpret_cast<uint2*>(SL + (r + 1) * B16_KP + 4 * kg) = l1;
                *reinterpret_cast<uint2*>(SL + (r + 2) * B16_KP + 4 * kg) = l2;
                *reinterpret_cast<uint2*>(SL + (r + 3) * B16_KP + 4 * kg) = l3;
            } else {
                w0.x = b16_pack(x[0].x, x[1].x); w0.y = b16_pack(x[2].x, x[3].x);
                w1.x = b16_pack(x[0].y, x[1].y); w1.y = b16_pack(x[2].y, x[3].y);
                w2.x = b16_pack(x[0].z, x[1].z); w2.y = b16_pack(x[2].z, x[3].z);
                w3.x = b16_pack(x[0].w, x[1].w); w3.y = b16_pack(x[2].w, x[3].w);
            }
            *reinterpret_cast<uint2*>(S + (r + 0) * B16_KP + 4 * kg) = w0;
            *reinterpret_cast<uint2*>(S + (r + 1) * B16_KP + 4 * kg) = w1;
            *reinterpret_cast<uint2*>(S + (r + 2) * B16_KP + 4 * kg) = w2;
            *reinterpret_cast<uint2*>(S + (r + 3) * B16_KP + 4 * kg) = w3;
        }
    }
}

// As / Bs: PL images of BM / BN rows each
template <bool A_KC, bool B_KC, int TM, int TN, bool VA, bool VB, int PL>
__device__ __forceinline__ void gemm_bf16_body(const GemmArgs& g, unsigned bx, unsigned by, unsigned bz,
                                               unsigned short* __restrict__ As, unsigned short* __restrict__ Bs) {
    constexpr int BM = 64 * TM, BN = 64 * TN;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int64_t m0 = (int64_t)by * BM;
    const int64_t n0 = (int64_t)bx * BN;
    const int64_t kbeg = (int64_t)bz * g.kchunk;
    const int64_t kend = min(g.K, kbeg + g.kchunk);
    f32x16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
    B16Stage<BM> ra;
    B16Stage<BN> rb;
    // bias gradient (weight-gradient layout): the first column panel sums its fp32 A values (= dZ^T) over the contraction --
    // from the registers, before they are rounded
    const bool do_colsum = !A_KC && g.colsum != nullptr && bx == 0;
    float4 csum = make_float4(0.f, 0.f, 0.f, 0.f);
    b16_load<A_KC, BM, VA>(g.A, g.lda, m0, g.M, kbeg, kend, ra);
    b16_load<B_KC, BN, VB>(g.B, g.ldb, n0, g.N, kbeg, kend, rb);
    const int lr = lane & 31, lh = lane >> 5;
    for (int64_t k0 = kbeg; k0 < kend; k0 += B16_BK) {
        __syncthreads();
        b16_store<A_KC, BM, PL>(As, ra, k0, kend);
        b16_store<B_KC, BN, PL>(Bs, rb, k0, kend);
        __syncthreads();
        if (!A_KC && do_colsum) {       // wave-uniform; no loads inside
#pragma unroll
            for (int i = 0; i < BM / 64; ++i) {
                const int kg = (threadIdx.x + i * 256) / (BM / 4);
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const bool ok = k0 + 4 * kg + u < kend;
                    const float4 x = ra.v[4 * i + u];
                    csum.x += ok ? x.x : 0.f; csum.y += ok ? x.y : 0.f; csum.z += ok ? x.z : 0.f; csum.w += ok ? x.w : 0.f;
                }
            }
        }
        // unconditional: past the last tile the clamped addresses just re-read valid data
        b16_load<A_KC, BM, VA>(g.A, g.lda, m0, g.M, k0 + B16_BK, kend, ra);
        b16_load<B_KC, BN, VB>(g.B, g.ldb, n0, g.N, k0 + B16_BK, kend, rb);
#pragma unroll
        for (int s = 0; s < B16_BK / 16; ++s) {
            b16x8 a[PL][TM], b[PL][TN];          // [0] hi, [1] lo
#pragma unroll
            for (int p = 0; p < PL; ++p) {
#pragma unroll
                for (int i = 0; i < TM; ++i) {
                    const int r = p * BM + wm * (32 * TM) + i * 32 + lr;
                    a[p][i] = __builtin_bit_cast(b16x8, *reinterpret_cast<const uint4*>(As + r * B16_KP + 16 * s + 8 * lh));
                }
#pragma unroll
                for (int j = 0; j < TN; ++j) {
                    const int c = p * BN + wn * (32 * TN) + j * 32 + lr;
                    b[p][j] = __builtin_bit_cast(b16x8, *reinterpret_cast<const uint4*>(Bs + c * B16_KP + 16 * s + 8 * lh));
                }
            }
            // PL = 2: lo*hi, hi*lo, then hi*hi; each pass over all accumulators, so that consecutive MFMAs are independent
#pragma unroll
            for (int t = (PL == 2 ? 0 : 2); t < 3; ++t) {
                const int pa = t == 0 ? PL - 1 : 0, pb = t == 1 ? PL - 1 : 0;
#pragma unroll
                for (int i = 0; i < TM; ++i)
#pragma unroll
                    for (int j = 0; j < TN; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[pa][i], b[pb][j], acc[i][j], 0, 0, 0);
            }
        }
    }
    if (!A_KC && do_colsum) {
        // the threads with equal (tid % (BM/4)) hold the same 4 rows for different contraction indices: combine them through
        // LDS in a fixed order
        __syncthreads();                        // every wave is done reading As
        float* red = reinterpret_cast<float*>(As);
        const int q = threadIdx.x / (BM / 4), r4 = (threadIdx.x % (BM / 4)) * 4;
        *reinterpret_cast<float4*>(red + q * BM + r4) = csum;
        __syncthreads();
        if (threadIdx.x < BM && m0 + threadIdx.x < g.M) {
            float s = 0.f;
#pragma unroll
            for (int qq = 0; qq < 1024 / BM; ++qq) s += red[qq * BM + threadIdx.x];
            g.colsum[(int64_t)bz * g.M + m0 + threadIdx.x] = s;
        }
    }
    float* C = g.C + (int64_t)bz * g.slab;
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            const int64_t col = n0 + wn * (32 * TN) + j * 32 + lr;
            if (col >= g.N) continue;
            const float bv = g.bias ? g.bias[col] : 0.f;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int64_t row = m0 + wm * (32 * TM) + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
                if (row >= g.M) continue;
                float v = acc[i][j][r] + bv;
                if (g.act == 1) v = v > 0.f ? v : 0.f;
                else if (g.act == 2) v = 1.0f / (1.0f + expf(-v));
                if (g.mask_act) {               // activation backward of the layer below, fused into the dgrad
                    const float x = g.mask[row * g.ldmask + col];
                    v = g.mask_act == 1 ? (x > 0.f ? v : 0.f) : v * ((1.0f - x) * x);
                }
                C[row * g.ldc + col] = v;
            }
        }
}

template <bool A_KC, bool B_KC, int TM, int TN, bool VA, bool VB, int PL>
__global__ void __launch_bounds__(256) k_gemm_bf16(GemmArgs g) {
    static_assert(PL * 64 * (TM + TN) * B16_KP * 2 <= 65536, "static LDS of a workgroup");
    __shared__ __attribute__((aligned(16))) unsigned short As[PL * 64 * TM * B16_KP];
    __shared__ __attribute__((aligned(16))) unsigned short Bs[PL * 64 * TN * B16_KP];
    const unsigned nwg = gridDim.x * gridDim.y * gridDim.z;
    const unsigned wgid = xcd_remap((blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x, nwg);
    gemm_bf16_body<A_KC, B_KC, TM, TN, VA, VB, PL>(g, wgid % gridDim.x, (wgid / gridDim.x) % gridDim.y,
                                                   wgid / (gridDim.x * gridDim.y), As, Bs);
}

// grouped launch of 64x64-tile problems (the weight gradients of several layers), each with its own contraction split
template <bool VA, bool VB, int PL>
__global__ void __launch_bounds__(256) k_gemm_bf16_group(GemmGroup grp) {
    __shared__ __attribute__((aligned(16))) unsigned short As[PL * 64 * B16_KP];
    __shared__ __attribute__((aligned(16))) unsigned short Bs[PL * 64 * B16_KP];
    const unsigned wgid = xcd_remap(blockIdx.x, gridDim.x);
    int p = 0;
#pragma unroll
    for (int q = 1; q < GEMM_GROUP_MAX; ++q)
        if (q < grp.n && wgid >= grp.first[q]) p = q;
    const GemmArgs& g = grp.g[p];
    const unsigned local = wgid - grp.first[p];
    const unsigned gx = (unsigned)((g.N + 63) / 64), gy = (unsigned)((g.M + 63) / 64);
    gemm_bf16_body<false, false, 1, 1, VA, VB, PL>(g, local % gx, (local / gx) % gy, local / (gx * gy), As, Bs);
}

// ---- host side ---------------------------------------------------------------------------------------------------------------

// The shape rule of the mode (layer terms: N outputs, K inputs): every GEMM of a layer with K >= 32 and N >= 32 -- never M, so
// results do not depend on the batch size.  The 13-wide first layer and the 1-wide head stay on their fp32 routes.
static inline bool bf16_layer_ok(int64_t N, int64_t K) { return N >= 32 && K >= 32; }

// The mode bits of a flags word -> operand planes: 0 fp32, 1 CDLRM_GEMM_BF16, 2 CDLRM_GEMM_BF16X3, -1 both (an error)
#define BF16_MODES (CDLRM_GEMM_BF16 | CDLRM_GEMM_BF16X3)
static inline int bf16_planes(int32_t flags) {
    const int32_t m = flags & BF16_MODES;
    return m == 0 ? 0 : m == CDLRM_GEMM_BF16 ? 1 : m == CDLRM_GEMM_BF16X3 ? 2 : -1;
}
static inline int bf16_family(int planes) { return planes == 2 ? CDLRM_ROUTE_BF16X3 : CDLRM_ROUTE_BF16; }

// 16-byte loads legal for one operand: rows 16-byte aligned, and >= 4 elements along the loaded direction
template <bool KC>
static inline bool bf16_vec(const float* P, int64_t ld, int64_t rows, int64_t kdim) {
    if (!aligned16(P) || ld % 4 != 0) return false;
    return KC ? kdim % 4 == 0 : (rows % 4 == 0 && rows >= 4);
}

// tile of an un-split forward / dgrad: the largest of 128x128, 64x128, 64x64 whose grid keeps >= 4 workgroups per CU (the
// loads, not the MFMAs, set the pace here: more workgroups in flight hide more of their latency).  (128x64 is never picked: its
// grid is never larger than 64x128's.)  Two planes: the same rule over 64x128 and 64x64 (55.3 and 36.9 KB of LDS: two and four
// workgroups per CU; 128x128 would need 73.7 KB, more than a workgroup may declare statically).
static inline void bf16_pick_tile(int64_t M, int64_t N, int planes, int* tm, int* tn) {
    const int cand[3][2] = {{2, 2}, {1, 2}, {1, 1}};
    for (int c = planes == 2 ? 1 : 0; c < 3; ++c) {
        if (cdiv(M, 64 * cand[c][0]) * cdiv(N, 64 * cand[c][1]) >= 2 * GEMM_MIN_BLOCKS || c == 2) {
            *tm = cand[c][0]; *tn = cand[c][1];
            return;
        }
    }
}

template <bool A_KC, bool B_KC, int TM, int TN, int PL>
static void launch_gemm_bf16_v(const GemmArgs& g, dim3 grid, hipStream_t s) {
    if (g.vecA && g.vecB) CDLRM_LAUNCH_EV((k_gemm_bf16<A_KC, B_KC, TM, TN, true, true, PL>), grid, dim3(256), 0, s, g);
    else if (g.vecA) CDLRM_LAUNCH_EV((k_gemm_bf16<A_KC, B_KC, TM, TN, true, false, PL>), grid, dim3(256), 0, s, g);
    else if (g.vecB) CDLRM_LAUNCH_EV((k_gemm_bf16<A_KC, B_KC, TM, TN, false, true, PL>), grid, dim3(256), 0, s, g);
    else CDLRM_LAUNCH_EV((k_gemm_bf16<A_KC, B_KC, TM, TN, false, false, PL>), grid, dim3(256), 0, s, g);
}

// Contraction slabs of a bf16 weight gradient over the batch M: ~1024 workgroups of 64x64 over `tiles` output tiles, each slab
// at least 4 K tiles deep, cut on K-tile boundaries.  Returns the slab length (kchunk); the slab count is cdiv(M, kchunk).
static inline int64_t bf16_wgrad_kchunk(int64_t M, int64_t tiles, int64_t max_splits) {
    int64_t s = cdiv(1024, tiles > 0 ? tiles : 1);
    const int64_t smax = cdiv(M, 4 * B16_BK);
    if (s > smax) s = smax;
    if (s > max_splits) s = max_splits;
    if (s < 1) s = 1;
    return cdiv(cdiv(M, s), B16_BK) * B16_BK;
}

// weight-gradient problems (dW = dZ^T X layout: both operands contraction-strided) as grouped launches of <= GEMM_GROUP_MAX
template <int PL>
static inline void launch_wgrad_bf16_v(const GemmGroup& grp, unsigned blocks, int va, int vb, hipStream_t s) {
    if (va && vb) CDLRM_LAUNCH_EV((k_gemm_bf16_group<true, true, PL>), dim3(blocks), dim3(256), 0, s, grp);
    else if (va) CDLRM_LAUNCH_EV((k_gemm_bf16_group<true, false, PL>), dim3(blocks), dim3(256), 0, s, grp);
    else if (vb) CDLRM_LAUNCH_EV((k_gemm_bf16_group<false, true, PL>), dim3(blocks), dim3(256), 0, s, grp);
    else CDLRM_LAUNCH_EV((k_gemm_bf16_group<false, false, PL>), dim3(blocks), dim3(256), 0, s, grp);
}

static inline int launch_wgrad_bf16(const GemmArgs* probs, int n, int va, int vb, int planes, hipStream_t s) {
    for (int q0 = 0; q0 < n; q0 += GEMM_GROUP_MAX) {
        GemmGroup grp;
        memset(&grp, 0, sizeof(grp));
        unsigned blocks = 0;
        for (int q = q0; q < n && q < q0 + GEMM_GROUP_MAX; ++q) {
            grp.first[grp.n] = blocks;
            grp.g[grp.n] = probs[q];
            blocks += (unsigned)(cdiv(probs[q].M, 64) * cdiv(probs[q].N, 64) * cdiv(probs[q].K, probs[q].kchunk));
            grp.n++;
        }
        grp.first[grp.n] = blocks;
        if (planes == 2) launch_wgrad_bf16_v<2>(grp, blocks, va, vb, s);
        else launch_wgrad_bf16_v<1>(grp, blocks, va, vb, s);
    }
    CDLRM_LAUNCH_CHECK();
    return 0;
}
