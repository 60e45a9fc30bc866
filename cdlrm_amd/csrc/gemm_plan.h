// Which kernel a dense GEMM goes to, decided in ONE place: gemm_plan turns a problem (GemmArgs) into a GemmPlan, gemm_launch
// launches from that value, the route queries copy its route out.  A new kernel is one more case in each of the two.
// Included behind every kernel header and behind the forward's two vector-ALU kernels and their launcher (dense.hip).
#pragma once
#include "gemm_wide.h"
#include "gemm_bf16.h"

// The plan of one problem in layout <A_KC, B_KC>: forward <true, true>, dgrad <true, false>, weight gradient <false, false>.
// splits: contraction slabs (g.kchunk long); planes: 0 fp32, 1 / 2 the caller's CDLRM_GEMM_BF16 / _BF16X3 mode; n_cu: the
// compute-unit count the wide kernel's rule is evaluated for.  Pure: no HIP call, no static state, pointers looked at for their
// alignment only.  The fields of g that depend on the choice -- vecA, vecB, vecC, kchunk -- are set for the kernel chosen.
template <bool A_KC, bool B_KC>
static GemmPlan gemm_plan(GemmArgs& g, int splits, int planes, int n_cu) {
    GemmPlan p;
    memset(&p, 0, sizeof(p));
    // the epilogue operands -- bias, activation mask -- are 16-byte loadable (or absent)
    const bool vbias = g.bias == nullptr || aligned16(g.bias);
    const bool vmask = g.mask_act == 0 || (aligned16(g.mask) && g.ldmask % 4 == 0);

    // ---- the opt-in bf16 / bf16x3 modes (gemm_bf16.h): the layers the shape rule admits, 16-byte flags from the operands -------
    if (planes && (A_KC ? bf16_layer_ok(g.N, g.K) : bf16_layer_ok(g.M, g.N))) {
        g.vecA = bf16_vec<A_KC>(g.A, g.lda, g.M, g.K);
        g.vecB = bf16_vec<B_KC>(g.B, g.ldb, g.N, g.K);
        int tm = 1, tn = 1;
        if (A_KC) {     // an un-split forward / dgrad
            g.kchunk = g.K;
            splits = 1;
            bf16_pick_tile(g.M, g.N, planes, &tm, &tn);
        }               // (the weight gradient: the grouped kernel's 64x64 tiles over the caller's slabs, bf16_wgrad_kchunk)
        p.r = {bf16_family(planes), tm, tn, 0, 0, splits, g.vecA, g.vecB, 0};
        p.grid = gemm_grid(g, 64 * tm, 64 * tn, splits);
        return p;
    }

    // ---- the forward's short contractions on the vector ALU (dense.hip) ----------------------------------------------------------
    if constexpr (A_KC && B_KC) {
        const bool fwd = splits == 1 && g.ldb == g.K && g.mask_act == 0;      // what cdlrm_linear_fwd passes
        // (Round 6, measured and removed: this layer on the matrix cores -- a wave owning 16 rows x 256 columns, the weights as
        //  16x16x4 fragments in registers, ascending k, bit-identical -- 10.9 us alone against 8.6 for the register kernel below at
        //  M = 8192 (64 scattered 4-byte weight loads per lane for 64 MFMAs), 0.5542 against 0.5519 ms per c3 step.)
        const int64_t blocks = cdiv(g.M, smallk_rows_per_wg(g.M)) * (g.N >> 8);       // of k_linear_smallk_rows
        if (fwd && g.K == 13 && g.N % 256 == 0 && g.ldc % 4 == 0 && aligned16(g.C) && vbias && g.M >= 256 && !g_cdlrm_debug[0] &&
            blocks <= 0x7fffffff) {
            p.r = {CDLRM_ROUTE_SMALLK_ROWS, 0, 0, 0, 0, 1, 0, 0, 0};
            p.grid = dim3((unsigned)blocks);
            return p;
        }
        if (fwd && g.K <= SK_KMAX && g.N % 4 == 0 && g.ldc % 4 == 0 && aligned16(g.C) && cdiv(g.M, 32) <= 65535) {
            p.r = {CDLRM_ROUTE_SMALLK, 0, 0, 0, 0, 1, 0, 0, 0};
            p.grid = dim3((unsigned)cdiv(g.N, 128), (unsigned)cdiv(g.M, 32));
            return p;
        }
    }

    // ---- fp32 on the matrix cores ------------------------------------------------------------------------------------------------
    if (g.K < 4) g.vecA = g.vecB = 0;
    const int64_t kc = g.kchunk < g.K ? g.kchunk : g.K;

    // The wide kernel (gemm_wide.h: k_gemm3, one workgroup per CU) takes the un-split forward / dgrad GEMMs whose tiles fill the
    // chip: where the 128x128 tiles fill whole rounds of one workgroup per CU (>= 90 % of the slots of the last round too: c3's
    // 512-wide layers at M = 8192 are exactly 256 tiles, c5's 2048 and 1024) -- measured against k_gemm2 on one box
    // (tools/gemm3_bench.hip, profiles/r06_gemm3_vs_gemm2.txt).  Returns IM (4: 128x128, 2: 64x128 tiles), 0: not taken.
    auto wide = [&]() -> int {
        if constexpr (!A_KC && B_KC) return 0;
        // Only for launches the caller marks as running ALONE (CDLRM_GEMM_ALONE: the top MLP's forward and its dgrad chain in the
        // training step).  Beside the weight-gradient GEMMs of the side queues a workgroup of this kernel (96 KB of LDS, 340
        // registers per lane) waits for a CU to drain: the bottom MLP's 512 <- 256 dgrad took 115.6 us there against 62.9 on
        // k_gemm2's 1024 small workgroups, the c3 step 0.5790 against 0.5580 ms (profiles/r06_ab_gemm3_in_step.txt).
        // cdlrm_debug_set(6, 32): never; (6, 256): every eligible launch (the stand-alone benches).
        if (g_cdlrm_debug[6] & 32) return 0;
        if (!A_KC && (g_cdlrm_debug[6] & 512)) {
            // (A/B: the split-M weight gradients on this kernel)
        } else if (!A_KC && (g_cdlrm_debug[6] & 1024) && (int64_t)g.M * g.N >= 512 * 480) {
            // (A/B: the two 512-wide ones only)
        } else if (!g.alone && !(g_cdlrm_debug[6] & 256)) return 0;
        if ((A_KC && splits != 1) || kc < 2 * G3_BK || !gemm3_applies<A_KC, B_KC>(g) || n_cu <= 0) return 0;
        // 128x128 tiles where they fill whole rounds of one workgroup per CU (>= 90 % of the last round's slots), else 64x128 tiles
        // under the same rule (M = 8192 x 256-wide layers, per-rank batches of 4096 x 512-wide: 256 tiles)
        auto fills = [&](int64_t tiles) { return tiles * 10 >= cdiv(tiles, n_cu) * n_cu * 9; };
        const int64_t t128 = cdiv(g.M, 128) * cdiv(g.N, 128) * splits, t64 = cdiv(g.M, 64) * cdiv(g.N, 128) * splits;
        // (short contractions, K <= 256, on k_gemm2's 64x64 tiles instead: c3 step 0.5594 against 0.5558 ms; on the 64x128 tiles: a tie)
        // (ragged tiles -- N = 480: a quarter of the tiles take the generic epilogue behind the loop -- only where every CU has ONE
        //  tile: at M = 65536 the 480 <- 512 dgrad took 333 us here against 304 on k_gemm2, at M = 8192 44.4 against 47.2)
        if ((g.N % 128 != 0 || g.M % 64 != 0) && t128 > n_cu) return 0;
        return fills(t128) ? 4 : A_KC && fills(t64) ? 2 : 0;
    };
    if (const int im = wide()) {
        // tiles inside the matrix finish under the last group's MFMAs where the epilogue operands are 16-byte loadable (k_gemm3 `fast`)
        p.r = {CDLRM_ROUTE_GEMM3, im, 4, 0, 0, splits, 1, 1, vbias && vmask};
        p.grid = gemm_grid(g, 32 * im, 128, splits);
        return p;
    }

    const bool dma = gemm2_applies<A_KC, B_KC>(g);
    // (long batches with a narrow output -- the 256 -> 128 layer at M = 8192, forward: 256 tiles of 64x64, and its weight
    //  gradient: 8 tiles x 32 slabs of the batch -- are better off on the LDS-DMA kernel's 64x64 tile than on the LDS-free
    //  one: 10.3 against 13.1 us forward)
    const bool long_narrow = (g.M >= 4096 || g.K >= 4096) && cdiv(g.M, 64) * cdiv(g.N, 64) * splits >= 256 && dma;
    // a 13-wide (or 1-wide) side that the DMA kernel cannot load: the LDS-free kernel's 32x32 tiles waste less of the
    // MFMA than the 64x64 staged tile, whatever the number of slabs (the 512 x 13 weight gradient at M = 65536, 128
    // slabs: 1100 us on the tiled kernel, c5's longest launch)
    const bool thin = !dma && (g.N <= 32 || g.M <= 32);
    if ((gemm_use_direct(g.M, g.N, splits) && !long_narrow) || thin) {
        // the 32x32-tile kernels: staged (16-byte loads throughout), the aligned loader (16-byte loads on the
        // contraction-contiguous operands), the generic one (va / vb: only contraction-contiguous operands use 16-byte loads)
        g.vecC = direct_vec_c(g);
        const DirectVariant v = direct_variant<A_KC, B_KC>(g);
        const bool va = A_KC && g.vecA, vb = B_KC && g.vecB;
        // direct_prefetch's launch-wide conditions (a thread also needs its float4 inside the matrix)
        const int pre = g.fastep && g.vecC && vbias && vmask;
        p.r = {v.staged ? CDLRM_ROUTE_STAGED : CDLRM_ROUTE_DIRECT, 0, 0, v.mode, v.staged || v.aligned, splits,
               v.staged ? 1 : v.aligned ? A_KC : va, v.staged ? 1 : v.aligned ? B_KC : vb, pre};
        p.grid = gemm_grid(g, 32, 32, splits);
        p.lds = v.staged ? ST_LDS_BYTES : 0;
        return p;
    }
    if (dma) {
        // LDS-DMA kernel.  Measured on the c3 layer shapes (tools/gemm2_bench.hip, M = 8192, all three layouts): 128x64
        // tiles win wherever they leave MORE than one workgroup per CU (512-wide layers 40-42 us against 43-47 for 64x64), the
        // 64x64 tile from there down (128-wide output: 9.9 against 14.3 us).  At exactly one per CU -- the 256-wide layers at
        // M = 8192: top forward 512 -> 256, bottom forward 512 -> 256, bottom dgrad 256 <- 128 -- 512 workgroups of 64x64 beat
        // 256 of 128x64 in the step: 0.5740 against 0.5767 ms, six rounds of 110 steps each, every round (round 4; bit-identical:
        // a tile's k order does not depend on its shape)
        int tm2 = 2, tn2 = 1;
        if (g.M <= 64 || cdiv(g.M, 128) * cdiv(g.N, 64) * splits <= 256) tm2 = 1;
        // ... and so do the short contractions (K <= 256 un-split: the dgrads 512 <- 256 of both sub-networks, eight K tiles per
        // workgroup, where prologue and store tail weigh most): 1024 workgroups of 64x64 instead of 512 of 128x64, 0.5681 against
        // 0.5739 ms per c3 step, six rounds, every round.  (EVERY forward / dgrad on 64x64: 0.5776 against 0.5747; the weight
        // gradients too: 0.5819 / 0.5863 -- the 512-wide layers keep 128x64.)
        if (splits == 1 && g.K <= 256) tm2 = 1;
        // ... and where a CU gets >= 4 tiles of 128x128 (un-split forward / dgrad at M = 65536: c5) that shape, one workgroup per
        // CU, a third less LDS fill per MFMA: stand-alone 297.5 against 313.7 us (512 x 512 forward), 283.1 / 297.7 (512 <- 480),
        // 158.7 / 165.9 (256 <- 512), dgrad 318.0 / 322.5 (profiles/r05_gemm_big_tiles.txt); in the c5 step 3.6927 against
        // 3.7159 ms, ten rounds (-0.6 %; cdlrm_debug_set(6, 16): 128x64 as before).  Bit-identical (a tile's k order does not
        // depend on its shape).  At M = 8192 the same shape is one tile per CU and loses (round 2, and again in round 5).
        if (!(g_cdlrm_debug[6] & 16) && A_KC && splits == 1 && tm2 == 2 && cdiv(g.M, 128) * cdiv(g.N, 128) >= 1024) tn2 = 2;
        // (the same shape for the split-M weight gradients of a long batch: a tie, c5 3.7017 against 3.6995 ms, ten rounds -- not taken)
        // full tiles of an un-split forward / dgrad take g2_epilogue_full where g2_full_ok holds (gemm2_tile_body)
        p.r = {CDLRM_ROUTE_GEMM2, tm2, tn2, 0, 0, splits, 1, 1, A_KC && splits == 1 && g2_full_ok<B_KC>(g)};
        p.grid = gemm_grid(g, 64 * tm2, 64 * tn2, splits);
        p.lds = (unsigned)G2_EXTRA_LDS(tm2, tn2);
        return p;
    }
    // the register-staged kernel
    int tm, tn;
    gemm_pick_tile(g.M, g.N, splits, &tm, &tn);
    if (tm == 2 && tn == 1) { tm = 1; tn = g.N <= 64 ? 1 : 2; }     // 128x64 is never the best shape here
    // vector loads also need extents >= 4 in the vectorised direction (clamped addresses must stay inside)
    if (!A_KC && g.M < 4) g.vecA = 0;
    if (!B_KC && g.N < 4) g.vecB = 0;
    p.r = {CDLRM_ROUTE_GEMM, tm, tn, 0, 0, splits, g.vecA, g.vecB, 0};
    p.grid = gemm_grid(g, 64 * tm, 64 * tn, splits);
    return p;
}

// Launch what the plan says.  The kernels that can carry a completion event (CDLRM_LAUNCH_EV) do so inside their launchers.
template <bool A_KC, bool B_KC>
static int gemm_launch(const GemmPlan& p, const GemmArgs& g, hipStream_t s) {
    const cdlrm_gemm_route& r = p.r;
    const int tile = 10 * r.tm + r.tn;
    switch (r.family) {
    case CDLRM_ROUTE_SMALLK_ROWS:
    case CDLRM_ROUTE_SMALLK:
        if constexpr (A_KC && B_KC) launch_linear_smallk(p, g, s);
        break;
    case CDLRM_ROUTE_GEMM3:
        if constexpr (A_KC || !B_KC) {
            if (r.tm == 4) launch_gemm3<A_KC, B_KC, 4, 4, 3>(g, p.grid, s);
            else launch_gemm3<A_KC, B_KC, 2, 4, 3>(g, p.grid, s);
        }
        break;
    case CDLRM_ROUTE_GEMM2: launch_gemm2<A_KC, B_KC>(g, r.tm, r.tn, p.grid, p.lds, s); break;
    case CDLRM_ROUTE_STAGED: launch_gemm_staged<A_KC, B_KC>(g, p.grid, r.mode, s); break;
    case CDLRM_ROUTE_DIRECT: launch_gemm_direct<A_KC, B_KC>(p, g, s); break;
    case CDLRM_ROUTE_GEMM:
        if (tile == 22) launch_gemm_v<A_KC, B_KC, 2, 2>(g, p.grid, s);
        else if (tile == 12) launch_gemm_v<A_KC, B_KC, 1, 2>(g, p.grid, s);
        else launch_gemm_v<A_KC, B_KC, 1, 1>(g, p.grid, s);
        break;
    case CDLRM_ROUTE_BF16:
    case CDLRM_ROUTE_BF16X3:
        if constexpr (!A_KC) return launch_wgrad_bf16(&g, 1, g.vecA, g.vecB, r.family == CDLRM_ROUTE_BF16X3 ? 2 : 1, s);
        else if (r.family == CDLRM_ROUTE_BF16X3) {
            if (tile == 12) launch_gemm_bf16_v<A_KC, B_KC, 1, 2, 2>(g, p.grid, s);
            else launch_gemm_bf16_v<A_KC, B_KC, 1, 1, 2>(g, p.grid, s);
        } else if (tile == 22) launch_gemm_bf16_v<A_KC, B_KC, 2, 2, 1>(g, p.grid, s);
        else if (tile == 12) launch_gemm_bf16_v<A_KC, B_KC, 1, 2, 1>(g, p.grid, s);
        else launch_gemm_bf16_v<A_KC, B_KC, 1, 1, 1>(g, p.grid, s);
        break;
    default: CDLRM_REQUIRE(false, "no kernel for this plan");
    }
    CDLRM_LAUNCH_CHECK();
    return 0;
}
