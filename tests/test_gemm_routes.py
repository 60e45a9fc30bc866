"""Every dense GEMM route of cdlrm_linear_fwd / cdlrm_linear_bwd against a plain float64 reference.

gemm_plan (csrc/gemm_plan.h: the matrix-core kernels and the forward's small-K kernels of dense.hip) sends an MLP
GEMM to one of seven kernel families by shape, alignment, split count, the CDLRM_GEMM_ALONE hint and the CU count; each family has
its own epilogue code for the bias, the activation and the dgrad's fused activation mask (x_act).  One table of cases below, each
with the route it is meant to reach, serves three checks:

  * CPU: ops.linear_fwd_route / linear_bwd_route (the same decision code, nothing launched) at MI355X's 256 CUs give the declared
    route, on integer addresses with the alignment facts of the GPU case;
  * CPU: one TrainEngine step per configuration (c2 and c3 / c5 layer shapes, per-rank batches 1024 ... 65536, tests/fake_ops.py)
    records the step's real linear_fwd / linear_bwd arguments; every route they resolve to, with its epilogue arguments, is in the
    table -- an engine or threshold change that sends the step to an untested route fails here;
  * GPU: each case asks the route with the device's real CU count, asserts it, runs the kernel and compares every element with
    |got - ref| <= C * K_eff * 2^-24 * (|A| @ |B|)_ij (+ 8 ulp of the reference for the activation, + a denormal floor), the
    rigorous bound of an fp32 fma chain of length K_eff (the contraction length; for a split weight gradient the slab length plus
    the number of slabs).  A mask on the wrong row, a dropped K tile or slab, a wrong pitch moves an element by O(its magnitude).

Pitch gaps of the inputs hold NaN (a kernel that reads the gap poisons its output), the gaps of the outputs a sentinel that must
survive.  The comparator itself is checked on the CPU with numpy negative controls.
"""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
N_CU_MI355X = 256
U = 2.0 ** -24
C_BOUND = 2.0           # one constant for every case: 1 is the rigorous bound of a length-K_eff fp32 chain, 2 leaves slack
TINY = 1e-30
SENTINEL = 12345.0

# ---- routes as short strings ----------------------------------------------------------------------------------------------


def route_str(r):
    """ops.linear_*_route's dict -> 'gemm3 4x4 fast', 'gemm2 128x64 /16', 'direct m1 v10', 'staged m2 fast', ... (None: no launch)."""
    if r is None:
        return None
    f = r["family"]
    if f in ("smallk_rows", "smallk"):
        s = f
    elif f == "direct":
        s = "direct m%d %s" % (r["mode"], "al" if r["aligned"] else "v%d%d" % (r["vec_a"], r["vec_b"]))
    elif f == "staged":
        s = "staged m%d" % r["mode"]
    elif f == "gemm2":
        s = "gemm2 %dx%d" % (64 * r["tm"], 64 * r["tn"])
    elif f == "gemm3":
        s = "gemm3 %dx%d" % (r["tm"], r["tn"])
    else:
        s = "gemm %dx%d v%d%d" % (r["tm"], r["tn"], r["vec_a"], r["vec_b"])
    if r["splits"] > 1:
        s += " /%d" % r["splits"]
    if r["fast"]:
        s += " fast"
    return s


def tile_of(route):
    """Output tile (rows, cols) of a route string, for failure reports."""
    fam = route.split()[0]
    if fam in ("gemm2", "gemm"):
        tm, tn = route.split()[1].split("x")[:2]
        return (int(tm), int(tn)) if fam == "gemm2" else (64 * int(tm), 64 * int(tn[0]))
    if fam == "gemm3":
        tm, tn = route.split()[1].split("x")
        return 32 * int(tm), 32 * int(tn)
    if fam == "smallk":
        return 32, 128
    if fam == "smallk_rows":
        return 1, 256
    return 32, 32


# ---- the case table -------------------------------------------------------------------------------------------------------

class Case:
    """One GEMM call and the route it must take.  fwd: Y = act(X W^T + b) for every act in `acts` and bias in `biases`.  bwd:
    dZ = dY * act'(Y) in place (act), dX = (dZ W) * x_act'(X) for every x_act in `x_acts`, dW = dZ^T X and db when `dW`.
    ld*: row pitches (default: the width), off*: element offsets from a 256-byte aligned base (the 16-byte alignment facts),
    debug: cdlrm_debug_set(6, debug) around the call."""

    def __init__(self, cid, op, M, N, K, route, acts=(0, 1, 2), biases=(True, False), x_acts=(0, 1, 2), act=0, dX=True, dW=False,
                 alone=False, ldx=None, ldy=None, lddx=None, offx=0, offw=0, offb=0, offy=0, offdx=0, debug=0):
        self.id, self.op, self.M, self.N, self.K = cid, op, M, N, K
        self.route = route                       # fwd: str; bwd: (dgrad, wgrad), None where no launch
        self.acts, self.biases, self.x_acts, self.act, self.dX, self.dW = acts, biases, x_acts, act, dX, dW
        self.alone, self.debug = alone, debug
        self.ldx, self.ldy, self.lddx = ldx or K, ldy or N, lddx or K
        self.offx, self.offw, self.offb, self.offy, self.offdx = offx, offw, offb, offy, offdx

    def __repr__(self):
        return self.id

    def variants(self):
        if self.op == "fwd":
            return [dict(act=a, bias=b) for a in self.acts for b in self.biases]
        return [dict(x_act=xa) for xa in (self.x_acts if self.dX else (0,))]

    def keys(self):
        """(direction, route, epilogue arguments, strided operands) of every variant: what the step's calls are matched with."""
        out = []
        for v in self.variants():
            if self.op == "fwd":
                out.append(("fwd", self.route, v["act"], v["bias"], self.ldx != self.K, self.ldy != self.N))
            else:
                out.append(("bwd", self.route, self.act, v["x_act"] if self.dX else None, self.dW, self.ldx != self.K,
                            self.ldy != self.N, self.lddx != self.K if self.dX else None))
        return out


F = lambda cid, M, N, K, route, **kw: Case(cid, "fwd", M, N, K, route, **kw)     # noqa: E731
B = lambda cid, M, N, K, route, **kw: Case(cid, "bwd", M, N, K, route, **kw)     # noqa: E731
PITCH_FEAT = 27 * 128           # the engine's feat[:, 0, :] at c3 / c5 (27 features x D = 128): Y of the bottom MLP's last layer
PITCH_FEAT_C2 = 27 * 32         # ... at c2 (D = 32)

CASES = [
    # ---- small K: the vector-ALU forward kernels ----
    F("smallk_rows_c3", 8192, 512, 13, "smallk_rows", alone=True),
    F("smallk_rows_ragged", 1000, 256, 13, "smallk_rows"),
    F("smallk", 1030, 200, 5, "smallk"),
    F("smallk_k32_pitch", 777, 132, 32, "smallk", ldx=33, ldy=136),
    # ---- LDS-free direct kernel: modes 0/1/2, aligned loader and generic one with each vec combination ----
    F("direct_m0_al", 300, 70, 32, "direct m0 al"),
    F("direct_m0_v11", 1000, 70, 36, "direct m0 v11"),
    F("direct_m1_v11", 1000, 96, 400, "direct m1 v11 fast"),
    F("direct_m2_v00", 640, 132, 601, "direct m2 v00 fast"),
    F("direct_m0_v01", 300, 70, 64, "direct m0 v01", ldx=65),
    F("direct_m1_v10", 300, 70, 400, "direct m1 v10", offw=1),
    F("direct_m2_v11_unaligned_y", 500, 128, 600, "direct m2 v11", ldy=130),
    F("staged_m0_thin_n", 8192, 1, 256, "staged m0"),
    B("dgrad_direct_m0_al", 1000, 256, 70, ("direct m0 al", None)),
    B("dgrad_direct_m1_al", 1000, 512, 70, ("direct m1 al", None)),
    B("dgrad_direct_m2_al", 700, 1024, 70, ("direct m2 al", None), x_acts=(1, 2)),
    B("dgrad_direct_c2_feat", 2048, 32, 256, ("direct m0 al fast", None), x_acts=(1,), ldy=PITCH_FEAT_C2, alone=False),
    B("dgrad_direct_unaligned", 900, 100, 130, ("direct m0 v00", None), ldx=131, ldy=101),
    B("wgrad_direct", 1000, 256, 70, (None, "direct m2 v00"), dX=False, dW=True),
    B("wgrad_direct_thin", 2048, 512, 13, ("direct m1 al", "direct m2 al"), dW=True, x_acts=(0,)),
    # ---- staged kernel ----
    F("staged_m0", 1024, 128, 256, "staged m0 fast", ldy=PITCH_FEAT),
    F("staged_m1", 1024, 512, 480, "staged m1 fast", alone=True),
    F("staged_m2", 600, 256, 1024, "staged m2 fast"),
    B("dgrad_staged_m0", 1024, 128, 256, ("staged m0 fast", None), ldy=PITCH_FEAT, x_acts=(1, 2)),
    B("dgrad_staged_m0_plain", 1024, 256, 512, ("staged m0 fast", None), alone=True),
    B("dgrad_staged_m1", 1024, 512, 480, ("staged m1 fast", None), alone=True),
    B("dgrad_staged_m1_act", 1000, 512, 256, ("staged m1 fast", "direct m2 v00 fast"), act=1, dW=True, x_acts=(1,)),
    B("dgrad_staged_act_sig", 1000, 512, 256, ("staged m1 fast", "direct m2 v00 fast"), act=2, dW=True, x_acts=(2,)),
    # ---- k_gemm2 (LDS-DMA) ----
    F("gemm2_64", 2048, 512, 480, "gemm2 64x64 fast", alone=True),
    F("gemm2_64_feat", 8192, 128, 256, "gemm2 64x64 fast", ldy=PITCH_FEAT, alone=True),
    F("gemm2_64_ragged", 8200, 264, 64, "gemm2 64x64 fast"),
    F("gemm2_128x64", 8192, 512, 512, "gemm2 128x64 fast"),
    F("gemm2_128x64_ragged", 6400, 500, 480, "gemm2 128x64 fast"),
    F("gemm2_128x128_c5", 65536, 512, 480, "gemm2 128x128 fast"),
    B("dgrad_gemm2_64", 2048, 512, 480, ("gemm2 64x64 fast", None), alone=True),
    B("dgrad_gemm2_64_feat", 8192, 128, 256, ("gemm2 64x64 fast", None), ldy=PITCH_FEAT),
    B("dgrad_gemm2_64_ragged", 8256, 256, 100, ("gemm2 64x64 fast", None)),
    B("dgrad_gemm_1x1_ragged", 8256, 264, 96, ("gemm 1x1 v11", None)),
    B("dgrad_gemm2_128x64", 8192, 512, 384, ("gemm2 128x64 fast", None), alone=True),
    B("dgrad_gemm2_128x64_ragged", 6400, 480, 500, ("gemm2 128x64 fast", None)),
    B("dgrad_gemm2_mask_pitch", 8192, 256, 512, ("gemm2 64x64", None), ldx=514, x_acts=(1, 2)),
    B("dgrad_gemm2_128x128_c5", 65536, 512, 480, ("gemm2 128x128 fast", None), alone=True, x_acts=(0, 1)),
    B("wgrad_gemm2_split", 8192, 512, 512, (None, "gemm2 128x64 /16"), dX=False, dW=True),
    B("wgrad_gemm2_split_ragged", 16384, 256, 480, ("gemm2 64x64 fast", "gemm2 128x64 /32"), dW=True, x_acts=(1,)),
    # ---- k_gemm3 (wide): 4x4 / 2x4, edge tiles in M and in N, wgrad layout through the development selector ----
    F("gemm3_4x4", 8192, 512, 512, "gemm3 4x4 fast", alone=True),
    F("gemm3_4x4_edge_m", 8100, 512, 96, "gemm3 4x4 fast", alone=True),
    F("gemm3_4x4_edge_n", 8192, 480, 512, "gemm3 4x4 fast", alone=True),
    F("gemm3_4x4_feat", 8192, 512, 256, "gemm3 4x4 fast", ldy=PITCH_FEAT, alone=True),
    F("gemm3_2x4", 4096, 512, 480, "gemm3 2x4 fast", alone=True),
    F("gemm3_2x4_c3", 8192, 256, 512, "gemm3 2x4 fast", alone=True),
    F("gemm3_4x4_bias_unaligned", 8192, 512, 512, "gemm3 4x4", alone=True, offb=1, biases=(True,)),
    B("dgrad_gemm3_4x4", 8192, 512, 512, ("gemm3 4x4 fast", None), alone=True),
    B("dgrad_gemm3_4x4_edge_n", 8192, 512, 480, ("gemm3 4x4 fast", None), alone=True),
    B("dgrad_gemm3_2x4_edge_m", 16300, 512, 96, ("gemm3 2x4 fast", None), alone=True),
    B("dgrad_gemm3_2x4", 4096, 512, 512, ("gemm3 2x4 fast", None), alone=True),
    B("dgrad_gemm3_mask_pitch", 8192, 512, 512, ("gemm3 4x4", None), alone=True, ldx=513, x_acts=(1, 2)),
    B("dgrad_gemm3_padded_dx", 8192, 512, 480, ("gemm3 4x4 fast", None), alone=True, lddx=484, x_acts=(0,)),
    B("wgrad_gemm3_selector", 8192, 512, 480, (None, "gemm3 4x4 /16 fast"), dX=False, dW=True, debug=512),
    # ---- register-staged k_gemm: 1x1 / 1x2 / 2x2, every vec combination, the wgrad layout ----
    F("gemm_1x1_v00", 4096, 512, 479, "gemm 1x1 v00"),
    F("gemm_1x1_v11", 4096, 512, 100, "gemm 1x1 v11"),
    F("gemm_1x1_v10", 4096, 512, 96, "gemm 1x1 v10", offw=2),
    F("gemm_1x1_v01", 4096, 512, 96, "gemm 1x1 v01", ldx=97),
    F("gemm_1x2_v11", 16384, 512, 100, "gemm 1x2 v11", acts=(1,)),
    F("gemm_2x2_v11", 32768, 512, 100, "gemm 2x2 v11", acts=(2,), biases=(True,)),
    B("dgrad_gemm_1x1", 8192, 100, 512, ("gemm 1x1 v11", None)),
    B("dgrad_gemm_1x1_v01", 4096, 99, 512, ("gemm 1x1 v01", None), x_acts=(1, 2)),
    B("dgrad_gemm_1x1_v00", 4096, 99, 510, ("gemm 1x1 v00", None), x_acts=(0, 1)),
    B("wgrad_gemm_split", 8100, 512, 96, ("staged m1 fast", "gemm 1x1 v11 /32"), dW=True, alone=True, x_acts=(1,)),
]


# ---- realising a case: on the device, or as integer addresses for the route query ---------------------------------------

class Addr:
    """Stand-in for a tensor in a route query: shape, row pitch, address (256-byte aligned base + offset)."""

    def __init__(self, rows, cols, ld, off):
        self.shape, self._ld, self._p = (rows, cols), ld, (1 << 32) + 4 * off

    def stride(self, i=0):
        return self._ld if i == 0 else 1

    def data_ptr(self):
        return self._p


def _query(ops, case, v, mk, n_cu):
    """Route of one variant; mk(rows, cols, ld, off) builds an operand."""
    c = case
    X = mk(c.M, c.K, c.ldx, c.offx)
    W = mk(c.N, c.K, c.K, c.offw)
    if c.op == "fwd":
        b = mk(1, c.N, c.N, c.offb) if v["bias"] else None
        return route_str(ops.linear_fwd_route(X, W, b, mk(c.M, c.N, c.ldy, c.offy), v["act"], alone=c.alone, n_cu=n_cu))
    Y = mk(c.M, c.N, c.ldy, c.offy)
    dY = mk(c.M, c.N, c.ldy, c.offy)
    dX = mk(c.M, c.K, c.lddx, c.offdx) if c.dX else None
    dW = mk(c.N, c.K, c.K, 0) if c.dW else None
    db = mk(1, c.N, c.N, 0) if c.dW else None
    r = ops.linear_bwd_route(X, W, Y if c.act else None, dY, dX, dW, db, c.act, x_act=v["x_act"], alone=c.alone, n_cu=n_cu)
    return tuple(route_str(x) for x in r)


class _debug6:
    def __init__(self, value):
        self.value = value

    def __enter__(self):
        from cdlrm_amd import _lib
        if self.value:
            assert _lib.raw().cdlrm_debug_set(6, self.value) == 0

    def __exit__(self, *exc):
        from cdlrm_amd import _lib
        if self.value:
            assert _lib.raw().cdlrm_debug_set(6, 0) == 0


@pytest.fixture(scope="module")
def ops():
    from cdlrm_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        sys.path.insert(0, ROOT)
        import __graft_entry__ as g
        g.build()
    _lib.lib()
    from cdlrm_amd import ops as _ops
    return _ops


# ---- comparator ---------------------------------------------------------------------------------------------------------

def assert_within(got, ref, mag, k_eff, what, route="direct", act_ulps=8.0):
    """|got - ref| <= C_BOUND * k_eff * 2^-24 * mag + act_ulps * 2^-24 * |ref| + TINY element by element (NaN fails); on failure
    the worst element with its row, column and output tile."""
    got = np.asarray(got, dtype=np.float64)
    ref = np.asarray(ref, dtype=np.float64)
    bound = C_BOUND * k_eff * U * np.asarray(mag, dtype=np.float64) + act_ulps * U * np.abs(ref) + TINY
    err = np.abs(got - ref)
    ok = err <= bound
    if ok.all():
        return
    ratio = np.where(np.isnan(err), np.inf, err / bound)
    i = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
    tr, tc = tile_of(route)
    rc = (i[0], i[1]) if len(i) == 2 else (0, i[0])
    raise AssertionError("%s: %d of %d elements outside the bound; worst at row %d, col %d (tile %d, %d of %dx%d, %s): got %r, "
                         "want %r, |err| %.3g > bound %.3g (K_eff %d)" % (
                             what, int((~ok).sum()), ok.size, rc[0], rc[1], rc[0] // tr, rc[1] // tc, tr, tc, route,
                             float(got[i]), float(ref[i]), float(err[i]), float(bound[i]), k_eff))


def act_fwd(v, act):
    return {0: v, 1: np.maximum(v, 0.0), 2: 1.0 / (1.0 + np.exp(-v))}[act]


def act_grad(y, act):
    """act'(pre-activation) from the activation OUTPUT y (threshold_backward / sigmoid_backward)."""
    return {0: np.ones_like(y), 1: (y > 0).astype(np.float64), 2: (1.0 - y) * y}[act]


# ---- CPU: the comparator's negative controls ---------------------------------------------------------------------------

def _seq_fp32(A, Bm, skip=None):
    """fp32 sequential multiply-add over k (a correct, un-fused fp32 GEMM), optionally without contraction indices `skip`."""
    acc = np.zeros((A.shape[0], Bm.shape[1]), dtype=np.float32)
    for k in range(A.shape[1]):
        if skip is not None and k in skip:
            continue
        acc = (acc + A[:, k:k + 1] * Bm[k:k + 1, :]).astype(np.float32)
    return acc


def test_comparator_negative_controls():
    """A correct fp32 computation passes the bound; a mask shifted by one row, a dropped K tile of 32, a bias added twice and the
    sigmoid mask in place of the ReLU one each fail it."""
    rng = np.random.RandomState(3)
    M, N, K = 64, 48, 256
    A = rng.randn(M, K).astype(np.float32)
    Bm = (rng.randn(K, N) / np.sqrt(K)).astype(np.float32)
    bias = rng.randn(N).astype(np.float32)
    Xm = np.maximum(rng.randn(M, N), 0).astype(np.float32)          # a ReLU output: the dgrad's mask operand
    A64, B64 = A.astype(np.float64), Bm.astype(np.float64)
    mag = np.abs(A64) @ np.abs(B64)
    # forward with bias
    ref_f = A64 @ B64 + bias
    got_f = (_seq_fp32(A, Bm) + bias).astype(np.float32)
    assert_within(got_f, ref_f, mag + np.abs(bias), K + 1, "correct forward")
    with pytest.raises(AssertionError, match="worst at row"):
        assert_within(got_f + bias, ref_f, mag + np.abs(bias), K + 1, "bias twice")
    with pytest.raises(AssertionError):
        assert_within((_seq_fp32(A, Bm, skip=set(range(96, 128))) + bias).astype(np.float32), ref_f, mag + np.abs(bias), K + 1,
                      "K tile dropped")
    # dgrad with the ReLU mask
    m = act_grad(Xm.astype(np.float64), 1)
    ref_d = (A64 @ B64) * m
    acc = _seq_fp32(A, Bm)
    assert_within(np.where(Xm > 0, acc, 0).astype(np.float32), ref_d, mag * m, K + 2, "correct dgrad")
    with pytest.raises(AssertionError):
        assert_within(np.where(np.roll(Xm, 1, axis=0) > 0, acc, 0).astype(np.float32), ref_d, mag * m, K + 2, "mask one row off")
    with pytest.raises(AssertionError):
        assert_within((acc * ((1 - Xm) * Xm)).astype(np.float32), ref_d, mag * m, K + 2, "sigmoid mask for ReLU")
    with pytest.raises(AssertionError):
        assert_within(np.where(Xm > 0, _seq_fp32(A, Bm, skip=set(range(0, 32))), 0).astype(np.float32), ref_d, mag * m, K + 2,
                      "K tile dropped")
    nan = got_f.copy()
    nan[5, 7] = np.nan
    with pytest.raises(AssertionError, match="row 5, col 7"):
        assert_within(nan, ref_f, mag + np.abs(bias), K + 1, "NaN")


# ---- CPU: the declared routes hold ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", CASES, ids=lambda c: c.id)
def test_declared_route_at_256_cus(ops, case):
    with _debug6(case.debug):
        for v in case.variants():
            got = _query(ops, case, v, Addr, N_CU_MI355X)
            assert got == case.route, "%s %r: routed to %r, the table declares %r" % (case.id, v, got, case.route)


def test_case_table_reaches_every_family_and_variant():
    """Every kernel family, tile and loader variant the issue of these tests names appears in the table."""
    routes = set()
    for c in CASES:
        for r in (c.route if c.op == "bwd" else (c.route,)):
            if r is not None:
                routes.add(" ".join(w for w in r.split() if w != "fast" and not w.startswith("/")))
    want = {"smallk_rows", "smallk", "direct m0 al", "direct m1 al", "direct m2 al", "direct m0 v11", "direct m1 v11",
            "direct m2 v00", "direct m0 v01", "direct m1 v10", "staged m0", "staged m1", "staged m2", "gemm2 64x64",
            "gemm2 128x64", "gemm2 128x128", "gemm3 4x4", "gemm3 2x4", "gemm 1x1 v00", "gemm 1x1 v11", "gemm 1x1 v10",
            "gemm 1x1 v01", "gemm 1x2 v11", "gemm 2x2 v11"}
    assert want <= routes, sorted(want - routes)


# ---- CPU: the training step's routes are all in the table ---------------------------------------------------------------

STEP_CONFIGS = {   # layer shapes of bench.py's configurations (c5 = c3's shapes at a per-rank batch of 65536)
    "c2": dict(D=32, bot=[13, 512, 256, 32], top=[512, 256, 1]),
    "c3": dict(D=128, bot=[13, 512, 256, 128], top=[512, 512, 256, 1]),
}


def _record_step(config, Bsz, itself=False, interactions=None):
    """One TrainEngine step on the CPU test double (tests/fake_ops.py, world 1, 26 small tables) with linear_fwd / linear_bwd
    wrapped: their real arguments.  `interactions` (a list; tests/test_interact_routes.py): interact_fwd / interact_bwd are wrapped
    too and their arguments appended to it."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import fake_ops
    import cdlrm_amd.engine as engine
    import cdlrm_amd.model_no_ddp as Mo
    from oracle import cdlrm_oracle as O
    cfg = STEP_CONFIGS[config]
    calls = []

    def desc(t):
        return None if t is None else (tuple(t.shape), t.stride(0), (t.data_ptr() % 16) // 4)

    def lf(X, W, b, Y, act, stream=None, alone=False):
        calls.append(("fwd", desc(X), desc(W), desc(b), desc(Y), act, alone))
        return fake_ops.linear_fwd(X, W, b, Y, act, stream, alone)

    def lb(X, W, Y, dY, dX, dW, db, act, work, stream=None, x_act=0, alone=False):
        calls.append(("bwd", desc(X), desc(W), desc(Y), desc(dY), desc(dX), desc(dW), desc(db), act, x_act, alone))
        return fake_ops.linear_bwd(X, W, Y, dY, dX, dW, db, act, work, stream, x_act, alone)

    class Ops:
        pass

    shim = Ops()
    shim.__dict__.update({k: getattr(fake_ops, k) for k in dir(fake_ops) if not k.startswith("__")})
    shim.linear_fwd, shim.linear_bwd = lf, lb
    if interactions is not None:
        def al(t):
            return t.data_ptr() % 16 == 0

        def xf(feat, its, R, stream=None):
            interactions.append(("fwd", feat.shape[1], feat.shape[2], int(bool(its)), None, R.stride(0), al(R), True))
            return fake_ops.interact_fwd(feat, its, R, stream)

        def xb(feat, dR, its, dfeat, stream=None, x_act=0):
            interactions.append(("bwd", feat.shape[1], feat.shape[2], int(bool(its)), x_act, dR.stride(0), al(dR), al(dfeat)))
            return fake_ops.interact_bwd(feat, dR, its, dfeat, stream, x_act)

        shim.interact_fwd, shim.interact_bwd = xf, xb
    saved = (engine.ops, Mo.ops, Mo.Embedding_Table_Group.__dict__.get("device_pointers"))
    engine.ops, Mo.ops = shim, shim
    Mo.Embedding_Table_Group.device_pointers = lambda self: self._fake_ptrs
    try:
        T, rows, D = 26, 40, cfg["D"]
        ln_emb = np.array([rows] * T)
        nf = T + 1
        ln_top = np.array([D + (nf * (nf + 1) // 2 if itself else nf * (nf - 1) // 2)] + cfg["top"])
        host = O.init_host_tables([int(x) for x in ln_emb], D)
        eg = Mo.Embedding_Table_Group(D, ln_emb, init="empty_meta")
        for k in range(T):
            eg.emb_l[k].weight.data = host[k]
        eg._fake_ptrs = fake_ops.register_host(host)
        eg._pinned = True
        np.random.seed(1)
        torch.manual_seed(1)
        cg = Mo.Embedding_Table_Cache_Group(D, ln_emb, 64, Bsz, 4)
        dl = Mo.DLRM_Net(np.array(cfg["bot"]), ln_top, "dot", bool(itself), True, -1, ln_top.size - 2, 0.0)
        eng = engine.TrainEngine(cg, dl, eg, lr=0.1, lr_embeds=0.1)
        pipe = engine.WindowPipeline(cg, eg, Bsz, parity_rng=True)
        rng = np.random.RandomState(0)
        X = torch.from_numpy(rng.rand(Bsz, cfg["bot"][0]).astype(np.float32))
        idx = torch.from_numpy(rng.randint(0, rows, size=(T, Bsz)).astype(np.int64))
        Tt = torch.from_numpy(np.round(rng.rand(Bsz, 1)).astype(np.float32))
        pipe.plan_window(idx)
        pipe.commit()
        pipe.wait_writeback()
        eng.step(X, idx, Tt, j=0)
        eng.finish()
    finally:
        engine.ops, Mo.ops = saved[0], saved[1]
        if saved[2] is None:
            del Mo.Embedding_Table_Group.device_pointers
        else:
            Mo.Embedding_Table_Group.device_pointers = saved[2]
    return calls


def _step_key(ops, call):
    """(key as Case.keys builds it, route) of one recorded call, the route at 256 CUs on the recorded alignment facts."""
    def mk(d):
        return None if d is None else Addr(d[0][0], d[0][1] if len(d[0]) > 1 else d[0][0], d[1], d[2])
    if call[0] == "fwd":
        _, X, W, b, Y, act, alone = call
        b_op = None if b is None else Addr(1, b[0][0], b[0][0], b[2])
        r = route_str(ops.linear_fwd_route(mk(X), mk(W), b_op, mk(Y), act, alone=alone, n_cu=N_CU_MI355X))
        return ("fwd", r, act, b is not None, X[1] != X[0][1], Y[1] != Y[0][1])
    _, X, W, Y, dY, dX, dW, db, act, x_act, alone = call
    db_op = None if db is None else Addr(1, db[0][0], db[0][0], db[2])
    r = tuple(route_str(x) for x in ops.linear_bwd_route(mk(X), mk(W), mk(Y), mk(dY), mk(dX), mk(dW), db_op, act, x_act=x_act,
                                                          alone=alone, n_cu=N_CU_MI355X))
    return ("bwd", r, act, x_act if dX is not None else None, dW is not None, X[1] != X[0][1], dY[1] != dY[0][1],
            (dX[1] != dX[0][1]) if dX is not None else None)


@pytest.mark.parametrize("config,batch", [(c, b) for c in STEP_CONFIGS for b in (1024, 2048, 4096, 8192, 65536)])
def test_training_step_routes_are_in_the_table(ops, config, batch):
    """Every GEMM route one training step takes (c2 and c3 / c5 layer shapes at per-rank batches 1024 ... 65536), with its
    epilogue arguments and strided operands, is a case of the table the GPU test runs."""
    table = set()
    for c in CASES:
        table.update(c.keys())
    calls = _record_step(config, batch)
    assert sum(c[0] == "fwd" for c in calls) >= 5 and sum(c[0] == "bwd" for c in calls) >= 3, calls
    missing = []
    for call in calls:
        key = _step_key(ops, call)
        if key not in table:
            missing.append((key, call))
    assert not missing, "step routes the table lacks:\n" + "\n".join("%r  <- %r" % m for m in missing)


# ---- GPU: every case against float64 -------------------------------------------------------------------------------------

def _dev_operand(rows, cols, ld, off, fill, gap):
    """[rows, cols] view with row pitch ld at element offset `off` of a fresh allocation; the pitch gap holds `gap`."""
    buf = torch.full((off + rows * ld + 4,), gap, dtype=torch.float32, device=DEV)
    v = buf[off:off + rows * ld].view(rows, ld)[:, :cols]
    if fill is not None:
        v.copy_(fill)
    return v, buf


def _gap_ok(v, ld, cols, gap):
    if ld == cols:
        return True
    g = v.as_strided((v.shape[0], ld - cols), (ld, 1), v.storage_offset() + cols).cpu()
    return bool(torch.isnan(g).all()) if np.isnan(gap) else bool((g == gap).all())


def _run_fwd(ops, c, n_cu, rng):
    nan = float("nan")
    X = rng.randn(c.M, c.K).astype(np.float32)
    W = (rng.randn(c.N, c.K) / np.sqrt(c.K)).astype(np.float32)
    bias = rng.randn(c.N).astype(np.float32)
    Xd, _ = _dev_operand(c.M, c.K, c.ldx, c.offx, torch.from_numpy(X), nan)
    Wd, _ = _dev_operand(c.N, c.K, c.K, c.offw, torch.from_numpy(W), nan)
    bd, _ = _dev_operand(1, c.N, c.N, c.offb, torch.from_numpy(bias)[None], nan)
    bd = bd[0]
    X64, W64 = X.astype(np.float64), W.astype(np.float64)
    pre, mag = X64 @ W64.T, np.abs(X64) @ np.abs(W64).T
    for v in c.variants():
        Yd, _ = _dev_operand(c.M, c.N, c.ldy, c.offy, None, SENTINEL)
        b = bd if v["bias"] else None
        got_route = route_str(ops.linear_fwd_route(Xd, Wd, b, Yd, v["act"], alone=c.alone, n_cu=n_cu))
        assert got_route == c.route, "%s %r: the library takes %r, the case is meant for %r" % (c.id, v, got_route, c.route)
        ops.linear_fwd(Xd, Wd, b, Yd, v["act"], alone=c.alone)
        Y1 = Yd.clone()
        ops.linear_fwd(Xd, Wd, b, Yd, v["act"], alone=c.alone)          # a second call on the same route: the same bits
        torch.cuda.synchronize()
        assert torch.equal(Y1, Yd), "%s %r: two calls differ" % (c.id, v)
        assert _gap_ok(Yd, c.ldy, c.N, SENTINEL), "%s %r: Y's pitch gap was written" % (c.id, v)
        ref = act_fwd(pre + bias if v["bias"] else pre, v["act"])
        m = mag + np.abs(bias) if v["bias"] else mag
        assert_within(Yd.cpu().numpy(), ref, m, c.K + 1, "%s %r Y" % (c.id, v), c.route)


def _run_bwd(ops, c, n_cu, rng):
    nan = float("nan")
    W = (rng.randn(c.N, c.K) / np.sqrt(c.K)).astype(np.float32)
    dY = rng.randn(c.M, c.N).astype(np.float32)
    Yv = {0: None, 1: np.maximum(rng.randn(c.M, c.N), 0), 2: 1 / (1 + np.exp(-rng.randn(c.M, c.N)))}[c.act]
    Yv = None if Yv is None else Yv.astype(np.float32)
    Wd, _ = _dev_operand(c.N, c.K, c.K, c.offw, torch.from_numpy(W), nan)
    Yd = None if Yv is None else _dev_operand(c.M, c.N, c.ldy, c.offy, torch.from_numpy(Yv), nan)[0]
    W64 = W.astype(np.float64)
    dZ = dY.astype(np.float64) * (act_grad(Yv.astype(np.float64), c.act) if c.act else 1.0)
    dZmag = np.abs(dZ)
    prod, pmag = (dZ @ W64, dZmag @ np.abs(W64)) if c.dX else (None, None)
    work = ops.linear_bwd_work(c.M, c.N, c.K, DEV)
    for v in c.variants():
        xa = v["x_act"]
        Xv = {0: rng.randn(c.M, c.K), 1: np.maximum(rng.randn(c.M, c.K), 0), 2: 1 / (1 + np.exp(-rng.randn(c.M, c.K)))}[xa]
        Xv = Xv.astype(np.float32)
        Xd, _ = _dev_operand(c.M, c.K, c.ldx, c.offx, torch.from_numpy(Xv), nan)
        dYd, _ = _dev_operand(c.M, c.N, c.ldy, c.offy, torch.from_numpy(dY), nan)
        dXd = _dev_operand(c.M, c.K, c.lddx, c.offdx, None, SENTINEL)[0] if c.dX else None
        dWd = torch.full((c.N, c.K), SENTINEL, device=DEV) if c.dW else None
        dbd = torch.full((c.N,), SENTINEL, device=DEV) if c.dW else None
        with _debug6(c.debug):
            got = ops.linear_bwd_route(Xd, Wd, Yd, dYd, dXd, dWd, dbd, c.act, x_act=xa, alone=c.alone, n_cu=n_cu)
            got_route = tuple(route_str(x) for x in got)
            assert got_route == c.route, "%s %r: the library takes %r, the case is meant for %r" % (c.id, v, got_route, c.route)
            ops.linear_bwd(Xd, Wd, Yd, dYd, dXd, dWd, dbd, c.act, work, x_act=xa, alone=c.alone)
            torch.cuda.synchronize()
            outs1 = [t.clone() for t in (dXd, dWd, dbd) if t is not None]
            dY2, _ = _dev_operand(c.M, c.N, c.ldy, c.offy, torch.from_numpy(dY), nan)
            ops.linear_bwd(Xd, Wd, Yd, dY2, dXd, dWd, dbd, c.act, work, x_act=xa, alone=c.alone)
            torch.cuda.synchronize()
        outs2 = [t for t in (dXd, dWd, dbd) if t is not None]
        assert all(torch.equal(a, b) for a, b in zip(outs1, outs2)), "%s %r: two calls differ" % (c.id, v)
        assert torch.equal(dYd, dY2), "%s %r: dZ differs between two calls" % (c.id, v)
        assert _gap_ok(dYd, c.ldy, c.N, nan), "%s %r: dY's pitch gap was written" % (c.id, v)
        if c.act:
            assert_within(dYd.cpu().numpy(), dZ, dZmag, 3, "%s %r dZ (in place)" % (c.id, v), c.route[0] or c.route[1])
        if c.dX:
            assert _gap_ok(dXd, c.lddx, c.K, SENTINEL), "%s %r: dX's pitch gap was written" % (c.id, v)
            m = act_grad(Xv.astype(np.float64), xa)
            assert_within(dXd.cpu().numpy(), prod * m, pmag * np.abs(m), c.N + 5, "%s %r dX" % (c.id, v), c.route[0])
        if c.dW:
            splits = got[1]["splits"]
            k_eff = (c.M if splits == 1 else -(-c.M // splits) + 32 + splits) + 3
            X64 = Xv.astype(np.float64)
            assert_within(dWd.cpu().numpy(), dZ.T @ X64, dZmag.T @ np.abs(X64), k_eff, "%s %r dW" % (c.id, v), c.route[1])
            assert_within(dbd.cpu().numpy(), dZ.sum(0), dZmag.sum(0), k_eff, "%s %r db" % (c.id, v), c.route[1])


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=lambda c: c.id)
def test_route_vs_float64(ops, case):
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    rng = np.random.RandomState(sum(map(ord, case.id)))
    if case.op == "fwd":
        with _debug6(case.debug):
            _run_fwd(ops, case, n_cu, rng)
    else:
        _run_bwd(ops, case, n_cu, rng)


@pytest.mark.gpu
def test_gemm2_128x128_equals_128x64(ops):
    """gemm_glds.h: a k_gemm2 tile's k order does not depend on its shape -- the 128x128 tile (M = 65536 x 512) and the 128x64 tile
    of cdlrm_debug_set(6, 16) give the same bits."""
    M, N, K = 65536, 512, 480
    rng = np.random.RandomState(11)
    X = torch.from_numpy(rng.randn(M, K).astype(np.float32)).to(DEV)
    W = torch.from_numpy((rng.randn(N, K) / np.sqrt(K)).astype(np.float32)).to(DEV)
    b = torch.from_numpy(rng.randn(N).astype(np.float32)).to(DEV)
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    for act in (1, 2):
        Y0, Y1 = torch.empty(M, N, device=DEV), torch.empty(M, N, device=DEV)
        assert route_str(ops.linear_fwd_route(X, W, b, Y0, act, n_cu=n_cu)) == "gemm2 128x128 fast"
        ops.linear_fwd(X, W, b, Y0, act)
        with _debug6(16):
            assert route_str(ops.linear_fwd_route(X, W, b, Y1, act, n_cu=n_cu)) == "gemm2 128x64 fast"
            ops.linear_fwd(X, W, b, Y1, act)
            torch.cuda.synchronize()
        assert torch.equal(Y0, Y1)
