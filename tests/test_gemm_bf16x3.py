"""The opt-in bf16x3 split-operand mode of the MLP GEMMs (CDLRM_GEMM_BF16X3, csrc/gemm_bf16.h with two planes) against float64.

Numerics contract: the layers of the bf16 mode (K >= 32 and N >= 32) run forward, dgrad and weight
gradient with every operand element x split into h = bf16(x) and l = bf16(x - h) (round-to-nearest-even, l = 0 where h is not
finite); a product a * b is al*bh + ah*bl + ah*bh, three exact products accumulated in fp32 in a fixed order.  Epilogues and
storage are fp32; the bias gradient is the column sum of the UNSPLIT dZ.

The reference here is float64 of the UNSPLIT operands, and the bound is

    |got - ref| <= (3.25 * 2^-16 + C_BOUND * 3 K_eff * 2^-24) * (|A| @ |B|) + 8 * 2^-24 |ref|

With u = 2^-8: |x - h| <= u |x| and |x - h - l| <= u^2 |x|, so (ah + al)(bh + bl) is within (2 u^2 + u^4) |a b| of a b, and the
dropped al*bl is at most u^2 |a b|: 3 u^2 = 3 * 2^-16 of each product's magnitude, 3.25 with the higher-order terms; the second
term is the fp32-chain bound of test_gemm_routes.py over the 3 K_eff accumulated terms; the third the activation's rounding.  K_eff is
what test_gemm_bf16.py uses (K + 1 with the bias, the slab formula for weight gradients).  The plain bf16 mode misses this bound
by two orders of magnitude, and so does a kernel that drops either cross product: the CPU controls below show that.

One table of cases, each with its declared route, serves three checks as in test_gemm_bf16.py:
  * CPU: the route queries give the declared route at 256 CUs; ineligible shapes report their fp32 route;
  * CPU: one TrainEngine step with matmul_precision="bf16x3" on the CPU test double: every flagged launch is in the table;
  * GPU: each case against float64, NaN in input pitch gaps, sentinels in output gaps, two launches bit-identical.

Tile rule of the mode: 64x128 where its grid has >= 1024 workgroups, else 64x64 (never 128x128: static LDS).  The cases use the
smallest M at which the declared route is taken: 64x64 at any M, 64x128 from cdiv(M, 64) * cdiv(N, 128) = 1024 on.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import test_gemm_routes as R      # noqa: E402  (the fp32 comparator, operand helpers, Case)
import test_gemm_bf16 as B16      # noqa: E402  (route strings of the bf16 family, the plan builder, the engine step)

DEV = "cuda:0"
N_CU = 256
U = R.U
SENTINEL = R.SENTINEL
PITCH_FEAT = R.PITCH_FEAT
PREC = "bf16x3"
C3_TOP, C3_BOT = B16.C3_TOP, B16.C3_BOT

ops = R.ops      # the module fixture: builds the library if needed


def route_str(r):
    """'bf16x3 64x128 v11 /16' for the bf16x3 family, test_gemm_bf16.route_str for the others."""
    if r is None or r["family"] != "bf16x3":
        return B16.route_str(r)
    s = "bf16x3 %dx%d v%d%d" % (64 * r["tm"], 64 * r["tn"], r["vec_a"], r["vec_b"])
    if r["splits"] > 1:
        s += " /%d" % r["splits"]
    return s


def x3_bound(ref, mag, k_eff):
    return (3.25 * 2.0 ** -16 + R.C_BOUND * 3 * k_eff * U) * np.asarray(mag, dtype=np.float64) + 8 * U * np.abs(ref) + R.TINY


def assert_within_x3(got, ref, mag, k_eff, what):
    """The bound of the module docstring, element by element (NaN fails).  Returns (worst |err|, worst |err| / bound)."""
    got = np.asarray(got, dtype=np.float64)
    ref = np.asarray(ref, dtype=np.float64)
    bound = x3_bound(ref, mag, k_eff)
    err = np.abs(got - ref)
    ok = err <= bound
    ratio = np.where(np.isnan(err), np.inf, err / bound)
    if not ok.all():
        i = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
        raise AssertionError("%s: %d of %d elements outside the bf16x3 bound; worst at %r: got %r, want %r, |err| %.3g > bound "
                             "%.3g (K_eff %d)" % (what, int((~ok).sum()), ok.size, tuple(int(x) for x in i), float(got[i]),
                                                  float(ref[i]), float(err[i]), float(bound[i]), k_eff))
    return float(err.max()), float(ratio.max())


F = lambda cid, M, N, K, route, **kw: R.Case(cid, "fwd", M, N, K, route, **kw)     # noqa: E731
B = lambda cid, M, N, K, route, **kw: R.Case(cid, "bwd", M, N, K, route, **kw)     # noqa: E731
X64 = "bf16x3 64x64 v11"
M128 = 255 * 64 + 1        # smallest M at which N = 512 (four 128-wide panels) gives 64x128 its 1024 workgroups

CASES = [
    # ---- forward: Y = act(X W^T + b), split operands ----
    F("fwd_min_32x32", 200, 32, 32, X64),
    F("fwd_top0_k480", 200, 512, 480, X64),
    F("fwd_k479_v00", 1000, 512, 479, "bf16x3 64x64 v00"),
    F("fwd_pitch_v01", 200, 256, 480, "bf16x3 64x64 v01", ldx=481),
    F("fwd_unaligned_w_v10", 200, 256, 480, "bf16x3 64x64 v10", offw=2),
    F("fwd_n479", 200, 479, 512, X64, ldy=480),
    F("fwd_256x512", 200, 256, 512, X64, acts=(1,), biases=(True,)),
    F("fwd_bot_feat", 200, 128, 256, X64, acts=(1,), biases=(True,), ldy=PITCH_FEAT),
    F("fwd_64x128", M128, 512, 96, "bf16x3 64x128 v11", acts=(1,)),
    # ---- dgrad: dX = (dZ W) * act'(X) ----
    B("dgrad_512", 200, 512, 512, (X64, None)),
    B("dgrad_ragged_m1000", 1000, 256, 480, (X64, None)),
    B("dgrad_n479_v01", 200, 479, 512, ("bf16x3 64x64 v01", None), ldy=480),
    B("dgrad_padded_dx", 200, 512, 480, (X64, None), lddx=484, x_acts=(0,)),
    B("dgrad_256_feat", 200, 128, 256, (X64, None), ldy=PITCH_FEAT, x_acts=(1,)),
    B("dgrad_mask_pitch", 200, 256, 512, (X64, None), ldx=514, x_acts=(1,)),
    B("dgrad_64x128", M128, 96, 512, ("bf16x3 64x128 v11", None), x_acts=(1,)),
    # ---- weight gradient: dW = dZ^T X in split-M slabs, db = column sums of dZ (fp32) ----
    B("wgrad_one_slab", 256, 512, 512, (None, X64), dX=False, dW=True),
    B("wgrad_short_v10", 1000, 256, 70, (None, "bf16x3 64x64 v10"), dX=False, dW=True),
    B("wgrad_ragged_m8200", 8200, 264, 480, (None, "bf16x3 64x64 v11 /26"), dX=False, dW=True),
    B("wgrad_act_relu", 2100, 256, 480, (X64, "bf16x3 64x64 v11 /9"), act=1, dW=True, x_acts=(1,)),
    B("wgrad_act_sigmoid", 600, 128, 256, (X64, X64), act=2, dW=True, x_acts=(2,)),
]

# with the flag set, these stay on their fp32 route (the route the same call takes without it)
FALLBACK = [
    F("fb_k13", 1000, 256, 13, None),
    F("fb_k31", 2048, 256, 31, None),
    F("fb_n1_head", 8192, 1, 256, None),
    F("fb_n31", 2048, 31, 512, None),
    B("fb_wgrad_n16", 8192, 16, 512, None, dW=True, x_acts=(0,)),
]


def _query(ops, case, v, mk, n_cu, **mode):
    c = case
    X = mk(c.M, c.K, c.ldx, c.offx)
    W = mk(c.N, c.K, c.K, c.offw)
    if c.op == "fwd":
        b = mk(1, c.N, c.N, c.offb) if v["bias"] else None
        return route_str(ops.linear_fwd_route(X, W, b, mk(c.M, c.N, c.ldy, c.offy), v["act"], alone=c.alone, n_cu=n_cu, **mode))
    Y = mk(c.M, c.N, c.ldy, c.offy)
    dY = mk(c.M, c.N, c.ldy, c.offy)
    dX = mk(c.M, c.K, c.lddx, c.offdx) if c.dX else None
    dW = mk(c.N, c.K, c.K, 0) if c.dW else None
    db = mk(1, c.N, c.N, 0) if c.dW else None
    r = ops.linear_bwd_route(X, W, Y if c.act else None, dY, dX, dW, db, c.act, x_act=v["x_act"], alone=c.alone, n_cu=n_cu,
                             **mode)
    return tuple(route_str(x) for x in r)


# ---- CPU: routes, sizes, flags ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", CASES, ids=lambda c: c.id)
def test_declared_bf16x3_route_at_256_cus(ops, case):
    for v in case.variants():
        got = _query(ops, case, v, R.Addr, N_CU, precision=PREC)
        assert got == case.route, "%s %r: routed to %r, the table declares %r" % (case.id, v, got, case.route)
        # without the flag there is no bf16x3 family, and the bf16 flag (either spelling) gives the bf16 family as before
        assert "bf16" not in str(_query(ops, case, v, R.Addr, N_CU)), case.id
        b16 = _query(ops, case, v, R.Addr, N_CU, bf16=True)
        assert "bf16x3" not in str(b16) and "bf16 " in str(b16), (case.id, b16)
        assert b16 == _query(ops, case, v, R.Addr, N_CU, precision="bf16")


def test_smallest_m_of_the_64x128_tile(ops):
    """One row less than the 64x128 cases' M and the rule picks 64x64: the cases sit on the threshold."""
    for c in CASES:
        if "64x128" not in str(c.route):
            continue
        below = R.Case(c.id, c.op, c.M - 1, c.N, c.K, c.route, acts=c.acts, biases=c.biases, x_acts=c.x_acts)
        got = _query(ops, below, below.variants()[0], R.Addr, N_CU, precision=PREC)
        assert "bf16x3 64x64" in str(got), (c.id, got)


@pytest.mark.parametrize("case", FALLBACK, ids=lambda c: c.id)
def test_ineligible_shapes_keep_their_fp32_route(ops, case):
    for v in case.variants():
        flagged = _query(ops, case, v, R.Addr, N_CU, precision=PREC)
        assert flagged == _query(ops, case, v, R.Addr, N_CU), (case.id, v, flagged)
        assert "bf16" not in str(flagged)


def _work_bytes(ops, M, layers, flags):
    from cdlrm_amd import _lib
    NA = C.c_int32 * len(layers)
    N, K = NA(*[n for n, _ in layers]), NA(*[k for _, k in layers])
    return int(_lib.lib().cdlrm_mlp_wgrad_work_bytes_ex(len(layers), M, N, K, flags))


def test_work_sizes(ops):
    """The work bytes of a bf16x3 plan are those of the bf16 plan; flags 0 gives the fp32 size."""
    from cdlrm_amd import _lib
    assert ops.PRECISIONS[PREC] == 0x400 and ops.GEMM_BF16X3 == 0x400
    for M in (1, 256, 1000, 2048, 8192, 65536):
        for layers in (C3_TOP, C3_BOT):
            x3, b16 = _work_bytes(ops, M, layers, ops.GEMM_BF16X3), _work_bytes(ops, M, layers, ops.GEMM_BF16)
            assert x3 == b16 > 0, (M, layers, x3, b16)
            NA = C.c_int32 * len(layers)
            N, K = NA(*[n for n, _ in layers]), NA(*[k for _, k in layers])
            assert _work_bytes(ops, M, layers, 0) == _lib.lib().cdlrm_mlp_wgrad_work_bytes(len(layers), M, N, K)
            assert ops.mlp_wgrad_work(M, [n for n, _ in layers], [k for _, k in layers], "cpu", precision=PREC).numel() >= x3


def test_both_flags_are_rejected(ops):
    from cdlrm_amd import _lib
    c = CASES[1]
    X, W, Y = R.Addr(c.M, c.K, c.K, 0), R.Addr(c.N, c.K, c.K, 0), R.Addr(c.M, c.N, c.N, 0)
    with pytest.raises(AssertionError):
        ops.linear_fwd_route(X, W, None, Y, 0, bf16=True, precision=PREC)
    with pytest.raises(AssertionError):
        ops.linear_bwd_route(X, W, None, Y, X, None, None, 0, bf16=True, precision=PREC)
    with pytest.raises(AssertionError):         # (the bf16= keyword beside ANY precision=, its own spelling included)
        ops.linear_fwd_route(X, W, None, Y, 0, bf16=True, precision="bf16")
    both = ops.GEMM_BF16 | ops.GEMM_BF16X3
    out = (_lib.GemmRoute * 8)()        # (room for a route per layer of the plan below)
    raw = _lib.raw()
    assert raw.cdlrm_linear_fwd_route(X.data_ptr(), c.K, W.data_ptr(), None, Y.data_ptr(), c.N, c.M, c.N, c.K, both, None, N_CU,
                                      C.byref(out[0])) != 0
    assert "exclude" in raw.cdlrm_last_error().decode()
    assert raw.cdlrm_linear_bwd_route(X.data_ptr(), c.K, W.data_ptr(), None, 0, Y.data_ptr(), c.N, X.data_ptr(), c.K, None, None,
                                      c.M, c.N, c.K, both, 0, 256, None, N_CU, out) != 0
    plan = B16._plan(ops, 1024, C3_TOP, precision=PREC)
    assert raw.cdlrm_mlp_wgrad_route(plan.n, plan.X, plan.ld_x, plan.dZ, plan.ld_dz, plan.dW, plan.db, plan.M, plan.N, plan.K,
                                     both, N_CU, out) != 0
    # each flag alone is accepted by the same calls
    for one in (ops.GEMM_BF16, ops.GEMM_BF16X3):
        assert raw.cdlrm_linear_fwd_route(X.data_ptr(), c.K, W.data_ptr(), None, Y.data_ptr(), c.N, c.M, c.N, c.K, one, None,
                                          N_CU, C.byref(out[0])) == 0


@pytest.mark.parametrize("M", [256, 1024, 8192, 65536])
def test_mlp_wgrad_route(ops, M):
    """cdlrm_mlp_wgrad_route: the eligible layers of a bf16x3 plan report the bf16x3 family with the slab count the bf16 plan
    gives them, the 13-wide and 1-wide layers the route of the fp32 plan."""
    for layers in (C3_TOP, C3_BOT):
        plan = B16._plan(ops, M, layers, precision=PREC)
        got = ops.mlp_wgrad_route(plan, n_cu=N_CU)
        b16 = ops.mlp_wgrad_route(plan, n_cu=N_CU, precision="bf16")
        fp = ops.mlp_wgrad_route(plan, n_cu=N_CU, precision="fp32")
        assert all(r["family"] not in ("bf16", "bf16x3") for r in fp), fp
        for r, rb, r32, (n, k) in zip(got, b16, fp, layers):
            if n >= 32 and k >= 32:
                assert route_str(r).startswith("bf16x3 64x64 v11"), (M, n, k, r)
                assert rb["family"] == "bf16" and dict(rb, family="bf16x3") == r, (r, rb)
            else:
                assert r == r32 == rb, (M, n, k, r, r32)


# ---- CPU: the comparator's controls -------------------------------------------------------------------------------------------

def _bf(a):
    """float32 of the bf16-rounded values (round-to-nearest-even)."""
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32)).to(torch.bfloat16).float().numpy()


def _split(a):
    a = np.asarray(a, dtype=np.float32)
    h = _bf(a)
    return h, _bf(a - h)


def _seq3(A, Bm, terms=("lh", "hl", "hh"), skip=()):
    """The mode's arithmetic emulated in fp32: per contraction index the products named in `terms` (a-plane, b-plane), each exact,
    added to one fp32 accumulator in that order."""
    (ah, al), (bh, bl) = _split(A), _split(Bm)
    pa, pb = {"h": ah, "l": al}, {"h": bh, "l": bl}
    acc = np.zeros((A.shape[0], Bm.shape[1]), dtype=np.float32)
    for k in range(A.shape[1]):
        if k in skip:
            continue
        for t in terms:
            acc = (acc + pa[t[0]][:, k:k + 1] * pb[t[1]][k:k + 1, :]).astype(np.float32)
    return acc


@pytest.mark.parametrize("M,N,K", [(64, 48, 480), (32, 32, 96), (64, 32, 32)])
def test_comparator_controls(M, N, K):
    """Against float64 of the UNSPLIT operands: the three-product emulation passes the bound (with room: <= 0.25 of it); plain
    bf16, either cross product dropped, and a dropped 64-deep K tile each fail it."""
    rng = np.random.RandomState(1000 + K)
    A = rng.randn(M, K).astype(np.float32)
    Bm = (rng.randn(K, N) / np.sqrt(K)).astype(np.float32)
    ref = A.astype(np.float64) @ Bm.astype(np.float64)
    mag = np.abs(A).astype(np.float64) @ np.abs(Bm).astype(np.float64)
    _, worst = assert_within_x3(_seq3(A, Bm), ref, mag, K, "three-product emulation")
    print("K = %d: emulation worst |err| / bound %.3f" % (K, worst))
    assert worst <= 0.25
    controls = {
        "plain bf16 (hi*hi only)": dict(terms=("hh",)),
        "al*bh dropped": dict(terms=("hl", "hh")),
        "ah*bl dropped": dict(terms=("lh", "hh")),
        "64-deep K tile dropped": dict(skip=set(range(max(K - 64, 0), K))),
    }
    for what, kw in controls.items():
        with pytest.raises(AssertionError):
            assert_within_x3(_seq3(A, Bm, **kw), ref, mag, K, what)


# ---- CPU: the engine's bf16x3 step --------------------------------------------------------------------------------------------

def _record_step(config, Bsz):
    """One TrainEngine(matmul_precision="bf16x3") step on the CPU test double, through a shim around tests/fake_ops.py that
    accepts the mode keywords and records them: (bf16, precision) of every linear_fwd / linear_bwd call, the plans, and the
    precision of every mlp_wgrad call."""
    import fake_ops
    import cdlrm_amd.engine as engine
    calls, plans, used = [], [], []

    def desc(t):
        return None if t is None else (tuple(t.shape), t.stride(0), (t.data_ptr() % 16) // 4)

    def lf(X, W, b, Y, act, stream=None, alone=False, bf16=False, precision=None):
        calls.append(((bf16, precision), ("fwd", desc(X), desc(W), desc(b), desc(Y), act, alone)))
        return fake_ops.linear_fwd(X, W, b, Y, act, stream, alone)

    def lb(X, W, Y, dY, dX, dW, db, act, work, stream=None, x_act=0, alone=False, bf16=False, precision=None):
        calls.append(((bf16, precision),
                      ("bwd", desc(X), desc(W), desc(Y), desc(dY), desc(dX), desc(dW), desc(db), act, x_act, alone)))
        return fake_ops.linear_bwd(X, W, Y, dY, dX, dW, db, act, work, stream, x_act, alone)

    def work(M, Ns, Ks, device, precision="fp32"):
        return fake_ops.mlp_wgrad_work(M, Ns, Ks, device)

    class Plan(fake_ops.WgradPlan):
        def __init__(self, Xs, dZs, dWs, dbs, work, precision="fp32"):
            super().__init__(Xs, dZs, dWs, dbs, work)
            self.precision = precision
            plans.append(self)

    def wg(plan, stream=None, lr=None):
        used.append(plan.precision)
        return fake_ops.mlp_wgrad(plan, stream, lr)

    class Shim:
        pass

    shim = Shim()
    shim.__dict__.update({k: getattr(fake_ops, k) for k in dir(fake_ops) if not k.startswith("__")})
    shim.linear_fwd, shim.linear_bwd, shim.mlp_wgrad_work, shim.WgradPlan, shim.mlp_wgrad = lf, lb, work, Plan, wg
    shim.bf16_eligible = lambda N, K: int(N) >= 32 and int(K) >= 32

    class Engine(engine.TrainEngine):       # (test_gemm_bf16's step builds its engine in bf16 mode: same step, this mode)
        def __init__(self, *a, **kw):
            kw["matmul_precision"] = PREC
            super().__init__(*a, **kw)

    saved = engine.TrainEngine
    engine.TrainEngine = Engine
    try:
        B16._run_engine_step(config, Bsz, shim)
    finally:
        engine.TrainEngine = saved
    return calls, plans, used


def _x3_key(ops, call):
    def mk(d):
        return None if d is None else R.Addr(d[0][0], d[0][1] if len(d[0]) > 1 else d[0][0], d[1], d[2])
    if call[0] == "fwd":
        _, X, W, b, Y, act, alone = call
        b_op = None if b is None else R.Addr(1, b[0][0], b[0][0], b[2])
        r = route_str(ops.linear_fwd_route(mk(X), mk(W), b_op, mk(Y), act, alone=alone, n_cu=N_CU, precision=PREC))
        return ("fwd", r, act, b is not None, X[1] != X[0][1], Y[1] != Y[0][1])
    _, X, W, Y, dY, dX, dW, db, act, x_act, alone = call
    db_op = None if db is None else R.Addr(1, db[0][0], db[0][0], db[2])
    r = tuple(route_str(x) for x in ops.linear_bwd_route(mk(X), mk(W), mk(Y), mk(dY), mk(dX), mk(dW), db_op, act, x_act=x_act,
                                                         alone=alone, n_cu=N_CU, precision=PREC))
    return ("bwd", r, act, x_act if dX is not None else None, dW is not None, X[1] != X[0][1], dY[1] != dY[0][1],
            (dX[1] != dX[0][1]) if dX is not None else None)


@pytest.mark.parametrize("batch", [1024, 8192])
def test_bf16x3_training_step_routes_are_in_the_table(ops, batch):
    """Every GEMM launch of a bf16x3 engine step at the c3 widths: eligible layers carry precision="bf16x3" (and never the bf16
    keyword) and resolve to a route of the table, ineligible ones (13-wide input, 1-wide head) carry no mode; the weight
    gradients go through bf16x3 plans only."""
    table = set()
    for c in CASES:
        table.update(c.keys())
    calls, plans, used = _record_step("c3", batch)
    assert sum(c[1][0] == "fwd" for c in calls) >= 5 and sum(c[1][0] == "bwd" for c in calls) >= 3, calls
    missing, flagged = [], 0
    for (bf16, precision), call in calls:
        W = call[2]
        eligible = W[0][0] >= 32 and W[0][1] >= 32
        assert not bf16, ("the bf16 keyword in a bf16x3 step", call)
        assert precision == (PREC if eligible else None), ("mode on an ineligible layer" if precision else
                                                            "eligible layer without the mode", call)
        if not eligible:
            continue
        flagged += 1
        key = _x3_key(ops, call)
        if key not in table:
            missing.append((key, call))
    assert flagged >= 4
    assert not missing, "bf16x3 step routes the table lacks:\n" + "\n".join("%r  <- %r" % m for m in missing)
    assert used and set(used) == {PREC}, used
    assert any(p.precision == PREC for p in plans)


def test_engine_rejects_an_unknown_precision():
    from cdlrm_amd.engine import TrainEngine

    class E:
        matmul_precision = "bf16x2"
    with pytest.raises(AssertionError, match="'fp32', 'bf16' or 'bf16x3'"):
        TrainEngine._mm(E(), None)


# ---- GPU: every case against float64 of the unsplit operands ------------------------------------------------------------------

def _mode(precision):
    return {"bf16": True} if precision == "bf16" else {"precision": precision}


def _check(precision, got, ref, mag, k_eff, what):
    """bf16x3: the bound.  bf16 (the relative check's other side): no bound here, the worst |err| only."""
    if precision == PREC:
        return assert_within_x3(got, ref, mag, k_eff, what)[0]
    return float(np.abs(np.asarray(got, dtype=np.float64) - ref).max())


def _run_fwd(ops, c, n_cu, rng, precision=PREC):
    """Every variant of a forward case; returns the worst |error| against float64 over all of them."""
    nan = float("nan")
    X = rng.randn(c.M, c.K).astype(np.float32)
    W = (rng.randn(c.N, c.K) / np.sqrt(c.K)).astype(np.float32)
    bias = rng.randn(c.N).astype(np.float32)
    Xd, _ = R._dev_operand(c.M, c.K, c.ldx, c.offx, torch.from_numpy(X), nan)
    Wd, _ = R._dev_operand(c.N, c.K, c.K, c.offw, torch.from_numpy(W), nan)
    bd, _ = R._dev_operand(1, c.N, c.N, c.offb, torch.from_numpy(bias)[None], nan)
    bd = bd[0]
    X64, W64 = X.astype(np.float64), W.astype(np.float64)
    pre, mag = X64 @ W64.T, np.abs(X64) @ np.abs(W64).T
    worst = 0.0
    for v in c.variants():
        Yd, _ = R._dev_operand(c.M, c.N, c.ldy, c.offy, None, SENTINEL)
        b = bd if v["bias"] else None
        if precision == PREC:
            got = route_str(ops.linear_fwd_route(Xd, Wd, b, Yd, v["act"], alone=c.alone, n_cu=n_cu, **_mode(precision)))
            assert got == c.route, "%s %r: the library takes %r, the case is meant for %r" % (c.id, v, got, c.route)
        ops.linear_fwd(Xd, Wd, b, Yd, v["act"], alone=c.alone, **_mode(precision))
        Y1 = Yd.clone()
        ops.linear_fwd(Xd, Wd, b, Yd, v["act"], alone=c.alone, **_mode(precision))
        torch.cuda.synchronize()
        assert torch.equal(Y1, Yd), "%s %r: two calls differ" % (c.id, v)
        assert R._gap_ok(Yd, c.ldy, c.N, SENTINEL), "%s %r: Y's pitch gap was written" % (c.id, v)
        ref = R.act_fwd(pre + bias if v["bias"] else pre, v["act"])
        m = mag + np.abs(bias) if v["bias"] else mag
        worst = max(worst, _check(precision, Yd.cpu().numpy(), ref, m, c.K + 1, "%s %r Y" % (c.id, v)))
    return worst


def _run_bwd(ops, c, n_cu, rng, precision=PREC):
    """Every variant of a backward case; returns (worst dX |error|, worst dW |error|) against float64."""
    nan = float("nan")
    W = (rng.randn(c.N, c.K) / np.sqrt(c.K)).astype(np.float32)
    dY = rng.randn(c.M, c.N).astype(np.float32)
    Yv = {0: None, 1: np.maximum(rng.randn(c.M, c.N), 0), 2: 1 / (1 + np.exp(-rng.randn(c.M, c.N)))}[c.act]
    Yv = None if Yv is None else Yv.astype(np.float32)
    Wd, _ = R._dev_operand(c.N, c.K, c.K, c.offw, torch.from_numpy(W), nan)
    Yd = None if Yv is None else R._dev_operand(c.M, c.N, c.ldy, c.offy, torch.from_numpy(Yv), nan)[0]
    # dZ as the kernel computes it in fp32 (dY * act'(Y): exact for ReLU; one fp32 rounding for the sigmoid's)
    dZ32 = dY * (((1.0 - Yv) * Yv).astype(np.float32) if c.act == 2 else (Yv > 0).astype(np.float32) if c.act == 1 else 1.0)
    dZ32 = dZ32.astype(np.float32)
    dz64, W64 = dZ32.astype(np.float64), W.astype(np.float64)
    prod, pmag = (dz64 @ W64, np.abs(dz64) @ np.abs(W64)) if c.dX else (None, None)
    work = ops.linear_bwd_work(c.M, c.N, c.K, DEV)
    worst_dx = worst_dw = 0.0
    for v in c.variants():
        xa = v["x_act"]
        Xv = {0: rng.randn(c.M, c.K), 1: np.maximum(rng.randn(c.M, c.K), 0), 2: 1 / (1 + np.exp(-rng.randn(c.M, c.K)))}[xa]
        Xv = Xv.astype(np.float32)
        Xd, _ = R._dev_operand(c.M, c.K, c.ldx, c.offx, torch.from_numpy(Xv), nan)
        dYd, _ = R._dev_operand(c.M, c.N, c.ldy, c.offy, torch.from_numpy(dY), nan)
        dXd = R._dev_operand(c.M, c.K, c.lddx, c.offdx, None, SENTINEL)[0] if c.dX else None
        dWd = torch.full((c.N, c.K), SENTINEL, device=DEV) if c.dW else None
        dbd = torch.full((c.N,), SENTINEL, device=DEV) if c.dW else None
        got = ops.linear_bwd_route(Xd, Wd, Yd, dYd, dXd, dWd, dbd, c.act, x_act=xa, alone=c.alone, n_cu=n_cu, **_mode(precision))
        if precision == PREC:
            got_route = tuple(route_str(x) for x in got)
            assert got_route == c.route, "%s %r: the library takes %r, the case is meant for %r" % (c.id, v, got_route, c.route)
        ops.linear_bwd(Xd, Wd, Yd, dYd, dXd, dWd, dbd, c.act, work, x_act=xa, alone=c.alone, **_mode(precision))
        torch.cuda.synchronize()
        outs1 = [t.clone() for t in (dXd, dWd, dbd) if t is not None]
        dY2, _ = R._dev_operand(c.M, c.N, c.ldy, c.offy, torch.from_numpy(dY), nan)
        ops.linear_bwd(Xd, Wd, Yd, dY2, dXd, dWd, dbd, c.act, work, x_act=xa, alone=c.alone, **_mode(precision))
        torch.cuda.synchronize()
        outs2 = [t for t in (dXd, dWd, dbd) if t is not None]
        assert all(torch.equal(a, b) for a, b in zip(outs1, outs2)), "%s %r: two calls differ" % (c.id, v)
        assert R._gap_ok(dYd, c.ldy, c.N, nan), "%s %r: dY's pitch gap was written" % (c.id, v)
        if c.act:
            R.assert_within(dYd.cpu().numpy(), dz64, np.abs(dZ32), 3, "%s %r dZ" % (c.id, v), "bf16")
        if c.dX:
            assert R._gap_ok(dXd, c.lddx, c.K, SENTINEL), "%s %r: dX's pitch gap was written" % (c.id, v)
            m = R.act_grad(Xv.astype(np.float64), xa)
            worst_dx = max(worst_dx, _check(precision, dXd.cpu().numpy(), prod * m, pmag * np.abs(m), c.N + 5,
                                            "%s %r dX" % (c.id, v)))
        if c.dW:
            splits = got[1]["splits"]
            k_eff = (c.M if splits == 1 else -(-c.M // splits) + 64 + splits) + 3
            x64 = Xv.astype(np.float64)
            worst_dw = max(worst_dw, _check(precision, dWd.cpu().numpy(), dz64.T @ x64, np.abs(dz64).T @ np.abs(x64), k_eff,
                                            "%s %r dW" % (c.id, v)))
            # the bias gradient: column sums of the UNSPLIT dZ, an fp32 epilogue under the fp32 bound
            R.assert_within(dbd.cpu().numpy(), dz64.sum(0), np.abs(dz64).sum(0), k_eff, "%s %r db" % (c.id, v), "bf16")
    return worst_dx, worst_dw


def _case(cid):
    return next(c for c in CASES if c.id == cid)


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=lambda c: c.id)
def test_bf16x3_route_vs_float64(ops, case):
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    rng = np.random.RandomState(sum(map(ord, case.id)))
    if case.op == "fwd":
        _run_fwd(ops, case, n_cu, rng)
    else:
        _run_bwd(ops, case, n_cu, rng)


@pytest.mark.gpu
@pytest.mark.parametrize("cid", ["fwd_top0_k480", "dgrad_512", "wgrad_one_slab"])
def test_bf16x3_error_is_a_64th_of_the_bf16_modes(ops, cid):
    """The same inputs through both modes, errors against float64 of the unsplit operands: the bf16x3 worst |error| is at most
    1/64 of the bf16 mode's.  (The representation errors stand as 3 * 2^-16 to 2 * 2^-9 per product, 1/170; emulated on the CPU
    the worst errors stand at about 1/500.)"""
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    c = _case(cid)
    one = R.Case(c.id, c.op, c.M, c.N, c.K, c.route, acts=(0,), biases=(False,), x_acts=(0,), dX=c.dX, dW=c.dW)
    worst = {}
    for precision in (PREC, "bf16"):
        rng = np.random.RandomState(77)
        if c.op == "fwd":
            worst[precision] = _run_fwd(ops, one, n_cu, rng, precision)
        else:
            worst[precision] = max(_run_bwd(ops, one, n_cu, rng, precision))
    print("%s: worst |err| bf16x3 %.3e, bf16 %.3e, ratio 1/%.0f" % (cid, worst[PREC], worst["bf16"], worst["bf16"] / worst[PREC]))
    assert worst["bf16"] > 0 and worst[PREC] <= worst["bf16"] / 64


@pytest.mark.gpu
def test_bf16x3_differs_from_fp32_and_bf16(ops):
    """The flag changes the arithmetic (the mode is on, and is not the bf16 mode): three different sets of bits."""
    rng = np.random.RandomState(2)
    X = torch.from_numpy(rng.randn(512, 512).astype(np.float32)).to(DEV)
    W = torch.from_numpy((rng.randn(512, 512) / 23).astype(np.float32)).to(DEV)
    Y = [torch.empty(512, 512, device=DEV) for _ in range(3)]
    ops.linear_fwd(X, W, None, Y[0], 0)
    ops.linear_fwd(X, W, None, Y[1], 0, bf16=True)
    ops.linear_fwd(X, W, None, Y[2], 0, precision=PREC)
    torch.cuda.synchronize()
    assert not torch.equal(Y[2], Y[0]) and not torch.equal(Y[2], Y[1])
    Y3 = torch.empty(512, 512, device=DEV)
    ops.linear_fwd(X, W, None, Y3, 0, precision="bf16")         # the other spelling of bf16=True
    torch.cuda.synchronize()
    assert torch.equal(Y3, Y[1])


@pytest.mark.gpu
@pytest.mark.parametrize("bad", [float("nan"), float("inf")])
def test_non_finite_input_stays_in_its_row(ops, bad):
    """One NaN / Inf in row 17 of X: that row of Y is non-finite, every other row finite (the lo plane of a non-finite element is
    0, so it reaches no other row through the staging)."""
    rng = np.random.RandomState(3)
    M, N, K = 200, 96, 160
    X = rng.randn(M, K).astype(np.float32)
    X[17, 70] = bad
    W = (rng.randn(N, K) / np.sqrt(K)).astype(np.float32)
    Y = torch.full((M, N), SENTINEL, device=DEV)
    ops.linear_fwd(torch.from_numpy(X).to(DEV), torch.from_numpy(W).to(DEV), None, Y, 0, precision=PREC)
    torch.cuda.synchronize()
    fin = torch.isfinite(Y).cpu()
    assert not fin[17].any(), "row 17 has finite outputs"
    assert fin[:17].all() and fin[18:].all(), "a non-finite value left its row"
    # ... and the same for W: its row is a column of Y
    X[17, 70] = 1.0
    W[5, 3] = bad
    ops.linear_fwd(torch.from_numpy(X).to(DEV), torch.from_numpy(W).to(DEV), None, Y, 0, precision=PREC)
    torch.cuda.synchronize()
    fin = torch.isfinite(Y).cpu()
    assert not fin[:, 5].any() and fin[:, :5].all() and fin[:, 6:].all()


@pytest.mark.gpu
@pytest.mark.parametrize("M", [256, 1024, 8200])
@pytest.mark.parametrize("layers", [C3_TOP, C3_BOT], ids=["top", "bot"])
def test_mlp_wgrad_ex_vs_float64_and_fused_sgd(ops, M, layers):
    """cdlrm_mlp_wgrad_ex(CDLRM_GEMM_BF16X3) with padded X rows: eligible layers against float64 of the unsplit operands under the
    bf16x3 bound, the others under the fp32 bound of their route AND bit-identical to the all-fp32 call; db from the unsplit dZ;
    two launches bit-identical; cdlrm_mlp_wgrad_sgd_ex bit-identical to cdlrm_mlp_wgrad_ex followed by sgd_step."""
    rng = np.random.RandomState(M + len(layers))
    plan = B16._plan(ops, M, layers, device=DEV, ldx_pad=4, precision=PREC)
    routes = ops.mlp_wgrad_route(plan, n_cu=torch.cuda.get_device_properties(0).multi_processor_count)
    Xs, dZs, dWs, dbs = plan._keep[:4]
    for x in Xs:
        x.copy_(torch.from_numpy(np.maximum(rng.randn(*x.shape), 0).astype(np.float32)))
    for d in dZs:
        d.copy_(torch.from_numpy(rng.randn(*d.shape).astype(np.float32)))
    ops.mlp_wgrad(plan)
    torch.cuda.synchronize()
    first = [t.clone() for t in dWs + dbs]
    for t in dWs + dbs:
        t.fill_(SENTINEL)
    ops.mlp_wgrad(plan)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(first, dWs + dbs)), "two launches differ"
    dW32 = [torch.full_like(w, SENTINEL) for w in dWs]
    db32 = [torch.full_like(b, SENTINEL) for b in dbs]
    plan32 = ops.WgradPlan(Xs, dZs, dW32, db32, ops.mlp_wgrad_work(M, [n for n, _ in layers], [k for _, k in layers], DEV))
    ops.mlp_wgrad(plan32)
    torch.cuda.synchronize()
    if M <= 256:
        assert all(r["splits"] == 1 for r, (n, k) in zip(routes, layers) if n >= 32 and k >= 32), routes
    for i, (n, k) in enumerate(layers):
        x, dz = Xs[i].cpu().numpy().astype(np.float64), dZs[i].cpu().numpy().astype(np.float64)
        r = routes[i]
        ref, mag = dz.T @ x, np.abs(dz).T @ np.abs(x)
        if n >= 32 and k >= 32:
            assert r["family"] == "bf16x3", r
            k_eff = (M if r["splits"] == 1 else -(-M // r["splits"]) + 64 + r["splits"]) + 3
            assert_within_x3(dWs[i].cpu().numpy(), ref, mag, k_eff, "layer %d dW" % i)
            assert not torch.equal(dW32[i], dWs[i]), "layer %d: the bits of the fp32 plan" % i
        else:
            assert r["family"] not in ("bf16", "bf16x3"), r
            assert torch.equal(dW32[i], dWs[i]) and torch.equal(db32[i], dbs[i]), "layer %d: fp32 layer differs from fp32 mode" % i
            k_eff = (M if r["splits"] == 1 else -(-M // r["splits"]) + 32 + r["splits"]) + 3
            R.assert_within(dWs[i].cpu().numpy(), ref, mag, k_eff, "layer %d dW" % i, "bf16")
        R.assert_within(dbs[i].cpu().numpy(), dz.sum(0), np.abs(dz).sum(0), k_eff, "layer %d db" % i, "bf16")
    # fused SGD: the same bits as the gradients followed by the SGD step
    lr = 0.05
    Ws = [torch.from_numpy(rng.randn(n, k).astype(np.float32)).to(DEV) for n, k in layers]
    bs = [torch.from_numpy(rng.randn(n).astype(np.float32)).to(DEV) for n, _ in layers]
    W_ref, b_ref = [w.clone() for w in Ws], [b.clone() for b in bs]
    ops.mlp_wgrad(plan)
    for w, g in zip(W_ref, dWs):
        ops.sgd_step(w, g, lr)
    for b, g in zip(b_ref, dbs):
        ops.sgd_step(b, g, lr)
    plan.set_params(Ws, bs)
    ops.mlp_wgrad(plan, lr=lr)
    torch.cuda.synchronize()
    for i in range(len(layers)):
        assert torch.equal(Ws[i], W_ref[i]), "layer %d: fused SGD weight differs" % i
        assert torch.equal(bs[i], b_ref[i]), "layer %d: fused SGD bias differs" % i
        assert torch.equal(dWs[i], first[i]), "layer %d: gradient left behind differs" % i
