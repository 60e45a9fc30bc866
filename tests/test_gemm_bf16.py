"""The opt-in bf16 matrix-core mode of the MLP GEMMs (CDLRM_GEMM_BF16, csrc/gemm_bf16.h) against float64.

Numerics contract ("bf16 mode"): a layer with K >= 32 and N >= 32 runs its forward, dgrad and weight
gradient on v_mfma_f32_32x32x16_bf16; each operand element is rounded once to bf16 (round-to-nearest-even), products are exact,
the sums are fp32 in a fixed order, and every epilogue (bias, activation, act' mask, bias gradient, slab reduction, SGD) is fp32.
So the reference here is float64 computed from the bf16-ROUNDED operands (`x.to(torch.bfloat16).double()`), and the bound is
the one of test_gemm_routes.py: |got - ref| <= C * K_eff * 2^-24 * (|A| @ |B|) -- the rigorous bound of an fp32 summation of
K_eff exact products in any order.  A kernel that skipped the rounding (products of the fp32 values) or rounded the wrong
operand is off by ~2^-9 of each product and fails it; the CPU negative controls below show that.  The bias gradient is a column
sum of the UNROUNDED dZ (an fp32 epilogue) and is checked against that.

One table of cases, each with its declared route, serves three checks as in test_gemm_routes.py:
  * CPU: the route queries give the declared route at 256 CUs; with the flag set, ineligible shapes report the fp32 route;
  * CPU: one TrainEngine step with matmul_precision="bf16" on the CPU test double (c2 / c3 / c5 widths, per-rank batches
    1024 ... 65536): every flagged launch resolves to a route of the table, no ineligible layer carries the flag;
  * GPU: each case against float64, NaN in input pitch gaps, sentinels in output gaps, two launches bit-identical.
"""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import test_gemm_routes as R      # noqa: E402  (the comparator, operand helpers, route strings and step recorder)

DEV = "cuda:0"
N_CU = 256
SENTINEL = R.SENTINEL
PITCH_FEAT = R.PITCH_FEAT


def route_str(r):
    """'bf16 64x128 v11 /16' for the bf16 family, test_gemm_routes.route_str for the others."""
    if r is None or r["family"] != "bf16":
        return R.route_str(r)
    s = "bf16 %dx%d v%d%d" % (64 * r["tm"], 64 * r["tn"], r["vec_a"], r["vec_b"])
    if r["splits"] > 1:
        s += " /%d" % r["splits"]
    return s


class Case(R.Case):
    pass


F = lambda cid, M, N, K, route, **kw: Case(cid, "fwd", M, N, K, route, **kw)     # noqa: E731
B = lambda cid, M, N, K, route, **kw: Case(cid, "bwd", M, N, K, route, **kw)     # noqa: E731

CASES = [
    # ---- forward: Y = act(bf16(X) bf16(W)^T + b) ----
    F("fwd_c3_top0", 8192, 512, 480, "bf16 64x64 v11"),
    F("fwd_c3_512", 8192, 512, 512, "bf16 64x64 v11"),
    F("fwd_c3_256", 8192, 256, 512, "bf16 64x64 v11"),
    F("fwd_c3_bot_feat", 8192, 128, 256, "bf16 64x64 v11", ldy=PITCH_FEAT),
    F("fwd_c5_128x128", 65536, 512, 480, "bf16 128x128 v11", acts=(1,)),
    F("fwd_c5_256", 65536, 256, 512, "bf16 128x128 v11", acts=(2,), biases=(True,)),
    F("fwd_64x128", 16384, 512, 96, "bf16 64x128 v11"),
    F("fwd_ragged_m1000", 1000, 512, 480, "bf16 64x64 v11"),
    F("fwd_ragged_m8200", 8200, 264, 64, "bf16 64x64 v11"),
    F("fwd_k479_v00", 4096, 512, 479, "bf16 64x64 v00"),
    F("fwd_pitch_v01", 4096, 256, 480, "bf16 64x64 v01", ldx=481),
    F("fwd_unaligned_w_v10", 4096, 256, 480, "bf16 64x64 v10", offw=2),
    F("fwd_n479", 4096, 479, 512, "bf16 64x64 v11", ldy=480),
    F("fwd_min_32x32", 2048, 32, 32, "bf16 64x64 v11"),
    F("fwd_c2_feat_64x128", 65536, 32, 256, "bf16 64x128 v11", acts=(1,), biases=(True,), ldy=R.PITCH_FEAT_C2),
    # ---- dgrad: dX = (bf16(dZ) bf16(W)) * act'(X) ----
    B("dgrad_c3_512", 8192, 512, 512, ("bf16 64x64 v11", None)),
    B("dgrad_c3_480", 8192, 512, 480, ("bf16 64x64 v11", None)),
    B("dgrad_c3_256_feat", 8192, 128, 256, ("bf16 64x64 v11", None), ldy=PITCH_FEAT, x_acts=(1, 2)),
    B("dgrad_mask_pitch", 8192, 256, 512, ("bf16 64x64 v11", None), ldx=514, x_acts=(1, 2)),
    B("dgrad_padded_dx", 8192, 512, 480, ("bf16 64x64 v11", None), lddx=484, x_acts=(0,)),
    B("dgrad_n479_v01", 4096, 479, 512, ("bf16 64x64 v01", None), ldy=480, x_acts=(0, 1)),
    B("dgrad_c5", 65536, 512, 480, ("bf16 128x128 v11", None), x_acts=(1,)),
    B("dgrad_ragged_m1000", 1000, 256, 480, ("bf16 64x64 v11", None)),
    B("dgrad_c2_384", 65536, 512, 384, ("bf16 128x128 v11", None), x_acts=(0,)),
    B("dgrad_c2_feat", 65536, 32, 256, ("bf16 128x128 v11", None), ldy=R.PITCH_FEAT_C2, x_acts=(1,)),
    # ---- weight gradient: dW = bf16(dZ)^T bf16(X) in split-M slabs, db = column sums of dZ (fp32) ----
    B("wgrad_split16", 8192, 512, 512, (None, "bf16 64x64 v11 /16"), dX=False, dW=True),
    B("wgrad_act_relu", 8192, 256, 480, ("bf16 64x64 v11", "bf16 64x64 v11 /32"), act=1, dW=True, x_acts=(1,)),
    B("wgrad_act_sigmoid", 4096, 128, 256, ("bf16 64x64 v11", "bf16 64x64 v11 /16"), act=2, dW=True, x_acts=(2,)),
    B("wgrad_short_v10", 1000, 256, 70, (None, "bf16 64x64 v10"), dX=False, dW=True),
    B("wgrad_ragged_m8200", 8200, 264, 480, (None, "bf16 64x64 v11 /26"), dX=False, dW=True),
]

# with the flag set, these stay on their fp32 route (the route the same call takes without it)
FALLBACK = [
    F("fb_k13", 8192, 512, 13, None),
    F("fb_k13_ragged", 1000, 256, 13, None),
    F("fb_k31", 2048, 256, 31, None),
    F("fb_n1_head", 8192, 1, 256, None),
    F("fb_n31", 2048, 31, 512, None),
    B("fb_wgrad_k13", 2048, 512, 13, None, dW=True, x_acts=(0,)),
    B("fb_dgrad_n1", 8192, 1, 256, None),
    B("fb_wgrad_n16", 8192, 16, 512, None, dW=True, x_acts=(0,)),
]


def _query(ops, case, v, mk, n_cu, bf16):
    c = case
    X = mk(c.M, c.K, c.ldx, c.offx)
    W = mk(c.N, c.K, c.K, c.offw)
    if c.op == "fwd":
        b = mk(1, c.N, c.N, c.offb) if v["bias"] else None
        return route_str(ops.linear_fwd_route(X, W, b, mk(c.M, c.N, c.ldy, c.offy), v["act"], alone=c.alone, n_cu=n_cu,
                                              bf16=bf16))
    Y = mk(c.M, c.N, c.ldy, c.offy)
    dY = mk(c.M, c.N, c.ldy, c.offy)
    dX = mk(c.M, c.K, c.lddx, c.offdx) if c.dX else None
    dW = mk(c.N, c.K, c.K, 0) if c.dW else None
    db = mk(1, c.N, c.N, 0) if c.dW else None
    r = ops.linear_bwd_route(X, W, Y if c.act else None, dY, dX, dW, db, c.act, x_act=v["x_act"], alone=c.alone, n_cu=n_cu,
                             bf16=bf16)
    return tuple(route_str(x) for x in r)


ops = R.ops      # the module fixture: builds the library if needed


# ---- CPU ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", CASES, ids=lambda c: c.id)
def test_declared_bf16_route_at_256_cus(ops, case):
    for v in case.variants():
        got = _query(ops, case, v, R.Addr, N_CU, True)
        assert got == case.route, "%s %r: routed to %r, the table declares %r" % (case.id, v, got, case.route)
        # ... and without the flag, never the bf16 family (the fp32 routes are what they were)
        plain = _query(ops, case, v, R.Addr, N_CU, False)
        assert "bf16" not in str(plain), (case.id, plain)


@pytest.mark.parametrize("case", FALLBACK, ids=lambda c: c.id)
def test_ineligible_shapes_keep_their_fp32_route(ops, case):
    for v in case.variants():
        flagged = _query(ops, case, v, R.Addr, N_CU, True)
        assert flagged == _query(ops, case, v, R.Addr, N_CU, False), (case.id, v, flagged)
        assert "bf16" not in str(flagged)


def _plan(ops, M, layers, device=None, ldx_pad=0, precision="bf16"):
    """A WgradPlan over layers [(N, K), ...] at batch M (device None: fake-address tensors on the CPU for the route query)."""
    dev = device or "cpu"
    Xs = [torch.empty(M, K + ldx_pad, device=dev)[:, :K] for _, K in layers]
    dZs = [torch.empty(M, N, device=dev) for N, _ in layers]
    dWs = [torch.empty(N, K, device=dev) for N, K in layers]
    dbs = [torch.empty(N, device=dev) for N, _ in layers]
    work = ops.mlp_wgrad_work(M, [n for n, _ in layers], [k for _, k in layers], dev, precision=precision)
    if device is None:          # host memory: 256-byte align it as the device allocator does
        raw = torch.empty(work.numel() + 256, dtype=torch.uint8)
        work = raw[(-raw.data_ptr()) % 256:][:work.numel()]
    return ops.WgradPlan(Xs, dZs, dWs, dbs, work, precision=precision)


C3_TOP = [(512, 480), (512, 512), (256, 512), (1, 256)]
C3_BOT = [(512, 13), (256, 512), (128, 256)]


@pytest.mark.parametrize("M", [1024, 2048, 8192, 65536])
def test_mlp_wgrad_route(ops, M):
    """cdlrm_mlp_wgrad_route: the eligible layers of a plan report the bf16 family with the group's slab count, the 13-wide and
    1-wide layers the route the fp32 plan gives them; without the flag no layer is bf16."""
    for layers in (C3_TOP, C3_BOT):
        plan = _plan(ops, M, layers)
        got = ops.mlp_wgrad_route(plan, n_cu=N_CU)
        fp = ops.mlp_wgrad_route(plan, n_cu=N_CU, precision="fp32")
        assert all(r is not None and r["family"] != "bf16" for r in fp), fp
        splits = {r["splits"] for r, (n, k) in zip(got, layers) if n >= 32 and k >= 32}
        assert len(splits) == 1, got
        for r, (n, k) in zip(got, layers):
            if n >= 32 and k >= 32:
                assert route_str(r).startswith("bf16 64x64 v11"), (M, n, k, r)
            else:
                assert r["family"] != "bf16", (M, n, k, r)
        # the fp32 layers keep the route -- kernel and slab count -- they have in the all-fp32 call
        for r, r32, (n, k) in zip(got, fp, layers):
            if not (n >= 32 and k >= 32):
                assert r == r32, (M, n, k, r, r32)


def test_fp32_work_sizes_unchanged(ops):
    """The flags-word size query with flags 0 is the fp32 one, for every batch and layer set."""
    from cdlrm_amd import _lib
    import ctypes as C
    for M in (1, 1000, 2048, 8192, 65536):
        for layers in (C3_TOP, C3_BOT):
            NA = C.c_int32 * len(layers)
            N, K = NA(*[n for n, _ in layers]), NA(*[k for _, k in layers])
            assert _lib.lib().cdlrm_mlp_wgrad_work_bytes_ex(len(layers), M, N, K, 0) == \
                _lib.lib().cdlrm_mlp_wgrad_work_bytes(len(layers), M, N, K)


def _bf(a):
    """float64 of the bf16-rounded values (round-to-nearest-even), as the kernels round."""
    return torch.as_tensor(np.asarray(a, dtype=np.float32)).to(torch.bfloat16).double().numpy()


def test_comparator_negative_controls():
    """The bf16 reference with the fp32-chain bound accepts a correct fp32 sum of the rounded products and rejects (a) the
    product of the UNROUNDED operands, (b) one operand rounded, the other not, (c) a dropped K tile of 64."""
    rng = np.random.RandomState(5)
    M, N, K = 64, 48, 480
    A = rng.randn(M, K).astype(np.float32)
    Bm = (rng.randn(K, N) / np.sqrt(K)).astype(np.float32)
    Ab, Bb = _bf(A), _bf(Bm)
    ref, mag = Ab @ Bb, np.abs(Ab) @ np.abs(Bb)
    ok = R._seq_fp32(Ab.astype(np.float32), Bb.astype(np.float32))
    R.assert_within(ok, ref, mag, K, "correct bf16 GEMM")
    with pytest.raises(AssertionError):
        R.assert_within(R._seq_fp32(A, Bm), ref, mag, K, "unrounded operands")
    with pytest.raises(AssertionError):
        R.assert_within(R._seq_fp32(Ab.astype(np.float32), Bm), ref, mag, K, "B not rounded")
    with pytest.raises(AssertionError):
        R.assert_within(R._seq_fp32(Ab.astype(np.float32), Bb.astype(np.float32), skip=set(range(128, 192))), ref, mag, K,
                        "K tile dropped")


# ---- CPU: the engine's bf16 step ----------------------------------------------------------------------------------------

STEP_CONFIGS = dict(R.STEP_CONFIGS)


def _record_bf16_step(config, Bsz):
    """One TrainEngine(matmul_precision="bf16") step on the CPU test double, with a shim around tests/fake_ops.py that accepts
    the bf16 keyword and the plans' precision and records: linear_fwd / linear_bwd calls with their flag, WgradPlans, and the
    precision of every mlp_wgrad call."""
    import fake_ops
    calls, plans, used = [], [], []

    def desc(t):
        return None if t is None else (tuple(t.shape), t.stride(0), (t.data_ptr() % 16) // 4)

    def lf(X, W, b, Y, act, stream=None, alone=False, bf16=False):
        calls.append((bf16, ("fwd", desc(X), desc(W), desc(b), desc(Y), act, alone)))
        return fake_ops.linear_fwd(X, W, b, Y, act, stream, alone)

    def lb(X, W, Y, dY, dX, dW, db, act, work, stream=None, x_act=0, alone=False, bf16=False):
        calls.append((bf16, ("bwd", desc(X), desc(W), desc(Y), desc(dY), desc(dX), desc(dW), desc(db), act, x_act, alone)))
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
    _run_engine_step(config, Bsz, shim)
    return calls, plans, used


def _run_engine_step(config, Bsz, shim):
    """test_gemm_routes._record_step's engine step, on `shim` as the engine's ops module."""
    import fake_ops
    import cdlrm_amd.engine as engine
    import cdlrm_amd.model_no_ddp as Mo
    from oracle import cdlrm_oracle as O
    cfg = STEP_CONFIGS[config]
    saved = (engine.ops, Mo.ops, Mo.Embedding_Table_Group.__dict__.get("device_pointers"))
    engine.ops, Mo.ops = shim, shim
    Mo.Embedding_Table_Group.device_pointers = lambda self: self._fake_ptrs
    try:
        T, rows, D = 26, 40, cfg["D"]
        ln_emb = np.array([rows] * T)
        nf = T + 1
        ln_top = np.array([D + nf * (nf - 1) // 2] + cfg["top"])
        host = O.init_host_tables([int(x) for x in ln_emb], D)
        eg = Mo.Embedding_Table_Group(D, ln_emb, init="empty_meta")
        for k in range(T):
            eg.emb_l[k].weight.data = host[k]
        eg._fake_ptrs = fake_ops.register_host(host)
        eg._pinned = True
        np.random.seed(1)
        torch.manual_seed(1)
        cg = Mo.Embedding_Table_Cache_Group(D, ln_emb, 64, Bsz, 4)
        dl = Mo.DLRM_Net(np.array(cfg["bot"]), ln_top, "dot", False, True, -1, ln_top.size - 2, 0.0)
        eng = engine.TrainEngine(cg, dl, eg, lr=0.1, lr_embeds=0.1, matmul_precision="bf16")
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


@pytest.mark.parametrize("config,batch", [(c, b) for c in STEP_CONFIGS for b in (1024, 2048, 4096, 8192, 65536)])
def test_bf16_training_step_routes_are_in_the_table(ops, config, batch):
    """Every GEMM launch of a bf16 engine step: eligible layers carry the flag and resolve to a bf16 route of the table (with its
    epilogue arguments and strided operands), ineligible ones (13-wide input, 1-wide head) carry no flag; the weight gradients
    go through bf16 plans only."""
    table = set()
    for c in CASES:
        table.update(c.keys())
    calls, plans, used = _record_bf16_step(config, batch)
    assert sum(c[1][0] == "fwd" for c in calls) >= 5 and sum(c[1][0] == "bwd" for c in calls) >= 3, calls
    missing, flagged = [], 0
    for bf16, call in calls:
        W = call[2]
        eligible = W[0][0] >= 32 and W[0][1] >= 32
        assert bool(bf16) == eligible, ("flag on an ineligible layer" if bf16 else "eligible layer without the flag", call)
        if not bf16:
            continue
        flagged += 1
        key = _bf16_key(ops, call)
        if key not in table:
            missing.append((key, call))
    assert flagged >= 4
    assert not missing, "bf16 step routes the table lacks:\n" + "\n".join("%r  <- %r" % m for m in missing)
    assert used and set(used) == {"bf16"}, used
    assert any(p.precision == "bf16" for p in plans)


def _bf16_key(ops, call):
    def mk(d):
        return None if d is None else R.Addr(d[0][0], d[0][1] if len(d[0]) > 1 else d[0][0], d[1], d[2])
    if call[0] == "fwd":
        _, X, W, b, Y, act, alone = call
        b_op = None if b is None else R.Addr(1, b[0][0], b[0][0], b[2])
        r = route_str(ops.linear_fwd_route(mk(X), mk(W), b_op, mk(Y), act, alone=alone, n_cu=N_CU, bf16=True))
        return ("fwd", r, act, b is not None, X[1] != X[0][1], Y[1] != Y[0][1])
    _, X, W, Y, dY, dX, dW, db, act, x_act, alone = call
    db_op = None if db is None else R.Addr(1, db[0][0], db[0][0], db[2])
    r = tuple(route_str(x) for x in ops.linear_bwd_route(mk(X), mk(W), mk(Y), mk(dY), mk(dX), mk(dW), db_op, act, x_act=x_act,
                                                         alone=alone, n_cu=N_CU, bf16=True))
    return ("bwd", r, act, x_act if dX is not None else None, dW is not None, X[1] != X[0][1], dY[1] != dY[0][1],
            (dX[1] != dX[0][1]) if dX is not None else None)


# ---- GPU: every case against float64 of the rounded operands ------------------------------------------------------------

def _run_fwd(ops, c, n_cu, rng):
    nan = float("nan")
    X = rng.randn(c.M, c.K).astype(np.float32)
    W = (rng.randn(c.N, c.K) / np.sqrt(c.K)).astype(np.float32)
    bias = rng.randn(c.N).astype(np.float32)
    Xd, _ = R._dev_operand(c.M, c.K, c.ldx, c.offx, torch.from_numpy(X), nan)
    Wd, _ = R._dev_operand(c.N, c.K, c.K, c.offw, torch.from_numpy(W), nan)
    bd, _ = R._dev_operand(1, c.N, c.N, c.offb, torch.from_numpy(bias)[None], nan)
    bd = bd[0]
    Xb, Wb = _bf(X), _bf(W)
    pre, mag = Xb @ Wb.T, np.abs(Xb) @ np.abs(Wb).T
    for v in c.variants():
        Yd, _ = R._dev_operand(c.M, c.N, c.ldy, c.offy, None, SENTINEL)
        b = bd if v["bias"] else None
        got = route_str(ops.linear_fwd_route(Xd, Wd, b, Yd, v["act"], alone=c.alone, n_cu=n_cu, bf16=True))
        assert got == c.route, "%s %r: the library takes %r, the case is meant for %r" % (c.id, v, got, c.route)
        ops.linear_fwd(Xd, Wd, b, Yd, v["act"], alone=c.alone, bf16=True)
        Y1 = Yd.clone()
        ops.linear_fwd(Xd, Wd, b, Yd, v["act"], alone=c.alone, bf16=True)
        torch.cuda.synchronize()
        assert torch.equal(Y1, Yd), "%s %r: two calls differ" % (c.id, v)
        assert R._gap_ok(Yd, c.ldy, c.N, SENTINEL), "%s %r: Y's pitch gap was written" % (c.id, v)
        ref = R.act_fwd(pre + bias if v["bias"] else pre, v["act"])
        m = mag + np.abs(bias) if v["bias"] else mag
        R.assert_within(Yd.cpu().numpy(), ref, m, c.K + 1, "%s %r Y" % (c.id, v), "bf16")


def _run_bwd(ops, c, n_cu, rng):
    nan = float("nan")
    W = (rng.randn(c.N, c.K) / np.sqrt(c.K)).astype(np.float32)
    dY = rng.randn(c.M, c.N).astype(np.float32)
    Yv = {0: None, 1: np.maximum(rng.randn(c.M, c.N), 0), 2: 1 / (1 + np.exp(-rng.randn(c.M, c.N)))}[c.act]
    Yv = None if Yv is None else Yv.astype(np.float32)
    Wd, _ = R._dev_operand(c.N, c.K, c.K, c.offw, torch.from_numpy(W), nan)
    Yd = None if Yv is None else R._dev_operand(c.M, c.N, c.ldy, c.offy, torch.from_numpy(Yv), nan)[0]
    # dZ as the kernel computes it in fp32 (dY * act'(Y): exact for ReLU; one fp32 rounding for the sigmoid's), then rounded
    dZ32 = dY * (((1.0 - Yv) * Yv).astype(np.float32) if c.act == 2 else (Yv > 0).astype(np.float32) if c.act == 1 else 1.0)
    dZ32 = dZ32.astype(np.float32)
    dZb, Wb = _bf(dZ32), _bf(W)
    prod, pmag = (dZb @ Wb, np.abs(dZb) @ np.abs(Wb)) if c.dX else (None, None)
    work = ops.linear_bwd_work(c.M, c.N, c.K, DEV)
    for v in c.variants():
        xa = v["x_act"]
        Xv = {0: rng.randn(c.M, c.K), 1: np.maximum(rng.randn(c.M, c.K), 0), 2: 1 / (1 + np.exp(-rng.randn(c.M, c.K)))}[xa]
        Xv = Xv.astype(np.float32)
        Xd, _ = R._dev_operand(c.M, c.K, c.ldx, c.offx, torch.from_numpy(Xv), nan)
        dYd, _ = R._dev_operand(c.M, c.N, c.ldy, c.offy, torch.from_numpy(dY), nan)
        dXd = R._dev_operand(c.M, c.K, c.lddx, c.offdx, None, SENTINEL)[0] if c.dX else None
        dWd = torch.full((c.N, c.K), SENTINEL, device=DEV) if c.dW else None
        dbd = torch.full((c.N,), SENTINEL, device=DEV) if c.dW else None
        got = ops.linear_bwd_route(Xd, Wd, Yd, dYd, dXd, dWd, dbd, c.act, x_act=xa, alone=c.alone, n_cu=n_cu, bf16=True)
        got_route = tuple(route_str(x) for x in got)
        assert got_route == c.route, "%s %r: the library takes %r, the case is meant for %r" % (c.id, v, got_route, c.route)
        ops.linear_bwd(Xd, Wd, Yd, dYd, dXd, dWd, dbd, c.act, work, x_act=xa, alone=c.alone, bf16=True)
        torch.cuda.synchronize()
        outs1 = [t.clone() for t in (dXd, dWd, dbd) if t is not None]
        dY2, _ = R._dev_operand(c.M, c.N, c.ldy, c.offy, torch.from_numpy(dY), nan)
        ops.linear_bwd(Xd, Wd, Yd, dY2, dXd, dWd, dbd, c.act, work, x_act=xa, alone=c.alone, bf16=True)
        torch.cuda.synchronize()
        outs2 = [t for t in (dXd, dWd, dbd) if t is not None]
        assert all(torch.equal(a, b) for a, b in zip(outs1, outs2)), "%s %r: two calls differ" % (c.id, v)
        assert R._gap_ok(dYd, c.ldy, c.N, nan), "%s %r: dY's pitch gap was written" % (c.id, v)
        if c.act:
            R.assert_within(dYd.cpu().numpy(), dZ32.astype(np.float64), np.abs(dZ32), 3, "%s %r dZ" % (c.id, v), "bf16")
        if c.dX:
            assert R._gap_ok(dXd, c.lddx, c.K, SENTINEL), "%s %r: dX's pitch gap was written" % (c.id, v)
            m = R.act_grad(Xv.astype(np.float64), xa)
            R.assert_within(dXd.cpu().numpy(), prod * m, pmag * np.abs(m), c.N + 5, "%s %r dX" % (c.id, v), "bf16")
        if c.dW:
            splits = got[1]["splits"]
            k_eff = (c.M if splits == 1 else -(-c.M // splits) + 64 + splits) + 3
            Xb = _bf(Xv)
            R.assert_within(dWd.cpu().numpy(), dZb.T @ Xb, np.abs(dZb).T @ np.abs(Xb), k_eff, "%s %r dW" % (c.id, v), "bf16")
            # the bias gradient: column sums of the UNROUNDED dZ (fp32 epilogue)
            dz64 = dZ32.astype(np.float64)
            R.assert_within(dbd.cpu().numpy(), dz64.sum(0), np.abs(dz64).sum(0), k_eff, "%s %r db" % (c.id, v), "bf16")


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=lambda c: c.id)
def test_bf16_route_vs_float64(ops, case):
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    rng = np.random.RandomState(sum(map(ord, case.id)))
    if case.op == "fwd":
        _run_fwd(ops, case, n_cu, rng)
    else:
        _run_bwd(ops, case, n_cu, rng)


@pytest.mark.gpu
def test_bf16_differs_from_fp32(ops):
    """The flag changes the arithmetic (the mode is on): the same forward without it gives different bits."""
    rng = np.random.RandomState(2)
    X = torch.from_numpy(rng.randn(4096, 512).astype(np.float32)).to(DEV)
    W = torch.from_numpy((rng.randn(512, 512) / 23).astype(np.float32)).to(DEV)
    Y0, Y1 = torch.empty(4096, 512, device=DEV), torch.empty(4096, 512, device=DEV)
    ops.linear_fwd(X, W, None, Y0, 0)
    ops.linear_fwd(X, W, None, Y1, 0, bf16=True)
    torch.cuda.synchronize()
    assert not torch.equal(Y0, Y1)


@pytest.mark.gpu
@pytest.mark.parametrize("M,layers,pad", [(256, C3_TOP, 0), (1024, C3_TOP, 0), (1024, C3_BOT, 0), (8192, C3_TOP, 0),
                                          (8192, C3_BOT, 0), (8200, C3_BOT, 4), (65536, C3_TOP[1:3], 0)])
def test_mlp_wgrad_ex_vs_float64_and_fused_sgd(ops, M, layers, pad):
    """cdlrm_mlp_wgrad_ex(CDLRM_GEMM_BF16): eligible layers against float64 of the rounded operands, the others against the fp32
    bound of their route AND bit-identical to the all-fp32 call; db from the unrounded dZ; two launches bit-identical;
    cdlrm_mlp_wgrad_sgd_ex bit-identical to cdlrm_mlp_wgrad_ex followed by sgd_step (M = 256: one slab, the SGD step without a
    reduction pass to ride in)."""
    rng = np.random.RandomState(M + len(layers))
    plan = _plan(ops, M, layers, device=DEV, ldx_pad=pad)
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
    # the fp32 layers: the bits of the all-fp32 call on the same inputs
    dW32 = [torch.full_like(w, SENTINEL) for w in dWs]
    db32 = [torch.full_like(b, SENTINEL) for b in dbs]
    plan32 = ops.WgradPlan(Xs, dZs, dW32, db32, ops.mlp_wgrad_work(M, [n for n, _ in layers], [k for _, k in layers], DEV))
    ops.mlp_wgrad(plan32)
    torch.cuda.synchronize()
    for i, (n, k) in enumerate(layers):
        if not (n >= 32 and k >= 32):
            assert torch.equal(dW32[i], dWs[i]) and torch.equal(db32[i], dbs[i]), "layer %d: fp32 layer differs from fp32 mode" % i
    if M <= 256:
        assert all(r["splits"] == 1 for r, (n, k) in zip(routes, layers) if n >= 32 and k >= 32), routes
    for i, (n, k) in enumerate(layers):
        x, dz = Xs[i].cpu().numpy(), dZs[i].cpu().numpy()
        r = routes[i]
        if n >= 32 and k >= 32:
            assert r["family"] == "bf16", r
            a, b = _bf(dz), _bf(x)
            k_eff = (M if r["splits"] == 1 else -(-M // r["splits"]) + 64 + r["splits"]) + 3
        else:
            assert r["family"] != "bf16", r
            a, b = dz.astype(np.float64), x.astype(np.float64)
            k_eff = (M if r["splits"] == 1 else -(-M // r["splits"]) + 32 + r["splits"]) + 3
        R.assert_within(dWs[i].cpu().numpy(), a.T @ b, np.abs(a).T @ np.abs(b), k_eff, "layer %d dW" % i, "bf16")
        d64 = dz.astype(np.float64)
        R.assert_within(dbs[i].cpu().numpy(), d64.sum(0), np.abs(d64).sum(0), k_eff, "layer %d db" % i, "bf16")
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
