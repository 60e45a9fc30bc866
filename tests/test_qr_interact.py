"""The quotient-remainder compose inside the interaction kernels (csrc/qr_interact.hip): cdlrm_qr_interact_fwd / _bwd bit for bit
against qr_cached_fwd + interact_fwd / interact_bwd and against a plain float64 reference, their refusals, and a TrainEngine with
fuse_qr.

Bounds (2^-24 = one fp32 rounding, C_BOUND of test_gemm_routes; |P|a the composition of absolute values):
  pairs   k_eff = D + 2, mag = |P|a |P|a^T: a D-long fma chain over operands that each carry one rounding (the compose)
  dfeat   k_eff = F + 3, mag = |G + G^T| |P|a (+ |dR| head on row 0), row 0 times |act'|; 8 ulp for the activation factor
No tolerance here is a measured number.
"""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import test_gemm_routes as R      # noqa: E402
from test_gemm_routes import assert_within, SENTINEL, _dev_operand, _gap_ok, ops      # noqa: E402,F401  (ops: the fixture)
from test_bag_interact import make_ctx, pad4, ref64, SETS, WAYS, AUX      # noqa: E402  (61 sets x 4 ways + 512 auxiliary rows)

DEV = R.DEV
NAN = float("nan")

# id: D, F, B, c, op (0 mult, 1 add), itself, the plain tables (collisions == 0; their Wr rows hold NaN)
CASES = {
    "d32": (32, 27, 5, 4, 0, 0, (0, 5)), "d64": (64, 27, 5, 4, 1, 1, (3,)), "d128": (128, 27, 5, 4, 0, 1, (25,)),
    "d256": (256, 27, 5, 4, 1, 0, ()), "d256_mult": (256, 27, 5, 4, 0, 1, (1,)), "f17": (64, 17, 5, 4, 0, 1, (0,)),
    "f32": (64, 32, 5, 4, 1, 1, ()), "f32_plain_last": (64, 32, 5, 4, 0, 0, (30,)), "b1": (32, 27, 1, 2, 0, 1, (2,)),
    "stride": (32, 27, 4 * 256 + 3, 4, 1, 0, (7,)), "c2": (64, 27, 5, 2, 1, 0, ()), "c16": (128, 27, 5, 16, 0, 0, (4,)),
}


def bits(t):
    return t.view(torch.int32)


@pytest.mark.gpu
@pytest.mark.parametrize("cid", sorted(CASES))
def test_kernels_equal_the_two_operators_and_float64(ops, cid):
    D, F, B, c, op, itself, plain = CASES[cid]
    T, n = F - 1, B
    rng = np.random.default_rng(sum(map(ord, cid)))
    ctx, w, base, weight = make_ctx(ops, T, D)
    assert ops.qr_interact_supported(ctx)
    if cid == "stride":
        for o in (0, 1):
            assert 4 * ops.qr_interact_grid(o, B, D)[0] < B, "some wave walks a second sample"
    coll = np.array([0 if t in plain else c for t in range(T)], dtype=np.int32)
    qr_t = np.flatnonzero(coll)
    slots = (rng.integers(0, 60, size=(T, n)) * 13 % (SETS * WAYS + AUX - 1)).astype(np.int32)      # repeats; some >= SETS * WAYS
    rem = rng.integers(0, c, size=(T, n)).astype(np.uint8)
    rem[qr_t[0], 0], rem[qr_t[1], 0] = 0, c - 1
    assert (slots >= SETS * WAYS).any() and {0, c - 1} <= set(rem[qr_t].ravel().tolist())
    Wr32 = (1.0 + 0.5 * rng.standard_normal((T, c, D))).astype(np.float32)
    Wr32[coll == 0] = NAN                   # a plain table never uses a Wr value
    x32 = rng.standard_normal((B, D), dtype=np.float32)
    npairs = F * (F + 1) // 2 if itself else F * (F - 1) // 2
    width, w4 = D + npairs, pad4(D + npairs)
    ld_R = w4 + 4
    dR32 = rng.standard_normal((B, width), dtype=np.float32)
    # ---- float64, composed from the fp32 operands ----
    P, Pa = np.zeros((B, F, D)), np.zeros((B, F, D))
    P[:, 0], Pa[:, 0] = x32, np.abs(x32)
    for t in range(T):
        q = w[base[t] + slots[t]].astype(np.float64)
        if coll[t]:
            y = Wr32[t, rem[t]].astype(np.float64)
            P[:, t + 1], Pa[:, t + 1] = (q * y, np.abs(q) * np.abs(y)) if op == 0 else (q + y, np.abs(q) + np.abs(y))
        else:
            P[:, t + 1], Pa[:, t + 1] = q, np.abs(q)
    # ---- device operands ----
    slots_d, coll_d, Wr_d = torch.from_numpy(slots).to(DEV), torch.from_numpy(coll).to(DEV), torch.from_numpy(Wr32).to(DEV)
    r_buf = torch.full((T, n + 3), 255, dtype=torch.uint8, device=DEV)
    r_d = r_buf[:, :n]
    r_d.copy_(torch.from_numpy(rem))
    x, _ = _dev_operand(B, D, D + 4, 0, torch.from_numpy(x32), NAN)
    feat = torch.zeros(B + 1, F, D, device=DEV)[:B]
    feat[:, 0, :] = x
    Rf, Rf_buf = _dev_operand(B, w4, ld_R, 0, None, SENTINEL)
    R2, R2_buf = _dev_operand(B, w4, ld_R, 0, None, SENTINEL)
    ops.qr_interact_fwd(ctx, slots_d, r_d, Wr_d, coll_d, op, x, bool(itself), Rf)
    ops.qr_cached_fwd(ctx, slots_d, r_d, Wr_d, coll_d, op, feat[:, 1:, :], feat.stride(0), D)
    ops.interact_fwd(feat, bool(itself), R2)
    torch.cuda.synchronize()
    assert torch.equal(bits(Rf_buf), bits(R2_buf)), cid + ": forward differs from qr_cached_fwd + interact_fwd"
    assert _gap_ok(Rf, ld_R, w4, SENTINEL)
    got = Rf.cpu().numpy()
    assert np.array_equal(got[:, :D].view(np.uint32), x32.view(np.uint32)) and (got[:, width:] == 0).all()
    for x_act in (0, 1, 2):
        what = "%s x_act=%d" % (cid, x_act)
        pairs, pmag, dP, dmag = ref64(P, Pa, dR32.astype(np.float64), D, F, itself, x_act)
        if x_act == 0:
            assert_within(got[:, D:width], pairs, pmag, D + 2, cid + " pairs", act_ulps=0)
        dRv, _ = _dev_operand(B, width, ld_R, 0, torch.from_numpy(dR32), NAN)
        dfeat = torch.zeros(B + 1, F, D, device=DEV)
        dfeat[:B] = SENTINEL
        dfeat2 = torch.zeros(B + 1, F, D, device=DEV)
        ops.qr_interact_bwd(ctx, slots_d, r_d, Wr_d, coll_d, op, x, dRv, bool(itself), dfeat[:B], x_act=x_act)
        ops.interact_bwd(feat, dRv, bool(itself), dfeat2[:B], x_act=x_act)
        torch.cuda.synchronize()
        assert torch.equal(bits(dfeat), bits(dfeat2)), what + ": backward differs from interact_bwd (row B: 0)"
        assert_within(dfeat[:B].cpu().numpy().reshape(B * F, D), dP.reshape(B * F, D), dmag.reshape(B * F, D), F + 3, what + " dfeat")
    assert torch.equal(weight.cpu(), torch.from_numpy(w)), cid + ": cache rows were written"
    assert np.array_equal(Wr_d.cpu().numpy().view(np.uint32), Wr32.view(np.uint32)) and bool((r_buf[:, n:] == 255).all())
    ctx.check()


@pytest.mark.gpu
@pytest.mark.parametrize("what,D,T,n_extra,c,r_off,ld_r_short,names", [
    ("d48", 48, 26, 0, 4, 0, 0, "unsupported D"), ("t15", 32, 15, 0, 4, 0, 0, "unsupported T"), ("t32", 32, 32, 0, 4, 0, 0, "unsupported T"),
    ("n", 32, 17, 1, 4, 0, 0, "n == B"), ("c1", 32, 17, 0, 1, 0, 0, "collisions c"), ("c17", 32, 17, 0, 17, 0, 0, "collisions c"),
    ("R", 32, 17, 0, 4, 1, 0, "R / dR"), ("ld_r", 32, 17, 0, 4, 0, 1, "ld_r")])
def test_refusals_name_the_argument_and_launch_nothing(ops, what, D, T, n_extra, c, r_off, ld_r_short, names):
    from cdlrm_amd import _lib
    B, F = 8, T + 1
    ctx = make_ctx(ops, T, D)[0]
    assert ops.qr_interact_supported(ctx) == (T == 17)
    slots = torch.zeros(T, 16, dtype=torch.int32, device=DEV)
    r = torch.zeros(T, 16, dtype=torch.uint8, device=DEV)
    Wr = torch.ones(T, 17, D, device=DEV)
    coll = torch.full((T,), 4, dtype=torch.int32, device=DEV)
    x = torch.ones(B, D, device=DEV)
    ld_R = pad4(D + F * (F - 1) // 2)
    Rb = torch.full((B * ld_R + 4,), SENTINEL, device=DEV)
    dfeat = torch.full((B, F, D), SENTINEL, device=DEV)
    n = B + n_extra
    head = (ctx.handle, slots.data_ptr(), n, r.data_ptr(), n - ld_r_short, Wr.data_ptr(), coll.data_ptr(), c, 0, x.data_ptr(), D)
    Rp = Rb.data_ptr() + 4 * r_off
    L = _lib.lib()
    for rc in (L.cdlrm_qr_interact_fwd(*head, B, 0, Rp, ld_R, None),
               L.cdlrm_qr_interact_bwd(*head, Rp, ld_R, B, 0, 0, dfeat.data_ptr(), None)):
        assert rc != 0 and names in _lib.raw().cdlrm_last_error().decode(), (rc, _lib.raw().cdlrm_last_error())
    torch.cuda.synchronize()
    assert bool((Rb == SENTINEL).all()) and bool((dfeat == SENTINEL).all())


def _engine_run(op, fuse, native):
    """Six steps over two windows of three and a test batch: 14 QR tables (rows_q ~ 760 > 64 sets x 4 ways: misses, evictions) and
    3 plain ones of 150 rows, c = 4, D = 64."""
    from cdlrm_amd.engine import TrainEngine, WindowPipeline
    from cdlrm_amd.model_no_ddp import DLRM_Net, Embedding_Table_Cache_Group, Embedding_Table_Group
    T, D, B, L, seed = 17, 64, 64, 3, 47
    ln_emb = np.array([150 if k % 6 == 2 else 3000 + 11 * k for k in range(T)])
    ln_bot, ln_top = np.array([13, 48, D]), np.array([D + (T + 1) * T // 2, 40, 1])
    rng = np.random.RandomState(seed)
    batches = [(torch.from_numpy(rng.rand(B, 13).astype(np.float32)),
                torch.from_numpy(np.stack([rng.zipf(1.3, size=B).astype(np.int64) * 2654435761 % ln_emb[k] for k in range(T)])),
                torch.from_numpy(np.round(rng.rand(B, 1)).astype(np.float32))) for _ in range(7)]
    np.random.seed(seed)
    torch.manual_seed(seed)
    host = Embedding_Table_Group(D, ln_emb, qr_flag=True, qr_operation=op, qr_collisions=4, qr_threshold=200).pin()
    cg = Embedding_Table_Cache_Group(D, ln_emb, 64, 512, 4, qr_layout=host.qr_layout()).to(DEV)
    dl = DLRM_Net(ln_bot, ln_top, "dot", False, True, -1, ln_top.size - 2, 0.0).to(DEV)
    eng = TrainEngine(cg, dl, host, lr=0.1, lr_embeds=0.3)
    eng.fuse_qr, eng.native_tape = fuse, native
    pipe = WindowPipeline(cg, host, L * B, parity_rng=True)
    losses = []
    for j, (X, idx, Y) in enumerate(batches[:6]):
        if j % L == 0:
            win = torch.cat([b[1] for b in batches[j:j + L]], dim=1).to(DEV)
            _, rwin = eng.qr_split(win, q=win)
            torch.manual_seed(500 + j)
            pipe.plan_window(win)
            pipe.commit()
            pipe.wait_writeback()
        cols = slice((j % L) * B, (j % L + 1) * B)
        losses.append(eng.step(X.to(DEV), win[:, cols], Y.to(DEV), j=j, r=rwin[:, cols])[0:1].clone())
    eng.finish()
    qe, re_ = eng.qr_split(batches[6][1].to(DEV))
    Z = eng.evaluate(batches[6][0].to(DEV), qe, r=re_).clone()
    torch.cuda.synchronize()
    cg.ctx.check()
    assert eng.tape_fallbacks == [] and eng._tapes and all((t["native"] is not None) == native for t in eng._tapes.values())
    cg.flush_to_host(host)
    state = [torch.cat(losses), Z, eng.param_flat.clone(), eng.Wr.clone(), cg.weight.data.clone(), cg.tags.clone()] + \
            [(E.weight_q if hasattr(E, "weight_q") else E.weight).data.clone() for E in host.emb_l]
    return state, [fn.__name__ for t in eng._tapes.values() for fn, _, is_lib in t["prog"] if is_lib]


@pytest.mark.gpu
@pytest.mark.parametrize("op", ["mult", "add"])
def test_engine_with_fused_qr_equals_the_two_operators(ops, op):
    want, names0 = _engine_run(op, False, True)
    got, names1 = _engine_run(op, True, True)
    py, names2 = _engine_run(op, True, False)
    assert {"cdlrm_qr_cached_fwd", "cdlrm_interact_fwd", "cdlrm_interact_bwd", "cdlrm_qr_cached_bwd", "cdlrm_qr_cached_bwd_finish"} <= set(names0)
    assert not any("qr_interact" in n for n in names0)
    assert {"cdlrm_qr_interact_fwd", "cdlrm_qr_interact_bwd", "cdlrm_qr_cached_bwd", "cdlrm_qr_cached_bwd_finish"} <= set(names1)
    assert not {"cdlrm_qr_cached_fwd", "cdlrm_interact_fwd", "cdlrm_interact_bwd"} & set(names1) and names1 == names2
    # the fused run's launches are the unfused run's with the three operators replaced, name for name
    swap = {"cdlrm_interact_fwd": "cdlrm_qr_interact_fwd", "cdlrm_interact_bwd": "cdlrm_qr_interact_bwd"}
    assert [swap.get(n, n) for n in names0 if n != "cdlrm_qr_cached_fwd"] == names1
    for k, (a, b, c) in enumerate(zip(want, got, py)):
        f = (lambda t: t.view(torch.int32) if t.dtype == torch.float32 else t)
        assert a.dtype == b.dtype and torch.equal(f(a), f(b)), "state %d: fused differs from the two operators" % k
        assert torch.equal(f(b), f(c)), "state %d: native tape replay differs from Python issue" % k
