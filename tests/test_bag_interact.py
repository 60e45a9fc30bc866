"""Multi-hot bags pooled inside the interaction kernels (csrc/bag_interact.hip): cdlrm_bag_interact_fwd / _bwd bit for bit against
embbag_fwd + interact_fwd / interact_bwd and against a plain float64 reference, their refusals, and a TrainEngine with fuse_bags.

Bounds (2^-24 = one fp32 rounding, C_BOUND of test_gemm_routes; Lmax the case's longest bag; |P|a the pool of absolute values):
  pairs   k_eff = D + 2 Lmax, mag = |P|a |P|a^T: a D-long fma chain over operands that each carry an Lmax-long chain of adds
  dfeat   k_eff = F + 2 + Lmax, mag = |G + G^T| |P|a (+ |dR| head on row 0), row 0 times |act'|; 8 ulp for the activation factor
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

DEV = R.DEV
NAN = float("nan")
WAYS, AUX, SETS = 4, 512, 61        # 61 sets x 4 ways + 512 auxiliary rows per table, as the gather cases of test_interact_routes
UD = 4                              # ops.BAG_INTERACT_U, asserted below
PATTERNS = (0, 1, 2, UD - 1, UD, UD + 1, 37)
POISON = 1 << 40                    # in the pitch gap of the offsets

# id: D, F, B, bag lengths ("rand": 0..3; "pat": PATTERNS), squared-off layout (n_bags == B + 1), itself
CASES = {
    "d32": (32, 27, 5, "rand", False, 0), "d64": (64, 27, 5, "rand", True, 1), "d128": (128, 27, 5, "rand", False, 1),
    "d256": (256, 27, 5, "rand", True, 0), "f17": (64, 17, 5, "rand", False, 1), "f32": (64, 32, 5, "rand", True, 1),
    "lens": (128, 27, 7, "pat", False, 0), "lens_sq": (128, 27, 7, "pat", True, 1),
    "stride": (32, 27, 4 * 256 + 3, "rand", True, 0), "b1": (32, 27, 1, "rand", False, 1),
}


def pad4(w):
    return (w + 3) & ~3


def make_ctx(ops, T, D):
    ln = [40000 + 7 * k for k in range(T)]
    ctx = ops.CacheCtx(ln, [SETS] * T, D, WAYS, AUX, torch.device(DEV))
    rng = np.random.default_rng(T * 1000 + D)
    w = rng.standard_normal((ctx.total_rows, D), dtype=np.float32)
    base = np.array(ctx.row_base[:T], dtype=np.int64)
    w[base + SETS * WAYS + AUX - 1] = SENTINEL           # the last auxiliary row of every table: what padding lookups name
    weight = torch.from_numpy(w).to(DEV)
    ctx.bind_cache(torch.full((ctx.total_tags,), -1, dtype=torch.int64, device=DEV), weight)
    return ctx, w, base, weight


def make_bags(rng, T, B, kind, squared):
    """lens [T, B], offsets int64 [T, n_bags] in a pitch of n_bags + 3 (gap poisoned), slots int32 [T, n] with repeats and
    auxiliary rows.  n_bags == B: every table has n lookups (its last bag takes up the slack); B + 1: ragged tables, the padding
    lookups behind off[t, B] name the sentinel row."""
    rows = SETS * WAYS + AUX
    if kind == "pat":       # patterns mixed inside a sample and moving from sample to sample; sample 3: every bag empty
        lens = np.array([[0 if b == 3 else PATTERNS[(t + 3 * b) % 7] for b in range(B)] for t in range(T)])
    else:
        lens = rng.integers(0, 4, size=(T, B))
    n = int(lens.sum(axis=1).max()) + (5 if squared else 0)
    if not squared:
        lens[:, B - 1] += n - lens.sum(axis=1)
    n = max(n, 1)
    nb = B + 1 if squared else B
    off = np.full((T, nb + 3), POISON, dtype=np.int64)
    off[:, 0] = 0
    off[:, 1:B + 1 if squared else B] = np.cumsum(lens, axis=1)[:, :B if squared else B - 1]
    slots = rng.integers(0, 60, size=(T, n)) * 13 % (rows - 1)        # 60 distinct ids per table: repeats; some >= SETS * WAYS
    for t in range(T):
        slots[t, lens[t].sum():] = rows - 1
    return lens, off, nb, slots.astype(np.int32)


def ref64(P, Pa, dR, D, F, itself, x_act):
    """float64: R = [x | tril(P P^T)], dfeat = (G + G^T) P (+ dR head, act' on row 0), and the magnitudes of their bounds."""
    li, lj = np.tril_indices(F, 0 if itself else -1)        # pair_base's order: row i, then j
    Z, Zm = P @ P.transpose(0, 2, 1), Pa @ Pa.transpose(0, 2, 1)
    G = np.zeros((P.shape[0], F, F))
    G[:, li, lj] = dR[:, D:]
    S = G + G.transpose(0, 2, 1)
    dP, mag = S @ P, np.abs(S) @ Pa
    dP[:, 0] += dR[:, :D]
    mag[:, 0] += np.abs(dR[:, :D])
    y = P[:, 0]
    d = {0: np.ones_like(y), 1: (y > 0).astype(np.float64), 2: (1.0 - y) * y}[x_act]
    dP[:, 0] *= d
    mag[:, 0] *= np.abs(d)
    return Z[:, li, lj], Zm[:, li, lj], dP, mag


@pytest.mark.gpu
@pytest.mark.parametrize("cid", sorted(CASES))
def test_kernels_equal_the_two_operators_and_float64(ops, cid):
    assert ops.BAG_INTERACT_U == UD
    D, F, B, kind, squared, itself = CASES[cid]
    T = F - 1
    rng = np.random.default_rng(sum(map(ord, cid)))
    ctx, w, base, weight = make_ctx(ops, T, D)
    assert ops.bag_interact_supported(ctx)
    lens, off, nb, slots = make_bags(rng, T, B, kind, squared)
    if cid == "stride":
        for op in (0, 1):
            assert 4 * ops.bag_interact_grid(op, B, D)[0] < B, "some wave walks a second sample"
    if kind == "pat":
        assert set(PATTERNS) <= set(lens[:, :B - 1].ravel().tolist()) and not lens[:, 3].any()
    x32 = rng.standard_normal((B, D), dtype=np.float32)
    npairs = F * (F + 1) // 2 if itself else F * (F - 1) // 2
    width, w4 = D + npairs, pad4(D + npairs)
    ld_r = w4 + 4
    dR32 = rng.standard_normal((B, width), dtype=np.float32)
    # ---- float64: pool by loop ----
    P, Pa = np.zeros((B, F, D)), np.zeros((B, F, D))
    P[:, 0], Pa[:, 0] = x32, np.abs(x32)
    for t in range(T):
        for b in range(B):
            lo = 0 if b == 0 else int(off[t, b])
            for s in slots[t, lo:lo + lens[t, b]]:
                P[b, t + 1] += w[base[t] + s]
                Pa[b, t + 1] += np.abs(w[base[t] + s])
    Lmax = int(lens.max())
    # ---- device operands ----
    slots_d = torch.from_numpy(slots).to(DEV)
    off_d = torch.from_numpy(off).to(DEV)[:, :nb]
    x, _ = _dev_operand(B, D, D + 4, 0, torch.from_numpy(x32), NAN)
    feat = torch.zeros(B + 1, F, D, device=DEV)[:B]
    feat[:, 0, :] = x
    Rf, Rf_buf = _dev_operand(B, w4, ld_r, 0, None, SENTINEL)
    R2, R2_buf = _dev_operand(B, w4, ld_r, 0, None, SENTINEL)
    ops.bag_interact_fwd(ctx, slots_d, off_d, x, bool(itself), Rf, n_bags=nb)
    ops.embbag_fwd(ctx, slots_d, off_d, feat[:, 1:, :], feat.stride(0), D, n_bags=nb)
    ops.interact_fwd(feat, bool(itself), R2)
    torch.cuda.synchronize()
    assert torch.equal(Rf_buf.view(torch.int32), R2_buf.view(torch.int32)), cid + ": forward differs from embbag_fwd + interact_fwd"
    assert _gap_ok(Rf, ld_r, w4, SENTINEL)
    got = Rf.cpu().numpy()
    assert np.array_equal(got[:, :D].view(np.uint32), x32.view(np.uint32)) and (got[:, width:] == 0).all()
    for x_act in (0, 1, 2):
        what = "%s x_act=%d" % (cid, x_act)
        pairs, pmag, dP, dmag = ref64(P, Pa, dR32.astype(np.float64), D, F, itself, x_act)
        if x_act == 0:
            assert_within(got[:, D:width], pairs, pmag, D + 2 * Lmax, cid + " pairs", act_ulps=0)
        dRv, _ = _dev_operand(B, width, ld_r, 0, torch.from_numpy(dR32), NAN)
        dfeat = torch.zeros(B + 1, F, D, device=DEV)
        dfeat[:B] = SENTINEL
        dfeat2 = torch.zeros(B + 1, F, D, device=DEV)
        ops.bag_interact_bwd(ctx, slots_d, off_d, x, dRv, bool(itself), dfeat[:B], n_bags=nb, x_act=x_act)
        ops.interact_bwd(feat, dRv, bool(itself), dfeat2[:B], x_act=x_act)
        torch.cuda.synchronize()
        assert torch.equal(dfeat.view(torch.int32), dfeat2.view(torch.int32)), what + ": backward differs from interact_bwd (row B: 0)"
        assert_within(dfeat[:B].cpu().numpy().reshape(B * F, D), dP.reshape(B * F, D), dmag.reshape(B * F, D), F + 2 + Lmax,
                      what + " dfeat")
    assert torch.equal(weight.cpu(), torch.from_numpy(w)), cid + ": cache rows were written"
    ctx.check()


@pytest.mark.gpu
@pytest.mark.parametrize("what,D,T,ld_extra,nb_extra,names", [
    ("d48", 48, 26, 0, 0, "unsupported D"), ("t15", 32, 15, 0, 0, "unsupported T"), ("t32", 32, 32, 0, 0, "unsupported T"),
    ("ld_r", 32, 17, 1, 0, "ld_r"), ("n_bags", 32, 17, 0, 2, "n_bags")])
def test_refusals_name_the_argument_and_launch_nothing(ops, what, D, T, ld_extra, nb_extra, names):
    from cdlrm_amd import _lib
    B, F = 8, T + 1
    ctx = make_ctx(ops, T, D)[0]
    assert ops.bag_interact_supported(ctx) == (what in ("ld_r", "n_bags"))
    slots = torch.zeros(T, 16, dtype=torch.int32, device=DEV)
    off = torch.arange(B + 3, device=DEV).repeat(T, 1)
    x = torch.ones(B, D, device=DEV)
    ld_r = pad4(D + F * (F - 1) // 2) + ld_extra
    Rb = torch.full((B * ld_r + 4,), SENTINEL, device=DEV)
    dfeat = torch.full((B, F, D), SENTINEL, device=DEV)
    head = (ctx.handle, slots.data_ptr(), 16, off.data_ptr(), B + nb_extra, off.stride(0), x.data_ptr(), D)
    L = _lib.lib()
    for rc in (L.cdlrm_bag_interact_fwd(*head, B, 0, Rb.data_ptr(), ld_r, None),
               L.cdlrm_bag_interact_bwd(*head, Rb.data_ptr(), ld_r, B, 0, 0, dfeat.data_ptr(), None)):
        assert rc != 0 and names in _lib.raw().cdlrm_last_error().decode(), (rc, _lib.raw().cdlrm_last_error())
    torch.cuda.synchronize()
    assert bool((Rb == SENTINEL).all()) and bool((dfeat == SENTINEL).all())


def _engine_run(ragged, fuse):
    from cdlrm_amd import _lib
    from cdlrm_amd.engine import TrainEngine, WindowPipeline, pad_window, square_bags
    from cdlrm_amd.model_no_ddp import DLRM_Net, Embedding_Table_Cache_Group, Embedding_Table_Group
    T, D, B, L, seed = 17, 32, 64, 3, 31
    ln_emb = [3000 + 11 * k for k in range(T)]
    ln_bot, ln_top = np.array([13, 48, D]), np.array([D + (T + 1) * T // 2, 40, 1])
    rng = np.random.RandomState(seed)
    batches = []
    for j in range(7):          # 6 training steps over two windows of 3, and a test batch
        lens = rng.randint(1, 6, size=(T, B)) if ragged else np.tile(rng.randint(1, 6, size=B), (T, 1))
        offs = [torch.from_numpy(np.concatenate([[0], np.cumsum(l)[:-1]])) for l in lens]
        lists = [torch.from_numpy(rng.zipf(1.3, size=int(l.sum())).astype(np.int64) * 2654435761 % ln_emb[k]) for k, l in enumerate(lens)]
        batches.append((torch.from_numpy(rng.rand(B, 13).astype(np.float32)), offs, lists,
                        torch.from_numpy(np.round(rng.rand(B, 1)).astype(np.float32))))
    np.random.seed(seed)
    torch.manual_seed(seed)
    host = Embedding_Table_Group(D, np.array(ln_emb)).pin()
    np.random.seed(seed)
    torch.manual_seed(seed)
    cg = Embedding_Table_Cache_Group(D, np.array(ln_emb), 64, 512, 4).to(DEV)
    dl = DLRM_Net(ln_bot, ln_top, "dot", False, True, -1, ln_top.size - 2, 0.0).to(DEV)
    eng = TrainEngine(cg, dl, host, lr=0.1, lr_embeds=0.3)
    eng.fuse_bags = fuse
    pipe = WindowPipeline(cg, host, 4096, parity_rng=True)
    losses, calls = [], []

    def squared(b):
        return square_bags(b[1], b[2], DEV) if ragged else (torch.stack(b[1]).to(DEV), torch.stack(b[2]).to(DEV))

    for j, b in enumerate(batches[:6]):
        if j % L == 0:
            torch.manual_seed(500 + j)
            pipe.plan_window(pad_window([torch.cat([c[2][k] for c in batches[j:j + L]]) for k in range(T)], DEV))
            pipe.commit()
            pipe.wait_writeback()
        off, idx = squared(b)
        assert off.shape[1] == (B + 1 if ragged else B)
        _lib.start_recording(calls)
        try:
            losses.append(eng.step(b[0].to(DEV), idx, b[3].to(DEV), lS_o=off, j=j)[0:1].clone())
        finally:
            _lib.stop_recording()
    eng.finish()
    off, idx = squared(batches[6])
    Z = eng.evaluate(batches[6][0].to(DEV), idx, lS_o=off).clone()
    torch.cuda.synchronize()
    cg.ctx.check()
    assert eng.tape_fallbacks == []
    # the fused calls as a native tape: the tape registry holds both entry points (an unknown one raises TapeUnsupported)
    fused = [(fn, a, True) for fn, a in calls if "bag_interact" in fn.__name__][:2]
    if fused and _lib.native_tape_ok():
        _lib.NativeTape(fused, {})
    state = [torch.cat(losses), Z, eng.param_flat.clone()] + [e.weight.detach().clone() for e in cg.emb_l] + \
            [t.clone() for t in cg.occupancy_tables]
    return state, {fn.__name__ for fn, _ in calls}


@pytest.mark.gpu
@pytest.mark.parametrize("ragged", [True, False], ids=["ragged_square_bags", "rectangular"])
def test_engine_with_fused_bags_equals_the_two_operators(ops, ragged):
    want, names0 = _engine_run(ragged, False)
    got, names1 = _engine_run(ragged, True)
    assert "cdlrm_embbag_fwd" in names0 and not any("bag_interact" in n for n in names0)
    assert {"cdlrm_bag_interact_fwd", "cdlrm_bag_interact_bwd"} <= names1 and "cdlrm_embbag_fwd" not in names1
    for k, (a, b) in enumerate(zip(want, got)):
        assert a.dtype == b.dtype and torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, b.view(torch.int32)
                                                  if b.dtype == torch.float32 else b), "state %d differs" % k
