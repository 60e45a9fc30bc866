"""The pairwise-dot interaction at 33 to 64 features (csrc/interact_wide.hip) against float64, and a training run on it.

Kernel cases: each (F, D) below with itself 0 / 1, x_act 0 / 1 / 2 in the backward and B in 1, 3, 5 -- and, for the first and the
last pipelined case, B = 4 * grid + 3 so that some wave carries its register ring across a sample boundary.  Every element is
compared, with the float64 reference and the derived bounds of tests/test_interact_routes.py (imported, not restated):
R[:, :D] bit for bit, pairs within C * D * 2^-24 * sum |T_ik| |T_jk|, dfeat within C * (F + 2) * 2^-24 * mag * |act'| + 8 * 2^-24 * |ref|
and exactly 0 where the ReLU mask is 0.  dR holds NaN behind the pairs; R and dfeat hold a sentinel wherever no output belongs.
"""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import test_interact_routes as IR      # noqa: E402
from test_interact_routes import SENTINEL, NAN, DEV, npairs_of, pad4, _dev_operand, _gap_ok      # noqa: E402

ops = IR.ops        # the fixture: builds the library where it is missing

# (F, D, family, pad of the pitch ("p4": rounded up to 4), element offset of R / dR, batch sizes past the grid)
CASES = [
    (33, 32, "wide_slab", "p4", 0, True),        # one row in the second block; one slab
    (33, 128, "wide_slab", "p4", 0, False),      # ... several slabs
    (48, 64, "wide_slab", "p4", 0, False),       # either side of a 16-row tile edge; first multi-slab width
    (49, 64, "wide_slab", "p4", 0, False),
    (64, 32, "wide_slab", "p4", 0, False),       # full Gram matrix; one slab
    (64, 256, "wide_slab", "p4", 0, True),       # full Gram matrix; most slabs, the register-tightest instance
    (33, 4, "wide_row", "p4", 0, False),         # whole-row family
    (64, 48, "wide_row", "p4", 0, False),
    (40, 128, "wide_row", 1, 1, False),          # forced onto it: ld_r = width + 1, R / dR offset by one element
]


def _past_the_grid(ops, F, D, past):
    """{op: 4 * grid + 3} with the grid a large batch gets: some wave of `op` walks a second sample there."""
    if not past:
        return {}
    return {op: 4 * ops.interact_wide_route(op, 1 << 20, F, D, False, pad4(D + npairs_of(F, 0)))["grid"] + 3 for op in ("fwd", "bwd")}


@pytest.mark.gpu
@pytest.mark.parametrize("F,D,fam,pad,off,past", CASES, ids=lambda v: str(v))
def test_wide_kernels_vs_float64(ops, F, D, fam, pad, off, past):
    pastB = _past_the_grid(ops, F, D, past)
    for itself in (0, 1):
        width = D + npairs_of(F, itself)
        ld = pad4(width) if pad == "p4" else width + pad
        for B in [1, 3, 5] + sorted(set(pastB.values())):
            what = "F=%d D=%d itself=%d B=%d" % (F, D, itself, B)
            rng = np.random.default_rng(IR.seed_of("wide", F, D, itself, B))
            T32 = IR.draw_block(rng, B, F, D)
            fd = torch.from_numpy(T32).to(DEV)
            # ---- forward ----
            Rv, Rbuf = _dev_operand(B, width, ld, off, None, SENTINEL)
            r = ops.interact_wide_route("fwd", B, F, D, bool(itself), ld, Rv.data_ptr() % 16 == 0)
            assert r["family"] == fam and r["lds_bytes"] <= 160 * 1024, (what, r)
            if B <= 5 or B == pastB.get("fwd"):     # a wave per sample, or some wave walks a second sample
                assert (r["grid"] == -(-B // 4)) == (B <= 5), (what, r)
            ops.interact_fwd(fd, bool(itself), Rv)
            torch.cuda.synchronize()
            buf = Rbuf.cpu().numpy()
            rows = buf[off:off + B * ld].reshape(B, ld)
            assert (buf[:off] == SENTINEL).all() and (buf[off + B * ld:] == SENTINEL).all(), what + ": written outside R"
            padw = rows[:, width:min(pad4(width), ld)]
            assert (padw == 0).all() if fam == "wide_slab" else ((padw == 0) | (padw == SENTINEL)).all(), what + ": pad word"
            assert (rows[:, pad4(width):] == SENTINEL).all(), what + ": R written behind pad4(width)"
            IR.check_fwd(rows, T32, itself, what, fam)
            # ---- backward ----
            dR32 = rng.standard_normal((B, width), dtype=np.float32)
            dR_src = torch.from_numpy(dR32).to(DEV)
            for x_act in (0, 1, 2):
                T32[:, 0] = IR.draw_row0(rng, B, D, x_act)
                fd = torch.from_numpy(T32).to(DEV)
                dRv, _ = _dev_operand(B, width, ld, off, dR_src, NAN)          # NaN in every column >= D + npairs
                dfbuf = torch.full((B * F * D + 4,), SENTINEL, dtype=torch.float32, device=DEV)
                dfeat = dfbuf[:B * F * D].view(B, F, D)
                r = ops.interact_wide_route("bwd", B, F, D, bool(itself), ld, dRv.data_ptr() % 16 == 0, True)
                assert r["family"] == fam and (B != pastB.get("bwd") or r["grid"] < -(-B // 4)), (what, r)
                ops.interact_bwd(fd, dRv, bool(itself), dfeat, x_act=x_act)
                torch.cuda.synchronize()
                assert _gap_ok(dRv, ld, width, NAN) and torch.equal(dRv, dR_src), what + ": dR was written"
                got = dfbuf.cpu().numpy()
                assert (got[B * F * D:] == SENTINEL).all(), what + ": written past row B of dfeat"
                IR.check_bwd(got[:B * F * D].reshape(B, F, D), T32, dR32, itself, x_act, "%s x_act=%d" % (what, x_act), fam)


@pytest.mark.gpu
def test_wide_refusals(ops):
    """F = 32 and F = 65, D = 130 and D = 512 (past the LDS budget) are refused by the wide calls and by their route query alike;
    the narrow route query still refuses F = 33."""
    from cdlrm_amd import _lib
    for F, D, msg in ((32, 32, "32<F<=64"), (65, 32, "32<F<=64"), (40, 130, "32<F<=64"), (40, 512, "LDS budget")):
        ld = pad4(D + npairs_of(F, 0))
        feat = torch.zeros(1, F, D, device=DEV)
        Rm = torch.full((1, ld), SENTINEL, device=DEV)
        df = torch.full((1, F, D), SENTINEL, device=DEV)
        L = _lib.lib()
        for call in (lambda: _lib.check(L.cdlrm_interact_wide_fwd(feat.data_ptr(), 1, F, D, 0, Rm.data_ptr(), ld, None)),
                     lambda: _lib.check(L.cdlrm_interact_wide_bwd(feat.data_ptr(), Rm.data_ptr(), ld, 1, F, D, 0, 0, df.data_ptr(), None)),
                     lambda: ops.interact_wide_route("fwd", 1, F, D, False, ld),
                     lambda: ops.interact_wide_route("bwd", 1, F, D, False, ld)):
            with pytest.raises(_lib.CdlrmError, match=msg):
                call()
        torch.cuda.synchronize()
        assert bool((Rm == SENTINEL).all()) and bool((df == SENTINEL).all())
    with pytest.raises(_lib.CdlrmError, match=r"F<=32, D%4==0"):
        ops.interact_route("fwd", 1, 33, 32, False, 1000)
    with pytest.raises(_lib.CdlrmError, match="ld_r"):
        ops.interact_wide_route("fwd", 1, 40, 32, False, 32 + npairs_of(40, 0) - 1)


def _train(T, m_spa, batches, L, B, ways, cache_size, seed, ln_emb, ln_bot, ln_top, native):
    from cdlrm_amd.engine import TrainEngine, WindowPipeline, WindowResolver
    from cdlrm_amd.model_no_ddp import DLRM_Net, Embedding_Table_Cache_Group, Embedding_Table_Group
    np.random.seed(seed)
    torch.manual_seed(seed)
    host = Embedding_Table_Group(m_spa, np.array(ln_emb)).pin()
    np.random.seed(seed)
    torch.manual_seed(seed)
    cg = Embedding_Table_Cache_Group(m_spa, np.array(ln_emb), cache_size, B, ways).to(DEV)
    dl = DLRM_Net(ln_bot, ln_top, "dot", False, True, -1, ln_top.size - 2, 0.0).to(DEV)
    eng = TrainEngine(cg, dl, host, lr=0.05, lr_embeds=0.2)
    eng.native_tape = native
    assert not eng._fused_gather(None), "the fused gather kernels stop at 32 features"
    pipe = WindowPipeline(cg, host, L * B, parity_rng=True)
    dev_idx = [b[1].to(DEV) for b in batches]
    losses = []
    for j, (X, idx, Tt) in enumerate(batches):
        jl = j % L
        if jl == 0:
            torch.manual_seed(700 + j)
            win = torch.cat([b[1] for b in batches[j:j + L]], dim=1).to(DEV)
            pipe.plan_window(win)
            pipe.commit()
            pipe.wait_writeback()
            rs = WindowResolver(eng, win, B, chunk=2)
        nxt = dev_idx[j + 1] if jl + 1 < L else None
        loss = eng.step(X.to(DEV), dev_idx[j], Tt.to(DEV), j=j, next_idx=nxt, res=rs.batch(jl),
                        next_res=rs.batch(jl + 1) if nxt is not None else None)
        rs.ensure(jl + rs.CH + 2)
        losses.append(loss[0:1].clone())
    eng.finish()
    cg.ctx.check()
    names = [p[0].__name__ for t in eng._tapes.values() for p in t["prog"] if p[2]]
    assert eng._tapes and not eng.tape_fallbacks
    assert (sum(t["native"] is not None for t in eng._tapes.values()) > 0) == native
    return torch.cat(losses).cpu().numpy(), [t.cpu() for t in cg.occupancy_tables], cg.weight.data.cpu().clone(), names


@pytest.mark.gpu
@pytest.mark.parametrize("T,m_spa", [(32, 32), (63, 64)])
def test_engine_with_33_and_64_features_vs_oracle(ops, T, m_spa):
    """TrainEngine at 32 and 63 tables (tiny tables: misses and evictions in every window), six steps across a window boundary:
    loss per iteration against the oracle trainer at rtol 1e-5, tags bit-exact; the natively taped run equals the Python-issued
    one bit for bit, and the step's interaction calls are the wide ones."""
    from oracle import cdlrm_oracle as O
    sizes = [2000, 30, 5, 900, 20000, 64, 311, 7]
    ln_emb = [sizes[k % len(sizes)] + k for k in range(T)]
    B, L, ways, cache_size, seed = 48, 3, 4, 24, 31
    ln_bot = np.array([13, 32, m_spa])
    nf = T + 1
    ln_top = np.array([m_spa + nf * (nf - 1) // 2, 32, 1])
    rng = np.random.RandomState(T)
    batches = []
    for j in range(6):
        X = torch.from_numpy(rng.rand(B, 13).astype(np.float32))
        idx = torch.stack([torch.from_numpy((rng.zipf(1.2, size=B).astype(np.int64) * 2654435761 % n)) for n in ln_emb])
        batches.append((X, idx, torch.from_numpy(np.round(rng.rand(B, 1)).astype(np.float32))))
    torch.set_num_threads(1)
    otr = O.OracleTrainer(ln_emb, m_spa, ln_bot, ln_top, cache_size=cache_size, num_ways=ways, mini_batch_size=B,
                          lr=0.05, lr_embeds=0.2, lookahead=L, table_agg_freq=10 ** 9, seed=seed)
    lS_o = torch.arange(B).repeat(T, 1)
    for j, (X, idx, Tt) in enumerate(batches):
        if j % L == 0:
            torch.manual_seed(700 + j)
            otr.refill(torch.cat([b[1] for b in batches[j:j + L]], dim=1))
        otr.step(j, X, lS_o, idx, Tt)
    args = (T, m_spa, batches, L, B, ways, cache_size, seed, ln_emb, ln_bot, ln_top)
    py, native = _train(*args, native=False), _train(*args, native=True)
    np.testing.assert_allclose(py[0], np.array([l[0] for l in otr.losses]), rtol=1e-5)
    for k in range(T):
        assert torch.equal(py[1][k], otr.occ[k]), "tag state differs for table %d" % k
    assert np.array_equal(py[0], native[0]) and torch.equal(py[2], native[2]), "the native tape's run differs"
    for names in (py[3], native[3]):
        assert "cdlrm_interact_wide_fwd" in names and "cdlrm_interact_wide_bwd" in names
        assert not [n for n in names if "interact" in n and "wide" not in n], names
