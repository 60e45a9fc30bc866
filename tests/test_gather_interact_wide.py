"""The fused gather at 33 to 64 features (cdlrm_gather_interact_wide_fwd / _bwd, csrc/interact_wide.hip): bit for bit against
embbag_fwd + interact_fwd / interact_bwd on the same slots, every element against float64 on the gathered block with the
comparators and bounds of tests/test_interact_routes.py (imported, not restated), the refusals, and a TrainEngine with
fuse_gather_wide against the same run on two operators.
"""
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import test_interact_routes as IR      # noqa: E402
from test_interact_routes import SENTINEL, NAN, DEV, npairs_of, pad4, _dev_operand, _gap_ok      # noqa: E402
from test_bag_interact import make_ctx, SETS, WAYS, AUX      # noqa: E402

ops = IR.ops        # the fixture: builds the library where it is missing
NAMES = ["cdlrm_gather_interact_wide_" + s for s in ("supported", "fwd", "bwd", "grid")]

# (F, D, also B = 4 * grid + 3: a wave carries its ring and its slot table across a sample boundary)
CASES = [(33, 32, True),        # one row in the second block; one slab, a ring one slab deep
         (33, 128, False),
         (49, 64, False),       # a 16-row tile edge; as many slabs as the ring is deep
         (64, 32, False),
         (64, 256, True)]       # full Gram matrix; the register-tightest instance


@pytest.mark.gpu
@pytest.mark.parametrize("F,D,past", CASES, ids=lambda v: str(v))
def test_wide_gather_kernels_vs_two_operators_and_float64(ops, F, D, past):
    T = F - 1
    ctx, w, base, _ = make_ctx(ops, T, D)
    assert ops.gather_interact_wide_supported(ctx) and not ops.gather_interact_supported(ctx)
    # past the larger of the two grids: some wave of either kernel walks a second sample there
    pastB = [4 * max(ops.gather_interact_wide_grid(ctx, op, 1 << 20)[0] for op in ("fwd", "bwd")) + 3] if past else []
    for itself in (0, 1):
        width = D + npairs_of(F, itself)
        ld = pad4(width)
        for B in [1, 3, 5] + pastB:
            what = "F=%d D=%d itself=%d B=%d" % (F, D, itself, B)
            for op in ("fwd", "bwd"):
                assert (ops.gather_interact_wide_grid(ctx, op, B)[0] < -(-B // 4)) == (B > 5), what
            rng = np.random.default_rng(IR.seed_of("gather_wide", F, D, itself, B))
            n = B + 28
            sl = (rng.integers(0, 60, size=(T, n)) * 13 % (SETS * WAYS + AUX - 1)).astype(np.int32)    # repeats; some auxiliary rows
            slots = torch.from_numpy(sl).to(DEV)
            T32 = np.empty((B, F, D), dtype=np.float32)
            T32[:, 1:] = w[base[:, None] + sl[:, :B]].transpose(1, 0, 2)
            dR32 = rng.standard_normal((B, width), dtype=np.float32)
            dR_src = torch.from_numpy(dR32).to(DEV)
            for x_act in (0, 1, 2):
                T32[:, 0] = IR.draw_row0(rng, B, D, x_act)
                xbuf = torch.full((B, D + 8), NAN, device=DEV)
                x = xbuf[:, 4:4 + D]
                x.copy_(torch.from_numpy(T32[:, 0]))
                feat = torch.full((B, F, D), NAN, device=DEV)
                feat[:, 0] = x
                ops.embbag_fwd(ctx, slots[:, :B].contiguous(), None, feat[:, 1:, :], F * D, D)
                if x_act == 0:      # ---- forward ----
                    Rv, Rbuf = _dev_operand(B, width, ld + 4, 0, None, SENTINEL)
                    R2 = torch.full((B, ld + 4), SENTINEL, device=DEV)
                    ops.gather_interact_wide_fwd(ctx, slots, x, bool(itself), Rv)
                    ops.interact_fwd(feat, bool(itself), R2)
                    rows = Rbuf.cpu().numpy()[:B * (ld + 4)].reshape(B, ld + 4)
                    assert (Rbuf[B * (ld + 4):] == SENTINEL).all(), what + ": written past row B of R"
                    assert torch.equal(Rv, R2[:, :width]), what + ": differs from embbag_fwd + interact_fwd"
                    assert (rows[:, width:ld] == 0).all() and (rows[:, ld:] == SENTINEL).all(), what + ": pad words / behind pad4(width)"
                    IR.check_fwd(rows, T32, itself, what, "wide_slab")
                # ---- backward ----
                dRv, _ = _dev_operand(B, width, ld, 0, dR_src, NAN)           # NaN in every column >= D + npairs
                dfbuf = torch.full((B * F * D + 4,), SENTINEL, dtype=torch.float32, device=DEV)
                dfeat, df2 = dfbuf[:B * F * D].view(B, F, D), torch.empty(B, F, D, device=DEV)
                ops.gather_interact_wide_bwd(ctx, slots, x, dRv, bool(itself), dfeat, x_act=x_act)
                ops.interact_bwd(feat, dRv, bool(itself), df2, x_act=x_act)
                assert _gap_ok(dRv, ld, width, NAN) and torch.equal(dRv, dR_src), what + ": dR was written"
                got = dfbuf.cpu().numpy()
                assert (got[B * F * D:] == SENTINEL).all(), what + ": written past row B of dfeat"
                assert torch.equal(dfeat, df2), "%s x_act=%d: differs from interact_bwd on the gathered block" % (what, x_act)
                IR.check_bwd(got[:B * F * D].reshape(B, F, D), T32, dR32, itself, x_act, "%s x_act=%d" % (what, x_act), "wide_slab")


@pytest.mark.gpu
def test_wide_gather_refusals(ops):
    """T + 1 = 32 and 65 and D = 48 have no kernel (supported is 0); an unaligned R and a pitch that is no multiple of 4 are
    refused on a supported context.  Every refusal has a message and leaves the outputs alone."""
    from cdlrm_amd import _lib
    for T, D, off, dld, msg in ((31, 32, 0, 0, "unsupported shape"), (64, 32, 0, 0, "unsupported shape"), (40, 48, 0, 0, "unsupported shape"),
                                (40, 32, 1, 0, "ld_r"), (40, 32, 0, 2, "ld_r")):
        ctx, _, _, _ = make_ctx(ops, T, D)
        assert ops.gather_interact_wide_supported(ctx) == (msg == "ld_r")
        ld = pad4(D + npairs_of(T + 1, 0)) + dld
        buf = torch.full((3 * ld + 4,), SENTINEL, device=DEV)
        Rm = buf[off:off + 3 * ld].view(3, ld)
        df = torch.full((3, T + 1, D), SENTINEL, device=DEV)
        slots, x = torch.zeros(T, 3, dtype=torch.int32, device=DEV), torch.zeros(3, D, device=DEV)
        for call in (lambda: ops.gather_interact_wide_fwd(ctx, slots, x, False, Rm),
                     lambda: ops.gather_interact_wide_bwd(ctx, slots, x, Rm, False, df)):
            with pytest.raises(_lib.CdlrmError, match=msg):
                call()
        if msg != "ld_r":
            with pytest.raises(_lib.CdlrmError, match=msg):
                ops.gather_interact_wide_grid(ctx, "fwd", 3)
        torch.cuda.synchronize()
        assert bool((buf == SENTINEL).all()) and bool((df == SENTINEL).all())


def _train(T, m_spa, fuse, native):
    """Six steps across a window boundary, the batches and geometry of test_engine_with_33_and_64_features_vs_oracle."""
    from cdlrm_amd.engine import TrainEngine, WindowPipeline, WindowResolver
    from cdlrm_amd.model_no_ddp import DLRM_Net, Embedding_Table_Cache_Group, Embedding_Table_Group
    sizes = [2000, 30, 5, 900, 20000, 64, 311, 7]
    ln_emb = [sizes[k % len(sizes)] + k for k in range(T)]
    B, L, ways, cache_size, seed = 48, 3, 4, 24, 31
    ln_bot, ln_top = np.array([13, 32, m_spa]), np.array([m_spa + (T + 1) * T // 2, 32, 1])
    rng = np.random.RandomState(T)
    batches = []
    for j in range(6):
        X = torch.from_numpy(rng.rand(B, 13).astype(np.float32))
        idx = torch.stack([torch.from_numpy((rng.zipf(1.2, size=B).astype(np.int64) * 2654435761 % n)) for n in ln_emb])
        batches.append((X, idx, torch.from_numpy(np.round(rng.rand(B, 1)).astype(np.float32))))
    np.random.seed(seed)
    torch.manual_seed(seed)
    host = Embedding_Table_Group(m_spa, np.array(ln_emb)).pin()
    np.random.seed(seed)
    torch.manual_seed(seed)
    cg = Embedding_Table_Cache_Group(m_spa, np.array(ln_emb), cache_size, B, ways).to(DEV)
    dl = DLRM_Net(ln_bot, ln_top, "dot", False, True, -1, ln_top.size - 2, 0.0).to(DEV)
    eng = TrainEngine(cg, dl, host, lr=0.05, lr_embeds=0.2)
    eng.native_tape, eng.fuse_gather_wide = native, fuse
    assert eng._fused_gather(None) == fuse
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
    assert eng._tapes and not eng.tape_fallbacks
    assert (sum(t["native"] is not None for t in eng._tapes.values()) > 0) == native
    names = [p[0].__name__ for t in eng._tapes.values() for p in t["prog"] if p[2]]
    return torch.cat(losses).cpu(), torch.cat([t.cpu().reshape(-1) for t in cg.occupancy_tables]), cg.weight.data.cpu().clone(), names


@pytest.mark.gpu
@pytest.mark.parametrize("T,m_spa", [(32, 32), (63, 64)])
def test_engine_with_fuse_gather_wide_equals_two_operators(ops, T, m_spa):
    two, py, native = _train(T, m_spa, False, False), _train(T, m_spa, True, False), _train(T, m_spa, True, True)
    for run in (py, native):
        assert all(torch.equal(a, b) for a, b in zip(two[:3], run[:3])), "losses, tags or cache rows differ from the two-operator run"
        assert "cdlrm_gather_interact_wide_fwd" in run[3] and "cdlrm_gather_interact_wide_bwd" in run[3]
        assert not [n for n in run[3] if "cdlrm_interact_wide" in n or n == "cdlrm_gather_interact_bwd_sgd"], run[3]
    assert "cdlrm_interact_wide_fwd" in two[3] and "cdlrm_embbag_fwd" in two[3]


def test_abi_and_cli_hold_the_wide_gather(ops):
    from cdlrm_amd import _lib
    from cdlrm_amd.main_no_ddp import ProcessArgs
    hdr = open(os.path.join(ROOT, "include", "cdlrm_hip.h")).read()
    tape = open(os.path.join(ROOT, "cdlrm_amd", "csrc", "tape.hip")).read()
    for name in NAMES:
        assert re.search(r"\bint %s\(" % name, hdr) and name in _lib.PROTOTYPES and hasattr(_lib.raw(), name), name
        assert ("TAPE_FN(%s)" % name in tape) == name.endswith(("_fwd", "_bwd")), name
    assert _lib.PROTOTYPES[NAMES[1]] == _lib.PROTOTYPES["cdlrm_gather_interact_fwd"]
    assert _lib.PROTOTYPES[NAMES[2]] == _lib.PROTOTYPES["cdlrm_gather_interact_bwd"]
    assert ProcessArgs(["--fuse-gather-wide"]).fuse_gather_wide and not ProcessArgs([]).fuse_gather_wide
