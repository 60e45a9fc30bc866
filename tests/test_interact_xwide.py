"""The pairwise-dot interaction at 65 to 128 features (csrc/interact_xwide.hip) against float64, and a training run on it.

Kernel cases: each (F, D) below with itself 0 / 1, x_act 0 / 1 / 2 in the backward and B in 1, 2, 3 -- and, for the first and the
last case, B = grid + 1 so that some workgroup carries its double buffer across a sample boundary.  Every element is compared,
with the float64 reference and the derived bounds of tests/test_interact_routes.py (imported, not restated): R[:, :D] bit for
bit, pairs within C * D * 2^-24 * sum |T_ik| |T_jk|, dfeat within C * (F + 2) * 2^-24 * mag * |act'| + 8 * 2^-24 * |ref| and
exactly 0 where the ReLU mask is 0.  dR holds NaN behind the pairs; R and dfeat hold a sentinel wherever no output belongs.
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import test_interact_routes as IR      # noqa: E402
import test_interact_wide as IW        # noqa: E402
from test_interact_routes import SENTINEL, NAN, DEV, npairs_of, pad4, _dev_operand, _gap_ok      # noqa: E402

ops = IR.ops        # the fixture: builds the library where it is missing

# (F, D, pad of the pitch ("p4": rounded up to 4), element offset of R / dR, a batch past the grid)
CASES = [
    (65, 32, "p4", 0, True),         # one row in the third block; one slab
    (65, 128, "p4", 0, False),       # ... several slabs
    (96, 64, "p4", 0, False),        # either side of the FP = 96 / 128 edge
    (97, 64, "p4", 0, False),
    (128, 32, "p4", 0, False),       # full matrix; one slab
    (128, 256, "p4", 0, True),       # full matrix; largest staging row; the double buffer across many slabs
    (100, 16, "p4", 0, False),       # zero-filled tail slab narrower than a slice
    (128, 4, "p4", 0, False),
    (80, 128, 1, 1, False),          # ld_r = width + 1, R / dR offset by one element: the scalar tiers
]


@pytest.mark.gpu
@pytest.mark.parametrize("F,D,pad,off,past", CASES, ids=lambda v: str(v))
def test_xwide_kernels_vs_float64(ops, F, D, pad, off, past):
    big = {op: ops.interact_xwide_route(op, 1 << 20, F, D, False, pad4(D + npairs_of(F, 0)))["grid"] + 1 for op in ("fwd", "bwd")}
    for itself in (0, 1):
        width = D + npairs_of(F, itself)
        ld = pad4(width) if pad == "p4" else width + pad
        for B in [1, 2, 3] + (sorted(set(big.values())) if past else []):
            what = "F=%d D=%d itself=%d B=%d" % (F, D, itself, B)
            rng = np.random.default_rng(IR.seed_of("xwide", F, D, itself, B))
            T32 = IR.draw_block(rng, B, F, D)
            fd = torch.from_numpy(T32).to(DEV)
            # ---- forward, twice ----
            Rv, Rbuf = _dev_operand(B, width, ld, off, None, SENTINEL)
            vec = Rv.data_ptr() % 16 == 0 and ld % 4 == 0
            r = ops.interact_xwide_route("fwd", B, F, D, bool(itself), ld, Rv.data_ptr() % 16 == 0)
            assert r["family"] == "xwide" and r["lds_bytes"] <= 160 * 1024 and r["grid"] == min(B, big["fwd"] - 1), (what, r)
            ops.interact_fwd(fd, bool(itself), Rv)
            first = Rbuf.clone()
            ops.interact_fwd(fd, bool(itself), Rv)
            torch.cuda.synchronize()
            assert torch.equal(first.view(torch.int32), Rbuf.view(torch.int32)), what + ": a second forward call differs"
            buf = Rbuf.cpu().numpy()
            rows = buf[off:off + B * ld].reshape(B, ld)
            assert (buf[:off] == SENTINEL).all() and (buf[off + B * ld:] == SENTINEL).all(), what + ": written outside R"
            padw = rows[:, width:min(pad4(width), ld)]
            assert (padw == 0).all() if vec else (padw == SENTINEL).all(), what + ": pad word"
            assert (rows[:, pad4(width):] == SENTINEL).all(), what + ": R written behind pad4(width)"
            IR.check_fwd(rows, T32, itself, what, "xwide")
            # ---- backward ----
            dR32 = rng.standard_normal((B, width), dtype=np.float32)
            dR_src = torch.from_numpy(dR32).to(DEV)
            for x_act in (0, 1, 2):
                T32[:, 0] = IR.draw_row0(rng, B, D, x_act)
                fd = torch.from_numpy(T32).to(DEV)
                dRv, _ = _dev_operand(B, width, ld, off, dR_src, NAN)          # NaN in every column >= D + npairs
                dfbuf = torch.full((B * F * D + 4,), SENTINEL, dtype=torch.float32, device=DEV)
                dfeat = dfbuf[:B * F * D].view(B, F, D)
                r = ops.interact_xwide_route("bwd", B, F, D, bool(itself), ld, dRv.data_ptr() % 16 == 0, True)
                assert r["family"] == "xwide" and r["lds_bytes"] <= 160 * 1024 and r["grid"] == min(B, big["bwd"] - 1), (what, r)
                ops.interact_bwd(fd, dRv, bool(itself), dfeat, x_act=x_act)
                torch.cuda.synchronize()
                assert _gap_ok(dRv, ld, width, NAN) and torch.equal(dRv, dR_src), what + ": dR was written"
                got = dfbuf.cpu().numpy()
                assert (got[B * F * D:] == SENTINEL).all(), what + ": written past row B of dfeat"
                IR.check_bwd(got[:B * F * D].reshape(B, F, D), T32, dR32, itself, x_act, "%s x_act=%d" % (what, x_act), "xwide")


@pytest.mark.gpu
@pytest.mark.parametrize("T,m_spa", [(64, 32), (127, 64)])
def test_engine_with_65_and_128_features_vs_oracle(ops, T, m_spa):
    """TrainEngine at 64 and 127 tables (tiny tables: misses and evictions in every window), four steps across a window boundary:
    loss per iteration against the oracle trainer at rtol 1e-5, tags bit-exact; the natively taped run equals the Python-issued
    one bit for bit, and the step's interaction calls are the xwide ones."""
    from oracle import cdlrm_oracle as O
    sizes = [40, 30, 5, 37, 50, 64, 31, 7]
    ln_emb = [sizes[k % len(sizes)] + k % 5 for k in range(T)]
    B, L, ways, cache_size, seed = 32, 2, 4, 16, 31
    ln_bot = np.array([13, 32, m_spa])
    nf = T + 1
    ln_top = np.array([m_spa + nf * (nf - 1) // 2, 32, 1])
    rng = np.random.RandomState(T)
    batches = []
    for j in range(4):
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
    py, native = IW._train(*args, native=False), IW._train(*args, native=True)
    np.testing.assert_allclose(py[0], np.array([l[0] for l in otr.losses]), rtol=1e-5)
    for k in range(T):
        assert torch.equal(py[1][k], otr.occ[k]), "tag state differs for table %d" % k
    assert np.array_equal(py[0], native[0]) and torch.equal(py[2], native[2]), "the native tape's run differs"
    for names in (py[3], native[3]):
        assert "cdlrm_interact_xwide_fwd" in names and "cdlrm_interact_xwide_bwd" in names
        assert not [n for n in names if "interact" in n and "xwide" not in n], names


def test_xwide_route_and_cli_limits(ops):
    """The route query refuses F = 64, F = 129 and D = 130 and takes (65, 4) and (128, 512) inside the LDS budget; the CLI takes
    127 tables past its table-count check and ends 128 in one ERROR: line that names 127."""
    from cdlrm_amd import _lib
    for F, D in ((64, 32), (129, 32), (100, 130)):
        for op in ("fwd", "bwd"):
            with pytest.raises(_lib.CdlrmError, match="64<F<=128"):
                ops.interact_xwide_route(op, 1, F, D, False, pad4(D + npairs_of(F, 0)))
    with pytest.raises(_lib.CdlrmError, match="ld_r"):
        ops.interact_xwide_route("fwd", 1, 80, 32, False, 32 + npairs_of(80, 0) - 1)
    for F, D in ((65, 4), (128, 512)):
        for op in ("fwd", "bwd"):
            r = ops.interact_xwide_route(op, 4, F, D, True, pad4(D + npairs_of(F, 1)))
            assert r["family"] == "xwide" and r["grid"] == 4 and r["lds_bytes"] <= 160 * 1024, r
    # (a bottom MLP that ends on another width than the tables' is the next check behind the table count, before any GPU call)
    for T, line in ((128, "ERROR: --arch-interaction-op=dot takes at most 127 embedding tables"), (127, "ERROR: arch-sparse-feature-size 16")):
        p = subprocess.run([sys.executable, "-m", "cdlrm_amd.main_no_ddp", "--arch-interaction-op=dot", "--arch-sparse-feature-size=16",
                            "--arch-mlp-bot=13-8", "--arch-embedding-size=" + "-".join(["10"] * T), "--data-generation=random",
                            "--world-size=1"],
                           cwd=ROOT, capture_output=True, text=True)
        assert p.returncode != 0 and line in p.stderr and p.stderr.count("ERROR:") == 1, (T, p.stderr[-400:])
