"""The opt-in bf16 / bf16x3 dot interaction at 65 to 128 features (csrc/interact_xwide_b16.hip) against float64.

Numerics contract: every operand element of the two contractions is converted once (feat forward; S = G + G^T and feat backward),
products of bf16 values are exact in fp32, accumulation is fp32; R[:, :D] and the dR[:, :D] term of dfeat row 0 are exact.
  bf16:   against the float64 contraction of the ROUNDED operands, within the fp32-chain bound of tests/test_interact_routes.py
          (K = D forward; backward K = F + 2 as there: the contraction, the fp32 add of dR[:, :D], act').
  bf16x3: against the float64 contraction of the UNSPLIT operands, within tests/test_gemm_bf16x3.py's bound, K = D forward, K = F
          backward.  Row 0 of the backward takes one more fp32 add, |dR[:, :D]| being part of its magnitude: at most 2^-24 * mag
          more, which K = F + 1 grants (6 * 2^-24 * mag); the roundings of act' -- (1 - y) * y and the product, three -- lie
          inside the bound's 8 * 2^-24 * |ref|.
Both bounds are imported, not restated.  dR holds NaN behind the pairs; R and dfeat hold a sentinel wherever no output belongs.
"""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import test_interact_routes as IR      # noqa: E402
import test_interact_wide as IW        # noqa: E402
import test_gemm_bf16x3 as X3          # noqa: E402
from test_interact_routes import SENTINEL, NAN, DEV, npairs_of, pad4, _dev_operand, _gap_ok, assert_within      # noqa: E402

ops = IR.ops        # the fixture: builds the library where it is missing
NAMES = ["cdlrm_interact_xwide_b16_%s" % s for s in ("fwd", "bwd", "route")]
# (F, D, pitch pad ("p4": rounded up to 4), element offset of R / dR, batches)
CASES = [
    (65, 4, "p4", 0, (1, 3, 513, 257)),     # third block a single row; one slab narrower than a k-step; one past either grid
    (96, 36, "p4", 0, (1, 3)),              # the 96 / 128 edge; second slab 4 columns wide
    (97, 48, "p4", 0, (1, 3)),              # NB = 4 with one row in block 3; tail slab exactly one k-step
    (128, 32, "p4", 0, (1, 3)),             # full matrix, one whole slab
    (128, 132, "p4", 0, (1, 3)),            # five slabs, narrow tail
    (80, 36, 1, 1, (3,)),                   # ld_r = width + 1, R / dR / dfeat off by one element: the scalar tiers
]


def bf(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).bfloat16().float().numpy()


def check(prec, got, ref, mag, k_chain, k_x3, what):
    if prec == "bf16":
        assert_within(got, ref, mag, k_chain, what, "xwide")
    else:
        X3.assert_within_x3(got, ref, mag, k_x3, what)


@pytest.mark.gpu
@pytest.mark.parametrize("prec", ["bf16", "bf16x3"])
@pytest.mark.parametrize("F,D,pad,off,batches", CASES, ids=lambda v: str(v))
def test_b16_kernels_vs_float64(ops, F, D, pad, off, batches, prec):
    for itself in (0, 1):
        width = D + npairs_of(F, itself)
        ld = pad4(width) if pad == "p4" else width + pad
        for B in batches:
            what = "%s F=%d D=%d itself=%d B=%d" % (prec, F, D, itself, B)
            rng = np.random.default_rng(IR.seed_of("xwide_b16", F, D, itself, B))
            T32 = IR.draw_block(rng, B, F, D)
            fd = torch.from_numpy(T32).to(DEV)
            # ---- forward, twice ----
            Rv, Rbuf = _dev_operand(B, width, ld, off, None, SENTINEL)
            vec = Rv.data_ptr() % 16 == 0 and ld % 4 == 0
            r = ops.interact_xwide_b16_route("fwd", B, F, D, bool(itself), ld, prec, Rv.data_ptr() % 16 == 0)
            assert r["family"] == "xwide_b16" and r["lds_bytes"] <= 160 * 1024 and r["grid"] == min(B, 512), (what, r)
            ops.interact_fwd(fd, bool(itself), Rv, precision=prec)
            first = Rbuf.clone()
            ops.interact_fwd(fd, bool(itself), Rv, precision=prec)
            torch.cuda.synchronize()
            assert torch.equal(first.view(torch.int32), Rbuf.view(torch.int32)), what + ": a second forward call differs"
            buf = Rbuf.cpu().numpy()
            rows = buf[off:off + B * ld].reshape(B, ld)
            assert (buf[:off] == SENTINEL).all() and (buf[off + B * ld:] == SENTINEL).all(), what + ": written outside R"
            padw = rows[:, width:min(pad4(width), ld)]
            assert (padw == 0).all() if vec else (padw == SENTINEL).all(), what + ": pad word"
            assert (rows[:, pad4(width):] == SENTINEL).all(), what + ": R written behind pad4(width)"
            assert np.array_equal(rows[:, :D].view(np.uint32), T32[:, 0].view(np.uint32)), what + ": R[:, :D] is not feature 0 bit for bit"
            Z, mag = IR.ref_fwd((bf(T32) if prec == "bf16" else T32).astype(np.float64), itself)
            check(prec, rows[:, D:width], Z, mag, D, D, what + " pairs")
            # ---- backward, twice ----
            dR32 = rng.standard_normal((B, width), dtype=np.float32)
            dR_src = torch.from_numpy(dR32).to(DEV)
            for x_act in (0, 1, 2):
                T32[:, 0] = IR.draw_row0(rng, B, D, x_act)
                fd = torch.from_numpy(T32).to(DEV)
                dRv, _ = _dev_operand(B, width, ld, off, dR_src, NAN)           # NaN in every column >= D + npairs
                dfbuf = torch.full((off + B * F * D + 4,), SENTINEL, dtype=torch.float32, device=DEV)
                dfeat = dfbuf[off:off + B * F * D].view(B, F, D)
                r = ops.interact_xwide_b16_route("bwd", B, F, D, bool(itself), ld, prec, dRv.data_ptr() % 16 == 0, off == 0)
                assert r["family"] == "xwide_b16" and r["lds_bytes"] <= 160 * 1024 and r["grid"] == min(B, 256), (what, r)
                ops.interact_bwd(fd, dRv, bool(itself), dfeat, x_act=x_act, precision=prec)
                first = dfbuf.clone()
                ops.interact_bwd(fd, dRv, bool(itself), dfeat, x_act=x_act, precision=prec)
                torch.cuda.synchronize()
                assert torch.equal(first.view(torch.int32), dfbuf.view(torch.int32)), what + ": a second backward call differs"
                assert _gap_ok(dRv, ld, width, NAN) and torch.equal(dRv, dR_src), what + ": dR was written"
                got = dfbuf.cpu().numpy()
                assert (got[:off] == SENTINEL).all() and (got[off + B * F * D:] == SENTINEL).all(), what + ": written outside dfeat"
                got = got[off:off + B * F * D].reshape(B, F, D)
                # the reference: operands rounded (bf16) or as they are (bf16x3); the direct path and act'(feature 0) never rounded
                Tq, dRq = T32.astype(np.float64), dR32.astype(np.float64)
                if prec == "bf16":
                    Tq, dRq = bf(T32).astype(np.float64), np.concatenate([dR32[:, :D], bf(dR32[:, D:])], axis=1).astype(np.float64)
                ref, mag = IR.ref_bwd(Tq, dRq, itself, 0)
                m = IR.R.act_grad(T32[:, 0].astype(np.float64), x_act)
                ref[:, 0] *= m
                mag[:, 0] *= np.abs(m)
                w = "%s x_act=%d dfeat" % (what, x_act)
                check(prec, got[:, 0], ref[:, 0], mag[:, 0], F + 2, F + 1, w + " row 0")
                check(prec, got[:, 1:].reshape(-1, D), ref[:, 1:].reshape(-1, D), mag[:, 1:].reshape(-1, D), F + 2, F, w)


@pytest.mark.gpu
@pytest.mark.parametrize("prec", ["bf16", "bf16x3"])
def test_inf_in_one_row_reaches_exactly_its_pairs(ops, prec):
    F, D, B, bad = 97, 36, 2, 70
    T32 = IR.draw_block(np.random.default_rng(5), B, F, D)
    T32[1, bad, 17] = np.inf
    R = torch.zeros(B, pad4(D + npairs_of(F, 1)), device=DEV)
    ops.interact_fwd(torch.from_numpy(T32).to(DEV), True, R, precision=prec)
    i, j = IR.pair_ij(F, 1)
    finite = np.isfinite(R.cpu().numpy()[:, D:D + len(i)])
    assert finite[0].all() and np.array_equal(~finite[1], (i == bad) | (j == bad))


@pytest.fixture(scope="module")
def runs():
    """(python-issued, natively taped) training runs by interact_precision, each made once: (T, D) = (64, 32), six steps, windows of
    three."""
    T, m_spa, B, L, ways, cache_size, seed = 64, 32, 32, 3, 4, 16, 31
    sizes = [40, 30, 5, 37, 50, 64, 31, 7]
    ln_emb = [sizes[k % len(sizes)] + k % 5 for k in range(T)]
    ln_bot, ln_top = np.array([13, 32, m_spa]), np.array([m_spa + (T + 1) * T // 2, 32, 1])
    rng = np.random.RandomState(T)
    batches = []
    for j in range(6):
        X = torch.from_numpy(rng.rand(B, 13).astype(np.float32))
        idx = torch.stack([torch.from_numpy((rng.zipf(1.2, size=B).astype(np.int64) * 2654435761 % n)) for n in ln_emb])
        batches.append((X, idx, torch.from_numpy(np.round(rng.rand(B, 1)).astype(np.float32))))
    args = (T, m_spa, batches, L, B, ways, cache_size, seed, ln_emb, ln_bot, ln_top)
    from cdlrm_amd.engine import TrainEngine
    done = {}

    def run(prec):
        if prec not in done:
            with pytest.MonkeyPatch.context() as mp:
                mp.setattr(TrainEngine, "interact_precision", prec)
                done[prec] = (IW._train(*args, native=False), IW._train(*args, native=True))
        return done[prec]
    return run


# max |loss - fp32 run's loss| over the six steps, measured on an MI355X: 7.31e-4 (bf16), 2.38e-7 (bf16x3).  The deviation depends
# on the seed's data, so each tolerance is four times its measured value (the margin of DESIGN.md 4.1).
LOSS_TOL = {"bf16": 4 * 7.31e-4, "bf16x3": 4 * 2.38e-7}


@pytest.mark.gpu
@pytest.mark.parametrize("prec", ["bf16x3", "bf16"])
def test_engine_trains_on_the_b16_pair(ops, runs, prec):
    (ref, _), (py, native) = runs("fp32"), runs(prec)
    assert np.array_equal(py[0], native[0]) and torch.equal(py[2], native[2]), "the native tape's run differs"
    for names in (py[3], native[3]):
        assert "cdlrm_interact_xwide_b16_fwd" in names and "cdlrm_interact_xwide_b16_bwd" in names
        assert not [n for n in names if "interact" in n and "b16" not in n], names
    assert "cdlrm_interact_xwide_fwd" in ref[3] and "cdlrm_interact_xwide_bwd" in ref[3] and not [n for n in ref[3] if "b16" in n]
    assert all(torch.equal(a, b) for a, b in zip(py[1], ref[1])), "tag state differs from the fp32 run's"
    dev = {p: float(np.abs(runs(p)[0][0].astype(np.float64) - ref[0]).max()) for p in ("bf16", "bf16x3")}
    print("max |loss - fp32 loss| over six steps:", dev)
    assert dev[prec] <= LOSS_TOL[prec] and dev["bf16x3"] <= dev["bf16"], dev


def test_route_query_cli_and_abi(ops):
    from cdlrm_amd import _lib
    for F, D in ((65, 4), (128, 512)):
        for op in ("fwd", "bwd"):
            for prec in ("bf16", "bf16x3"):
                r = ops.interact_xwide_b16_route(op, 4, F, D, True, pad4(D + npairs_of(F, 1)), prec)
                assert r["family"] == "xwide_b16" and r["grid"] == 4 and r["ns"] == (D + 31) // 32 and r["lds_bytes"] <= 160 * 1024, r
    for F, D, planes, words in ((64, 32, 1, "64<F<=128"), (129, 32, 2, "64<F<=128"), (100, 130, 1, "64<F<=128"), (100, 32, 3, "planes")):
        for op in ("fwd", "bwd"):
            with pytest.raises(_lib.CdlrmError, match=words):
                ops.interact_xwide_b16_route(op, 1, F, D, False, pad4(D + npairs_of(F, 0)), planes)
    with pytest.raises(_lib.CdlrmError, match="ld_r"):
        ops.interact_xwide_b16_route("fwd", 1, 80, 32, False, 32 + npairs_of(80, 0) - 1, "bf16")
    p = subprocess.run([sys.executable, "-m", "cdlrm_amd.main_no_ddp", "--interaction-precision=bf16x4", "--data-generation=random",
                        "--world-size=1"], cwd=ROOT, capture_output=True, text=True)
    assert p.returncode != 0 and "ERROR: --interaction-precision=bf16x4" in p.stderr and p.stderr.count("ERROR:") == 1, p.stderr[-400:]
    hdr = open(os.path.join(ROOT, "include", "cdlrm_hip.h")).read()
    tape = open(os.path.join(ROOT, "cdlrm_amd", "csrc", "tape.hip")).read()
    for name in NAMES:
        assert re.search(r"\bint %s\(" % name, hdr) and name in _lib.PROTOTYPES and hasattr(_lib.raw(), name), name
        assert ("TAPE_FN(%s)" % name in tape) == name.endswith(("_fwd", "_bwd")), name
