"""The fused gather at 65 to 128 features (cdlrm_gather_interact_xwide_fwd / _bwd, csrc/interact_xwide.hip): bit for bit against
embbag_fwd + interact_fwd / interact_bwd on the same slots, every element against float64 on the gathered block with the
comparators and bounds of tests/test_interact_routes.py (imported, not restated), the refusals, and a TrainEngine with
fuse_gather_wide at 64 and 127 tables against the same run on two operators.
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
from test_gather_interact_wide import _train      # noqa: E402

ops = IR.ops        # the fixture: builds the library where it is missing
NAMES = ["cdlrm_gather_interact_xwide_" + s for s in ("supported", "fwd", "bwd", "grid")]
CAPS = {"fwd": 512, "bwd": 256}

# (F, D, also B = 2 * the larger grid + 1: a workgroup of either kernel walks three samples, the two-ahead ids past their priming)
CASES = [(65, 32, True),        # one gathered row in the third block; one slab, every step a sample switch
         (96, 64, False),       # three full blocks, the idle fourth wave
         (97, 128, False),      # first four-block shape
         (128, 20, True),       # full matrix, zero-filled tail slab, rows of 80 bytes
         (128, 256, False)]     # full matrix, many slabs


@pytest.mark.gpu
@pytest.mark.parametrize("F,D,walk", CASES, ids=lambda v: str(v))
def test_xwide_gather_kernels_vs_two_operators_and_float64(ops, F, D, walk):
    T = F - 1
    ctx, w, base, _ = make_ctx(ops, T, D)
    assert ops.gather_interact_xwide_supported(ctx) and not ops.gather_interact_wide_supported(ctx)
    walkB = [2 * max(ops.gather_interact_xwide_grid(ctx, op, 1 << 20)[0] for op in CAPS) + 1] if walk else []
    for itself in (0, 1):
        width = D + npairs_of(F, itself)
        ld = pad4(width)
        for B in [1, 2, 3] + walkB:
            what = "F=%d D=%d itself=%d B=%d" % (F, D, itself, B)
            for op, cap in CAPS.items():
                assert ops.gather_interact_xwide_grid(ctx, op, B)[0] == min(B, cap), what
            rng = np.random.default_rng(IR.seed_of("gather_xwide", F, D, itself, B))
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
                    ops.gather_interact_xwide_fwd(ctx, slots, x, bool(itself), Rv)
                    ops.interact_fwd(feat, bool(itself), R2)
                    rows = Rbuf.cpu().numpy()[:B * (ld + 4)].reshape(B, ld + 4)
                    assert (Rbuf[B * (ld + 4):] == SENTINEL).all(), what + ": written past row B of R"
                    assert torch.equal(Rv, R2[:, :width]), what + ": differs from embbag_fwd + interact_fwd"
                    assert (rows[:, width:ld] == 0).all() and (rows[:, ld:] == SENTINEL).all(), what + ": pad words / behind pad4(width)"
                    IR.check_fwd(rows, T32, itself, what, "xwide")
                # ---- backward ----
                dRv, _ = _dev_operand(B, width, ld, 0, dR_src, NAN)           # NaN in every column >= D + npairs
                dfbuf = torch.full((B * F * D + 4,), SENTINEL, dtype=torch.float32, device=DEV)
                dfeat, df2 = dfbuf[:B * F * D].view(B, F, D), torch.empty(B, F, D, device=DEV)
                ops.gather_interact_xwide_bwd(ctx, slots, x, dRv, bool(itself), dfeat, x_act=x_act)
                ops.interact_bwd(feat, dRv, bool(itself), df2, x_act=x_act)
                assert _gap_ok(dRv, ld, width, NAN) and torch.equal(dRv, dR_src), what + ": dR was written"
                got = dfbuf.cpu().numpy()
                assert (got[B * F * D:] == SENTINEL).all(), what + ": written past row B of dfeat"
                assert torch.equal(dfeat, df2), "%s x_act=%d: differs from interact_bwd on the gathered block" % (what, x_act)
                IR.check_bwd(got[:B * F * D].reshape(B, F, D), T32, dR32, itself, x_act, "%s x_act=%d" % (what, x_act), "xwide")


@pytest.mark.gpu
def test_xwide_gather_refusals(ops):
    """T + 1 = 64 and 129 and D = 516 have no kernel (supported is 0); D = 30 cannot even be a context; an unaligned R and a pitch
    that is no multiple of 4 are refused on a supported context.  Every refusal has a message and leaves the outputs alone."""
    from cdlrm_amd import _lib
    with pytest.raises(_lib.CdlrmError, match="multiple of 4"):
        make_ctx(ops, 80, 30)
    for T, D, off, dld, msg in ((63, 32, 0, 0, "unsupported shape"), (128, 32, 0, 0, "unsupported shape"),
                                (80, 516, 0, 0, "unsupported shape"), (80, 32, 1, 0, "ld_r"), (80, 32, 0, 2, "ld_r")):
        ctx, _, _, _ = make_ctx(ops, T, D)
        assert ops.gather_interact_xwide_supported(ctx) == (msg == "ld_r")
        ld = pad4(D + npairs_of(T + 1, 0)) + dld
        buf = torch.full((3 * ld + 4,), SENTINEL, device=DEV)
        Rm = buf[off:off + 3 * ld].view(3, ld)
        df = torch.full((3, T + 1, D), SENTINEL, device=DEV)
        slots, x = torch.zeros(T, 3, dtype=torch.int32, device=DEV), torch.zeros(3, D, device=DEV)
        for call in (lambda: ops.gather_interact_xwide_fwd(ctx, slots, x, False, Rm),
                     lambda: ops.gather_interact_xwide_bwd(ctx, slots, x, Rm, False, df)):
            with pytest.raises(_lib.CdlrmError, match=msg):
                call()
        if msg != "ld_r":
            with pytest.raises(_lib.CdlrmError, match=msg):
                ops.gather_interact_xwide_grid(ctx, "fwd", 3)
        torch.cuda.synchronize()
        assert bool((buf == SENTINEL).all()) and bool((df == SENTINEL).all())


@pytest.mark.gpu
@pytest.mark.parametrize("T,m_spa", [(64, 32), (127, 64)])
def test_engine_with_fuse_gather_wide_above_64_features_equals_two_operators(ops, T, m_spa):
    two, py, native = _train(T, m_spa, False, False), _train(T, m_spa, True, False), _train(T, m_spa, True, True)
    for run in (py, native):
        assert all(torch.equal(a, b) for a, b in zip(two[:3], run[:3])), "losses, tags or cache rows differ from the two-operator run"
        assert "cdlrm_gather_interact_xwide_fwd" in run[3] and "cdlrm_gather_interact_xwide_bwd" in run[3]
        assert not [n for n in run[3] if "cdlrm_interact_xwide" in n or n == "cdlrm_embbag_fwd" or "_wide_" in n], run[3]
    assert "cdlrm_interact_xwide_fwd" in two[3] and "cdlrm_embbag_fwd" in two[3]


def test_abi_holds_the_xwide_gather(ops):
    from cdlrm_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "cdlrm_hip.h")).read()
    tape = open(os.path.join(ROOT, "cdlrm_amd", "csrc", "tape.hip")).read()
    for name in NAMES:
        assert re.search(r"\bint %s\(" % name, hdr) and name in _lib.PROTOTYPES and hasattr(_lib.raw(), name), name
        assert ("TAPE_FN(%s)" % name in tape) == name.endswith(("_fwd", "_bwd")), name
    assert _lib.PROTOTYPES[NAMES[1]] == _lib.PROTOTYPES["cdlrm_gather_interact_fwd"]
    assert _lib.PROTOTYPES[NAMES[2]] == _lib.PROTOTYPES["cdlrm_gather_interact_bwd"]
