"""The embedding-backward apply kernels' device results, bit for bit, against digests recorded from the build in front of the
consolidation of the SGD and row-wise Adagrad kernel bodies: tests/golden/emb_apply_digests.json.

Per case of test_rowwise_adagrad.KERNEL_CASES (seeded numpy inputs), sha256 of the bytes after ONE launch on fresh rows / state:
  sgd   weight                      (cdlrm_embbag_bwd_apply / _apply_sorted; the state stays S0, asserted as such)
  ada   weight, state               (the _opt entries, opt = rowwise_adagrad)
  rest  weight, touched             (cdlrm_embbag_bwd_apply_rest / _apply_sorted(rest = 1) with a touched buffer: the skip-once
                                     branch and, without offsets, the lean k_bwd_blocks_sgd<.., 1, 8>; the state stays S0)
The kernels use no float atomics and the long-run list's atomicAdd only orders independent runs, so the bytes do not depend on the
run or the machine: the comparison is equality.  `python tests/test_emb_apply_digests.py OUT.json` records the fixture (GPU).
"""
import hashlib
import json
import os
import sys

import numpy as np
import pytest
import torch

import test_rowwise_adagrad as A

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(A.ROOT, "tests", "golden", "emb_apply_digests.json")
ops = A.ops


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def _rest(ops, c, entry, phase, touched):
    """The `rest` apply of the case's batch: the runs of >= 2 lookups; runs of one lookup only flag their rows."""
    n, D = c.n, c.D
    work = ops.embbag_bwd_work(c.ctx, n, A.DEV)
    if entry == "apply":
        ops.embbag_bwd_prepare(c.ctx, torch.from_numpy(c.slots).to(A.DEV), work)
        ops.embbag_bwd_apply_rest(c.ctx, n, c.offs, c.grad, 3 * D, D, A.LR, work, touched)
    else:
        nb, j = 2, 1
        ws = torch.from_numpy(np.concatenate([c.slots[:, ::-1], c.slots], axis=1).copy()).to(A.DEV)
        sbuf = ops.embbag_bwd_sorted(c.ctx, nb, n, A.DEV)
        ops.embbag_bwd_prepare_window(c.ctx, ws, n, nb, n, sbuf)
        k, m, _ = ops.embbag_bwd_sorted_views(c.ctx, sbuf, nb, n, j)
        ops.embbag_bwd_apply_sorted(c.ctx, n, c.grad, 3 * D, D, A.LR, work, k, m, nb * n, phase, True, touched)
    torch.cuda.synchronize()
    c.ctx.check()
    return c.weight.cpu().numpy(), c.state.cpu().numpy()


def digests_of(ops, D, n, kind, entry, form, bags):
    c = A.Case(ops, D, n, kind, bags)
    phase = 1 if entry == "sorted" else 0
    out = {}
    with A.debug6(64 if form == "blocks" else 0):
        c.reset()
        w, s = c.launch(ops, entry, opt="sgd", lr=A.LR, aux_phase=phase, sgd_sibling=True)
        assert np.array_equal(s.view(np.int32), c.S0.view(np.int32))
        out["sgd"] = {"weight": _sha(w)}
        c.reset()
        w, s = c.launch(ops, entry, opt="rowwise_adagrad", lr=A.LR, aux_phase=phase)
        out["ada"] = {"weight": _sha(w), "state": _sha(s)}
        c.reset()
        touched = torch.zeros(c.ctx.total_rows, dtype=torch.uint8, device=A.DEV)
        route = ops.embbag_bwd_route(3, D, n, bags, "sorted_rest" if entry == "sorted" else "rest", nb=2 if entry == "sorted" else 1)
        assert route["apply"] == ("blocks" if bags else "blocks_lean")
        w, s = _rest(ops, c, entry, phase, touched)
        assert np.array_equal(s.view(np.int32), c.S0.view(np.int32))
        t = touched.cpu().numpy()
        assert t.any() or n == 1
        out["rest"] = {"weight": _sha(w), "touched": _sha(t)}
    return out


@pytest.fixture(scope="module")
def recorded():
    with open(GOLDEN) as f:
        return json.load(f)["cases"]


def test_the_fixture_names_every_kernel_case(recorded):
    assert sorted(recorded) == sorted(A.KERNEL_IDS)


@pytest.mark.parametrize("case", A.KERNEL_CASES, ids=A.KERNEL_IDS)
def test_apply_bits_are_the_recorded_ones(ops, recorded, case):
    got = digests_of(ops, *case)
    assert got == recorded[A.KERNEL_IDS[A.KERNEL_CASES.index(case)]]


if __name__ == "__main__":
    sys.path.insert(0, A.ROOT)
    from cdlrm_amd import _lib
    _lib.lib()
    from cdlrm_amd import ops as _ops
    rec = {"what": "sha256 of the device bytes after one launch per case of tests/test_rowwise_adagrad.py KERNEL_CASES; "
                   "recorded at commit 91dd06f, in front of the consolidation of the apply kernels",
           "cases": {i: digests_of(_ops, *c) for i, c in zip(A.KERNEL_IDS, A.KERNEL_CASES)}}
    with open(sys.argv[1], "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")
    print("recorded %d cases" % len(rec["cases"]))
