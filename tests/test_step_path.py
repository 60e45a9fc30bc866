"""A training step decides its control path once (engine.StepPath) and the launch tapes are keyed by it.

The step's calls -- every entry of tests/step_trace.py's log: name, streams and events by label, scalars by value, tensors by
shape and strides -- are held to what the commit before StepPath issued (tests/golden/step_traces_*.json, made by running
tests/step_trace.py there), untaped and as tapes; in the same runs equal (path, layout) keys must mean equal call sequences,
step by step; every assignable knob the path holds must change it; and the hand-over record between steps is checked on its
own."""
import functools
import json
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import step_trace as ST     # noqa: E402


@functools.lru_cache(maxsize=None)
def _fixture(which):
    with open(os.path.join(ROOT, "tests", "golden", "step_traces_%s.json" % which)) as f:
        return json.load(f)


def _same_key_same_trace(keys, steps, where):
    first = {}
    for j, (k, t) in enumerate(zip(keys, steps)):
        assert k is not None and hash(k) is not None
        j0 = first.setdefault(k, j)
        assert steps[j0] == t, "%s: steps %d and %d have one key and two call sequences" % (where, j0, j)


# ---- CPU ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ST.CPU_CASES, ids=ST.cpu_case_name)
def test_cpu_steps_issue_the_parents_calls_and_the_key_determines_them(case):
    keys = []
    tr = ST.cpu_run(case, ST.Pool(), after_step=lambda eng, j, nxt: keys.append(eng._step_key))
    fix = _fixture("cpu")
    want = ST.expand(fix, fix["runs"][ST.cpu_case_name(case)]["steps"])
    got = ST.expand(tr.pool, tr.steps)
    assert len(got) == len(want) == 6
    for j, (g, w) in enumerate(zip(got, want)):
        assert g == w, "step %d" % j
    assert len(keys) == len(tr.steps)
    _same_key_same_trace(keys, tr.steps, ST.cpu_case_name(case))


# knob -> another value.  B is 64 in these runs: gather_alone_min and tape_lanes_below are assigned ACROSS it
KNOBS = dict(gather_alone_min=1, attach_events=False, fuse_gather=False, fuse_once=False, wide_gemm=False,
             matmul_precision="bf16", tape_lanes=2, tape_lanes_below=1, lr=0.05, lr_embeds=0.05)


@pytest.mark.parametrize("knob", sorted(KNOBS))
def test_assigning_a_knob_between_two_steps_changes_the_path(knob, monkeypatch):
    """Two calls of the path's one builder on the same batch in the same engine state, the knob assigned in between.  The
    knobs that only act on a HIP device (attached events, the fused gather and its once-only fold) are asked as on one: with
    the device test and the kernels' shape query answering yes, and sorted lists for this batch."""
    import cdlrm_amd.engine as E
    case = dict(aux=2, alone=None, defer=False, op="dot")
    got = []

    def ask(eng, j, nxt):
        if j != 1:
            return
        monkeypatch.setattr(E.S, "is_hip", lambda dev: True)
        monkeypatch.setattr(E.ops, "gather_interact_supported", lambda ctx: True, raising=False)
        cur, eng._cur_sorted = eng._cur_sorted, E.SortedViews(1, 2, 3, 64, None, 1)
        X, idx = torch.zeros(64, 5), torch.zeros(eng.T, 64, dtype=torch.int64)
        try:
            old = getattr(eng, knob)
            a = eng._step_path(X, idx, None, nxt)
            b = eng._step_path(X, idx, None, nxt)
            setattr(eng, knob, KNOBS[knob])
            c = eng._step_path(X, idx, None, nxt)
            setattr(eng, knob, old)
            got.append((a, b, c, eng._step_path(X, idx, None, nxt)))
        finally:
            eng._cur_sorted = cur
            monkeypatch.undo()

    ST.cpu_run(case, ST.Pool(), before_step=ask, steps=3)
    a, b, c, d = got[0]
    assert a == b == d and hash(a) == hash(b), "the path is a function of the step's inputs"
    assert c != a, knob
    if knob == "gather_alone_min":
        assert a.side_gather and not c.side_gather and not a.gather_alone and c.gather_alone


def test_the_handover_record():
    """matches(): the index tensor by address and shape.  A launch tape keeps the record without the address, and the record
    made from it for the next batch equals the one the recording step left behind."""
    import cdlrm_amd.engine as E
    case = dict(aux=2, alone=None, defer=False, op="dot")
    seen = []

    def tape_on(eng, j, nxt):
        eng.use_tape, eng.native_tape = True, False       # (both steps record: they run _fwd_bwd itself)

    def look(eng, j, nxt):
        if j == 0:
            left = eng._pref
            assert isinstance(left, E.Handover) and left.matches(nxt)
            assert not left.matches(nxt.clone()), "another address"
            assert not left.matches(nxt[:, :32]), "another shape"
            assert not left.matches(nxt[:, 1:]), "another address and shape"
            stored = list(eng._tapes.values())[-1]["pref"]
            assert stored.ptr == 0 and not stored.matches(nxt)
            assert stored.handed(nxt) == left
            seen.append(len(eng._tapes))

    ST.cpu_run(case, ST.Pool(), before_step=tape_on, after_step=look, steps=2)
    assert seen == [1]


# ---- GPU ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _untaped(shape, variant):
    """(expanded traces, keys, step trace numbers, losses, pool) of one untaped run: made once, shared by the tests below."""
    import numpy as np
    golden = lambda name: np.load(os.path.join(ROOT, "tests", "golden", name + ".npz"))
    keys = []
    tr, _, losses = ST.gpu_run(ST.gpu_shapes(golden)[shape], variant, False, ST.Pool(),
                               after_step=lambda eng, j: keys.append(eng._step_key))
    return ST.expand(tr.pool, tr.steps), keys, tr.steps, losses, tr.pool


SHAPES = ("train_small", "train_c1", "fused_shape")


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ST.GPU_VARIANTS)
def test_gpu_steps_issue_the_parents_calls(variant):
    fix = _fixture("gpu")
    for shape in SHAPES:
        got, keys, steps, _, _ = _untaped(shape, variant)
        want = ST.expand(fix, fix["runs"]["%s/%s" % (shape, variant)]["steps"])
        assert len(got) == len(want)
        for j, (g, w) in enumerate(zip(got, want)):
            assert g == w, "%s step %d" % (shape, j)
        _same_key_same_trace(keys, steps, "%s/%s" % (shape, variant))


@pytest.mark.gpu
def test_the_gpu_matrix_reaches_the_hip_only_branches():
    """The once-only fold, both take streams, the attached mark of a placed resolve and the slice-sorted update all occur in
    the runs above (and did on the parent: the fixture holds them too)."""
    want = (("gather_interact_bwd_sgd", {}), ("embbag_take", dict(stream="stream:pref")),
            ("embbag_take", dict(stream="stream:side")), ("event_attach_next", dict(first="event:fwd_mark")),
            ("embbag_bwd_apply_sorted", {}))
    fix = _fixture("gpu")
    fpool = ST.Pool()
    fpool.entries, fpool.traces = fix["entries"], fix["traces"]
    missing = {w[0] + repr(w[1]) for w in want}
    for name, kw in want:
        assert ST.has_entry(fpool, range(len(fix["traces"])), name, **kw), "the fixture misses %s %r" % (name, kw)
        for shape in SHAPES:
            for variant in ST.GPU_VARIANTS:
                _, _, steps, _, pool = _untaped(shape, variant)
                if ST.has_entry(pool, steps, name, **kw):
                    missing.discard(name + repr(kw))
    assert not missing
    # ... each where it is meant to: the chained take on the side stream, the placed resolve's mark on the fused forward
    _, _, steps, _, pool = _untaped("train_c1", "gather_alone_min_1")
    assert ST.has_entry(pool, steps, "embbag_take", stream="stream:side")
    _, _, steps, _, pool = _untaped("fused_shape", "place_resolve")
    assert ST.has_entry(pool, steps, "event_attach_next", first="event:fwd_mark")
    _, _, steps, _, pool = _untaped("fused_shape", "default")
    assert ST.has_entry(pool, steps, "gather_interact_bwd_sgd")


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ST.GPU_VARIANTS)
def test_gpu_tapes_are_the_parents_and_replay_the_untaped_losses(variant):
    import numpy as np
    golden = lambda name: np.load(os.path.join(ROOT, "tests", "golden", name + ".npz"))
    fix = _fixture("gpu")
    for shape in SHAPES:
        _, eng, losses = ST.gpu_run(ST.gpu_shapes(golden)[shape], variant, True)
        assert not eng.tape_fallbacks
        want = fix["runs"]["%s/%s" % (shape, variant)]["tapes"]
        got = ST.tape_names(eng)
        assert len(got) == len(want), shape
        assert got == want, shape
        assert all(isinstance(k[0], type(eng._step_key[0])) and t["prog"] and "cells" in t and "native" in t
                   for k, t in eng._tapes.items())
        assert torch.equal(losses, _untaped(shape, variant)[3]), "%s: taped and untaped losses differ" % shape
