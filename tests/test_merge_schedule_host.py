"""The touched-row merge's schedule on the host: engine.MergeSchedule / merge_pieces against a restatement written here, and
engine.MergePump's bookkeeping with its device work (issue) replaced by a recorder.

Every rank has to cut a merge into the same pieces in the same order; the arithmetic that decides them (deadline classes, the
rows step d needs, rows per step, chunk cuts) runs here without a device, driven the way TrainEngine.step drives it: an
advance for d = 1 at the merge step, then per step wait(d) followed by advance(d + 1)."""
import itertools

import pytest

from cdlrm_amd import _streams as S
from cdlrm_amd.engine import MERGE_CLASS_FIRST, MERGE_LOOKAHEAD, MergePump, MergeSchedule, merge_pieces

NCLS = len(MERGE_CLASS_FIRST) + 1       # the deadline classes and the cold one
US = (1, 2, 7, 8, 9, 100, 1000)
KS = (1, 2, 3, 4, 8, 16, 33, 64)


def offsets(U, pattern):
    """Class offsets (NCLS + 1 entries, 0 first, U last) of a merge of U rows."""
    if pattern == "class0":         # every row is needed by the very next batch
        sizes = [U] + [0] * (NCLS - 1)
    elif pattern == "cold":         # no known batch needs any
        sizes = [0] * (NCLS - 1) + [U]
    elif pattern == "gaps":         # classes 1, 4 and 6 hold the rows, the others (the cold one too) are empty
        sizes = [0] * NCLS
        sizes[1], sizes[4] = U // 3, U // 2
        sizes[6] = U - sizes[1] - sizes[4]
    else:                           # "spread": about a seventh of what is left per class, the rest cold
        sizes, left = [], U
        for c in range(NCLS - 1):
            sizes.append(-(-left // 7))
            left -= sizes[-1]
        sizes.append(left)
    off = [0]
    for n in sizes:
        off.append(off[-1] + n)
    assert len(off) == NCLS + 1 and off[-1] == U and all(n >= 0 for n in sizes)
    return tuple(off)


PATTERNS = ("class0", "cold", "gaps", "spread")


def need_ref(off, K, U, d):
    """Rows due before the d-th step after the merge: the classes whose first batch is <= d, everything past the K known."""
    if d > K:
        return U
    return max([0] + [off[c + 1] for c in range(len(MERGE_CLASS_FIRST)) if MERGE_CLASS_FIRST[c] <= d])


def test_the_classes_are_the_ones_this_test_restates():
    assert MERGE_CLASS_FIRST == (1, 2, 3, 5, 9, 17, 33) and MERGE_LOOKAHEAD == 64
    assert merge_pieces(0, 9, 4) == [(0, 4), (4, 8), (8, 9)] and merge_pieces(5, 5, 4) == [] and merge_pieces(3, 5, 0) == [(3, 4), (4, 5)]


@pytest.mark.parametrize("U", US)
def test_schedule_against_the_restatement(U):
    for pattern, K, chunk in itertools.product(PATTERNS, KS, (1, 4, 8, U + 5)):
        off = offsets(U, pattern)
        for budget in sorted({1, 4, 8, U, 2 * U}):
            s = MergeSchedule(off, K, U, budget)
            case = (pattern, K, chunk, budget)
            issued, pieces = 0, []

            def advance(d_next):
                target = s.target(d_next, issued)
                assert target == max(need_ref(off, K, U, d_next), min(U, issued + budget)), case
                cuts = merge_pieces(issued, target, chunk)
                assert (cuts[-1][1] if cuts else issued) == target, case
                pieces.extend(cuts)
                return target

            issued = advance(1)                             # the merge step
            last = 0
            for d in range(1, K + 3):
                need = s.need(d)
                assert need == need_ref(off, K, U, d), (case, d)
                assert last <= need <= U and (d <= K or need == U), (case, d)          # monotone; everything past K
                assert issued >= need, ("rows step %d needs were never issued" % d, case)
                last = need
                issued = advance(d + 1)
                assert s.target(d + 1, issued, everything=True) == U
            assert issued == U, case
            # contiguous, non-empty, at most a chunk long, [0, U) exactly once
            assert pieces[0][0] == 0 and pieces[-1][1] == U, case
            assert all(a[1] == b[0] for a, b in zip(pieces, pieces[1:])), case
            assert all(0 < hi - lo <= chunk for lo, hi in pieces), case


# ---- MergePump's bookkeeping ---------------------------------------------------------------------------------------------
class _Stream:
    def __init__(self):
        self.waited = []

    def wait_event(self, ev):
        self.waited.append(ev)


class _Engine:
    """What MergePump reads of a TrainEngine between start() and the merge's last wait."""
    dev = "cpu"

    def __init__(self, chunk):
        self.agg_chunk_rows = chunk
        self.side = _Stream()
        self.comm = S.new_stream("cpu")


class _Piece:
    """The event behind a recorded piece."""
    def __init__(self, hi):
        self.hi = hi


def _recording(chunk):
    eng = _Engine(chunk)
    pump = MergePump(eng)
    calls = []

    def issue(lo, hi):
        calls.append((lo, hi))
        return _Piece(hi)
    pump.issue = issue
    return eng, pump, calls


RS, J0, STEP0 = object(), 5, 100


def _start(pump, sched):
    pump.start(sched, None, None, 1.0, None, S.new_event("cpu"), RS, J0, STEP0)


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("U,K,budget,chunk", [(1, 1, 1, 1), (9, 4, 1, 4), (100, 8, 8, 8), (100, 33, 4, 105), (1000, 16, 8, 8)])
def test_pump_issues_the_schedules_pieces_and_waits_for_the_chunk_a_step_needs(pattern, U, K, budget, chunk):
    sched = MergeSchedule(offsets(U, pattern), K, U, budget)
    eng, pump, calls = _recording(chunk)
    assert not pump.pending
    _start(pump, sched)
    want = merge_pieces(0, sched.target(1, 0), chunk)
    assert calls == want and pump.pending and pump.issued == want[-1][1] and pump.waited == 0
    waited = 0
    for d in range(1, K + 3):
        it = STEP0 + d
        chunks, need = list(pump.chunks), sched.need(d)
        assert [hi for hi, _ in chunks] == [hi for _, hi in want]
        n_before = len(eng.side.waited)
        pump.before_step((RS, J0 + d), it)
        assert calls == want, "the expected next batch of the merge's window must not drain it"
        if need > waited:
            first = next(ev for hi, ev in chunks if hi >= need)
            assert eng.side.waited[n_before:] == [first]
            waited = first.hi
        else:
            assert eng.side.waited[n_before:] == []
        assert pump.pending == (waited < U), (d, waited)
        if not pump.pending:
            break
        assert pump.waited == waited
        want += merge_pieces(pump.issued, sched.target(d + 1, pump.issued), chunk)
        pump.after_step(it)
        assert calls == want and pump.issued == want[-1][1]
    assert not pump.pending and want[-1][1] == U and d <= K + 1
    assert (pump.issued, pump.waited, pump.chunks, pump.sched) == (0, 0, [], None)
    pump.after_step(STEP0 + d)          # idle: nothing
    assert calls == want


@pytest.mark.parametrize("pos", [None, (object(), J0 + 1), (RS, J0 + 2), (RS, J0)])
def test_a_step_that_is_not_the_expected_next_batch_gets_the_whole_merge_first(pos):
    sched = MergeSchedule(offsets(100, "spread"), 16, 100, 4)
    eng, pump, calls = _recording(8)
    _start(pump, sched)
    assert pump.pending and pump.issued < 100
    pump.before_step(pos, STEP0 + 1)
    assert not pump.pending
    assert calls == merge_pieces(0, sched.target(1, 0), 8) + merge_pieces(sched.target(1, 0), 100, 8)
    assert eng.side.waited[-1].hi == 100


def test_an_idle_pump_has_nothing_to_drain():
    eng, pump, calls = _recording(8)
    pump.drain()
    pump.before_step((RS, J0), STEP0)
    pump.after_step(STEP0)
    assert calls == [] and eng.side.waited == [] and not pump.pending
