"""The kernels that move cache rows by an index list outside the training step, against numpy at their edges.

    multi-rank touched-row merge   cdlrm_mark_rows, cdlrm_agg_compact, cdlrm_agg_mark_tier, cdlrm_agg_split,
                                   cdlrm_agg_gather, cdlrm_agg_scatter                    (csrc/window.hip, csrc/scan.hip)
    drop-in row helpers            cdlrm_gather_rows, cdlrm_scatter_rows, cdlrm_blend_rows                (csrc/window.hip)
    victim write-back              cdlrm_victim_writeback                                                 (csrc/embbag.hip)

tests/row_merge_restated.py holds each contract as plain numpy, the inputs and the comparators.  Everything goes through
the cdlrm_amd.ops wrappers the engine uses and is compared bit for bit: these kernels copy, sort, divide once or
add-and-halve once.  Every output buffer starts as a sentinel bit pattern with PAD more elements behind it, and what the
contract does not write has to come back unchanged; inputs have to come back unchanged; every test ends on ctx.check().

Which size reaches which path:

    mark_rows / agg_mark_tier   n = 262145: one more than 1024 blocks x 256 threads, the grid-stride trip
    agg_compact                 8231 flags: three 4096-flag blocks, a 7-byte tail behind the last whole 16-byte group
    agg_split                   1024 list entries per block; 131073 entries x 8 classes = 129 blocks, 1032 scanned counters:
                                k_scan_tops makes a second trip with a carry
    agg_gather / agg_scatter    32769 rows x 32 float4 > 4096 blocks x 256 threads: the grid-stride trip; D = 12: D4 = 3
    victim write-back           2500 positions, > 2048 misses: a wave takes a second miss; D = 512: two column trips

The unmarked tests run anywhere: the inputs hold the edges they are meant to hold, and the comparators reject an unstable
split, shifted class offsets, a reciprocal multiply for the division, first-occurrence-wins and a repeated blend."""
import numpy as np
import pytest
import torch

import row_merge_restated as R
from row_merge_restated import PAD, same_bits, sentinel

gpu = pytest.mark.gpu
DEV = "cuda:0"


def ids(values, fmt="%s"):
    return [fmt % v for v in values]


# ---- on any machine: the inputs hold their edges -------------------------------------------------------------------

def test_fixture_holds_every_edge():
    geo = R.GEO_FLAGS
    total = geo.total_rows
    assert geo.rows == [4089, 17, 4125] and total == 8231
    assert total > 2 * R.FLAG_BLOCK and total % R.FLAG_GROUP != 0, "three flag blocks and a byte-wise tail"
    # mark_rows: every special slot value in every list that has room, repeats, and a last entry of its own
    for n in R.MARK_N:
        s = R.mark_slots(n)
        assert s.shape == (geo.T, n)
        for t in range(geo.T):
            if n >= 5:
                for v in R.mark_specials(geo, t):
                    assert v in s[t], (n, t, v)
                assert np.count_nonzero(s[t] == s[t, -1]) == 1 and 0 <= s[t, -1] < geo.rows[t]
                assert np.unique(s[t]).size < n, "repeats"
        assert R.mark_rows_ref(geo, s, np.zeros(total, np.uint8)).any(), n
    assert max(R.MARK_N) == 1024 * 256 + 1
    # agg_compact: a flag on each side of every block boundary, a full 16-byte group, a full block, odd byte values
    edges = R.compact_flags("block-edges")
    for b in range(R.FLAG_BLOCK, total, R.FLAG_BLOCK):
        assert edges[b - 1] and edges[b]
    assert np.flatnonzero(edges).size == 4
    for name, at in zip(R.COMPACT_SINGLES, (0, 15, 16, 4095, 4096, 4097, total - 2, total - 1)):
        assert np.flatnonzero(R.compact_flags("one@" + name)).tolist() == [at]
    g = np.flatnonzero(R.compact_flags("group16"))
    assert g.size == 16 and g[0] % R.FLAG_GROUP == 0 and g[-1] == g[0] + 15
    assert np.flatnonzero(R.compact_flags("block")).tolist() == list(range(4096, 8192))
    assert R.compact_flags("all").all() and not R.compact_flags("empty").any()
    r3 = R.compact_flags("random3")
    assert 0.02 * total < np.count_nonzero(r3) < 0.04 * total and r3[total - total % 16:].size == 7
    assert set(np.unique(R.compact_flags("random3-bytes")).tolist()) == {0, 1, 2, 128, 255}
    # agg_mark_tier: cache slots, aux slots, negatives, repeats; a row two batches name, a row all three name
    for n in R.TIER_N:
        named = []
        for s in R.tier_batches(n):
            assert s.shape == (geo.T, n) and not (s == R.TIER_PAD_SLOT).any()
            named.append(R.mark_tier_ref(geo, s, 0, np.ones(total, np.uint8)) == 0)
            if n >= 256:
                for t in range(geo.T):
                    assert (s[t] < 0).any() and (s[t] >= geo.first_aux[t]).any() and (s[t] == geo.first_aux[t] - 1).any()
                    assert np.unique(s[t]).size < n
        assert (named[0] & named[1] & named[2]).any(), n
        if n >= 256:
            assert (named[0] & named[1] & ~named[2]).any() and (named[0] & ~named[1] & ~named[2]).any()
    # agg_split: every class empty somewhere, a tier byte >= C, all four elements of a thread in different classes
    assert R.GEO_SPLIT.total_rows >= 140000
    assert -(-131073 // R.SPLIT_BLOCK) == 129 and 129 * 8 > 1024
    for C in R.SPLIT_CLASSES:
        rows = R.split_rows(1025)
        counts = {p: np.bincount(np.minimum(R.split_tier(1025, C, p)[rows], C - 1), minlength=C) for p in R.split_patterns(C)}
        for c in range(C):
            assert counts["single%d" % c][c] == 1025
            if C > 1:
                assert any(cnt[c] == 0 for cnt in counts.values()), (C, c)
        if C >= 3:
            cnt = counts["empty-middle"]
            assert cnt[C // 2] == 0 and cnt[C // 2 - 1] > 0 and cnt[C // 2 + 1] > 0
        raw = R.split_tier(1025, C, "clamp")[rows]
        assert (raw >= C).any() and (raw == 255).any() and (raw == C).any()
        assert counts["skewed-cold"][C - 1] > 0.8 * 1025
    cyc = R.split_tier(4097, 8, "cycle")[R.split_rows(4097)]
    assert all(len(set(cyc[i:i + 4].tolist())) == 4 for i in range(0, 4096, 4))
    for count in R.SPLIT_COUNTS:
        rows = R.split_rows(count)
        assert rows.size == count and (np.diff(rows) > 0).all()
    # chunked gather / scatter: a chunk that straddles the count word, a chunk wholly beyond it
    straddle = beyond = 0
    for size in R.AGG_CHUNKS:
        for count in R.AGG_COUNT_WORDS.values():
            for lo, hi in R.chunks(R.AGG_U, size):
                straddle += lo < count < hi
                beyond += count - lo < 0
    assert straddle > 0 and beyond > 0
    assert R.AGG_BIG * (128 // 4) > 4096 * 256 and R.AGG_BIG <= R.geo_agg(128).total_rows
    w = R.plant_specials(R.any_bits_weight(64, 4).copy(), np.arange(10, 20))
    assert set(R.SPECIALS32.tolist()) <= set(R.bits(w[10:20]).reshape(-1).tolist())
    for scale in (2.0, 3.0, 7.0):
        q = np.abs(R.divided(R.normal_weight(1000, 12), scale))
        assert np.isfinite(q).all() and (q >= np.finfo(np.float32).tiny).all()
    # row helpers: the ends of the table, a doubled and a tripled row
    for count in R.ROW_COUNTS + (R.ROW_BIG,):
        n = R.row_table_rows(count)
        for order in R.ROW_ORDERS:
            idx = R.row_index(count, order)
            assert idx.size == count == np.unique(idx).size and (count == 0 or (0 <= idx.min() and idx.max() < n))
        if count >= 2:
            assert {0, n - 1} <= set(R.row_index(count, "ends").tolist())
            assert (np.diff(R.row_index(count, "sorted")) > 0).all() and (np.diff(R.row_index(count, "permuted")) < 0).any()
        if count >= 6:
            idx, src = R.row_index_repeats(count)
            assert sorted(np.bincount(idx)[np.bincount(idx) > 1].tolist()) == [2, 3] and (idx == idx[src]).all()
    # victim write-back: > 2048 misses, hits interleaved, the miss distances, first and last miss alike, 64 and 65 misses
    for phase in (0, 1):
        for shape, (n, n_miss) in R.VWB_SHAPES.items():
            idx, slots, miss = R.vwb_batch(shape, phase)
            g4 = R.geo_vwb(4)
            for t in range(g4.T):
                M = int(miss[t].sum())
                mi = idx[t][miss[t]]
                assert mi[0] == mi[-1] and miss[t, 0] and miss[t, -1] and not miss[t].all()
                first = g4.first_aux[t] + phase * g4.aux
                assert slots[t][miss[t]].tolist() == list(range(first, first + M)) and (slots[t][~miss[t]] < g4.first_aux[t]).all()
                assert (slots[t] >= 0).all() and slots[t].max() < g4.rows[t] and idx[t].max() < g4.table_rows[t]
                if n_miss is None:
                    assert M > 2048 and 0.05 * n < n - M < 0.15 * n
                    assert set(R.VWB_DISTANCES) <= R.miss_distances(idx[t], miss[t])
                else:
                    assert M == n_miss and (n_miss - 1) in R.miss_distances(idx[t], miss[t])
                assert np.isin(idx[t][~miss[t]], mi).any() and not np.isin(idx[t][~miss[t]], mi).all()
            v_idx, v_off = R.vwb_victims(shape, phase)
            wsrc = R.vwb_wsrc(shape, phase)
            for t in range(g4.T):
                v = v_idx[v_off[t]:v_off[t + 1]]
                mi = idx[t][miss[t]]
                assert (np.diff(v) > 0).all() and np.isin(mi, v).any() and not np.isin(mi, v).all() and not np.isin(v, mi).all()
                assert (wsrc[t][miss[t]] >= 0).any() and (wsrc[t][miss[t]] < 0).any()
                assert (np.isin(mi, v) & (wsrc[t][miss[t]] < 0)).any(), "a listed index whose wsrc says -1"
    assert R.geo_vwb(512).D // 4 > 64


# ---- on any machine: the comparators reject the plausible wrong answers ------------------------------------------------

def split_outputs(count, C, pattern):
    rows, tier = R.split_rows(count), R.split_tier(count, C, pattern)
    out, off = R.split_ref(rows, count, tier, C)
    got_rows, got_off = sentinel(count + PAD, np.int64), sentinel(C + 1 + PAD, np.int64)
    got_rows[:count], got_off[:C + 1] = out, off
    return rows, tier, got_rows, got_off


@pytest.mark.parametrize("pattern", ["cycle", "skewed-cold", "clamp"])
def test_comparator_rejects_unstable_split(pattern):
    C, count = 8, 4097
    rows, tier, got_rows, got_off = split_outputs(count, C, pattern)
    R.check_split(rows, count, tier, C, got_rows, got_off)
    cls = np.minimum(tier[got_rows[:count]], C - 1)
    i = int(np.flatnonzero(cls[:-1] == cls[1:])[0])
    got_rows[[i, i + 1]] = got_rows[[i + 1, i]]                  # two rows of one class swapped: still grouped by class
    with pytest.raises(AssertionError):
        R.check_split(rows, count, tier, C, got_rows, got_off)


@pytest.mark.parametrize("C", [2, 8])
def test_comparator_rejects_shifted_class_off(C):
    count = 1025
    rows, tier, got_rows, got_off = split_outputs(count, C, "cycle")
    got_off[1] += 1
    with pytest.raises(AssertionError):
        R.check_split(rows, count, tier, C, got_rows, got_off)
    rows, tier, got_rows, got_off = split_outputs(count, C, "cycle")
    got_rows[count] = got_rows[count - 1]                        # one entry written behind the list
    with pytest.raises(AssertionError):
        R.check_split(rows, count, tier, C, got_rows, got_off)


@pytest.mark.parametrize("scale", [3.0, 7.0])
@pytest.mark.parametrize("D", R.AGG_DIMS)
def test_comparator_rejects_reciprocal_multiply(D, scale):
    geo = R.geo_agg(D)
    rows = R.sorted_subset(geo.total_rows, R.AGG_U, 57)
    w = R.normal_weight(geo.total_rows, D)[rows]
    wrong = w * np.float32(1 / scale)
    n_diff = int((R.bits(wrong) != R.bits(R.divided(w, scale))).sum())
    print("D", D, "scale", scale, "elements where multiply and divide differ:", n_diff, "of", w.size)
    assert n_diff >= 1
    with pytest.raises(AssertionError):
        same_bits(wrong, R.divided(w, scale), "w / scale")
    same_bits(w * np.float32(0.5), R.divided(w, 2.0), "w / 2 is exact either way")


@pytest.mark.parametrize("shape", list(R.VWB_SHAPES))
def test_comparator_rejects_first_occurrence_wins(shape):
    geo = R.geo_vwb(4)
    idx, slots, _ = R.vwb_batch(shape, 1)
    victims = R.vwb_victims(shape, 1)
    weight = R.any_bits_weight(geo.total_rows, 4)
    host = [R.any_bits_weight(n, 4, seed=81 + t) for t, n in enumerate(geo.table_rows)]
    v_rows = R.any_bits_weight(int(victims[1][-1]) + 4, 4, seed=85)
    want_h, want_v = R.vwb_ref(geo, idx, slots, 1, weight, host, victims=victims, v_rows=v_rows)
    got_h, got_v = R.vwb_ref(geo, idx, slots, 1, weight, host, victims=victims, v_rows=v_rows, first_wins=True)
    for t in range(geo.T):
        with pytest.raises(AssertionError):
            same_bits(got_h[t], want_h[t], "host table")
    assert (R.bits(got_v) != R.bits(want_v)).any()


@pytest.mark.parametrize("D", R.ROW_DIMS)
def test_comparator_rejects_repeated_blend(D):
    count = 64
    idx, src = R.row_index_repeats(count)
    dst = R.normal_weight(R.row_table_rows(count), D, seed=91)
    v = R.normal_weight(count, D, seed=93)[src]
    want = R.scatter_rows_ref(dst, idx, v, average=True, distinct=False)
    wrong = R.scatter_rows_blend_per_entry(dst, idx, v)
    once = np.setdiff1d(idx, idx[src != np.arange(count)])
    same_bits(wrong[once], want[once], "rows listed once")
    with pytest.raises(AssertionError):
        same_bits(wrong, want, "blended rows")


# ---- device side ------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def ops():
    from cdlrm_amd import ops as _ops
    from cdlrm_amd import _lib
    _lib.lib()
    yield _ops
    _CTX.clear()
    _DEVICE_COPIES.clear()


_CTX, _DEVICE_COPIES = {}, {}


def dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)


def host(t):
    return t.cpu().numpy()


def new_ctx(ops, geo):
    return ops.CacheCtx(geo.table_rows, geo.sets, geo.D, geo.ways, geo.aux, torch.device(DEV), aux_phases=geo.aux_phases)


def ctx_for(ops, geo):
    """One library context per geometry for the module (every test leaves its error word clear)."""
    key = (tuple(geo.sets), geo.ways, geo.aux, geo.D, geo.aux_phases)
    if key not in _CTX:
        _CTX[key] = new_ctx(ops, geo)
    return _CTX[key]


def pristine(key, make):
    """A device copy of an input that several cases start from; callers clone it."""
    if key not in _DEVICE_COPIES:
        _DEVICE_COPIES[key] = dev(make())
    return _DEVICE_COPIES[key].clone()


def bind_weight(ctx, geo, d_weight):
    ctx.bind_cache(torch.full((geo.total_tags,), -1, dtype=torch.int64, device=DEV), d_weight)


def padded(a, dtype=None):
    """`a` with PAD sentinel elements (rows, for a matrix) behind it."""
    a = np.asarray(a)
    out = sentinel((a.shape[0] + PAD,) + a.shape[1:], dtype or a.dtype)
    out[:a.shape[0]] = a
    return out


# ---- 1. flags to list ----------------------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("n", R.MARK_N, ids=ids(R.MARK_N, "n%d"))
def test_mark_rows(ops, n):
    geo = R.GEO_FLAGS
    ctx, total = ctx_for(ops, geo), geo.total_rows
    slots = R.mark_slots(n)
    before = sentinel(total + PAD, np.uint8)
    d_slots, d_touched = dev(slots), dev(before)
    ops.mark_rows(ctx, d_slots, d_touched[:total])
    want = before.copy()
    want[:total] = R.mark_rows_ref(geo, slots, before[:total])
    same_bits(host(d_touched), want, "touched")
    same_bits(host(d_slots), slots, "slots")
    for t in range(geo.T):                                   # one table's slots alone: no byte of another table changes
        only = np.full_like(slots, -1)
        only[t] = slots[t]
        d_touched = dev(before)
        ops.mark_rows(ctx, dev(only), d_touched[:total])
        got = host(d_touched)
        same_bits(got[geo.row_base[t]:geo.row_base[t + 1]], want[geo.row_base[t]:geo.row_base[t + 1]], "table %d" % t)
        got[geo.row_base[t]:geo.row_base[t + 1]] = R.SENT8
        same_bits(got, before, "the other tables, with table %d marked" % t)
    ctx.check()


def run_compact(ops, ctx, flags, cap):
    total = flags.size
    d_flags, d_rows, d_count = dev(padded(flags)), dev(sentinel(cap + PAD, np.int64)), dev(sentinel(1 + PAD, np.int64))
    ops.agg_compact(ctx, d_flags[:total], d_rows[:cap], d_count[:1])
    count = host(d_count)
    same_bits(count[1:], sentinel(PAD, np.int64), "behind count_out")
    R.check_compact(flags, cap, host(d_rows), count[0], host(d_flags))


@gpu
@pytest.mark.parametrize("name", R.COMPACT_PATTERNS)
def test_agg_compact(ops, name):
    ctx = ctx_for(ops, R.GEO_FLAGS)
    flags = R.compact_flags(name)
    run_compact(ops, ctx, flags, flags.size)
    ctx.check()


@gpu
@pytest.mark.parametrize("name", ["random3", "all", "block-edges"])
def test_agg_compact_overflow_drops_and_reports(ops, name):
    """cap = count - 1 (csrc/scan.h): the first cap entries are right, the one beyond is dropped, count_out keeps the true
    count and the error word gets bit 4, which CacheCtx.check raises once; the next clean call passes."""
    from cdlrm_amd._lib import CdlrmError
    ctx = new_ctx(ops, R.GEO_FLAGS)
    flags = R.compact_flags(name)
    run_compact(ops, ctx, flags, np.count_nonzero(flags) - 1)
    with pytest.raises(CdlrmError) as e:
        ctx.check()
    assert "device error word = 4 " in str(e.value), str(e.value)
    ctx.check()                                              # (the word was cleared by the check that reported it)
    run_compact(ops, ctx, flags, np.count_nonzero(flags))
    ctx.check()


# ---- 2. deadline classes -------------------------------------------------------------------------------------------------

def mark_tiers(ops, ctx, geo, batches, d_tier):
    """The engine's order: tier.fill_(C - 1), then class by class from the latest deadline to the earliest.  The slots
    are column slices of a wider buffer, as the window's resolved slots are.  Returns the restated tier bytes."""
    C, total = R.TIER_CLASSES, geo.total_rows
    d_tier[:total].fill_(C - 1)
    want = np.full(total, C - 1, dtype=np.uint8)
    for value, s in zip(reversed(range(C - 1)), batches):
        n = s.shape[1]
        wide = np.full((geo.T, n + 5), R.TIER_PAD_SLOT, dtype=np.int32)
        wide[:, 2:2 + n] = s
        d_wide = dev(wide)
        view = d_wide[:, 2:2 + n]
        assert view.stride(0) > n
        ops.agg_mark_tier(ctx, view, value, d_tier[:total])
        want = R.mark_tier_ref(geo, s, value, want)
        same_bits(host(d_wide), wide, "slots")
    return want


@gpu
@pytest.mark.parametrize("n", R.TIER_N, ids=ids(R.TIER_N, "n%d"))
def test_agg_mark_tier(ops, n):
    geo = R.GEO_FLAGS
    ctx, total, C = ctx_for(ops, geo), geo.total_rows, R.TIER_CLASSES
    d_tier = dev(sentinel(total + PAD, np.uint8))
    want = mark_tiers(ops, ctx, geo, R.tier_batches(n), d_tier)
    got = host(d_tier)
    same_bits(got[:total], want, "tier")
    same_bits(got[total:], sentinel(PAD, np.uint8), "behind the tier bytes")
    for t in range(geo.T):
        assert got[geo.row_base[t] + 2] == 0, "the earliest class wins on a row all batches name"
        assert (got[geo.row_base[t] + geo.first_aux[t]:geo.row_base[t + 1]] == C - 1).all(), "aux rows stay cold"
        assert got[geo.row_base[t] + R.TIER_PAD_SLOT] == C - 1, "nothing outside the [T, n] view is read"
    if n >= 256:
        named = [R.mark_tier_ref(geo, s, 0, np.ones(total, np.uint8)) == 0 for s in R.tier_batches(n)]
        assert (got[:total][named[0] & named[1] & ~named[2]] == 1).all(), "class 1 wins over class 2"
    ctx.check()


# ---- 3. stable split -----------------------------------------------------------------------------------------------------

def run_split(ops, ctx, count, C, pattern):
    geo = R.GEO_SPLIT
    rows, tier = R.split_rows(count), R.split_tier(count, C, pattern)
    rows_in = np.full(count + PAD, geo.total_rows - 1, dtype=np.int64)     # behind the list: a valid row, never to be read
    rows_in[:count] = rows
    d_rows, d_tier = dev(rows_in), dev(padded(tier))
    d_out, d_off = dev(sentinel(count + PAD, np.int64)), dev(sentinel(C + 1 + PAD, np.int64))
    ops.agg_split(ctx, d_rows, count, d_tier[:geo.total_rows], C, d_out, d_off)
    got_rows, got_off = host(d_out), host(d_off)
    R.check_split(rows, count, tier, C, got_rows, got_off)
    same_bits(host(d_rows), rows_in, "rows")
    same_bits(host(d_tier), padded(tier), "tier")
    return got_rows, got_off


@gpu
@pytest.mark.parametrize("count", R.SPLIT_COUNTS, ids=ids(R.SPLIT_COUNTS, "count%d"))
@pytest.mark.parametrize("C,pattern", R.SPLIT_CASES, ids=["C%d-%s" % cp for cp in R.SPLIT_CASES])
def test_agg_split(ops, C, pattern, count):
    ctx = ctx_for(ops, R.GEO_SPLIT)
    got_rows, got_off = run_split(ops, ctx, count, C, pattern)
    if count == 0:
        assert not got_off[:C + 1].any()
        same_bits(got_rows, sentinel(PAD, np.int64), "rows_out of an empty list")
    assert got_off[C] == count
    ctx.check()


@gpu
def test_agg_split_twice_with_growing_scratch(ops):
    """One context's merge scratch from small to large, with a compaction between the splits: a small split, a compaction
    (grows it), the largest split (grows it again), a compaction (reuses it), the largest split once more."""
    ctx = new_ctx(ops, R.GEO_SPLIT)
    flags = R.compact_flags("random3", R.GEO_SPLIT.total_rows)
    run_split(ops, ctx, 3, 8, "cycle")
    run_compact(ops, ctx, flags, flags.size)
    a = run_split(ops, ctx, 131073, 8, "cycle")
    run_compact(ops, ctx, flags, flags.size)
    b = run_split(ops, ctx, 131073, 8, "cycle")
    same_bits(a[0], b[0], "rows_out of the two runs")
    same_bits(a[1], b[1], "class_off of the two runs")
    ctx.check()


# ---- 4. chunked gather / scatter -----------------------------------------------------------------------------------------

def agg_weight(geo, rows, scale):
    """Device weight for a gather at `scale`: arbitrary bits with the special values planted at scale 1, normal-range
    values where the kernel divides."""
    D, n = geo.D, geo.total_rows
    if scale == 1.0:
        return pristine(("bits", n, D, rows.size), lambda: R.plant_specials(R.any_bits_weight(n, D).copy(), rows))
    return pristine(("normal", n, D), lambda: R.normal_weight(n, D))


def run_gather_scatter(ops, ctx, geo, U, chunk_list, count, scales):
    D = geo.D
    rows = R.sorted_subset(geo.total_rows, U, 57)
    rows_in = np.full(U + PAD, geo.total_rows - 1, dtype=np.int64)
    rows_in[:U] = rows
    d_rows, d_count = dev(rows_in), dev(np.array([count], dtype=np.int64))
    m = min(count, U)
    for scale in scales:
        d_w = agg_weight(geo, rows, scale)
        w = host(d_w)
        bind_weight(ctx, geo, d_w)
        buf = sentinel((U + PAD, D), np.float32)
        d_buf = dev(buf)
        for lo, hi in chunk_list:
            ops.agg_gather(ctx, d_rows[lo:], d_count, scale, d_buf[lo:hi], hi - lo, first=lo)
            R.agg_gather_ref(w, rows[lo:], count, scale, buf[lo:hi], hi - lo, lo)
        same_bits(buf[:m], R.divided(w[rows[:m]], scale), "the restated chunks add up to the list's first rows")
        same_bits(buf[m:], sentinel((U + PAD - m, D), np.float32), "the restated chunks move nothing else")
        same_bits(host(d_buf), buf, "buf at scale %g" % scale)
        same_bits(host(d_w), w, "weight behind a gather")
        if scale == 1.0:
            for lo, hi in chunk_list:
                ops.agg_scatter(ctx, d_rows[lo:], d_count, d_buf[lo:hi], hi - lo, first=lo)
            same_bits(host(d_w), w, "gather at scale 1, then scatter")
            other = R.any_bits_weight(U, D, seed=59)
            d_other = dev(other)
            want = w.copy()
            for lo, hi in chunk_list:
                ops.agg_scatter(ctx, d_rows[lo:], d_count, d_other[lo:hi], hi - lo, first=lo)
                R.agg_scatter_ref(want, rows[lo:], count, other[lo:hi], hi - lo, lo)
            same_bits(host(d_w), want, "weight behind a scatter")
            same_bits(host(d_other), other, "buf behind a scatter")
            unlisted = np.setdiff1d(np.arange(geo.total_rows), rows[:m])
            same_bits(want[unlisted], w[unlisted], "rows the list does not name")
    same_bits(host(d_rows), rows_in, "rows")
    same_bits(host(d_count), np.array([count], dtype=np.int64), "count")


@gpu
@pytest.mark.parametrize("cw", list(R.AGG_COUNT_WORDS), ids=["count=" + k for k in R.AGG_COUNT_WORDS])
@pytest.mark.parametrize("chunk", R.AGG_CHUNKS, ids=ids(R.AGG_CHUNKS, "chunk%d"))
@pytest.mark.parametrize("D", R.AGG_DIMS, ids=ids(R.AGG_DIMS, "D%d"))
@pytest.mark.parametrize("scale", R.AGG_SCALES, ids=ids(R.AGG_SCALES, "scale%g"))
def test_agg_gather_scatter_chunks(ops, scale, D, chunk, cw):
    """Scale 1 copies bits (and is followed by the scatters); 2, 3 and 7 divide."""
    geo = R.geo_agg(D)
    ctx = ctx_for(ops, geo)
    run_gather_scatter(ops, ctx, geo, R.AGG_U, R.chunks(R.AGG_U, chunk), R.AGG_COUNT_WORDS[cw], [scale])
    ctx.check()


@gpu
@pytest.mark.parametrize("scale", [1.0, 3.0], ids=["scale1", "scale3"])
def test_agg_gather_scatter_one_chunk_of_32769_rows(ops, scale):
    geo = R.geo_agg(128)
    ctx = ctx_for(ops, geo)
    run_gather_scatter(ops, ctx, geo, R.AGG_BIG, [(0, R.AGG_BIG)], R.AGG_BIG, [scale])
    ctx.check()


@gpu
def test_two_rank_merge_in_class_order_equals_one_piece(ops):
    """Two contexts of one geometry stand for two ranks: three steps of mark_rows, the flags' maximum for their all-reduce,
    agg_compact, agg_mark_tier, agg_split, then the rows exchanged in class order in chunks of 8 with buf_a + buf_b for the
    all-reduce.  Every touched row of both ends as fp32 wa / 2 + wb / 2, nothing else changes, and the one-piece merge of
    the same rows gives the same bits."""
    geo = R.GEO_FLAGS
    total, D, C = geo.total_rows, geo.D, R.TIER_CLASSES
    w0 = [R.normal_weight(total, D, seed=101), R.normal_weight(total, D, seed=103)]
    ctxs = [new_ctx(ops, geo), new_ctx(ops, geo)]
    d_w = [dev(w) for w in w0]
    for ctx, dw in zip(ctxs, d_w):
        bind_weight(ctx, geo, dw)
    d_touched = [torch.zeros(total, dtype=torch.uint8, device=DEV) for _ in ctxs]
    flags = np.zeros(total, dtype=np.uint8)
    for step in range(3):
        for r, ctx in enumerate(ctxs):
            s = R.mark_slots(255, seed=200 + 10 * step + r)
            ops.mark_rows(ctx, dev(s), d_touched[r])
            flags = R.mark_rows_ref(geo, s, flags)
    both = torch.maximum(d_touched[0], d_touched[1])
    same_bits(host(both), flags, "touched flags of both ranks")
    touched_rows = np.flatnonzero(flags).astype(np.int64)
    U = touched_rows.size
    assert (flags[geo.row_base[1] - geo.aux:geo.row_base[1]] != 0).any(), "an aux row is merged too"
    d_list, d_count, d_sorted, offs = [], [], [], []
    for r, ctx in enumerate(ctxs):
        d_touched[r].copy_(both)
        d_list.append(dev(sentinel(total, np.int64)))
        d_count.append(dev(sentinel(1, np.int64)))
        ops.agg_compact(ctx, d_touched[r], d_list[r], d_count[r])
        assert int(d_count[r]) == U
        same_bits(host(d_list[r])[:U], touched_rows, "row list of rank %d" % r)
        d_tier = dev(sentinel(total + PAD, np.uint8))
        tier = mark_tiers(ops, ctx, geo, R.tier_batches(256), d_tier)
        d_sorted.append(dev(sentinel(U + PAD, np.int64)))
        d_off = dev(sentinel(C + 1 + PAD, np.int64))
        ops.agg_split(ctx, d_list[r], U, d_tier[:total], C, d_sorted[r], d_off)
        R.check_split(touched_rows, U, tier, C, host(d_sorted[r]), host(d_off))
        offs.append(host(d_off)[:C + 1].tolist())
    assert offs[0] == offs[1] and all(offs[0][c] < offs[0][c + 1] for c in range(C)), offs
    d_buf = [dev(sentinel((U, D), np.float32)) for _ in ctxs]
    for c in range(C):
        for lo in range(offs[0][c], offs[0][c + 1], 8):
            hi = min(lo + 8, offs[0][c + 1])
            for r, ctx in enumerate(ctxs):
                ops.agg_gather(ctx, d_sorted[r][lo:], d_count[r], 2.0, d_buf[r][lo:hi], hi - lo, first=lo)
            d_buf[0][lo:hi] += d_buf[1][lo:hi]
            d_buf[1][lo:hi] = d_buf[0][lo:hi]
            for r, ctx in enumerate(ctxs):
                ops.agg_scatter(ctx, d_sorted[r][lo:], d_count[r], d_buf[r][lo:hi], hi - lo, first=lo)
    want = [w.copy() for w in w0]
    for w in want:
        w[touched_rows] = R.mean2(w0[0][touched_rows], w0[1][touched_rows])
    piecewise = [host(dw) for dw in d_w]
    for r in range(2):
        same_bits(piecewise[r], want[r], "weight of rank %d" % r)
    same_bits(piecewise[0][touched_rows], piecewise[1][touched_rows], "the ranks' merged rows")
    # the same merge in one piece, on the unsorted list
    d_w1 = [dev(w) for w in w0]
    d_buf = [dev(sentinel((U, D), np.float32)) for _ in ctxs]
    for r, ctx in enumerate(ctxs):
        bind_weight(ctx, geo, d_w1[r])
        ops.agg_gather(ctx, d_list[r], d_count[r], 2.0, d_buf[r], U)
    total_buf = d_buf[0] + d_buf[1]
    for r, ctx in enumerate(ctxs):
        ops.agg_scatter(ctx, d_list[r], d_count[r], total_buf, U)
        same_bits(host(d_w1[r]), piecewise[r], "one-piece merge of rank %d" % r)
    for ctx in ctxs:
        ctx.check()


# ---- 5. row helpers ------------------------------------------------------------------------------------------------------

ROW_CASES = [(D, c) for D in R.ROW_DIMS for c in R.ROW_COUNTS] + [(128, R.ROW_BIG)]
ROW_CASE_IDS = ["D%d-count%d" % dc for dc in ROW_CASES]


def row_table(kind, count, D, seed):
    make = R.any_bits_weight if kind == "bits" else R.normal_weight
    n = R.row_table_rows(count)
    return pristine((kind, n, D, seed), lambda: make(n, D, seed=seed))


@gpu
@pytest.mark.parametrize("order", R.ROW_ORDERS)
@pytest.mark.parametrize("D,count", ROW_CASES, ids=ROW_CASE_IDS)
def test_gather_and_scatter_rows(ops, D, count, order):
    """count 0: an empty list's tensors have no address (data_ptr() is 0), and the helpers have to return before they
    look at a pointer -- they used to refuse the call as a bad argument."""
    idx = R.row_index(count, order)
    d_idx = dev(idx)
    d_table = row_table("bits", count, D, 111)
    table = host(d_table)
    out = ops.gather_rows(d_table.data_ptr(), d_idx, D)
    assert tuple(out.shape) == (count, D)
    same_bits(host(out), table[idx], "gathered rows")
    same_bits(host(d_table), table, "table behind a gather")
    v = R.any_bits_weight(count, D, seed=113)
    d_v = dev(v)
    ops.scatter_rows(d_table.data_ptr(), d_idx, d_v, average=False)
    want = R.scatter_rows_ref(table, idx, v, average=False)
    same_bits(host(d_table), want, "table behind a scatter")
    unlisted = np.setdiff1d(np.arange(table.shape[0]), idx)
    same_bits(want[unlisted], table[unlisted], "rows the list does not name")
    # the mean with the old row, a distinct list; one pair overflows to inf
    d_table = row_table("normal", count, D, 115)
    v = R.normal_weight(count, D, seed=117).copy()
    if count:
        big = np.float32(3e38)
        d_table[int(idx[0]), D - 1] = float(big)
        v[0, D - 1] = big
    table, d_v = host(d_table), dev(v)
    ops.scatter_rows(d_table.data_ptr(), d_idx, d_v, average=True, distinct=True)
    want = R.scatter_rows_ref(table, idx, v, average=True)
    if count:
        assert np.isposinf(want[idx[0], D - 1])
    same_bits(host(d_table), want, "table behind an averaging scatter")
    same_bits(host(d_v), v, "rows")
    same_bits(host(d_idx), idx, "index")
    torch.cuda.synchronize()


@gpu
@pytest.mark.parametrize("D,count", ROW_CASES, ids=ROW_CASE_IDS)
def test_scatter_rows_average_with_repeats_blends_once(ops, D, count):
    """average=True, distinct=False (cdlrm_blend_rows, then the plain scatter): a row listed two or three times, each time
    with the same new row, ends as (old + new) / 2 -- once."""
    if count >= 6:
        idx, src = R.row_index_repeats(count)
    else:
        idx, src = R.row_index(count, "permuted"), np.arange(count)
    d_table = row_table("normal", count, D, 121)
    table = host(d_table)
    v = R.normal_weight(count, D, seed=123)[src]
    d_idx, d_v = dev(idx), dev(v)
    ops.scatter_rows(d_table.data_ptr(), d_idx, d_v, average=True, distinct=False)
    want = R.scatter_rows_ref(table, idx, v, average=True, distinct=False)
    same_bits(host(d_table), want, "table behind a blending scatter")
    if count >= 6:
        assert (R.bits(R.scatter_rows_blend_per_entry(table, idx, v)) != R.bits(want)).any()
    same_bits(host(d_v), v, "rows")
    same_bits(host(d_idx), idx, "index")
    torch.cuda.synchronize()


# ---- 6. victim write-back --------------------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("shape", list(R.VWB_SHAPES))
@pytest.mark.parametrize("mode", R.VWB_MODES)
@pytest.mark.parametrize("aux_phase", [0, 1], ids=["phase0", "phase1"])
@pytest.mark.parametrize("D", R.VWB_DIMS, ids=ids(R.VWB_DIMS, "D%d"))
def test_victim_writeback(ops, D, aux_phase, mode, shape):
    geo = R.geo_vwb(D)
    ctx = ctx_for(ops, geo)
    idx, slots, _ = R.vwb_batch(shape, aux_phase)
    T, n = idx.shape
    d_w = pristine(("bits", geo.total_rows, D, 131), lambda: R.any_bits_weight(geo.total_rows, D, seed=131))
    weight = host(d_w)
    bind_weight(ctx, geo, d_w)
    host0 = [R.any_bits_weight(rows, D, seed=133 + t) for t, rows in enumerate(geo.table_rows)]
    pinned = [torch.from_numpy(h.copy()).pin_memory() for h in host0]
    ctx.bind_host_tables([p.data_ptr() for p in pinned])
    victims = wsrc = v_rows = vict = d_wsrc_wide = None
    if mode != "no-victims":
        victims = R.vwb_victims(shape, aux_phase)
        nv = int(victims[1][-1])
        vict = ops.Victims(ctx, nv + 4)
        v_rows = R.any_bits_weight(nv + 4, D, seed=137)
        vict.idx[:nv] = dev(victims[0])
        vict.off[:T + 1] = dev(victims[1])
        vict.off[T + 1] = nv
        vict.rows.copy_(dev(v_rows))
    ctx.bind_victims(vict)
    if mode == "wsrc":
        wsrc = R.vwb_wsrc(shape, aux_phase)
        wide = np.full((T, n + 3), -1, dtype=np.int32)
        wide[:, 1:1 + n] = wsrc
        d_wsrc_wide = dev(wide)
    idx_wide = np.zeros((T, n + 5), dtype=np.int64)
    idx_wide[:, 3:3 + n] = idx
    d_idx_wide, d_slots = dev(idx_wide), dev(slots)
    work = ops.victim_writeback_work(ctx, n)
    try:
        ops.victim_writeback(ctx, d_idx_wide[:, 3:3 + n], d_slots, None if wsrc is None else d_wsrc_wide[:, 1:1 + n], aux_phase, work)
        ctx.check()
        torch.cuda.synchronize()
    finally:
        ctx.bind_victims(None)
    want_host, want_v = R.vwb_ref(geo, idx, slots, aux_phase, weight, host0, victims=victims, wsrc=wsrc, v_rows=v_rows)
    for t in range(T):
        same_bits(pinned[t].numpy(), want_host[t], "host table %d" % t)
        missed = np.unique(idx[t][slots[t] >= geo.first_aux[t]])
        others = np.setdiff1d(np.arange(geo.table_rows[t]), missed)
        same_bits(want_host[t][others], host0[t][others], "host rows of indices that did not miss")
    if vict is not None:
        same_bits(host(vict.rows), want_v, "victim rows")
        assert (R.bits(want_v) != R.bits(v_rows)).any() and (R.bits(want_v[-4:]) == R.bits(v_rows[-4:])).all()
        same_bits(host(vict.idx[:nv]), victims[0], "victim index list")
        same_bits(host(vict.off[:T + 1]), victims[1], "victim offsets")
    same_bits(host(d_w), weight, "cache weight")
    same_bits(host(d_idx_wide), idx_wide, "idx")
    same_bits(host(d_slots), slots, "slots")
    if d_wsrc_wide is not None:
        same_bits(host(d_wsrc_wide), wide, "wsrc")
