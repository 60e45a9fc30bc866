"""The contracts of the kernels that move cache rows by an index list outside the training step, as plain numpy: the
touched-row merge (cdlrm_mark_rows, cdlrm_agg_compact, cdlrm_agg_mark_tier, cdlrm_agg_split, cdlrm_agg_gather,
cdlrm_agg_scatter), the drop-in row helpers (cdlrm_gather_rows, cdlrm_scatter_rows, cdlrm_blend_rows) and the victim
write-back (cdlrm_victim_writeback).  It imports nothing from the package.  Next to every restatement stand the builder of
the inputs the tests feed both sides and the comparator the tests use; tests/test_row_merge_kernels.py checks on any
machine that the inputs hold the edges they are meant to hold and that the comparators reject the plausible wrong answers.

These kernels copy, sort, divide once or add-and-halve once: every comparison is on the bits, there is no tolerance."""
import functools

import numpy as np

SENT8 = 0xA5                                                                    # what no kernel here ever writes
SENT64 = int(np.array([0xA5A5A5A5A5A5A5A5], dtype=np.uint64).view(np.int64)[0])
SENT32 = 0x7FA5A5A5                                                             # as fp32: a NaN with a payload
PAD = 64                                                                        # sentinel elements behind every buffer


class Geo:
    """A cache group's row layout, as ops.CacheCtx computes it."""

    def __init__(self, sets, ways, aux, D, aux_phases=1, table_rows=None):
        self.sets, self.ways, self.aux, self.D, self.aux_phases = list(sets), ways, aux, D, aux_phases
        self.T = len(self.sets)
        self.table_rows = list(table_rows) if table_rows else [p + 1000 for p in self.sets]
        self.first_aux = [p * ways for p in self.sets]
        self.rows = [p * ways + aux * aux_phases for p in self.sets]
        self.row_base = [0]
        for r in self.rows:
            self.row_base.append(self.row_base[-1] + r)
        self.total_rows = self.row_base[-1]
        self.total_tags = sum(self.first_aux)


def frozen(a):
    a.flags.writeable = False
    return a


def bits(a):
    """An array's bit patterns as unsigned integers of its element size."""
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def sentinel(shape, dtype):
    """A buffer pre-filled with the sentinel of its type."""
    dtype = np.dtype(dtype)
    if dtype == np.float32:
        return np.full(shape, SENT32, dtype=np.uint32).view(np.float32)
    return np.full(shape, {1: SENT8, 4: SENT32, 8: SENT64}[dtype.itemsize], dtype=dtype)


def same_bits(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    g, w = bits(got).reshape(-1), bits(want).reshape(-1)
    bad = np.flatnonzero(g != w)
    assert bad.size == 0, "%s: %d of %d elements differ, first at %d: got %#x want %#x" % (
        what, bad.size, g.size, bad[0], g[bad[0]], w[bad[0]])


def sorted_subset(total, count, seed):
    rng = np.random.RandomState(seed)
    return np.sort(rng.permutation(total)[:count]).astype(np.int64)


# ---- 1. flags to list: mark_rows, agg_compact ---------------------------------------------------------------------

GEO_FLAGS = Geo([1021, 3, 1030], ways=4, aux=5, D=4)       # rows 4089 + 17 + 4125 = 8231: three flag blocks, tail of 7
FLAG_BLOCK, FLAG_GROUP = 4096, 16                          # flags per block / per lane of the compaction
MARK_N = (1, 255, 256, 257, 262145)                        # 262145: one more than 1024 blocks x 256 threads


def mark_specials(geo, t):
    """Slot values every slot list of table t holds: skipped (-1), the first row, the last aux row, out of range (skipped)."""
    return [-1, 0, geo.rows[t] - 1, geo.rows[t], geo.rows[t] + 7]


@functools.lru_cache(maxsize=None)
def mark_slots(n, seed=11):
    """slots int32 [T, n] for cdlrm_mark_rows on GEO_FLAGS: the specials first (rotated per table, so that n = 1 still sets a
    byte), then draws with repeats from half of the table's rows; the LAST entry is a row nothing else names."""
    geo = GEO_FLAGS
    rng = np.random.RandomState(seed + n)
    out = np.empty((geo.T, n), dtype=np.int32)
    for t in range(geo.T):
        pool = rng.permutation(np.arange(1, geo.rows[t] - 1))
        half, tail = pool[:len(pool) // 2], pool[-1]
        out[t] = rng.choice(half, size=n)
        sp = mark_specials(geo, t)
        sp = sp[(t + 2) % 5:] + sp[:(t + 2) % 5]
        k = min(n, len(sp))
        out[t, :k] = sp[:k]
        if n > len(sp):
            out[t, n - 1] = tail
    return frozen(out)


def mark_rows_ref(geo, slots, touched):
    """touched[row_base[t] + s] = 1 for every slot 0 <= s < rows[t]; everything else as it was."""
    out = touched.copy()
    for t in range(geo.T):
        s = slots[t].astype(np.int64)
        s = s[(s >= 0) & (s < geo.rows[t])]
        out[geo.row_base[t] + s] = 1
    return out


COMPACT_SINGLES = ("0", "15", "16", "4095", "4096", "4097", "total-2", "total-1")
COMPACT_PATTERNS = ("empty",) + tuple("one@" + s for s in COMPACT_SINGLES) + (
    "group16", "block", "all", "block-edges", "random3", "random3-bytes")


@functools.lru_cache(maxsize=None)
def compact_flags(name, total=GEO_FLAGS.total_rows, seed=23):
    rng = np.random.RandomState(seed)
    f = np.zeros(total, dtype=np.uint8)
    if name.startswith("one@"):
        at = name[4:]
        f[total + int(at[5:]) if at.startswith("total") else int(at)] = 1
    elif name == "group16":
        f[FLAG_BLOCK - FLAG_GROUP:FLAG_BLOCK] = 1                        # the last lane of block 0, all 16 bytes
    elif name == "block":
        f[FLAG_BLOCK:2 * FLAG_BLOCK] = 1
    elif name == "all":
        f[:] = 1
    elif name == "block-edges":
        for b in range(FLAG_BLOCK, total, FLAG_BLOCK):
            f[b - 1] = f[b] = 1
    elif name == "random3":
        f[rng.rand(total) < 0.03] = 1
    elif name == "random3-bytes":                                        # any non-zero byte is a set flag
        m = rng.rand(total) < 0.03
        f[m] = rng.choice([1, 2, 128, 255], size=int(m.sum()))
        f[np.flatnonzero(m)[0]] = 255
    else:
        assert name == "empty", name
    return frozen(f)


def check_compact(flags, cap, got_rows, got_count, got_flags):
    """got_rows: the whole sentinel-filled buffer (cap entries the kernel may write, the rest behind them); got_flags: the
    flag buffer with its pad.  Entries beyond cap are dropped, the count stays the true one."""
    want = np.flatnonzero(flags).astype(np.int64)
    assert int(got_count) == want.size, (int(got_count), want.size)
    k = min(cap, want.size)
    same_bits(got_rows[:k], want[:k], "rows_out[:count]")
    same_bits(got_rows[k:], sentinel(got_rows.size - k, np.int64), "rows_out behind the list")
    assert not got_flags[:flags.size].any(), "flags are consumed"
    same_bits(got_flags[flags.size:], sentinel(got_flags.size - flags.size, np.uint8), "bytes behind the flags")


# ---- 2. deadline classes: agg_mark_tier ---------------------------------------------------------------------------

TIER_N = (1, 256, 257, 262145)
TIER_CLASSES = 4                                           # three marked classes + cold
TIER_PAD_SLOT = 1                                          # what the slot buffer holds outside the [T, n] view: a cache
                                                           # slot no batch names, so a read outside the view shows


@functools.lru_cache(maxsize=None)
def tier_batches(n, seed=31):
    """Three slot batches int32 [T, n] on GEO_FLAGS, for the classes 2, 1, 0 in the order the engine marks them.  Each
    draws (with repeats) from its own 30 % of a table's cache slots, so the batches overlap partly; besides: aux slots
    (first_aux .. rows - 1 and beyond) and negatives, which are skipped.  Slot 2 of every table is in all three."""
    geo = GEO_FLAGS
    rng = np.random.RandomState(seed + n)
    out = []
    for b in range(3):
        s = np.empty((geo.T, n), dtype=np.int32)
        for t in range(geo.T):
            fa = geo.first_aux[t]
            pool = np.arange(3, fa)
            own = pool[rng.rand(pool.size) < 0.3]
            s[t] = rng.choice(own if own.size else pool[:2], size=n)
            sp = [2, fa, geo.rows[t] - 1, -1, fa - 1, geo.rows[t] + 3, -7, 0]
            sp = sp[:1] + sp[1 + b:] + sp[1:1 + b]                       # n = 1: slot 2 in every batch
            k = min(n, len(sp))
            s[t, :k] = sp[:k]
        out.append(frozen(s))
    return tuple(out)


def mark_tier_ref(geo, slots, value, tier):
    """tier[row_base[t] + s] = value for every cache slot 0 <= s < P_t * ways."""
    out = tier.copy()
    for t in range(geo.T):
        s = slots[t].astype(np.int64)
        s = s[(s >= 0) & (s < geo.first_aux[t])]
        out[geo.row_base[t] + s] = value
    return out


# ---- 3. stable split: agg_split ------------------------------------------------------------------------------------

GEO_SPLIT = Geo([30000, 5000], ways=4, aux=16, D=4)        # 140032 rows
SPLIT_BLOCK = 1024                                         # list entries per block: 256 threads x 4
SPLIT_COUNTS = (0, 1, 3, 1023, 1024, 1025, 4097, 131073)   # 131073 x 8 classes: 129 blocks, 1032 scanned counters
SPLIT_CLASSES = (1, 2, 8)


def split_patterns(C):
    p = ["single%d" % c for c in range(C)]
    if C >= 3:
        p.append("empty-middle")
    return p + ["cycle", "skewed-cold", "clamp"]


SPLIT_CASES = [(C, p) for C in SPLIT_CLASSES for p in split_patterns(C)]


@functools.lru_cache(maxsize=None)
def split_rows(count, seed=41):
    return frozen(sorted_subset(GEO_SPLIT.total_rows, count, seed))


@functools.lru_cache(maxsize=None)
def split_tier(count, C, pattern, seed=43):
    """The tier bytes of all of GEO_SPLIT's rows; rows outside the list hold any byte."""
    rows = split_rows(count)
    rng = np.random.RandomState(seed + 7 * C + count)
    tier = rng.randint(0, 256, size=GEO_SPLIT.total_rows).astype(np.uint8)
    n = rows.size
    if pattern.startswith("single"):
        cls = np.full(n, int(pattern[6:]))
    elif pattern == "empty-middle":
        cls = rng.randint(0, C - 1, size=n)
        cls[cls >= C // 2] += 1
    elif pattern == "cycle":
        cls = np.arange(n) % C
    elif pattern == "skewed-cold":
        cls = np.where(rng.rand(n) < 0.9, C - 1, rng.randint(0, C, size=n))
    else:
        assert pattern == "clamp", pattern
        cls = rng.randint(0, C + 3, size=n)
        over = cls >= C
        cls[over] = rng.choice([C, C + 1, 200, 255], size=int(over.sum()))
        if n:
            cls[0] = 255
        if n > 1:
            cls[n - 1] = C
    tier[rows] = cls
    return frozen(tier)


def split_ref(rows, count, tier, C):
    """(rows grouped by class, ascending inside a class; class offsets [C + 1])."""
    cls = np.minimum(tier[rows[:count]].astype(np.int64), C - 1)
    order = np.argsort(cls, kind="stable")
    off = np.zeros(C + 1, dtype=np.int64)
    off[1:] = np.cumsum(np.bincount(cls, minlength=C))
    return rows[:count][order], off


def check_split(rows, count, tier, C, got_rows, got_off):
    """got_rows / got_off: the whole sentinel-filled buffers."""
    want_rows, want_off = split_ref(rows, count, tier, C)
    assert int(want_off[C]) == count
    same_bits(got_off[:C + 1], want_off, "class_off")
    same_bits(got_off[C + 1:], sentinel(got_off.size - C - 1, np.int64), "behind class_off")
    same_bits(got_rows[:count], want_rows, "rows_out[:count]")
    same_bits(got_rows[count:], sentinel(got_rows.size - count, np.int64), "rows_out behind the list")


# ---- 4. chunked agg_gather / agg_scatter ---------------------------------------------------------------------------

AGG_DIMS = (4, 12, 128)
AGG_U = 1000
AGG_CHUNKS = (1, 8, 333, AGG_U)
AGG_COUNT_WORDS = {"U": AGG_U, "U-3": AGG_U - 3, "0": 0}
AGG_SCALES = (1.0, 2.0, 3.0, 7.0)
AGG_BIG = 32769                                            # x 32 float4 per row > 4096 blocks x 256 threads


def geo_agg(D):
    return Geo([8200, 500], ways=4, aux=16, D=D)           # 34832 rows


def chunks(U, size):
    return [(lo, min(U, lo + size)) for lo in range(0, U, size)]


SPECIALS32 = np.array([0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x7FC00001, 0xFFC12345, 0x00000001, 0x807FFFFF,
                       0x3FC00000, 0xC2F6E979], dtype=np.uint32)     # +-0, +-inf, two NaNs, two denormals, 1.5, -123.456


@functools.lru_cache(maxsize=None)
def any_bits_weight(n, D, seed=51):
    """Rows of arbitrary bit patterns (NaNs, infinities and denormals among them): for exact copies."""
    rng = np.random.RandomState(seed)
    return frozen(rng.randint(0, 1 << 32, size=(n, D), dtype=np.uint64).astype(np.uint32).view(np.float32))


def plant_specials(w, rows):
    """The special values, cycled through the elements of the first listed rows."""
    D = w.shape[1]
    k = min(len(rows), -(-2 * SPECIALS32.size // D))
    flat = bits(w)
    for j, r in enumerate(rows[:k]):
        flat[r] = SPECIALS32[(j * D + np.arange(D)) % SPECIALS32.size]
    return w


@functools.lru_cache(maxsize=None)
def normal_weight(n, D, seed=53):
    """Random signs and mantissas, exponents 2^-63 .. 2^63: every quotient by 2, 3, 7 and every mean of two is normal."""
    rng = np.random.RandomState(seed)
    b = (rng.randint(0, 2, size=(n, D), dtype=np.uint64) << 31) | (rng.randint(64, 191, size=(n, D), dtype=np.uint64) << 23) \
        | rng.randint(0, 1 << 23, size=(n, D), dtype=np.uint64)
    return frozen(b.astype(np.uint32).view(np.float32))


def divided(w, scale):
    """weight / world_size as the reference divides: a true fp32 division, the bits passed through at scale 1."""
    return w if scale == 1.0 else w / np.float32(scale)


def agg_gather_ref(weight, rows, count, scale, buf, cap, first):
    """One call: `rows` and `buf` start at entry `first` of the list whose length is the count word."""
    m = max(0, min(count - first, cap))
    buf[:m] = divided(weight[rows[:m]], scale)


def agg_scatter_ref(weight, rows, count, buf, cap, first):
    m = max(0, min(count - first, cap))
    weight[rows[:m]] = buf[:m]


def mean2(a, b):
    """The two-rank mean as the merge computes it: each rank's row divided by 2, the quotients added."""
    return a / np.float32(2) + b / np.float32(2)


# ---- 5. row helpers ------------------------------------------------------------------------------------------------

ROW_DIMS = (4, 12, 128)
ROW_COUNTS = (0, 1, 63, 64, 65)
ROW_BIG = 32769
ROW_ORDERS = ("sorted", "permuted", "ends")


def row_table_rows(count):
    return 33000 if count > 1000 else 257


@functools.lru_cache(maxsize=None)
def row_index(count, order, seed=61):
    """A list of DISTINCT row numbers; "ends" holds row 0 and the last row."""
    n = row_table_rows(count)
    rng = np.random.RandomState(seed + count)
    idx = rng.permutation(np.arange(1, n - 1))[:count].astype(np.int64)
    if order == "sorted":
        idx = np.sort(idx)
    elif order == "ends":
        if count >= 1:
            idx[count // 2] = n - 1
        if count >= 2:
            idx[0] = 0
    return frozen(idx)


@functools.lru_cache(maxsize=None)
def row_index_repeats(count, seed=67):
    """(index, source entry of every entry): one row listed twice and one three times, the copies apart from each other;
    repeats carry identical rows, so entry i brings the row of entry src[i]."""
    assert count >= 6
    idx = row_index(count, "permuted", seed).copy()
    src = np.arange(count)
    for a, b in ((0, count - 1), (1, count // 2), (1, count - 2)):
        idx[b], src[b] = idx[a], a
    return frozen(idx), frozen(src)


def halved_sum(h, v):
    with np.errstate(over="ignore", invalid="ignore"):
        return (h + v) / np.float32(2)


def scatter_rows_ref(dst, index, rows, average, distinct=True):
    """dst[index[i]] = rows[i], or the mean with the OLD destination row -- once per listed row, however often it is listed."""
    out = dst.copy()
    if average:
        rows = halved_sum(dst[index], rows)
    for i, r in enumerate(index):
        out[r] = rows[i]
    return out


def scatter_rows_blend_per_entry(dst, index, rows):
    """The wrong answer for a list with repeats: every entry blended against what the entry before it left."""
    out = dst.copy()
    for i, r in enumerate(index):
        out[r] = halved_sum(out[r], rows[i])
    return out


# ---- 6. victim write-back -------------------------------------------------------------------------------------------

VWB_DIMS = (4, 128, 512)                                   # 512: two trips of the 64-lane column loop
VWB_AUX = 2500
VWB_DISTANCES = (1, 63, 64, 65)                            # miss distances between two occurrences of one index
VWB_SHAPES = {"n2500": (2500, None), "64-misses": (72, 64), "65-misses": (73, 65)}       # n, number of misses
VWB_MODES = ("no-victims", "victim-search", "wsrc")


def geo_vwb(D):
    return Geo([64, 7], ways=4, aux=VWB_AUX, D=D, aux_phases=2, table_rows=[3000, 2600])


@functools.lru_cache(maxsize=None)
def vwb_batch(shape, aux_phase, seed=71):
    """(idx int64 [T, n], slots int32 [T, n], miss mask [T, n]).  About a tenth of the positions are hits, interleaved; the
    i-th miss of a table (position order) sits in aux row i of the phase.  The misses' indices are distinct except for the
    planted repeats: at every miss distance of VWB_DISTANCES that fits, and the first miss's index again at the last."""
    n, n_miss = VWB_SHAPES[shape]
    geo = geo_vwb(4)
    rng = np.random.RandomState(seed + n)
    idx = np.empty((geo.T, n), dtype=np.int64)
    slots = np.empty((geo.T, n), dtype=np.int32)
    miss = np.empty((geo.T, n), dtype=bool)
    for t in range(geo.T):
        if n_miss is None:
            m = rng.rand(n) >= 0.1
            m[0] = m[n - 1] = True
        else:
            m = np.ones(n, dtype=bool)
            m[rng.permutation(np.arange(1, n - 1))[:n - n_miss]] = False
        M = int(m.sum())
        pool = rng.permutation(geo.table_rows[t])
        mi, rest = pool[:M].copy(), pool[M:]
        a = 3
        for d in VWB_DISTANCES:
            if a + d < M - 1:
                mi[a + d] = mi[a]
                a += d + 5
        mi[M - 1] = mi[0]
        idx[t, m] = mi
        # hits: half of them on indices that also miss in this batch (their host rows ARE written, by the miss), half elsewhere
        h = np.flatnonzero(~m)
        also = rng.rand(h.size) < 0.5
        also[:2] = (True, False)
        idx[t, h] = np.where(also, rng.choice(mi, size=h.size), rng.choice(rest, size=h.size))
        slots[t, m] = geo.first_aux[t] + aux_phase * geo.aux + np.arange(M)
        slots[t, h] = rng.randint(0, geo.first_aux[t], size=h.size)
        miss[t] = m
    return frozen(idx), frozen(slots), frozen(miss)


def miss_distances(idx_t, miss_t):
    """The distances, in misses, between consecutive occurrences of one index among a table's misses."""
    mi = idx_t[miss_t]
    last, out = {}, set()
    for i, v in enumerate(mi.tolist()):
        if v in last:
            out.add(i - last[v])
        last[v] = i
    return out


@functools.lru_cache(maxsize=None)
def vwb_victims(shape, aux_phase, seed=73):
    """A window's victim list for the batch: per table the sorted indices of about half of the batch's distinct missing
    indices plus as many that do not miss; (v_idx int64 [V], v_off int64 [T + 1])."""
    idx, _, miss = vwb_batch(shape, aux_phase)
    geo = geo_vwb(4)
    rng = np.random.RandomState(seed)
    parts, off = [], [0]
    for t in range(geo.T):
        mi = np.unique(idx[t][miss[t]])
        take = mi[rng.rand(mi.size) < 0.5]
        if take.size == 0:
            take = mi[:1]
        others = np.setdiff1d(np.arange(geo.table_rows[t]), mi)
        extra = rng.choice(others, size=min(take.size, others.size // 2), replace=False)
        v = np.sort(np.concatenate([take, extra]))
        parts.append(v)
        off.append(off[-1] + v.size)
    return frozen(np.concatenate(parts).astype(np.int64)), frozen(np.array(off, dtype=np.int64))


@functools.lru_cache(maxsize=None)
def vwb_wsrc(shape, aux_phase, seed=79):
    """The resolver's answer per position, int32 [T, n]: where the index's copy sits among the victim rows, or -1.  One
    answer per index; a third of the listed indices answer -1 all the same (the kernel has to believe wsrc, not search)."""
    idx, _, _ = vwb_batch(shape, aux_phase)
    v_idx, v_off = vwb_victims(shape, aux_phase)
    rng = np.random.RandomState(seed)
    out = np.full(idx.shape, -1, dtype=np.int32)
    for t in range(idx.shape[0]):
        lo, hi = int(v_off[t]), int(v_off[t + 1])
        keep = rng.rand(hi - lo) >= 1 / 3
        q = lo + np.searchsorted(v_idx[lo:hi], idx[t])
        q = np.minimum(q, hi - 1)
        found = (v_idx[q] == idx[t]) & keep[q - lo]
        out[t, found] = q[found]
    return frozen(out)


def vwb_ref(geo, idx, slots, aux_phase, weight, host, victims=None, wsrc=None, v_rows=None, first_wins=False):
    """Position by position: host[t][idx] = the miss's aux row, and the same for the index's copy among the victim rows
    (where wsrc says, or where the sorted list holds the index).  The last occurrence wins.  Returns (host, v_rows) copies.
    first_wins: the wrong answer, for the comparator's control."""
    host = [h.copy() for h in host]
    v_rows = None if v_rows is None else v_rows.copy()
    for t in range(geo.T):
        first = geo.first_aux[t] + aux_phase * geo.aux
        seen = set()
        for p in range(idx.shape[1]):
            s = int(slots[t, p])
            if s < first:
                continue
            key = int(idx[t, p])
            if first_wins and key in seen:
                continue
            seen.add(key)
            row = weight[geo.row_base[t] + s]
            host[t][key] = row
            vp = -1
            if wsrc is not None:
                vp = int(wsrc[t, p])
            elif victims is not None:
                v_idx, v_off = victims
                lo, hi = int(v_off[t]), int(v_off[t + 1])
                q = lo + int(np.searchsorted(v_idx[lo:hi], key))
                if q < hi and v_idx[q] == key:
                    vp = q
            if vp >= 0:
                v_rows[vp] = row
    return host, v_rows
