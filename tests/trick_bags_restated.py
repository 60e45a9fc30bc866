"""The contracts of the stand-alone bag operators of csrc/qr.hip as plain numpy in float64: the quotient-remainder bag
(cdlrm_qr_embbag_fwd / _bwd behind tricks.QREmbeddingBag) and the plain sum bag of any width (cdlrm_bag_fwd / _bwd behind
tricks.PrEmbeddingBag.embs).  It imports nothing from the package.  Next to every restatement stand the builders of the inputs
the tests feed both sides and the comparator; tests/test_trick_bags_edges.py checks on any machine that the inputs hold the
edges they are meant to hold and that the comparator rejects the plausible wrong answers.

Every bound is derived, per element, from the inputs.  u = 2^-24; L = lookups of a bag.  The kernels add sequentially in fp32
and the sums hold no multiply-add:

    pooled operand     |E^ - E| <= (L - 1) u sum|W[row_i]|
    add                bound(Eq) + bound(Er) + u |Eq + Er|
    mult               |Er| bound(Eq) + |Eq| bound(Er) + u |Eq Er|
    concat             the operand bounds themselves
    backward element   that receives m contributions d_i: (m - 1) u sum|d_i| for the sum in any order (float atomics); for
                       mult, u sum|d_i| more for the one product rounding and sum|g_i| bound(saved operand) for the operand

each times SLACK = 1.0625 for the second-order terms, and nothing else added."""
import functools

import numpy as np

U = 2.0 ** -24
SLACK = 1.0625
PAD = 64                                                   # sentinel elements behind every output buffer
SENT32 = 0x7FA5A5A5                                        # as fp32: a NaN with a payload, which no kernel here writes
OPS = ("mult", "add", "concat")
OP_CODE = {"mult": 0, "add": 1, "concat": 2}
C4 = 4                                                     # collisions of every QR case

RAGGED = (0, 1, 0, 0, 2, 7, 1000, 1, 0)                    # empty first, two empties in a row, one long, empty last
QR_DIMS = (4, 12, 16, 20, 32, 36, 64, 68, 128, 132, 256)   # every lane instance, once with idle lanes and once full
QR_DIMS_TWO_TRIPS = (260, 512)                             # D4 = 65 and 128: a second trip of the 64-lane column loop
QR_BAGS = 37
QR_GRID_CAP = 8192
BAG_DIMS = (1, 2, 3, 5, 7, 8, 13, 64)
BAG_BAGS = 300
QR_CAP_64 = (132, 32769)                                   # D, bags: 8192 blocks x 4 bags + 1
QR_CAP_4 = (4, 524289)                                     # 8192 x 64 + 1
BAG_CAP = (3, 699051)                                      # 699051 x 3 = 8192 x 256 + 1
N_C4 = 39884406                                            # the largest Terabyte table
QUIRK_IDS = (0, 3, 16777215, 16777216, 16777217, 33554433, 25000003, 39884403, 39884405)
N_TOP = (1 << 24) + 4                                      # categories whose top id's float32 quotient is rows_q
CONTENTION_BAGS, CONTENTION_N = 64, 8192


def frozen(a):
    a.flags.writeable = False
    return a


def pow2ceil(x):
    p = 1
    while p < x:
        p *= 2
    return p


def qr_lanes(D):
    """Lanes per row of k_qr_fwd / k_qr_bwd for an embedding width D (one float4 per lane and trip)."""
    return min(64, max(4, pow2ceil(-(-D // 4))))


def sentinel(shape):
    return np.full(shape, SENT32, dtype=np.uint32).view(np.float32)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def same_bits(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    g, w = bits(got).reshape(-1), bits(want).reshape(-1)
    bad = np.flatnonzero(g != w)
    assert bad.size == 0, "%s: %d of %d elements differ, first at %d: got %#x want %#x" % (
        what, bad.size, g.size, bad[0], g[bad[0]], w[bad[0]])


def within(got, want, bound, what):
    """|got - want| <= bound element by element; a NaN fails.  The bound is an array of the output's shape."""
    got = np.asarray(got, dtype=np.float64)
    want, bound = np.asarray(want, dtype=np.float64), np.asarray(bound, dtype=np.float64)
    assert got.shape == want.shape == bound.shape, (what, got.shape, want.shape, bound.shape)
    err = np.abs(got - want)
    ok = err <= bound
    if ok.all():
        return
    over = np.where(ok, 0.0, np.where(np.isnan(err), np.inf, err - bound))
    i = np.unravel_index(int(np.argmax(over)), over.shape)
    raise AssertionError("%s: %d of %d elements outside their bound; worst at %s: got %r, want %r, |err| %.3g > bound %.3g" % (
        what, int((~ok).sum()), ok.size, i, float(got[i]), float(want[i]), float(err[i]), float(bound[i])))


# ---- inputs --------------------------------------------------------------------------------------------------------

def ragged_lengths(n_bags, long=1000, last=0):
    """RAGGED repeated, every repetition rotated one further, cut to n_bags; the last bag is empty (`ragged`: its offset equals
    n) or holds `last` lookups (`closed_by_n`: its end comes from n)."""
    base = [long if v == 1000 else v for v in RAGGED]
    out = []
    for k in range(-(-n_bags // len(base))):
        out += base[k % len(base):] + base[:k % len(base)]
    out = out[:n_bags]
    out[-1] = last
    return np.array(out, dtype=np.int64)


def offsets_of(lengths):
    """(offsets int64 [n_bags], n)."""
    off = np.zeros(lengths.size, dtype=np.int64)
    off[1:] = np.cumsum(lengths)[:-1]
    return off, int(lengths.sum())


@functools.lru_cache(maxsize=None)
def bags(kind, n_bags, long=1000):
    """`ragged` / `closed_by_n` -> (offsets, n), frozen."""
    assert kind in ("ragged", "closed_by_n"), kind
    off, n = offsets_of(ragged_lengths(n_bags, long, last=0 if kind == "ragged" else 3))
    return frozen(off), n


@functools.lru_cache(maxsize=None)
def cycle_bags(n_bags, cycle=(1, 0, 2)):
    lengths = np.resize(np.array(cycle, dtype=np.int64), n_bags)
    off, n = offsets_of(lengths)
    return frozen(off), n


@functools.lru_cache(maxsize=None)
def small_ids(n, ncat, seed):
    return frozen(np.random.RandomState(seed).randint(0, ncat, size=n).astype(np.int64))


@functools.lru_cache(maxsize=None)
def cap_ids(n, below, tail, seed):
    """The ids of a grid-cap case: draws below `below`, and `tail` -- rows no other lookup names -- as the last lookups.  The
    gradient rows of the bag behind the grid then hold that bag's contribution alone: thousands of contributions on one
    element would bury a missing one in their bound."""
    idx = np.random.RandomState(seed).randint(0, below, size=n).astype(np.int64)
    idx[n - len(tail):] = tail
    return frozen(idx)


@functools.lru_cache(maxsize=None)
def quirk_ids(n, seed=7, n_cat=N_C4):
    """Ids below n_cat: a third anywhere, the rest above 2^25 (where float32 holds multiples of 4), QUIRK_IDS planted at evenly
    spread positions and again at the very end and the very start."""
    rng = np.random.RandomState(seed)
    idx = np.where(rng.rand(n) < 1 / 3, rng.randint(0, n_cat, size=n), rng.randint(1 << 25, n_cat, size=n)).astype(np.int64)
    q = np.array(QUIRK_IDS, dtype=np.int64)
    q = q[q < n_cat]
    if n >= 4 * q.size:
        idx[np.linspace(q.size, n - q.size - 1, q.size).astype(np.int64)] = q
        idx[:q.size] = q
        idx[n - q.size:] = q[::-1]
    else:
        idx[:min(n, q.size)] = q[:min(n, q.size)]
    return frozen(idx)


def quirk_share(idx, c):
    """The share of an index list whose float32 quotient is not the integer one."""
    return float(np.mean(quotient(idx, c) != idx // c))


@functools.lru_cache(maxsize=None)
def top_ids(n, at, seed=9):
    """Ids below N_TOP = 2^24 + 4 with the top id, 2^24 + 3, exactly once, at position `at`: float32 holds even numbers there,
    the tie goes to 2^24 + 4 and the quotient by 4 is 2^22 + 1 = ceil(N_TOP / 4) = rows_q.  No other id reaches rows_q."""
    idx = np.random.RandomState(seed).randint(0, N_TOP - 4, size=n).astype(np.int64)
    idx[at] = N_TOP - 1
    return frozen(idx)


@functools.lru_cache(maxsize=None)
def contention_input():
    """(idx, offsets, n): 8192 lookups in 64 bags of 128, every one on quotient row 5 of a 26-row table (c = 4); the
    remainders are 0 and 3 only, so remainder rows 1 and 2 are absent."""
    rng = np.random.RandomState(13)
    idx = 5 * C4 + np.where(rng.rand(CONTENTION_N) < 0.5, 0, 3).astype(np.int64)
    off = np.arange(0, CONTENTION_N, CONTENTION_N // CONTENTION_BAGS, dtype=np.int64)
    return frozen(idx), frozen(off), CONTENTION_N


@functools.lru_cache(maxsize=None)
def weights(rows, D, seed):
    return frozen(np.random.RandomState(seed).randn(rows, D).astype(np.float32))


class RowIsIndex:
    """A table too large to hold on the host whose row i is i in every column (exact in fp32 below 2^24)."""

    def __init__(self, rows, D):
        self.shape = (rows, D)

    def __getitem__(self, rows):
        rows = np.asarray(rows)
        assert rows.size == 0 or (rows.min() >= 0 and rows.max() < self.shape[0])
        return np.repeat(rows.astype(np.float64)[:, None], self.shape[1], axis=1)


# ---- restatements --------------------------------------------------------------------------------------------------

def quotient(idx, c):
    """torch's (idx / c).long(): a float32 true division, truncated."""
    return (idx.astype(np.float32) / np.float32(c)).astype(np.int64)


def bag_ends(off, n):
    """Bag b covers lookups [off[b], off[b + 1]); the last bag ends at n."""
    return np.append(off[1:], n).astype(np.int64)


def lookups(off, ends):
    """(position of every lookup that lies in a bag, its bag), in bag order."""
    lengths = ends - off
    assert (lengths >= 0).all()
    bag = np.repeat(np.arange(off.size), lengths)
    first = np.repeat(off - (np.cumsum(lengths) - lengths), lengths)
    return first + np.arange(bag.size), bag


def sum_by(keys, vals, n_keys):
    """out[k] = the float64 sum of vals[i] over keys[i] == k, vals [n, D]."""
    out = np.zeros((n_keys,) + vals.shape[1:], dtype=np.float64)
    if keys.size:
        order = np.argsort(keys, kind="stable")
        k = keys[order]
        starts = np.flatnonzero(np.append(True, k[1:] != k[:-1]))
        out[k[starts]] = np.add.reduceat(vals[order], starts, axis=0)
    return out


def pooled(W, rows, bag, n_bags):
    """(E [n_bags, D] float64, its bound) of the fp32 sequential sum of W[rows] per bag."""
    w = np.asarray(W[rows], dtype=np.float64)
    E, A = sum_by(bag, w, n_bags), sum_by(bag, np.abs(w), n_bags)
    L = np.bincount(bag, minlength=n_bags).astype(np.float64)
    return E, np.maximum(L - 1, 0)[:, None] * U * A


class QR:
    """The quotient-remainder bag on one input, float64.  q: the quotient of every lookup (default: the float32 one); ends:
    where every bag ends (default: the next offset, n for the last); oob_row0: lookups whose quotient is >= rows_q read row 0,
    as the kernel substitutes."""

    def __init__(self, idx, off, n, Wq, Wr, c, q=None, ends=None, oob_row0=False):
        self.c, self.n_bags, self.D = c, off.size, Wq.shape[1]
        self.rows_q = Wq.shape[0]
        pos, self.bag = lookups(off, bag_ends(off, n) if ends is None else ends)
        v = idx[pos]
        self.q = (quotient(v, c) if q is None else q[pos])
        self.r = v % c
        self.outside = self.q >= self.rows_q
        if oob_row0:
            self.q = np.where(self.outside, 0, self.q)
        self.Eq, self.bEq = pooled(Wq, self.q, self.bag, self.n_bags)
        self.Er, self.bEr = pooled(Wr, self.r, self.bag, self.n_bags)

    def forward(self, op):
        """(out, bound): [n_bags, D], [n_bags, 2 D] for concat."""
        Eq, Er, bq, br = self.Eq, self.Er, self.bEq, self.bEr
        if op == "mult":
            out, bound = Eq * Er, np.abs(Er) * bq + np.abs(Eq) * br + U * np.abs(Eq * Er)
        elif op == "add":
            out, bound = Eq + Er, bq + br + U * np.abs(Eq + Er)
        else:
            out, bound = np.concatenate([Eq, Er], axis=1), np.concatenate([bq, br], axis=1)
        return out, SLACK * bound

    def backward(self, op, G, mult_dq_from_eq=False):
        """Dense (gWq, bound, gWr, bound) for grad_out G [n_bags, D or 2 D].  mult_dq_from_eq: the wrong answer that takes the
        quotient's own pooled operand for its gradient."""
        G = np.asarray(G, dtype=np.float64)
        D = self.D
        if op == "mult":
            dq, dr = G * (self.Eq if mult_dq_from_eq else self.Er), G * self.Eq
            oq, orr = np.abs(G) * self.bEr, np.abs(G) * self.bEq                # the saved operand's forward error
        elif op == "add":
            dq, dr, oq, orr = G, G, None, None
        else:
            dq, dr, oq, orr = G[:, :D], G[:, D:], None, None
        res = []
        for rows, n_rows, d, o in ((self.q, self.rows_q, dq, oq), (self.r, self.c, dr, orr)):
            contrib = d[self.bag]
            g = sum_by(rows, contrib, n_rows)
            S = sum_by(rows, np.abs(contrib), n_rows)
            m = np.bincount(rows, minlength=n_rows).astype(np.float64)
            bound = np.maximum(m - 1, 0)[:, None] * U * S
            if op == "mult":
                bound = bound + U * S + sum_by(rows, o[self.bag], n_rows)
            res += [g, SLACK * bound]
        return tuple(res)


class Bag:
    """The plain sum bag of any width, float64; ids outside [0, rows) are skipped by the backward (skip_outside) -- the forward
    refuses them."""

    def __init__(self, idx, off, n, W_shape, skip_outside=False):
        self.shape, self.n_bags = tuple(W_shape), off.size
        pos, self.bag = lookups(off, bag_ends(off, n))
        self.rows = idx[pos]
        if skip_outside:
            keep = (self.rows >= 0) & (self.rows < self.shape[0])
            self.rows, self.bag = self.rows[keep], self.bag[keep]

    def forward(self, W):
        E, b = pooled(W, self.rows, self.bag, self.n_bags)
        return E, SLACK * b

    def backward(self, G):
        contrib = np.asarray(G, dtype=np.float64)[self.bag]
        g = sum_by(self.rows, contrib, self.shape[0])
        S = sum_by(self.rows, np.abs(contrib), self.shape[0])
        m = np.bincount(self.rows, minlength=self.shape[0]).astype(np.float64)
        return g, SLACK * np.maximum(m - 1, 0)[:, None] * U * S


# ---- the cases of the reference fixture (tools/make_golden.py: g_qr_edges, g_md_edges) -----------------------------

FIX_DIMS = (12, 20)
FIX_BAGS, FIX_LONG = 18, 150                               # two rotations of RAGGED: 2 x 161 lookups
FIX_NCAT = 103
FIX_WIDTHS = (3, 5)


def fixture_qr_inputs(kind, D):
    """kind `ragged`: small ids in ragged bags; `quirk`: ids of the N_C4 table in closed_by_n bags.  -> dict(idx, off, n,
    ncat, c, G).  G is [n_bags, 2 D]; mult and add take its first D columns."""
    off, n = bags("ragged" if kind == "ragged" else "closed_by_n", FIX_BAGS, FIX_LONG)
    ncat = FIX_NCAT if kind == "ragged" else N_C4
    idx = small_ids(n, ncat, 300 + D) if kind == "ragged" else quirk_ids(n, seed=310 + D)
    G = np.random.RandomState(320 + D).randn(FIX_BAGS, 2 * D).astype(np.float32)
    return dict(idx=idx, off=off, n=n, ncat=ncat, c=C4, G=frozen(G))


def fixture_bag_inputs(D):
    off, n = bags("ragged", FIX_BAGS, FIX_LONG)
    return dict(idx=small_ids(n, FIX_NCAT, 330 + D), off=off, n=n, ncat=FIX_NCAT,
                G=frozen(np.random.RandomState(340 + D).randn(FIX_BAGS, D).astype(np.float32)))



class FormulaTable:
    """A table too large to hold on the host: w[i, d] = ((37 i + 11 d + salt) mod 1024) / 1024 - 0.5, exact in fp32 (the
    contents tests/test_hip_kernels.py gives its 10 GB quotient table); neighbouring rows differ in every column."""

    def __init__(self, rows, D, salt):
        self.shape, self.salt = (rows, D), salt

    def __getitem__(self, rows):
        rows = np.asarray(rows, dtype=np.int64)
        assert rows.size == 0 or (rows.min() >= 0 and rows.max() < self.shape[0])
        d = np.arange(self.shape[1], dtype=np.int64)[None, :]
        return ((rows[:, None] * 37 + d * 11 + self.salt) & 1023).astype(np.float64) / 1024.0 - 0.5


@functools.lru_cache(maxsize=None)
def contention_grad(cols, kind):
    """grad_out [64, cols] of the contention case.  `spread`: normal draws times 2^-8 .. 2^8, element by element -- the bound
    of 8192 adds in any order, (m - 1) u sum|d_i|, is 4.3 times the MEAN contribution, so only a contribution well above the
    mean can be missed visibly.  `integers`: -8 .. 8, every partial sum of which is an integer below 2^24: `add` is exact."""
    rng = np.random.RandomState(17)
    if kind == "integers":
        return frozen(rng.randint(-8, 9, size=(CONTENTION_BAGS, cols)).astype(np.float32))
    assert kind == "spread", kind
    return frozen((rng.randn(CONTENTION_BAGS, cols) * 2.0 ** rng.randint(-8, 9, size=(CONTENTION_BAGS, cols))).astype(np.float32))
