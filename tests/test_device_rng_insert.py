"""The device-drawn cache insert (k_assign with q == NULL: --device-rng, every bench.py line) against a host restatement of
its draw, bit for bit.

The draw is counter-based, so it has one right value.  For claimant m (numbered over all tables of a window, in table then
index order) and way w, k_assign takes the Philox4x32-10 block at counter (c0, c1, c2, c3) = (lo32(m * ways + w),
hi32(m * ways + w), 0x43444c52, 0) under the key (lo32(seed), hi32(seed)), keeps x = r[0] >> 8 (u = (x + 1) * 2^-24 in
(0, 1], q = -log(u) ~ Exp(1)) and picks argmax(p / q) over the available ways -- p is one value over them and -log falls
strictly, so that is THE FIRST MAXIMUM OF x OVER THE AVAILABLE WAYS, and the kernel compares the 24-bit integers as they are.
(It compared p / -__logf(u) in float before this file existed: u = 1 gave q = -0, so the draw that should win lost to every
other available way, and 0 / -0 = NaN at a protected way 0 kept that way.  With the integers there is no logarithm left, so
no pair of draws is ambiguous and no margin is needed: every comparison below is exact.)

philox4x32_10 / draw_u restate that in numpy (checked against the three published Philox4x32-10 known-answer vectors).  To run
the oracle on exactly that rule, O.cache_embeddings gets a q source that returns, per claimant, q[w] = 1 + the dense
descending rank of x[w] over all ways: p / q then takes values among p, p / 2, ... p / 64, distinct floats, so
O.choose_ways' float argmax is the integer argmax with no rounding question (equal x share a rank; the first wins on both
sides).  Which ways are available comes from the oracle's own tag state, never from the device.  The q source is called
table by table while the device's m runs over all tables, so it carries a running offset and is made anew per window.

Fixtures are the window-cycle ones (test_window_cycle_shapes.py: eight (row width, way count) geometries, three windows).
Window w of a case draws at seed base * 1000003 + w, the engine's formula; BASE_SEEDS hold the CLI's default 123 (product
below 2^32), three whose product passes 2^32 and one past 2^60, so the key's upper word is non-zero in most cases.

Not reachable at these shapes, and not forced: the counter's upper word c1 (needs m * ways >= 2^32) and the cap_uniq cut of
the claimant count.
"""
import functools
from collections import namedtuple

import numpy as np
import pytest
import torch

from oracle import cdlrm_oracle as O
from test_hip_kernels import DEV, DevState
from test_window_cycle_shapes import (CASES, CASE_IDS, N_WINDOWS, CycleState, assert_window_equals_oracle, build_fixture,
                                      oracle_windows, run_window)
from test_window_cycle_shapes import ops, _free_the_case_before_the_next      # noqa: F401  (fixtures)

gpu = pytest.mark.gpu

SEED_STEP = 1000003            # WindowPipeline.plan_window: seed * 1000003 + window_no
BASE_SEEDS = [123, 5, 4295, 99991, (1 << 33) + 9, 7, 31337, (1 << 40) + 3]      # per case
assert len(BASE_SEEDS) == len(CASES) and sum(b * SEED_STEP >= 1 << 32 for b in BASE_SEEDS) >= 1
# (seed, counter) whose draw is x = 0xFFFFFF, u = 1 exactly (found by a search on the CPU; test_u_equal_one_seeds re-checks)
U_ONE = [(6664496, 1), (9451941, 1), (4513832, 3), (8905528, 7)]
X_MAX = 0xFFFFFF


# ---- 1. host restatement (numpy, no GPU) ----------------------------------------------------------------------------

_M32 = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 (Salmon et al., SC'11), vectorised over numpy arrays of 32-bit words; returns the four output words."""
    c0, c1, c2, c3, k0, k1 = (np.asarray(x, dtype=np.uint64) & _M32 for x in (c0, c1, c2, c3, k0, k1))
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> _S32) ^ c1 ^ k0, p1 & _M32, (p0 >> _S32) ^ c3 ^ k1, p0 & _M32
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & _M32, (k1 + np.uint64(0xBB67AE85)) & _M32
    return c0, c1, c2, c3


def draw_u(seed, m0, M, ways):
    """[M, ways] int64: r[0] >> 8 of the blocks k_assign draws for claimants m0 .. m0 + M - 1."""
    seed = int(seed) & ((1 << 64) - 1)
    ctr = np.arange(m0, m0 + M, dtype=np.uint64)[:, None] * np.uint64(ways) + np.arange(ways, dtype=np.uint64)[None, :]
    r0 = philox4x32_10(ctr & _M32, ctr >> _S32, 0x43444c52, 0, seed & 0xFFFFFFFF, seed >> 32)[0]
    return (r0 >> np.uint64(8)).astype(np.int64)


def rank_q(x):
    """q[m, w] = 1 + dense descending rank of x[m, w] within its row (equal x share a rank), float32."""
    order = np.argsort(-x, axis=1, kind="stable")
    s = np.take_along_axis(x, order, 1)
    step = np.concatenate([np.ones((x.shape[0], 1), dtype=np.int64), (s[:, 1:] != s[:, :-1]).astype(np.int64)], 1)
    q = np.empty_like(x)
    np.put_along_axis(q, order, np.cumsum(step, 1), 1)
    return q.astype(np.float32)


class RankQ:
    """The q source of ONE window at `seed`: called table by table, numbers the claimants through."""

    def __init__(self, seed):
        self.seed, self.m0, self.x = seed, 0, []

    def __call__(self, M, ways):
        x = draw_u(self.seed, self.m0, M, ways)
        self.m0 += M
        self.x.append(x)
        return torch.from_numpy(rank_q(x))


def first_max_over_available(x, avail):
    return np.argmax(np.where(avail, x, -1), axis=1)


def claimant_avail(pre_occ, uniq, P):
    """[claimants, ways] bool: the unprotected ways of each claimant's set (main_no_ddp.py:160-177 on the tags the
    window meets), claimants in index order."""
    set_idx = torch.remainder(uniq, P)
    eq = pre_occ[set_idx] == uniq.view(-1, 1)
    hit = eq.any(dim=1)
    avail = torch.ones(pre_occ.shape, dtype=torch.bool)
    avail[set_idx[hit], eq.nonzero(as_tuple=True)[1]] = False
    a = avail[set_idx[~hit]]
    return a[a.any(dim=1)].numpy()


def window_seed(base, w):
    return base * SEED_STEP + w


DrawRef = namedtuple("DrawRef", "fx wins seeds x avail way")


def draw_reference_of(fx, seeds):
    """The oracle over len(seeds) windows of fx with the rank-q source at seeds[w]; per window also the draws x, the
    available ways and the chosen way of every claimant ([M, ways], [M, ways], [M])."""
    ways, T = fx.case.ways, fx.case.T
    srcs = [RankQ(s) for s in seeds]
    wins = oracle_windows(fx, srcs.__getitem__, n_windows=len(seeds))
    xs, avails, chosen = [], [], []
    pre = O.new_occupancy_tables(fx.cache_sizes, ways)
    for w, wr in enumerate(wins):
        a = [claimant_avail(pre[k], wr.uniq[k], fx.cache_sizes[k]) for k in range(T)]
        assert [len(v) for v in a] == wr.kept_n, w
        xs.append(np.concatenate(srcs[w].x))
        avails.append(np.concatenate(a))
        chosen.append(torch.cat(wr.way).numpy())
        pre = wr.occ
    return DrawRef(fx, wins, list(seeds), xs, avails, chosen)


@functools.lru_cache(maxsize=None)
def fixture_of(ci):
    return build_fixture(CASES[ci])


@functools.lru_cache(maxsize=None)
def draw_reference(ci):
    """Shared by every test of the case and never modified."""
    return draw_reference_of(fixture_of(ci), [window_seed(BASE_SEEDS[ci], w) for w in range(N_WINDOWS)])


@pytest.fixture(autouse=True, scope="module")
def _drop_the_references_after_the_module():
    yield
    draw_reference.cache_clear()
    fixture_of.cache_clear()
    seed_word_references.cache_clear()


# ---- 2. CPU tests ---------------------------------------------------------------------------------------------------

def test_philox_known_answer_vectors():
    kat = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
           ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
            (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]
    for ctr, key, want in kat:
        assert tuple(int(v) for v in philox4x32_10(*ctr, *key)) == want
    # vectorised: the three at once
    got = philox4x32_10(*[np.array([k[0][i] for k in kat]) for i in range(4)], *[np.array([k[1][i] for k in kat]) for i in range(2)])
    assert [tuple(int(v[j]) for v in got) for j in range(3)] == [k[2] for k in kat]


def test_u_equal_one_seeds():
    """Each (seed, counter) of U_ONE draws x = 0xFFFFFF -- at any way count that splits the counter as m * ways + w."""
    for seed, ctr in U_ONE:
        assert int(draw_u(seed, 0, ctr + 1, 1)[ctr, 0]) == X_MAX, (seed, ctr)
        for ways in (2, 3, 4):
            m, w = divmod(ctr, ways)
            assert int(draw_u(seed, m, 1, ways)[0, w]) == X_MAX, (seed, ctr, ways)


def test_rank_q_reproduces_the_integer_argmax():
    """Through O.choose_ways, with ties and with every availability pattern of 5 ways: p / rank_q picks the first maximum
    of x over the available ways."""
    rng = np.random.RandomState(0)
    x = rng.randint(0, 6, size=(4000, 5)).astype(np.int64)          # small range: many ties
    avail = rng.rand(4000, 5) < 0.6
    avail[avail.sum(1) == 0, 3] = True
    got = O.choose_ways(torch.from_numpy(avail), torch.from_numpy(rank_q(x))).numpy()
    assert np.array_equal(got, first_max_over_available(x, avail))
    x64 = rng.randint(0, 1 << 24, size=(500, 64)).astype(np.int64)
    a64 = rng.rand(500, 64) < 0.5
    a64[:, 63] = True
    got = O.choose_ways(torch.from_numpy(a64), torch.from_numpy(rank_q(x64))).numpy()
    assert np.array_equal(got, first_max_over_available(x64, a64))


def wilson_hilferty(df, z):
    return df * (1 - 2 / (9 * df) + z * (2 / (9 * df)) ** 0.5) ** 3


@pytest.mark.parametrize("ci", range(len(CASES)), ids=CASE_IDS)
def test_fixture_exercises_the_draw(ci):
    """What the GPU tests rely on, from the reference alone.  Every window: contested slots, and the oracle's way is the
    first maximum of x over the available ways.  Over the case (window 1 meets empty tags, so all of ITS sets have every
    way available; later windows protect their hits): for ways > 1 claimants of sets with fewer than `ways` and with
    exactly `ways` available ways; for ways >= 3 every way number chosen."""
    ref = draw_reference(ci)
    ways = ref.fx.case.ways
    partial = whole = 0
    hist = np.zeros(ways, dtype=np.int64)
    for w in range(N_WINDOWS):
        x, avail, way = ref.x[w], ref.avail[w], ref.way[w]
        assert x.shape == avail.shape == (len(way), ways) and x.min() >= 0 and x.max() <= X_MAX
        assert np.array_equal(way, first_max_over_available(x, avail)), w
        n_av = avail.sum(1)
        contested = ref.wins[w].counts["contested"]
        print(CASE_IDS[ci], "window", w + 1, "seed", ref.seeds[w], "claimants", len(way), "contested", contested,
              "with fewer than all ways", int((n_av < ways).sum()), "ambiguous 0 (integer comparison)")
        assert len(way) > 0 and contested > 0, w
        partial += int((n_av < ways).sum())
        whole += int((n_av == ways).sum())
        hist += np.bincount(way, minlength=ways)
    print(CASE_IDS[ci], "ways chosen", hist.tolist())
    if ways > 1:
        assert partial > 0 and whole > 0
    if ways >= 3:
        assert hist.min() > 0


@pytest.mark.parametrize("ci", [i for i, c in enumerate(CASES) if c.ways > 1], ids=[i for i, c in zip(CASE_IDS, CASES) if c.ways > 1])
def test_reference_draw_is_uniform(ci):
    """The defined draw, pooled over the windows, grouped by the number k >= 2 of available ways: in every group of at least
    50 k claimants the chi-square statistic of the chosen way's rank among the available ones is below the 0.999 quantile of
    chi2(k - 1) (Wilson-Hilferty).  Seeds are fixed, so this is deterministic: a failure says the counter layout favours a
    way (a stride that makes claimants share blocks does), not that another seed is needed."""
    ref = draw_reference(ci)
    avail, way = np.concatenate(ref.avail), np.concatenate(ref.way)
    n_av = avail.sum(1)
    rank = np.cumsum(avail, 1)[np.arange(len(way)), way] - 1
    tested = 0
    for k in range(2, ref.fx.case.ways + 1):
        sel = n_av == k
        n = int(sel.sum())
        if n < 50 * k:
            continue
        obs = np.bincount(rank[sel], minlength=k)
        chi2 = float(((obs - n / k) ** 2).sum() / (n / k))
        bound = wilson_hilferty(k - 1, 3.090232)
        print(CASE_IDS[ci], "k", k, "claimants", n, "chi2", round(chi2, 2), "0.999 quantile", round(bound, 2))
        assert chi2 < bound, k
        tested += 1
    assert tested > 0


# ---- 3. GPU: the kernel at every geometry ------------------------------------------------------------------------------

def device_windows(ops, ref):
    """The reference's windows through the kernels on a fresh state, each at its seed; everything asserted after each."""
    fx = ref.fx
    st = CycleState(ops, fx)
    plan = ops.WindowPlan(st.ctx, fx.case.n_win)
    exp_host = [h.clone() for h in fx.host]
    ways = []
    for w in range(len(ref.wins)):
        _, ko, wo = run_window(st, plan, ref, w, seed=ref.seeds[w])
        assert_window_equals_oracle(st, plan, ref, w, ko, wo, exp_host)
        ways.append(plan.way[:ko[-1]].cpu().long())
    st.ctx.check()
    return ways


@gpu
@pytest.mark.parametrize("ci", range(len(CASES)), ids=CASE_IDS)
def test_device_draw_three_windows_equal_the_oracle(ops, ci):
    """unique -> probe -> assign(None, seed) -> fetch -> commit -> writeback over three windows: after each the unique
    lists, claimant counts, ways, winners, tags, cache rows, evicted (tag, row) set and host tables equal the oracle run on
    the restated draw bit for bit, the aux rows are untouched and the plan's scratch is clean."""
    device_windows(ops, draw_reference(ci))


# ---- 4. GPU: both seed words -------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def seed_word_references():
    s = window_seed(BASE_SEEDS[0], 0)
    return [draw_reference_of(fixture_of(0), [seed]) for seed in (s, s + (1 << 32), s + 1)]


def test_seed_words_change_the_reference():
    a, b, c = [r.way[0] for r in seed_word_references()]
    assert not np.array_equal(a, b) and not np.array_equal(a, c) and not np.array_equal(b, c)


@gpu
def test_both_seed_words_reach_the_draw(ops):
    """26/128/4, window 1, at seeds s, s + 2^32 and s + 1: each equals its own reference, and the three way vectors differ
    pairwise (a dropped upper word would make the first two one draw)."""
    got = [device_windows(ops, r)[0] for r in seed_word_references()]
    assert not torch.equal(got[0], got[1]) and not torch.equal(got[0], got[2]) and not torch.equal(got[1], got[2])


# ---- 5. GPU: the draw u = 1 --------------------------------------------------------------------------------------------

EDGE_TABLES, EDGE_SETS, EDGE_D = [50, 60], [7, 7], 4
EDGE_WINDOW = [[3, 11, 20, 25], [5, 9, 33, 5]]      # claimants 0 1 2 3 | 4 5 6 when the tags are empty
# (ways, seed, counter, protect): the claimant m = counter // ways draws u = 1 at way w = counter % ways.  protect: id 25
# sits in way 0 of claimant 1's set (11 % 7 == 25 % 7) and is in the window, so that way is protected and claimant 1 must
# stay off it whatever it draws there.
EDGE_CASES = [(4, s, c, False) for s, c in U_ONE] + [(2, 4513832, 3, False), (3, 4513832, 3, False), (3, 4513832, 3, True)]


def edge_reference(ways, seed, protect):
    occ = O.new_occupancy_tables(EDGE_SETS, ways)
    if protect:
        occ[0][25 % 7, 0] = 25
    pre = [o.clone() for o in occ]
    host = [torch.zeros(n, EDGE_D) for n in EDGE_TABLES]
    weights = [torch.zeros(ways * p, EDGE_D) for p in EDGE_SETS]
    rows, uniqs, _ = O.process_batch_slice([torch.tensor(r) for r in EDGE_WINDOW], host, build_maps=False)
    src = RankQ(seed)
    _, det = O.cache_embeddings(rows, uniqs, occ, weights, EDGE_SETS, src)
    avail = np.concatenate([claimant_avail(pre[k], uniqs[k], EDGE_SETS[k]) for k in range(2)])
    return pre, torch.cat([d["way"] for d in det]), np.concatenate(src.x), avail


@pytest.mark.parametrize("ways,seed,ctr,protect", EDGE_CASES)
def test_u_equal_one_fixture(ways, seed, ctr, protect):
    """The edge fixture puts x = 0xFFFFFF where it says (the claimant numbering shifts by one when id 25 is a hit)."""
    m, w = divmod(ctr, ways)
    _, way, x, avail = edge_reference(ways, seed, protect)
    assert len(way) == (6 if protect else 7) and int(x[m, w]) == X_MAX
    if protect:
        assert w == 0 and not avail[m, 0] and avail[m, 1:].all() and int(way[m]) != 0
        assert avail.sum() == avail.size - 1
    else:
        assert avail.all() and int(way[m]) == w


@gpu
@pytest.mark.parametrize("ways,seed,ctr,protect", EDGE_CASES)
def test_u_equal_one_wins(ops, ways, seed, ctr, protect):
    """Two tables, D = 4, a window of a few ids: the claimant that draws u = 1 at an available way takes that way (it is
    the largest u there is; at way 0 it is also the first candidate), the one that draws it at a protected way 0 stays off
    that way, and every claimant's way equals the reference."""
    pre, want, _, _ = edge_reference(ways, seed, protect)
    aux = 8
    st = DevState(ops, EDGE_TABLES, EDGE_SETS, EDGE_D, ways, aux, pre, [torch.zeros(ways * p + aux, EDGE_D) for p in EDGE_SETS],
                  [torch.zeros(n, EDGE_D) for n in EDGE_TABLES])
    plan = ops.WindowPlan(st.ctx, len(EDGE_WINDOW[0]))
    plan.unique(torch.tensor(EDGE_WINDOW).to(DEV))
    plan.probe()
    _, ko, _ = plan.offsets()
    assert ko[-1] == want.numel()
    plan.assign(None, seed=seed)
    torch.cuda.synchronize()
    st.ctx.check()
    got = plan.way[:ko[-1]].cpu().long()
    m, w = divmod(ctr, ways)
    assert (int(got[m]) != 0) if protect else (int(got[m]) == w), got.tolist()
    assert torch.equal(got, want), (got.tolist(), want.tolist())


# ---- 6. GPU: the engine's use of the draw --------------------------------------------------------------------------------

ENG_TABLES, ENG_D, ENG_WAYS, ENG_CACHE, ENG_B, ENG_N, ENG_WINDOWS, ENG_SEED = [5000, 40, 20000], 16, 4, 50, 64, 2000, 4, 5


def engine_windows():
    rng = np.random.RandomState(23)
    return [torch.from_numpy(np.stack([(rng.zipf(1.2, size=ENG_N).astype(np.int64) * 2654435761) % n for n in ENG_TABLES]))
            for _ in range(ENG_WINDOWS)]


def engine_oracle(cache_sizes, host, weights, seeds):
    """The oracle over engine_windows() from empty tags, window w at seeds[w]; host / weights are moved in place.
    Returns the tags."""
    occ = O.new_occupancy_tables(cache_sizes, ENG_WAYS)
    for win, seed in zip(engine_windows(), seeds):
        rows, uniqs, _ = O.process_batch_slice(list(win), host, build_maps=False)
        ev, _ = O.cache_embeddings(rows, uniqs, occ, weights, cache_sizes, RankQ(seed))
        O.eviction_writeback(host, ev)
    return occ


def test_engine_fixture_tells_a_repeated_seed():
    """A pipeline that drew every window at window_no 0 would leave other tags than one that counts its windows."""
    P = O.find_next_prime(ENG_CACHE)
    cache_sizes = [min(n, P) for n in ENG_TABLES]
    occs = []
    for seeds in ([window_seed(ENG_SEED, w) for w in range(ENG_WINDOWS)], [window_seed(ENG_SEED, 0)] * ENG_WINDOWS):
        host = [torch.zeros(n, 1) for n in ENG_TABLES]
        occs.append(engine_oracle(cache_sizes, host, [torch.zeros(ENG_WAYS * p, 1) for p in cache_sizes], seeds))
    assert sum(int((a != b).sum()) for a, b in zip(*occs)) > 50


@gpu
@pytest.mark.parametrize("host_gather", [False, True])
def test_pipeline_draws_each_window_at_its_own_seed(ops, host_gather):
    """WindowPipeline(parity_rng=False, seed=5), in-line and host-gather plans: after four planned and committed windows
    the tags, cache rows and host tables equal the oracle run at seeds 5 * 1000003 + {0, 1, 2, 3}."""
    from cdlrm_amd.engine import WindowPipeline
    from cdlrm_amd.model_no_ddp import Embedding_Table_Cache_Group, Embedding_Table_Group
    np.random.seed(3)
    torch.manual_seed(3)
    host = Embedding_Table_Group(ENG_D, np.array(ENG_TABLES)).pin()
    cg = Embedding_Table_Cache_Group(ENG_D, np.array(ENG_TABLES), ENG_CACHE, ENG_B, ENG_WAYS).to(DEV)
    pipe = WindowPipeline(cg, host, ENG_N, parity_rng=False, seed=ENG_SEED, host_gather=host_gather, gather_threads=3)
    assert pipe.host_gather == host_gather
    T, sizes = len(ENG_TABLES), cg.cache_sizes
    assert sizes == [min(n, O.find_next_prime(ENG_CACHE)) for n in ENG_TABLES]
    want_host = [E.weight.data.clone() for E in host.emb_l]
    want_rows = [cg.emb_l[k].weight[:ENG_WAYS * sizes[k]].cpu().clone() for k in range(T)]
    want_occ = engine_oracle(sizes, want_host, want_rows, [window_seed(ENG_SEED, w) for w in range(ENG_WINDOWS)])
    for win in engine_windows():
        pipe.plan_window(win.to(DEV))
        pipe.commit()
        pipe.wait_writeback()
    torch.cuda.synchronize()
    pipe.close()
    cg.ctx.check()
    for k in range(T):
        assert torch.equal(cg.occupancy_tables[k].cpu(), want_occ[k]), k
        assert torch.equal(cg.emb_l[k].weight[:ENG_WAYS * sizes[k]].cpu(), want_rows[k]), k
        assert torch.equal(host.emb_l[k].weight.data, want_host[k]), k
