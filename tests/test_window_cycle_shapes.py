"""The look-ahead cache window cycle against the CPU oracle at every row width and tag-group width.

One fixture builder (plain Python) makes, per case (T, D, ways, P, n_win): table sizes that sit on the bitmap / set-count
edges, three partly overlapping Zipf-like windows that hold the ids 0 and n_rows - 1 of every table, random host tables and
cache rows, empty tags.  The oracle (oracle/cdlrm_oracle.py) runs the three windows on CPU copies once per case; the GPU
tests replay them through the kernels of csrc/window.hip, csrc/scan.hip and the front half of csrc/embbag.hip and compare
bit for bit (integer work and exact row copies), except the multi-hot sum, whose bound is derived below.

The unmarked self-check runs the oracle alone and asserts that every class of index the GPU tests rely on (hits, kept and
contested claimants, evictions, victims, host-fallback misses) is non-empty in every case -- so a fixture that degenerates
fails on any machine, not silently on the GPU one.

Which template instance a case singles out (lanes per row = min(64, max(4, pow2ceil(D / 4))), lanes per tag group =
min(16, pow2ceil(ways))):

    T / D / ways     row movers                      tag probes
    26 / 128 / 4     32 lanes                        4 lanes                      (the training geometry)
    33 / 16 / 1      4 lanes                         1 lane; table searches take a sixth step (T > 32)
    4 / 256 / 16     64 lanes                        16 lanes
    27 / 64 / 64     16 lanes                        16 lanes x 4 trips; `full = ~0` at 64 ways
    5 / 512 / 2      64 lanes x 2 chunk trips        2 lanes
    26 / 32 / 8      8 lanes                         8 lanes
    3 / 4 / 32       4 lanes, 3 of them idle         16 lanes x 2 trips
    6 / 48 / 3       16 lanes, 4 of them idle        4 lanes, 1 of them idle
"""
import functools
import gc
from collections import namedtuple

import numpy as np
import pytest
import torch

from oracle import cdlrm_oracle as O
from test_hip_kernels import DEV, DevState

gpu = pytest.mark.gpu

SIZES = [7, 64, 65, 4096, 65536, 65537, 70000, 131072, 1000, 300]
BATCH_LENS = (1, 63, 64, 65, 2500)
AUX = max(BATCH_LENS)          # >= every batch (and every padded resolve segment): the aux region never overflows
N_WINDOWS = 3
RANK_SHIFT = 37                # Zipf ranks move by this much per window: consecutive windows overlap only partly

Case = namedtuple("Case", "T D ways P n_win tables seed")
CASES = [
    Case(26, 128, 4, 521, 6000, None, 1),
    Case(33, 16, 1, 61, 3000, None, 2),
    Case(4, 256, 16, 127, 9000, None, 3),
    Case(27, 64, 64, 13, 3000, None, 4),
    Case(5, 512, 2, 1031, 20000, None, 5),
    Case(26, 32, 8, 257, 5000, None, 6),
    Case(3, 4, 32, 31, 4000, (65536, 70000, 4096), 7),       # the cache must be smaller than the window
    Case(6, 48, 3, 127, 4000, None, 8),
]
CASE_IDS = ["%d-%d-%d" % (c.T, c.D, c.ways) for c in CASES]
BY_POSITION_CASES = (0, 7)                                   # 32-lane and 16-lane (idle lanes) k_fetch / gather_rows
MULTIHOT_CASES = [i for i, c in enumerate(CASES) if c.D in (4, 48, 128, 512)]


# ---- 1. fixture builder (no GPU) -----------------------------------------------------------------------------------

def table_sizes(case):
    return list(case.tables) if case.tables else [SIZES[i % len(SIZES)] for i in range(case.T)]


def zipf_ids(rng, n_rows, count, shift):
    """Zipf-like ranks, moved by `shift`, scrambled over the table by a multiplicative hash."""
    r = rng.zipf(1.15, size=count).astype(np.int64) % (1 << 30)
    return (r + shift) * 2654435761 % n_rows


Fixture = namedtuple("Fixture", "case ln_emb cache_sizes windows host weight0 batches")


def build_fixture(case):
    T, D, ways, P = case.T, case.D, case.ways, case.P
    assert O.is_prime_ref(P) and all(P % f for f in range(2, P))
    ln_emb = table_sizes(case)
    cache_sizes = [min(P, n) for n in ln_emb]
    rng = np.random.RandomState(case.seed)
    gen = torch.Generator().manual_seed(case.seed)
    windows = []
    for w in range(N_WINDOWS):
        win = np.empty((T, case.n_win), dtype=np.int64)
        for k, n in enumerate(ln_emb):
            win[k] = zipf_ids(rng, n, case.n_win, w * RANK_SHIFT)
            win[k, 0], win[k, -1] = 0, n - 1
        windows.append(torch.from_numpy(win))
    host = [torch.rand(n, D, generator=gen) - 0.5 for n in ln_emb]
    weight0 = [torch.rand(ways * p + 2 * AUX, D, generator=gen) - 0.5 for p in cache_sizes]
    # per-iteration lookups on the state window 2 leaves: half from window 2, a quarter from window 1 (partly evicted by
    # now), a quarter uniform over the table (outside both windows: host fallback); shuffled so the classes interleave
    batches = []
    for B in BATCH_LENS:
        b = np.empty((T, B), dtype=np.int64)
        n1 = B // 4
        nu = B // 4
        for k, n in enumerate(ln_emb):
            parts = [rng.choice(windows[1][k].numpy(), B - n1 - nu), rng.choice(windows[0][k].numpy(), n1),
                     rng.randint(0, n, nu)]
            b[k] = rng.permutation(np.concatenate(parts))
        batches.append(torch.from_numpy(b))
    return Fixture(case, ln_emb, cache_sizes, windows, host, weight0, batches)


# ---- the oracle's run of the three windows, once per case ------------------------------------------------------------

WindowRef = namedtuple("WindowRef", "uniq q way kept_n win_idx victims victim_pos ev occ weight host_delta counts")
Reference = namedtuple("Reference", "fx wins")


def oracle_windows(fx, q_source_of, n_windows=N_WINDOWS):
    """The oracle over the fixture's first n_windows windows, on copies; q_source_of(w) is window w's q source
    (O.cache_embeddings calls it table by table).  One WindowRef per window."""
    case, T, ways = fx.case, fx.case.T, fx.case.ways
    host = [h.clone() for h in fx.host]
    occ = O.new_occupancy_tables(fx.cache_sizes, ways)
    weights = [fx.weight0[k][:ways * fx.cache_sizes[k]].clone() for k in range(T)]
    wins = []
    for w in range(n_windows):
        pre = [o.clone() for o in occ]
        rows, uniqs, _ = O.process_batch_slice([fx.windows[w][k] for k in range(T)], host, build_maps=False)
        ev, det = O.cache_embeddings(rows, uniqs, occ, weights, fx.cache_sizes, q_source_of(w))
        O.eviction_writeback(host, ev, average_on_writeback=(w == N_WINDOWS - 1))
        win_idx, victims, victim_pos, evd, delta = [], [], [], [], []
        counts = dict(hits=0, kept=0, contested=0, evictions=0, victims=0)
        flat0 = 0
        for k in range(T):
            u, d = uniqs[k], det[k]
            s = d["slots"].numpy()
            _, first_in_rev = np.unique(s[::-1], return_index=True)
            wi = d["kept_idx"][torch.from_numpy(np.sort(len(s) - 1 - first_in_rev))]
            hit = torch.isin(u, pre[k][pre[k] != -1])
            vm = ~hit & ~torch.isin(u, wi)
            win_idx.append(wi)
            victims.append(u[vm])
            victim_pos.append(flat0 + vm.nonzero().flatten())
            flat0 += u.numel()
            di, dr = O.dedup_evictions(*ev[k])
            evd.append((di, dr))
            delta.append((di, host[k][di].clone()))
            counts["hits"] += int(hit.sum())
            counts["kept"] += len(s)
            counts["contested"] += len(s) - wi.numel()
            counts["evictions"] += di.numel()
            counts["victims"] += int(vm.sum())
        wins.append(WindowRef(uniqs, [d["q"] for d in det], [d["way"] for d in det], [len(d["way"]) for d in det], win_idx,
                              victims, victim_pos, evd, [o.clone() for o in occ], [x.clone() for x in weights], delta, counts))
    return wins


@functools.lru_cache(maxsize=None)
def reference(ci):
    """Fixture + what the oracle leaves after each window.  Shared by every test of the case and never modified."""
    fx = build_fixture(CASES[ci])
    gen = torch.Generator().manual_seed(1000 + fx.case.seed)
    return Reference(fx, oracle_windows(fx, lambda w: lambda M, wy: O.draw_q(M, wy, gen)))


def host_after(ref, n_windows):
    """The oracle's host tables after the first n_windows windows (fresh copies)."""
    host = [h.clone() for h in ref.fx.host]
    for w in range(n_windows):
        for k, (di, rows) in enumerate(ref.wins[w].host_delta):
            host[k][di] = rows
    return host


def batch_classes(ref, j):
    """(hits, misses the window-2 victim list holds, misses outside it) of batch j on the state window 2 leaves."""
    w2 = ref.wins[1]
    hits = listed = other = 0
    for k in range(ref.fx.case.T):
        idx = ref.fx.batches[j][k]
        _, miss_pos, miss_idx = O.probe_table(w2.occ[k], idx, ref.fx.cache_sizes[k])
        in_list = torch.isin(miss_idx, w2.victims[k])
        hits += idx.numel() - miss_pos.numel()
        listed += int(in_list.sum())
        other += int((~in_list).sum())
    return hits, listed, other


# ---- 5. CPU self-check: every class the GPU tests rely on is there ----------------------------------------------------------

@pytest.mark.parametrize("ci", range(len(CASES)), ids=CASE_IDS)
def test_fixture_exercises_every_class(ci):
    ref = reference(ci)
    case, fx = ref.fx.case, ref.fx
    for k, n in enumerate(fx.ln_emb):
        for w in range(N_WINDOWS):
            assert ref.wins[w].uniq[k][0] == 0 and ref.wins[w].uniq[k][-1] == n - 1
    for name in ("hits", "kept", "contested", "evictions", "victims"):
        got = sum(ref.wins[w].counts[name] for w in (1, 2))
        print(CASE_IDS[ci], name, got)
        assert got > 0, name
    assert ref.wins[1].counts["victims"] > 1, "window 2 must leave a victim list that can be cut in half"
    if case.D == 512:
        for w in range(N_WINDOWS):
            assert max(u.numel() for u in ref.wins[w].uniq) > 4096
    for j, B in enumerate(BATCH_LENS):
        if B >= 63:
            hits, listed, other = batch_classes(ref, j)
            print(CASE_IDS[ci], "B", B, "hits", hits, "victim misses", listed, "host misses", other)
            assert hits > 0 and listed > 0 and other > 0
    # consecutive windows overlap, and only partly
    for k in range(case.T):
        if fx.ln_emb[k] >= 65536:
            a, b = ref.wins[0].uniq[k], ref.wins[1].uniq[k]
            common = int(torch.isin(a, b).sum())
            assert 0 < common < min(a.numel(), b.numel())


# ---- device side ----------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def ops():
    from cdlrm_amd import ops as _ops
    from cdlrm_amd import _lib
    _lib.lib()
    return _ops


class CycleState(DevState):
    """DevState with two aux regions per table (aux_phase 0 / 1)."""

    def __init__(self, ops, fx):
        c = fx.case
        self.ops = ops
        self.ctx = ops.CacheCtx(fx.ln_emb, fx.cache_sizes, c.D, c.ways, AUX, torch.device(DEV), aux_phases=2)
        self.tags = torch.cat([o.reshape(-1) for o in O.new_occupancy_tables(fx.cache_sizes, c.ways)]).to(DEV)
        self.weight = torch.cat(fx.weight0).contiguous().to(DEV)
        self.ctx.bind_cache(self.tags, self.weight)
        self.host = [h.clone().pin_memory() for h in fx.host]
        self.ctx.bind_host_tables([h.data_ptr() for h in self.host])
        self.cache_sizes, self.ways = list(fx.cache_sizes), c.ways
        self.host_ptrs = [h.data_ptr() for h in self.host]


@pytest.fixture(autouse=True, scope="module")
def _drop_the_references_after_the_module():
    yield
    reference.cache_clear()


@pytest.fixture(autouse=True)
def _free_the_case_before_the_next():
    """Pinned host tables and cache buffers of one case go back before the next case allocates its own."""
    yield
    gc.collect()
    if torch.cuda.is_available() and torch.cuda.is_initialized():
        torch.cuda.empty_cache()
        empty_host = getattr(torch._C, "_host_emptyCache", None)
        if empty_host is not None:
            empty_host()


def run_window(st, plan, ref, w, by_position=False, victims=(), seed=None):
    """One window on the device, with the oracle's q (seed given: with the device's own draw at that seed instead).  The
    unique lists and the claimant counts are asserted on the way (the q tensor only fits when they are right).  Returns
    (uniq_off, kept_off, win_off)."""
    ops, fx, wr = st.ops, ref.fx, ref.wins[w]
    T, D, ways = fx.case.T, fx.case.D, fx.case.ways
    plan.unique(fx.windows[w].to(DEV))
    plan.probe()
    uo, ko, _ = plan.offsets()
    assert uo == np.cumsum([0] + [u.numel() for u in wr.uniq]).tolist(), w
    assert torch.equal(plan.uniq[:uo[T]].cpu(), torch.cat(wr.uniq)), w
    assert [ko[k + 1] - ko[k] for k in range(T)] == wr.kept_n, w
    if seed is None:
        plan.assign(torch.cat([q.reshape(-1, ways) for q in wr.q]).contiguous().to(DEV))
    else:
        plan.assign(None, seed=seed)
    if by_position:
        rows = [ops.gather_rows(st.host_ptrs[k], plan.uniq[uo[k]:uo[k + 1]], D) for k in range(T)]
        for k in range(T):
            assert torch.equal(rows[k].cpu(), st.host[k][wr.uniq[k]]), (w, k)
        plan.fetch([r.data_ptr() for r in rows], True)
    else:
        plan.fetch(st.host_ptrs, False)
    for v in victims:
        plan.victims(v)
    plan.commit()
    plan.writeback(st.host_ptrs, w == N_WINDOWS - 1)
    _, _, wo = plan.offsets()
    torch.cuda.synchronize()
    st.ctx.check()
    return uo, ko, wo


# ---- 2. plan + row movement against the oracle ---------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("ci,by_position", [(i, False) for i in range(len(CASES))] + [(i, True) for i in BY_POSITION_CASES],
                         ids=CASE_IDS + [CASE_IDS[i] + "-by_position" for i in BY_POSITION_CASES])
def test_three_windows_equal_the_oracle(ops, ci, by_position):
    """unique -> probe -> assign(q) -> fetch -> commit -> writeback over three consecutive windows; after each one the
    unique lists, claimant counts, ways, tags, cache rows, evicted (tag, row) set and host tables equal the oracle's, bit
    for bit, and the plan's scratch is clean.  Window 3 writes back with average=True: (h + v) / 2 is one correctly rounded
    fp32 addition and an exact halving on both sides."""
    ref = reference(ci)
    fx = ref.fx
    st = CycleState(ops, fx)
    plan = ops.WindowPlan(st.ctx, fx.case.n_win)
    exp_host = [h.clone() for h in fx.host]
    for w in range(N_WINDOWS):
        _, ko, wo = run_window(st, plan, ref, w, by_position)
        assert_window_equals_oracle(st, plan, ref, w, ko, wo, exp_host)
    st.ctx.check()


def assert_window_equals_oracle(st, plan, ref, w, ko, wo, exp_host):
    """After run_window(w): ways, winners, tags, cache rows, the evicted (tag, row) set and the host tables equal the oracle's
    window w bit for bit, the aux rows are untouched and the plan's scratch is clean.  exp_host (the oracle's host tables
    before the window) moves on to the state after it."""
    fx, wr = ref.fx, ref.wins[w]
    T, ways = fx.case.T, fx.case.ways
    way, tags, weight = plan.way[:ko[T]].cpu().long(), st.tags.cpu(), st.weight.cpu()
    ev_tag, ev_rows = plan.ev_tag[:wo[T]].cpu(), plan.stage[:wo[T]].cpu()
    c = st.ctx
    for k in range(T):
        assert wo[k + 1] - wo[k] == wr.win_idx[k].numel(), (w, k)
        assert torch.equal(way[ko[k]:ko[k + 1]], wr.way[k]), (w, k)
        assert torch.equal(tags[c.tag_base[k]:c.tag_base[k + 1]].view(-1, ways), wr.occ[k]), (w, k)
        nslots = ways * fx.cache_sizes[k]
        assert torch.equal(weight[c.row_base[k]:c.row_base[k] + nslots], wr.weight[k]), (w, k)
        # the aux rows are not the window path's to touch
        assert torch.equal(weight[c.row_base[k] + nslots:c.row_base[k + 1]], fx.weight0[k][nslots:]), (w, k)
        et, er = ev_tag[wo[k]:wo[k + 1]], ev_rows[wo[k]:wo[k + 1]]
        valid = et != -1
        mi, mr = O.dedup_evictions(et[valid], er[valid])
        assert torch.equal(mi, wr.ev[k][0]) and torch.equal(mr, wr.ev[k][1]), (w, k)
        di, rows = wr.host_delta[k]
        exp_host[k][di] = rows
        assert torch.equal(st.host[k], exp_host[k]), (w, k)
    assert torch.equal(plan.win_idx[:wo[T]].cpu(), torch.cat(wr.win_idx)), w
    assert int((plan.winner != -1).sum()) == 0 and int(plan.prot.abs().sum()) == 0, w
    assert int(plan.bitmap.abs().sum()) == 0, w


# ---- 3. per-iteration path on the state window 2 left ---------------------------------------------------------------------

def two_windows(ops, ref, with_victims):
    """Device state after window 2's commit and write-back, checked against the oracle's; with_victims: window 2's victim
    lists at cap = total and cap = total // 2 as well."""
    fx, T = ref.fx, ref.fx.case.T
    st = CycleState(ops, fx)
    plan = ops.WindowPlan(st.ctx, fx.case.n_win)
    run_window(st, plan, ref, 0)
    total = sum(v.numel() for v in ref.wins[1].victims)
    vics = [ops.Victims(st.ctx, cap) for cap in (total, total // 2)] if with_victims else []
    run_window(st, plan, ref, 1, victims=vics)
    w2 = ref.wins[1]
    assert torch.equal(st.tags.cpu(), torch.cat([o.reshape(-1) for o in w2.occ]))
    host2 = host_after(ref, 2)
    for k in range(T):
        assert torch.equal(st.w(k)[:st.ways * fx.cache_sizes[k]], w2.weight[k]), k
        assert torch.equal(st.host[k], host2[k]), k
    return st, plan, vics, host2


def check_victim_list(ref, vic, host2):
    """idx, pos, off, rows and the un-capped length equal unique - resident - winners, cut at the list's capacity."""
    w2, T = ref.wins[1], ref.fx.case.T
    total = sum(v.numel() for v in w2.victims)
    cap = vic.cap
    off = vic.off.cpu().tolist()
    assert off[T] == min(total, cap) and off[T + 1] == total
    assert torch.equal(vic.idx[:off[T]].cpu(), torch.cat(w2.victims)[:cap])
    assert torch.equal(vic.pos[:off[T]].cpu().long(), torch.cat(w2.victim_pos)[:cap])
    rows = vic.rows[:off[T]].cpu()
    lo = 0
    for k in range(T):
        hi = min(cap, lo + w2.victims[k].numel())
        assert off[k] == lo, k
        assert torch.equal(rows[lo:hi], host2[k][w2.victims[k][:hi - lo]]), k
        lo = hi


@gpu
@pytest.mark.parametrize("ci", range(len(CASES)), ids=CASE_IDS)
def test_per_iteration_path_equals_the_oracle(ops, ci):
    """On the state window 2 leaves, for B in BATCH_LENS and both aux phases: slot ids, miss positions and counts, the aux
    rows written (and every other cache row left alone) and the one-index-per-bag gather equal O.cache_forward -- from
    embbag_probe with no victims bound, with window 2's victim list bound (whole, and cut in half), and from
    window_resolve (once over the five batches, one AUX-long segment each) + embbag_take per batch."""
    ref = reference(ci)
    fx, T, D, ways = ref.fx, ref.fx.case.T, ref.fx.case.D, ref.fx.case.ways
    st, plan, vics, host2 = two_windows(ops, ref, True)
    ctx = st.ctx
    for v in vics:
        check_victim_list(ref, v, host2)
    w2 = ref.wins[1]
    first_aux = [ways * p for p in fx.cache_sizes]
    wiped = st.weight.clone()
    for k in range(T):
        wiped[ctx.row_base[k] + first_aux[k]:ctx.row_base[k + 1]] = -7.0
    # the five batches end to end, one segment of AUX lookups each (the tail of a segment repeats the batch's first id)
    seg = AUX
    look = torch.cat([torch.cat([b, b[:, :1].expand(T, seg - b.shape[1])], 1) for b in fx.batches], 1).contiguous().to(DEV)
    resolved = []
    for v in [None] + vics:
        ctx.bind_victims(v)
        ws = torch.empty(T, look.shape[1], dtype=torch.int32, device=DEV)
        wsrc = torch.empty_like(ws)
        ops.window_resolve(ctx, look, seg, ws, wsrc)
        resolved.append((v, ws, wsrc))
    torch.cuda.synchronize()
    weights_o = [torch.cat([w2.weight[k], torch.zeros(AUX, D)]) for k in range(T)]
    for j, B in enumerate(BATCH_LENS):
        idx = fx.batches[j]
        ly, cg = O.cache_forward(w2.occ, weights_o, fx.cache_sizes, [torch.arange(B)] * T, [idx[k] for k in range(T)], host2)
        slots0 = torch.stack(cg)
        miss = torch.stack([cg[k] >= first_aux[k] for k in range(T)])
        miss_pos = [miss[k].nonzero().flatten() for k in range(T)]
        assert all(int(m.numel()) <= AUX for m in miss_pos)
        exp_feat = torch.stack(ly, 1).to(DEV)
        idx_dev = look[:, j * seg:j * seg + B]
        for phase in (0, 1):
            exp_slots = (slots0 + miss.to(torch.int32) * (phase * AUX)).to(DEV)
            exp_weight = wiped.clone()
            for k in range(T):
                a0 = ctx.row_base[k] + first_aux[k] + phase * AUX
                exp_weight[a0:a0 + miss_pos[k].numel()] = host2[k][idx[k][miss_pos[k]]].to(DEV)
            for v, ws, wsrc in resolved:
                what = (B, phase, None if v is None else v.cap)
                ctx.bind_victims(v)
                st.weight.copy_(wiped)
                slots, mp, mc = ops.embbag_probe(ctx, idx_dev, aux_phase=phase)
                torch.cuda.synchronize()
                assert torch.equal(slots, exp_slots), what
                assert mc.cpu().tolist() == [m.numel() for m in miss_pos], what
                mp = mp.cpu()
                for k in range(T):
                    assert torch.equal(mp[k, :miss_pos[k].numel()].long(), miss_pos[k]), what + (k,)
                assert torch.equal(st.weight, exp_weight), what
                if v is None:
                    feat = torch.full((B, T, D), 3.0, device=DEV)
                    ops.embbag_fwd(ctx, slots, None, feat, T * D, D)
                    torch.cuda.synchronize()
                    assert torch.equal(feat, exp_feat), what
                st.weight.copy_(wiped)
                taken = torch.empty(T, B, dtype=torch.int32, device=DEV)
                ops.embbag_take(ctx, idx_dev, ws[:, j * seg:j * seg + B], wsrc[:, j * seg:j * seg + B], taken, aux_phase=phase)
                torch.cuda.synchronize()
                assert torch.equal(taken, exp_slots), what
                assert torch.equal(st.weight, exp_weight), what
    ctx.bind_victims(None)
    ctx.check()


def bag_offsets(rng, T, n, n_bags):
    """[T, n_bags] bag starts over n lookups: lengths 0 .. 9, the first and the last bag empty."""
    off = np.empty((T, n_bags), dtype=np.int64)
    for k in range(T):
        ln = rng.randint(0, 10, size=n_bags)
        ln[0] = ln[-1] = 0
        while ln.sum() != n:
            b = rng.randint(1, n_bags - 1)
            if ln.sum() < n and ln[b] < 9:
                ln[b] += 1
            elif ln.sum() > n and ln[b] > 0:
                ln[b] -= 1
        off[k] = np.cumsum(ln) - ln
    return off


@gpu
@pytest.mark.parametrize("ci", MULTIHOT_CASES, ids=[CASE_IDS[i] for i in MULTIHOT_CASES])
def test_multihot_bags_against_fp64(ops, ci):
    """k_embbag_fwd_bags over the slots of the B = 2500 batch (cache and aux rows), bags of 0 .. 9 lookups with empty first
    and last bags, against an fp64 sum.  The kernel adds a bag's L rows in lookup order in fp32; the error of such a
    recursive sum is at most (L - 1) * 2^-24 * sum |row_i| per element (Rump 2012, no higher-order term), and the first
    addition (0 + row) is exact -- so bags of at most one lookup are exact.  A CPU fp32 sum in the same order has to pass the
    same check."""
    ref = reference(ci)
    fx, T, D = ref.fx, ref.fx.case.T, ref.fx.case.D
    st, plan, _, _ = two_windows(ops, ref, False)
    n = BATCH_LENS[-1]
    slots, _, _ = ops.embbag_probe(st.ctx, fx.batches[-1].to(DEV))
    n_bags = 600
    off = bag_offsets(np.random.RandomState(100 + ci), T, n, n_bags)
    out = torch.full((n_bags, T, D), 3.0, device=DEV)
    ops.embbag_fwd(st.ctx, slots, torch.from_numpy(off).to(DEV), out, T * D, D)
    torch.cuda.synchronize()
    st.ctx.check()
    out, slots, weight = out.cpu(), slots.cpu().long(), st.weight.cpu()
    seen = set()
    for k in range(T):
        ln = np.diff(np.append(off[k], n))
        seen |= set(ln.tolist())
        rows = weight[st.ctx.row_base[k] + slots[k]]
        bag = torch.from_numpy(np.repeat(np.arange(n_bags), ln))
        ref64 = torch.zeros(n_bags, D, dtype=torch.float64).index_add_(0, bag, rows.double())
        mag = torch.zeros(n_bags, D, dtype=torch.float64).index_add_(0, bag, rows.double().abs())
        L = torch.from_numpy(ln).double().view(-1, 1)
        bound = (L - 1).clamp(min=0) * 2.0 ** -24 * mag
        seq = torch.zeros(n_bags, D)
        for p in range(int(ln.max())):
            has = torch.from_numpy(ln > p)
            seq[has] = seq[has] + rows[torch.from_numpy(off[k] + p)[has]]
        for name, got in (("cpu fp32", seq), ("kernel", out[:, k, :])):
            err = (got.double() - ref64).abs()
            assert bool((err <= bound).all()), (name, k, float((err - bound).max()))
        assert torch.equal(out[ln == 0, k, :], torch.zeros(int((ln == 0).sum()), D)), k
        assert torch.equal(out[ln == 1, k, :], rows[torch.from_numpy(off[k])[ln == 1]]), k
    assert seen == set(range(10))


# ---- 4. the unique scan alone at full table size ----------------------------------------------------------------------------

@gpu
def test_unique_scan_at_full_table_size(ops):
    """Tables of 39 884 406, 65 536 * 1024 (exactly 1024 bitmap blocks) and 3 rows: 1634 block sums, so the single-workgroup
    scan of the sums takes a second 1024-wide trip and carries across it.  Twice on one plan; the bitmap is zero after each."""
    ln_emb = [39_884_406, 65_536 * 1024, 3]
    T, n_win = len(ln_emb), 50_000
    ctx = ops.CacheCtx(ln_emb, [7, 7, 3], 4, 1, 1, torch.device(DEV))
    assert ctx.total_bm_words // 1024 > 1024 and ctx.bm_words[1] == 1024 * 1024
    plan = ops.WindowPlan(ctx, n_win)
    rng = np.random.RandomState(9)
    for rep in range(2):
        win = np.stack([rng.randint(0, n, size=n_win) for n in ln_emb])
        win[:, 0] = 0
        win[:, -1] = np.array(ln_emb) - 1
        plan.unique(torch.from_numpy(win).to(DEV))
        uo, _, _ = plan.offsets()
        ctx.check()
        want = [np.unique(win[k]) for k in range(T)]
        assert uo == np.cumsum([0] + [len(u) for u in want]).tolist(), rep
        assert torch.equal(plan.uniq[:uo[T]].cpu(), torch.from_numpy(np.concatenate(want))), rep
        assert int(plan.bitmap.count_nonzero()) == 0, rep
