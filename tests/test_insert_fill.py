"""The "fill" insert policy on the MI355X (cdlrm_plan_count_* / cdlrm_plan_assign_fill, WindowPipeline(insert_policy="fill"),
--insert-policy=fill) against its numpy restatement (tests/fill_policy_restated.py), bit for bit: the policy draws no random
number, so every list, tag and row has one right value."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import fill_policy_restated as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ops():
    from cdlrm_amd import ops as _ops
    from cdlrm_amd import _lib
    _lib.lib()
    return _ops


def host_row(k, v, D):
    """Host row v of table k: a value nothing else holds (exact in fp32)."""
    return (np.asarray(v, dtype=np.int64)[:, None] * 8 + np.arange(D)[None, :] % 8 + k * 262144).astype(np.float32)


class State:
    """Flat device cache state for per-table numpy tags [P, ways]; rows of resident tags hold host row + 0.5 (a trained
    row: its write-back is visible in the host table).  host=False: no host tables (plans that move no rows)."""

    def __init__(self, ops, ln_emb, tags, D, aux=8, host=True):
        self.ops, self.ln_emb, self.D = ops, list(ln_emb), D
        self.sets = [t.shape[0] for t in tags]
        self.ways = tags[0].shape[1]
        self.ctx = ops.CacheCtx(self.ln_emb, self.sets, D, self.ways, aux, torch.device(DEV))
        c = self.ctx
        self.tags = torch.from_numpy(np.concatenate([t.reshape(-1) for t in tags])).to(DEV)
        w = np.zeros((c.total_rows, D), dtype=np.float32)
        for k, t in enumerate(tags):
            s, y = np.nonzero(t != -1)
            w[c.row_base[k] + self.sets[k] * y + s] = host_row(k, t[s, y], D) + 0.5
        self.weight_np = w                                   # the mirror the restatement moves rows in
        self.weight = torch.from_numpy(w).to(DEV)
        c.bind_cache(self.tags, self.weight)
        self.host = self.host_np = None
        if host:
            self.host_np = [host_row(k, np.arange(n), D) for k, n in enumerate(self.ln_emb)]
            self.host = [torch.from_numpy(h.copy()).pin_memory() for h in self.host_np]
            self.ptrs = [h.data_ptr() for h in self.host]
            c.bind_host_tables(self.ptrs)

    def tags_of(self, k):
        c = self.ctx
        return self.tags[c.tag_base[k]:c.tag_base[k + 1]].view(self.sets[k], self.ways).cpu().numpy()


def fill_plan(plan, idx, use_counts=True):
    plan.unique(idx)
    plan.probe()
    if use_counts:
        plan.count_reset()
        plan.count_add(idx)
    plan.assign_fill(use_counts=use_counts)


def check_scratch_clean(plan):
    torch.cuda.synchronize()
    assert int((plan.claim != 0).sum()) == 0, "claim words left behind"
    assert int((plan.winner != -1).sum()) == 0, "winner scratch left behind"
    assert int((plan.prot != 0).sum()) == 0, "prot left behind"


def check_lists(st, plan, per, prot_before=None):
    """way, kept and the winner lists of `plan` against one window's restated plans `per` (one dict per table)."""
    c, T, ways = st.ctx, st.ctx.T, st.ways
    uo, ko, wo = plan.offsets()
    assert [uo[k + 1] - uo[k] for k in range(T)] == [len(r["uniq"]) for r in per]
    assert np.array_equal(plan.uniq[:uo[T]].cpu().numpy(), np.concatenate([r["uniq"] for r in per]))
    assert [ko[k + 1] - ko[k] for k in range(T)] == [len(r["plan"]["kept"]) for r in per]
    assert np.array_equal(plan.kept[:ko[T]].cpu().numpy(), np.concatenate([uo[k] + r["plan"]["kept"] for k, r in enumerate(per)]))
    assert [wo[k + 1] - wo[k] for k in range(T)] == [len(r["winners"]) for r in per]
    way = plan.way[:ko[T]].cpu().numpy().astype(np.int64)
    for k, r in enumerate(per):
        p, wk = r["plan"], way[ko[k]:ko[k + 1]]
        assert np.array_equal(wk[p["placed"]], p["way"][p["placed"]]), k
        # a claimant that is not inserted carries a way of its set that another claimant won: every unprotected way of its
        # set is taken (it would have been placed otherwise), so any of them will do
        lost = ~p["placed"]
        assert not p["prot"][p["sets"][lost], wk[lost]].any(), k
    want_claim = np.concatenate([ko[k] + r["winners"] for k, r in enumerate(per)])
    assert np.array_equal(plan.win_claim[:wo[T]].cpu().numpy(), want_claim)
    want_idx = np.concatenate([r["plan"]["idx"][r["winners"]] for r in per])
    want_row = np.concatenate([c.row_base[k] + st.sets[k] * r["plan"]["way"][r["winners"]] + r["plan"]["sets"][r["winners"]]
                               for k, r in enumerate(per)])
    want_tag = np.concatenate([c.tag_base[k] + r["plan"]["sets"][r["winners"]] * ways + r["plan"]["way"][r["winners"]]
                               for k, r in enumerate(per)])
    assert np.array_equal(plan.win_idx[:wo[T]].cpu().numpy(), want_idx)
    assert np.array_equal(plan.win_row[:wo[T]].cpu().numpy(), want_row)
    assert np.array_equal(plan.win_tag[:wo[T]].cpu().numpy(), want_tag)
    return uo, ko, wo, want_row


_restated = {}


def restated(ways, use_counts=True):
    """The restatement over the shared windows: computed once per number of ways, never changed afterwards."""
    key = (ways, use_counts)
    if key not in _restated:
        if "wins" not in _restated:
            _restated["wins"] = R.windows()
        _restated[key] = R.run_windows(R.initial_tags(ways), _restated["wins"], use_counts=use_counts)
    return _restated["wins"], _restated[key]


@pytest.mark.parametrize("strided", [False, True])
@pytest.mark.parametrize("ways", [1, 3, 16, 64])
def test_three_windows_bit_exact(ops, ways, strided):
    """Three consecutive windows [3, 300 000] (fill_policy_restated.windows: a table that only hits, the 65 534 .. 70 000
    counts in one set, more claimants than slots) through unique / probe / count / assign_fill / fetch / victims / commit /
    writeback: lists, tags, the inserted cache rows, the rows written back to the host tables and the victim list."""
    wins, want = restated(ways)
    D, T = 8, 3
    st = State(ops, R.LN_EMB, R.initial_tags(ways), D)
    c = st.ctx
    plan = ops.WindowPlan(c, R.N_WIN)
    vic = ops.Victims(c, plan.cap_uniq)
    for w, (win, per) in enumerate(zip(wins, want)):
        if strided:
            buf = torch.full((T, R.N_WIN + 13), -5, dtype=torch.int64, device=DEV)      # (a read of the padding would flag an error)
            idx = buf[:, 3:3 + R.N_WIN]
            idx.copy_(torch.from_numpy(win))
            assert idx.stride(0) > idx.shape[1]
        else:
            idx = torch.from_numpy(win).to(DEV)
        fill_plan(plan, idx)
        plan.fetch(st.ptrs, False)
        plan.victims(vic)
        uo, ko, wo, rows = check_lists(st, plan, per)
        plan.commit()
        plan.writeback(st.ptrs, False)
        check_scratch_clean(plan)
        c.check()
        # counters: exact below the clamp, anything >= 65 535 at or above it
        cnt = plan.count[:uo[T]].cpu().numpy().astype(np.int64)
        want_cnt = np.concatenate([R.window_counts(r["uniq"], win[k], R.LN_EMB[k]) for k, r in enumerate(per)])
        assert np.array_equal(np.minimum(cnt, R.CLAMP), np.minimum(want_cnt, R.CLAMP)), w
        # the mirror: evicted rows go to the host table, the winners' host rows come in
        ev = plan.ev_tag[:wo[T]].cpu().numpy()
        assert np.array_equal(ev, np.concatenate([r["evicted"] for r in per])), w
        for k, r in enumerate(per):
            rk = rows[wo[k]:wo[k + 1]]
            old = r["evicted"]
            st.host_np[k][old[old != -1]] = st.weight_np[rk[old != -1]]
            st.weight_np[rk] = st.host_np[k][r["plan"]["idx"][r["winners"]]]
            assert np.array_equal(st.tags_of(k), r["tags"]), (w, k)
            assert np.array_equal(st.host[k].numpy(), st.host_np[k]), (w, k)
        assert np.array_equal(st.weight.cpu().numpy(), st.weight_np), w
        voff = vic.off.cpu().numpy()
        assert [int(voff[k + 1] - voff[k]) for k in range(T)] == [len(r["victims"]) for r in per] and voff[T + 1] == voff[T]
        assert np.array_equal(vic.pos[:voff[T]].cpu().numpy(), np.concatenate([uo[k] + r["victims"] for k, r in enumerate(per)]))
        assert np.array_equal(vic.idx[:voff[T]].cpu().numpy(), np.concatenate([r["uniq"][r["victims"]] for r in per]))
        want_rows = np.concatenate([st.host_np[k][r["uniq"][r["victims"]]] for k, r in enumerate(per)])
        assert np.array_equal(vic.rows[:voff[T]].cpu().numpy(), want_rows), w      # (a victim is not resident: no write-back touches it)
    if ways <= 16:      # table 2 had more claimants than the plan has winner slots for it
        assert len(want[0][2]["plan"]["kept"]) > min(R.LN_EMB[2], ways * R.SETS[2])


def test_grid_stride_large_case(ops):
    """One table of 2 M rows, an empty cache of 20 000 sets x 16 ways and a window of 1 M uniform lookups: about 790 k
    claimants, more than the 2048 x 256 threads of a launch, so every kernel of the policy loops."""
    n_rows, P, ways, n = 2_000_000, 20_000, 16, 1_000_000
    rng = np.random.RandomState(8)
    row = rng.randint(0, n_rows, size=n).astype(np.int64)
    tags = [np.full((P, ways), -1, dtype=np.int64)]
    st = State(ops, [n_rows], tags, 4, host=False)
    uniq = np.unique(row)
    p = R.plan_fill(tags[0], uniq, R.window_counts(uniq, row, n_rows))
    assert len(p["kept"]) > 2048 * 256 + 50_000
    per = [dict(uniq=uniq, plan=p, winners=np.nonzero(p["placed"])[0])]
    plan = ops.WindowPlan(st.ctx, n)
    fill_plan(plan, torch.from_numpy(row).to(DEV).view(1, -1))
    check_lists(st, plan, per)
    check_scratch_clean(plan)
    st.ctx.check()


def test_no_counts_is_index_order(ops):
    """count = NULL (the drop-in entry has unique lists and no window): all priorities equal."""
    ways = 3
    wins, want = restated(ways, use_counts=False)
    st = State(ops, R.LN_EMB, R.initial_tags(ways), 8)
    plan = ops.WindowPlan(st.ctx, R.N_WIN)
    fill_plan(plan, torch.from_numpy(wins[0]).to(DEV), use_counts=False)
    check_lists(st, plan, want[0])
    check_scratch_clean(plan)
    with_counts = restated(ways)[1]
    assert not np.array_equal(want[0][2]["tags"], with_counts[0][2]["tags"])         # (the counts do change this plan)
    # the same through set_unique, as CacheEmbeddings hands the lists over
    plan.set_unique([torch.from_numpy(r["uniq"]) for r in want[0]])
    plan.probe()
    plan.assign_fill(use_counts=False)
    check_lists(st, plan, want[0])
    st.ctx.check()


def test_two_calls_same_bits_and_clean_scratch(ops):
    ways = 16
    wins, want = restated(ways)
    st = State(ops, R.LN_EMB, R.initial_tags(ways), 8)
    plan = ops.WindowPlan(st.ctx, R.N_WIN)
    assert plan.count is None and plan.claim is None           # nothing allocated before the first use
    idx = torch.from_numpy(wins[0]).to(DEV)
    got = []
    for _ in range(2):
        fill_plan(plan, idx)
        check_scratch_clean(plan)
        uo, ko, wo = plan.offsets()
        got.append([t.clone() for t in (plan.way[:ko[-1]], plan.win_claim[:wo[-1]], plan.win_idx[:wo[-1]],
                                        plan.win_row[:wo[-1]], plan.win_tag[:wo[-1]], plan.kept[:ko[-1]])] + [uo, ko, wo])
    for a, b in zip(got[0][:6], got[1][:6]):
        assert torch.equal(a, b)
    assert got[0][6:] == got[1][6:]
    check_lists(st, plan, want[0])
    st.ctx.check()


def test_never_a_lost_insert_and_the_reference_policy_loses_some(ops):
    """600 sets x 16 empty ways, about 9 claimants per set: fill inserts min(claimants, free) in EVERY set; the shipped
    reference policy (device RNG, fixed seed) inserts fewer rows on the same input.  With >= 500 sets of >= 2 claimants the
    reference keeps all of them only if no two claimants of any set draw the same way: at most (15/16)^500 < 1e-14."""
    n_rows, P, ways = 60_000, 600, 16
    rng = np.random.RandomState(4)
    row = rng.randint(0, n_rows, size=6000).astype(np.int64)
    tags = [np.full((P, ways), -1, dtype=np.int64)]
    uniq = np.unique(row)
    p = R.plan_fill(tags[0], uniq, R.window_counts(uniq, row, n_rows))
    per_set = np.bincount(p["sets"], minlength=P)
    assert int(((per_set >= 2) & (p["nfree"] >= 2)).sum()) >= 500
    st = State(ops, [n_rows], tags, 4, host=False)
    plan = ops.WindowPlan(st.ctx, 6000)
    idx = torch.from_numpy(row).to(DEV).view(1, -1)
    plan.unique(idx)
    plan.probe()
    plan.assign(None, seed=5)
    n_ref = plan.offsets()[2][-1]
    fill_plan(plan, idx)
    _, ko, wo = plan.offsets()
    got_sets = plan.win_idx[:wo[-1]].cpu().numpy() % P
    assert np.array_equal(np.bincount(got_sets, minlength=P), np.minimum(per_set, p["nfree"]))
    assert wo[-1] == p["expected_inserts"] and n_ref < wo[-1], (n_ref, wo[-1])
    check_scratch_clean(plan)
    st.ctx.check()


# ---- WindowPipeline ------------------------------------------------------------------------------------------------------

def _pipeline(ln_emb, D, cache, B, ways, max_window, init_seed=3, **kw):
    from cdlrm_amd.engine import WindowPipeline
    from cdlrm_amd.model_no_ddp import Embedding_Table_Cache_Group, Embedding_Table_Group
    np.random.seed(init_seed)
    torch.manual_seed(init_seed)
    host = Embedding_Table_Group(D, np.array(ln_emb)).pin()
    cg = Embedding_Table_Cache_Group(D, np.array(ln_emb), cache, B, ways).to(DEV)
    return WindowPipeline(cg, host, max_window, **kw), cg, host


def _small_windows(ln_emb, n, nwin, seed):
    rng = np.random.RandomState(seed)
    return [np.stack([(rng.zipf(1.2, size=n).astype(np.int64) * 2654435761) % m for m in ln_emb]) for _ in range(nwin)]


def _pipe_lists(pipe):
    p = pipe.plan
    uo, ko, wo = p.offsets()
    return [uo, ko, wo] + [t.cpu().clone() for t in (p.uniq[:uo[-1]], p.kept[:ko[-1]], p.way[:ko[-1]], p.win_claim[:wo[-1]],
                                                     p.win_idx[:wo[-1]], p.win_row[:wo[-1]], p.win_tag[:wo[-1]])]


def _same(a, b):
    return a[:3] == b[:3] and all(torch.equal(x, y) for x, y in zip(a[3:], b[3:]))


@pytest.mark.parametrize("host_gather", [False, True])
def test_streamed_window_equals_one_shot(ops, host_gather):
    """The same windows as one tensor and as 5 uneven chunks from a callable (iterated once for the unique scan and once
    more for the counts): identical lists, tags, cache rows and host tables -- in-line and host-gather plans."""
    ln_emb, D, B, ways, n = [5000, 64, 9, 20000], 16, 64, 4, 4096
    wins = _small_windows(ln_emb, n, 2, 17)
    cuts = [0, 700, 701, 2749, 3082, n]
    out = []
    for streamed in (False, True):
        pipe, cg, host = _pipeline(ln_emb, D, 50, B, ways, n, parity_rng=False, seed=5, insert_policy="fill",
                                   host_gather=host_gather)
        lists = []
        for win in wins:
            idx = torch.from_numpy(win).to(DEV)
            calls = []

            def chunks(idx=idx, calls=calls):
                calls.append(1)
                return iter([idx[:, a:b] for a, b in zip(cuts[:-1], cuts[1:])])

            pipe.plan_window(chunks if streamed else idx)
            pipe.commit()
            pipe.wait_writeback()
            torch.cuda.synchronize()
            assert len(calls) == (2 if streamed else 0)
            lists.append(_pipe_lists(pipe))
        pipe.close()
        cg.ctx.check()
        out.append((lists, cg.tags.cpu().clone(), cg.weight.data.cpu().clone(),
                    [host.emb_l[k].weight.data.clone() for k in range(len(ln_emb))]))
    (la, ta, wa, ha), (lb, tb, wb, hb) = out
    assert all(_same(a, b) for a, b in zip(la, lb))
    assert torch.equal(ta, tb) and torch.equal(wa, wb) and all(torch.equal(a, b) for a, b in zip(ha, hb))
    assert int((ta != -1).sum()) > 0 and la[1][2][-1] > 0


def test_default_policy_unchanged(ops):
    """insert_policy="reference" is the pipeline without the argument: same way choices, same tags, nothing allocated."""
    ln_emb, D, B, ways, n = [5000, 64, 9, 20000], 16, 64, 4, 2048
    wins = _small_windows(ln_emb, n, 2, 23)
    out = []
    for kw in ({}, {"insert_policy": "reference"}):
        pipe, cg, _ = _pipeline(ln_emb, D, 50, B, ways, n, parity_rng=False, seed=5, **kw)
        lists = []
        for win in wins:
            pipe.plan_window(torch.from_numpy(win).to(DEV))
            pipe.commit()
            pipe.wait_writeback()
            torch.cuda.synchronize()
            lists.append(_pipe_lists(pipe))
        assert pipe.plan.count is None and pipe.plan.claim is None
        out.append((lists, cg.tags.cpu().clone()))
    assert all(_same(a, b) for a, b in zip(out[0][0], out[1][0])) and torch.equal(out[0][1], out[1][1])
    # ... and the fill policy is another plan on this input (the comparison above can tell policies apart)
    pipe, cg, _ = _pipeline(ln_emb, D, 50, B, ways, n, parity_rng=False, seed=5, insert_policy="fill")
    for win in wins:
        pipe.plan_window(torch.from_numpy(win).to(DEV))
        pipe.commit()
        pipe.wait_writeback()
    torch.cuda.synchronize()
    assert not torch.equal(cg.tags.cpu(), out[0][1])


def test_parity_plan_draws_nothing_from_the_torch_generator(ops):
    ln_emb, D, B, ways, n = [5000, 64, 9, 20000], 16, 64, 4, 2048
    pipe, cg, _ = _pipeline(ln_emb, D, 50, B, ways, n, parity_rng=True, insert_policy="fill")
    state = torch.get_rng_state()
    for win in _small_windows(ln_emb, n, 2, 29):
        pipe.plan_window(torch.from_numpy(win).to(DEV), q_source=lambda M, w: pytest.fail("a draw was asked for"))
        pipe.commit()
        pipe.wait_writeback()
    torch.cuda.synchronize()
    assert torch.equal(torch.get_rng_state(), state)
    assert int((cg.tags != -1).sum()) > 0
    cg.ctx.check()


# ---- Run / CLI -----------------------------------------------------------------------------------------------------------

RUN_FLAGS = ["--arch-sparse-feature-size=16", "--arch-mlp-bot=13-32-16", "--arch-mlp-top=32-1",
             "--arch-embedding-size=3000-50-40000", "--mini-batch-size=64", "--lookahead=4", "--cache-size=40", "--num-ways=4",
             "--loss-function=bce", "--round-targets=True", "--learning-rate=0.1", "--lr-embeds=0.3", "--print-freq=1",
             "--world-size=1", "--numpy-rand-seed=11", "--table-agg-freq=5", "--data-generation=dataset",
             "--insert-policy=fill"]


def _batches(ln_emb, B, nb, seed):
    rng = np.random.RandomState(seed)
    lS_o = torch.arange(B).repeat(len(ln_emb), 1)
    out = []
    for _ in range(nb):
        X = torch.from_numpy(rng.rand(B, 13).astype(np.float32))
        idx = torch.stack([torch.from_numpy((rng.zipf(1.2, size=B).astype(np.int64) * 2654435761 % n)) for n in ln_emb])
        T = torch.from_numpy(np.round(rng.rand(B, 1)).astype(np.float32))
        out.append((X, lS_o, idx, T))
    return out


def check_invariants(tags, P):
    """Every tag sits in set tag % P and is resident once."""
    s, y = np.nonzero(tags != -1)
    assert np.array_equal(tags[s, y] % P, s)
    assert len(np.unique(tags[s, y])) == len(s)


@pytest.mark.parametrize("device_rng", [False, True])
def test_through_run(monkeypatch, capsys, device_rng):
    """main_no_ddp.Run with --insert-policy=fill, 3 tables, D = 16, B = 64, L = 4, three windows: the tags after every window's
    commit are the restatement's (they depend on the index stream only), the structural invariants hold, the loss is finite
    and a second run prints the same loss bits -- with the parity plan (in-line, torch CPU generator untouched) and with
    --device-rng (look-ahead plan, host-gather)."""
    from cdlrm_amd import engine
    from cdlrm_amd.main_no_ddp import ProcessArgs, Run
    from cdlrm_amd.model_no_ddp import Embedding_Table_Group
    ln_emb = np.array([3000, 50, 40000])
    m_spa, B, L, nb = 16, 64, 4, 12
    ln_bot = np.array([13, 32, 16])
    nf = len(ln_emb) + 1
    ln_top = np.array([m_spa + nf * (nf - 1) // 2, 32, 1])
    batches = _batches(ln_emb, B, nb, 5)
    snaps = []
    real_commit = engine.WindowPipeline.commit

    def commit(self):
        real_commit(self)
        torch.cuda.synchronize()
        snaps.append([o.cpu().numpy().copy() for o in self.cg.occupancy_tables])

    monkeypatch.setattr(engine.WindowPipeline, "commit", commit)
    printed = []
    for rep in range(2):
        args = ProcessArgs(RUN_FLAGS + (["--device-rng"] if device_rng else []))
        np.random.seed(11)
        torch.manual_seed(11)
        eg = Embedding_Table_Group(m_spa, ln_emb).pin()
        capsys.readouterr()
        eng = Run(0, m_spa, ln_emb, ln_bot, ln_top, list(batches), None, None, None, None, eg, args)
        printed.append(capsys.readouterr().out)
        eng.cg.ctx.check()
    assert "Insert policy: fill" in printed[0]
    losses = [re.findall(r"Loss = ([0-9.eE+-]+),", p) for p in printed]
    assert len(losses[0]) == nb - 1 and all(np.isfinite(float(x)) for x in losses[0])
    assert losses[0] == losses[1]
    assert len(snaps) == 6
    sets = [t.shape[0] for t in snaps[0]]
    tags = [np.full((P, 4), -1, dtype=np.int64) for P in sets]
    wins = [torch.cat([b[2] for b in batches[j:j + L]], dim=1).numpy() for j in range(0, nb, L)]
    want = R.run_windows(tags, wins, ln_emb=[int(n) for n in ln_emb])
    for w in range(3):
        for k in range(len(ln_emb)):
            assert np.array_equal(snaps[w][k], want[w][k]["tags"]), (w, k)
            assert np.array_equal(snaps[3 + w][k], want[w][k]["tags"]), (w, k)
            check_invariants(snaps[w][k], sets[k])
    assert sum(int((r["evicted"] != -1).sum()) for per in want for r in per) > 0        # (the windows do evict)


def test_two_emulated_ranks_agree_with_one(tmp_path):
    """Two ranks emulated on the one GPU (CDLRM_BENCH_EMULATE=1, gloo) and a world-1 run of the same command: every rank ends
    every window with the same tags.  tests/insert_fill_cli_dump.py is the CLI with a dump of the tags after each commit."""
    from cdlrm_amd import launch
    flags = [f for f in RUN_FLAGS if not f.startswith(("--world-size", "--data-generation"))]
    flags += ["--data-generation=criteo-synthetic", "--num-batches=12"]
    helper = os.path.join(ROOT, "tests", "insert_fill_cli_dump.py")
    env = dict(os.environ)
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT", "MASTER_ADDR", "GROUP_RANK", "LOCAL_WORLD_SIZE",
              "TORCHELASTIC_RUN_ID"):
        env.pop(k, None)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    env["CDLRM_BENCH_EMULATE"] = "1"
    two, one = str(tmp_path / "w2"), str(tmp_path / "w1")
    cmds = [launch.launcher_command(2, [two] + flags + ["--world-size=2"], script=helper),
            [sys.executable, helper, one] + flags + ["--world-size=1"]]
    for cmd in cmds:
        p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
        assert p.returncode == 0, p.stderr[-3000:]
    d1 = torch.load(one + ".rank0")
    d2 = [torch.load(two + ".rank%d" % r) for r in range(2)]
    assert len(d1) == 3 and len(d2[0]) == 3 and len(d2[1]) == 3
    for w in range(3):
        assert torch.equal(d2[0][w], d2[1][w]) and torch.equal(d2[0][w], d1[w]), w
    assert int((d1[2] != -1).sum()) > 0
