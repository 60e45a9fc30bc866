"""Row-wise Adagrad for the cached embedding rows on the MI355X:

  1. the kernels behind cdlrm_embbag_bwd_apply_opt / _apply_sorted_opt (k_bwd_chunks, both forms of k_bwd_blocks and k_bwd_long
     with the AdaRow update, one to four column chunks per lane: D = 16 .. 1024) against a float64 reference on the exact fp32
     run sums, which the SGD sibling (k_bwd_chunks with the SgdRow update, k_bwd_blocks_sgd, k_bwd_long_sgd: the same sums in
     the same order) yields on zeroed rows with lr = -1:
         |S - S64| <= (D + 4) u S64,   |W - W64| <= (D/2 + 16) u |lr G / std| + u |W64|        (u = 2^-24)
     aux rows and the accumulators of indices the batch did not look up bit-unchanged, a second launch the same bits, opt = 0
     the sibling's bits;
  2. TrainEngine(embed_optimizer="rowwise_adagrad") against the restated trainer (tests/rowwise_adagrad_restated.py);
  3. Run / main() with --embed-optimizer=rowwise-adagrad, --save-model / --load-model.
"""
import os
import re
import sys

import numpy as np
import pytest
import torch

import rowwise_adagrad_restated as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WAYS = 2
LR, EPS = 0.25, 1e-10
EDGE_RUNS = [1, 2, 31, 32, 33, 64, 65, 1000]        # 1000: 32 chunk partials behind one head (k_bwd_long)


@pytest.fixture(scope="module")
def ops():
    from cdlrm_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        sys.path.insert(0, ROOT)
        import __graft_entry__ as g
        g.build()
    _lib.lib()
    from cdlrm_amd import ops as _ops
    return _ops


class debug6:
    """cdlrm_debug_set(6, bits) for the block (64: the apply on k_bwd_blocks instead of k_bwd_chunks), back to 0 behind it."""

    def __init__(self, bits):
        self.bits = bits

    def __enter__(self):
        from cdlrm_amd import _lib
        assert _lib.raw().cdlrm_debug_set(6, self.bits) == 0

    def __exit__(self, *a):
        from cdlrm_amd import _lib
        _lib.raw().cdlrm_debug_set(6, 0)


# ---- 1. kernels ----------------------------------------------------------------------------------------------------------------

def _runs(n, kind):
    """Run lengths (lookups per distinct slot) that add up to n."""
    if kind == "edges":
        runs, fill, i = list(EDGE_RUNS), (1, 3, 1, 2, 5, 1, 1, 4), 0
        assert n > sum(runs)
        while sum(runs) < n:            # (slots are drawn at random: where a run lies in the sorted order is not its place here)
            runs.append(min(fill[i % len(fill)], n - sum(runs)))
            i += 1
        return runs
    rng = np.random.RandomState(n)
    runs = []
    while sum(runs) < n:
        runs.append(min(int(rng.choice([1, 1, 1, 2, 3, 40])), n - sum(runs)))
    return runs


class Case:
    """Three tables: a run-length script (its last runs on aux slots), every lookup on ONE cache-proper slot, every lookup on ONE
    aux slot.  Tags name a distinct table index per cache-proper slot; every accumulator starts non-zero."""

    def __init__(self, ops, D, n, kind, bags):
        self.D, self.n, self.bags = D, n, bags
        rng = np.random.RandomState(D * 7 + n)
        scripts = [_runs(n, kind), [n], [n]]
        R0 = len(scripts[0])
        self.P = [max(R0, 8) // WAYS + 3, 5, 4]
        self.aux = max(4, R0 // 8 + 2)
        self.n_rows = [3 * p + 2 for p in self.P]
        self.ctx = ops.CacheCtx(self.n_rows, self.P, D, WAYS, self.aux, torch.device(DEV), aux_phases=2)
        tags = []
        for p in self.P:
            t = np.empty((p, WAYS), dtype=np.int64)
            for s in range(p):
                for w in range(WAYS):
                    t[s, w] = s + p * ((w + s) % 3)             # index % P == set, distinct per slot, < 3 P
            tags.append(t.reshape(-1))
        self.tags_np = tags
        self.tags = torch.from_numpy(np.concatenate(tags)).to(DEV)
        self.W0 = rng.randn(self.ctx.total_rows, D).astype(np.float32)
        self.weight = torch.from_numpy(self.W0).to(DEV)
        self.ctx.bind_cache(self.tags, self.weight)
        self.state_off = np.concatenate([[0], np.cumsum(self.n_rows)]).astype(np.int64)
        self.S0 = (0.05 + rng.rand(int(self.state_off[-1]))).astype(np.float32)
        self.state = torch.from_numpy(self.S0).to(DEV)
        self.state_base = torch.from_numpy(self.state_off[:-1].copy()).to(DEV)
        # slots (phase-0 numbering): table 0 scripted, its last n_aux runs on aux slots
        main0 = WAYS * self.P[0]
        n_aux = min(self.aux, max(1, R0 // 8)) if R0 > 1 else 0
        run_slot = np.concatenate([np.sort(rng.choice(main0, R0 - n_aux, replace=False)),
                                   main0 + np.sort(rng.choice(self.aux, n_aux, replace=False))]).astype(np.int64)
        s0 = np.empty(n, dtype=np.int64)
        s0[np.random.RandomState(1000 + n).permutation(n)] = np.repeat(run_slot, scripts[0])
        self.run_slots = [run_slot, np.array([3]), np.array([WAYS * self.P[2] + 1])]
        self.slots = np.stack([s0, np.full(n, 3), np.full(n, WAYS * self.P[2] + 1)]).astype(np.int32)
        self.n_bags = -(-n // 3) if bags else n
        self.offs = torch.arange(0, n, 3, dtype=torch.int64).repeat(3, 1).to(DEV).contiguous() if bags else None
        self.grad = torch.from_numpy(rng.randn(self.n_bags, 3 * D).astype(np.float32)).to(DEV)

    def launch(self, ops, entry, *, opt, lr, aux_phase=0, sgd_sibling=False):
        """One backward on the current weight / state; entry "apply": the batch's own sort; "sorted": a window chunk's lists."""
        n, D = self.n, self.D
        work = ops.embbag_bwd_work(self.ctx, n, DEV)
        kw = dict(opt=opt, eps=EPS, state=self.state, state_base=self.state_base)
        if entry == "apply":
            ops.embbag_bwd_prepare(self.ctx, torch.from_numpy(self.slots).to(DEV), work)
            if sgd_sibling:
                ops.embbag_bwd_apply(self.ctx, n, self.offs, self.grad, 3 * D, D, lr, work)
            else:
                ops.embbag_bwd_apply_opt(self.ctx, n, self.offs, self.grad, 3 * D, D, lr, work, **kw)
        else:
            nb, j = 2, 1
            ws = torch.from_numpy(np.concatenate([self.slots[:, ::-1], self.slots], axis=1).copy()).to(DEV)
            sbuf = ops.embbag_bwd_sorted(self.ctx, nb, n, DEV)
            ops.embbag_bwd_prepare_window(self.ctx, ws, n, nb, n, sbuf)
            k, m, _ = ops.embbag_bwd_sorted_views(self.ctx, sbuf, nb, n, j)
            if sgd_sibling:
                ops.embbag_bwd_apply_sorted(self.ctx, n, self.grad, 3 * D, D, lr, work, k, m, nb * n, aux_phase, False)
            else:
                ops.embbag_bwd_apply_sorted_opt(self.ctx, n, self.grad, 3 * D, D, lr, work, k, m, nb * n, aux_phase, False, **kw)
        torch.cuda.synchronize()
        self.ctx.check()
        return self.weight.cpu().numpy(), self.state.cpu().numpy()

    def reset(self, zero_rows=False):
        self.weight.copy_(torch.zeros_like(self.weight) if zero_rows else torch.from_numpy(self.W0).to(DEV))
        self.state.copy_(torch.from_numpy(self.S0).to(DEV))

    def proper(self):
        """(cache rows, accumulator cells) of every looked-up cache-proper slot, all tables."""
        rows, cells = [], []
        for t in range(3):
            s = self.run_slots[t]
            s = s[s < WAYS * self.P[t]]
            P = self.P[t]
            rows.append(self.ctx.row_base[t] + s)
            cells.append(self.state_off[t] + self.tags_np[t][(s % P) * WAYS + s // P])
        return np.concatenate(rows).astype(np.int64), np.concatenate(cells).astype(np.int64)


KERNEL_CASES = ([(D, 1500, "edges", entry, form, False) for D in (16, 128, 256, 512) for entry in ("apply", "sorted")
                 for form in ("chunks", "blocks")]
                + [(D, 1500, "edges", "apply", form, True) for D in (16, 128, 256, 512) for form in ("chunks", "blocks")]
                + [(128, n, "random", "apply", form, False) for n in (1, 255, 256, 8193) for form in ("chunks", "blocks")]
                + [(512, 8193, "random", "sorted", "chunks", False), (16, 255, "random", "apply", "blocks", True)]
                # D = 1024: four column chunks per lane (NCH = 4 at LPR = 64), the widest row the Adagrad policy takes
                + [(1024, 1500, "edges", entry, form, False) for entry in ("apply", "sorted") for form in ("chunks", "blocks")])
KERNEL_IDS = ["d%d_n%d_%s_%s_%s%s" % (c[0], c[1], c[2], c[3], c[4], "_bags" if c[5] else "") for c in KERNEL_CASES]


@pytest.mark.parametrize("D,n,kind,entry,form,bags", KERNEL_CASES, ids=KERNEL_IDS)
def test_kernels_against_float64(ops, D, n, kind, entry, form, bags):
    c = Case(ops, D, n, kind, bags)
    phase = 1 if entry == "sorted" else 0
    with debug6(64 if form == "blocks" else 0):
        route = ops.embbag_bwd_route(3, D, n, bags, entry, nb=2 if entry == "sorted" else 1)
        assert route["apply"] == form and route["lpr"] == min(64, max(4, 1 << (D // 4 - 1).bit_length()))
        # the exact fp32 run sums: the SGD sibling on zeroed rows, lr = -1 (W = fma(1, G, 0))
        c.reset(zero_rows=True)
        Gall, _ = c.launch(ops, entry, opt="sgd", lr=-1.0, aux_phase=phase, sgd_sibling=True)
        # opt = 0 through the new entry: the sibling's bits
        c.reset()
        w_sib, _ = c.launch(ops, entry, opt="sgd", lr=LR, aux_phase=phase, sgd_sibling=True)
        c.reset()
        w_opt0, s_opt0 = c.launch(ops, entry, opt="sgd", lr=LR, aux_phase=phase)
        assert np.array_equal(w_sib.view(np.int32), w_opt0.view(np.int32)) and np.array_equal(s_opt0, c.S0)
        c.reset()
        W, S = c.launch(ops, entry, opt="rowwise_adagrad", lr=LR, aux_phase=phase)
        c.reset()
        W2, S2 = c.launch(ops, entry, opt="rowwise_adagrad", lr=LR, aux_phase=phase)
    assert np.array_equal(W.view(np.int32), W2.view(np.int32)) and np.array_equal(S.view(np.int32), S2.view(np.int32))
    rows, cells = c.proper()
    assert len(set(cells.tolist())) == len(cells)
    G = Gall[rows]
    assert np.isfinite(G).all() and (np.abs(G).sum(axis=1) > 0).all()
    rs, rw = R.kernel_check(S[cells], W[rows], c.S0[cells], c.W0[rows], G, LR, EPS, what="%s/%s" % (entry, form))
    print("D=%d n=%d %s %s%s: %d rows; max |S err| / bound = %.3g, max |W err| / bound = %.3g"
          % (D, n, entry, form, " bags" if bags else "", len(rows), rs, rw))
    # every other row -- the aux rows of the batch's misses among them -- and every other accumulator: bit-unchanged
    other = np.ones(W.shape[0], dtype=bool)
    other[rows] = False
    assert np.array_equal(W[other].view(np.int32), c.W0[other].view(np.int32)), "a row outside the cache-proper lookups changed"
    aux_rows = c.ctx.row_base[0] + c.run_slots[0][c.run_slots[0] >= WAYS * c.P[0]] + phase * c.aux
    assert len(aux_rows) > 0 or n == 1
    assert (Gall[aux_rows] != 0).any() or n == 1, "the SGD sibling trains the aux rows: the case has misses"
    others = np.ones(S.shape[0], dtype=bool)
    others[cells] = False
    assert np.array_equal(S[others].view(np.int32), c.S0[others].view(np.int32)), "an accumulator outside the lookups changed"


def test_entry_refusals(ops):
    from cdlrm_amd import _lib
    c = Case(ops, 16, 64, "random", False)
    work = ops.embbag_bwd_work(c.ctx, c.n, DEV)
    ops.embbag_bwd_prepare(c.ctx, torch.from_numpy(c.slots).to(DEV), work)
    kw = dict(state=c.state, state_base=c.state_base)
    with pytest.raises(_lib.CdlrmError):
        ops.embbag_bwd_apply_opt(c.ctx, c.n, None, c.grad, 48, 16, LR, work, opt="rowwise_adagrad", eps=0.0, **kw)
    with pytest.raises(_lib.CdlrmError):
        ops.embbag_bwd_apply_opt(c.ctx, c.n, None, c.grad, 48, 16, LR, work, opt="rowwise_adagrad", eps=EPS)
    sbuf = ops.embbag_bwd_sorted(c.ctx, 1, c.n, DEV)
    ops.embbag_bwd_prepare_window(c.ctx, torch.from_numpy(c.slots).to(DEV), c.n, 1, c.n, sbuf)
    k, m, _ = ops.embbag_bwd_sorted_views(c.ctx, sbuf, 1, c.n, 0)
    with pytest.raises(_lib.CdlrmError):        # rest = 1: the once-only slots took an SGD step
        ops.embbag_bwd_apply_sorted_opt(c.ctx, c.n, c.grad, 48, 16, LR, work, k, m, c.n, 0, True, opt="rowwise_adagrad", eps=EPS, **kw)
    torch.cuda.synchronize()
    assert np.array_equal(c.weight.cpu().numpy(), c.W0) and np.array_equal(c.state.cpu().numpy(), c.S0)


# ---- 2. the engine against the restated trainer ------------------------------------------------------------------------------

LN_EMB = [5000, 30, 2000, 900]          # 30 rows: smaller than the cache; table 2 draws from five indices (heavy repeats)
# 17 tables at D = 32: the shape at which an SGD step's gather rides in the interaction kernels and the once-only slots are
# updated by cdlrm_gather_interact_bwd_sgd -- the fold row-wise Adagrad must not take
LN_EMB17 = [3000, 50, 7, 1200, 40000, 90, 2500, 13, 700, 15000, 333, 41, 8000, 5, 1900, 620, 27000]
ECFG = dict(B=64, L=3, ways=4, cache=40, seed=13, nbatch=9, lr=0.1, lr_emb=0.01, eps=1e-10)


def _mlps(D, n_dense, ln_emb=LN_EMB):
    nf = len(ln_emb) + 1
    return np.array([n_dense, 32, D]), np.array([D + nf * (nf - 1) // 2, 32, 1])


def _batches(D, multihot, ln_emb=LN_EMB):
    if not multihot:
        return R.criteo_batches(ln_emb, 13, ECFG["B"], ECFG["nbatch"], 77 + D, heavy=(2,))
    # three lookups per bag, every table
    rng = np.random.RandomState(99 + D)
    out = []
    for _ in range(ECFG["nbatch"]):
        X = torch.from_numpy(rng.rand(ECFG["B"], 13).astype(np.float32))
        idx = torch.stack([torch.from_numpy(((rng.zipf(1.2, size=3 * ECFG["B"]).astype(np.int64) % 5) * 7 % n) if k == 2 else
                                            (rng.zipf(1.2, size=3 * ECFG["B"]).astype(np.int64) * 2654435761 % n))
                           for k, n in enumerate(LN_EMB)])
        out.append((X, idx, torch.from_numpy(np.round(rng.rand(ECFG["B"], 1)).astype(np.float32))))
    return out


_restated = {}


def restated(D, multihot, ln_emb=LN_EMB):
    """The restated trainer's run, computed once per configuration and never changed."""
    key = (D, multihot, len(ln_emb))
    if key not in _restated:
        ln_bot, ln_top = _mlps(D, 13, ln_emb)
        aux = 3 * ECFG["B"] if multihot else ECFG["B"]
        tr = R.RowwiseAdagradTrainer(ln_emb, D, ln_bot, ln_top, cache_size=ECFG["cache"], num_ways=ECFG["ways"],
                                     mini_batch_size=aux, lr=ECFG["lr"], lr_embeds=ECFG["lr_emb"], lookahead=ECFG["L"],
                                     table_agg_freq=10 ** 9, seed=ECFG["seed"], adagrad_eps=ECFG["eps"])
        host0 = [h.clone() for h in tr.host]
        batches = _batches(D, multihot, ln_emb)
        n = batches[0][1].shape[1]
        lS_o = (torch.arange(0, n, 3) if multihot else torch.arange(n)).repeat(len(ln_emb), 1)
        torch.set_num_threads(1)
        for j, (X, idx, T) in enumerate(batches):
            if j % ECFG["L"] == 0:
                torch.manual_seed(900 + j)
                tr.refill(torch.cat([b[1] for b in batches[j:j + ECFG["L"]]], dim=1))
            tr.step(j, X, lS_o, idx, T)
        first_aux = [int(p) * ECFG["ways"] for p in tr.cache_sizes]
        misses = sum(int((t[k].long() >= first_aux[k]).sum()) for t in tr.touched[0] for k in range(len(ln_emb)))
        assert misses > 20 and any(not torch.equal(a, b) for a, b in zip(tr.host, host0)), "misses and evictions are meant to occur"
        _restated[key] = (tr, batches, host0, lS_o)
    return _restated[key]


def engine_run(D, multihot, *, optimizer="rowwise_adagrad", native=True, ln_emb=LN_EMB):
    from cdlrm_amd.engine import TrainEngine, WindowPipeline, WindowResolver
    from cdlrm_amd.model_no_ddp import DLRM_Net, Embedding_Table_Cache_Group, Embedding_Table_Group
    tr, batches, host0, lS_o = restated(D, multihot, ln_emb)
    ln_bot, ln_top = _mlps(D, 13, ln_emb)
    B, L = ECFG["B"], ECFG["L"]
    aux = 3 * B if multihot else B
    host = Embedding_Table_Group(D, np.array(ln_emb))
    for k, E in enumerate(host.emb_l):
        E.weight.data = host0[k].clone()
    host.pin()
    np.random.seed(ECFG["seed"])
    torch.manual_seed(ECFG["seed"])
    cg = Embedding_Table_Cache_Group(D, np.array(ln_emb), ECFG["cache"], aux, ECFG["ways"]).to(DEV)
    dl = DLRM_Net(ln_bot, ln_top, "dot", False, True, -1, ln_top.size - 2, 0.0).to(DEV)
    kw = {} if optimizer == "sgd" else dict(embed_optimizer=optimizer, adagrad_eps=ECFG["eps"])
    eng = TrainEngine(cg, dl, host, lr=ECFG["lr"], lr_embeds=ECFG["lr_emb"], **kw)
    eng.native_tape = native
    pipe = WindowPipeline(cg, host, L * aux, parity_rng=True)
    off = lS_o.to(DEV) if multihot else None
    losses, sorted_steps = [], 0
    for j, (X, idx, T) in enumerate(batches):
        jl = j % L
        if jl == 0:
            torch.manual_seed(900 + j)
            win = torch.cat([b[1] for b in batches[j:j + L]], dim=1).to(DEV)
            pipe.plan_window(win)
            pipe.commit()
            pipe.wait_writeback()
            rs = None if multihot else WindowResolver(eng, win, B, chunk=2)
        n = idx.shape[1]
        cur = win[:, jl * n:(jl + 1) * n]
        if multihot:        # the per-step path: the batch's own probe and sort
            loss = eng.step(X.to(DEV), cur, T.to(DEV), lS_o=off, j=j)
        else:               # the window-resident path, as bench.py and Run drive it
            nxt = win[:, (jl + 1) * n:(jl + 2) * n] if jl + 1 < L else None
            loss = eng.step(X.to(DEV), cur, T.to(DEV), j=j, next_idx=nxt, res=rs.batch(jl),
                            next_res=rs.batch(jl + 1) if nxt is not None else None)
            sorted_steps += eng._cur_sorted is not None
            rs.ensure(jl + rs.CH + 2)
        losses.append(loss[0:1].clone())
    eng.finish()
    cg.ctx.check()
    assert eng.tape_fallbacks == [], eng.tape_fallbacks
    if not multihot:
        assert sorted_steps >= len(batches) - 1, "the steps are meant to run on their look-ahead slices' sorted lists"
    return dict(losses=torch.cat(losses).cpu().numpy(), cg=cg, host=host, eng=eng, tr=tr)


def lib_names(eng):
    return {fn.__name__ for t in eng._tapes.values() for fn, _, is_lib in t["prog"] if is_lib}


@pytest.mark.parametrize("D,multihot,ln_emb", [(16, False, LN_EMB), (128, False, LN_EMB), (16, True, LN_EMB), (128, True, LN_EMB),
                                               (32, False, LN_EMB17)],
                         ids=["d16_criteo_sorted", "d128_criteo_sorted", "d16_multihot_per_step", "d128_multihot_per_step",
                              "d32_t17_fused_gather"])
def test_engine_matches_the_restated_trainer(D, multihot, ln_emb):
    run = engine_run(D, multihot, ln_emb=ln_emb)
    tr, cg, host, eng = run["tr"], run["cg"], run["host"], run["eng"]
    want = np.array([l[0] for l in tr.losses])
    print("D=%d %s: max relative loss difference %.3g" % (D, "multi-hot" if multihot else "criteo",
                                                          float(np.max(np.abs(run["losses"] - want) / np.abs(want)))))
    np.testing.assert_allclose(run["losses"], want, rtol=1e-5)
    state = eng.emb_state_to_host()
    for k in range(len(ln_emb)):
        assert torch.equal(cg.occupancy_tables[k].cpu(), tr.occ[k]), k
        nrow = ECFG["ways"] * cg.cache_sizes[k]
        np.testing.assert_allclose(cg.emb_l[k].weight[:nrow].cpu().numpy(), tr.weights[0][k][:nrow].numpy(), rtol=2e-5, atol=1e-6)
        assert state[k].shape == (ln_emb[k],)
        np.testing.assert_allclose(state[k].numpy(), tr.state[k].numpy(), rtol=2e-5, atol=1e-6)
        assert float(state[k].max()) > 0
    # host rows after a flush: every valid cache row goes back to its host row, on both sides
    cg.flush_to_host(host)
    for k in range(len(ln_emb)):
        P = int(tr.cache_sizes[k])
        want_host = tr.host[k].clone()
        occ = tr.occ[k]
        for s in range(P):
            for w in range(ECFG["ways"]):
                if int(occ[s, w]) >= 0:
                    want_host[int(occ[s, w])] = tr.weights[0][k][P * w + s]
        np.testing.assert_allclose(host.emb_l[k].weight.data.numpy(), want_host.numpy(), rtol=2e-5, atol=1e-6)
    names = lib_names(eng)
    if not multihot:
        assert "cdlrm_embbag_bwd_apply_sorted_opt" in names and "cdlrm_gather_interact_bwd_sgd" not in names
        assert not names & {"cdlrm_embbag_bwd_apply", "cdlrm_embbag_bwd_apply_rest", "cdlrm_embbag_bwd_apply_sorted"}
        assert eng._tapes and all(t["native"] is not None for t in eng._tapes.values())
        assert eng._fused_gather(None) == (ln_emb is LN_EMB17)


def test_tags_equal_an_sgd_run_and_the_tape_is_the_python_issue():
    kw = dict(ln_emb=LN_EMB17)
    a = engine_run(32, False, native=True, **kw)
    b = engine_run(32, False, native=False, **kw)
    s = engine_run(32, False, optimizer="sgd", **kw)
    # (the shape at which the SGD step folds the once-only slots into the interaction backward: Adagrad records no such call)
    assert a["eng"]._fused_gather(None) and "cdlrm_gather_interact_bwd_sgd" not in lib_names(a["eng"])
    assert "cdlrm_gather_interact_bwd" in lib_names(a["eng"])
    assert torch.equal(a["cg"].tags, s["cg"].tags)                      # tags depend on the index stream and the draws only
    assert s["eng"].emb_state is None and s["eng"].state_base is None
    assert not any(n.endswith("_opt") for n in lib_names(s["eng"])) and "cdlrm_gather_interact_bwd_sgd" in lib_names(s["eng"])
    assert not np.array_equal(a["losses"], s["losses"])
    assert all(t["native"] is not None for t in a["eng"]._tapes.values())
    assert all(t["native"] is None for t in b["eng"]._tapes.values())
    assert np.array_equal(a["losses"], b["losses"])
    assert torch.equal(a["cg"].weight.data, b["cg"].weight.data) and torch.equal(a["eng"].emb_state, b["eng"].emb_state)
    # the optimizer keys the tapes
    assert all(k[0].embed_optimizer == "rowwise_adagrad" and not k[0].once for k in a["eng"]._tapes)
    assert all(k[0].embed_optimizer == "sgd" for k in s["eng"]._tapes) and any(k[0].once for k in s["eng"]._tapes)


def test_sgd_default_issues_the_golden_tapes():
    """embed_optimizer="sgd" (the default): the recorded steps are, name for name, tests/golden/qr_default_tapes.json's."""
    import json
    import test_qr_cached as Q
    eng = Q.default_run()
    assert eng.embed_optimizer == "sgd" and eng.emb_state is None
    got = Q.tape_names(eng)
    with open(os.path.join(ROOT, "tests", "golden", "qr_default_tapes.json")) as f:
        want = json.load(f)["tapes"]
    assert len(got) == len(want) and all(a == b for a, b in zip(got, want))


def test_engine_refusals():
    from cdlrm_amd.engine import TrainEngine
    from cdlrm_amd.model_no_ddp import DLRM_Net, Embedding_Table_Cache_Group, Embedding_Table_Group
    host = Embedding_Table_Group(16, np.array([1000])).pin()
    cg = Embedding_Table_Cache_Group(16, np.array([1000]), 50, 8, 2, cache_init="zeros").to(DEV)
    dl = DLRM_Net(np.array([13, 16]), np.array([17, 1]), "dot", False, True, -1, 0, 0.0).to(DEV)
    for kw, word in ((dict(adagrad_eps=0.0), "eps"), (dict(adagrad_eps=-1e-3), "eps"), (dict(world_size=2), "one rank")):
        with pytest.raises(ValueError, match=word):
            TrainEngine(cg, dl, host, lr=0.1, lr_embeds=0.1, embed_optimizer="rowwise_adagrad", **kw)
    with pytest.raises(ValueError, match="embed_optimizer"):
        TrainEngine(cg, dl, host, lr=0.1, lr_embeds=0.1, embed_optimizer="adam")
    qh = Embedding_Table_Group(16, np.array([1000]), qr_flag=True, qr_operation="mult", qr_collisions=4, qr_threshold=200).pin()
    qcg = Embedding_Table_Cache_Group(16, np.array([1000]), 50, 8, 2, cache_init="zeros", qr_layout=qh.qr_layout()).to(DEV)
    with pytest.raises(ValueError, match="quotient-remainder"):
        TrainEngine(qcg, dl, qh, lr=0.1, lr_embeds=0.1, embed_optimizer="rowwise_adagrad")
    eng = TrainEngine(cg, dl, host, lr=0.1, lr_embeds=0.1, embed_optimizer="rowwise_adagrad")
    eng.evict_victim = True
    with pytest.raises(ValueError, match="evict-victim-cache"):
        eng.step(torch.zeros(8, 13, device=DEV), torch.zeros(1, 8, dtype=torch.int64, device=DEV), torch.zeros(8, 1, device=DEV))


# ---- 3. Run / main() ---------------------------------------------------------------------------------------------------------

RUN_EMB = [300, 50, 7, 120]             # every table fits the cache: a run resumed on an empty cache trains the same rows
FLAGS = ["--arch-sparse-feature-size=16", "--arch-mlp-bot=13-32-16", "--arch-mlp-top=32-1",
         "--arch-embedding-size=" + "-".join(map(str, RUN_EMB)), "--mini-batch-size=64", "--lookahead=4", "--cache-size=400",
         "--num-ways=4", "--loss-function=bce", "--round-targets=True", "--learning-rate=0.1", "--lr-embeds=0.01",
         "--print-freq=1", "--world-size=1", "--numpy-rand-seed=11", "--data-generation=criteo-synthetic",
         "--embed-optimizer=rowwise-adagrad"]


class _Loader(list):
    pass


def _run(loader, extra, capsys):
    from cdlrm_amd.main_no_ddp import ProcessArgs, Run
    from cdlrm_amd.model_no_ddp import Embedding_Table_Group
    np.random.seed(11)
    torch.manual_seed(11)
    eg = Embedding_Table_Group(16, np.array(RUN_EMB)).pin()
    capsys.readouterr()
    eng = Run(0, 16, np.array(RUN_EMB), np.array([13, 32, 16]), np.array([16 + 5 * 4 // 2, 32, 1]), _Loader(loader), None, None,
              None, None, eg, ProcessArgs(FLAGS + extra))
    out = capsys.readouterr().out
    return eng, eg, [float(x) for x in re.findall(r"Loss = ([0-9.eE+-]+),", out)], out


def test_save_then_load_continues_the_uninterrupted_run(tmp_path, capsys):
    lS_o = torch.arange(64).repeat(len(RUN_EMB), 1)
    batches = [(X, lS_o, idx, T) for X, idx, T in R.criteo_batches(RUN_EMB, 13, 64, 8, 5)]
    whole, wpath, path = str(tmp_path / "whole.pt"), None, str(tmp_path / "half.pt")
    eng_w, _, loss_w, _ = _run(batches, ["--save-model=" + whole], capsys)
    assert eng_w.embed_optimizer == "rowwise_adagrad" and len(loss_w) == 7
    _run(batches[:4], ["--save-model=" + path], capsys)
    half = torch.load(path)
    assert [tuple(s.shape) for s in half["emb_state"]] == [(n,) for n in RUN_EMB] and all(float(s.max()) > 0 for s in half["emb_state"])
    eng_b, _, loss_b, out_b = _run(batches[4:], ["--load-model=" + path, "--save-model=" + str(tmp_path / "cont.pt")], capsys)
    assert "emb_state" not in out_b
    # printed: the first line of a run averages its steps 0 and 1 (fp64 sums of loss * 64), then one step per line
    assert loss_b == [(loss_w[3] * 64 + loss_w[4] * 64) / 128, loss_w[5], loss_w[6]]
    a, b = torch.load(whole), torch.load(str(tmp_path / "cont.pt"))
    for k in range(len(RUN_EMB)):
        assert torch.equal(a["emb"][k], b["emb"][k]) and torch.equal(a["emb_state"][k], b["emb_state"][k]), k
    for name in a["dlrm"]:
        assert torch.equal(a["dlrm"][name], b["dlrm"][name]), name
    # a checkpoint without emb_state (an SGD run's): the accumulators start at zero, and one line says so
    del half["emb_state"]
    torch.save(half, path)
    eng_z, _, _, out_z = _run([], ["--load-model=" + path], capsys)
    assert not bool(eng_z.emb_state.any())
    assert len([l for l in out_z.splitlines() if "emb_state" in l]) == 1


def test_main_cli_runs_rowwise_adagrad_on_criteo_synthetic(capsys):
    from cdlrm_amd import main_no_ddp
    flags = [f for f in FLAGS if not f.startswith("--embed-optimizer")] + ["--num-batches=8"]
    losses = {}
    for opt in ("sgd", "rowwise-adagrad"):
        capsys.readouterr()
        main_no_ddp.main(flags + ["--embed-optimizer=" + opt, "--adagrad-eps=1e-8"])
        losses[opt] = [float(x) for x in re.findall(r"Loss = ([0-9.eE+-]+),", capsys.readouterr().out)]
        assert len(losses[opt]) == 7 and np.isfinite(losses[opt]).all()
    assert losses["sgd"][1:] != losses["rowwise-adagrad"][1:]
