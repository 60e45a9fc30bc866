"""Quotient-remainder tables trained through the embedding cache on the MI355X: the three kernels of
csrc/qr_cached.hip against numpy, the engine against the restated trainer (tests/qr_cached_restated.py)."""
import os
import sys

import numpy as np
import pytest
import torch

import qr_cached_restated as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -24


def gamma(m):
    """gamma_m = m u / (1 - m u): the bound of a sum of m terms in any order (Higham, Accuracy and Stability, 4.2)."""
    m = np.asarray(m, dtype=np.float64)
    return m * U / (1.0 - m * U)


def dev_i32(a):
    return torch.tensor(list(a), dtype=torch.int32, device=DEV)


def dev_i64(a):
    return torch.tensor(list(a), dtype=torch.int64, device=DEV)


def scan_ctx(rows):
    """A context that only lends its table count and error word (no cache is bound)."""
    from cdlrm_amd import ops
    return ops.CacheCtx(list(rows), [1] * len(rows), 4, 1, 0, torch.device(DEV))


# ---- split -------------------------------------------------------------------------------------------------------------

BIG = [40_000_000, 39_884_406]


def _split_case(n, kinds, rows, seed):
    rng = np.random.RandomState(seed)
    idx = np.stack([rng.randint(0, rows[k], size=n).astype(np.int64) for k in range(len(kinds))])
    edge = [0, 1, (1 << 24) - 3, (1 << 24) - 1, 1 << 24, (1 << 24) + 1, (1 << 24) + 5]
    for k in range(len(kinds)):
        special = [v for v in edge if v < rows[k]] + [rows[k] - 1, rows[k] - 2]
        for i, v in enumerate(special[:n]):
            idx[k, (i * 7) % n if n > len(special) else i] = v
    idx[:, -1] = [r - 1 for r in rows]
    return idx


@pytest.mark.parametrize("n", [1, 63, 64, 65, 1000])
@pytest.mark.parametrize("in_place", [False, True])
def test_split_mixed_tables_pitch_and_offset(n, in_place):
    """T = 3 (plain, c = 4, c = 3) over a rectangle with pitch > n whose first column sits at an odd element offset; ids just
    below and above 2^24 and the last id of a 40 M-row table.  Bit for bit against the numpy split."""
    from cdlrm_amd import ops
    kinds, rows = [0, 4, 3], [1000] + BIG
    ctx = scan_ctx(R.rows_q_of(rows, kinds))
    idx = _split_case(n, kinds, rows, n)
    pitch = n + 7
    buf = torch.full((3, pitch), -7, dtype=torch.int64, device=DEV)
    view = buf[:, 3:3 + n]
    view.copy_(torch.from_numpy(idx))
    rbuf = torch.full((3, pitch + 2), 99, dtype=torch.uint8, device=DEV)
    rview = rbuf[:, 5:5 + n]
    q, r = ops.qr_split(ctx, view, dev_i32(kinds), dev_i64(rows), q=view if in_place else None, r=rview)
    ctx.check()
    for k in range(3):
        wq, wr = R.split(idx[k], rows[k], kinds[k])
        assert np.array_equal(q[k].cpu().numpy(), wq), k
        assert np.array_equal(r[k].cpu().numpy(), wr), k
    if not in_place:
        assert np.array_equal(view.cpu().numpy(), idx)
    # nothing outside the rectangles was written
    assert bool((buf[:, :3] == -7).all()) and bool((buf[:, 3 + n:] == -7).all())
    assert bool((rbuf[:, :5] == 99).all()) and bool((rbuf[:, 5 + n:] == 99).all())


@pytest.mark.parametrize("c", [2, 3, 4, 16])
def test_split_every_collision_count(c):
    from cdlrm_amd import ops
    rows = [BIG[0]]
    ctx = scan_ctx(R.rows_q_of(rows, [c]))
    idx = _split_case(777, [c], rows, c)
    q, r = ops.qr_split(ctx, torch.from_numpy(idx).to(DEV), dev_i32([c]), dev_i64(rows))
    ctx.check()
    wq, wr = R.split(idx[0], rows[0], c)
    assert np.array_equal(q[0].cpu().numpy(), wq) and np.array_equal(r[0].cpu().numpy(), wr)
    assert int(q.max()) <= -(-rows[0] // c) - 1


@pytest.mark.parametrize("bad", [-1, 1000])
def test_split_out_of_range_sets_the_error_word(bad):
    from cdlrm_amd import _lib, ops
    ctx = scan_ctx([250])
    idx = torch.tensor([[5, bad, 7]], dtype=torch.int64, device=DEV)
    ops.qr_split(ctx, idx, dev_i32([4]), dev_i64([1000]))
    with pytest.raises(_lib.CdlrmError) as e:
        ctx.check()
    assert e.value.rc == -34
    ctx.check()     # read and cleared


# ---- forward / backward kernels -----------------------------------------------------------------------------------------

def _cache(D, seed, c, n):
    """Three tables (plain, QR, QR) with a bound cache of random rows; slots with repeats and aux slots; r over [0, c)."""
    from cdlrm_amd import ops
    rng = np.random.RandomState(seed)
    sets, ways, aux = [5, 7, 3], 2, 8
    ctx = ops.CacheCtx([40, 100, 60], sets, D, ways, aux, torch.device(DEV), aux_phases=2)
    tags = torch.full((ctx.total_tags,), -1, dtype=torch.int64, device=DEV)
    W = torch.from_numpy(rng.standard_normal((ctx.total_rows, D)).astype(np.float32)).to(DEV)
    ctx.bind_cache(tags, W)
    slots = np.stack([rng.randint(0, ways * sets[k] + 2 * aux, size=n) for k in range(3)]).astype(np.int32)
    slots[:, : n // 4] = slots[:, n // 4: 2 * (n // 4)]          # repeated slots
    slots[:, -3:] = np.array([[ways * s, ways * s + aux, ways * s + 2 * aux - 1] for s in sets])      # aux slots of both regions
    r = rng.randint(0, c, size=(3, n)).astype(np.uint8)
    Wr = rng.uniform(0.1, 1.0, size=(3, c, D)).astype(np.float32)
    return ctx, W, slots, r, Wr


def _rows(ctx, W, slots):
    Wn = W.cpu().numpy()
    return np.stack([Wn[ctx.row_base[k] + slots[k].astype(np.int64)] for k in range(slots.shape[0])])        # [T, n, D]


@pytest.mark.parametrize("D", [4, 16, 128, 256])
@pytest.mark.parametrize("op", ["mult", "add"])
def test_forward_composes_into_the_feature_rows(D, op):
    """One rounding per element: bit for bit against numpy's fp32 multiply / add of the same rows; written straight into
    feat[:, 1:, :] of a [B, 1 + T, D] block, the dense feature's row left alone; r columns of a wider rectangle."""
    from cdlrm_amd import ops
    n, c = 1000, 4
    ctx, W, slots, r, Wr = _cache(D, D + len(op), c, n)
    coll = [0, c, c]
    feat = torch.full((n + 1, 4, D), 7.0, dtype=torch.float32, device=DEV)[:n]
    rbuf = torch.zeros((3, n + 9), dtype=torch.uint8, device=DEV)
    rv = rbuf[:, 4:4 + n]
    rv.copy_(torch.from_numpy(r))
    ops.qr_cached_fwd(ctx, torch.from_numpy(slots).to(DEV), rv, torch.from_numpy(Wr).to(DEV), dev_i32(coll), ops.QR_OPS[op],
                      feat[:, 1:, :], feat.stride(0), D)
    got = feat.cpu().numpy()
    rows = _rows(ctx, W, slots)
    for k in range(3):
        y = Wr[k][r[k]]
        want = rows[k] if coll[k] == 0 else (rows[k] * y if op == "mult" else rows[k] + y)
        assert np.array_equal(got[:, 1 + k, :], want.astype(np.float32)), k
    assert bool((feat[:, 0, :] == 7.0).all())


def _bwd_case(D, op, n, c, r, seed):
    from cdlrm_amd import ops
    ctx, W, slots, _, Wr = _cache(D, seed, c, n)
    coll = [0, c, c]
    rng = np.random.RandomState(seed + 1)
    g = rng.standard_normal((n, 4, D)).astype(np.float32)
    lr = 0.25           # (exact in fp32: the bound below has no term for its conversion)
    d_slots, d_r, d_coll = torch.from_numpy(slots).to(DEV), torch.from_numpy(r).to(DEV), dev_i32(coll)
    work = ops.qr_cached_bwd_work(ctx, n, c)
    outs = []
    for _ in range(2):
        dfeat = torch.from_numpy(g).to(DEV)
        d_Wr = torch.from_numpy(Wr).to(DEV)
        gWr = torch.full_like(d_Wr, 5.0)
        work.fill_(float("nan"))
        ops.qr_cached_bwd(ctx, d_slots, d_r, d_Wr, d_coll, ops.QR_OPS[op], dfeat[:, 1:, :], dfeat.stride(0), D, work)
        ops.qr_cached_bwd_finish(ctx, d_coll, n, work, lr, d_Wr, gWr)
        outs.append((dfeat.cpu().numpy(), gWr.cpu().numpy(), d_Wr.cpu().numpy()))
    return ctx, W, slots, Wr, coll, g, lr, outs


def _check_bwd(D, op, n, c, r, seed):
    ctx, W, slots, Wr, coll, g, lr, outs = _bwd_case(D, op, n, c, r, seed)
    (df, gWr, Wr_new), second = outs
    for a, b in zip(outs[0], second):           # two calls: the same bits
        assert np.array_equal(a, b)
    rows = _rows(ctx, W, slots)
    assert np.array_equal(df[:, 0, :], g[:, 0, :])
    for k in range(3):
        gk = g[:, 1 + k, :]
        if coll[k] == 0:
            assert np.array_equal(df[:, 1 + k, :], gk)
            assert np.array_equal(Wr_new[k], Wr[k])
            continue
        want = gk * Wr[k][r[k]] if op == "mult" else gk
        assert np.array_equal(df[:, 1 + k, :], want.astype(np.float32)), k        # the cache rows' gradient, in place
        terms = gk.astype(np.float64) * rows[k].astype(np.float64) if op == "mult" else gk.astype(np.float64)
        for rr in range(c):
            sel = r[k] == rr
            m = int(sel.sum())
            if m == 0:
                assert np.array_equal(gWr[k, rr], np.zeros(D, np.float32))
                assert np.array_equal(Wr_new[k, rr], Wr[k, rr]), "an absent remainder's row changed"
                continue
            S, A = terms[sel].sum(axis=0), np.abs(terms[sel]).sum(axis=0)
            err = np.abs(gWr[k, rr].astype(np.float64) - S)
            print("D=%d %s n=%d table %d r=%d m=%d: max |err| / (gamma_m * sum|terms|) = %.3g"
                  % (D, op, n, k, rr, m, float((err / (gamma(m) * A)).max())))
            assert (err <= gamma(m) * A).all(), (k, rr)
            # Wr' = fl(Wr - fl(lr * s)), |s - S| <= gamma_m A:  |Wr' - (Wr - lr S)| <= lr gamma_{m+1} A (1 + u) + u |Wr - lr S|
            exact = Wr[k, rr].astype(np.float64) - lr * S
            errw = np.abs(Wr_new[k, rr].astype(np.float64) - exact)
            assert (errw <= lr * gamma(m + 1) * A * (1 + U) + U * np.abs(exact)).all(), (k, rr)


@pytest.mark.parametrize("D", [4, 16, 128, 256])
@pytest.mark.parametrize("op", ["mult", "add"])
def test_backward_rows_in_place_and_remainder_sums(D, op):
    n, c = 1000, 4
    r = np.random.RandomState(D).randint(0, c, size=(3, n)).astype(np.uint8)
    _check_bwd(D, op, n, c, r, 100 + D)


@pytest.mark.parametrize("n", [1000, 8192])
@pytest.mark.parametrize("c", [4, 16])
def test_backward_every_lookup_on_one_remainder(n, c):
    """m = n terms in one sum (the longest chain the partition can produce); every other remainder is absent and its Wr row
    stays bit-identical."""
    r = np.full((3, n), c - 2, dtype=np.uint8)
    _check_bwd(16, "mult", n, c, r, n + c)


def test_backward_one_remainder_absent():
    n, c = 1000, 3
    r = (np.random.RandomState(3).randint(0, 2, size=(3, n)) * 2).astype(np.uint8)      # 0 and 2 only
    _check_bwd(128, "mult", n, c, r, 77)
    _check_bwd(128, "add", n, c, r, 78)


# ---- the engine against the restated trainer ----------------------------------------------------------------------------

CFG = dict(ln_emb=[10_000] * 6 + [150] * 2, m_spa=16, B=128, L=32, ways=4, cache=2000, c=4, thr=200, seed=31, nbatch=96,
           ln_bot=[13, 32, 16], top=[32, 1], lr=0.1, lr_emb=0.3)
CFG_D256 = dict(CFG, ln_emb=[10_000, 150], m_spa=256, ln_bot=[13, 32, 256], nbatch=40, L=20)


def _ln_top(cfg):
    nf = len(cfg["ln_emb"]) + 1
    return np.array([cfg["m_spa"] + nf * (nf - 1) // 2] + cfg["top"])


def restated_run(cfg, op, world=1, agg_freq=10 ** 9, agg_op="mean", eval_at=None):
    host, wr = R.init_tables(cfg["ln_emb"], cfg["m_spa"], cfg["c"], cfg["thr"], cfg["seed"])
    host0, wr0 = [h.clone() for h in host], [None if w is None else w.clone() for w in wr]
    tr = R.QRCachedTrainer(cfg["ln_emb"], cfg["m_spa"], cfg["ln_bot"], _ln_top(cfg), qr_collisions=cfg["c"],
                           qr_threshold=cfg["thr"], qr_operation=op, host_tables=host, weight_r=wr, cache_size=cfg["cache"],
                           num_ways=cfg["ways"], mini_batch_size=cfg["B"], world_size=world, lr=cfg["lr"],
                           lr_embeds=cfg["lr_emb"], lookahead=cfg["L"], table_agg_freq=agg_freq, table_agg_op=agg_op,
                           seed=cfg["seed"])
    batches = R.criteo_batches(cfg["ln_emb"], cfg["ln_bot"][0], cfg["B"], cfg["nbatch"], cfg["seed"] + 1)
    lS_o = torch.arange(cfg["B"]).repeat(len(cfg["ln_emb"]), 1)
    L, scores = cfg["L"], None
    torch.set_num_threads(1)
    for j, (X, idx, T) in enumerate(batches):
        if j % L == 0:
            torch.manual_seed(5000 + j)
            tr.refill(torch.cat([b[1] for b in batches[j:j + L]], dim=1))
        tr.step(j, X, lS_o, idx, T)
        if eval_at is not None and j == eval_at:
            Xe, ie, _ = batches[(j + 7) % len(batches)]
            scores = tr.evaluate(Xe, lS_o, ie).numpy().copy()
    return tr, batches, host0, wr0, scores


_restated = {}


def restated(cfg_name, op):
    """Computed once per (configuration, operation), shared by the tests that need it, never changed."""
    key = (cfg_name, op)
    if key not in _restated:
        cfg = CFG if cfg_name == "mixed" else CFG_D256
        _restated[key] = restated_run(cfg, op, eval_at=cfg["nbatch"] // 2)
    return _restated[key]


def build_engine(cfg, op, host0, wr0, world=1, rank=0, agg_freq=10 ** 9, agg_op="mean", qr=True, insert_policy=None,
                 replicated=False):
    from cdlrm_amd.engine import TrainEngine, WindowPipeline
    from cdlrm_amd.model_no_ddp import DLRM_Net, Embedding_Table_Cache_Group, Embedding_Table_Group
    ln_emb, m = np.array(cfg["ln_emb"]), cfg["m_spa"]
    if qr:
        host = Embedding_Table_Group(m, ln_emb, qr_flag=True, qr_operation=op, qr_collisions=cfg["c"], qr_threshold=cfg["thr"])
        for k, E in enumerate(host.emb_l):
            if wr0[k] is None:
                E.weight.data = host0[k].clone()
            else:
                E.weight_q.data, E.weight_r.data = host0[k].clone(), wr0[k].clone()
        layout = host.qr_layout()
    else:       # a plain-mode engine over tables of rows_q rows, fed the q stream
        ln_emb = np.array(R.rows_q_of(cfg["ln_emb"], R.collisions_of(cfg["ln_emb"], cfg["c"], cfg["thr"])))
        host = Embedding_Table_Group(m, ln_emb)
        for k, E in enumerate(host.emb_l):
            E.weight.data = host0[k].clone()
        layout = None
    host.pin()
    host._replicated = bool(replicated)     # (world > 1: every rank holds and writes back to a private copy, as hostmem.py's "replicas")
    np.random.seed(cfg["seed"])
    torch.manual_seed(cfg["seed"])
    cg = Embedding_Table_Cache_Group(m, ln_emb, cfg["cache"], cfg["B"], cfg["ways"], **({"qr_layout": layout} if qr else {})).to(DEV)
    dl = DLRM_Net(np.array(cfg["ln_bot"]), _ln_top(cfg), "dot", False, True, -1, 1, 0.0).to(DEV)
    eng = TrainEngine(cg, dl, host, lr=cfg["lr"], lr_embeds=cfg["lr_emb"], world_size=world, rank=rank,
                      table_agg_freq=agg_freq, table_agg_op=agg_op)
    kw = {} if insert_policy is None else dict(insert_policy=insert_policy)
    pipe = WindowPipeline(cg, host, cfg["L"] * cfg["B"], parity_rng=True, rank=rank, world_size=world, **kw)
    return host, cg, dl, eng, pipe


def engine_run(cfg, op, batches, host0, wr0, *, resolved=True, native=True, eval_at=None, qr=True, tags_per_window=None):
    from cdlrm_amd.engine import WindowResolver
    host, cg, dl, eng, pipe = build_engine(cfg, op, host0, wr0, qr=qr)
    eng.native_tape = native
    L, B = cfg["L"], cfg["B"]
    coll = R.collisions_of(cfg["ln_emb"], cfg["c"], cfg["thr"])
    losses, scores = [], None
    for j, (X, idx, T) in enumerate(batches):
        if j % L == 0:
            raw = torch.cat([b[1] for b in batches[j:j + L]], dim=1)
            if qr:      # the window rectangle, split once where it is built: q in place, r in a parallel uint8 rectangle
                win = raw.to(DEV)
                _, rwin = eng.qr_split(win, q=win)
            else:
                win, rwin = R.split_tables(raw, cfg["ln_emb"], coll)[0].to(DEV), None
            torch.manual_seed(5000 + j)
            pipe.plan_window(win)
            pipe.commit()
            pipe.wait_writeback()
            if tags_per_window is not None:
                tags_per_window.append(cg.tags.cpu().clone())
            rs = WindowResolver(eng, win, B, chunk=3) if resolved else None
        jl = j % L
        cols = slice(jl * B, (jl + 1) * B)
        nxt = win[:, (jl + 1) * B:(jl + 2) * B] if (resolved and jl + 1 < L and j + 1 < len(batches)) else None
        loss = eng.step(X.to(DEV), win[:, cols], T.to(DEV), j=j, next_idx=nxt, res=rs.batch(jl) if rs is not None else None,
                        next_res=rs.batch(jl + 1) if (rs is not None and nxt is not None) else None,
                        **({"r": rwin[:, cols]} if qr else {}))
        if rs is not None:
            rs.ensure(jl + rs.CH + 2)
        losses.append(loss[0:1].clone())
        if eval_at is not None and j == eval_at:
            Xe, ie, _ = batches[(j + 7) % len(batches)]
            qe, re_ = eng.qr_split(ie.to(DEV))
            scores = eng.evaluate(Xe.to(DEV), qe, r=re_).cpu().numpy().copy()
    eng.finish()
    cg.ctx.check()
    assert eng.tape_fallbacks == [], eng.tape_fallbacks
    return dict(losses=torch.cat(losses).cpu().numpy(), cg=cg, host=host, eng=eng, scores=scores, pipe=pipe)


def _compare_state(run, tr, cfg):
    cg, host, eng = run["cg"], run["host"], run["eng"]
    coll = R.collisions_of(cfg["ln_emb"], cfg["c"], cfg["thr"])
    for k in range(len(cfg["ln_emb"])):
        assert torch.equal(cg.occupancy_tables[k].cpu(), tr.occ[k]), k                      # tags bit-exact
        nrow = cfg["ways"] * cg.cache_sizes[k]
        np.testing.assert_allclose(cg.emb_l[k].weight[:nrow].cpu().numpy(), tr.weights[0][k][:nrow].numpy(), rtol=2e-5, atol=1e-6)
        hw = host.emb_l[k].weight_q if coll[k] else host.emb_l[k].weight
        np.testing.assert_allclose(hw.data.numpy(), tr.host[k].numpy(), rtol=2e-5, atol=1e-6)
        if coll[k]:
            np.testing.assert_allclose(eng.Wr[k].cpu().numpy(), tr.Wr[0][k].numpy(), rtol=2e-5, atol=1e-6)


@pytest.mark.parametrize("op", ["mult", "add"])
def test_engine_matches_the_restated_trainer(op):
    """8 tables, 6 x 10 000 rows (QR: rows_q = 2500 > P = 2003, so misses and evictions occur) and 2 x 150 rows (plain), c = 4,
    D = 16, B = 128, L = 32, 96 steps; the window-resident path with the native tape, as bench.py and Run drive a step."""
    tr, batches, host0, wr0, scores = restated("mixed", op)
    assert max(tr.cache_sizes) == 2003
    first_aux = [p * CFG["ways"] for p in tr.cache_sizes]
    assert sum(int((t[k].long() >= first_aux[k]).sum()) for t in tr.touched[0] for k in range(8)) > 100      # lookups miss
    assert any(not torch.equal(tr.host[k], host0[k]) for k in range(6))                                     # rows are evicted
    run = engine_run(CFG, op, batches, host0, wr0, eval_at=CFG["nbatch"] // 2)
    np.testing.assert_allclose(run["losses"], np.array([l[0] for l in tr.losses]), rtol=1e-5)
    _compare_state(run, tr, CFG)
    np.testing.assert_allclose(run["scores"], scores, rtol=1e-5, atol=1e-6)
    assert run["eng"]._tapes and all(t["native"] is not None for t in run["eng"]._tapes.values())


def test_engine_matches_the_restated_trainer_at_d256():
    tr, batches, host0, wr0, scores = restated("d256", "mult")
    run = engine_run(CFG_D256, "mult", batches, host0, wr0, eval_at=CFG_D256["nbatch"] // 2)
    np.testing.assert_allclose(run["losses"], np.array([l[0] for l in tr.losses]), rtol=1e-5)
    _compare_state(run, tr, CFG_D256)
    np.testing.assert_allclose(run["scores"], scores, rtol=1e-5, atol=1e-6)


def test_engine_per_step_probe_matches_too():
    """No resolver, no next batch handed over: the in-line probe path."""
    tr, batches, host0, wr0, _ = restated("mixed", "mult")
    run = engine_run(CFG, "mult", batches, host0, wr0, resolved=False)
    np.testing.assert_allclose(run["losses"], np.array([l[0] for l in tr.losses]), rtol=1e-5)
    _compare_state(run, tr, CFG)


def test_tag_state_equals_a_plain_run_on_the_q_stream():
    """Tags depend only on the index stream and the draws: after every refill the QR run's tags equal, bit for bit, those of a
    plain-mode engine fed q over tables of rows_q rows."""
    _, batches, host0, wr0, _ = restated("mixed", "mult")
    a, b = [], []
    engine_run(CFG, "mult", batches, host0, wr0, tags_per_window=a)
    engine_run(CFG, "mult", batches, host0, wr0, qr=False, tags_per_window=b)
    assert len(a) == len(b) == 3
    for x, y in zip(a, b):
        assert torch.equal(x, y)


def test_native_tape_and_python_issue_the_same_bits():
    _, batches, host0, wr0, _ = restated("mixed", "mult")
    a = engine_run(CFG, "mult", batches, host0, wr0, native=True)
    b = engine_run(CFG, "mult", batches, host0, wr0, native=False)
    assert all(t["native"] is not None for t in a["eng"]._tapes.values())
    assert all(t["native"] is None for t in b["eng"]._tapes.values())
    names = set()
    for t in a["eng"]._tapes.values():
        names |= {fn.__name__ for fn, _, is_lib in t["prog"] if is_lib}
    assert {"cdlrm_qr_cached_fwd", "cdlrm_qr_cached_bwd", "cdlrm_qr_cached_bwd_finish"} <= names
    assert np.array_equal(a["losses"], b["losses"])
    assert torch.equal(a["cg"].weight.data, b["cg"].weight.data) and torch.equal(a["cg"].tags, b["cg"].tags)
    assert torch.equal(a["eng"].Wr, b["eng"].Wr)


def test_flush_writes_wr_back_and_load_restores_it():
    """flush_to_host copies the cache rows to weight_q, flush_wr copies Wr to the host group's weight_r; load_wr brings it back."""
    _, batches, host0, wr0, _ = restated("mixed", "mult")
    run = engine_run(CFG, "mult", batches[:8], host0, wr0)
    eng, cg, host = run["eng"], run["cg"], run["host"]
    assert not torch.equal(host.emb_l[0].weight_r.data, eng.Wr[0].cpu())
    cg.flush_to_host(host)
    eng.flush_wr(host)
    for k in range(6):
        assert torch.equal(host.emb_l[k].weight_r.data, eng.Wr[k].cpu())
    saved = eng.Wr.clone()
    eng.Wr.zero_()
    eng.load_wr(host)
    assert torch.equal(eng.Wr, saved)


def test_refusals_of_the_engine():
    from cdlrm_amd.model_no_ddp import Embedding_Table_Group
    _, batches, host0, wr0, _ = restated("mixed", "mult")
    host, cg, dl, eng, pipe = build_engine(CFG, "mult", host0, wr0)
    X, idx, T = batches[0]
    q, r = eng.qr_split(idx.to(DEV))
    with pytest.raises(ValueError, match="one lookup per bag"):
        eng.step(X.to(DEV), q, T.to(DEV), lS_o=torch.arange(CFG["B"], device=DEV).repeat(8, 1), r=r)
    with pytest.raises(NotImplementedError):
        cg(None, q, host, 0)
    from cdlrm_amd.engine import TrainEngine
    from cdlrm_amd.model_no_ddp import DLRM_Net, Embedding_Table_Cache_Group
    for kw, word in ((dict(qr_operation="concat", qr_collisions=4), "concat"), (dict(qr_operation="mult", qr_collisions=17), "2 .. 16"),
                     (dict(qr_operation="mult", qr_collisions=1), "2 .. 16")):
        bad = Embedding_Table_Group(16, np.array([1000]), qr_flag=True, qr_threshold=200, **kw).pin()
        bcg = Embedding_Table_Cache_Group(16, np.array([1000]), 50, 8, 2, cache_init="zeros", qr_layout=bad.qr_layout()).to(DEV)
        bdl = DLRM_Net(np.array([13, 16]), np.array([17, 1]), "dot", False, True, -1, 0, 0.0).to(DEV)
        with pytest.raises(ValueError, match=word):
            TrainEngine(bcg, bdl, bad, lr=0.1, lr_embeds=0.1)
    from cdlrm_amd import ops
    assert ops.qr_cached_shape_ok(256, 16) and ops.qr_cached_shape_ok(256, 4) and not ops.qr_cached_shape_ok(512, 16)


def tape_names(eng):
    """The recorded steps of an engine in the order they were recorded: per tape, the entry names in issue order (library
    entry points by symbol, stream / event calls by method name)."""
    return [[getattr(fn, "__name__", type(fn).__name__) for fn, _, _ in t["prog"]] for t in eng._tapes.values()]


def default_run():
    """A plain-mode engine (no QR layout) over 40 batches of the mixed configuration's q stream: the run whose recorded launch
    sequences tests/golden/qr_default_tapes.json pins, taken from the commit before quotient-remainder mode existed."""
    _, batches, host0, wr0, _ = restated("mixed", "mult")
    return engine_run(CFG, "mult", batches[:40], host0, wr0, qr=False)["eng"]


def test_default_run_allocates_nothing_and_issues_the_parents_sequence():
    """Without a QR layout: no Wr, no r window, no scratch -- and every recorded step is, call for call, the one the parent
    commit recorded for the same run: the same number of tapes, the same length, the same entry names in the same order."""
    import json
    eng = default_run()
    assert eng.qr is None and eng.Wr is None and eng._r is None and not any(k[0] == "qr" for k in eng._bufs if isinstance(k, tuple))
    got = tape_names(eng)
    with open(os.path.join(ROOT, "tests", "golden", "qr_default_tapes.json")) as f:
        want = json.load(f)["tapes"]
    assert len(got) == len(want) and len(want) >= 2
    for a, b in zip(got, want):
        assert len(a) == len(b) and a == b
    assert not any(n.startswith("cdlrm_qr_") for t in got for n in t)
