"""Element-wise Adagrad for the MLP parameters on the MI355X:

  1. cdlrm_dense_opt_step / _step2 against float64 (tests/dense_adagrad_restated.py: |S - S64| <= 4 u S64,
     |p - p64| <= 18 u |step| + u |p64|) at the vector / scalar / grid-stride edges, everything outside the ranges bit-unchanged,
     opt = 0 the SGD siblings' bits;
  2. cdlrm_mlp_wgrad_opt_ex on a layer set that reaches the reduction's bias part, 16-byte path and scalar path and the
     element-wise launches, in fp32, bf16 and bf16x3: gradients the bits of cdlrm_mlp_wgrad_ex, parameters and accumulators
     within the bounds of float64 Adagrad on those gradients;
  3. TrainEngine(dense_optimizer="adagrad") per step against float64 on its own grad_flat, against the restated trainer, with
     row-wise Adagrad on the embedding rows against the two restated trainers composed, on two ranks, through Run / --save-model / --load-model, and the default's golden tapes.
"""
import os
import re
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import dense_adagrad_restated as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LR, EPS = 0.05, 1e-10


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


def _np(t):
    return t.detach().cpu().numpy()


def _values(n, seed, zero_state=False):
    """(p, g, S) on the host: gradients over four decades with exact zeros among them, accumulators non-zero unless asked."""
    rng = np.random.RandomState(seed)
    p = rng.randn(n).astype(np.float32)
    g = (rng.randn(n) * 10.0 ** rng.uniform(-3, 0, size=n)).astype(np.float32)
    g[::7] = 0.0
    S = np.zeros(n, np.float32) if zero_state else (rng.rand(n) ** 2).astype(np.float32)
    S[::14] = 0.0           # zero gradient on zero state among them
    return p, g, S


# ---- 1. the element-wise entries ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 3, 4, 255, 1027, 2 * 524288 + 3])
@pytest.mark.parametrize("lead,state_lead", [(0, 0), (1, 1), (3, 2)], ids=["aligned", "odd_start", "state_alignment_differs"])
def test_dense_opt_step_against_float64(ops, n, lead, state_lead):
    """lead: elements in front of the range inside each buffer (the range then starts off a 16-byte boundary: scalar head, 16-byte
    body, scalar tail); a state buffer aligned differently from the parameters leaves the scalar walk only.  The last n is past
    one pass of the capped grid in either walk."""
    p0, g, S0 = _values(n, n + lead)
    pad = 8
    buf = lambda a, ld: torch.from_numpy(np.concatenate([np.full(ld, 7.5, np.float32), a, np.full(pad, 7.5, np.float32)])).to(DEV)
    P, G, S = buf(p0, lead), buf(g, lead), buf(S0, state_lead)
    ops.dense_opt_step(P[lead:lead + n], G[lead:lead + n], S[state_lead:state_lead + n], LR, "adagrad", EPS)
    torch.cuda.synchronize()
    P, S = _np(P), _np(S)
    assert (P[:lead] == 7.5).all() and (P[lead + n:] == 7.5).all() and (S[:state_lead] == 7.5).all() and (S[state_lead + n:] == 7.5).all()
    R.kernel_check(S[state_lead:state_lead + n], P[lead:lead + n], S0, p0, g, LR, EPS, what="n=%d" % n)
    zero = (g == 0) & (S0 == 0)
    assert zero.any() and np.array_equal(P[lead:lead + n][zero], p0[zero]) and (S[state_lead:state_lead + n][zero] == 0).all()


def test_dense_opt_step_from_zero_state(ops):
    n = 1027
    p0, g, S0 = _values(n, 3, zero_state=True)
    P, G, S = (torch.from_numpy(a).to(DEV) for a in (p0, g, S0))
    ops.dense_opt_step(P, G, S, LR, "adagrad", EPS)
    R.kernel_check(_np(S), _np(P), S0, p0, g, LR, EPS)
    assert np.array_equal(_np(P)[g == 0], p0[g == 0]) and np.isfinite(_np(P)).all()


STEP2 = [(1, 1027, 1500, 200), (8, 0, 100, 37), (5, 300, 2000, 0), (0, 256, 256, 513), (2001, 7, 3, 5), (0, 0, 0, 0)]


@pytest.mark.parametrize("off0,n0,off1,n1", STEP2, ids=["odd_off0", "n0_zero", "n1_zero", "adjacent", "second_first", "empty"])
def test_dense_opt_step2_against_float64(ops, off0, n0, off1, n1):
    N = 3000
    p0, g, S0 = _values(N, off0 + n1)
    P, G, S = (torch.from_numpy(a).to(DEV) for a in (p0, g, S0))
    ops.dense_opt_step2(P, G, S, off0, n0, off1, n1, LR, "adagrad", EPS)
    P, S = _np(P), _np(S)
    inside = np.zeros(N, bool)
    inside[off0:off0 + n0] = True
    inside[off1:off1 + n1] = True
    assert np.array_equal(P[~inside], p0[~inside]) and np.array_equal(S[~inside], S0[~inside]), "written outside the ranges"
    if inside.any():
        R.kernel_check(S[inside], P[inside], S0[inside], p0[inside], g[inside], LR, EPS)


def test_opt_zero_is_the_sgd_sibling_and_reads_no_state(ops):
    for n in (1, 255, 1027):
        p0, g, _ = _values(n, n)
        A, B, G = torch.from_numpy(p0).to(DEV), torch.from_numpy(p0).to(DEV), torch.from_numpy(g).to(DEV)
        ops.sgd_step(A, G, LR)
        ops.dense_opt_step(B, G, None, LR, "sgd", 0.0)
        assert torch.equal(A, B)
    p0, g, _ = _values(3000, 1)
    A, B, G = torch.from_numpy(p0).to(DEV), torch.from_numpy(p0).to(DEV), torch.from_numpy(g).to(DEV)
    ops.sgd_step2(A, G, 1, 1027, 1500, 200, LR)
    ops.dense_opt_step2(B, G, None, 1, 1027, 1500, 200, LR, "sgd", 0.0)
    assert torch.equal(A, B) and not torch.equal(A, torch.from_numpy(p0).to(DEV))


def test_entry_refusals(ops):
    from cdlrm_amd import _lib
    L = _lib.raw()
    t = torch.zeros(16, device=DEV)
    for opt, eps, state in ((2, 1e-10, t.data_ptr()), (1, 0.0, t.data_ptr()), (1, float("nan"), t.data_ptr()), (1, 1e-10, None)):
        assert L.cdlrm_dense_opt_step(t.data_ptr(), t.data_ptr(), state, 16, 0.1, opt, eps, None) != 0
        assert L.cdlrm_dense_opt_step2(t.data_ptr(), t.data_ptr(), state, 0, 4, 8, 4, 0.1, opt, eps, None) != 0
    assert L.cdlrm_dense_opt_step2(t.data_ptr(), t.data_ptr(), t.data_ptr(), 0, 8, 4, 8, 0.1, 1, 1e-10, None) != 0      # overlap
    torch.cuda.synchronize()
    assert not bool(t.any())


# ---- 2. the fused entry ------------------------------------------------------------------------------------------------------

# N * K: 832 (x4), 2048 (x4), 512 (x4), 39 (scalar), 2145 (scalar), 32 (x4; the head's 1-wide layer); bias counts 64, 32, 16, 3, 65, 1
LAYERS = [(64, 13), (32, 64), (16, 32), (3, 13), (65, 33), (1, 32)]
# 64: no reduction (element-wise launches); 300: 2 .. 7 slabs (the 8-slab block is skipped, the tail runs); 2048: the last grouped
# M; 2049 / 4133: per-layer splits of 9 / 17 (one 8-slab block and a tail)
MS = (64, 300, 2048, 2049, 4133)
PRECISIONS = ("fp32", "bf16", "bf16x3")


def _fused_case(ops, M, precision, seed=0):
    g = torch.Generator(device="cpu").manual_seed(1000 + M + seed)
    mk = lambda *s: torch.randn(*s, generator=g).to(DEV)
    Xs = [mk(M, K) for _, K in LAYERS]
    dZs = [mk(M, N) * 0.01 for N, _ in LAYERS]
    Ns, Ks = [N for N, _ in LAYERS], [K for _, K in LAYERS]
    new = lambda: ([torch.zeros(N, K, device=DEV) for N, K in LAYERS], [torch.zeros(N, device=DEV) for N, _ in LAYERS])
    plan = lambda dW, db: ops.WgradPlan(Xs, dZs, dW, db, ops.mlp_wgrad_work(M, Ns, Ks, DEV, precision=precision), precision=precision)
    W0 = [mk(N, K) for N, K in LAYERS]
    b0 = [mk(N) for N, _ in LAYERS]
    S0 = [mk(N, K) ** 2 for N, K in LAYERS]
    Sb0 = [mk(N) ** 2 for N, _ in LAYERS]
    return new, plan, W0, b0, S0, Sb0


def test_route_table_reaches_every_reduction_form(ops):
    seen = set()
    for M in MS:
        for precision in PRECISIONS:
            new, plan, *_ = _fused_case(ops, M, precision)
            seen |= {r["splits"] for r in ops.mlp_wgrad_route(plan(*new()))}
    print("slab counts over the table:", sorted(seen))
    assert 1 in seen and any(2 <= s <= 7 for s in seen) and any(s >= 9 for s in seen)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("M", MS)
def test_mlp_wgrad_opt_against_float64(ops, M, precision):
    new, plan, W0, b0, S0, Sb0 = _fused_case(ops, M, precision)
    clone = lambda ts: [t.clone() for t in ts]
    # the gradients alone
    dWr, dbr = new()
    ops.mlp_wgrad(plan(dWr, dbr))

    def run(opt):
        dW, db = new()
        W, b, S, Sb = clone(W0), clone(b0), clone(S0), clone(Sb0)
        pl = plan(dW, db)
        pl.set_params(W, b)
        pl.set_state(S, Sb)
        ops.mlp_wgrad(pl, lr=LR, **({} if opt is None else {"opt": opt}))
        torch.cuda.synchronize()
        return dW, db, W, b, S, Sb

    dW, db, W, b, S, Sb = run(("adagrad", EPS))
    worst = [0.0, 0.0]
    for i, (N, K) in enumerate(LAYERS):
        assert torch.equal(dW[i], dWr[i]) and torch.equal(db[i], dbr[i]), "layer %d: the optimizer changed the gradient" % i
        for got_S, got_p, s0, p0, g in ((S[i], W[i], S0[i], W0[i], dWr[i]), (Sb[i], b[i], Sb0[i], b0[i], dbr[i])):
            e = R.kernel_check(_np(got_S), _np(got_p), _np(s0), _np(p0), _np(g), LR, EPS, what="M=%d %s layer %d" % (M, precision, i))
            worst = [max(a, c) for a, c in zip(worst, e)]
    print("M=%d %s: largest error / bound: accumulators %.3f, parameters %.3f" % (M, precision, worst[0], worst[1]))
    again = run(("adagrad", EPS))
    for a, c in zip((dW, db, W, b, S, Sb), again):
        assert all(torch.equal(x, y) for x, y in zip(a, c)), "two launches on equal inputs differ"
    # opt = 0: the SGD sibling's bits, state untouched
    s_sib, s_opt = run(None), run(("sgd", 0.0))
    for a, c in zip(s_sib, s_opt):
        assert all(torch.equal(x, y) for x, y in zip(a, c))
    assert all(torch.equal(x, y) for x, y in zip(s_opt[4] + s_opt[5], S0 + Sb0))
    assert not torch.equal(s_opt[2][0], W[0])


# ---- 3. the engine -----------------------------------------------------------------------------------------------------------

def _engine(ln_emb, host0, B, *, seed, lr, lr_embeds, cache, ways, mlp=None, **kw):
    from cdlrm_amd.engine import TrainEngine, WindowPipeline
    from cdlrm_amd.model_no_ddp import DLRM_Net, Embedding_Table_Cache_Group, Embedding_Table_Group
    D = R.ENGINE_CASE["m_spa"]
    ln_bot, ln_top = mlp or R.engine_shapes(ln_emb, D)
    host = Embedding_Table_Group(D, np.array(ln_emb))
    for k, E in enumerate(host.emb_l):
        E.weight.data = host0[k].clone()
    host.pin()
    np.random.seed(seed)
    torch.manual_seed(seed)
    cg = Embedding_Table_Cache_Group(D, np.array(ln_emb), cache, B, ways).to(DEV)
    dl = DLRM_Net(ln_bot, ln_top, "dot", False, True, -1, ln_top.size - 2, 0.0).to(DEV)
    eng = TrainEngine(cg, dl, host, lr=lr, lr_embeds=lr_embeds, **kw)
    return eng, cg, dl, host, WindowPipeline


def _drive(eng, cg, host, WindowPipeline, batches, B, L, after_step=None, before_step=None):
    """The window-resident path, as bench.py and Run drive it."""
    from cdlrm_amd.engine import WindowResolver
    pipe = WindowPipeline(cg, host, L * B, parity_rng=True)
    losses = []
    for j, (X, idx, T) in enumerate(batches):
        jl = j % L
        if jl == 0:
            torch.manual_seed(900 + j)
            win = torch.cat([b[1] for b in batches[j:j + L]], dim=1).to(DEV)
            pipe.plan_window(win)
            pipe.commit()
            pipe.wait_writeback()
            rs = WindowResolver(eng, win, B, chunk=2)
        cur = win[:, jl * B:(jl + 1) * B]
        nxt = win[:, (jl + 1) * B:(jl + 2) * B] if (jl + 1 < L and (jl + 1) * B < win.shape[1]) else None
        if before_step:
            before_step(j)
        loss = eng.step(X.to(DEV), cur, T.to(DEV), j=j, next_idx=nxt, res=rs.batch(jl),
                        next_res=rs.batch(jl + 1) if nxt is not None else None)
        rs.ensure(jl + rs.CH + 2)
        losses.append(loss[0:1].clone())
        if after_step:
            after_step(j)
    eng.finish()
    cg.ctx.check()
    return torch.cat(losses).cpu().numpy()


@pytest.mark.parametrize("B,defer,precision", [(64, True, "fp32"), (64, False, "fp32"), (2176, True, "fp32"), (2176, True, "bf16"),
                                               (2176, True, "bf16x3")])
def test_engine_steps_against_float64_on_its_own_gradients(ops, B, defer, precision):
    """Per step, no exclusions: param_flat and dense_state after the step against float64 Adagrad on the step's grad_flat."""
    from oracle import cdlrm_oracle as O
    c = R.ENGINE_CASE
    np.random.seed(c["seed"])
    torch.manual_seed(c["seed"])
    host0 = O.init_host_tables(R.LN_EMB, c["m_spa"])
    batches = R.engine_batches(B=B, nbatch=3, seed=17)
    # 13-64-32-16 and 26-64-32-1: the [32, 64] layer of either sub-network is one the bf16 modes take (K >= 32 and N >= 32)
    nf = len(R.LN_EMB) + 1
    mlp = (np.array([13, 64, 32, c["m_spa"]]), np.array([c["m_spa"] + nf * (nf - 1) // 2, 64, 32, 1]))
    eng, cg, dl, host, WP = _engine(R.LN_EMB, host0, B, seed=c["seed"], lr=LR, lr_embeds=c["lr_embeds"], cache=c["cache_size"],
                                    ways=c["ways"], mlp=mlp, defer_top_update=defer, matmul_precision=precision,
                                    dense_optimizer="adagrad", dense_adagrad_eps=EPS)
    before = {}

    def snap(j):
        eng.finish()
        torch.cuda.synchronize()
        before["p"], before["S"] = eng.param_flat.clone(), eng.dense_state.clone()

    def check(j):
        eng.finish()
        torch.cuda.synchronize()
        e = R.kernel_check(_np(eng.dense_state), _np(eng.param_flat), _np(before["S"]), _np(before["p"]), _np(eng.grad_flat), LR, EPS,
                           what="B=%d step %d" % (B, j))
        print("B=%d defer=%s %s step %d: largest error / bound: accumulators %.3f, parameters %.3f" % (B, defer, precision, j, *e))

    _drive(eng, cg, host, WP, batches, B, c["L"], after_step=check, before_step=snap)
    assert float(eng.dense_state.max()) > 0 and eng.tape_fallbacks == []
    if B > 2048:
        whole, split = eng._wplans(eng._buffers(B))
        routes = [r for p in split for r in ops.mlp_wgrad_route(p)]
        assert max(r["splits"] for r in routes) > 1, "the slabbed reduction is meant to run"
        assert any(r["family"].startswith("bf16") for r in routes) == (precision != "fp32")
        assert {r["family"] for r in routes if r["family"].startswith("bf16")} <= {precision}


_runs = {}


def restated():
    if "tr" not in _runs:
        b = R.engine_batches()
        tr0 = R.run_restated([], dtype=torch.float32)           # (its host tables before any refill)
        _runs["tr"] = (R.run_restated(b), b, [h.clone() for h in tr0.host])
    return _runs["tr"]


def engine_run(*, dense="adagrad", native=True, embed="sgd"):
    key = (dense, native, embed)
    if key in _runs:
        return _runs[key]
    c = R.ENGINE_CASE
    tr, batches, host0 = restated()
    kw = dict(defer_top_update=True)
    if dense != "sgd":
        kw.update(dense_optimizer=dense, dense_adagrad_eps=EPS)
    if embed != "sgd":
        kw.update(embed_optimizer=embed, adagrad_eps=1e-10)
    eng, cg, dl, host, WP = _engine(R.LN_EMB, host0, c["B"], seed=c["seed"], lr=c["lr"], lr_embeds=c["lr_embeds"],
                                    cache=c["cache_size"], ways=c["ways"], **kw)
    eng.native_tape = native
    losses = _drive(eng, cg, host, WP, batches, c["B"], c["L"])
    assert eng.tape_fallbacks == [], eng.tape_fallbacks
    _runs[key] = dict(losses=losses, eng=eng, cg=cg, dl=dl)
    return _runs[key]


def lib_names(eng):
    return {fn.__name__ for t in eng._tapes.values() for fn, _, is_lib in t["prog"] if is_lib}


def _layers(dl):
    from cdlrm_amd.model_no_ddp import _linears
    return _linears(dl.bot_l) + _linears(dl.top_l)


def _within_the_share(what, got, ref):
    """At most 0.5 % of the elements outside rtol 2e-5 / atol 1e-6."""
    assert got.shape == ref.shape, what
    out = np.abs(got - ref) > 1e-6 + 2e-5 * np.abs(ref)
    print("%s outside rtol 2e-5 / atol 1e-6: %d of %d" % (what, int(out.sum()), out.size))
    assert out.mean() <= 0.005, what


def _dense_within_the_share(eng, dl, tr):
    ls = _layers(dl)
    got_p = torch.cat([l.weight.data.reshape(-1) for l in ls] + [l.bias.data.reshape(-1) for l in ls]).cpu().numpy()
    got_S = torch.cat([eng.SW[l][:, :l.in_features].reshape(-1) for l in ls] + [eng.Sb[l].reshape(-1) for l in ls]).cpu().numpy()
    _within_the_share("parameters", got_p, tr.dense_params().numpy())
    _within_the_share("accumulators", got_S, tr.dense_state().numpy())


def test_engine_matches_the_restated_trainer(ops):
    run = engine_run()
    tr, eng, dl = restated()[0], run["eng"], run["dl"]
    want = np.array([l[0] for l in tr.losses])
    print("max relative loss difference %.3g" % float(np.max(np.abs(run["losses"] - want) / np.abs(want))))
    np.testing.assert_allclose(run["losses"], want, rtol=1e-5)
    _dense_within_the_share(eng, dl, tr)
    assert float(eng.dense_state.max()) > 0
    # (the pad column of the first top layer's weight storage: zero gradient, zero state, never moved)
    from cdlrm_amd.model_no_ddp import _linears
    top0 = _linears(dl.top_l)[0]
    assert eng.SW[top0].shape[1] > top0.in_features and not bool(eng.SW[top0][:, top0.in_features:].any())
    names = lib_names(eng)
    assert "cdlrm_mlp_wgrad_opt_ex" in names
    assert not names & {"cdlrm_mlp_wgrad_sgd_ex", "cdlrm_mlp_wgrad_sgd", "cdlrm_sgd_step", "cdlrm_sgd_step2"}
    assert eng._tapes and all(t["native"] is not None for t in eng._tapes.values())
    assert all(k[0].dense_optimizer == "adagrad" and k[0].dense_adagrad_eps == EPS for k in eng._tapes)


def test_tags_equal_an_sgd_run_and_the_tape_is_the_python_issue(ops):
    a, b, s = engine_run(), engine_run(native=False), engine_run(dense="sgd")
    assert torch.equal(a["cg"].tags, s["cg"].tags)
    assert s["eng"].dense_state is None and not any("_opt" in n for n in lib_names(s["eng"]))
    assert "cdlrm_mlp_wgrad_sgd_ex" in lib_names(s["eng"]) or "cdlrm_mlp_wgrad_sgd" in lib_names(s["eng"])
    assert not np.array_equal(a["losses"], s["losses"])
    assert all(t["native"] is None for t in b["eng"]._tapes.values())
    assert np.array_equal(a["losses"], b["losses"])
    assert torch.equal(a["eng"].param_flat, b["eng"].param_flat) and torch.equal(a["eng"].dense_state, b["eng"].dense_state)
    assert torch.equal(a["cg"].weight.data, b["cg"].weight.data)


def test_with_rowwise_adagrad_on_the_embedding_rows(ops):
    both = engine_run(embed="rowwise_adagrad")
    eng = both["eng"]
    names = lib_names(eng)
    assert "cdlrm_mlp_wgrad_opt_ex" in names and "cdlrm_embbag_bwd_apply_sorted_opt" in names
    assert all(t["native"] is not None for t in eng._tapes.values())
    assert np.isfinite(both["losses"]).all() and float(eng.dense_state.max()) > 0 and float(eng.emb_state.max()) > 0
    assert both["losses"][0] == engine_run()["losses"][0] and not np.array_equal(both["losses"], engine_run()["losses"])
    # against the two restated trainers composed (R.BothAdagradTrainer), by the criteria of the single-mode engine tests
    if "both" not in _runs:
        _runs["both"] = R.run_restated(restated()[1], embed="rowwise_adagrad")
    tr, cg = _runs["both"], both["cg"]
    want = np.array([l[0] for l in tr.losses])
    print("max relative loss difference %.3g" % float(np.max(np.abs(both["losses"] - want) / np.abs(want))))
    np.testing.assert_allclose(both["losses"], want, rtol=1e-5)
    _dense_within_the_share(eng, both["dl"], tr)
    state = eng.emb_state_to_host()
    for k in range(len(R.LN_EMB)):
        assert torch.equal(cg.occupancy_tables[k].cpu(), tr.occ[k]), k
        nrow = R.ENGINE_CASE["ways"] * cg.cache_sizes[k]
        _within_the_share("table %d cache-proper rows" % k, cg.emb_l[k].weight[:nrow].detach().cpu().numpy(),
                          tr.weights[0][k][:nrow].numpy())
        _within_the_share("table %d row-wise accumulators" % k, state[k].numpy(), tr.state[k].numpy())


def test_sgd_default_issues_the_golden_tapes(ops):
    """dense_optimizer="sgd" (the default): the recorded steps are, name for name, tests/golden/qr_default_tapes.json's."""
    import json
    import test_qr_cached as Q
    eng = Q.default_run()
    assert eng.dense_optimizer == "sgd" and eng.dense_state is None
    got = Q.tape_names(eng)
    with open(os.path.join(ROOT, "tests", "golden", "qr_default_tapes.json")) as f:
        want = json.load(f)["tapes"]
    assert len(got) == len(want) and all(a == b for a, b in zip(got, want))


# ---- two ranks on one GPU ------------------------------------------------------------------------------------------------------

W2 = dict(table_agg_freq=2, steps=6)


def _w2_worker(rank, world, port, host_shared, ret):
    import faulthandler
    faulthandler.dump_traceback_later(150, exit=True)
    try:
        _w2_body(rank, world, port, host_shared, ret)
    except BaseException:
        import traceback
        ret.put((rank, {"error": traceback.format_exc()}))
        raise


def _w2_body(rank, world, port, host_shared, ret):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import torch.distributed as dist
    import cdlrm_amd.engine as engine
    import cdlrm_amd.model_no_ddp as M
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.cuda.set_device(0)
    c = R.ENGINE_CASE
    ln_emb, D, B, L = np.array(R.LN_EMB), c["m_spa"], c["B"], c["L"]
    ln_bot, ln_top = R.engine_shapes()
    eg = M.Embedding_Table_Group(D, ln_emb, init="empty_meta")
    for k in range(len(ln_emb)):
        eg.emb_l[k].weight.data = host_shared[k]
    eg.register_shared()
    np.random.seed(c["seed"])
    torch.manual_seed(c["seed"])
    cg = M.Embedding_Table_Cache_Group(D, ln_emb, c["cache_size"], B, c["ways"]).to(DEV)
    dl = M.DLRM_Net(ln_bot, ln_top, "dot", False, True, -1, ln_top.size - 2, 0.0).to(DEV)
    eng = engine.TrainEngine(cg, dl, eg, lr=c["lr"], lr_embeds=c["lr_embeds"], world_size=world, rank=rank,
                             table_agg_freq=W2["table_agg_freq"], table_agg_op="mean", defer_top_update=True,
                             dense_optimizer="adagrad", dense_adagrad_eps=EPS)
    # the order of the exchanges and the dense steps, by name
    log = []
    real_step2, real_ar = engine.ops.dense_opt_step2, dist.all_reduce
    engine.ops.dense_opt_step2 = lambda *a, **k: (log.append("cdlrm_dense_opt_step2"), real_step2(*a, **k))[1]
    engine.ops.sgd_step2 = lambda *a, **k: log.append("cdlrm_sgd_step2")
    engine.ops.sgd_step = lambda *a, **k: log.append("cdlrm_sgd_step")
    engine.dist.all_reduce = lambda t, *a, **k: (log.append("all_reduce") if t.numel() > 1 and t.dtype == torch.float32 and
                                                 t.data_ptr() in grad_ptrs else None, real_ar(t, *a, **k))[1]
    grad_ptrs = {v.data_ptr() for v in eng._grad_views}
    pipe = engine.WindowPipeline(cg, eg, L * B, parity_rng=True, rank=rank, world_size=world)
    lbs = -(-B // world)
    sl = slice(rank * lbs, (rank + 1) * lbs)
    batches = R.engine_batches(nbatch=W2["steps"])
    losses, dev_idx, per_step = [], {}, []
    for j, (X, lS_i, Tt) in enumerate(batches):
        if j % L == 0:
            eng.sync_touched_to_rank0()
            torch.manual_seed(900 + j)
            pipe.plan_window(torch.cat([b[1] for b in batches[j:j + L]], dim=1).to(DEV))
            pipe.commit()
            pipe.wait_writeback()
        if j not in dev_idx:
            dev_idx[j] = lS_i[:, sl].contiguous().to(DEV)
        nxt = None
        if j + 1 < len(batches) and (j + 1) % L != 0:
            dev_idx[j + 1] = batches[j + 1][1][:, sl].contiguous().to(DEV)
            nxt = dev_idx[j + 1]
        del log[:]
        loss = eng.step(X[sl].to(DEV), dev_idx[j], Tt[sl].to(DEV), j=j, next_idx=nxt)
        per_step.append(list(log))
        losses.append(float(loss[0]))
    eng.finish()
    cg.ctx.check()
    torch.cuda.synchronize()
    ret.put((rank, dict(losses=np.array(losses), log=per_step, state_w=eng.dense_state[:eng.n_weight].cpu().numpy(),
                        state_b=eng.dense_state[eng.n_weight:].cpu().numpy(), params=eng.param_flat.cpu().numpy())))
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_on_one_gpu(ops):
    from oracle import cdlrm_oracle as O
    c = R.ENGINE_CASE
    batches = R.engine_batches(nbatch=W2["steps"])
    tr = R.run_restated(batches, world_size=2, table_agg_freq=W2["table_agg_freq"])
    np.random.seed(c["seed"])
    torch.manual_seed(c["seed"])
    host = [h.share_memory_() for h in O.init_host_tables(R.LN_EMB, c["m_spa"])]
    ctx = mp.get_context("spawn")
    ret = ctx.Queue()
    procs = [ctx.Process(target=_w2_worker, args=(r, 2, 29891, host, ret)) for r in range(2)]
    for p in procs:
        p.start()
    got = {}
    for _ in range(2):
        r, payload = ret.get(timeout=300)
        assert "error" not in payload, payload["error"]
        got[r] = payload
    for p in procs:
        p.join(timeout=60)
    want = np.array(tr.losses)
    for r in range(2):
        np.testing.assert_allclose(got[r]["losses"], want[:, r], rtol=1e-5)
        for names in got[r]["log"]:
            # the top exchange, the top ranges' step behind it; the bottom exchange, the bottom ranges' step behind it
            assert names == ["all_reduce", "cdlrm_dense_opt_step2", "all_reduce", "cdlrm_dense_opt_step2"], names
    # the averaged weight gradients are the same numbers on both ranks, so are their accumulators; the biases' are each rank's own
    assert np.array_equal(got[0]["state_w"], got[1]["state_w"]) and float(got[0]["state_w"].max()) > 0
    assert not np.array_equal(got[0]["state_b"], got[1]["state_b"])


# ---- Run / main() -----------------------------------------------------------------------------------------------------------------

RUN_EMB = [300, 50, 7, 120]             # every table fits the cache: a run resumed on an empty cache trains the same rows
FLAGS = ["--arch-sparse-feature-size=16", "--arch-mlp-bot=13-32-16", "--arch-mlp-top=32-1",
         "--arch-embedding-size=" + "-".join(map(str, RUN_EMB)), "--mini-batch-size=64", "--lookahead=4", "--cache-size=400",
         "--num-ways=4", "--loss-function=bce", "--round-targets=True", "--learning-rate=0.05", "--lr-embeds=0.01",
         "--print-freq=1", "--world-size=1", "--numpy-rand-seed=11", "--data-generation=criteo-synthetic"]
ADA = ["--dense-optimizer=adagrad"]


class _Loader(list):
    pass


@pytest.fixture
def own_stream():
    """Run trains on a stream of its own and leaves it current: the tests that call it hand the process back with ours."""
    saved = torch.cuda.current_stream()
    try:
        yield
    finally:
        torch.cuda.synchronize()
        torch.cuda.set_stream(saved)


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
    return eng, [float(x) for x in re.findall(r"Loss = ([0-9.eE+-]+),", out)], out


def test_save_then_load_continues_the_uninterrupted_run(ops, own_stream, tmp_path, capsys):
    from rowwise_adagrad_restated import criteo_batches
    lS_o = torch.arange(64).repeat(len(RUN_EMB), 1)
    batches = [(X, lS_o, idx, T) for X, idx, T in criteo_batches(RUN_EMB, 13, 64, 8, 5)]
    whole, path, cont = str(tmp_path / "whole.pt"), str(tmp_path / "half.pt"), str(tmp_path / "cont.pt")
    eng_w, loss_w, _ = _run(batches, ADA + ["--save-model=" + whole], capsys)
    assert eng_w.dense_optimizer == "adagrad" and len(loss_w) == 7
    _run(batches[:4], ADA + ["--save-model=" + path], capsys)
    half = torch.load(path)
    assert half["dense_state"].shape == (eng_w.param_flat.numel(),) and float(half["dense_state"].max()) > 0
    assert half["dense_state"].device.type == "cpu"
    eng_b, loss_b, out_b = _run(batches[4:], ADA + ["--load-model=" + path, "--save-model=" + cont], capsys)
    assert "dense_state" not in out_b
    # printed: the first line of a run averages its steps 0 and 1 (fp64 sums of loss * 64), then one step per line
    assert loss_b == [(loss_w[3] * 64 + loss_w[4] * 64) / 128, loss_w[5], loss_w[6]]
    a, b = torch.load(whole), torch.load(cont)
    assert torch.equal(a["dense_state"], b["dense_state"])
    for name in a["dlrm"]:
        assert torch.equal(a["dlrm"][name], b["dlrm"][name]), name
    # a checkpoint written by an SGD run: no dense_state in it; it loads with zeros and the one line saying so
    sgd = str(tmp_path / "sgd.pt")
    _run(batches[:4], ["--save-model=" + sgd], capsys)
    assert "dense_state" not in torch.load(sgd)
    eng_z, _, out_z = _run([], ADA + ["--load-model=" + sgd], capsys)
    assert eng_z.dense_state is not None and not bool(eng_z.dense_state.any())
    assert len([l for l in out_z.splitlines() if "dense_state" in l]) == 1


def test_main_cli_runs_dense_adagrad_on_criteo_synthetic(ops, own_stream, capsys):
    from cdlrm_amd import main_no_ddp
    losses = {}
    for opt in ("sgd", "adagrad"):
        capsys.readouterr()
        main_no_ddp.main(FLAGS + ["--num-batches=8", "--dense-optimizer=" + opt, "--dense-adagrad-eps=1e-8"])
        losses[opt] = [float(x) for x in re.findall(r"Loss = ([0-9.eE+-]+),", capsys.readouterr().out)]
        assert len(losses[opt]) == 7 and np.isfinite(losses[opt]).all()
    assert losses["sgd"] != losses["adagrad"]


def test_the_cli_tests_leave_the_current_stream_as_they_found_it(ops):
    """(runs behind them: a later test module of the suite records its tapes on whatever stream is current)"""
    assert torch.cuda.current_stream() == torch.cuda.default_stream()
