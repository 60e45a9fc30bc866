"""Warm-up / polynomial-decay learning-rate schedules on the MI355X.

The rates of a scheduled run are two float cells of the launch tapes (TrainEngine.set_lr_factor): a step replayed from a native
tape under the schedule W = 4, S0 = 6, N = 5 has to leave the bits of the untaped step whose base rates were ASSIGNED the same
float32 effective rates -- the mechanism the engine had before, a path and a recording per rate -- on the three run descriptions
of tests/step_trace.py, in two lanes, with both Adagrad optimizers and through quotient-remainder tables, without one tape more
than a constant factor needs; the scheduled engine follows the oracle's trainer with per-step rates on one rank and on two;
and the command line's step counter travels with --save-model / --load-model."""
import functools
import os
import re
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from cdlrm_amd.lr_schedule import LRSchedule, effective_rate      # noqa: E402

W_, S0_, N_ = 4, 6, 5
SCHED = LRSchedule(W_, S0_, N_)
SCHED_FLAGS = ["--lr-num-warmup-steps=%d" % W_, "--lr-decay-start-step=%d" % S0_, "--lr-num-decay-steps=%d" % N_]
SHAPES = ("train_small", "train_c1", "fused_shape")


_AT_START = {}


@pytest.fixture(scope="module", autouse=True)
def _the_stream_this_module_found():
    """(whatever an earlier module of the suite left current: the tests below hand back THAT stream)"""
    _AT_START["stream"] = torch.cuda.current_stream()
    yield


def _rates(base, base_emb, j):
    """The float32 effective rates of step j (0-based: optimizer step s = j + 1), as Python floats."""
    f = SCHED.factor(j + 1)
    return float(effective_rate(base, f)), float(effective_rate(base_emb, f))


def _shape(name):
    import step_trace as ST
    return ST.gpu_shapes(lambda n: np.load(os.path.join(ROOT, "tests", "golden", n + ".npz")))[name]


def _drive(name, mode, *, adagrad=False, lanes=None):
    """One run description of step_trace.gpu_shapes, driven as step_trace.gpu_run drives it (windows of L batches, a
    WindowResolver with chunks of 3, the next batch handed over inside a window).
    mode "cells": native tapes, set_lr_factor(factor of the step) in front of every step; "const": the same with the factor held
    at 1.0; "assigned": untaped, eng.lr / eng.lr_embeds assigned the step's effective rates.
    adagrad: both Adagrad optimizers.  lanes: tape_lanes, with tape_lanes_below above the batch (call it on a stream of the
    caller's own: the null stream has one lane)."""
    import test_engine_parity as P
    import cdlrm_amd.engine as E
    g = _shape(name)
    host, cg, dl, eng, pipe = P.build(g, aux_phases=2)
    if adagrad:
        eng.dense_optimizer, eng.dense_adagrad_eps = "adagrad", 1e-8
        eng.embed_optimizer, eng.adagrad_eps = "rowwise_adagrad", 1e-8
    base = (eng.lr, eng.lr_embeds)
    eng.use_tape = mode != "assigned"
    eng.native_tape = True
    if lanes is not None:
        eng.tape_lanes, eng.tape_lanes_below = lanes, int(g["B"]) + 1
    L = int(g["L"])
    batches = P.make_batches(g)
    dev = [(X.to(DEV), idx.to(DEV), Tt.to(DEV)) for X, idx, Tt in batches]
    losses = []
    for j, (X, idx, Tt) in enumerate(dev):
        if j % L == 0:
            win = torch.cat([b[1] for b in batches[j:j + L]], dim=1).to(DEV)
            torch.manual_seed(5000 + j)
            pipe.plan_window(win)
            pipe.commit()
            pipe.wait_writeback()
            rs = E.WindowResolver(eng, win, int(g["B"]), chunk=3)
        jl = j % L
        nxt = dev[j + 1][1] if j + 1 < len(dev) and jl + 1 < L else None
        if mode == "cells":
            eng.set_lr_factor(SCHED.factor(j + 1))
        elif mode == "const":
            eng.set_lr_factor(1.0)
        else:
            eng.lr, eng.lr_embeds = _rates(*base, j)
        loss = eng.step(X, idx, Tt, j=j, next_idx=nxt, res=rs.batch(jl), next_res=rs.batch(jl + 1) if nxt is not None else None)
        rs.ensure(jl + rs.CH + 2)
        losses.append(loss[0:3].clone())
        if mode == "cells":
            assert tuple(float(x) for x in eng.effective_rates()) == _rates(*base, j)
    eng.finish()
    torch.cuda.synchronize()
    cg.ctx.check()
    return dict(eng=eng, losses=torch.stack(losses).cpu(), params=eng.param_flat.detach().cpu().clone(),
                rows=cg.weight.data.detach().cpu().clone(), tags=cg.tags.cpu().clone(),
                dense_state=None if eng.dense_state is None else eng.dense_state.cpu().clone(),
                emb_state=None if eng.emb_state is None else eng.emb_state.cpu().clone())


@functools.lru_cache(maxsize=None)
def _run(name, mode, adagrad=False):
    return _drive(name, mode, adagrad=adagrad)


def _same_bits(a, b, what):
    assert torch.equal(a["losses"], b["losses"]), "%s: losses" % what
    assert torch.equal(a["params"], b["params"]), "%s: MLP parameters" % what
    assert torch.equal(a["rows"], b["rows"]), "%s: cache rows" % what
    assert torch.equal(a["tags"], b["tags"]), what
    for k in ("dense_state", "emb_state"):
        assert (a[k] is None) == (b[k] is None) and (a[k] is None or torch.equal(a[k], b[k])), "%s: %s" % (what, k)


def _rate_args_are_cells(eng):
    """Every float argument of a recorded library call that takes a rate IS one of the engine's two cells."""
    import ctypes as C
    cells = {id(eng._lr_cell): "lr", id(eng._lr_embeds_cell): "lr_embeds"}
    rated = ("cdlrm_sgd_step", "cdlrm_sgd_step2", "cdlrm_dense_opt_step", "cdlrm_dense_opt_step2", "cdlrm_mlp_wgrad_sgd_ex",
             "cdlrm_mlp_wgrad_opt_ex", "cdlrm_embbag_bwd_sgd", "cdlrm_embbag_bwd_apply", "cdlrm_embbag_bwd_apply_rest",
             "cdlrm_embbag_bwd_apply_sorted", "cdlrm_embbag_bwd_apply_opt", "cdlrm_embbag_bwd_apply_sorted_opt",
             "cdlrm_gather_interact_bwd_sgd", "cdlrm_qr_cached_bwd_finish")
    seen = set()
    for t in eng._tapes.values():
        for fn, args, is_lib in t["prog"]:
            if not is_lib:
                continue
            fl = [a for a, ty in zip(args, fn.argtypes) if ty is C.c_float]
            if fn.__name__ in rated:
                assert id(fl[0]) in cells, "%s: its rate is recorded by value" % fn.__name__     # (the rate is its first float)
                seen.add((fn.__name__, cells[id(fl[0])]))
                assert all(id(a) not in cells for a in fl[1:]), fn.__name__
            else:
                assert all(id(a) not in cells for a in fl), fn.__name__
    return seen


# ---- 1. taped equals assigned ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SHAPES)
def test_taped_with_a_factor_equals_untaped_with_assigned_rates(name):
    a, c, u = _run(name, "cells"), _run(name, "const"), _run(name, "assigned")
    _same_bits(a, u, name)
    eng = a["eng"]
    assert eng.tape_fallbacks == [] and c["eng"].tape_fallbacks == []
    assert eng._tapes and all(t["native"] is not None and t["native"]._fcells is not None for t in eng._tapes.values())
    assert len(eng._tapes) == len(c["eng"]._tapes), "distinct factors add no tape"
    assert len(eng._tapes) < len(a["losses"]), "steps are replayed"
    assert all(k[0].lr_cells and (k[0].lr, k[0].lr_embeds) == (eng.lr, eng.lr_embeds) for k in eng._tapes)
    assert not u["eng"]._tapes and not u["eng"].lr_cells and not u["eng"]._step_key[0].lr_cells
    assert not torch.equal(a["losses"], c["losses"]), "the schedule moves the run"
    seen = _rate_args_are_cells(eng)
    assert {w for _, w in seen} == {"lr", "lr_embeds"}
    if name == "fused_shape":       # the once-only fold of the fused interaction backward reads the embedding rate's cell
        assert ("cdlrm_gather_interact_bwd_sgd", "lr_embeds") in seen


# ---- 2. lanes ---------------------------------------------------------------------------------------------------------------------
def test_the_helper_lanes_read_the_float_cells():
    torch.cuda.synchronize()
    own = torch.cuda.Stream(priority=-1)
    own.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(own):
        a = _drive("train_small", "cells", lanes=2)
    torch.cuda.current_stream().wait_stream(own)
    torch.cuda.synchronize()
    eng = a["eng"]
    assert eng.tape_fallbacks == []
    assert eng._tapes and all(t["native"] is not None and t["native"].lanes == 2 for t in eng._tapes.values())
    assert all(k[0].lanes == 2 for k in eng._tapes)
    # the embedding update is the side queue's: its rate is read by the helper thread
    _same_bits(a, _run("train_small", "assigned"), "two lanes")


# ---- 3. optimizers -------------------------------------------------------------------------------------------------------------
def test_both_adagrad_optimizers_take_the_factor():
    a, u = _run("fused_shape", "cells", True), _run("fused_shape", "assigned", True)
    _same_bits(a, u, "adagrad")
    eng = a["eng"]
    assert eng.tape_fallbacks == [] and float(a["dense_state"].max()) > 0 and float(a["emb_state"].max()) > 0
    seen = _rate_args_are_cells(eng)
    assert {n for n, _ in seen} & {"cdlrm_mlp_wgrad_opt_ex", "cdlrm_dense_opt_step", "cdlrm_dense_opt_step2"}
    assert {n for n, _ in seen} & {"cdlrm_embbag_bwd_apply_sorted_opt", "cdlrm_embbag_bwd_apply_opt"}
    assert not torch.equal(a["losses"], _run("fused_shape", "cells")["losses"])


@pytest.fixture
def own_stream():
    """Run trains on a stream of its own and leaves it current: the tests that call it hand the process back with ours."""
    saved = torch.cuda.current_stream()
    try:
        yield
    finally:
        torch.cuda.synchronize()
        torch.cuda.set_stream(saved)


def test_quotient_remainder_tables_take_the_factor(own_stream, monkeypatch, capsys):
    """Run with --qr-flag, set up as tests/test_qr_cached_run.py does: the scheduled run (its steps replayed from tapes) against
    the same run without the flags whose every step is untaped with the effective rates assigned."""
    import test_qr_cached_run as Q
    import cdlrm_amd.engine as E
    from cdlrm_amd.main_no_ddp import ProcessArgs, Run
    host, wr = Q.R.init_tables(Q.LN_EMB, 16, 4, 200, 11)
    ln_top = np.array([16 + 6 * 5 // 2, 32, 1])
    nb = 14

    def run(extra):
        eg = Q._host_group("mult", host, wr)
        capsys.readouterr()
        eng = Run(0, 16, np.array(Q.LN_EMB), np.array([13, 32, 16]), ln_top, Q._Loader(Q._loader(nb, 5)), None, None, None, None,
                  eg, ProcessArgs(Q.FLAGS + extra))
        out = capsys.readouterr().out
        return eng, re.findall(r"Loss = ([0-9.eE+-]+),", out), out

    eng_a, loss_a, out_a = run(SCHED_FLAGS)
    assert eng_a.qr is not None and eng_a.lr_cells and eng_a.tape_fallbacks == []
    assert eng_a._tapes and len(eng_a._tapes) < nb and all(t["native"] is not None for t in eng_a._tapes.values())
    assert ("cdlrm_qr_cached_bwd_finish", "lr_embeds") in _rate_args_are_cells(eng_a)
    step0, count = E.TrainEngine.step, [0]

    def assigned_step(self, *a, **k):
        self.use_tape = False
        self.lr, self.lr_embeds = _rates(0.1, 0.3, count[0])
        count[0] += 1
        return step0(self, *a, **k)

    monkeypatch.setattr(E.TrainEngine, "step", assigned_step)
    eng_u, loss_u, out_u = run([])
    monkeypatch.undo()
    assert count[0] == nb and not eng_u.lr_cells and not eng_u._tapes
    assert loss_a == loss_u and len(loss_a) == nb - 1
    assert torch.equal(eng_a.param_flat, eng_u.param_flat) and torch.equal(eng_a.Wr, eng_u.Wr)
    assert torch.equal(eng_a.cg.weight.data, eng_u.cg.weight.data) and torch.equal(eng_a.cg.tags, eng_u.cg.tags)
    assert "Learning rates at step" in out_a and "Learning rate" not in out_u


def test_the_qr_test_leaves_the_current_stream_as_it_found_it():
    assert torch.cuda.current_stream() == _AT_START["stream"]


# ---- 4. against the oracle -------------------------------------------------------------------------------------------------------
def test_the_scheduled_engine_follows_the_oracle_with_per_step_rates():
    from oracle import cdlrm_oracle as O
    from test_oracle_golden import make_batches as oracle_batches
    g = _shape("train_small")
    ln_emb = [int(x) for x in g["ln_emb"]]
    L, m_spa = int(g["L"]), int(g["m_spa"])
    ln_top = np.array([m_spa + (len(ln_emb) + 1) * len(ln_emb) // 2] + list(g["top"]))
    torch.set_num_threads(1)
    tr = O.OracleTrainer(ln_emb, m_spa, g["ln_bot"], ln_top, cache_size=int(g["cache_size"]), num_ways=int(g["ways"]),
                         mini_batch_size=int(g["B"]), lr=float(g["lr"]), lr_embeds=float(g["lr_emb"]), lookahead=L,
                         table_agg_freq=10 ** 9, seed=int(g["seed"]))
    ob = oracle_batches(g)
    for j, (X, lS_o, lS_i, Tt) in enumerate(ob):
        if j % L == 0:
            torch.manual_seed(5000 + j)
            tr.refill(torch.cat([b[2] for b in ob[j:j + L]], dim=1))
        tr.lr, tr.lr_embeds = _rates(float(g["lr"]), float(g["lr_emb"]), j)
        tr.step(j, X, lS_o, lS_i, Tt)
    a = _run("train_small", "cells")
    got, want = a["losses"][:, 0].double().numpy(), np.array([l[0] for l in tr.losses])
    print("max relative loss difference under the schedule: %.3g" % float(np.max(np.abs(got - want) / np.abs(want))))
    np.testing.assert_allclose(got, want, rtol=1e-5)
    for k in range(len(ln_emb)):
        assert torch.equal(a["eng"].cg.occupancy_tables[k].cpu(), tr.occ[k]), k
    # the schedule is what the oracle followed: its unscheduled trajectory (the golden file's) is another one
    assert float(np.max(np.abs(want - g["losses"]) / np.abs(want))) > 1e-4


# ---- 5. two ranks on one GPU -----------------------------------------------------------------------------------------------------
W2 = dict(table_agg_freq=2, steps=12)


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
    import dense_adagrad_restated as R
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
                             table_agg_freq=W2["table_agg_freq"], table_agg_op="mean", defer_top_update=True)
    pipe = engine.WindowPipeline(cg, eg, L * B, parity_rng=True, rank=rank, world_size=world)
    lbs = -(-B // world)
    sl = slice(rank * lbs, (rank + 1) * lbs)
    batches = R.engine_batches(nbatch=W2["steps"])
    losses, dev_idx = [], {}
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
        eng.set_lr_factor(SCHED.factor(j + 1))          # every rank from its own counter: nothing is communicated
        loss = eng.step(X[sl].to(DEV), dev_idx[j], Tt[sl].to(DEV), j=j, next_idx=nxt)
        losses.append(float(loss[0]))
    eng.finish()
    cg.ctx.check()
    torch.cuda.synchronize()
    ret.put((rank, dict(losses=np.array(losses), weights=eng.param_flat[:eng.n_weight].cpu().numpy(),
                        biases=eng.param_flat[eng.n_weight:].cpu().numpy(), tapes=len(eng._tapes),
                        fallbacks=list(eng.tape_fallbacks), cells=all(k[0].lr_cells for k in eng._tapes))))
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_on_one_gpu():
    """Set up as tests/test_dense_adagrad.py::test_two_ranks_on_one_gpu (spawned children, gloo), twelve steps so that the
    warm-up, the whole decay and the floor behind it are run: each rank's losses against OracleTrainer(world_size=2) with the
    per-step rates.  The dense parameters the ranks exchange gradients for -- all weights -- end up equal on both; the bias
    gradients are not reduced (main_no_ddp.py:234-247, as the oracle restates), so the biases are each rank's own with or
    without a schedule."""
    from oracle import cdlrm_oracle as O
    import dense_adagrad_restated as R
    c = R.ENGINE_CASE
    batches = R.engine_batches(nbatch=W2["steps"])
    ln_bot, ln_top = R.engine_shapes()
    torch.set_num_threads(1)
    tr = O.OracleTrainer(R.LN_EMB, c["m_spa"], ln_bot, ln_top, cache_size=c["cache_size"], num_ways=c["ways"],
                         mini_batch_size=c["B"], world_size=2, lr=c["lr"], lr_embeds=c["lr_embeds"], lookahead=c["L"],
                         table_agg_freq=W2["table_agg_freq"], seed=c["seed"])
    lS_o = torch.arange(c["B"]).repeat(len(R.LN_EMB), 1)
    for j, (X, idx, T) in enumerate(batches):
        if j % c["L"] == 0:
            torch.manual_seed(900 + j)
            tr.refill(torch.cat([b[1] for b in batches[j:j + c["L"]]], dim=1))
        tr.lr, tr.lr_embeds = _rates(c["lr"], c["lr_embeds"], j)
        tr.step(j, X, lS_o, idx, T)
    np.random.seed(c["seed"])
    torch.manual_seed(c["seed"])
    host = [h.share_memory_() for h in O.init_host_tables(R.LN_EMB, c["m_spa"])]
    ctx = mp.get_context("spawn")
    ret = ctx.Queue()
    procs = [ctx.Process(target=_w2_worker, args=(r, 2, 29893, host, ret)) for r in range(2)]
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
        print("rank %d: max relative loss difference %.3g" % (r, float(np.max(np.abs(got[r]["losses"] - want[:, r]) / want[:, r]))))
        np.testing.assert_allclose(got[r]["losses"], want[:, r], rtol=1e-5)
        assert got[r]["fallbacks"] == [] and got[r]["cells"]
    assert np.array_equal(got[0]["weights"], got[1]["weights"]), "the exchanged dense parameters are one set of numbers"
    assert not np.array_equal(got[0]["biases"], got[1]["biases"])
    assert got[0]["tapes"] == got[1]["tapes"]


# ---- 6. the command line ----------------------------------------------------------------------------------------------------------
def _cli(loader, extra, capsys):
    import test_dense_adagrad as DA
    from cdlrm_amd.main_no_ddp import ProcessArgs, Run
    from cdlrm_amd.model_no_ddp import Embedding_Table_Group
    np.random.seed(11)
    torch.manual_seed(11)
    eg = Embedding_Table_Group(16, np.array(DA.RUN_EMB)).pin()
    capsys.readouterr()
    eng = Run(0, 16, np.array(DA.RUN_EMB), np.array([13, 32, 16]), np.array([16 + 5 * 4 // 2, 32, 1]), DA._Loader(loader), None,
              None, None, None, eg, ProcessArgs(DA.FLAGS + extra))
    out = capsys.readouterr().out
    return eng, [float(x) for x in re.findall(r"Loss = ([0-9.eE+-]+),", out)], out


def test_save_then_load_continues_the_schedule(own_stream, tmp_path, capsys):
    """2k = 16 steps in one run against k = 8 steps saved and k more from the loaded file: the split lies inside the decay (steps
    6 .. 10), so a counter that restarted would send the second half through the warm-up again."""
    import test_dense_adagrad as DA
    from rowwise_adagrad_restated import criteo_batches
    k = 8
    lS_o = torch.arange(64).repeat(len(DA.RUN_EMB), 1)
    batches = [(X, lS_o, idx, T) for X, idx, T in criteo_batches(DA.RUN_EMB, 13, 64, 2 * k, 5)]
    half, plain = str(tmp_path / "half.pt"), str(tmp_path / "plain.pt")
    eng_w, loss_w, out_w = _cli(batches, SCHED_FLAGS, capsys)
    assert eng_w.lr_cells and len(loss_w) == 2 * k - 1
    _cli(batches[:k], SCHED_FLAGS + ["--save-model=" + half], capsys)
    assert torch.load(half)["lr_step"] == k
    eng_b, loss_b, out_b = _cli(batches[k:], SCHED_FLAGS + ["--load-model=" + half], capsys)
    # printed: the first line of a run averages its steps 0 and 1 (fp64 sums of loss * 64), then one step per line
    assert loss_b == [(loss_w[k - 1] * 64 + loss_w[k] * 64) / 128] + loss_w[k + 1:]
    assert "lr_step" not in out_b
    # one line at start names W, S0 and N; one rate line behind every statistics line, with the two effective rates
    for out, first in ((out_w, 2), (out_b, k + 2)):
        lines = out.splitlines()
        assert len([l for l in lines if l.startswith("Learning-rate schedule:")]) == 1
        head = [l for l in lines if l.startswith("Learning-rate schedule:")][0]
        assert all(re.search(r"\b%d\b" % v, head) for v in (W_, S0_, N_))
        at = [i for i, l in enumerate(lines) if l.startswith("Epoch ") and "Loss = " in l]
        rate = [i for i, l in enumerate(lines) if l.startswith("Learning rates at step")]
        assert rate == [i + 1 for i in at]
        for n, i in enumerate(rate):
            s = first + n
            m = re.match(r"Learning rates at step (\d+): (\S+) \(MLPs\), (\S+) \(embeddings\)$", lines[i])
            assert m and int(m.group(1)) == s
            # (printed with float32's shortest digits: they read back as the same float32)
            assert (np.float32(m.group(2)), np.float32(m.group(3))) == (effective_rate(0.05, SCHED.factor(s)),
                                                                        effective_rate(0.01, SCHED.factor(s)))
            assert len(m.group(2)) <= 14 and len(m.group(3)) <= 14
    # a restarted counter would show: the resumed run without the stored counter trains other losses, and says so in one line
    ck = torch.load(half)
    del ck["lr_step"]
    torch.save(ck, plain)
    _, loss_r, out_r = _cli(batches[k:], SCHED_FLAGS + ["--load-model=" + plain], capsys)
    assert len([l for l in out_r.splitlines() if "lr_step" in l]) == 1 and loss_r != loss_b
    # without a schedule: no line of either kind, no cells
    eng_n, loss_n, out_n = _cli(batches[:k], [], capsys)
    assert "Learning" not in out_n and "lr_step" not in out_n and not eng_n.lr_cells
    assert len(loss_n) == k - 1 and loss_n != loss_w[:k - 1]


def test_main_cli_takes_the_flags_on_criteo_synthetic(own_stream, capsys):
    import test_dense_adagrad as DA
    from cdlrm_amd import main_no_ddp
    losses = {}
    for name, extra in (("plain", []), ("scheduled", SCHED_FLAGS)):
        capsys.readouterr()
        main_no_ddp.main(DA.FLAGS + ["--num-batches=16"] + extra)
        out = capsys.readouterr().out
        losses[name] = [float(x) for x in re.findall(r"Loss = ([0-9.eE+-]+),", out)]
        assert len(losses[name]) == 15 and np.isfinite(losses[name]).all()
        assert out.count("Learning rates at step") == (15 if extra else 0)
        assert ("Learning-rate schedule:" in out) == bool(extra)
    assert losses["plain"] != losses["scheduled"]


def test_the_cli_tests_leave_the_current_stream_as_they_found_it():
    """(runs behind them: a later test module of the suite records its tapes on whatever stream is current)"""
    assert torch.cuda.current_stream() == _AT_START["stream"]
