"""TrainEngine(matmul_precision="bf16") end to end on the MI355X: the opt-in bf16 matrix-core mode of the MLP GEMMs
("bf16 mode") over whole training runs.

The configuration has at least two eligible layers (K >= 32 and N >= 32) in each MLP: D = 64, bottom 13-128-64 (the 13-wide first
layer stays fp32), top 100-128-64-1 (the head stays fp32).  50 steps, the window pipeline of the parity tests.
  * the cache tag state does not depend on values: bit-exact against the fp32 engine;
  * the loss trajectory stays within LOSS_RTOL of the fp32 one (bf16 operands move a logit by ~2^-9 relative per product,
    the BCE loss of these runs by well under 1 %), and is NOT bit-identical to it (the mode is on);
  * two bf16 runs, taped and untaped steps, defer_top_update on and off, and the constructor keyword against a setattr after
    construction all give the same bits;
  * ONE step against a float64 restatement of it written here, with the bf16 rounding of the eligible GEMMs' operands: the
    updated MLP weights and biases within a stated bound (test_one_step_against_float64);
  * two ranks on one GPU (gloo), with and without defer_top_update: both ranks end with bitwise-identical MLP weights.
"""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import test_engine_parity as P      # noqa: E402  (the engine builder and batch stream of the parity tests)

DEV = "cuda:0"
STEPS = 50
# per-step loss, bf16 against fp32: measured on the MI355X at most 4.4e-5 relative over the 50 steps below and 6.2e-5 over the CLI
# run's 12; the bound leaves a margin of ~3x over the larger
LOSS_RTOL = 2e-4


class Cfg(dict):
    """The fields of a golden file the parity tests' builder reads."""

    @property
    def files(self):
        return list(self.keys())


CFG = Cfg(ln_emb=np.array([4000, 300, 9000, 50, 2500, 7000, 120, 3000]), m_spa=np.array(64), ln_bot=np.array([13, 128, 64]),
          top=np.array([128, 64, 1]), cache_size=np.array(1500), ways=np.array(4), B=np.array(512), L=np.array(10),
          nbatch=np.array(STEPS), seed=np.array(7), lr=np.array(0.1), lr_emb=np.array(0.3), alpha=np.array(1.2))


def _run(precision="fp32", setattr_after=False, tape=True, defer=False):
    from cdlrm_amd.engine import TrainEngine
    g = CFG
    host, cg, dl, eng0, pipe = P.build(g)
    kw = {} if (precision == "fp32" or setattr_after) else {"matmul_precision": precision}
    eng = TrainEngine(cg, dl, host, lr=eng0.lr, lr_embeds=eng0.lr_embeds, defer_top_update=defer, **kw)
    if setattr_after:
        eng.matmul_precision = precision
    eng.use_tape = tape
    L = int(g["L"])
    batches = P.make_batches(g)
    dev_idx = [b[1].to(DEV) for b in batches]
    losses = []
    for j, (X, lS_i, Tt) in enumerate(batches):
        if j % L == 0:
            win = torch.cat([b[1] for b in batches[j:j + L]], dim=1).to(DEV)
            torch.manual_seed(5000 + j)
            pipe.plan_window(win)
            pipe.commit()
            pipe.wait_writeback()
        nxt = dev_idx[j + 1] if j + 1 < len(batches) and (j + 1) % L != 0 else None
        loss = eng.step(X.to(DEV), dev_idx[j], Tt.to(DEV), j=j, next_idx=nxt)
        losses.append(float(loss[0]))
    eng.finish()
    torch.cuda.synchronize()
    from cdlrm_amd.model_no_ddp import _linears
    weights = [l.weight.data.clone().cpu() for l in _linears(dl.bot_l) + _linears(dl.top_l)]
    weights += [l.bias.data.clone().cpu() for l in _linears(dl.bot_l) + _linears(dl.top_l)]
    tags = [t.clone().cpu() for t in cg.occupancy_tables]
    return np.array(losses), tags, weights


@pytest.fixture(scope="module")
def runs():
    return {"fp32": _run("fp32"), "bf16": _run("bf16")}


def test_bf16_run_against_fp32(runs):
    l32, tags32, w32 = runs["fp32"]
    l16, tags16, w16 = runs["bf16"]
    assert len(tags32) == len(tags16) and all(torch.equal(a, b) for a, b in zip(tags32, tags16)), "tag state differs"
    assert np.all(np.isfinite(l16))
    rel = np.abs(l16 - l32) / np.abs(l32)
    print("bf16 vs fp32 over %d steps: max relative loss difference %.3e, final %.6f vs %.6f" % (STEPS, rel.max(), l16[-1],
                                                                                                l32[-1]))
    assert rel.max() <= LOSS_RTOL, rel
    assert not np.array_equal(l16, l32) or not all(torch.equal(a, b) for a, b in zip(w16, w32)), "bf16 run equals fp32"
    assert not all(torch.equal(a, b) for a, b in zip(w16, w32)), "bf16 weights equal fp32 weights"


def test_bf16_runs_are_reproducible(runs):
    l16, tags16, w16 = runs["bf16"]
    l2, tags2, w2 = _run("bf16")
    assert np.array_equal(l16, l2)
    assert all(torch.equal(a, b) for a, b in zip(w16, w2))


def test_bf16_setattr_equals_constructor_keyword(runs):
    l16, _, w16 = runs["bf16"]
    l2, _, w2 = _run("bf16", setattr_after=True)
    assert np.array_equal(l16, l2)
    assert all(torch.equal(a, b) for a, b in zip(w16, w2))


def test_bf16_untaped_steps_give_the_same_bits(runs):
    l16, _, w16 = runs["bf16"]
    l2, _, w2 = _run("bf16", tape=False)
    assert np.array_equal(l16, l2)
    assert all(torch.equal(a, b) for a, b in zip(w16, w2))


def test_bf16_defer_top_update_gives_the_same_bits(runs):
    l16, _, w16 = runs["bf16"]
    l2, _, w2 = _run("bf16", defer=True)
    assert np.array_equal(l16, l2)
    assert all(torch.equal(a, b) for a, b in zip(w16, w2))


def test_precision_switch_between_steps_never_replays_the_other_tape():
    """matmul_precision switched every second step on one engine: taped steps give the bits of untaped ones, so no tape
    recorded under one precision was replayed under the other (the precision is part of the tape key)."""
    from cdlrm_amd.engine import TrainEngine
    out = []
    for tape in (True, False):
        host, cg, dl, eng0, pipe = P.build(CFG)
        eng = TrainEngine(cg, dl, host, lr=eng0.lr, lr_embeds=eng0.lr_embeds)
        eng.use_tape = tape
        batches = P.make_batches(CFG)[:10]
        win = torch.cat([b[1] for b in batches], dim=1).to(DEV)
        torch.manual_seed(5000)
        pipe.plan_window(win)
        pipe.commit()
        pipe.wait_writeback()
        losses = []
        for j, (X, lS_i, Tt) in enumerate(batches):
            eng.matmul_precision = "bf16" if (j // 2) % 2 else "fp32"
            losses.append(float(eng.step(X.to(DEV), lS_i.to(DEV), Tt.to(DEV), j=j)[0]))
        eng.finish()
        out.append(losses)
    assert out[0] == out[1]


def test_cli_matmul_precision(capsys):
    """python -m cdlrm_amd.main_no_ddp --matmul-precision=bf16 on a tiny configuration runs, and its losses differ from the fp32
    run's within LOSS_RTOL."""
    import re
    from cdlrm_amd import main_no_ddp
    flags = ["--arch-sparse-feature-size=32", "--arch-mlp-bot=13-64-32", "--arch-mlp-top=64-32-1",
             "--arch-embedding-size=3000-50-7-1200-40000", "--mini-batch-size=256", "--lookahead=4", "--cache-size=400",
             "--num-ways=4", "--loss-function=bce", "--round-targets=True", "--learning-rate=0.1", "--lr-embeds=0.3",
             "--print-freq=1", "--world-size=1", "--numpy-rand-seed=11", "--data-generation=criteo-synthetic",
             "--num-batches=12"]
    out = {}
    saved = torch.cuda.current_stream()         # Run trains on a stream of its own and leaves it current: restore ours
    try:
        for prec in ("fp32", "bf16"):
            main_no_ddp.main(flags + ["--matmul-precision=" + prec])
            text = capsys.readouterr().out
            out[prec] = np.array([float(x) for x in re.findall(r"Loss = ([0-9.eE+-]+),", text)])
    finally:
        torch.cuda.synchronize()
        torch.cuda.set_stream(saved)
    assert len(out["bf16"]) == len(out["fp32"]) >= 10
    assert np.all(np.isfinite(out["bf16"]))
    rel = np.abs(out["bf16"] - out["fp32"]) / np.abs(out["fp32"])
    print("CLI bf16 vs fp32: max relative loss difference %.3e" % rel.max())
    assert rel.max() <= LOSS_RTOL
    assert not np.array_equal(out["bf16"], out["fp32"])


# ---- one step against a float64 restatement ------------------------------------------------------------------------------

def _r(t):
    """float64 of the bf16 rounding (round-to-nearest-even) of t."""
    return t.to(torch.bfloat16).double()


class _Lin(torch.autograd.Function):
    """Y = X W^T + b in float64; with `rnd` the GEMM operands are rounded to bf16 as the kernels round them: X and W forward,
    dZ and W for dX, dZ and X for dW; db is the column sum of the unrounded dZ.  Records (layer, rounded dZ, rounded X) for the
    bound."""

    @staticmethod
    def forward(ctx, x, W, b, rnd, key, rec):
        ctx.save_for_backward(x, W)
        ctx.rnd, ctx.key, ctx.rec = rnd, key, rec
        f = _r if rnd else (lambda t: t)
        return f(x) @ f(W).T + b

    @staticmethod
    def backward(ctx, g):
        x, W = ctx.saved_tensors
        f = _r if ctx.rnd else (lambda t: t)
        ctx.rec[ctx.key] = (f(g).detach(), f(x).detach())
        return f(g) @ f(W), f(g).T @ f(x), g.sum(0), None, None, None


def test_one_step_against_float64():
    """One bf16 step (world 1, the whole-network weight-gradient plan, SGD after it) against the same step restated in float64
    with the bf16 rounding of the eligible GEMMs' operands.  Bound on every updated weight:
        |W1 - W1_ref| <= lr * (2^-7 + 2 K 2^-24) * (|dZ|^T |X|)_ij + 2^-23 |W1_ref|_ij
    2 K 2^-24 (|dZ|^T |X|) is the fp32-chain bound of the kernels' accumulation (test_gemm_routes.py); 2^-7 allows each of a
    product's two factors to round to the neighbouring bf16 value in one computation and not in the other (the fp32 activations
    the engine rounds are not exactly the float64 ones), 2^-8 each; 2^-23 |W| the fp32 rounding of the update.  Biases the same
    with sum |dZ|.  The bound is tighter than the update itself on at least a quarter of each layer's weights (checked): a
    skipped SGD step fails it, as would a gradient taken from a wrong or stale buffer."""
    from cdlrm_amd.engine import TrainEngine
    from cdlrm_amd.model_no_ddp import _linears
    from oracle import cdlrm_oracle as O
    host, cg, dl, eng0, pipe = P.build(CFG)
    eng = TrainEngine(cg, dl, host, lr=eng0.lr, lr_embeds=eng0.lr_embeds, matmul_precision="bf16")
    lr = eng.lr
    batches = P.make_batches(CFG)
    X, lS_i, Tt = batches[0]
    rows = [host.emb_l[k].weight.data[lS_i[k]].double().clone() for k in range(len(CFG["ln_emb"]))]
    layers = [(l, a) for l, a in eng.bot] + [(l, a) for l, a in eng.top]
    W0 = [l.weight.data.double().cpu().clone() for l, _ in layers]
    b0 = [l.bias.data.double().cpu().clone() for l, _ in layers]
    win = torch.cat([b[1] for b in batches[:int(CFG["L"])]], dim=1).to(DEV)
    torch.manual_seed(5000)
    pipe.plan_window(win)
    pipe.commit()
    pipe.wait_writeback()
    loss = float(eng.step(X.to(DEV), lS_i.to(DEV), Tt.to(DEV), j=0)[0])
    eng.finish()
    torch.cuda.synchronize()
    W1 = [l.weight.data.double().cpu() for l, _ in layers]
    b1 = [l.bias.data.double().cpu() for l, _ in layers]
    # the restatement
    Ws = [w.clone().requires_grad_(True) for w in W0]
    bs = [b.clone().requires_grad_(True) for b in b0]
    rec = {}

    def mlp(x, ls, first):
        for i, (l, act) in enumerate(ls):
            q = first + i
            rnd = l.out_features >= 32 and l.in_features >= 32
            x = _Lin.apply(x, Ws[q], bs[q], rnd, q, rec)
            x = torch.relu(x) if act == 1 else torch.sigmoid(x) if act == 2 else x
        return x

    xb = mlp(X.double(), eng.bot, 0)
    R = O.interact_features(xb, rows, "dot", False)
    z = mlp(R, eng.top, len(eng.bot))
    loss_ref = torch.nn.functional.binary_cross_entropy(z, Tt.double())
    loss_ref.backward()
    assert abs(loss - loss_ref.item()) <= 1e-5 * loss_ref.item(), (loss, loss_ref.item())
    U = 2.0 ** -24
    M = X.shape[0]
    for q, (l, _) in enumerate(layers):
        gz, x = rec[q]
        mag_w = (gz.abs().T @ x.abs()).numpy()
        mag_b = gz.abs().sum(0).numpy()
        ref_w = (W0[q] - lr * Ws[q].grad.detach()).numpy()
        ref_b = (b0[q] - lr * bs[q].grad.detach()).numpy()
        bound_w = lr * (2.0 ** -7 + 2 * M * U) * mag_w + 2 * U * np.abs(ref_w) + 1e-30
        bound_b = lr * (2.0 ** -7 + 2 * M * U) * mag_b + 2 * U * np.abs(ref_b) + 1e-30
        err_w = np.abs(W1[q].numpy() - ref_w)
        err_b = np.abs(b1[q].numpy() - ref_b)
        assert (err_w <= bound_w).all(), "layer %d weight: worst |err| / bound %.3g" % (q, (err_w / bound_w).max())
        assert (err_b <= bound_b).all(), "layer %d bias: worst |err| / bound %.3g" % (q, (err_b / bound_b).max())
        # negative control: the bound is tighter than the update itself on at least a quarter of every layer's weights
        # (measured: 43 % on the tightest layer, the 128 -> 64 top layer; the rest are updates that cancel over the batch or are
        # zero -- inputs a ReLU kept at 0), so a skipped SGD step, or a gradient from a wrong buffer, fails it
        frac = (np.abs(W0[q].numpy() - ref_w) > bound_w).mean()
        assert frac > 0.25, "layer %d: the bound is not tighter than the update (%.3f)" % (q, frac)


# ---- two ranks on one GPU ------------------------------------------------------------------------------------------------

def _rank_worker(rank, world, port, host_shared, defer, ret):
    import faulthandler
    faulthandler.dump_traceback_later(150, exit=True)
    try:
        ret.put((rank, _rank_body(rank, world, port, host_shared, defer)))
    except BaseException:
        import traceback
        ret.put((rank, {"error": traceback.format_exc()}))
        raise


def _rank_body(rank, world, port, host_shared, defer):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import torch.distributed as dist
    import cdlrm_amd.engine as engine
    import cdlrm_amd.model_no_ddp as Mo
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.cuda.set_device(0)
    g = CFG
    ln_emb = np.array([int(x) for x in g["ln_emb"]])
    m_spa, seed, B, L = int(g["m_spa"]), int(g["seed"]), int(g["B"]), int(g["L"])
    nf = len(ln_emb) + 1
    ln_top = np.array([m_spa + nf * (nf - 1) // 2] + [int(x) for x in g["top"]])
    eg = Mo.Embedding_Table_Group(m_spa, ln_emb, init="empty_meta")
    for k in range(len(ln_emb)):
        eg.emb_l[k].weight.data = host_shared[k]
    eg.register_shared()
    np.random.seed(seed)
    torch.manual_seed(seed)
    cg = Mo.Embedding_Table_Cache_Group(m_spa, ln_emb, int(g["cache_size"]), B, int(g["ways"])).to(DEV)
    dl = Mo.DLRM_Net(np.array(g["ln_bot"]), ln_top, "dot", False, True, -1, ln_top.size - 2, 0.0).to(DEV)
    eng = engine.TrainEngine(cg, dl, eg, lr=float(g["lr"]), lr_embeds=float(g["lr_emb"]), world_size=world, rank=rank,
                             table_agg_freq=3, table_agg_op="mean", defer_top_update=defer, matmul_precision="bf16")
    pipe = engine.WindowPipeline(cg, eg, L * B, parity_rng=True, rank=rank, world_size=world)
    lbs = B // world
    sl = slice(rank * lbs, (rank + 1) * lbs)
    batches = P.make_batches(g)[:20]
    losses = []
    for j, (X, lS_i, Tt) in enumerate(batches):
        if j % L == 0:
            eng.sync_touched_to_rank0()
            torch.manual_seed(5000 + j)
            pipe.plan_window(torch.cat([b[1] for b in batches[j:j + L]], dim=1).to(DEV))
            pipe.commit()
            pipe.wait_writeback()
        loss = eng.step(X[sl].to(DEV), lS_i[:, sl].contiguous().to(DEV), Tt[sl].to(DEV), j=j)
        losses.append(float(loss[0]))
    eng.finish()
    torch.cuda.synchronize()
    lin = Mo._linears(dl.bot_l) + Mo._linears(dl.top_l)
    out = dict(losses=np.array(losses), w=[l.weight.data.cpu().numpy() for l in lin])
    dist.barrier()
    dist.destroy_process_group()
    return out


@pytest.mark.parametrize("defer,port", [(False, 29861), (True, 29862)])
def test_two_ranks_one_gpu_bf16_weights_identical(defer, port):
    """Two ranks in bf16 mode (the multi-rank step: weight gradients, their all-reduce, then the SGD step; with defer_top_update
    the split plans with the top MLP's exchange on the side stream): both ranks end with bitwise-identical MLP weights, which
    moved away from the initial ones."""
    import torch.multiprocessing as mp
    from oracle import cdlrm_oracle as O
    np.random.seed(int(CFG["seed"]))
    host = [h.share_memory_() for h in O.init_host_tables([int(x) for x in CFG["ln_emb"]], int(CFG["m_spa"]))]
    ctx = mp.get_context("spawn")
    ret = ctx.Queue()
    procs = [ctx.Process(target=_rank_worker, args=(r, 2, port, host, defer, ret)) for r in range(2)]
    for p in procs:
        p.start()
    got = {}
    for _ in range(2):
        r, payload = ret.get(timeout=300)
        assert "error" not in payload, payload["error"]
        got[r] = payload
    for p in procs:
        p.join(timeout=60)
    assert all(np.all(np.isfinite(got[r]["losses"])) for r in range(2))
    for i, (a, b) in enumerate(zip(got[0]["w"], got[1]["w"])):
        assert np.array_equal(a, b), "layer %d: the ranks' weights differ" % i
    assert not np.array_equal(got[0]["losses"], got[1]["losses"])        # each rank trained on its own slice
