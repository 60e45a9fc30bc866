"""TrainEngine(matmul_precision="bf16x3") end to end on the MI355X: the opt-in split-operand mode of the MLP GEMMs (DESIGN.md
section 4.2) over whole training runs, on test_engine_bf16.py's configuration and builder (three eligible layers: bottom
128 -> 64, top 100 -> 128 -> 64).

  * the cache tag state does not depend on values: bit-exact against the fp32 engine;
  * the loss trajectory is finite, NOT bit-identical to the fp32 one (the mode is on), and its largest relative deviation from
    it is at most 1/8 of the bf16 mode's, both measured in the same test run (the operand errors stand as 3 * 2^-16 to 2^-8,
    ~1/170; an eighth leaves room for the fp32 accumulation both modes share);
  * two runs, taped and untaped steps, defer_top_update on and off, and the constructor keyword against a setattr after
    construction all give the same bits; so do taped and untaped steps with the precision cycled fp32 -> bf16 -> bf16x3;
  * ONE step against a float64 restatement of it written here with the SPLIT operands of the eligible GEMMs and the three
    products of the mode (test_one_step_against_float64);
  * the CLI choice runs; two ranks on one GPU (gloo) end with bitwise-identical MLP weights.
"""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import test_engine_bf16 as E        # noqa: E402  (the configuration and the 50-step run)
import test_engine_parity as P      # noqa: E402  (the engine builder and batch stream of the parity tests)

DEV = "cuda:0"
PREC = "bf16x3"
CFG = E.CFG


@pytest.fixture(scope="module")
def runs():
    return {p: E._run(p) for p in ("fp32", "bf16", PREC)}


def _same(a, b):
    return np.array_equal(a[0], b[0]) and all(torch.equal(x, y) for x, y in zip(a[2], b[2]))


def test_bf16x3_run_against_fp32_and_bf16(runs):
    l32, tags32, w32 = runs["fp32"]
    l16, _, _ = runs["bf16"]
    l3, tags3, w3 = runs[PREC]
    assert len(tags32) == len(tags3) and all(torch.equal(a, b) for a, b in zip(tags32, tags3)), "tag state differs"
    assert np.all(np.isfinite(l3))
    dev3 = (np.abs(l3 - l32) / np.abs(l32)).max()
    dev16 = (np.abs(l16 - l32) / np.abs(l32)).max()
    print("max relative loss deviation from fp32 over %d steps: bf16x3 %.3e, bf16 %.3e (ratio 1/%.1f)" % (
        E.STEPS, dev3, dev16, dev16 / max(dev3, 1e-300)))
    assert not np.array_equal(l3, l32), "bf16x3 losses are the fp32 bits"
    assert not all(torch.equal(a, b) for a, b in zip(w3, w32)), "bf16x3 weights equal fp32 weights"
    assert not np.array_equal(l3, l16), "bf16x3 losses are the bf16 mode's bits"
    assert dev3 <= dev16 / 8, (dev3, dev16)


def test_bf16x3_runs_are_reproducible(runs):
    assert _same(runs[PREC], E._run(PREC))


def test_bf16x3_setattr_equals_constructor_keyword(runs):
    assert _same(runs[PREC], E._run(PREC, setattr_after=True))


def test_bf16x3_untaped_steps_give_the_same_bits(runs):
    assert _same(runs[PREC], E._run(PREC, tape=False))


def test_bf16x3_defer_top_update_gives_the_same_bits(runs):
    assert _same(runs[PREC], E._run(PREC, defer=True))


def test_precision_cycle_never_replays_another_precisions_tape():
    """matmul_precision cycled fp32 -> bf16 -> bf16x3 every two steps on one engine: taped steps give the bits of untaped ones
    (the precision is part of the tape key), and the three precisions' steps are not all alike."""
    from cdlrm_amd.engine import TrainEngine
    cycle = ("fp32", "bf16", PREC)
    out = []
    for tape in (True, False):
        host, cg, dl, eng0, pipe = P.build(CFG)
        eng = TrainEngine(cg, dl, host, lr=eng0.lr, lr_embeds=eng0.lr_embeds)
        eng.use_tape = tape
        batches = P.make_batches(CFG)[:14]
        win = torch.cat([b[1] for b in batches], dim=1).to(DEV)
        torch.manual_seed(5000)
        pipe.plan_window(win)
        pipe.commit()
        pipe.wait_writeback()
        losses = []
        for j, (X, lS_i, Tt) in enumerate(batches):
            eng.matmul_precision = cycle[(j // 2) % 3]
            losses.append(float(eng.step(X.to(DEV), lS_i.to(DEV), Tt.to(DEV), j=j)[0]))
        eng.finish()
        assert {"wgrad_" + p for p in cycle} <= set(eng._buffers(batches[0][0].shape[0])), "a precision without its own plans"
        out.append(losses)
    assert out[0] == out[1]


def test_cli_matmul_precision_bf16x3(capsys):
    """python -m cdlrm_amd.main_no_ddp --matmul-precision=bf16x3 on test_engine_bf16's tiny configuration runs; its losses are
    finite and within that test's bf16 tolerance of the fp32 run's."""
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
        for prec in ("fp32", PREC):
            main_no_ddp.main(flags + ["--matmul-precision=" + prec])
            text = capsys.readouterr().out
            out[prec] = np.array([float(x) for x in re.findall(r"Loss = ([0-9.eE+-]+),", text)])
    finally:
        torch.cuda.synchronize()
        torch.cuda.set_stream(saved)
    assert len(out[PREC]) == len(out["fp32"]) >= 10
    assert np.all(np.isfinite(out[PREC]))
    rel = np.abs(out[PREC] - out["fp32"]) / np.abs(out["fp32"])
    print("CLI bf16x3 vs fp32: max relative loss difference %.3e" % rel.max())
    assert rel.max() <= E.LOSS_RTOL


# ---- one step against a float64 restatement ----------------------------------------------------------------------------------

def _split(t):
    """(h, l) in float64: h = bf16(x), l = bf16(x - h) of the fp32 value x of t, as the kernels split."""
    x = t.float()
    h = x.to(torch.bfloat16).float()
    l = (x - h).to(torch.bfloat16).float()
    return h.double(), l.double()


def _mm3(a, b):
    """a @ b the way the mode multiplies: al bh + ah bl + ah bh, in float64."""
    (ah, al), (bh, bl) = _split(a), _split(b)
    return al @ bh + ah @ bl + ah @ bh


class _Lin(torch.autograd.Function):
    """Y = X W^T + b in float64; with `x3` every GEMM multiplies the split operands as the kernels do: X and W forward, dZ and
    W for dX, dZ and X for dW; db is the column sum of the unsplit dZ.  Records (layer, dZ, X) for the bound."""

    @staticmethod
    def forward(ctx, x, W, b, x3, key, rec):
        ctx.save_for_backward(x, W)
        ctx.x3, ctx.key, ctx.rec = x3, key, rec
        return (_mm3(x, W.T) if x3 else x @ W.T) + b

    @staticmethod
    def backward(ctx, g):
        x, W = ctx.saved_tensors
        ctx.rec[ctx.key] = (g.detach(), x.detach())
        if ctx.x3:
            return _mm3(g, W), _mm3(g.T, x), g.sum(0), None, None, None
        return g @ W, g.T @ x, g.sum(0), None, None, None


def test_one_step_against_float64():
    """One bf16x3 step (world 1, the whole-network weight-gradient plan, SGD after it) against the same step restated in float64
    with the split operands and three products of the eligible GEMMs.  Bound on every updated weight, test_engine_bf16's with
    its 2^-7 term replaced:
        |W1 - W1_ref| <= lr * (4 * 2^-16 + 2 M 2^-24) * (|dZ|^T |X|)_ij + 2^-23 |W1_ref|_ij
    2 M 2^-24 (|dZ|^T |X|) is the fp32-chain bound of the kernels' accumulation; 4 * 2^-16 allows each of a product's two
    factors to split differently by one lo-ulp (2^-16 of the value, twice for a rounding boundary) in one computation and not
    in the other -- the fp32 activations the engine splits are not exactly the float64 ones; 2^-23 |W| the fp32 rounding of the
    update.  Biases the same with sum |dZ|.  The bound is tighter than the update itself on more than a quarter of each
    layer's weights (checked): a skipped SGD step fails it, as would a gradient taken from a wrong or stale buffer."""
    from cdlrm_amd.engine import TrainEngine
    from oracle import cdlrm_oracle as O
    host, cg, dl, eng0, pipe = P.build(CFG)
    eng = TrainEngine(cg, dl, host, lr=eng0.lr, lr_embeds=eng0.lr_embeds, matmul_precision=PREC)
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
            x3 = l.out_features >= 32 and l.in_features >= 32
            x = _Lin.apply(x, Ws[q], bs[q], x3, q, rec)
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
    n_x3 = 0
    for q, (l, _) in enumerate(layers):
        n_x3 += l.out_features >= 32 and l.in_features >= 32
        gz, x = rec[q]
        mag_w = (gz.abs().T @ x.abs()).numpy()
        mag_b = gz.abs().sum(0).numpy()
        ref_w = (W0[q] - lr * Ws[q].grad.detach()).numpy()
        ref_b = (b0[q] - lr * bs[q].grad.detach()).numpy()
        bound_w = lr * (4 * 2.0 ** -16 + 2 * M * U) * mag_w + 2 * U * np.abs(ref_w) + 1e-30
        bound_b = lr * (4 * 2.0 ** -16 + 2 * M * U) * mag_b + 2 * U * np.abs(ref_b) + 1e-30
        err_w = np.abs(W1[q].numpy() - ref_w)
        err_b = np.abs(b1[q].numpy() - ref_b)
        print("layer %d: worst |err| / bound, weight %.3g, bias %.3g" % (q, (err_w / bound_w).max(), (err_b / bound_b).max()))
        assert (err_w <= bound_w).all(), "layer %d weight: worst |err| / bound %.3g" % (q, (err_w / bound_w).max())
        assert (err_b <= bound_b).all(), "layer %d bias: worst |err| / bound %.3g" % (q, (err_b / bound_b).max())
        # negative control: the bound is tighter than the update itself on more than a quarter of every layer's weights, so a
        # skipped SGD step, or a gradient from a wrong buffer, fails it
        frac = (np.abs(W0[q].numpy() - ref_w) > bound_w).mean()
        assert frac > 0.25, "layer %d: the bound is not tighter than the update (%.3f)" % (q, frac)
    assert n_x3 == 3        # bottom 128 -> 64, top 100 -> 128 and 128 -> 64: the restatement did split operands


# ---- two ranks on one GPU ----------------------------------------------------------------------------------------------------

def _rank_worker(rank, world, port, host_shared, ret):
    import faulthandler
    faulthandler.dump_traceback_later(150, exit=True)
    try:
        ret.put((rank, _rank_body(rank, world, port, host_shared)))
    except BaseException:
        import traceback
        ret.put((rank, {"error": traceback.format_exc()}))
        raise


def _rank_body(rank, world, port, host_shared):
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
    lin = Mo._linears(dl.bot_l) + Mo._linears(dl.top_l)
    w0 = [l.weight.data.cpu().numpy().copy() for l in lin]
    eng = engine.TrainEngine(cg, dl, eg, lr=float(g["lr"]), lr_embeds=float(g["lr_emb"]), world_size=world, rank=rank,
                             table_agg_freq=3, table_agg_op="mean", matmul_precision=PREC)
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
    out = dict(losses=np.array(losses), w=[l.weight.data.cpu().numpy() for l in lin], w0=w0)
    dist.barrier()
    dist.destroy_process_group()
    return out


def test_two_ranks_one_gpu_bf16x3_weights_identical():
    """Two ranks in bf16x3 mode (the multi-rank step: weight gradients, their all-reduce, then the SGD step): both ranks end with
    bitwise-identical MLP weights, which moved away from the initial ones."""
    import torch.multiprocessing as mp
    from oracle import cdlrm_oracle as O
    np.random.seed(int(CFG["seed"]))
    host = [h.share_memory_() for h in O.init_host_tables([int(x) for x in CFG["ln_emb"]], int(CFG["m_spa"]))]
    ctx = mp.get_context("spawn")
    ret = ctx.Queue()
    procs = [ctx.Process(target=_rank_worker, args=(r, 2, 29871, host, ret)) for r in range(2)]
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
        assert not np.array_equal(a, got[0]["w0"][i]), "layer %d: the weights did not move" % i
    assert not np.array_equal(got[0]["losses"], got[1]["losses"])        # each rank trained on its own slice
