"""Ragged multi-hot bags data-parallel across ranks (engine.BagWindows, csrc/bags.hip): rank r trains
samples [r * lbs, min(B, (r + 1) * lbs)) and takes of every table exactly the lookups of those bags, cut on the device from
the window's global lists.  The kernels against the host definition (square_bags / pad_window of the host-sliced lists), the
one-lookup-per-bag case against the reference's 2-rank golden runs, ragged bags at 2 and 3 ranks against the oracle with
the bag-range slice, and the CLI at --world-size=2 with the reference's default random front end.  The ranks run as
processes on the one GPU of the test box with gloo collectives, as in test_multirank_gpu.py."""
import math
import os
import re
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"


# ------------------------------------------------------------------------------------------------ kernels vs host definition

def _host_rank_slice(lS_o, lS_i, lbs, rank):
    """The definition on the host: the rank's bags (samples [r * lbs, (r + 1) * lbs) of the batch, lbs = the run's local
    batch), their lookups, offsets rebased -> square_bags()."""
    from cdlrm_amd.engine import square_bags
    off = torch.as_tensor(lS_o)
    T, B = off.shape
    s0, s1 = min(B, rank * lbs), min(B, (rank + 1) * lbs)
    lists, offs = [], []
    for k in range(T):
        a = int(off[k, s0])
        e = int(off[k, s1]) if s1 < B else int(lS_i[k].numel())
        lists.append(lS_i[k][a:e])
        offs.append(off[k, s0:s1] - a)
    return square_bags(offs, lists), (s0, s1)


def _edge_batches():
    """Batches of 3 samples (mini-batch 3) whose bag sizes make rank slices of 1 lookup, exactly 256 / 512, and one past;
    a short one-sample batch whose tables hold 1, 256 and 257 lookups."""
    rng = np.random.RandomState(17)

    def batch(sizes):
        B = len(sizes[0])
        off = torch.from_numpy(np.stack([np.concatenate([[0], np.cumsum(s)[:-1]]) for s in sizes]).astype(np.int64))
        lists = [torch.from_numpy(rng.randint(0, 5000, size=int(sum(s))).astype(np.int64)) for s in sizes]
        return (torch.rand(B, 5), off, lists, torch.ones(B, 1))

    return [batch([[1, 256, 257], [256, 1, 255], [512, 3, 1]]),
            batch([[1], [256], [257]]),
            batch([[128, 1, 127], [1, 1, 1], [300, 44, 256]])]


def _random_batches(fixed, B=23):
    """6 batches of the random front end, the last one short: --data-size 134 at --mini-batch-size 23 (19 samples)."""
    from cdlrm_amd import dlrm_data_pytorch as DP
    args = SimpleNamespace(data_size=134, num_batches=0, mini_batch_size=B, num_indices_per_lookup=9,
                           num_indices_per_lookup_fixed=fixed, round_targets=True, data_generation="random", numpy_rand_seed=5)
    _, loader = DP.make_random_data_and_loader(args, np.array([900, 40, 6, 2500, 70]), 5)
    return [(X, lS_o, list(lS_i), Tt) for X, lS_o, lS_i, Tt in loader]


@pytest.mark.parametrize("source", ["edge", "random", "random_fixed"])
@pytest.mark.parametrize("world", [1, 2, 3])
def test_bag_kernels_equal_host_definition(source, world):
    from cdlrm_amd.engine import BagWindows, pad_window
    batches = _edge_batches() if source == "edge" else _random_batches(source == "random_fixed")
    assert source == "edge" or batches[-1][0].shape[0] == 19
    lbs = math.ceil((3 if source == "edge" else 23) / world)       # the run's local batch: ceil(mini_batch_size / W)
    T = len(batches[0][2])
    L = 3 if source == "edge" else 2
    wins = [batches[i:i + L] for i in range(0, len(batches), L)]

    def check(w, bw, rank):
        got_w = bw.window_indices()
        want_w = pad_window([torch.cat([b[2][k] for b in w]) for k in range(T)])
        assert torch.equal(got_w.cpu(), want_w)
        for b, (X, lS_o, lS_i, Tt) in enumerate(w):
            (want_o, want_i), (s0, s1) = _host_rank_slice(lS_o, lS_i, lbs, rank)
            got_o, got_i, rows = bw.rank_batch(b)
            assert rows == slice(s0, s1) and (s0, s1) == (rank * lbs, min(X.shape[0], (rank + 1) * lbs))
            assert got_i.shape[1] % 256 == 0 and got_o.shape == (T, s1 - s0 + 1)
            assert torch.equal(got_o.cpu(), want_o), (b, rank)
            assert torch.equal(got_i.cpu(), want_i), (b, rank)

    for rank in range(world):
        holders = BagWindows(T, DEV, lbs, world_size=world, rank=rank)
        wins_r = wins
        if source == "edge" and world > 1:
            with pytest.raises(ValueError, match="no sample"):     # the one-sample batch leaves ranks >= 1 without one
                holders.load(wins[0])
            wins_r = [[batches[0]], [batches[2]], [batches[2], batches[0]]]
        loaded = []
        for w in wins_r:
            loaded.append((w, holders.load(w)))
            check(*loaded[-1], rank)
        for w, bw in loaded[-2:]:             # more windows than the ring holds: the last two stay valid
            check(w, bw, rank)
        torch.cuda.synchronize()


def test_edge_slice_lengths_are_covered():
    """The edge batches do reach the lengths they are meant to: 1, 256, 257 and 512 lookups in one rank slice."""
    from cdlrm_amd.engine import rank_bag_slice
    X, off, lists, _ = _edge_batches()[0]
    lens = torch.tensor([x.numel() for x in lists])
    seen = set()
    for r in range(3):
        _, _, a, e, n = rank_bag_slice(off, lens, 1, r)          # mini-batch 3 over 3 ranks
        seen.update((e - a).tolist())
    assert {1, 256, 257, 512} <= seen


# ------------------------------------------------------------------------------------------------ ranks as processes

def _worker(rank, world, port, cfg, batches, host_shared, ret):
    import faulthandler
    faulthandler.dump_traceback_later(240, exit=True)
    try:
        _worker_body(rank, world, port, cfg, batches, host_shared, ret)
    except BaseException:
        import traceback
        ret.put((rank, {"error": traceback.format_exc()}))
        raise


def _worker_body(rank, world, port, cfg, batches, host_shared, ret):
    sys.path.insert(0, ROOT)
    import torch.distributed as dist
    import cdlrm_amd.engine as engine
    import cdlrm_amd.model_no_ddp as M
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.cuda.set_device(0)
    ln_emb = np.array(cfg["ln_emb"])
    m_spa, seed, L, aux, ways, cache = cfg["m_spa"], cfg["seed"], cfg["L"], cfg["aux"], cfg["ways"], cfg["cache_size"]
    eg = M.Embedding_Table_Group(m_spa, ln_emb, init="empty_meta")
    for k in range(len(ln_emb)):
        eg.emb_l[k].weight.data = host_shared[k]
    eg.register_shared()
    np.random.seed(seed)
    torch.manual_seed(seed)
    cg = M.Embedding_Table_Cache_Group(m_spa, ln_emb, cache, aux, ways).to(DEV)
    dl = M.DLRM_Net(np.array(cfg["ln_bot"]), np.array(cfg["ln_top"]), "dot", False, True, -1, len(cfg["ln_top"]) - 2,
                    0.0).to(DEV)
    if cfg.get("init_aux"):
        # the cache rows as a group with the golden run's aux region draws them (the N(0, 1) init runs table after table
        # over ways * P + aux rows); rows not yet filled by an insert are part of the golden's weight sums
        torch.manual_seed(seed)
        ref = M.Embedding_Table_Cache_Group(m_spa, ln_emb, cache, cfg["init_aux"], ways)
        for k in range(len(ln_emb)):
            nrow = ways * cg.cache_sizes[k]
            cg.emb_l[k].weight[:nrow].copy_(ref.emb_l[k].weight[:nrow])
    eng = engine.TrainEngine(cg, dl, eg, lr=cfg["lr"], lr_embeds=cfg["lr_emb"], world_size=world, rank=rank,
                             table_agg_freq=cfg["agg_freq"], table_agg_op=cfg["agg_op"], defer_top_update=cfg["defer"])
    pipe = engine.WindowPipeline(cg, eg, L * aux, parity_rng=True, rank=rank, world_size=world)
    bags = engine.BagWindows(len(ln_emb), DEV, cfg["lbs"], world_size=world, rank=rank)
    losses = []
    for j, (X, lS_o, lS_i, Tt) in enumerate(batches):
        if j % L == 0:
            eng.sync_touched_to_rank0()
            torch.manual_seed(cfg["seed_base"] + j)
            bw = bags.load(batches[j:j + L])
            pipe.plan_window(bw.window_indices())
            pipe.commit()
            pipe.wait_writeback()
        off, idx, sl = bw.rank_batch(j % L)
        loss = eng.step(X[sl].to(DEV), idx, Tt[sl].to(DEV), lS_o=off, j=j)
        losses.append(float(loss[0]))
    eng.finish()
    cg.ctx.check()
    lin = M._linears(dl.top_l)
    rows = [cg.emb_l[k].weight[:ways * cg.cache_sizes[k]].cpu().numpy() for k in range(len(ln_emb))]
    ret.put((rank, dict(losses=np.array(losses), occ=[o.cpu().numpy() for o in cg.occupancy_tables],
                        top_w=[l.weight.data.cpu().numpy() for l in lin], rows=rows,
                        wsum=[float(r.astype(np.float64).sum()) for r in rows])))
    dist.barrier()
    dist.destroy_process_group()


def _run_ranks(world, port, cfg, batches, host):
    ctx = mp.get_context("spawn")
    ret = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, world, port, cfg, batches, host, ret)) for r in range(world)]
    for p in procs:
        p.start()
    got = {}
    try:
        for _ in range(world):
            r, payload = ret.get(timeout=400)
            assert "error" not in payload, payload["error"]
            got[r] = payload
    finally:
        for p in procs:
            p.join(timeout=60)
            if p.is_alive():
                p.kill()
    return got


@pytest.mark.parametrize("name,port,defer", [("train_w2_mean", 29881, False), ("train_w2_freq1", 29882, True)])
def test_one_lookup_per_bag_reduces_to_the_reference(golden, name, port, defer):
    """The reference's 2-rank golden runs fed as multi-hot bags with lS_o = arange(B): the bag-range slice is the
    reference's lS_i[:, rank*b:(rank+1)*b] then, so losses, tags, top MLP, cache rows and host tables are the golden's."""
    from oracle import cdlrm_oracle as O
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from test_distributed_gloo import _batches
    g = golden(name)
    ln_emb = [int(x) for x in g["ln_emb"]]
    T, B, m_spa = len(ln_emb), int(g["B"]), int(g["m_spa"])
    nf = T + 1
    cfg = dict(ln_emb=ln_emb, m_spa=m_spa, seed=int(g["seed"]), L=int(g["L"]), lbs=-(-B // 2), aux=256, init_aux=B,
               ways=int(g["ways"]),
               cache_size=int(g["cache_size"]), ln_bot=[int(x) for x in g["ln_bot"]],
               ln_top=[m_spa + nf * (nf - 1) // 2] + [int(x) for x in g["top"]], lr=float(g["lr"]),
               lr_emb=float(g["lr_emb"]), agg_freq=int(g["agg_freq"]), agg_op=str(g["agg_op"]), defer=defer, seed_base=5000)
    off = torch.arange(B).repeat(T, 1)
    batches = [(X, off, [lS_i[k].clone() for k in range(T)], Tt) for X, lS_i, Tt in _batches(g)]
    np.random.seed(int(g["seed"]))
    host = [h.share_memory_() for h in O.init_host_tables(ln_emb, m_spa)]
    got = _run_ranks(2, port, cfg, batches, host)
    for r in range(2):
        np.testing.assert_allclose(got[r]["losses"], g[f"r{r}_losses"], rtol=1e-5)
        for k in range(T):
            assert np.array_equal(got[r]["occ"][k], g[f"occ_{k}"]), (r, k)
            np.testing.assert_allclose(got[r]["wsum"][k], float(g[f"r{r}_weight_sum_{k}"]), rtol=1e-5, atol=1e-4)
        for i in range(len(got[r]["top_w"])):
            np.testing.assert_allclose(got[r]["top_w"][i], g[f"r{r}_top_w{i}"], rtol=1e-4, atol=1e-6)
    for k in range(T):
        np.testing.assert_allclose(float(host[k].double().sum()), float(g[f"host_sum_{k}"]), rtol=1e-6)


def _ragged_oracle_class():
    from oracle import cdlrm_oracle as O

    class BagRangeOracle(O.OracleTrainer):
        """The oracle's trainer with one phase of its step replaced, rank_slice: rank r's slice is the bag range of
        engine.rank_bag_slice (the lookups of samples [r * lbs, min(B, (r + 1) * lbs)), offsets rebased) instead of the
        one-lookup-per-sample cut."""

        def __init__(self, *a, batch_size, **kw):
            super().__init__(*a, **kw)
            self.lbs = math.ceil(batch_size / self.W)

        def rank_slice(self, r, X, lS_o, lS_i, T):
            B = X.shape[0]
            s0, s1 = min(B, r * self.lbs), min(B, (r + 1) * self.lbs)
            Ir, Or = [], []
            for k in range(len(self.ln_emb)):
                a = int(lS_o[k][s0])
                e = int(lS_o[k][s1]) if s1 < B else int(lS_i[k].numel())
                Ir.append(lS_i[k][a:e])
                Or.append(lS_o[k][s0:s1] - a)
            return X[s0:s1], Or, Ir, T[s0:s1], None

    return BagRangeOracle


@pytest.mark.parametrize("world,port,agg_op,defer", [(2, 29883, "mean", True), (3, 29884, "mean", False),
                                                     (3, 29885, "max", True)])
def test_ragged_bags_ranks_vs_oracle(world, port, agg_op, defer):
    """Ragged bags of the reference's random front end at 2 and 3 ranks (mini-batch 29: the last rank's slice is short at 3;
    --data-size 255: the ninth batch is short, 23 samples, cut at the run's local batch like X), a row merge after every
    step (the ranks' ragged touched sets): per-rank losses, tags, cache rows, top MLP, host tables against the oracle with
    the bag-range slice."""
    from cdlrm_amd import dlrm_data_pytorch as DP
    from oracle import cdlrm_oracle as O
    ln_emb, m_spa, B, L, ways, cache_size, seed, aux = [900, 40, 6, 2500], 16, 29, 3, 4, 300, 23, 256
    nf = len(ln_emb) + 1
    ln_bot, ln_top = [5, 32, m_spa], [m_spa + nf * (nf - 1) // 2, 24, 1]
    args = SimpleNamespace(data_size=255, num_batches=0, mini_batch_size=B, num_indices_per_lookup=7,
                           num_indices_per_lookup_fixed=False, round_targets=True, data_generation="random",
                           numpy_rand_seed=seed)
    _, loader = DP.make_random_data_and_loader(args, np.array(ln_emb), 5)
    batches = [(X, lS_o, [x.clone() for x in lS_i], Tt) for X, lS_o, lS_i, Tt in loader]
    assert len({int(x.numel()) for x in batches[0][2]}) > 1, "ragged tables expected"
    assert len(batches) == 9 and batches[-1][0].shape[0] == 23
    np.random.seed(seed)
    torch.manual_seed(seed)
    host = [h.share_memory_() for h in O.init_host_tables(ln_emb, m_spa)]
    torch.set_num_threads(1)
    otr = _ragged_oracle_class()(ln_emb, m_spa, np.array(ln_bot), np.array(ln_top), cache_size=cache_size, num_ways=ways,
                                 mini_batch_size=aux, batch_size=B, world_size=world, lr=0.1, lr_embeds=0.3, lookahead=L,
                                 table_agg_freq=1, table_agg_op=agg_op, seed=seed)
    for j, (X, lS_o, lS_i, Tt) in enumerate(batches):
        if j % L == 0:
            torch.manual_seed(800 + j)
            otr.refill([torch.cat([b[2][k] for b in batches[j:j + L]]) for k in range(len(ln_emb))])
        otr.step(j, X, lS_o, lS_i, Tt)
    cfg = dict(ln_emb=ln_emb, m_spa=m_spa, seed=seed, L=L, lbs=-(-B // world), aux=aux, ways=ways, cache_size=cache_size, ln_bot=ln_bot,
               ln_top=ln_top, lr=0.1, lr_emb=0.3, agg_freq=1, agg_op=agg_op, defer=defer, seed_base=800)
    got = _run_ranks(world, port, cfg, batches, host)
    for r in range(world):
        np.testing.assert_allclose(got[r]["losses"], np.array([l[r] for l in otr.losses]), rtol=1e-5)
        for k in range(len(ln_emb)):
            assert torch.equal(torch.from_numpy(got[r]["occ"][k]), otr.occ[k]), (r, k)
            nrow = got[r]["rows"][k].shape[0]
            np.testing.assert_allclose(got[r]["rows"][k], otr.weights[r][k][:nrow].numpy(), rtol=2e-5, atol=1e-6)
        for i in range(len(got[r]["top_w"])):
            np.testing.assert_allclose(got[r]["top_w"][i], otr.top[r][0][i].numpy(), rtol=1e-4, atol=1e-6)
    for k in range(len(ln_emb)):
        np.testing.assert_allclose(float(host[k].double().sum()), float(otr.host[k].double().sum()), rtol=1e-6)


# ------------------------------------------------------------------------------------------------ CLI

@pytest.mark.parametrize("extra", [["--num-batches=10"], ["--num-batches=10", "--device-rng"], ["--data-size=616"]])
def test_cli_random_multi_hot_world_size_2(extra):
    """python -m cdlrm_amd.main_no_ddp with the reference's default random front end at --world-size=2 (two ranks emulated on
    the one GPU): exits 0 with finite losses.  --device-rng plans the next window while the current one trains (both
    windows' lists on the device at once); --data-size 616 at --mini-batch-size 64 ends on a short batch of 40 samples,
    32 on rank 0 and 8 on rank 1 (X, T and the bags cut at the same rows)."""
    env = dict(os.environ)
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT", "MASTER_ADDR"):
        env.pop(k, None)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    env["CDLRM_BENCH_EMULATE"] = "1"
    flags = ["--arch-sparse-feature-size=16", "--arch-mlp-bot=13-32-16", "--arch-mlp-top=32-1",
             "--arch-embedding-size=3000-50-7-1200", "--mini-batch-size=64", "--lookahead=4", "--cache-size=40",
             "--num-ways=4", "--loss-function=bce", "--round-targets=True", "--learning-rate=0.1", "--lr-embeds=0.3",
             "--print-freq=1", "--numpy-rand-seed=11", "--table-agg-freq=3", "--data-generation=random",
             "--num-indices-per-lookup=6", "--world-size=2"] + extra
    p = subprocess.run([sys.executable, "-m", "cdlrm_amd.main_no_ddp"] + flags, env=env, capture_output=True, text=True,
                       timeout=600, cwd=ROOT)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-3000:])
    losses = [float(x) for x in re.findall(r"Loss = ([0-9.eE+-]+),", p.stdout)]
    assert len(losses) == 9 and all(np.isfinite(losses)) and all(0.0 < x < 10.0 for x in losses), p.stdout[-2000:]
