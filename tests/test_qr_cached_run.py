"""Quotient-remainder tables through the embedding cache as a user drives them on the MI355X: main_no_ddp.Run
and main() with --qr-flag, --save-model / --load-model, the "fill" insert policy on the q window, and two ranks emulated on one
GPU -- against the restated trainer (tests/qr_cached_restated.py) and the restated fill policy."""
import os
import re
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import qr_cached_restated as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

LN_EMB = [3000, 50, 7, 1200, 40000]             # the c1-sized tables tests/test_run_cli.py uses; 3 of them above the threshold
FLAGS = ["--arch-sparse-feature-size=16", "--arch-mlp-bot=13-32-16", "--arch-mlp-top=32-1",
         "--arch-embedding-size=3000-50-7-1200-40000", "--mini-batch-size=64", "--lookahead=4", "--cache-size=40",
         "--num-ways=4", "--loss-function=bce", "--round-targets=True", "--learning-rate=0.1", "--lr-embeds=0.3",
         "--print-freq=1", "--world-size=1", "--numpy-rand-seed=11", "--table-agg-freq=5",
         "--qr-flag", "--qr-collisions=4", "--qr-threshold=200", "--data-generation=dataset"]


class _Loader(list):
    pass


def _loader(nb, seed, B=64):
    lS_o = torch.arange(B).repeat(len(LN_EMB), 1)
    return [(X, lS_o, idx, T) for X, idx, T in R.criteo_batches(LN_EMB, 13, B, nb, seed)]


def _host_group(op, host, wr):
    from cdlrm_amd.model_no_ddp import Embedding_Table_Group
    eg = Embedding_Table_Group(16, np.array(LN_EMB), qr_flag=True, qr_operation=op, qr_collisions=4, qr_threshold=200)
    for k, E in enumerate(eg.emb_l):
        if wr[k] is None:
            E.weight.data = host[k].clone()
        else:
            E.weight_q.data, E.weight_r.data = host[k].clone(), wr[k].clone()
    return eg.pin()


def _restated(op, batches, host, wr, L=4, seed=11):
    ln_top = np.array([16 + 6 * 5 // 2, 32, 1])
    tr = R.QRCachedTrainer(LN_EMB, 16, [13, 32, 16], ln_top, qr_collisions=4, qr_threshold=200, qr_operation=op,
                           host_tables=[h.clone() for h in host], weight_r=wr, cache_size=40, num_ways=4, mini_batch_size=64,
                           lr=0.1, lr_embeds=0.3, lookahead=L, table_agg_freq=5, seed=seed)
    return tr, ln_top


@pytest.mark.parametrize("op", ["mult", "add"])
def test_run_matches_the_restated_trainer(capsys, op):
    """Run on a list loader, 14 batches (three windows and a short last one), with the rank-0 test loop: the printed losses and
    test accuracies are the restated trainer's, the tags bit-exact, quotient tables and Wr within the row tolerance."""
    from cdlrm_amd.main_no_ddp import ProcessArgs, Run
    L, nb = 4, 14
    host, wr = R.init_tables(LN_EMB, 16, 4, 200, 11)
    batches, test_batches = _Loader(_loader(nb, 5)), _loader(3, 77)
    tr, ln_top = _restated(op, batches, host, wr)
    torch.set_num_threads(1)
    want_acc = []
    for j, (X, lS_o, idx, T) in enumerate(batches):
        if j % L == 0:
            tr.refill(torch.cat([b[2] for b in batches[j:j + L]], dim=1))
        tr.step(j, X, lS_o, idx, T)
        if (j > 0 and j % 5 == 0) or j == nb - 1:
            Zs = [tr.evaluate(Xt, lS_ot, idxt) for Xt, lS_ot, idxt, _ in test_batches]
            ok = sum(int((torch.round(Z) == b[3]).sum()) for Z, b in zip(Zs, test_batches))
            want_acc.append(100 * ok / (3 * 64))
            assert min(float((Z - 0.5).abs().min()) for Z in Zs) > 2e-5         # (no score the GPU could round the other way)
    eg = _host_group(op, host, wr)
    capsys.readouterr()
    eng = Run(0, 16, np.array(LN_EMB), np.array([13, 32, 16]), ln_top, batches, test_batches, None, None, None, eg,
              ProcessArgs(FLAGS + ["--test-freq=5", "--qr-operation=" + op]))
    printed = capsys.readouterr().out
    got = [float(x) for x in re.findall(r"Loss = ([0-9.eE+-]+),", printed)]
    want = np.array([l[0] for l in tr.losses])
    assert len(got) == nb - 1
    np.testing.assert_allclose(np.array(got), np.concatenate([[(want[0] + want[1]) / 2], want[2:]]), rtol=1e-5)
    got_acc = [float(x) for x in re.findall(r"Test accuracy = ([0-9.eE+-]+)%", printed)]
    np.testing.assert_allclose(got_acc, want_acc, rtol=0, atol=1e-9)
    eng.cg.ctx.check()
    assert eng.qr is not None and not eng._fused_gather(None)
    for k in range(len(LN_EMB)):
        assert torch.equal(eng.cg.occupancy_tables[k].cpu(), tr.occ[k]), k
        hw = eg.emb_l[k].weight_q if tr.coll[k] else eg.emb_l[k].weight
        np.testing.assert_allclose(hw.data.numpy(), tr.host[k].numpy(), rtol=2e-5, atol=1e-6)
        if tr.coll[k]:
            np.testing.assert_allclose(eng.Wr[k].cpu().numpy(), tr.Wr[0][k].numpy(), rtol=2e-5, atol=1e-6)


def test_save_model_then_load_model_restores_wr_and_the_quotient_tables(tmp_path):
    from cdlrm_amd.main_no_ddp import ProcessArgs, Run
    host, wr = R.init_tables(LN_EMB, 16, 4, 200, 11)
    ln_top = np.array([16 + 6 * 5 // 2, 32, 1])
    path = str(tmp_path / "model.pt")
    eg = _host_group("mult", host, wr)
    eng = Run(0, 16, np.array(LN_EMB), np.array([13, 32, 16]), ln_top, _Loader(_loader(8, 5)), None, None, None, None, eg,
              ProcessArgs(FLAGS + ["--save-model=" + path]))
    saved = torch.load(path)
    coll = R.collisions_of(LN_EMB, 4, 200)
    for k, E in enumerate(eg.emb_l):
        if coll[k]:
            assert torch.equal(saved["emb_r"][k], eng.Wr[k].cpu()) and torch.equal(E.weight_r.data, eng.Wr[k].cpu())
            assert not torch.equal(saved["emb_r"][k], wr[k])                                    # it was trained
            assert torch.equal(saved["emb"][k], E.weight_q.data) and not torch.equal(saved["emb"][k], host[k])
        else:
            assert saved["emb_r"][k] is None and torch.equal(saved["emb"][k], E.weight.data)
    # a fresh run over zeroed tables that loads the file and trains nothing
    eg2 = _host_group("mult", [torch.zeros_like(h) for h in host], [None if w is None else torch.zeros_like(w) for w in wr])
    eng2 = Run(0, 16, np.array(LN_EMB), np.array([13, 32, 16]), ln_top, _Loader([]), None, None, None, None, eg2,
               ProcessArgs(FLAGS + ["--load-model=" + path]))
    for k, E in enumerate(eg2.emb_l):
        if coll[k]:
            assert torch.equal(eng2.Wr[k].cpu(), saved["emb_r"][k]) and torch.equal(E.weight_q.data, saved["emb"][k])
        else:
            assert torch.equal(E.weight.data, saved["emb"][k]) and not eng2.Wr[k].any()


def test_main_cli_day_files_with_qr_flag(tmp_path, capsys):
    """The CLI over the day-file fixture of tests/test_run_cli.py with --qr-flag: it runs to its last line with the host and
    with the device loader, the two print the same losses, and those are the restated trainer's on the same day-file batches
    and the tables main() builds from its seed (plain tables from numpy's generator, QR tables from torch's)."""
    from cdlrm_amd import main_no_ddp
    rng = np.random.RandomState(3)
    counts = np.array([900, 40, 7, 300, 1500])
    sizes = [64 * 5 + 9, 64 * 4 + 30, 64 * 2]
    for day, n in enumerate(sizes):
        np.savez(os.path.join(tmp_path, "day_%d_reordered.npz" % day), X_int=rng.randint(0, 500, size=(n, 13)).astype(np.int32),
                 X_cat=np.stack([rng.randint(0, c, size=n) for c in counts], axis=1).astype(np.int32),
                 y=rng.randint(0, 2, size=n).astype(np.int32))
    np.savez(os.path.join(tmp_path, "day_day_count.npz"), total_per_file=np.array(sizes))
    np.savez(os.path.join(tmp_path, "day_fea_count.npz"), counts=counts)
    flags = [f for f in FLAGS if not f.startswith("--arch-embedding-size")]
    n_train = (sizes[0] + sizes[1]) // 64
    losses = {}
    for loader in ("host", "device"):
        capsys.readouterr()
        main_no_ddp.main(flags + ["--data-generation=dataset", "--raw-data-file=" + os.path.join(tmp_path, "day"),
                                  "--day-file-loader=" + loader])
        out = capsys.readouterr().out
        assert "Quotient-remainder tables: 3 of 5 (c = 4, mult)" in out
        assert out.count("Epoch 0: Finished") == n_train - 1
        assert out.count("Testing at") == 1 and "Test AUC = " in out
        losses[loader] = re.findall(r"Loss = ([0-9.eE+-]+),", out)
        assert all(np.isfinite(float(x)) for x in losses[loader])
    assert losses["host"] == losses["device"]
    # the restated trainer over the host loader's batches (the loader is not what is under test here)
    from cdlrm_amd.data_loader_terabyte import DataLoader
    ln = [int(c) for c in counts]
    host, wr = R.init_tables(ln, 16, 4, 200, 11)
    assert sum(w is not None for w in wr) == 3
    ln_top = np.array([16 + 6 * 5 // 2, 32, 1])
    tr = R.QRCachedTrainer(ln, 16, [13, 32, 16], ln_top, qr_collisions=4, qr_threshold=200, qr_operation="mult",
                           host_tables=host, weight_r=wr, cache_size=40, num_ways=4, mini_batch_size=64, lr=0.1, lr_embeds=0.3,
                           lookahead=4, table_agg_freq=5, seed=11)
    batches = [(X.clone().float(), torch.as_tensor(I).clone().long(), T.clone().float().view(-1, 1))
               for X, _, I, T in DataLoader("day", str(tmp_path), [0, 1], 64, -1, "train", True)]
    assert len(batches) == n_train
    lS_o = torch.arange(64).repeat(len(ln), 1)
    torch.set_num_threads(1)
    for j, (X, idx, T) in enumerate(batches):
        if j % 4 == 0:
            tr.refill(torch.cat([b[1] for b in batches[j:j + 4]], dim=1))
        tr.step(j, X, lS_o, idx, T)
    want = np.array([l[0] for l in tr.losses])
    np.testing.assert_allclose(np.array([float(x) for x in losses["host"]]),
                               np.concatenate([[(want[0] + want[1]) / 2], want[2:]]), rtol=1e-5)


@pytest.mark.parametrize("extra", [[], ["--device-rng"], ["--device-rng", "--qr-operation=add", "--qr-collisions=16"]])
def test_main_cli_synthetic_with_qr_flag(capsys, extra):
    """The CLI on the synthetic Criteo-layout generator (one index per bag) with --qr-flag: the parity plan at the window
    boundary, and --device-rng (the next window is split and planned while this one trains)."""
    from cdlrm_amd import main_no_ddp
    flags = [f for f in FLAGS if not f.startswith("--data-generation")]
    main_no_ddp.main(flags + ["--data-generation=criteo-synthetic", "--num-batches=21"] + extra)
    out = capsys.readouterr().out
    assert "Quotient-remainder tables: 3 of 5" in out
    assert len([l for l in out.splitlines() if l.startswith("Epoch 0: Finished")]) == 20
    losses = [float(x) for x in re.findall(r"Loss = ([0-9.eE+-]+),", out)]
    # (finite and inside BCE's range -- its log is clamped at -100; `add` of two U(sqrt(1/n), 1) tables saturates the sigmoid)
    assert len(losses) == 20 and all(np.isfinite(losses)) and 0.0 < min(losses) and max(losses) <= 100.0


def test_fill_policy_tags_equal_the_restatement_on_the_q_window():
    """insert_policy="fill" in quotient-remainder mode: after every commit the tags are the restated policy's over the q windows
    and tables of rows_q rows."""
    import fill_policy_restated as F
    from test_qr_cached import CFG, build_engine
    cfg = dict(CFG, L=8, nbatch=24, cache=100)        # 404 slots for 2500 quotient rows: the windows evict
    host0, wr0 = R.init_tables(cfg["ln_emb"], cfg["m_spa"], cfg["c"], cfg["thr"], cfg["seed"])
    batches = R.criteo_batches(cfg["ln_emb"], 13, cfg["B"], cfg["nbatch"], cfg["seed"] + 1)
    host, cg, dl, eng, pipe = build_engine(cfg, "mult", host0, wr0, insert_policy="fill")
    coll = R.collisions_of(cfg["ln_emb"], cfg["c"], cfg["thr"])
    rows_q = R.rows_q_of(cfg["ln_emb"], coll)
    snaps, wins = [], []
    for j in range(0, cfg["nbatch"], cfg["L"]):
        raw = torch.cat([b[1] for b in batches[j:j + cfg["L"]]], dim=1)
        wins.append(R.split_tables(raw, cfg["ln_emb"], coll)[0].numpy())
        win = raw.to(DEV)
        eng.qr_split(win, q=win)
        pipe.plan_window(win)
        pipe.commit()
        pipe.wait_writeback()
        torch.cuda.synchronize()
        snaps.append([o.cpu().numpy().copy() for o in cg.occupancy_tables])
    cg.ctx.check()
    tags = [np.full((P, cfg["ways"]), -1, dtype=np.int64) for P in cg.cache_sizes]
    want = F.run_windows(tags, wins, ln_emb=rows_q)
    for w in range(len(wins)):
        for k in range(len(rows_q)):
            assert np.array_equal(snaps[w][k], want[w][k]["tags"]), (w, k)
    assert sum(int((r["evicted"] != -1).sum()) for per in want for r in per) > 0


# ---- two ranks emulated on one GPU (gloo), as tests/test_multirank_gpu.py does it -----------------------------------------

RANKS_CFG = dict(ln_emb=[10_000] * 3 + [150], m_spa=16, B=64, L=8, ways=4, cache=600, c=4, thr=200, seed=41, nbatch=17,
                 ln_bot=[13, 32, 16], top=[32, 1], lr=0.1, lr_emb=0.3)


def _rank_worker(rank, world, port, op, agg_op, ret):
    import faulthandler
    faulthandler.dump_traceback_later(150, exit=True)        # a stuck worker says where, instead of a silent time-out
    try:
        sys.path.insert(0, ROOT)
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import torch.distributed as dist
        from test_qr_cached import build_engine
        os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
        dist.init_process_group("gloo", rank=rank, world_size=world)
        torch.cuda.set_device(0)
        cfg = RANKS_CFG
        host0, wr0 = R.init_tables(cfg["ln_emb"], cfg["m_spa"], cfg["c"], cfg["thr"], cfg["seed"])
        batches = R.criteo_batches(cfg["ln_emb"], 13, cfg["B"], cfg["nbatch"], cfg["seed"] + 1)
        # every rank keeps a private copy of the host tables and applies every eviction to it (hostmem.py "replicas")
        host, cg, dl, eng, pipe = build_engine(cfg, op, host0, wr0, world=world, rank=rank, agg_freq=4, agg_op=agg_op,
                                               replicated=True)
        assert pipe.replicated_host
        L, B = cfg["L"], cfg["B"]
        lbs = -(-B // world)
        losses, wr_after_agg = [], None
        for j, (X, idx, T) in enumerate(batches):
            if j % L == 0:
                eng.sync_touched_to_rank0()
                win = torch.cat([b[1] for b in batches[j:j + L]], dim=1).to(DEV)
                _, rwin = eng.qr_split(win, q=win)
                torch.manual_seed(5000 + j)
                pipe.plan_window(win)
                pipe.commit()
                pipe.wait_writeback()
            sl = slice(rank * lbs, (rank + 1) * lbs)
            lo = (j % L) * B + rank * lbs
            nxt = win[:, lo + B:lo + B + lbs] if (j + 1 < len(batches) and (j + 1) % L != 0) else None
            loss = eng.step(X[sl].to(DEV), win[:, lo:lo + lbs], T[sl].to(DEV), j=j, next_idx=nxt, r=rwin[:, lo:lo + lbs])
            losses.append(float(loss[0]))
            if j > 0 and j % 4 == 0:
                eng.finish()
                wr_after_agg = eng.Wr.cpu().numpy().copy()
        eng.finish()
        cg.ctx.check()
        nrow = [cfg["ways"] * p for p in cg.cache_sizes]
        ret.put((rank, dict(losses=np.array(losses), occ=[o.cpu().numpy() for o in cg.occupancy_tables],
                            rows=[cg.emb_l[k].weight[:nrow[k]].cpu().numpy() for k in range(len(nrow))],
                            host=[(E.weight_q if hasattr(E, "weight_q") else E.weight).data.numpy().copy() for E in host.emb_l],
                            Wr=eng.Wr.cpu().numpy(), wr_after_agg=wr_after_agg)))
        dist.barrier()
        dist.destroy_process_group()
    except BaseException:      # a dead worker must fail the test, not hang it
        import traceback
        ret.put((rank, {"error": traceback.format_exc()}))
        raise


@pytest.mark.parametrize("agg_op,port", [("mean", 29861), ("max", 29862)])
def test_two_ranks_one_gpu_match_the_restated_trainer(agg_op, port):
    """world_size = 2, table_agg_freq = 4, 17 steps (the last one aggregates): per-rank losses, shared tags, cache rows, quotient
    host tables and Wr against the restated trainer; Wr equal on both ranks right after an aggregation."""
    from test_qr_cached import restated_run
    cfg = RANKS_CFG
    tr, _, _, _, _ = restated_run(cfg, "mult", world=2, agg_freq=4, agg_op=agg_op)
    ctx = mp.get_context("spawn")
    ret = ctx.Queue()
    procs = [ctx.Process(target=_rank_worker, args=(r, 2, port, "mult", agg_op, ret)) for r in range(2)]
    for p in procs:
        p.start()
    got = {}
    for _ in range(2):
        r, payload = ret.get(timeout=300)
        assert "error" not in payload, payload["error"]
        got[r] = payload
    for p in procs:
        p.join(timeout=60)
    coll = R.collisions_of(cfg["ln_emb"], cfg["c"], cfg["thr"])
    for r in range(2):
        np.testing.assert_allclose(got[r]["losses"], np.array([l[r] for l in tr.losses]), rtol=1e-5)
        for k in range(len(coll)):
            assert np.array_equal(got[r]["occ"][k], tr.occ[k].numpy()), (r, k)
            n = got[r]["rows"][k].shape[0]
            np.testing.assert_allclose(got[r]["rows"][k], tr.weights[r][k][:n].numpy(), rtol=2e-5, atol=1e-6)
            np.testing.assert_allclose(got[r]["host"][k], tr.host[k].numpy(), rtol=2e-5, atol=1e-6)
            if coll[k]:
                np.testing.assert_allclose(got[r]["Wr"][k], tr.Wr[r][k].numpy(), rtol=2e-5, atol=1e-6)
    assert got[0]["wr_after_agg"] is not None and np.array_equal(got[0]["wr_after_agg"], got[1]["wr_after_agg"])
    assert np.array_equal(got[0]["Wr"], got[1]["Wr"])           # the last step aggregated
