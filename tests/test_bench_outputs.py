"""`bench.py --dump-outputs DIR`: what the timed path computed in its last step, as .npy files, so that two builds run with the
same arguments can be compared output for output.  CPU part: bench.dump_outputs on a small cache group against a plain
per-lookup walk of the tag table, and the argument checks; GPU part: two c1 runs dump the same bits."""
import json
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NAMES = {"loss", "prediction", "dense_params", "emb_rows", "emb_lookups"}


def _env():
    env = dict(os.environ)
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT", "MASTER_ADDR"):
        env.pop(k, None)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    return env


def _load(d):
    return {n[:-4]: np.load(os.path.join(d, n)) for n in sorted(os.listdir(d))}


# ------------------------------------------------------------------------------------------------ CPU

def test_dump_reads_cached_rows_from_the_cache_and_the_others_from_the_host(tmp_path):
    import bench
    from cdlrm_amd.model_no_ddp import Embedding_Table_Cache_Group
    ln_emb, D, ways, B = [500, 30, 7000], 8, 4, 64
    cg = Embedding_Table_Cache_Group(D, np.array(ln_emb), 40, B, ways, cache_init="zeros")
    g = torch.Generator().manual_seed(1)
    cg.weight.data.copy_(torch.randn(cg.weight.shape, generator=g))
    host = types.SimpleNamespace(emb_l=[types.SimpleNamespace(weight=types.SimpleNamespace(
        data=torch.randn(n, D, generator=g))) for n in ln_emb])
    idx = torch.stack([torch.randint(0, n, (B,), generator=g) for n in ln_emb])
    # about half of the batch's rows cached, each in a way of its own set
    for k, n in enumerate(ln_emb):
        occ = cg.occupancy_tables[k]
        for i in idx[k][::2].tolist():
            s = i % cg.cache_sizes[k]
            free = (occ[s] == -1).nonzero().flatten()
            if i not in occ[s].tolist() and free.numel():
                occ[s, int(free[0])] = i
    loss = torch.tensor([0.5, 40.0, 32.0] + [0.0] * 62)
    Z = torch.randn(B, 1, generator=g)
    eng = types.SimpleNamespace(_buffers=lambda n: {"loss": loss}, prediction=lambda n: Z,
                                param_flat=torch.randn(100, generator=g))
    shapes = bench.dump_outputs(str(tmp_path / "a"), eng, cg, host, idx, seed=7)
    out = _load(tmp_path / "a")
    assert set(out) == NAMES and shapes == {k: list(v.shape) for k, v in out.items()}
    assert all(v.dtype in (np.float32, np.float64) for v in out.values())
    np.testing.assert_array_equal(out["loss"], [0.5, 40.0, 32.0])
    np.testing.assert_array_equal(out["prediction"], Z.numpy().ravel())
    np.testing.assert_array_equal(out["dense_params"], eng.param_flat.numpy())
    lk = out["emb_lookups"]
    assert lk.shape == (len(ln_emb) * B, 3), "a batch below the sample size is dumped whole"
    n_cached = 0
    for (k, i, c), row in zip(lk.astype(np.int64), out["emb_rows"]):
        occ = cg.occupancy_tables[k]
        s = i % cg.cache_sizes[k]
        hit = (occ[s] == i).nonzero().flatten()
        assert c == (hit.numel() == 1)
        if c:
            want = cg.weight.data[cg.row_base[k] + int(hit[0]) * cg.cache_sizes[k] + s]
            n_cached += 1
        else:
            want = host.emb_l[k].weight.data[i]
        np.testing.assert_array_equal(row, want.numpy())
    assert 0 < n_cached < len(lk)
    # the sample is fixed: same arguments, same files
    bench.dump_outputs(str(tmp_path / "b"), eng, cg, host, idx, seed=7)
    again = _load(tmp_path / "b")
    assert all(np.array_equal(out[k], again[k]) for k in NAMES)


def test_dump_samples_a_large_batch_within_the_budget(tmp_path, monkeypatch):
    import bench
    from cdlrm_amd.model_no_ddp import Embedding_Table_Cache_Group
    monkeypatch.setattr(bench, "DUMP_ROWS", 100)
    ln_emb, D, B = [300, 300], 4, 512
    cg = Embedding_Table_Cache_Group(D, np.array(ln_emb), 40, B, 2, cache_init="zeros")
    host = types.SimpleNamespace(emb_l=[types.SimpleNamespace(weight=types.SimpleNamespace(
        data=torch.arange(n * D, dtype=torch.float32).view(n, D))) for n in ln_emb])
    idx = torch.stack([torch.randint(0, n, (B,)) for n in ln_emb])
    eng = types.SimpleNamespace(_buffers=lambda n: {"loss": torch.zeros(65)}, prediction=lambda n: torch.zeros(n, 1),
                                param_flat=torch.zeros(10))
    bench.dump_outputs(str(tmp_path), eng, cg, host, idx, seed=7)
    out = _load(tmp_path)
    lk = out["emb_lookups"].astype(np.int64)
    assert out["emb_rows"].shape == (100, D) and len({(k, i) for k, i, _ in lk}) <= 100
    for (k, i, c), row in zip(lk, out["emb_rows"]):
        assert c == 0 and i in idx[k].tolist()
        np.testing.assert_array_equal(row, host.emb_l[k].weight.data[i].numpy())


@pytest.mark.parametrize("args", [["--steps", "0"], ["--warmup", "-1"]])
def test_bench_refuses_a_run_without_timed_steps(args):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--config", "c1"] + args, env=_env(),
                       capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert p.returncode == 2 and "--steps must be at least 1" in p.stderr, p.stderr[-800:]


def test_plain_run_is_the_default_and_full_is_opt_in(monkeypatch):
    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "20", "--warmup", "5"])
    assert bench.parse().full is False
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "20", "--warmup", "5", "--full"])
    assert bench.parse().full is True


# ------------------------------------------------------------------------------------------------ GPU

@pytest.mark.gpu
def test_two_runs_dump_the_same_outputs(tmp_path):
    """Same arguments, same inputs, same bits -- and the dump is the last TIMED step: its loss is the line's final_loss, the
    line's ms_per_step is that of exactly --steps timed steps."""
    recs = []
    for run in ("a", "b"):
        p = subprocess.run([sys.executable, "bench.py", "--config", "c1", "--steps", "7", "--warmup", "3", "--prewarm-ms", "0",
                            "--no-cpu-baseline", "--dump-outputs", str(tmp_path / run)], env=_env(), capture_output=True,
                           text=True, timeout=600, cwd=ROOT)
        assert p.returncode == 0, p.stderr[-3000:]
        lines = [l for l in p.stdout.splitlines() if l.startswith("{") and '"metric"' in l]
        assert len(lines) == 1, p.stdout[-3000:]
        recs.append(json.loads(lines[0]))
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert set(a) == NAMES and sum(v.nbytes for v in a.values()) <= 64 << 20
    for k in NAMES:
        assert np.array_equal(a[k], b[k]), k
    r = recs[0]
    assert r["steps"] == 7 and r["ms_per_step"] > 0 and abs(r["value"] * r["ms_per_step"] * 1e-3 - 128) < 1e-6 * 128
    assert float(a["loss"][0]) == np.float32(r["config"]["final_loss"])
    assert r["config"]["dump_outputs"] == {k: list(v.shape) for k, v in a.items()}
    assert a["prediction"].shape == (128,) and a["emb_rows"].shape == (8 * 128, 16)
    assert 0 < a["emb_lookups"][:, 2].sum(), "the last step's rows come (partly) from the cache"


@pytest.mark.gpu
def test_full_adds_its_legs_behind_the_same_timed_steps(tmp_path):
    """A plain run stops at the JSON line; --full trains on through a whole window, times the stand-alone gather legs and the CPU
    baseline behind the timed region.  The timed steps are the same: same loss, same dumped outputs to the bit."""
    recs = {}
    for run, extra in (("plain", []), ("full", ["--full"])):
        # (2 + 1 steps end in front of the window's plan launch at iteration 16 of c1's 32: the whole-window leg runs)
        p = subprocess.run([sys.executable, "bench.py", "--config", "c1", "--steps", "2", "--warmup", "1", "--prewarm-ms", "0",
                            "--dump-outputs", str(tmp_path / run)] + extra, env=_env(), capture_output=True, text=True,
                           timeout=600, cwd=ROOT)
        assert p.returncode == 0, p.stderr[-3000:]
        lines = [l for l in p.stdout.splitlines() if l.startswith("{") and '"metric"' in l]
        assert len(lines) == 1, p.stdout[-3000:]
        recs[run] = json.loads(lines[0])
    plain, full = recs["plain"], recs["full"]
    for r in (plain, full):
        assert r["steps"] == 2 and r["warmup"] == 1 and r["ms_per_step"] > 0 and r["unit"] == "samples/s"
        assert r["higher_is_better"] is True and r["dtype"] == "f32"
    assert plain["config"]["final_loss"] == full["config"]["final_loss"]
    a, b = _load(tmp_path / "plain"), _load(tmp_path / "full")
    assert set(a) == NAMES and all(np.array_equal(a[k], b[k]) for k in NAMES)
    assert "cpu_baseline" not in plain and "skipped" in plain["config"]["whole_window"]
    assert plain["roofline"]["alone"] is None and plain["roofline"]["gather_operator"] is None
    assert full["cpu_baseline"]["value"] > 0
    assert full["config"]["whole_window"]["steps"] == 32 and full["config"]["whole_window"]["window_commits"] == 1
    if full["roofline"]["fused_gather"]:
        assert full["roofline"]["alone"] is not None and full["roofline"]["gather_operator"] is not None
