"""Day-file batches cut on the device: the kernel (`ops.dayfile_window`, csrc/dayfile.hip) against the host loader's
`transform_features`, `DeviceDayLoader` against the reference's batches (tests/golden/criteo_loader.npz) and against the
host `DataLoader` while its ring is being reused, and the CLI with `--day-file-loader=device` against the same run with the
host loader (one rank, and two ranks emulated on one GPU).

Bounds.  Indices and targets are integers: equal bit for bit.  X = log(x + 1) is compared with the correctly rounded value
float32(log(float64(float32(x) + float32(1)))): at most 1 ulp away, the bound the host's torch.log keeps itself; host and
device therefore differ by at most 2 ulp."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"


def _ordered(a: np.ndarray) -> np.ndarray:
    """float32 -> integers whose difference is the distance in ulp"""
    i = np.ascontiguousarray(a, dtype=np.float32).view(np.int32).astype(np.int64)
    return np.where(i < 0, -(i & 0x7fffffff), i)


def _ulp(a, b) -> int:
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    assert np.all(np.isfinite(a)) and np.all(np.isfinite(b))
    return int(np.abs(_ordered(a) - _ordered(b)).max()) if a.size else 0


def _log_exact(x_int: np.ndarray) -> np.ndarray:
    return np.log((x_int.astype(np.float32) + np.float32(1)).astype(np.float64)).astype(np.float32)


def _rows(rng, n, nd, nc, dense_hi=500):
    x_int = rng.randint(0, dense_hi, size=(n, nd)).astype(np.int32)
    x_cat = rng.randint(-2 ** 31, 2 ** 31, size=(n, nc), dtype=np.int64).astype(np.int32)
    edge = np.array([2 ** 31 - 1, 2 ** 31 - 2, -2 ** 31, -2 ** 31 + 1, -1, 0, 1], dtype=np.int64).astype(np.int32)
    where = rng.rand(n, nc) < 0.2
    x_cat[where] = edge[rng.randint(0, len(edge), size=int(where.sum()))]
    y = rng.randint(0, 2, size=n).astype(np.int32)
    return x_int, x_cat, y


def _dev_rows(arrs, offset):
    """the three arrays on the device, each `offset` dwords behind a 16-byte aligned base"""
    out = []
    for a in arrs:
        buf = torch.empty(a.size + 8, dtype=torch.int32, device=DEV)
        assert buf.data_ptr() % 16 == 0
        v = buf[offset:offset + a.size].view(a.shape)
        v.copy_(torch.from_numpy(a))
        out.append(v)
    return out


@pytest.mark.parametrize("nd,nc", [(13, 26), (5, 7), (1, 1), (3, 60)])
@pytest.mark.parametrize("offset", [0, 1, 3])
def test_dayfile_window_kernel_matches_the_host_transform(nd, nc, offset):
    from cdlrm_amd import ops
    from cdlrm_amd.data_loader_terabyte import transform_features
    tile = ops.dayfile_tile()
    rng = np.random.RandomState(1000 * nd + 10 * nc + offset)
    sizes = [1, tile - 1, tile, tile + 1, 5 * tile + 77] + ([200003] if (nd, nc) == (13, 26) else [])
    SENT_I, SENT_F = -0x0123456789abcdef, -12345.5
    for n in sizes:
        for mir in (-1, 0, 7, 40000, 2 ** 31 - 1):
            arrs = _rows(rng, n, nd, nc)
            col0 = 0 if mir in (-1, 40000) else 3 * tile + 5          # also: a segment that starts off every alignment
            rows = col0 + n + 9
            X = torch.full((rows, nd), SENT_F, dtype=torch.float32, device=DEV)
            I = torch.full((nc, rows), SENT_I, dtype=torch.int64, device=DEV)
            T = torch.full((rows, 1), SENT_F, dtype=torch.float32, device=DEV)
            xi, xc, y = _dev_rows(arrs, offset)
            ops.dayfile_window(xi, xc, y, mir, X, I, T, col0=col0)
            torch.cuda.synchronize()
            hX, _, hI, hT = transform_features(*arrs, mir)
            X, I, T = X.cpu(), I.cpu(), T.cpu()
            tag = (nd, nc, offset, n, mir)
            assert torch.equal(I[:, col0:col0 + n], hI), tag
            assert torch.equal(T[col0:col0 + n], hT), tag
            if mir > 0:
                assert int(I[:, col0:col0 + n].min()) >= 0 and int(I[:, col0:col0 + n].max()) < mir
            exact = _log_exact(arrs[0])
            assert _ulp(X[col0:col0 + n].numpy(), exact) <= 1, tag
            assert _ulp(X[col0:col0 + n].numpy(), hX.numpy()) <= 2, tag
            # nothing outside the segment's samples is written
            assert bool((I[:, :col0] == SENT_I).all()) and bool((I[:, col0 + n:] == SENT_I).all()), tag
            assert bool((X[:col0] == SENT_F).all()) and bool((X[col0 + n:] == SENT_F).all()), tag
            assert bool((T[:col0] == SENT_F).all()) and bool((T[col0 + n:] == SENT_F).all()), tag


def test_dayfile_window_writes_into_a_column_range_of_a_wider_rectangle():
    """several segments of one window, one launch each, through views of the window's buffers"""
    from cdlrm_amd import ops
    from cdlrm_amd.data_loader_terabyte import transform_features
    rng = np.random.RandomState(5)
    segs = [_rows(rng, n, 13, 26) for n in (300, 1, 511)]
    W = sum(s[2].shape[0] for s in segs)
    X = torch.zeros(W, 13, device=DEV)
    I = torch.zeros(26, W, dtype=torch.int64, device=DEV)
    T = torch.zeros(W, 1, device=DEV)
    col = 0
    for s in segs:
        ops.dayfile_window(*_dev_rows(s, 0), 1000, X, I, T, col0=col)
        col += s[2].shape[0]
    torch.cuda.synchronize()
    hX, _, hI, hT = transform_features(*(np.concatenate([s[i] for s in segs]) for i in range(3)), 1000)
    assert torch.equal(I.cpu(), hI) and torch.equal(T.cpu(), hT) and _ulp(X.cpu().numpy(), hX.numpy()) <= 2
    with pytest.raises(AssertionError):         # a segment that does not fit its window is refused before any launch
        ops.dayfile_window(*_dev_rows(segs[0], 0), 1000, X, I, T, col0=W - 299)


def test_dayfile_window_log_is_within_one_ulp_of_the_correctly_rounded_value():
    from cdlrm_amd import ops
    rng = np.random.RandomState(9)
    dense = np.concatenate([np.arange(0, 2 * 10 ** 6 + 1, dtype=np.int64),
                            rng.randint(0, 2 ** 31, size=2 * 10 ** 6 - 1, dtype=np.int64),
                            np.array([2 ** 31 - 1, 2 ** 24, 2 ** 24 + 1, 2 ** 24 - 1], dtype=np.int64)]).astype(np.int32)
    assert dense.size % 4 == 0
    x_int = dense.reshape(-1, 4)
    n = x_int.shape[0]
    xi, xc, y = _dev_rows((x_int, np.zeros((n, 2), np.int32), np.zeros(n, np.int32)), 0)
    X = torch.empty(n, 4, device=DEV)
    ops.dayfile_window(xi, xc, y, -1, X, torch.empty(2, n, dtype=torch.int64, device=DEV), torch.empty(n, 1, device=DEV))
    got = X.cpu().numpy()
    host = torch.log(torch.as_tensor(x_int, dtype=torch.float) + 1).numpy()
    exact = _log_exact(x_int)
    d_dev, d_host, d_both = _ulp(got, exact), _ulp(host, exact), _ulp(got, host)
    print("log(x + 1) over %d values: device %d ulp, host %d ulp from the correctly rounded value; device - host %d ulp"
          % (dense.size, d_dev, d_host, d_both))
    assert d_dev <= 1
    assert d_both <= 2


# ------------------------------------------------------------------------------------------------ the loader

def _write_days(d, arrays, name="day"):
    for day, (xi, xc, y) in enumerate(arrays):
        np.savez(os.path.join(d, "%s_%d_reordered.npz" % (name, day)), X_int=xi, X_cat=xc, y=y)
    np.savez(os.path.join(d, "%s_day_count.npz" % name), total_per_file=np.array([a[2].shape[0] for a in arrays]))


@pytest.mark.parametrize("name,days,split,drop", [("train", [0, 1, 2], "train", False),
                                                  ("train_drop", [0, 1, 2], "train", True), ("val", [2], "val", False),
                                                  ("test", [1, 2], "test", False)])
def test_device_day_loader_matches_reference(golden, tmp_path, name, days, split, drop):
    from cdlrm_amd.data_loader_terabyte import DeviceDayLoader, batch_segments
    g = golden("criteo_loader")
    arrays = [(g["xi_%d" % d], g["xc_%d" % d], g["y_%d" % d]) for d in range(len(g["sizes"]))]
    _write_days(str(tmp_path), arrays)
    B, mir, nb = int(g["B"]), int(g["max_ind_range"]), int(g[name + "_nb"])
    segs = batch_segments([int(n) for n in g["sizes"]], days, B, split, drop)
    exact = _log_exact(np.concatenate([arrays[d][0][a:b] for s in segs for d, a, b in s]))
    for window in (1, 2, nb + 1):
        ld = DeviceDayLoader("day", str(tmp_path), days, B, max_ind_range=mir, split=split, drop_last_batch=drop, device=DEV,
                             window=window)
        assert len(ld) == int(g[name + "_len"])
        for epoch in range(2):
            # (every batch is copied as it is handed out: the loader reuses a window's buffers two windows later)
            batches = [tuple(t.clone() for t in b) for b in ld]
            torch.cuda.synchronize()
            assert len(batches) == nb
            assert [b[3].shape[0] for b in batches] == g[name + "_sizes"].tolist()
            assert torch.equal(torch.cat([b[2] for b in batches], dim=1).cpu(), torch.from_numpy(g[name + "_lS_i"]))
            assert torch.equal(torch.cat([b[3] for b in batches]).cpu(), torch.from_numpy(g[name + "_T"]))
            assert torch.equal(batches[-1][1].cpu(), torch.from_numpy(g[name + "_lS_o_last"]))
            X = torch.cat([b[0] for b in batches]).cpu().numpy()
            assert _ulp(X, exact) <= 1 and _ulp(X, g[name + "_X"]) <= 2, (window, epoch)
            X0, lS_o, lS_i, T = batches[0]
            assert X0.dtype == torch.float32 and lS_i.dtype == torch.int64 and lS_o.dtype == torch.int64 and T.shape[1] == 1
            assert all(t.is_cuda for t in batches[0])
        first = next(iter(ld))
        assert first.win_pos == 0 and first.window_rect.shape == (26, sum(g[name + "_sizes"].tolist()[:window]))
        assert first[2].data_ptr() == first.window_rect.data_ptr() and first[2].stride(1) == 1      # a view: no copy


def test_device_day_loader_ring_is_safe_under_a_slow_consumer(tmp_path):
    """Many short windows; the consumer is SLOW (a spin kernel in front of every read, on the stream the batches are handed out
    on) and every yielded batch of the two most recent windows is held as the view it is.  The reads of window u are still
    queued when the loader recycles the slot of window u - 2 and uploads ahead: only the ring rule (three slots, the copy stream
    behind an event on the consumer's stream) keeps them right."""
    from cdlrm_amd.data_loader_terabyte import DataLoader, DeviceDayLoader
    rng = np.random.RandomState(17)
    arrays = [_rows(rng, n, 13, 26) for n in (331, 257, 129)]
    _write_days(str(tmp_path), arrays)
    B, L = 8, 2
    want = list(DataLoader("day", str(tmp_path), [0, 1, 2], B, max_ind_range=5000))
    ld = DeviceDayLoader("day", str(tmp_path), [0, 1, 2], B, max_ind_range=5000, device=DEV, window=L)
    assert len(want) == len(ld) == len(ld.batches) and len(want) >= 80
    for epoch in range(2):
        read, held = [], []
        for j, b in enumerate(ld):
            if b.win_pos == 0:
                held = held[-L:]            # the previous window stays, the one before it goes
            held.append((j, b))
            torch.cuda._sleep(400000)       # the consumer lags behind the hand-out
            read.append((b[0].clone(), b[2].clone(), b[3].clone()))
        torch.cuda.synchronize()
        assert len(read) == len(want)
        for j, (X, I, T) in enumerate(read):
            assert torch.equal(I.cpu(), want[j][2]) and torch.equal(T.cpu(), want[j][3]), (epoch, j)
            assert _ulp(X.cpu().numpy(), want[j][0].numpy()) <= 2
        assert len(held) >= L + 1
        for j, b in held:                   # the two most recent windows, as the views that were handed out
            assert torch.equal(b[2].cpu(), want[j][2]) and torch.equal(b[3].cpu(), want[j][3]), (epoch, j)
            assert torch.equal(b[1].cpu(), want[j][1])


# ------------------------------------------------------------------------------------------------ training

FLAGS = ["--arch-sparse-feature-size=16", "--arch-mlp-bot=13-32-16", "--arch-mlp-top=32-1", "--mini-batch-size=64",
         "--lookahead=4", "--cache-size=40", "--num-ways=4", "--loss-function=bce", "--round-targets=True",
         "--learning-rate=0.1", "--lr-embeds=0.3", "--print-freq=1", "--numpy-rand-seed=11", "--table-agg-freq=5",
         "--data-generation=dataset"]


def _cli_day_files(d, sizes):
    rng = np.random.RandomState(3)
    counts = np.array([900, 40, 7, 300, 1500])
    for day, n in enumerate(sizes):
        np.savez(os.path.join(d, "day_%d_reordered.npz" % day), X_int=rng.randint(0, 500, size=(n, 13)).astype(np.int32),
                 X_cat=np.stack([rng.randint(0, c, size=n) for c in counts], axis=1).astype(np.int32),
                 y=rng.randint(0, 2, size=n).astype(np.int32))
    np.savez(os.path.join(d, "day_day_count.npz"), total_per_file=np.array(sizes))
    np.savez(os.path.join(d, "day_fea_count.npz"), counts=counts)


def _compare_runs(outs, tags, n_steps, world):
    losses = {k: [float(x) for x in re.findall(r"Loss = ([0-9.eE+-]+),", o)] for k, o in outs.items()}
    assert len(losses["host"]) == len(losses["device"]) == n_steps - 1, outs["device"][-2000:]
    rel = np.abs(np.array(losses["device"]) - np.array(losses["host"])) / np.abs(np.array(losses["host"]))
    print("world %d: largest relative loss deviation device vs host loader: %.3g" % (world, rel.max()))
    assert rel.max() <= 1e-5
    acc = {k: re.findall(r"Test accuracy = .*", o) for k, o in outs.items()}
    assert len(acc["host"]) >= 1 and acc["host"] == acc["device"]
    assert "Day-file loader: device" in outs["device"] and "Day-file loader" not in outs["host"]
    for r in range(world):
        th, td = torch.load(tags["host"] + ".rank%d" % r), torch.load(tags["device"] + ".rank%d" % r)
        assert th.dtype == torch.int64 and int((th >= 0).sum()) > 0
        assert torch.equal(th, td), "cache tags differ on rank %d" % r


@pytest.fixture()
def keep_current_stream():
    """`main_no_ddp.Run` makes a stream of its own the thread's current one (as the CLI process should); tests that run after
    this module in the same process expect the stream they started on."""
    before = torch.cuda.current_stream()
    yield
    torch.cuda.synchronize()
    torch.cuda.set_stream(before)


@pytest.mark.parametrize("extra", [["--device-rng"], []], ids=["lookahead-plan", "plan-at-boundary"])
def test_cli_device_loader_trains_like_the_host_loader(tmp_path, capsys, monkeypatch, keep_current_stream, extra):
    """The shapes of test_main_cli_criteo_day_files: three windows (4 + 4 + 1 batches), batch 5 runs across the file boundary
    inside the second window, the short last batch is dropped as the CLI does."""
    from cdlrm_amd import main_no_ddp
    sizes = [64 * 5 + 9, 64 * 4 + 30, 64 * 2]
    _cli_day_files(str(tmp_path), sizes)
    outs, tags = {}, {}
    for mode in ("host", "device"):
        tags[mode] = os.path.join(tmp_path, "tags_" + mode)
        monkeypatch.setenv("CDLRM_DUMP_TAGS", tags[mode])
        main_no_ddp.main(FLAGS + extra + ["--world-size=1", "--raw-data-file=" + os.path.join(tmp_path, "day"),
                                          "--day-file-loader=" + mode])
        outs[mode] = capsys.readouterr().out
    _compare_runs(outs, tags, (sizes[0] + sizes[1]) // 64, 1)


def test_cli_device_loader_world_size_2(tmp_path):
    """Two ranks emulated on one GPU (CDLRM_BENCH_EMULATE=1, as tests/test_self_launch.py): every rank runs its own loader
    over the same files, uploads whole windows and trains its column slice."""
    sizes = [64 * 9 + 9, 64 * 8 + 30, 64 * 2]
    _cli_day_files(str(tmp_path), sizes)
    env = dict(os.environ)
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT", "MASTER_ADDR", "GROUP_RANK", "LOCAL_WORLD_SIZE",
              "TORCHELASTIC_RUN_ID"):
        env.pop(k, None)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    env["CDLRM_BENCH_EMULATE"] = "1"
    outs, tags = {}, {}
    for mode in ("host", "device"):
        tags[mode] = os.path.join(tmp_path, "tags_" + mode)
        env["CDLRM_DUMP_TAGS"] = tags[mode]
        p = subprocess.run([sys.executable, "-m", "cdlrm_amd.main_no_ddp"] + FLAGS +
                           ["--world-size=2", "--table-agg-freq=3", "--test-freq=6", "--device-rng",
                            "--raw-data-file=" + os.path.join(tmp_path, "day"), "--day-file-loader=" + mode],
                           env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
        assert p.returncode == 0, p.stderr[-3000:]
        outs[mode] = p.stdout
    _compare_runs(outs, tags, (sizes[0] + sizes[1]) // 64, 2)
