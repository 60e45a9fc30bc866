"""MLPerf binary Criteo records cut on the device: the kernel (`ops.binfile_window`, csrc/binfile.hip) against the host
loader's `transform_features` and, bit for bit, against the day-file kernel on the same samples; `DeviceBinLoader` against the
reference's batches (tests/golden/criteo_bin.npz) and against the host `BinLoader` while its ring is being reused; the CLI
with `--mlperf-bin-loader` on the host and on the device loader (one rank, two ranks emulated on one GPU) and against the
day-file run over the same samples.

Bounds (tests/test_dayfile_device.py).  Indices and targets are integers: equal bit for bit.  X = log(x + 1) is compared
with the correctly rounded value float32(log(float64(float32(x) + float32(1)))): at most 1 ulp away, the bound the host's
torch.log keeps itself; host and device therefore differ by at most 2 ulp.  The two kernels state the same arithmetic in the
same order: their outputs are equal bit for bit."""
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
SENT_I, SENT_F = -0x0123456789abcdef, -12345.5


def _ordered(a: np.ndarray) -> np.ndarray:
    """float32 -> integers whose difference is the distance in ulp"""
    i = np.ascontiguousarray(a, dtype=np.float32).view(np.int32).astype(np.int64)
    return np.where(i < 0, -(i & 0x7fffffff), i)


def _ulp(a, b) -> int:
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    assert a.shape == b.shape and np.all(np.isfinite(a)) and np.all(np.isfinite(b))
    return int(np.abs(_ordered(a) - _ordered(b)).max()) if a.size else 0


def _log_exact(x_int: np.ndarray) -> np.ndarray:
    return np.log((x_int.astype(np.float32) + np.float32(1)).astype(np.float64)).astype(np.float32)


def _rows(rng, n, nd, nc, dense_hi=500):
    """(x_int, x_cat, y): categorical entries over the whole int32 range, a fifth of them at its edges and around zero"""
    x_int = rng.randint(0, dense_hi, size=(n, nd)).astype(np.int32)
    x_cat = rng.randint(-2 ** 31, 2 ** 31, size=(n, nc), dtype=np.int64).astype(np.int32)
    edge = np.array([2 ** 31 - 1, 2 ** 31 - 2, -2 ** 31, -2 ** 31 + 1, -1, 0, 1], dtype=np.int64).astype(np.int32)
    where = rng.rand(n, nc) < 0.2
    x_cat[where] = edge[rng.randint(0, len(edge), size=int(where.sum()))]
    y = rng.randint(0, 2, size=n).astype(np.int32)
    return x_int, x_cat, y


def _records(x_int, x_cat, y) -> np.ndarray:
    """[y | dense | categorical] int32, as the binary file stores a sample"""
    return np.ascontiguousarray(np.concatenate([y.reshape(-1, 1), x_int, x_cat], axis=1).astype(np.int32))


def write_bin(path, x_int, x_cat, y) -> np.ndarray:
    rec = _records(np.asarray(x_int), np.asarray(x_cat), np.asarray(y))
    with open(path, "wb") as f:
        f.write(rec.tobytes())
    return rec


def _on_device(a: np.ndarray, offset: int = 0) -> torch.Tensor:
    """the array on the device, `offset` dwords behind a 16-byte aligned base"""
    buf = torch.empty(a.size + 8, dtype=torch.int32, device=DEV)
    assert buf.data_ptr() % 16 == 0
    v = buf[offset:offset + a.size].view(a.shape)
    v.copy_(torch.from_numpy(a))
    return v


def _window(rows, nd, nc):
    return (torch.full((rows, nd), SENT_F, dtype=torch.float32, device=DEV),
            torch.full((nc, rows), SENT_I, dtype=torch.int64, device=DEV),
            torch.full((rows, 1), SENT_F, dtype=torch.float32, device=DEV))


@pytest.mark.parametrize("nd,nc", [(13, 26), (5, 7), (1, 1), (3, 60)])
@pytest.mark.parametrize("col0", [0, 1, 3])
def test_binfile_window_kernel_matches_the_host_transform(nd, nc, col0):
    """Every n at a tile edge, the record stream at every dword offset from a 16-byte boundary, a rectangle wider than the
    piece whose other cells keep their sentinel, negative categorical entries under the modulus."""
    from cdlrm_amd import ops
    from cdlrm_amd.data_loader_terabyte import transform_features
    tile = ops.binfile_tile()
    rng = np.random.RandomState(1000 * nd + 10 * nc + col0)
    for n in (tile - 1, tile, tile + 1, 3 * tile + 5):
        for mir, offset in ((-1, 0), (7, 1), (40000, 2), (2 ** 31 - 1, 3), (0, col0)):
            arrs = _rows(rng, n, nd, nc)
            rows = col0 + n + 9
            X, I, T = _window(rows, nd, nc)
            ops.binfile_window(_on_device(_records(*arrs), offset), nd, mir, X, I, T, col0=col0)
            torch.cuda.synchronize()
            hX, _, hI, hT = transform_features(*arrs, mir)
            X, I, T = X.cpu(), I.cpu(), T.cpu()
            tag = (nd, nc, col0, n, mir, offset)
            assert torch.equal(I[:, col0:col0 + n], hI), tag
            assert torch.equal(T[col0:col0 + n], hT), tag
            if mir > 0:
                assert int(I[:, col0:col0 + n].min()) >= 0 and int(I[:, col0:col0 + n].max()) < mir
            d_exact, d_host = _ulp(X[col0:col0 + n].numpy(), _log_exact(arrs[0])), _ulp(X[col0:col0 + n].numpy(), hX.numpy())
            assert d_exact <= 1 and d_host <= 2, tag + (d_exact, d_host)
            # nothing outside the piece's samples is written
            assert bool((I[:, :col0] == SENT_I).all()) and bool((I[:, col0 + n:] == SENT_I).all()), tag
            assert bool((X[:col0] == SENT_F).all()) and bool((X[col0 + n:] == SENT_F).all()), tag
            assert bool((T[:col0] == SENT_F).all()) and bool((T[col0 + n:] == SENT_F).all()), tag


def test_binfile_window_pieces_of_one_window_and_refusals():
    """several pieces of one window, one launch each, through views of the window's buffers; what does not fit is refused
    before any launch"""
    from cdlrm_amd import ops
    from cdlrm_amd.data_loader_terabyte import transform_features
    rng = np.random.RandomState(5)
    segs = [_rows(rng, n, 13, 26) for n in (300, 1, 511)]
    W = sum(s[2].shape[0] for s in segs)
    X, I, T = _window(W, 13, 26)
    col = 0
    for s in segs:
        ops.binfile_window(_on_device(_records(*s)), 13, 1000, X, I, T, col0=col)
        col += s[2].shape[0]
    torch.cuda.synchronize()
    hX, _, hI, hT = transform_features(*(np.concatenate([s[i] for s in segs]) for i in range(3)), 1000)
    assert torch.equal(I.cpu(), hI) and torch.equal(T.cpu(), hT) and _ulp(X.cpu().numpy(), hX.numpy()) <= 2
    with pytest.raises(AssertionError):
        ops.binfile_window(_on_device(_records(*segs[0])), 13, 1000, X, I, T, col0=W - 299)
    from cdlrm_amd._lib import CdlrmError
    with pytest.raises(CdlrmError):             # 61 categorical features: the library refuses
        ops.binfile_window(_on_device(np.zeros((4, 65), np.int32)), 3, -1, *_window(4, 3, 61))


@pytest.mark.parametrize("nd,nc", [(13, 26), (5, 7), (1, 1), (3, 60)])
def test_binfile_window_is_bit_identical_to_the_dayfile_kernel(nd, nc):
    from cdlrm_amd import ops
    tile = ops.binfile_tile()
    assert tile == ops.dayfile_tile()
    rng = np.random.RandomState(77 + nc)
    for n, mir, col0 in ((tile - 1, -1, 0), (tile + 1, 40000, 3), (3 * tile + 5, 7, 1), (40 * tile + 3, 2 ** 31 - 1, 0)):
        x_int, x_cat, y = _rows(rng, n, nd, nc, dense_hi=2 ** 31 - 1)
        rows = col0 + n + 2
        a, b = _window(rows, nd, nc), _window(rows, nd, nc)
        ops.binfile_window(_on_device(_records(x_int, x_cat, y)), nd, mir, *a, col0=col0)
        ops.dayfile_window(_on_device(x_int), _on_device(x_cat), _on_device(y), mir, *b, col0=col0)
        torch.cuda.synchronize()
        for u, v, what in zip(a, b, ("X", "lS_i", "T")):
            u, v = u.cpu(), v.cpu()
            if u.dtype == torch.float32:
                u, v = u.view(torch.int32), v.view(torch.int32)
            assert torch.equal(u, v), (what, nd, nc, n, mir, col0)


# ------------------------------------------------------------------------------------------------ the loader

def _golden_files(g, d):
    files = {}
    for split in ("train", "test", "val"):
        files[split] = os.path.join(d, split + ".bin")
        with open(files[split], "wb") as f:
            f.write(g[split + "_bytes"].tobytes())
    counts = os.path.join(d, "day_fea_count.npz")
    np.savez(counts, counts=np.full(26, 100000))
    return files, counts


def _dense_of(file_bytes):
    return np.frombuffer(file_bytes.tobytes(), dtype=np.int32).reshape(-1, 40)[:, 1:14]


def _check_epoch(batches, g, name, exact, tag):
    assert [b[3].shape[0] for b in batches] == g[name + "_sizes"].tolist(), tag
    assert torch.equal(torch.cat([b[2] for b in batches], dim=1).cpu(), torch.from_numpy(g[name + "_lS_i"])), tag
    assert torch.equal(torch.cat([b[3] for b in batches]).cpu(), torch.from_numpy(g[name + "_T"])), tag
    assert torch.equal(batches[-1][1].cpu(), torch.from_numpy(g[name + "_lS_o_last"])), tag
    for b in batches:
        assert torch.equal(b[1].cpu(), torch.arange(b[3].shape[0]).repeat(26, 1)), tag
    X = torch.cat([b[0] for b in batches]).cpu().numpy()
    assert _ulp(X, exact) <= 1 and _ulp(X, g[name + "_X"]) <= 2, tag
    X0, lS_o, lS_i, T = batches[0]
    assert X0.dtype == torch.float32 and lS_i.dtype == torch.int64 and lS_o.dtype == torch.int64 and T.shape[1] == 1
    assert all(t.is_cuda for t in batches[0])


@pytest.mark.parametrize("window", [1, 2, 3, 5])
@pytest.mark.parametrize("split,mir", [("train", 50), ("train", -1), ("test", 50), ("val", -1)])
def test_device_bin_loader_matches_reference(golden, tmp_path, split, mir, window):
    from cdlrm_amd.data_loader_terabyte import CriteoBinDataset, DeviceBinLoader
    g = golden("criteo_bin")
    files, counts = _golden_files(g, str(tmp_path))
    B = int(g["B"])
    name = "%s_m%d" % (split, mir if mir > 0 else 0)
    ld = DeviceBinLoader(CriteoBinDataset(files[split], counts, B, mir), device=DEV, window=window)
    assert len(ld) == int(g[name + "_len"])
    exact = _log_exact(_dense_of(g[split + "_bytes"]))
    sizes = g[name + "_sizes"].tolist()
    for epoch in range(2):
        # (every batch is copied as it is handed out: the loader reuses a window's buffers two windows later)
        got, shape = [], []
        for b in ld:
            got.append(tuple(t.clone() for t in b))
            shape.append((b.win_pos, b.win_batches, b.window_rect.shape[1]))
        torch.cuda.synchronize()
        _check_epoch(got, g, name, exact, (split, mir, window, epoch))
        # unshuffled, the short last batch is the last batch of the last window: every window before it is whole
        want = [(j % window, min(window, len(sizes) - j // window * window), sum(sizes[j // window * window:][:window]))
                for j in range(len(sizes))]
        assert shape == want
    first = next(iter(ld))
    assert first.win_pos == 0 and first.window_rect.shape == (26, sum(sizes[:window]))
    assert first[2].data_ptr() == first.window_rect.data_ptr() and first[2].stride(1) == 1      # a view: no copy


@pytest.mark.parametrize("window", [1, 2, 3, 5])
def test_device_bin_loader_shuffled_matches_reference(golden, tmp_path, window):
    """`RandomSampler`'s order under the golden's seed, two epochs.  In epoch 0 the short entry comes fifth: the window that
    holds it has fewer than window * B columns and the batches behind it start where it ends."""
    from cdlrm_amd.data_loader_terabyte import CriteoBinDataset, DeviceBinLoader
    g = golden("criteo_bin")
    files, counts = _golden_files(g, str(tmp_path))
    B = int(g["B"])
    ld = DeviceBinLoader(CriteoBinDataset(files["train"], counts, B, 50), shuffle=True, device=DEV, window=window)
    dense = _dense_of(g["train_bytes"])
    torch.manual_seed(int(g["seed"]))
    assert g["shuffle_e0_sizes"].tolist().index(5) == 4
    for epoch in range(2):
        name = "shuffle_e%d" % epoch
        order, sizes = g[name + "_order"].tolist(), g[name + "_sizes"].tolist()
        got, rects = [], []
        for b in ld:
            got.append(tuple(t.clone() for t in b))
            rects.append((b.win_pos, b.window_rect.shape[1], b[2].data_ptr() - b.window_rect.data_ptr()))
        torch.cuda.synchronize()
        exact = _log_exact(np.concatenate([dense[i * B:(i + 1) * B] for i in order]))
        _check_epoch(got, g, name, exact, (window, epoch))
        for j, (pos, cols, off) in enumerate(rects):
            w0 = j - pos
            assert pos == j % window and cols == sum(sizes[w0:w0 + window]) and off == 8 * sum(sizes[w0:j]), (window, epoch, j)


def test_device_bin_loader_ring_is_safe_under_a_slow_consumer(tmp_path):
    """tests/test_dayfile_device.py's ring test for the binary loader.  Many short windows; the consumer is SLOW (a spin kernel
    in front of every read, on the stream the batches are handed out on) and every yielded batch of the two most recent
    windows is held as the view it is.  The reads of window u are still queued when the loader recycles the slot of window
    u - 2 and uploads ahead: only the ring rule keeps them right.  Shuffled and not."""
    from cdlrm_amd.data_loader_terabyte import BinLoader, CriteoBinDataset, DeviceBinLoader
    rng = np.random.RandomState(17)
    x_int, x_cat, y = _rows(rng, 331 + 257 + 129, 13, 26)
    write_bin(str(tmp_path / "t.bin"), x_int, x_cat, y)
    np.savez(str(tmp_path / "c.npz"), counts=np.full(26, 5000))
    B, L = 8, 2
    ds = CriteoBinDataset(str(tmp_path / "t.bin"), str(tmp_path / "c.npz"), B, 5000)
    for shuffle in (False, True):
        host = BinLoader(ds, shuffle=shuffle)
        ld = DeviceBinLoader(ds, shuffle=shuffle, device=DEV, window=L)
        assert len(host) == len(ld) >= 80
        for epoch in range(2):
            torch.manual_seed(100 + epoch)
            want = list(host)
            torch.manual_seed(100 + epoch)
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
                assert torch.equal(I.cpu(), want[j][2]) and torch.equal(T.cpu(), want[j][3]), (shuffle, epoch, j)
                assert _ulp(X.cpu().numpy(), want[j][0].numpy()) <= 2
            assert len(held) >= L + 1
            for j, b in held:                   # the two most recent windows, as the views that were handed out
                assert torch.equal(b[2].cpu(), want[j][2]) and torch.equal(b[3].cpu(), want[j][3]), (shuffle, epoch, j)
                assert torch.equal(b[1].cpu(), want[j][1])


def test_device_bin_loader_cuts_pieces_at_the_stage(tmp_path):
    """a window longer than the pinned stage (STAGE_BATCHES batches) goes up in several pieces, each at its column"""
    from cdlrm_amd.data_loader_terabyte import BinLoader, CriteoBinDataset, DeviceBinLoader
    rng = np.random.RandomState(23)
    write_bin(str(tmp_path / "t.bin"), *_rows(rng, 16 * 40 + 9, 13, 26))
    np.savez(str(tmp_path / "c.npz"), counts=np.full(26, 77))
    ds = CriteoBinDataset(str(tmp_path / "t.bin"), str(tmp_path / "c.npz"), 16, 77)

    class Small(DeviceBinLoader):
        STAGE_BATCHES = 3

    ld = Small(ds, device=DEV, window=10)
    for epoch in range(2):
        got = [tuple(t.clone() for t in b) for b in ld]
        torch.cuda.synchronize()
        want = list(BinLoader(ds))
        assert len(got) == len(want) == 41
        for g_, w in zip(got, want):
            assert torch.equal(g_[2].cpu(), w[2]) and torch.equal(g_[3].cpu(), w[3]) and _ulp(g_[0].cpu().numpy(), w[0].numpy()) <= 2


# ------------------------------------------------------------------------------------------------ training

FLAGS = ["--arch-sparse-feature-size=16", "--arch-mlp-bot=13-32-16", "--arch-mlp-top=32-1", "--mini-batch-size=64",
         "--lookahead=4", "--cache-size=40", "--num-ways=4", "--loss-function=bce", "--round-targets=True",
         "--learning-rate=0.1", "--lr-embeds=0.3", "--print-freq=1", "--numpy-rand-seed=11", "--table-agg-freq=5",
         "--data-generation=dataset"]
COUNTS = np.array([900, 40, 7, 300, 1500])


def _cli_rows(n, seed=3):
    rng = np.random.RandomState(seed)
    return (rng.randint(0, 500, size=(n, 13)).astype(np.int32),
            np.stack([rng.randint(0, c, size=n) for c in COUNTS], axis=1).astype(np.int32), rng.randint(0, 2, size=n).astype(np.int32))


def _cli_bin_files(d, n_train, n_test=150):
    """<d>/tb_train.bin, <d>/tb_test.bin, <d>/day_fea_count.npz -> the flags that name them"""
    write_bin(os.path.join(d, "tb_train.bin"), *_cli_rows(n_train))
    write_bin(os.path.join(d, "tb_test.bin"), *_cli_rows(n_test, seed=4))
    np.savez(os.path.join(d, "day_fea_count.npz"), counts=COUNTS)
    return ["--mlperf-bin-loader", "--raw-data-file=" + os.path.join(d, "day"),
            "--processed-data-file=" + os.path.join(d, "tb.npz")]


def _losses(out):
    return [float(x) for x in re.findall(r"Loss = ([0-9.eE+-]+),", out)]


def _compare_runs(outs, tags, n_steps, world, a="host", b="device"):
    losses = {k: _losses(o) for k, o in outs.items()}
    assert len(losses[a]) == len(losses[b]) == n_steps - 1, outs[b][-2000:]
    rel = np.abs(np.array(losses[b]) - np.array(losses[a])) / np.abs(np.array(losses[a]))
    print("world %d: largest relative loss deviation %s vs %s: %.3g" % (world, b, a, rel.max()))
    assert rel.max() <= 1e-5
    acc = {k: re.findall(r"Test accuracy = .*", o) for k, o in outs.items()}
    assert len(acc[a]) >= 1 and acc[a] == acc[b]
    for r in range(world):
        ta, tb = torch.load(tags[a] + ".rank%d" % r), torch.load(tags[b] + ".rank%d" % r)
        assert ta.dtype == torch.int64 and int((ta >= 0).sum()) > 0
        assert torch.equal(ta, tb), "cache tags differ on rank %d" % r


@pytest.fixture()
def keep_current_stream():
    """`main_no_ddp.Run` makes a stream of its own the thread's current one (as the CLI process should); tests that run after
    this module in the same process expect the stream they started on."""
    before = torch.cuda.current_stream()
    yield
    torch.cuda.synchronize()
    torch.cuda.set_stream(before)


@pytest.mark.parametrize("extra", [["--device-rng"], [], ["--device-rng", "--mlperf-bin-shuffle"]],
                         ids=["lookahead-plan", "plan-at-boundary", "shuffled"])
def test_cli_bin_loader_device_trains_like_host(tmp_path, capsys, monkeypatch, keep_current_stream, extra):
    """Three windows (4 + 4 + 1 batches) and a short last batch of 39 records, which the training loader leaves out."""
    from cdlrm_amd import main_no_ddp
    n = 64 * 9 + 39
    flags = _cli_bin_files(str(tmp_path), n)
    outs, tags = {}, {}
    for mode in ("host", "device"):
        tags[mode] = os.path.join(tmp_path, "tags_" + mode)
        monkeypatch.setenv("CDLRM_DUMP_TAGS", tags[mode])
        main_no_ddp.main(FLAGS + extra + flags + ["--world-size=1", "--day-file-loader=" + mode])
        outs[mode] = capsys.readouterr().out
    _compare_runs(outs, tags, n // 64, 1)
    assert "MLPerf binary loader: BinLoader (host) reads " + os.path.join(tmp_path, "tb_train.bin") in outs["host"]
    assert "MLPerf binary loader: DeviceBinLoader (device) reads " + os.path.join(tmp_path, "tb_train.bin") in outs["device"]
    assert "Day-file loader" not in outs["device"]


def _child_env():
    env = dict(os.environ)
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT", "MASTER_ADDR", "GROUP_RANK", "LOCAL_WORLD_SIZE",
              "TORCHELASTIC_RUN_ID"):
        env.pop(k, None)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    return env


def test_cli_bin_loader_world_size_2(tmp_path):
    """Two ranks emulated on one GPU (CDLRM_BENCH_EMULATE=1, as tests/test_self_launch.py): every rank reads the file itself,
    uploads whole windows and trains its column slice."""
    n = 64 * 17 + 39
    flags = _cli_bin_files(str(tmp_path), n)
    env = _child_env()
    env["CDLRM_BENCH_EMULATE"] = "1"
    outs, tags = {}, {}
    for mode in ("host", "device"):
        tags[mode] = os.path.join(tmp_path, "tags_" + mode)
        env["CDLRM_DUMP_TAGS"] = tags[mode]
        p = subprocess.run([sys.executable, "-m", "cdlrm_amd.main_no_ddp"] + FLAGS + flags +
                           ["--world-size=2", "--table-agg-freq=3", "--test-freq=6", "--device-rng", "--day-file-loader=" + mode],
                           env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
        assert p.returncode == 0, p.stderr[-3000:]
        outs[mode] = p.stdout
    _compare_runs(outs, tags, n // 64, 2)
    assert "MLPerf binary loader: DeviceBinLoader" in outs["device"]


def test_cli_bin_run_ends_on_the_tags_of_the_day_file_run(tmp_path, capsys, monkeypatch, keep_current_stream):
    """The same samples once as ONE day file (train and test both read it: the test split is its first half) and once as
    tb_train.bin + tb_test.bin: the same batches -- nine of 64, the short tenth left out by both -- so the same losses, test
    accuracy and final cache tags."""
    from cdlrm_amd import main_no_ddp
    n = 64 * 9 + 39
    x_int, x_cat, y = _cli_rows(n)
    d = str(tmp_path)
    np.savez(os.path.join(d, "day_0_reordered.npz"), X_int=x_int, X_cat=x_cat, y=y)
    np.savez(os.path.join(d, "day_day_count.npz"), total_per_file=np.array([n]))
    np.savez(os.path.join(d, "day_fea_count.npz"), counts=COUNTS)
    half = int(np.ceil(n / 2.))
    write_bin(os.path.join(d, "tb_train.bin"), x_int, x_cat, y)
    write_bin(os.path.join(d, "tb_test.bin"), x_int[:half], x_cat[:half], y[:half])
    raw = "--raw-data-file=" + os.path.join(d, "day")
    runs = dict(day=[raw, "--day-file-loader=host"],
                bin=[raw, "--mlperf-bin-loader", "--processed-data-file=" + os.path.join(d, "tb.npz"), "--day-file-loader=device"])
    outs, tags = {}, {}
    for k, flags in runs.items():
        tags[k] = os.path.join(d, "tags_" + k)
        monkeypatch.setenv("CDLRM_DUMP_TAGS", tags[k])
        main_no_ddp.main(FLAGS + ["--device-rng", "--world-size=1"] + flags)
        outs[k] = capsys.readouterr().out
    _compare_runs(outs, tags, n // 64, 1, a="day", b="bin")
    assert "MLPerf binary loader" in outs["bin"] and "MLPerf binary loader" not in outs["day"]


def test_cli_flag_is_no_longer_ignored(tmp_path):
    """with --mlperf-bin-loader and only day files present the run ends on one ERROR line that names the binary file"""
    d = str(tmp_path)
    x_int, x_cat, y = _cli_rows(64 * 3)
    np.savez(os.path.join(d, "day_0_reordered.npz"), X_int=x_int, X_cat=x_cat, y=y)
    np.savez(os.path.join(d, "day_day_count.npz"), total_per_file=np.array([64 * 3]))
    np.savez(os.path.join(d, "day_fea_count.npz"), counts=COUNTS)
    p = subprocess.run([sys.executable, "-m", "cdlrm_amd.main_no_ddp"] + FLAGS +
                       ["--world-size=1", "--data-set=terabyte", "--large-batch", "--memory-map", "--mlperf-bin-loader",
                        "--raw-data-file=" + os.path.join(d, "day"), "--processed-data-file=" + os.path.join(d, "tb.npz")],
                       env=_child_env(), capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert p.returncode != 0 and "Loss =" not in p.stdout
    lines = [l for l in p.stderr.splitlines() if l.startswith("ERROR:")]
    assert len(lines) == 1 and os.path.join(d, "tb_train.bin") in lines[0], p.stderr[-2000:]
