"""Rows of the processed Criteo file cut on the device by an order: the kernel (`ops.rows_window`, csrc/dayfile.hip:
k_rows_window) against `ops.dayfile_window` on the same rows gathered on the host -- bit for bit -- and against the host
transform, a byte offset beyond 2^32, the entry point's refusals, `DeviceProcessedLoader` against `ProcessedLoader` while its
ring is being reused, and the CLI with `--day-file-loader=device` against the same run with the host loader (one rank, and two
ranks emulated on one GPU) and against the oracle trainer fed the reference's batches (tests/golden/criteo_processed.npz).

Bounds (tests/test_dayfile_device.py).  Indices and targets are integers: equal bit for bit.  X = log(x + 1) is compared
with the correctly rounded value float32(log(float64(float32(x) + float32(1)))): at most 1 ulp away, the bound the host's
torch.log keeps itself; host and device therefore differ by at most 2 ulp.  The two device kernels share their arithmetic:
for the same rows they give the same bits."""
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
    assert np.all(np.isfinite(a)) and np.all(np.isfinite(b))
    return int(np.abs(_ordered(a) - _ordered(b)).max()) if a.size else 0


def _log_exact(x_int: np.ndarray) -> np.ndarray:
    return np.log((x_int.astype(np.float32) + np.float32(1)).astype(np.float64)).astype(np.float32)


def _rows(rng, n, nd, nc):
    x_int = rng.randint(0, 500, size=(n, nd)).astype(np.int32)
    dense_edge = np.array([0, 1, 2 ** 24 - 1, 2 ** 24, 2 ** 24 + 1, 2 ** 31 - 1], dtype=np.int64).astype(np.int32)
    where = rng.rand(n, nd) < 0.2
    x_int[where] = dense_edge[rng.randint(0, len(dense_edge), size=int(where.sum()))]
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
        v.copy_(torch.from_numpy(np.ascontiguousarray(a)))
        out.append(v)
    return out


def _window(nd, nc, rows):
    return (torch.full((rows, nd), SENT_F, dtype=torch.float32, device=DEV),
            torch.full((nc, rows), SENT_I, dtype=torch.int64, device=DEV),
            torch.full((rows, 1), SENT_F, dtype=torch.float32, device=DEV))


@pytest.mark.parametrize("nd,nc", [(13, 26), (1, 1), (5, 7), (3, 60)])
@pytest.mark.parametrize("offset", [0, 1, 2, 3])      # dwords off a 16-byte base (0 and 2: 8-byte row loads at an even n_cat)
def test_rows_window_kernel_equals_the_consecutive_kernel_on_gathered_rows(nd, nc, offset):
    from cdlrm_amd import ops
    from cdlrm_amd.data_loader_terabyte import transform_features
    tile = ops.rows_tile()
    assert tile == ops.dayfile_tile()
    rng = np.random.RandomState(1000 * nd + 10 * nc + offset)
    n_rows = 2 * tile + 3 + 29
    src = _rows(rng, n_rows, nd, nc)
    dsrc = _dev_rows(src, offset)           # resident once; every case below picks from it
    for ni, n in enumerate((1, tile - 1, tile, tile + 1, 2 * tile + 3)):
        orders = dict(identity=np.arange(n), reversed=n_rows - 1 - np.arange(n), random=rng.permutation(n_rows)[:n],
                      repeated=rng.choice(rng.randint(0, n_rows, size=3), size=n))
        for ki, (kind, order) in enumerate(orders.items()):
            # over the five sizes every order meets every range and every column offset (0, and off every alignment)
            mir = (-1, 0, 7, 2 ** 31 - 1)[(ki + ni) % 4]
            col0 = (0, 3 * tile + 5, 1, 6)[(ki + 3 * ni + 1) % 4]
            order = order.astype(np.int64)
            tag = (nd, nc, offset, n, kind, mir, col0)
            rows = col0 + n + 9
            got, want = _window(nd, nc, rows), _window(nd, nc, rows)
            ops.rows_window(*dsrc, torch.from_numpy(order).to(DEV), mir, *got, col0=col0)
            picked = tuple(a[order] for a in src)
            ops.dayfile_window(*_dev_rows(picked, offset), mir, *want, col0=col0)
            torch.cuda.synchronize()
            got, want = [t.cpu() for t in got], [t.cpu() for t in want]
            # bit for bit, sentinels around the piece included: nothing outside columns [col0, col0 + n) is written
            assert torch.equal(got[0].view(torch.int32), want[0].view(torch.int32)), tag
            assert torch.equal(got[1], want[1]) and torch.equal(got[2].view(torch.int32), want[2].view(torch.int32)), tag
            X, I, T = got
            assert bool((I[:, :col0] == SENT_I).all()) and bool((I[:, col0 + n:] == SENT_I).all()), tag
            assert bool((X[:col0] == SENT_F).all()) and bool((X[col0 + n:] == SENT_F).all()), tag
            assert bool((T[:col0] == SENT_F).all()) and bool((T[col0 + n:] == SENT_F).all()), tag
            hX, _, hI, hT = transform_features(*picked, mir)
            assert torch.equal(I[:, col0:col0 + n], hI) and torch.equal(T[col0:col0 + n], hT), tag
            if mir > 0:
                assert int(I[:, col0:col0 + n].min()) >= 0 and int(I[:, col0:col0 + n].max()) < mir
            assert _ulp(X[col0:col0 + n].numpy(), _log_exact(picked[0])) <= 1, tag
            assert _ulp(X[col0:col0 + n].numpy(), hX.numpy()) <= 2, tag


def test_rows_window_reaches_rows_beyond_a_4_gib_byte_offset():
    """x_cat of 2^32 // 104 + 16 rows of 26: the last rows start past byte 2^32, the smallest shape at which a row address
    formed in 32 bits goes wrong.  The array is allocated and left untouched but for its first and last few rows."""
    from cdlrm_amd import ops
    n_rows, nd, nc, k = 2 ** 32 // 104 + 16, 1, 26, 5
    assert (n_rows - k) * 104 > 2 ** 32
    x_cat = torch.empty(n_rows, nc, dtype=torch.int32, device=DEV)
    x_int = torch.empty(n_rows, nd, dtype=torch.int32, device=DEV)
    y = torch.empty(n_rows, dtype=torch.int32, device=DEV)
    rng = np.random.RandomState(2)
    ends = _rows(rng, 2 * k, nd, nc)
    where = np.concatenate([np.arange(k), np.arange(n_rows - k, n_rows)])
    for dst, a in zip((x_int, x_cat, y), ends):
        dst[:k].copy_(torch.from_numpy(a[:k]))
        dst[n_rows - k:].copy_(torch.from_numpy(a[k:]))
    pick = rng.permutation(2 * k)
    order = torch.from_numpy(where[pick].astype(np.int64)).to(DEV)
    X, I, T = _window(nd, nc, 2 * k)
    ops.rows_window(x_int, x_cat, y, order, -1, X, I, T)
    torch.cuda.synchronize()
    assert torch.equal(I.cpu(), torch.from_numpy(ends[1][pick].astype(np.int64)).t())
    assert torch.equal(T.cpu().view(-1), torch.from_numpy(ends[2][pick].astype(np.float32)))
    assert _ulp(X.cpu().numpy(), _log_exact(ends[0][pick])) <= 1
    del x_cat, x_int, y
    torch.cuda.empty_cache()


def test_rows_window_refusals_return_an_error_code_and_launch_nothing():
    from cdlrm_amd import _lib
    L = _lib.raw()
    rng = np.random.RandomState(4)
    n = 40
    X, I, T = _window(13, 61, n + 8)
    order = torch.arange(n, dtype=torch.int64, device=DEV)
    st = torch.cuda.current_stream().cuda_stream

    def call(x_cat_cols, n_cat, order_ptr, pitch, col0, n_rows=n):
        xi, xc, y = _dev_rows(_rows(rng, n, 13, x_cat_cols), 0)
        return L.cdlrm_rows_window(xi.data_ptr(), xc.data_ptr(), y.data_ptr(), n_rows, order_ptr, n, 13, n_cat, -1, X.data_ptr(),
                                   I.data_ptr(), pitch, col0, T.data_ptr(), st)

    assert call(61, 61, order.data_ptr(), n + 8, 0) != 0 and b"60" in L.cdlrm_last_error()
    assert call(26, 26, None, n + 8, 0) != 0 and b"null" in L.cdlrm_last_error()
    assert call(26, 26, order.data_ptr(), 8 + n - 1, 8) != 0 and b"rectangle" in L.cdlrm_last_error()
    assert call(26, 26, order.data_ptr() + 4, n + 8, 0) != 0 and b"misaligned" in L.cdlrm_last_error()
    assert call(26, 26, order.data_ptr(), n + 8, 0, n_rows=0) != 0
    torch.cuda.synchronize()
    assert bool((X == SENT_F).all()) and bool((I == SENT_I).all()) and bool((T == SENT_F).all())
    assert call(26, 26, order.data_ptr(), n + 8, 8) == 0        # ... and the same call with a pitch that fits goes through
    torch.cuda.synchronize()
    assert bool((I[:26, 8:] != SENT_I).all()) and bool((I[:, :8] == SENT_I).all())


# ------------------------------------------------------------------------------------------------ the loader

MODES = ("total", "day", "none")


def _files(g, d):
    pro = os.path.join(d, "kaggleAdDisplayChallenge_processed.npz")
    np.savez(pro, X_int=g["X_int"], X_cat=g["X_cat"], y=g["y"], counts=g["counts"])
    np.savez(os.path.join(d, "train_day_count.npz"), total_per_file=g["sizes"])
    return pro


@pytest.mark.parametrize("mir", [-1, 50])
@pytest.mark.parametrize("randomize", MODES)
def test_device_processed_loader_matches_the_host_loader(golden, tmp_path, randomize, mir):
    from cdlrm_amd.data_loader_processed import DeviceProcessedLoader, ProcessedDataset, ProcessedLoader, processed_order
    g = golden("criteo_processed")
    ds = ProcessedDataset(_files(g, str(tmp_path)), g["sizes"])
    B = int(g["B"])
    np.random.seed(int(g["seed"]))
    orders = {split: processed_order(g["sizes"], split, randomize) for split in ("train", "test")}
    for split, drop in (("train", False), ("train", True), ("test", False)):
        want = list(ProcessedLoader(ds, orders[split], B, mir, drop))
        sizes = [b[3].shape[0] for b in want]
        exact = _log_exact(ds.X_int[orders[split]][:sum(sizes)])
        for window in (1, 3, len(want) + 2):
            ld = DeviceProcessedLoader(ds, orders[split], B, mir, drop, device=DEV, window=window)
            assert len(ld) == len(want)
            assert (ld.first_row is None) == (split == "train" and randomize != "none")     # consecutive rows need no order
            for epoch in range(2):
                # (every batch is copied as it is handed out: the loader reuses a window's buffers two windows later)
                got, shape = [], []
                for b in ld:
                    got.append(tuple(t.clone() for t in b))
                    shape.append((b.win_pos, b.win_batches, b.window_rect.shape[1], b[2].data_ptr() - b.window_rect.data_ptr()))
                torch.cuda.synchronize()
                tag = (randomize, mir, split, drop, window, epoch)
                assert len(got) == len(want), tag
                for j, (b, w) in enumerate(zip(got, want)):
                    assert torch.equal(b[2].cpu(), w[2]) and torch.equal(b[3].cpu(), w[3]) and torch.equal(b[1].cpu(), w[1]), tag
                    assert _ulp(b[0].cpu().numpy(), w[0].numpy()) <= 2, tag
                    assert all(t.is_cuda for t in b) and b[2].dtype == torch.int64 and b[0].dtype == torch.float32
                assert _ulp(torch.cat([b[0] for b in got]).cpu().numpy(), exact) <= 1, tag
                # window_rect / win_pos / win_batches: batch j is columns [sum of the sizes before it, ...) of its window's rectangle
                assert shape == [(j % window, min(window, len(sizes) - j // window * window),
                                  sum(sizes[j // window * window:][:window]), 8 * sum(sizes[j // window * window:j]))
                                 for j in range(len(sizes))], tag
            first = next(iter(ld))
            assert first[2].data_ptr() == first.window_rect.data_ptr() and first[2].stride(1) == 1      # a view: no copy
            if split == "test":
                name = "%s_test_m%d" % (randomize, mir if mir > 0 else 0)       # ... and the reference's own batches
                assert torch.equal(torch.cat([b[2] for b in got], dim=1).cpu(), torch.from_numpy(g[name + "_lS_i"]))
                assert _ulp(torch.cat([b[0] for b in got]).cpu().numpy(), g[name + "_X"]) <= 2
    # the train and the test loaders read ONE resident copy
    assert ds.uploads == 1


def test_device_processed_loader_refuses_what_does_not_fit_before_it_allocates(golden, tmp_path):
    from cdlrm_amd.data_loader_processed import DeviceProcessedLoader, ProcessedDataset, processed_order
    g = golden("criteo_processed")
    ds = ProcessedDataset(_files(g, str(tmp_path)), g["sizes"])
    order = processed_order(g["sizes"], "train", "total", np.random.RandomState(1))
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated(DEV)
    ld = DeviceProcessedLoader(ds, order, 16, device=DEV, window=3, hbm_fraction=1e-9)
    with pytest.raises(ValueError, match="--day-file-loader=host") as e:
        next(iter(ld))
    assert "kaggleAdDisplayChallenge_processed.npz" in str(e.value) and "GB" in str(e.value)
    assert torch.cuda.memory_allocated(DEV) == before and ds.uploads == 0 and ld._slots is None
    raw, ordr, ring = ld.hbm_bytes(len(ld))
    assert raw == len(ds) * 160 and ordr == 8 * order.size and ring == 3 * 3 * 16 * (13 * 4 + 26 * 8 + 4)
    ok = DeviceProcessedLoader(ds, order, 16, device=DEV, window=3)         # the default fraction takes it
    assert len(list(ok)) == len(ok) and ds.uploads == 1
    assert DeviceProcessedLoader(ds, order, 16, device=DEV, window=3).hbm_bytes(len(ok))[0] == 0    # resident by now


def test_device_processed_loader_ring_is_safe_under_a_slow_consumer(tmp_path):
    """tests/test_dayfile_device.py's ring test for the resident loader.  Many short windows; the consumer is SLOW (a spin
    kernel in front of every read, on the stream the batches are handed out on) and every yielded batch of the two most recent
    windows is held as the view it is, until the window two later is asked for."""
    from cdlrm_amd.data_loader_processed import DeviceProcessedLoader, ProcessedDataset, ProcessedLoader, processed_order
    rng = np.random.RandomState(17)
    sizes = [201, 1, 160, 97, 129, 64, 65]
    xi, xc, y = _rows(rng, sum(sizes), 13, 26)
    pro = str(tmp_path / "terabyte_processed.npz")
    np.savez(pro, X_int=xi, X_cat=xc, y=y, counts=np.full(26, 5000))
    ds = ProcessedDataset(pro, sizes)
    order = processed_order(sizes, "train", "total", rng)
    B, L = 8, 2
    want = list(ProcessedLoader(ds, order, B, 5000))
    ld = DeviceProcessedLoader(ds, order, B, 5000, device=DEV, window=L)
    assert len(want) == len(ld) and len(want) >= 80
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
    assert ds.uploads == 1


# ------------------------------------------------------------------------------------------------ training

FLAGS = ["--arch-sparse-feature-size=16", "--arch-mlp-bot=13-32-16", "--arch-mlp-top=32-1", "--mini-batch-size=16",
         "--lookahead=4", "--cache-size=40", "--num-ways=4", "--loss-function=bce", "--round-targets=True",
         "--learning-rate=0.1", "--lr-embeds=0.3", "--print-freq=1", "--numpy-rand-seed=4321", "--table-agg-freq=5",
         "--data-generation=dataset", "--data-set=kaggle", "--max-ind-range=50"]
N_TRAIN = 11        # 177 training rows in batches of 16, the short last batch dropped: windows of 4 + 4 + 3


def _data_flags(d):
    return ["--raw-data-file=" + os.path.join(d, "train.txt"),
            "--processed-data-file=" + os.path.join(d, "kaggleAdDisplayChallenge_processed.npz")]


def _losses(out):
    return [float(x) for x in re.findall(r"Loss = ([0-9.eE+-]+),", out)]


def _compare_runs(outs, tags, world):
    losses = {k: _losses(o) for k, o in outs.items()}
    assert len(losses["host"]) == len(losses["device"]) == N_TRAIN - 1, outs["device"][-2000:]
    rel = np.abs(np.array(losses["device"]) - np.array(losses["host"])) / np.abs(np.array(losses["host"]))
    print("world %d: largest relative loss deviation device vs host loader: %.3g" % (world, rel.max()))
    assert rel.max() <= 1e-5
    for what in (r"Test accuracy = .*", r"Test AUC = .*"):
        seen = {k: re.findall(what, o) for k, o in outs.items()}
        assert len(seen["host"]) >= 1 and seen["host"] == seen["device"]
    assert "DeviceProcessedLoader (device) reads" in outs["device"] and "ProcessedLoader (host) reads" in outs["host"]
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


def _oracle_losses(g, seed):
    """The oracle trainer fed the REFERENCE's batches of the fixture (total order, --max-ind-range=50), on the host tables the
    CLI starts from; the losses as the CLI prints them (the first line averages iterations 0 and 1)."""
    from cdlrm_amd.hostmem import make_host_tables
    from oracle import cdlrm_oracle as O
    ln_emb = np.minimum(g["counts"], 50)
    m_spa, B, L = 16, int(g["B"]), 4
    ln_bot = np.array([13, 32, 16])
    nf = len(ln_emb) + 1
    ln_top = np.array([m_spa + nf * (nf - 1) // 2, 32, 1])
    host = make_host_tables(ln_emb, m_spa, device=torch.device(DEV), seed=seed)
    torch.set_num_threads(1)
    otr = O.OracleTrainer([int(n) for n in ln_emb], m_spa, ln_bot, ln_top, cache_size=40, num_ways=4, mini_batch_size=B,
                          lr=0.1, lr_embeds=0.3, lookahead=L, table_agg_freq=5, seed=seed,
                          host_tables=[E.weight.data.clone() for E in host.emb_l])
    X, I, T = (torch.from_numpy(g["total_train_m50_" + k]) for k in ("X", "lS_i", "T"))
    batches = [(X[j * B:(j + 1) * B], I[:, j * B:(j + 1) * B], T[j * B:(j + 1) * B]) for j in range(N_TRAIN)]
    lS_o = torch.arange(B).repeat(len(ln_emb), 1)
    for j, (Xj, Ij, Tj) in enumerate(batches):
        if j % L == 0:
            otr.refill(torch.cat([b[1] for b in batches[j:j + L]], dim=1))
        otr.step(j, Xj, lS_o, Ij, Tj)
    want = np.array([l[0] for l in otr.losses])
    return np.concatenate([[(want[0] + want[1]) / 2], want[2:]])


@pytest.mark.parametrize("extra", [["--device-rng"], []], ids=["lookahead-plan", "plan-at-boundary"])
def test_cli_device_loader_trains_like_the_host_loader(golden, tmp_path, capsys, monkeypatch, keep_current_stream, extra):
    from cdlrm_amd import main_no_ddp
    g = golden("criteo_processed")
    _files(g, str(tmp_path))
    outs, tags = {}, {}
    for mode in ("host", "device"):
        tags[mode] = os.path.join(tmp_path, "tags_" + mode)
        monkeypatch.setenv("CDLRM_DUMP_TAGS", tags[mode])
        main_no_ddp.main(FLAGS + extra + ["--world-size=1", "--day-file-loader=" + mode] + _data_flags(str(tmp_path)))
        outs[mode] = capsys.readouterr().out
    _compare_runs(outs, tags, 1)
    if not extra:
        # parity mode: the way choices are the reference's draws, so the oracle trainer on the reference's batches gives the run
        want = _oracle_losses(g, 4321)
        got = np.array(_losses(outs["host"]))
        print("largest relative loss deviation host loader vs oracle: %.3g" % (np.abs(got - want) / np.abs(want)).max())
        np.testing.assert_allclose(got, want, rtol=1e-5)


def test_cli_device_loader_world_size_2(golden, tmp_path):
    """Two ranks emulated on one GPU (CDLRM_BENCH_EMULATE=1, as tests/test_self_launch.py): every rank draws the same order,
    keeps its own resident copy, cuts whole windows and trains its column slice."""
    g = golden("criteo_processed")
    _files(g, str(tmp_path))
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
                           ["--world-size=2", "--table-agg-freq=3", "--test-freq=6", "--device-rng", "--data-randomize=day",
                            "--day-file-loader=" + mode] + _data_flags(str(tmp_path)),
                           env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
        assert p.returncode == 0, p.stderr[-3000:]
        outs[mode] = p.stdout
    _compare_runs(outs, tags, 2)
