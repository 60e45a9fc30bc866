"""The MLPerf binary Criteo files on the host: `CriteoBinDataset` / `BinLoader` against what the reference's own class and
torch's DataLoader gave for the same file bytes (tests/golden/criteo_bin.npz, tools/make_golden_bin.py), `bin_extents`
against the loader, the refusals, and the CLI's `ERROR:` line when the files the flag names are missing.  No GPU.

Bounds (tests/test_dayfile_device.py): indices, targets and offsets are integers, equal bit for bit; X = log(x + 1) at most
1 ulp from float32(log(float64(float32(x) + float32(1)))) and at most 2 ulp from the reference's torch.log."""
import os

import numpy as np
import pytest
import torch

from cdlrm_amd.data_loader_terabyte import BinLoader, CriteoBinDataset, bin_extents, transform_features


def _ordered(a):
    i = np.ascontiguousarray(a, dtype=np.float32).view(np.int32).astype(np.int64)
    return np.where(i < 0, -(i & 0x7fffffff), i)


def _ulp(a, b) -> int:
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    assert a.shape == b.shape and np.all(np.isfinite(a)) and np.all(np.isfinite(b))
    return int(np.abs(_ordered(a) - _ordered(b)).max()) if a.size else 0


def _log_exact(x_int):
    return np.log((x_int.astype(np.float32) + np.float32(1)).astype(np.float64)).astype(np.float32)


def write_bin(path, x_int, x_cat, y):
    """records [y | dense | categorical] of int32, as the binary file stores them"""
    rec = np.concatenate([np.asarray(y).reshape(-1, 1), x_int, x_cat], axis=1).astype(np.int32)
    with open(path, "wb") as f:
        f.write(rec.tobytes())
    return rec


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


def _check(batches, g, name, exact):
    assert [b[3].shape[0] for b in batches] == g[name + "_sizes"].tolist()
    assert torch.equal(torch.cat([b[2] for b in batches], dim=1), torch.from_numpy(g[name + "_lS_i"]))
    assert torch.equal(torch.cat([b[3] for b in batches]), torch.from_numpy(g[name + "_T"]))
    assert torch.equal(batches[-1][1], torch.from_numpy(g[name + "_lS_o_last"]))
    for X, lS_o, lS_i, T in batches:
        n = T.shape[0]
        assert X.dtype == torch.float32 and X.shape == (n, 13) and T.dtype == torch.float32 and T.shape == (n, 1)
        assert lS_i.dtype == torch.int64 and lS_i.shape == (26, n)
        assert torch.equal(lS_o, torch.arange(n).repeat(26, 1))
    X = torch.cat([b[0] for b in batches]).numpy()
    assert _ulp(X, exact) <= 1 and _ulp(X, g[name + "_X"]) <= 2


def test_writer_of_this_file_writes_the_reference_bytes(golden, tmp_path):
    g = golden("criteo_bin")
    days = [(g["xi_%d" % d], g["xc_%d" % d], g["y_%d" % d]) for d in range(3)]
    write_bin(str(tmp_path / "t.bin"), *(np.concatenate([d[i] for d in days]) for i in range(3)))
    assert open(tmp_path / "t.bin", "rb").read() == g["train_bytes"].tobytes()
    half = int(np.ceil(days[2][2].shape[0] / 2.))
    write_bin(str(tmp_path / "v.bin"), *(a[half:] for a in days[2]))
    assert open(tmp_path / "v.bin", "rb").read() == g["val_bytes"].tobytes()


@pytest.mark.parametrize("mir", [50, -1])
@pytest.mark.parametrize("split", ["train", "test", "val"])
def test_bin_dataset_matches_reference(golden, tmp_path, split, mir):
    g = golden("criteo_bin")
    files, counts = _golden_files(g, str(tmp_path))
    B = int(g["B"])
    name = "%s_m%d" % (split, mir if mir > 0 else 0)
    ds = CriteoBinDataset(files[split], counts, batch_size=B, max_ind_range=mir)
    assert len(ds) == int(g[name + "_len"]) and ds.counts.tolist() == [100000] * 26
    exact = _log_exact(_dense_of(g[split + "_bytes"]))
    _check([ds[i] for i in range(len(ds))], g, name, exact)
    ld = BinLoader(ds)
    assert len(ld) == len(ds)
    for epoch in range(2):
        _check(list(ld), g, name, exact)
    if mir > 0:
        I = torch.cat([b[2] for b in ld], dim=1)
        assert int(I.min()) >= 0 and int(I.max()) < mir         # the golden holds negative entries: floor-mod
    with pytest.raises(IndexError):
        ds[len(ds)]


def test_bin_loader_shuffle_is_torchs_random_sampler(golden, tmp_path):
    g = golden("criteo_bin")
    files, counts = _golden_files(g, str(tmp_path))
    ds = CriteoBinDataset(files["train"], counts, batch_size=int(g["B"]), max_ind_range=50)
    ld = BinLoader(ds, shuffle=True)
    torch.manual_seed(int(g["seed"]))
    dense = _dense_of(g["train_bytes"])
    for epoch in range(2):
        order = g["shuffle_e%d_order" % epoch].tolist()
        batches = list(ld)
        # the entry order, read off the batches themselves: every entry's targets + indices are unlike any other's
        want = [ds[i] for i in order]
        assert len(batches) == len(order) == len(ds)
        for b, w in zip(batches, want):
            assert torch.equal(b[2], w[2]) and torch.equal(b[3], w[3])
        exact = _log_exact(np.concatenate([dense[i * 7:(i + 1) * 7] for i in order]))
        _check(batches, g, "shuffle_e%d" % epoch, exact)
    assert g["shuffle_e0_order"].tolist() != g["shuffle_e1_order"].tolist()     # a fresh permutation per epoch
    assert sorted(g["shuffle_e0_order"].tolist()) == list(range(len(ds)))


def test_bin_loader_drop_last_batch(golden, tmp_path):
    """the CLI's training loader: the short entry is left out wherever the permutation has it"""
    g = golden("criteo_bin")
    files, counts = _golden_files(g, str(tmp_path))
    ds = CriteoBinDataset(files["train"], counts, batch_size=7, max_ind_range=50)
    ld = BinLoader(ds, shuffle=True, drop_last_batch=True)
    torch.manual_seed(int(g["seed"]))
    got = list(ld)
    order = [i for i in g["shuffle_e0_order"].tolist() if i != 7]
    assert len(ld) == len(got) == 7 and all(b[3].shape[0] == 7 for b in got)
    assert all(torch.equal(b[2], ds[i][2]) for b, i in zip(got, order))
    ds6 = CriteoBinDataset(files["train"], counts, batch_size=6, max_ind_range=50)      # 54 = 9 * 6: nothing to drop
    assert len(BinLoader(ds6, drop_last_batch=True)) == len(list(BinLoader(ds6, drop_last_batch=True))) == 9


def test_bin_extents_against_golden_and_loader(golden, tmp_path):
    g = golden("criteo_bin")
    assert [n for _, n in bin_extents(54, 7)] == g["train_m50_sizes"].tolist()
    assert [n for _, n in bin_extents(9, 7)] == g["test_m50_sizes"].tolist()
    assert [n for _, n in bin_extents(8, 7)] == g["val_m50_sizes"].tolist()
    order = g["shuffle_e0_order"].tolist()
    assert [n for _, n in bin_extents(54, 7, order)] == g["shuffle_e0_sizes"].tolist()
    assert bin_extents(54, 7, order)[0] == (order[0] * 7, 7)
    assert bin_extents(0, 7) == []
    with pytest.raises(IndexError):
        bin_extents(54, 7, [8])
    rng = np.random.RandomState(4)
    counts = str(tmp_path / "c.npz")
    np.savez(counts, counts=np.arange(1, 4))
    cases = [(3, 5), (1, 1), (10, 10), (20, 5), (21, 5), (19, 5), (1, 2)]
    cases += [(int(k * B + e), int(B)) for B in rng.randint(1, 40, size=12) for k in (1, 3) for e in (-1, 0, 1) if k * B + e > 0]
    cases += [(int(n), int(B)) for n, B in zip(rng.randint(1, 300, size=20), rng.randint(1, 50, size=20))]
    for n, B in cases:
        rec = write_bin(str(tmp_path / "p.bin"), rng.randint(0, 99, size=(n, 13)), rng.randint(0, 99, size=(n, 3)),
                        rng.randint(0, 2, size=n))
        ds = CriteoBinDataset(str(tmp_path / "p.bin"), counts, batch_size=B)
        ext = bin_extents(n, B)
        assert len(ext) == len(ds) == len(BinLoader(ds)), (n, B)
        assert sum(k for _, k in ext) == n and all(0 < k <= B for _, k in ext)
        for (a, k), (X, lS_o, lS_i, T) in zip(ext, BinLoader(ds)):
            w = transform_features(rec[a:a + k, 1:14], rec[a:a + k, 14:], rec[a:a + k, 0], -1)
            assert torch.equal(X, w[0]) and torch.equal(lS_i, w[2]) and torch.equal(T, w[3]) and torch.equal(lS_o, w[1]), (n, B)


def test_bin_dataset_refuses_truncated_and_missing_files(golden, tmp_path):
    g = golden("criteo_bin")
    files, counts = _golden_files(g, str(tmp_path))
    cut = str(tmp_path / "cut_train.bin")
    with open(cut, "wb") as f:
        f.write(g["train_bytes"].tobytes()[:-3])
    with pytest.raises(ValueError, match="cut_train.bin"):
        CriteoBinDataset(cut, counts, batch_size=7)
    gone = str(tmp_path / "gone_train.bin")
    with pytest.raises(OSError, match="gone_train.bin"):
        CriteoBinDataset(gone, counts, batch_size=7)
    with pytest.raises(OSError, match="gone_fea_count.npz"):
        CriteoBinDataset(files["train"], str(tmp_path / "gone_fea_count.npz"), batch_size=7)


def test_cli_names_the_missing_bin_file(tmp_path, capsys):
    """--mlperf-bin-loader is no longer ignored: with only day files there, the run ends on the ERROR line that names the
    binary file (before any GPU is asked for)."""
    from cdlrm_amd import main_no_ddp
    d = str(tmp_path)
    np.savez(os.path.join(d, "day_0_reordered.npz"), X_int=np.zeros((8, 13), np.int32), X_cat=np.zeros((8, 26), np.int32),
             y=np.zeros(8, np.int32))
    np.savez(os.path.join(d, "day_day_count.npz"), total_per_file=np.array([8]))
    np.savez(os.path.join(d, "day_fea_count.npz"), counts=np.full(26, 10))
    argv = ["--data-generation=dataset", "--data-set=terabyte", "--large-batch", "--memory-map", "--mlperf-bin-loader",
            "--raw-data-file=" + os.path.join(d, "day"), "--processed-data-file=" + os.path.join(d, "terabyte_processed.npz"),
            "--arch-mlp-bot=13-8-4", "--arch-sparse-feature-size=4", "--arch-mlp-top=8-1", "--mini-batch-size=4", "--world-size=1"]
    with pytest.raises(SystemExit) as e:
        main_no_ddp.main(argv)
    msg = str(e.value.code)
    assert msg.startswith("ERROR:") and "\n" not in msg and os.path.join(d, "terabyte_processed_train.bin") in msg
