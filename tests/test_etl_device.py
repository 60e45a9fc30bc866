"""The Criteo ETL on the device (csrc/etl.hip, cdlrm_amd/data_utils.py), every part against the restated contract
(tests/etl_restated.py) and, end to end, against what the reference wrote for the same text (tests/golden/criteo_etl.npz).
Everything is an integer: equality, no tolerance anywhere.  Malformed text is reported through the error word; nothing
here aims at a fault."""
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import etl_restated as R  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENT = -0x12345678


def _dev(raw: bytes) -> torch.Tensor:
    return torch.from_numpy(np.frombuffer(raw, dtype=np.uint8).copy()).to(DEV)


def _index(raw: bytes, pad: int = 0):
    """(starts, count) of the device's line index for raw, as numpy; pad: bytes of other text behind `length`."""
    from cdlrm_amd import ops
    text = _dev(raw + b"\n" * pad)
    starts = torch.full((len(raw) + 2,), SENT, dtype=torch.int64, device=DEV)
    st, count = ops.etl_line_index(text, len(raw), starts)
    n = int(count.item())
    got = st.cpu().numpy()
    assert (got[n + 1:] == SENT).all(), "nothing is written behind starts[count]"
    return got[:n + 1], n


def _parse(raw: bytes, mir: int = -1, line0: int = 0):
    """raw through line index + parse -> (y, x_int, x_cat, error, n, tail offset)."""
    from cdlrm_amd import ops
    text = _dev(raw)
    starts, count = ops.etl_line_index(text, len(raw))
    n = int(count.item())
    y = torch.full((n + 1,), SENT, dtype=torch.int32, device=DEV)
    x_int = torch.full((n + 1, 13), SENT, dtype=torch.int32, device=DEV)
    x_cat = torch.full((n + 1, 26), SENT, dtype=torch.int32, device=DEV)
    err = ops.etl_error_word(DEV)
    ops.etl_parse(text, len(raw), starts, n, line0, mir, y, x_int, x_cat, err)
    found = ops.etl_error(err)
    y, x_int, x_cat = y.cpu().numpy(), x_int.cpu().numpy(), x_cat.cpu().numpy()
    assert y[n] == SENT and (x_int[n] == SENT).all() and (x_cat[n] == SENT).all(), "row n is not written"
    return y[:n], x_int[:n], x_cat[:n], found, n, int(starts[n].item())


def _line(**fields):
    f = ["1"] + [str(k) for k in range(13)] + ["%x" % (k + 1) for k in range(26)]
    for k, v in fields.items():
        f[int(k[1:])] = v
    return "\t".join(f).encode()


# ---- line index -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257])
def test_line_index_counts(n):
    rng = np.random.RandomState(n)
    raw = b"".join(b"x" * int(k) + b"\n" for k in rng.randint(0, 40, size=n)) + b"tail\twithout newline"
    starts, count = _index(raw)
    want, want_n = R.line_starts(raw)
    assert count == want_n == n and np.array_equal(starts, want)
    # the bytes behind `length` belong to another chunk: they are not looked at
    starts, count = _index(raw, pad=33)
    assert count == n and np.array_equal(starts, want)


def test_line_index_at_workgroup_and_lane_edges():
    """A workgroup spans 4096 bytes, a lane 16: newlines as the last byte of a span and the first of the next, of a lane and the
    next, two in a row, at byte 0 and as the last byte; a length that is no multiple of 16."""
    for at in ([4095], [4096], [4095, 4096], [0], [15, 16], [0, 1, 2], [4095, 4096, 8191, 8192, 8200], [12287 + 5]):
        buf = bytearray(b"a" * (3 * 4096 + 6))
        for p in at:
            buf[p] = 10
        starts, count = _index(bytes(buf))
        want, n = R.line_starts(bytes(buf))
        assert count == n == len(at) and np.array_equal(starts, want), at
    for length in (1, 15, 16, 17, 4095, 4096, 4097):
        raw = (b"ab\n" * 1400)[:length]
        starts, count = _index(raw, pad=7)
        want, n = R.line_starts(raw)
        assert count == n and np.array_equal(starts, want), length


def test_line_index_chunk_ends(golden):
    g = golden("criteo_etl")
    raw = g["tb_raw_0"].tobytes()
    first_nl = raw.index(b"\n")
    a_tab = [p for p, c in enumerate(raw) if c == 9][45]                       # a tab of the second line (39 in the first)
    in_field = next(p for p in range(first_nl + 2, len(raw)) if raw[p - 1] not in (9, 10) and raw[p] not in (9, 10))
    cuts = {"right after a newline": first_nl + 1, "in the middle of a field": in_field, "right behind a tab": a_tab + 1,
            "no newline": first_nl, "empty": 0}
    assert raw[cuts["right behind a tab"] - 1] == 9 and first_nl < a_tab < raw.index(b"\n", first_nl + 1) and in_field < a_tab + 400
    for what, c in cuts.items():
        starts, count = _index(raw[:c])
        want, n = R.line_starts(raw[:c])
        assert count == n and np.array_equal(starts, want), what
        assert count == (0 if what in ("no newline", "empty") else 1) and starts[-1] == (first_nl + 1 if count else 0)


# ---- parse ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mir", [-1, 10])
def test_parse_equals_the_restated_parser_whole_and_cut(golden, mir):
    g = golden("criteo_etl")
    raw = g["kaggle_raw"].tobytes() + b"\n"
    lines = R.split_lines(raw)
    want = R.parse_lines(lines, mir)
    assert not want[3]
    y, x_int, x_cat, found, n, tail = _parse(raw, mir)
    assert found is None and n == len(lines) == 75 and tail == len(raw)
    assert np.array_equal(y, want[0]) and np.array_equal(x_int, want[1]) and np.array_equal(x_cat, want[2])
    assert x_int.min() == 0 and any(b"\t-" in l for l in lines)              # negatives were there and are clamped
    # cut at every kind of chunk edge: the first chunk's lines, then the carry + the rest, give the arrays of the uncut text
    nl = [p for p, c in enumerate(raw) if c == 10]
    tabs = [p for p, c in enumerate(raw) if c == 9]
    cuts = [nl[4] + 1, nl[4] + 9, next(t for t in tabs if t > nl[9]) + 1, nl[0] - 3, nl[-1], 4096, 4097]
    for c in cuts:
        a = _parse(raw[:c], mir)
        b = _parse(raw[a[5]:], mir, line0=a[4])
        assert a[3] is None and b[3] is None and a[4] + b[4] == 75, c
        for k in range(3):
            assert np.array_equal(np.concatenate([a[k], b[k]]), want[k]), (c, k)


def test_parse_wrap_values():
    raw = _line(f14="7fffffff", f15="80000000", f16="ffffffff", f39="FFFFFFFE") + b"\n" + _line(f14="ffffffff", f15="80000000") + b"\n"
    for mir in (-1, 10, 2 ** 31, 2 ** 32 + 5):
        y, x_int, x_cat, found, n, _ = _parse(raw, mir)
        want = R.parse_lines(R.split_lines(raw), mir)
        assert found is None and n == 2 and np.array_equal(x_cat, want[2]) and np.array_equal(x_int, want[1]), mir
    x_cat = _parse(raw)[2]
    assert x_cat[0, :3].tolist() == [2 ** 31 - 1, -2 ** 31, -1] and x_cat[0, 25] == -2


MALFORMED = [
    (b"\t".join([b"1"] * 39), R.ERR_FIELDS), (b"\t".join([b"1"] * 41), R.ERR_FIELDS), (b"", R.ERR_FIELDS),
    (_line(f3="-"), R.ERR_DEC_BYTE), (_line(f3="+1"), R.ERR_DEC_BYTE), (_line(f5="\xff"), R.ERR_DEC_BYTE),
    (_line(f3="9" * 300), R.ERR_DEC_RANGE), (_line(f0="-2147483649"), R.ERR_DEC_RANGE),
    (_line(f20="123456789"), R.ERR_HEX_LONG), (_line(f20="f" * 300), R.ERR_HEX_LONG),
    (_line(f20="0x12"), R.ERR_HEX_BYTE), (_line(f39="ab\r"), R.ERR_HEX_BYTE), (_line(f20="12345678g"), R.ERR_HEX_BYTE)]


@pytest.mark.parametrize("k", range(len(MALFORMED)))
def test_a_malformed_line_is_reported_and_its_neighbours_are_parsed(k, tmp_path):
    from cdlrm_amd import data_utils as DU
    bad, code = MALFORMED[k]
    assert R.parse_line(bad)[0] == code
    good = [_line(f1=str(j), f14="%x" % (j * 77)) for j in range(70)]
    lines = good[:66] + [bad] + good[66:]                                      # line 67: in the second wave of the launch
    raw = b"\n".join(lines) + b"\n"
    y, x_int, x_cat, found, n, _ = _parse(raw, line0=1000)
    want = R.parse_lines(lines)
    assert found == (1067, code) and want[3] == [(67, code)] and n == 71
    assert np.array_equal(y, want[0]) and np.array_equal(x_int, want[1]) and np.array_equal(x_cat, want[2])
    assert y[66] == 0 and not x_int[66].any() and not x_cat[66].any()
    # two bad lines: the first one is reported, whichever lane got there first
    raw2 = b"\n".join([good[0], _line(f20="g"), good[1], bad]) + b"\n"
    assert _parse(raw2)[3] == (2, R.ERR_HEX_BYTE)
    # ... and the ETL names file and line
    path = os.path.join(str(tmp_path), "day_0")
    with open(path, "wb") as f:
        f.write(raw)
    with pytest.raises(ValueError, match=re.escape(path) + r": line 67 is malformed.*\(code %d\)" % code):
        DU.getCriteoAdData(os.path.join(str(tmp_path), "day"), "terabyte_processed", days=1, criteo_kaggle=False,
                           chunk_bytes=max(1024, len(bad) + 400))
    assert os.listdir(str(tmp_path)) == ["day_0"]


def test_parse_never_reads_a_span_that_is_not_in_the_text():
    """A starts array that is no line index of the text: reported (code 7), zeros written, nothing read."""
    from cdlrm_amd import ops
    raw = _line() + b"\n"
    text = _dev(raw)
    for starts in ([0, len(raw) + 50], [-5, len(raw)], [30, 20]):
        y = torch.full((1,), SENT, dtype=torch.int32, device=DEV)
        x_int, x_cat = torch.full((1, 13), SENT, dtype=torch.int32, device=DEV), torch.full((1, 26), SENT, dtype=torch.int32, device=DEV)
        err = ops.etl_error_word(DEV)
        ops.etl_parse(text, len(raw), torch.tensor(starts, dtype=torch.int64, device=DEV), 1, 0, -1, y, x_int, x_cat, err)
        assert ops.etl_error(err) == (1, 7) and int(y[0]) == 0 and not x_int.any() and not x_cat.any()


# ---- sub-sample -------------------------------------------------------------------------------------------------------------

def _subsample(y, x_int, x_cat, rand_u, line0, rate, out, rows_in):
    from cdlrm_amd import ops
    t = [torch.from_numpy(a).to(DEV) for a in (y, x_int, x_cat)]
    rows = [torch.tensor([rows_in], dtype=torch.int64, device=DEV), torch.full((1,), SENT, dtype=torch.int64, device=DEV)]
    ops.etl_subsample(t[0], t[1], t[2], len(y), rand_u, line0, rate, out[0], out[1], out[2], rows[0], rows[1])
    assert int(rows[0].item()) == rows_in
    return int(rows[1].item())


@pytest.mark.parametrize("n", [1, 256, 257])
@pytest.mark.parametrize("labels", ["ones", "zeros", "alternating", "random"])
def test_subsample_compacts_stably(n, labels):
    rng = np.random.RandomState(n)
    y = {"ones": np.ones(n), "zeros": np.zeros(n), "alternating": np.arange(n) % 2, "random": rng.randint(0, 3, size=n)}[labels]
    y = y.astype(np.int32)
    x_int = rng.randint(0, 2 ** 31 - 1, size=(n, 13)).astype(np.int32)
    x_cat = rng.randint(-2 ** 31, 2 ** 31 - 1, size=(n, 26)).astype(np.int32)
    u = rng.uniform(size=n + 9)
    line0, rows_in = 9, 5
    for rate in (1.0, 0.5):
        keep = R.keep_mask(y, u[line0:], rate)
        out = [torch.full((n + 6,) + s, SENT, dtype=torch.int32, device=DEV) for s in ((), (13,), (26,))]
        rows_out = _subsample(y, x_int, x_cat, torch.from_numpy(u).to(DEV), line0, rate, out, rows_in)
        kept = int(keep.sum())
        assert rows_out == rows_in + kept
        if labels == "ones":
            assert kept == n
        if labels == "zeros" and rate == 1.0:
            assert kept == 0
        for got, src in zip(out, (y, x_int, x_cat)):
            got = got.cpu().numpy()
            assert np.array_equal(got[rows_in:rows_in + kept], src[keep]), (labels, rate)
            assert (got[:rows_in] == SENT).all() and (got[rows_in + kept:] == SENT).all()


def test_subsample_indexes_rand_u_by_the_file_line_across_chunks():
    rng = np.random.RandomState(8)
    n = 300
    y = (rng.rand(n) < 0.3).astype(np.int32)
    x_int = rng.randint(0, 1000, size=(n, 13)).astype(np.int32)
    x_cat = rng.randint(0, 1000, size=(n, 26)).astype(np.int32)
    u = rng.uniform(size=n)
    keep = R.keep_mask(y, u, 0.6)
    out = [torch.full((n,) + s, SENT, dtype=torch.int32, device=DEV) for s in ((), (13,), (26,))]
    ud = torch.from_numpy(u).to(DEV)
    cut = 130
    mid = _subsample(y[:cut], x_int[:cut], x_cat[:cut], ud, 0, 0.6, out, 0)
    end = _subsample(y[cut:], x_int[cut:], x_cat[cut:], ud, cut, 0.6, out, mid)
    assert mid == int(keep[:cut].sum()) and end == int(keep.sum()) and 0 < end < n
    for got, src in zip(out, (y, x_int, x_cat)):
        assert np.array_equal(got.cpu().numpy()[:end], src[keep])


# ---- encode -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("m", [1, 2, 255, 256, 257])
def test_encode_by_binary_search(m):
    from cdlrm_amd import ops
    rng = np.random.RandomState(m)
    keys = np.unique(np.concatenate([rng.randint(-2 ** 31, 2 ** 31 - 1, size=m * 2), [-2 ** 31, 2 ** 31 - 1, -1, 0]]).astype(np.int32))
    keys = np.sort(rng.permutation(keys)[:m]) if m > 2 else np.array([-2 ** 31, 2 ** 31 - 1][:m], dtype=np.int32)
    assert keys.size == m and keys[0] < 0
    ids = rng.permutation(m).astype(np.int32)
    n = 300
    x = rng.randint(0, 99, size=(n, 26)).astype(np.int32)
    col = 5
    x[:, col] = keys[rng.randint(0, m, size=n)]
    x[0, col], x[n - 1, col] = keys[0], keys[-1]
    want = x.copy()
    want[:, col] = ids[np.searchsorted(keys, x[:, col])]
    xd, err = torch.from_numpy(x).to(DEV), ops.etl_error_word(DEV)
    ops.etl_encode(xd, col, torch.from_numpy(keys).to(DEV), torch.from_numpy(ids).to(DEV), err)
    assert ops.etl_error(err) is None and np.array_equal(xd.cpu().numpy(), want)
    # rows behind n stay as they are
    xd = torch.from_numpy(x).to(DEV)
    ops.etl_encode(xd, col, torch.from_numpy(keys).to(DEV), torch.from_numpy(ids).to(DEV), err, n=n - 7)
    assert np.array_equal(xd.cpu().numpy()[n - 7:], x[n - 7:]) and np.array_equal(xd.cpu().numpy()[:n - 7], want[:n - 7])
    # a value the table does not hold: the first such row is reported
    missing = next(v for v in (7, 8, 9, -7, 12345) if v not in set(keys.tolist()))
    x2 = x.copy()
    x2[[40, 290], col] = missing
    xd = torch.from_numpy(x2).to(DEV)
    ops.etl_encode(xd, col, torch.from_numpy(keys).to(DEV), torch.from_numpy(ids).to(DEV), err, row0=1000)
    assert ops.etl_error(err) == (1041, R.ERR_NOT_IN_DICT)
    got = xd.cpu().numpy()
    keep = np.ones(n, bool)
    keep[[40, 290]] = False
    assert np.array_equal(got[keep], want[keep]) and got[40, col] == 0


def test_dictionary_extension_gives_first_appearance_ids():
    from cdlrm_amd.data_utils import _Dictionary
    rng = np.random.RandomState(1)
    d, seen, base = _Dictionary(DEV), {}, 0
    for n in (50, 0, 1, 300):
        vals = rng.randint(-20, 20, size=n).astype(np.int32) * 100000007
        d.extend(torch.from_numpy(vals).to(DEV), base)
        for v in vals.tolist():
            seen.setdefault(v, len(seen))
        base += n
        keys, ids = d.keys.cpu().numpy(), d.ids().cpu().numpy()
        assert np.array_equal(keys, np.sort(np.array(list(seen), dtype=np.int32))) and [seen[k] for k in keys.tolist()] == ids.tolist()
        assert d.unique().tolist() == list(seen)


# ---- end to end -------------------------------------------------------------------------------------------------------------

def _check_outputs(g, tag, d, d_file, npzfile, o_file, days):
    with np.load(os.path.join(d, d_file + "_day_count.npz")) as z:
        assert np.array_equal(z["total_per_file"], g[tag + "_total_per_file"]) and z["total_per_file"].dtype == np.int64
    for j in range(26):
        with np.load(os.path.join(d, d_file + "_fea_dict_%d.npz" % j)) as z:
            assert z["unique"].dtype == np.int32 and np.array_equal(z["unique"], g["%s_unique_%d" % (tag, j)]), j
    with np.load(os.path.join(d, d_file + "_fea_count.npz")) as z:
        assert z["counts"].dtype == np.int32 and np.array_equal(z["counts"], g[tag + "_counts"])
    for i in range(days):
        with np.load(npzfile + "_%d_processed.npz" % i) as z:
            assert sorted(z.files) == ["X_cat", "X_int", "y"] and z["X_cat"].dtype == z["X_int"].dtype == z["y"].dtype == np.int32
            for k in ("X_cat", "X_int", "y"):
                assert np.array_equal(z[k], g["%s_day%d_%s" % (tag, i, k)].astype(np.int32)), (i, k)
    with np.load(o_file) as z:
        assert sorted(z.files) == ["X_cat", "X_int", "counts", "y"] and z["X_cat"].dtype == np.int32
        for k in ("X_cat", "X_int", "y", "counts"):
            assert z[k].dtype == np.int32 and np.array_equal(z[k], g["%s_all_%s" % (tag, k)].astype(np.int32)), k


@pytest.mark.parametrize("tag", ["k_r0_m0", "k_r5_m0", "k_r0_m10"])
def test_etl_kaggle_writes_what_the_reference_wrote(golden, tmp_path, tag):
    from cdlrm_amd import data_utils as DU
    g = golden("criteo_etl")
    d = str(tmp_path)
    raw = os.path.join(d, "train.txt")
    with open(raw, "wb") as f:
        f.write(g["kaggle_raw"].tobytes())
    np.random.seed(int(g["seed"]))
    o = DU.getCriteoAdData(raw, "kaggleAdDisplayChallenge_processed", int(g[tag + "_max_ind_range"]), float(g[tag + "_rate"]), 7,
                           chunk_bytes=700)
    assert o == os.path.join(d, "kaggleAdDisplayChallenge_processed.npz")
    _check_outputs(g, tag, d, "train", os.path.join(d, "train_day"), o, 7)
    assert not os.path.exists(os.path.join(d, "train_day_0")) and not os.path.exists(os.path.join(d, "train_day_0.npz"))
    assert len(os.listdir(d)) == 1 + 1 + 26 + 1 + 7 + 1
    # a second call refuses the outputs of the first; forced (and stored, one big chunk) it writes the same arrays again
    with pytest.raises(FileExistsError, match="train_day_count.npz"):
        DU.getCriteoAdData(raw, "kaggleAdDisplayChallenge_processed", chunk_bytes=700)
    np.random.seed(int(g["seed"]))
    DU.getCriteoAdData(raw, "kaggleAdDisplayChallenge_processed", int(g[tag + "_max_ind_range"]), float(g[tag + "_rate"]), 7,
                       force=True, store=True)
    _check_outputs(g, tag, d, "train", os.path.join(d, "train_day"), o, 7)


def test_etl_terabyte_and_the_command_line(golden, tmp_path, capsys):
    from cdlrm_amd import data_utils as DU
    g = golden("criteo_etl")
    d = str(tmp_path)
    for i in range(3):
        with open(os.path.join(d, "day_%d" % i), "wb") as f:
            f.write(g["tb_raw_%d" % i].tobytes())
    o = DU.main(["--raw-data-file=" + os.path.join(d, "day"), "--processed-data-file=" + os.path.join(d, "terabyte_processed.npz"),
                 "--data-set=terabyte", "--days=3", "--chunk-bytes=512"])
    assert o == os.path.join(d, "terabyte_processed.npz") and ("Wrote " + o) in capsys.readouterr().out
    _check_outputs(g, "tb", d, "day", os.path.join(d, "day"), o, 3)
    with pytest.raises(SystemExit) as e:
        DU.main(["--raw-data-file=" + os.path.join(d, "day"), "--data-set=terabyte", "--days=3"])
    assert str(e.value).startswith("ERROR: ") and "exists" in str(e.value) and "\n" not in str(e.value)
    # memory_map: the per-day files, one printed line, no concatenation
    os.remove(o)
    DU.main(["--raw-data-file=" + os.path.join(d, "day"), "--data-set=terabyte", "--days=3", "--memory-map", "--force"])
    assert "memory_map: stopping after the per-day processed files" in capsys.readouterr().out and not os.path.exists(o)
    # a line longer than the chunk capacity is a refusal, not a hang
    with pytest.raises(ValueError, match="longer than the chunk capacity"):
        DU.getCriteoAdData(os.path.join(d, "day"), "terabyte_processed", days=3, criteo_kaggle=False, force=True, chunk_bytes=64)


def test_etl_wrapped_hashes_and_later_days_against_the_restated_etl(tmp_path):
    """What the reference cannot produce: hashes >= 2^31 as dictionary keys, through sub-sampling, ids across days."""
    from cdlrm_amd import data_utils as DU
    rng = np.random.RandomState(77)
    pool = ["ffffffff", "80000000", "7fffffff", "0", "deadBEEF", "1", "cafe", "FFFFFFFE"]
    days = []
    for n in (40, 3, 300):
        days.append([_line(f0=str(int(rng.rand() < 0.4)), f1=str(int(rng.randint(-5, 50))),
                           **{"f%d" % (14 + j): pool[rng.randint(0, 2 + (j * len(days)) % 7)] for j in range(26)}) for _ in range(n)])
    d = str(tmp_path)
    for i, lines in enumerate(days):
        with open(os.path.join(d, "day_%d" % i), "wb") as f:
            f.write(b"\n".join(lines) + (b"\n" if i != 1 else b""))
    np.random.seed(11)
    want = R.etl(days, sub_sample_rate=0.7)
    np.random.seed(11)
    o = DU.getCriteoAdData(os.path.join(d, "day"), "terabyte_processed", -1, 0.7, 3, criteo_kaggle=False, chunk_bytes=2048)
    with np.load(o) as z:
        for k in ("X_cat", "X_int", "y", "counts"):
            assert z[k].dtype == np.int32 and np.array_equal(z[k], want[k]), k
    assert want["X_cat"].shape[0] < 343 and min(int(u.min()) for u in want["unique"]) == -2 ** 31
    for j in range(26):
        with np.load(os.path.join(d, "day_fea_dict_%d.npz" % j)) as z:
            assert np.array_equal(z["unique"], want["unique"][j])
    with np.load(os.path.join(d, "day_day_count.npz")) as z:
        assert np.array_equal(z["total_per_file"], want["total_per_file"])


def test_etl_refuses_what_does_not_fit_before_it_allocates(golden, tmp_path, monkeypatch):
    from cdlrm_amd import data_utils as DU
    g = golden("criteo_etl")
    raw = os.path.join(str(tmp_path), "train.txt")
    with open(raw, "wb") as f:
        f.write(g["kaggle_raw"].tobytes())
    monkeypatch.setattr(DU, "_device_free_bytes", lambda device: 5000)
    monkeypatch.setattr(DU, "_Ring", None)                                     # an allocation would fail loudly
    rows, ring, dictionary = DU._day_bytes(11, 700, False, 0)
    with pytest.raises(ValueError, match=r"%d bytes of parsed rows \(11 lines\) \+ %d of text chunk ring \+ %d of dictionary = %d, 5000 free"
                       % (rows, ring, dictionary, rows + ring + dictionary)):
        DU.getCriteoAdData(raw, "kaggleAdDisplayChallenge_processed", chunk_bytes=700)
    assert os.listdir(str(tmp_path)) == ["train.txt"]


@pytest.fixture()
def keep_current_stream():
    """`main_no_ddp.Run` makes a stream of its own the thread's current one; later tests expect the one they started on."""
    before = torch.cuda.current_stream()
    yield
    torch.cuda.synchronize()
    torch.cuda.set_stream(before)


def test_the_written_file_feeds_the_processed_loader_and_a_training_run(golden, tmp_path, capsys, keep_current_stream):
    from cdlrm_amd import data_utils as DU
    from cdlrm_amd import main_no_ddp
    from cdlrm_amd.data_loader_processed import ProcessedDataset
    g = golden("criteo_etl")
    d = str(tmp_path)
    raw = os.path.join(d, "train.txt")
    with open(raw, "wb") as f:
        f.write(g["kaggle_raw"].tobytes())
    o = DU.getCriteoAdData(raw, "kaggleAdDisplayChallenge_processed", chunk_bytes=700)
    with np.load(os.path.join(d, "train_day_count.npz")) as z:
        ds = ProcessedDataset(o, z["total_per_file"])
    assert len(ds) == 75 and (ds.m_den, ds.n_emb) == (13, 26) and np.array_equal(ds.X_cat, g["k_r0_m0_all_X_cat"].astype(np.int32))
    assert np.array_equal(ds.counts, g["k_r0_m0_counts"])
    capsys.readouterr()
    main_no_ddp.main(["--arch-sparse-feature-size=16", "--arch-mlp-bot=13-32-16", "--arch-mlp-top=32-1", "--mini-batch-size=8",
                      "--lookahead=4", "--cache-size=40", "--num-ways=4", "--loss-function=bce", "--round-targets=True",
                      "--learning-rate=0.1", "--lr-embeds=0.3", "--print-freq=1", "--numpy-rand-seed=4321", "--table-agg-freq=5",
                      "--data-generation=dataset", "--data-set=kaggle", "--max-ind-range=50", "--world-size=1",
                      "--raw-data-file=" + raw, "--processed-data-file=" + o])
    out = capsys.readouterr().out
    losses = [float(x) for x in re.findall(r"Loss = ([0-9.eE+-]+),", out)]
    assert len(losses) >= 4 and all(np.isfinite(losses)) and all(0.0 < l < 5.0 for l in losses), out[-2000:]
