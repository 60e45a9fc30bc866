"""The Criteo ETL without a GPU: the restated contract (tests/etl_restated.py) against what the reference wrote for the same
text (tests/golden/criteo_etl.npz, tools/make_golden_etl.py), the parts of the contract the reference cannot produce (the
>= 2^31 wrap, the malformed-line codes), the refusals `getCriteoAdData` makes before it touches the device, the command
line, the ABI entries, and csrc/etl_parse.h -- the parser the kernels run -- on the CPU under AddressSanitizer and UBSan
(tools/etl_parse_check.cpp, an executable of its own run as a child process)."""
import ctypes as C
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import etl_restated as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KAGGLE_CASES = ("k_r0_m0", "k_r5_m0", "k_r0_m10")


def _check_against_fixture(g, tag, got, n_days):
    assert np.array_equal(got["total_per_file"], g[tag + "_total_per_file"])
    assert got["counts"].dtype == g[tag + "_counts"].dtype == np.int32 and np.array_equal(got["counts"], g[tag + "_counts"])
    assert np.array_equal(got["counts"], g[tag + "_all_counts"])
    for j in range(R.N_CAT):
        want = g["%s_unique_%d" % (tag, j)]
        assert got["unique"][j].dtype == want.dtype == np.int32 and np.array_equal(got["unique"][j], want), j
    assert len(got["days"]) == n_days
    for i, (x_cat, x_int, y) in enumerate(got["days"]):
        want = [g["%s_day%d_%s" % (tag, i, k)] for k in ("X_cat", "X_int", "y")]
        assert want[0].dtype == np.float64 and want[1].dtype == want[2].dtype == np.int32
        assert x_cat.dtype == x_int.dtype == y.dtype == np.int32
        assert np.array_equal(want[0], want[0].astype(np.int32))            # the cast loses nothing
        assert np.array_equal(x_cat, want[0].astype(np.int32)) and np.array_equal(x_int, want[1]) and np.array_equal(y, want[2]), i
    for k in ("X_cat", "X_int", "y"):
        assert np.array_equal(got[k], g["%s_all_%s" % (tag, k)].astype(np.int32)), k


@pytest.mark.parametrize("tag", KAGGLE_CASES)
def test_restated_etl_equals_the_reference_kaggle(golden, tag):
    g = golden("criteo_etl")
    rate, mir = float(g[tag + "_rate"]), int(g[tag + "_max_ind_range"])
    np.random.seed(int(g["seed"]))
    got = R.etl(R.kaggle_days(g["kaggle_raw"].tobytes()), mir, rate)
    _check_against_fixture(g, tag, got, 7)
    if rate > 0:
        # total_per_file holds the counts AFTER dropping (data_utils.py:1062)
        assert got["total_per_file"].sum() < 75 and (got["total_per_file"] <= np.array(R.kaggle_split(75, 7))).all()
    else:
        assert got["total_per_file"].tolist() == [11, 11, 11, 11, 11, 10, 10]


def test_restated_etl_equals_the_reference_terabyte(golden):
    g = golden("criteo_etl")
    got = R.etl([R.split_lines(g["tb_raw_%d" % i].tobytes()) for i in range(3)])
    _check_against_fixture(g, "tb", got, 3)
    assert got["total_per_file"].tolist() == [17, 1, 9]


def test_fixture_holds_the_cases_it_is_meant_to(golden):
    g = golden("criteo_etl")
    raw = g["kaggle_raw"].tobytes()
    assert not raw.endswith(b"\n")                                           # a final line without its newline
    lines = R.split_lines(raw)
    assert len(lines) == 75 and any(l.endswith(b"\t") for l in lines) and any(b"\t\t" in l for l in lines)
    assert any(b"\t-" in l for l in lines)
    assert g["k_r0_m0_counts"][7] == 1 and g["k_r0_m0_counts"].max() > 20
    assert int(g["k_r0_m0_all_X_cat"].max()) < 2 ** 31 and os.path.getsize(os.path.join(ROOT, "tests", "golden", "criteo_etl.npz")) < 100e3


def _line(**fields):
    f = ["1"] + [str(k) for k in range(13)] + ["%x" % (k + 1) for k in range(26)]
    for k, v in fields.items():
        f[int(k[1:])] = v
    return "\t".join(f).encode()


def test_wrap_values_keep_their_int32_bit_pattern():
    code, y, x_int, x_cat = R.parse_line(_line(f14="7fffffff", f15="80000000", f16="ffffffff", f39="FFFFFFFE"))
    assert code == 0 and x_cat[0] == 2 ** 31 - 1 and x_cat[1] == -2 ** 31 and x_cat[2] == -1 and x_cat[25] == -2
    # the modulus is taken of the NON-NEGATIVE value first
    code, _, _, x_cat = R.parse_line(_line(f14="ffffffff", f15="80000000"), max_ind_range=10)
    assert code == 0 and x_cat[0] == (2 ** 32 - 1) % 10 and x_cat[1] == 2 ** 31 % 10
    # ... and the dictionary is keyed by the int32
    got = R.etl([[_line(f14="ffffffff"), _line(f14="80000000"), _line(f14="ffffffff")]])
    assert got["unique"][0].tolist() == [-1, -2 ** 31] and got["X_cat"][:, 0].tolist() == [0, 1, 0]


def test_ids_follow_first_appearance_across_days():
    days = [[_line(f14="b"), _line(f14="a")], [_line(f14="c"), _line(f14="a"), _line(f14="0")], [_line(f14="")]]
    got = R.etl(days)
    assert got["unique"][0].tolist() == [0xb, 0xa, 0xc, 0]                   # not sorted: first appearance, day order
    assert [d[0][:, 0].tolist() for d in got["days"]] == [[0, 1], [2, 1, 3], [3]]
    assert got["counts"][0] == 4 and got["total_per_file"].tolist() == [2, 3, 1]


def test_sub_sampling_drops_zero_targets_below_the_rate_and_counts_what_is_left():
    lines = [_line(f0=str(k % 2)) for k in range(10)]
    rng = np.random.RandomState(3)
    u = rng.uniform(size=10)
    got = R.etl([lines], sub_sample_rate=0.5, rng=np.random.RandomState(3))
    keep = [(k % 2 == 1) or not (u[k] < 0.5) for k in range(10)]
    assert got["total_per_file"].tolist() == [sum(keep)] and 5 < sum(keep) < 10
    assert R.keep_mask([0, 0, 1], [0.5, 0.49999, 0.0], 0.5).tolist() == [True, False, True]


@pytest.mark.parametrize("line,code", [
    (b"\t".join([b"1"] * 39), R.ERR_FIELDS), (b"\t".join([b"1"] * 41), R.ERR_FIELDS), (b"", R.ERR_FIELDS),
    (_line(f3="-"), R.ERR_DEC_BYTE), (_line(f3="+1"), R.ERR_DEC_BYTE), (_line(f3=" 1"), R.ERR_DEC_BYTE), (_line(f3="1_0"), R.ERR_DEC_BYTE),
    (_line(f3="9" * 300), R.ERR_DEC_RANGE), (_line(f3="2147483648"), R.ERR_DEC_RANGE), (_line(f0="-2147483649"), R.ERR_DEC_RANGE),
    (_line(f20="123456789"), R.ERR_HEX_LONG), (_line(f20="0x12"), R.ERR_HEX_BYTE), (_line(f20="12g"), R.ERR_HEX_BYTE),
    (_line(f39="ab\r"), R.ERR_HEX_BYTE), (_line(f5="\xff"), R.ERR_DEC_BYTE),
    (_line(f20="12345678g"), R.ERR_HEX_BYTE), (_line(f0="2147483648", f2="x"), R.ERR_DEC_RANGE)])
def test_malformed_lines_have_their_codes_and_zero_outputs(line, code):
    got = R.parse_line(line)
    assert got[0] == code and got[1] == 0 and not any(got[2]) and not any(got[3])
    with pytest.raises(R.Malformed) as e:
        R.etl([[_line(), line, _line()]])
    assert e.value.line1 == 2 and e.value.code == code


def test_well_formed_edges():
    code, y, x_int, x_cat = R.parse_line(_line(f0="", f1="-2147483648", f2="2147483647", f3="-0", f4="0" * 300, f39=""))
    assert code == 0 and y == 0 and x_int[:4] == [0, 2 ** 31 - 1, 0, 0] and x_cat[25] == 0
    assert R.parse_line(b"\t" * 39)[0] == 0
    assert R.split_lines(b"a\nb") == [b"a", b"b"] and R.split_lines(b"a\nb\n") == [b"a", b"b"] and R.split_lines(b"") == []
    starts, n = R.line_starts(b"ab\n\ncd")
    assert n == 2 and starts.tolist() == [0, 3, 4]


# ---- what getCriteoAdData refuses before it touches the device ------------------------------------------------------------------

def _write_kaggle(g, d):
    raw = os.path.join(str(d), "train.txt")
    with open(raw, "wb") as f:
        f.write(g["kaggle_raw"].tobytes())
    return raw


def test_an_existing_output_is_refused_unless_forced(golden, tmp_path):
    from cdlrm_amd import data_utils as DU
    raw = os.path.join(str(tmp_path), "train.txt")                            # the raw file itself is missing
    for name in ("train_day_count.npz", "train_fea_dict_25.npz", "train_day_3_processed.npz", "kaggleAdDisplayChallenge_processed.npz"):
        p = os.path.join(str(tmp_path), name)
        open(p, "wb").close()
        with pytest.raises(FileExistsError, match=re.escape(p)):
            DU.getCriteoAdData(raw, "kaggleAdDisplayChallenge_processed")
        # forced: past that refusal, on to the next one (no raw file) -- still before the device
        with pytest.raises(FileNotFoundError, match="train.txt"):
            DU.getCriteoAdData(raw, "kaggleAdDisplayChallenge_processed", force=True)
        with pytest.raises(SystemExit) as e:
            DU.main(["--raw-data-file=" + raw, "--data-set=kaggle"])
        assert str(e.value).startswith("ERROR: ") and p in str(e.value) and "\n" not in str(e.value)
        with pytest.raises(SystemExit) as e:
            DU.main(["--raw-data-file=" + raw, "--data-set=kaggle", "--force"])
        assert str(e.value).startswith("ERROR: ") and "train.txt" in str(e.value) and "exists" not in str(e.value)
        os.remove(p)
    # memory_map writes no concatenated file, so an existing one is not in its way
    open(os.path.join(str(tmp_path), "kaggleAdDisplayChallenge_processed.npz"), "wb").close()
    with pytest.raises(FileNotFoundError):
        DU.getCriteoAdData(raw, "kaggleAdDisplayChallenge_processed", memory_map=True)


def test_a_missing_day_file_is_named(golden, tmp_path):
    from cdlrm_amd import data_utils as DU
    g = golden("criteo_etl")
    for i in (0, 2):
        with open(os.path.join(str(tmp_path), "day_%d" % i), "wb") as f:
            f.write(g["tb_raw_%d" % i].tobytes())
    with pytest.raises(FileNotFoundError, match="day_1"):
        DU.getCriteoAdData(os.path.join(str(tmp_path), "day"), "terabyte_processed", days=3, criteo_kaggle=False)
    with pytest.raises(SystemExit) as e:
        DU.main(["--raw-data-file=" + os.path.join(str(tmp_path), "day"), "--data-set=terabyte", "--days=3"])
    assert str(e.value).startswith("ERROR: ") and "day_1" in str(e.value) and "\n" not in str(e.value)
    assert sorted(os.listdir(str(tmp_path))) == ["day_0", "day_2"]            # nothing was written


def test_command_line_refusals_and_flags(tmp_path):
    from cdlrm_amd import data_utils as DU
    with pytest.raises(SystemExit) as e:
        DU.main(["--raw-data-file=/nowhere/train.txt", "--data-set=avazu"])
    assert str(e.value) == "ERROR: Data set option is not supported: --data-set=avazu (kaggle | terabyte)"
    with pytest.raises(SystemExit) as e:
        DU.main(["--data-set=kaggle"])
    assert str(e.value).startswith("ERROR: --raw-data-file")
    with pytest.raises(SystemExit) as e:
        DU.main(["--raw-data-file=/nowhere/train.txt", "--processed-data-file=/elsewhere/x.npz"])
    assert str(e.value).startswith("ERROR: --processed-data-file") and "/nowhere/kaggleAdDisplayChallenge_processed.npz" in str(e.value)
    with pytest.raises(ValueError, match="sub_sample_rate"):
        DU.getCriteoAdData("/nowhere/train.txt", "x", sub_sample_rate=1.5)
    a = DU.build_parser().parse_args([])
    assert (a.max_ind_range, a.data_sub_sample_rate, a.numpy_rand_seed, a.memory_map, a.days, a.force, a.store, a.data_set) == \
        (-1, 0.0, 123, False, 0, False, False, "kaggle")
    a = DU.build_parser().parse_args(["--raw-data-file=r", "--processed-data-file=p", "--data-set=terabyte", "--max-ind-range=40000000",
                                      "--data-sub-sample-rate=0.875", "--numpy-rand-seed=7", "--memory-map", "--days=3", "--force",
                                      "--store"])
    assert (a.raw_data_file, a.processed_data_file, a.data_set, a.max_ind_range, a.data_sub_sample_rate, a.numpy_rand_seed,
            a.memory_map, a.days, a.force, a.store) == ("r", "p", "terabyte", 40000000, 0.875, 7, True, 3, True, True)
    assert DU.DATA_SETS == {"kaggle": (7, "kaggleAdDisplayChallenge_processed"), "terabyte": (24, "terabyte_processed")}


def test_host_side_of_the_text(golden, tmp_path):
    """Line counts, the byte ranges of the Kaggle pieces and the last-newline search, against the restated split."""
    from cdlrm_amd import data_utils as DU
    g = golden("criteo_etl")
    raw = _write_kaggle(g, tmp_path)
    text = g["kaggle_raw"].tobytes()
    for block in (7, 64, 1 << 20):
        n, per_block = DU._count_lines(raw, block)
        assert n == 75 and sum(per_block) == 74
        for k in (1, 11, 74):
            off = DU._offset_after_newline(raw, per_block, k, block)
            assert text[:off].count(b"\n") == k and text[off - 1:off] == b"\n"
    src = DU._sources(raw, "", 7, True)
    want = R.kaggle_days(text)
    assert [s.lines for s in src] == [len(d) for d in want] and [s.line0 for s in src] == [0, 11, 22, 33, 44, 55, 65]
    for s, lines in zip(src, want):
        assert R.split_lines(text[s.begin:s.end]) == lines
    assert src[-1].end == len(text)
    # more pieces than lines: the empty ones are empty ranges
    small = os.path.join(str(tmp_path), "small.txt")
    with open(small, "wb") as f:
        f.write(b"a\nb")
    assert [(s.begin, s.end, s.lines) for s in DU._sources(small, "", 3, True)] == [(0, 2, 1), (2, 3, 1), (3, 3, 0)]
    buf = np.frombuffer(b"x" * 70000 + b"\n" + b"y" * 66000, dtype=np.uint8)
    assert DU._last_newline(buf, buf.size) == 70000 and DU._last_newline(buf, 70000) == -1 and DU._last_newline(buf, 0) == -1
    rows, ring, dictionary = DU._day_bytes(1000, 4096, True, 50)
    assert rows == 1000 * 160 + 8000 and ring > 9 * 4096 and dictionary == 16 * 50 + 40 * 1050


# ---- ABI ------------------------------------------------------------------------------------------------------------------------

def test_etl_entry_points_header_prototypes_and_exports():
    from cdlrm_amd import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cdlrm_hip.h")).read(), flags=re.S)
    vp, i64, i32 = C.c_void_p, C.c_int64, C.c_int32
    want = {
        "cdlrm_etl_line_index_work_bytes": (i64, [i64]),
        "cdlrm_etl_line_index": (C.c_int, [vp, i64, vp, i64, vp, vp, i64, vp]),
        "cdlrm_etl_parse": (C.c_int, [vp, i64, vp, i64, i64, i64, vp, vp, vp, vp, vp]),
        "cdlrm_etl_subsample_work_bytes": (i64, [i64]),
        "cdlrm_etl_subsample": (C.c_int, [vp, vp, vp, i64, vp, i64, i64, C.c_double, vp, vp, vp, i64, vp, vp, vp, i64, vp]),
        "cdlrm_etl_encode": (C.c_int, [vp, i64, i32, i32, vp, vp, i64, i64, vp, vp]),
    }
    ctype = {"int64_t": i64, "int32_t": i32, "double": C.c_double, "int": C.c_int}
    for name, (res, args) in want.items():
        m = re.search(r"(\w+)\s+%s\(([^)]*)\);" % name, hdr)
        assert m, name + " is not declared"
        declared = [vp if "*" in a else ctype[a.split()[-2]] for a in m.group(2).split(",")]
        assert ctype[m.group(1)] is res and declared == args, name
        assert _lib.PROTOTYPES[name] == (res, args), name
        assert hasattr(_lib.raw(), name), name
    # the work-buffer queries are plain host arithmetic: callable without a device
    L = _lib.raw()
    assert L.cdlrm_etl_line_index_work_bytes(0) == 16 and L.cdlrm_etl_line_index_work_bytes(4097) == 32
    assert L.cdlrm_etl_subsample_work_bytes(257) == 32 and L.cdlrm_etl_line_index_work_bytes(-1) == -1
    # the codes the host names are the header's
    from cdlrm_amd import ops
    parse_h = open(os.path.join(ROOT, "cdlrm_amd", "csrc", "etl_parse.h")).read()
    codes = {int(v): k for k, v in re.findall(r"#define (ETL_ERR_\w+) (\d+)", parse_h)}
    assert sorted(codes) == sorted(ops.ETL_CODES) == [1, 2, 3, 4, 5, 6, 7]
    assert (R.ERR_FIELDS, R.ERR_DEC_BYTE, R.ERR_DEC_RANGE, R.ERR_HEX_BYTE, R.ERR_HEX_LONG, R.ERR_NOT_IN_DICT) == tuple(
        k for k in sorted(codes) if codes[k] != "ETL_ERR_SPAN")


# ---- the parser under the sanitizers ----------------------------------------------------------------------------------------------

def test_parser_is_clean_under_address_and_undefined_sanitizers(golden, tmp_path):
    cxx = next((c for c in (os.environ.get("CXX"), "c++", "g++", "clang++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = os.path.join(str(tmp_path), "etl_parse_check")
    base = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
            "-I", os.path.join(ROOT, "cdlrm_amd", "csrc"), os.path.join(ROOT, "tools", "etl_parse_check.cpp"), "-o", exe]
    # the sanitizer runtime inside the executable where the compiler can put it there (gcc links it shared by default)
    for extra in (["-static-libasan", "-static-libubsan"], ["-static-libsan"], []):
        built = subprocess.run(base + extra, capture_output=True, text=True)
        if built.returncode == 0:
            break
    assert built.returncode == 0, built.stderr[-3000:]
    g = golden("criteo_etl")
    files = {"kaggle": g["kaggle_raw"].tobytes()}
    files.update({"tb%d" % i: g["tb_raw_%d" % i].tobytes() for i in range(3)})
    paths = []
    for name, raw in files.items():
        paths.append(os.path.join(str(tmp_path), name))
        with open(paths[-1], "wb") as f:
            f.write(raw)
    run = subprocess.run([exe] + paths, capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-4000:])
    assert "etl_parse_check: all cases ok" in run.stdout and "runtime error" not in run.stderr and "Sanitizer" not in run.stderr
    seen = re.findall(r"^(\S+): range (-?\d+) lines (\d+) errors (\d+) sum (-?\d+)$", run.stdout, flags=re.M)
    assert len(seen) == 2 * len(files)
    for path, mir, lines, errors, total in seen:
        y, x_int, x_cat, errs = R.parse_lines(R.split_lines(files[os.path.basename(path)]), int(mir))
        assert (int(lines), int(errors)) == (len(y), len(errs)) == (len(y), 0)
        assert int(total) == int(y.astype(np.int64).sum() + x_int.astype(np.int64).sum() + x_cat.astype(np.int64).sum())
