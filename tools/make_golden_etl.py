#!/usr/bin/env python3
"""Generate tests/golden/criteo_etl.npz by IMPORTING the reference's data_utils, as tools/make_golden_processed.py does (same
container, same rules: only data travels -- the raw text and what the reference wrote for it).

    PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_etl.py

Small synthetic raw Criteo text goes through the reference's `getCriteoAdData` (data_utils.py:876-1121) in a temporary
directory, and everything it wrote is recorded: `total_per_file`, the 26 `unique` arrays, `counts`, every day's processed
arrays and the concatenated file.

  kaggle     one train.txt of 75 lines (7 pieces: 11 11 11 11 11 10 10), the last line without its newline, run three
             times: (rate 0, range -1), (rate 0.5 with np.random.seed(5), range -1), (rate 0, range 10)
  terabyte   three day files of 17, 1 and 9 lines, (rate 0, range -1)

The text holds empty fields (an empty last field too), negative dense values, hashes that repeat and hashes seen once, a
value that first appears on a later day, and a column with one distinct value.  Every hash stays below 2^31: above it the
reference raises OverflowError on numpy >= 1.24 (data_utils.py:998-1006).  X_cat is recorded as the reference writes it,
float64.  The archive is written with fixed zip timestamps so that a second run gives the same bytes."""
import contextlib
import io
import os
import sys
import tempfile
import zipfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as MG  # noqa: E402

KAGGLE_LINES, TB_LINES = 75, (17, 1, 9)
KAGGLE_CASES = {"k_r0_m0": (0.0, -1), "k_r5_m0": (0.5, -1), "k_r0_m10": (0.0, 10)}
SEED = 5


def make_text(rng, n, newline_at_end=True):
    """n lines of raw Criteo text."""
    pools = [rng.randint(0, 2 ** 31, size=sz, dtype=np.int64) for sz in rng.randint(2, 40, size=26)]
    lines = []
    for k in range(n):
        f = [str(int(rng.rand() < 0.35))]
        for j in range(13):
            u = rng.rand()
            f.append("" if u < 0.15 else str(int(rng.randint(-3, 0))) if u < 0.3 else str(int(rng.zipf(1.5) % 100000)))
        for j in range(26):
            u = rng.rand()
            if j == 7:
                v = "1f2e3d4c"                                   # a column with one distinct value
            elif j == 11 and k < n // 2:
                v = "%x" % pools[j][0]                           # its other values first appear in later days
            elif u < 0.1:
                v = ""
            elif u < 0.25:
                v = "%08x" % rng.randint(0, 2 ** 31)             # seen once, zero-padded
            else:
                v = "%x" % pools[j][rng.randint(0, len(pools[j]))]
            if rng.rand() < 0.3:
                v = v.upper()
            f.append(v)
        if k % 9 == 4:
            f[39] = ""                                           # an empty last field
        if k % 13 == 5:
            f[0] = ""                                            # an empty label is 0
        lines.append("\t".join(f))
    return ("\n".join(lines) + ("\n" if newline_at_end else "")).encode("ascii")


def record(out, tag, d, d_file, npzfile, o_file, days):
    with np.load(os.path.join(d, d_file + "_day_count.npz")) as z:
        out[tag + "_total_per_file"] = z["total_per_file"]
    for j in range(26):
        with np.load(os.path.join(d, d_file + "_fea_dict_%d.npz" % j)) as z:
            out["%s_unique_%d" % (tag, j)] = z["unique"]
    with np.load(os.path.join(d, d_file + "_fea_count.npz")) as z:
        out[tag + "_counts"] = z["counts"]
    for i in range(days):
        with np.load(npzfile + "_%d_processed.npz" % i) as z:
            for k in ("X_cat", "X_int", "y"):
                out["%s_day%d_%s" % (tag, i, k)] = z[k]
    with np.load(o_file) as z:
        for k in ("X_cat", "X_int", "y", "counts"):
            out["%s_all_%s" % (tag, k)] = z[k]


def save_fixed(path, arrs):
    """np.savez_compressed with fixed member timestamps (the same arrays give the same bytes)."""
    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_DEFLATED) as zf:
        for k in sorted(arrs):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arrs[k]), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            zf.writestr(info, buf.getvalue())
    print("wrote %s (%.1f KB)" % (path, os.path.getsize(path) / 1024))


def main():
    sys.dont_write_bytecode = True
    sys.path.insert(0, MG.REF)
    import data_utils as DU
    rng = np.random.RandomState(2024)
    kaggle_raw = make_text(rng, KAGGLE_LINES, newline_at_end=False)
    tb_raw = [make_text(rng, n) for n in TB_LINES]
    out = dict(kaggle_raw=np.frombuffer(kaggle_raw, dtype=np.uint8), seed=np.array(SEED),
               tb_lines=np.array(TB_LINES))
    for i, raw in enumerate(tb_raw):
        out["tb_raw_%d" % i] = np.frombuffer(raw, dtype=np.uint8)
    for tag, (rate, mir) in KAGGLE_CASES.items():
        with tempfile.TemporaryDirectory() as d:
            with open(os.path.join(d, "train.txt"), "wb") as f:
                f.write(kaggle_raw)
            np.random.seed(SEED)
            with contextlib.redirect_stdout(io.StringIO()):
                o = DU.getCriteoAdData(os.path.join(d, "train.txt"), "kaggleAdDisplayChallenge_processed", mir, rate, 7,
                                       "train", "total", True, False)
            record(out, tag, d, "train", os.path.join(d, "train_day"), o, 7)
            out[tag + "_rate"], out[tag + "_max_ind_range"] = np.array(rate), np.array(mir)
    with tempfile.TemporaryDirectory() as d:
        for i, raw in enumerate(tb_raw):
            with open(os.path.join(d, "day_%d" % i), "wb") as f:
                f.write(raw)
        with contextlib.redirect_stdout(io.StringIO()):
            o = DU.getCriteoAdData(os.path.join(d, "day"), "terabyte_processed", -1, 0.0, 3, "train", "total", False, False)
        record(out, "tb", d, "day", os.path.join(d, "day"), o, 3)
    save_fixed(os.path.join(MG.OUT, "criteo_etl.npz"), out)


if __name__ == "__main__":
    main()
