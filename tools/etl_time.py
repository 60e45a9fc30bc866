#!/usr/bin/env python3
"""Time the stages of the Criteo ETL (cdlrm_amd/data_utils.py) on synthetic Criteo-shaped text, against two yardsticks taken
in the same run: the host->device copy of the same chunk, and the restated per-line Python loop (tests/etl_restated.py).

    python tools/etl_time.py [--lines 2000000] [--chunk-bytes 33554432] [--reps 5] [--out profiles/etl_times.json]

The text is written locally from a seed: one label, 13 decimal fields and 26 eight-digit hex fields per line, 288 bytes a line
(the Kaggle train.txt averages about 240), the hashes drawn skewed from per-column pools of 10 to 2 * 10^6 values and spread
over all 32 bits, so about half of them wrap.  Per chunk and repetition the stages run one after the other between device
events on one stream -- copy, line index, parse, drop (rate 0.5), encode -- so the yardstick copy and the kernels alternate
inside every repetition; the first repetition is warm-up, the figures are medians over the chunks of the others, with the
smallest and largest beside them.  File read, dictionary extension, download and the npz writes are host clocks around work
that ends in a synchronise.  The whole of `getCriteoAdData` is then timed end to end (compressed and stored), and the restated
Python loop on a slice.  Needs the GPU: there is no figure without one."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

LINE_BYTES = 1 + 13 * 4 + 26 * 9 + 1


def write_text(path, n_lines, seed=7, block=250000):
    """n_lines of fixed-width Criteo-shaped text; returns the bytes written."""
    rng = np.random.RandomState(seed)
    cards = np.unique(np.round(np.logspace(1, np.log10(2e6), 26)).astype(np.int64))
    cards = np.resize(cards, 26)
    hexd = np.frombuffer(b"0123456789abcdef", dtype=np.uint8)
    with open(path, "wb") as f:
        for at in range(0, n_lines, block):
            n = min(block, n_lines - at)
            m = np.empty((n, LINE_BYTES), dtype=np.uint8)
            m[:, 0] = 48 + (rng.rand(n) < 0.25)
            dense = rng.randint(0, 1000, size=(n, 13))
            for j in range(13):
                c = 1 + 4 * j
                m[:, c] = 9
                m[:, c + 1] = 48 + dense[:, j] // 100
                m[:, c + 2] = 48 + dense[:, j] // 10 % 10
                m[:, c + 3] = 48 + dense[:, j] % 10
            neg = rng.rand(n) < 0.05                                    # "-01" .. : clamped to 0
            m[neg, 2] = 45
            for j in range(26):
                c = 1 + 52 + 9 * j
                v = ((rng.zipf(1.2, size=n) % cards[j]).astype(np.uint64) * np.uint64(2654435761 + 2 * j)) & np.uint64(0xffffffff)
                m[:, c] = 9
                for d in range(8):
                    m[:, c + 1 + d] = hexd[((v >> np.uint64(4 * (7 - d))) & np.uint64(15)).astype(np.int64)]
            m[:, LINE_BYTES - 1] = 10
            f.write(m.tobytes())
    return n_lines * LINE_BYTES


def stats(ms):
    ms = np.asarray(ms, dtype=np.float64)
    return dict(median_ms=float(np.median(ms)), min_ms=float(ms.min()), max_ms=float(ms.max()), samples=int(ms.size))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lines", type=int, default=2000000)
    ap.add_argument("--chunk-bytes", type=int, default=32 << 20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--python-lines", type=int, default=100000)
    ap.add_argument("--dir", type=str, default="")
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "etl_times.json"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("ERROR: tools/etl_time.py measures on the GPU; none found")
    import etl_restated as R
    from cdlrm_amd import data_utils as DU
    from cdlrm_amd import ops
    dev = torch.device("cuda:0")
    work = args.dir or tempfile.mkdtemp(prefix="etl_time_")
    path = os.path.join(work, "day_0")
    t0 = time.perf_counter()
    total_bytes = write_text(path, args.lines)
    print("wrote %d lines, %.1f MB in %.1f s" % (args.lines, total_bytes / 1e6, time.perf_counter() - t0), flush=True)
    cap = args.chunk_bytes // LINE_BYTES * LINE_BYTES                    # whole lines per chunk: every chunk alike
    chunks = [(o, min(cap, total_bytes - o)) for o in range(0, total_bytes, cap)]
    lines_per_chunk = cap // LINE_BYTES

    # ---- file read (page cache warm: the file was just written), into pinned memory
    pinned = torch.empty(cap, dtype=torch.uint8).pin_memory()
    host = pinned.numpy()
    read_ms = []
    with open(path, "rb", buffering=0) as f:
        for o, n in chunks:
            t = time.perf_counter()
            got = f.readinto(memoryview(host)[:n])
            read_ms.append((time.perf_counter() - t) * 1e3)
            assert got == n

    # ---- per chunk: copy | index | parse | drop | encode between events, alternating inside every repetition
    stream = torch.cuda.Stream(device=dev)
    per = {k: [] for k in ("copy", "index", "parse", "drop")}
    with torch.cuda.stream(stream):
        text = torch.empty(cap, dtype=torch.uint8, device=dev)
        starts = torch.empty(cap + 1, dtype=torch.int64, device=dev)
        count = torch.empty(1, dtype=torch.int64, device=dev)
        err = ops.etl_error_word(dev)
        y = torch.empty(args.lines, dtype=torch.int32, device=dev)
        x_int = torch.empty((args.lines, 13), dtype=torch.int32, device=dev)
        x_cat = torch.empty((args.lines, 26), dtype=torch.int32, device=dev)
        oy, oi, oc = torch.empty_like(y[:lines_per_chunk]), torch.empty_like(x_int[:lines_per_chunk]), torch.empty_like(x_cat[:lines_per_chunk])
        rand_u = torch.from_numpy(np.random.RandomState(1).uniform(size=args.lines)).to(dev)
        rows = [torch.zeros(1, dtype=torch.int64, device=dev) for _ in range(2)]
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(6)]
        with open(path, "rb", buffering=0) as f:
            for rep in range(args.reps + 1):
                f.seek(0)
                row0 = 0
                for o, n in chunks:
                    f.readinto(memoryview(host)[:n])
                    ev[0].record(stream)
                    text[:n].copy_(pinned[:n], non_blocking=True)
                    ev[1].record(stream)
                    ops.etl_line_index(text, n, starts, count, stream=stream)
                    ev[2].record(stream)
                    nl = n // LINE_BYTES
                    ops.etl_parse(text, n, starts, nl, row0, -1, y, x_int, x_cat, err, row0=row0, stream=stream)
                    ev[3].record(stream)
                    rows[0].zero_()
                    ev[4].record(stream)
                    ops.etl_subsample(y[row0:row0 + nl], x_int[row0:row0 + nl], x_cat[row0:row0 + nl], nl, rand_u, row0, 0.5, oy, oi, oc,
                                      rows[0], rows[1], stream=stream)
                    ev[5].record(stream)
                    stream.synchronize()
                    assert int(count.item()) == nl and ops.etl_error(err) is None
                    if rep and n == cap:                                 # repetition 0 is warm-up; a short last chunk is left out
                        per["copy"].append(ev[0].elapsed_time(ev[1]))
                        per["index"].append(ev[1].elapsed_time(ev[2]))
                        per["parse"].append(ev[2].elapsed_time(ev[3]))
                        per["drop"].append(ev[4].elapsed_time(ev[5]))
                    row0 += nl
        # ---- dictionary extension over the whole day, then encode per chunk (a pristine copy is put back before every repetition)
        torch.cuda.synchronize()
        dict_ms = []
        for rep in range(3):
            t = time.perf_counter()
            dicts = [DU._Dictionary(dev) for _ in range(26)]
            for j, d in enumerate(dicts):
                d.extend(x_cat[:, j].contiguous(), 0)
            tables = [(d.keys, d.ids()) for d in dicts]
            torch.cuda.synchronize()
            dict_ms.append((time.perf_counter() - t) * 1e3)
        keys_total = int(sum(k.numel() for k, _ in tables))
        pristine = x_cat[:lines_per_chunk].clone()
        enc_ms = []
        for rep in range(args.reps + 1):
            x_cat[:lines_per_chunk].copy_(pristine)
            ev[0].record(stream)
            for j, (k, i) in enumerate(tables):
                ops.etl_encode(x_cat, j, k, i, err, n=lines_per_chunk, stream=stream)
            ev[1].record(stream)
            stream.synchronize()
            assert ops.etl_error(err) is None
            if rep:
                enc_ms.append(ev[0].elapsed_time(ev[1]))
        # ---- download of the day's arrays
        t = time.perf_counter()
        day = dict(X_cat=x_cat.cpu().numpy(), X_int=x_int.cpu().numpy(), y=y.cpu().numpy())
        down_ms = (time.perf_counter() - t) * 1e3
        del text, starts, x_cat, x_int, y, oy, oi, oc, rand_u, pristine, tables, dicts
    torch.cuda.empty_cache()
    # ---- npz writes
    t = time.perf_counter()
    np.savez(os.path.join(work, "stored.npz"), **day)
    store_ms = (time.perf_counter() - t) * 1e3
    t = time.perf_counter()
    np.savez_compressed(os.path.join(work, "compressed.npz"), **day)
    compress_ms = (time.perf_counter() - t) * 1e3
    del day

    # ---- the whole ETL, end to end
    e2e = {}
    for name, store in (("stored", True), ("compressed", False)):
        t = time.perf_counter()
        DU.getCriteoAdData(os.path.join(work, "day"), "terabyte_processed", days=1, criteo_kaggle=False, force=True, store=store,
                           chunk_bytes=args.chunk_bytes)
        e2e[name] = time.perf_counter() - t

    # ---- the restated per-line Python loop on a slice
    with open(path, "rb") as f:
        lines = R.split_lines(f.read(args.python_lines * LINE_BYTES))
    t = time.perf_counter()
    R.parse_lines(lines)
    py_parse_s = time.perf_counter() - t
    t = time.perf_counter()
    R.etl([lines])
    py_etl_s = time.perf_counter() - t

    s = {k: stats(v) for k, v in per.items()}
    s["encode"] = stats(enc_ms)
    gpu_ms = s["index"]["median_ms"] + s["parse"]["median_ms"] + s["encode"]["median_ms"]
    out = dict(
        device=torch.cuda.get_device_name(0), lines=args.lines, line_bytes=LINE_BYTES, text_bytes=total_bytes, chunk_bytes=cap,
        lines_per_chunk=lines_per_chunk, reps=args.reps, dictionary_keys=keys_total,
        per_chunk=s, file_read_per_chunk=stats(read_ms), dictionary_whole_day=stats(dict_ms), download_ms=down_ms,
        npz_store_ms=store_ms, npz_compress_ms=compress_ms,
        gpu_stages_ms_per_chunk=gpu_ms, copy_ms_per_chunk=s["copy"]["median_ms"], gpu_stages_over_copy=gpu_ms / s["copy"]["median_ms"],
        parse_over_copy=s["parse"]["median_ms"] / s["copy"]["median_ms"],
        copy_GBps=cap / s["copy"]["median_ms"] / 1e6, parse_GBps=cap / s["parse"]["median_ms"] / 1e6,
        end_to_end_s=e2e, end_to_end_lines_per_s={k: args.lines / v for k, v in e2e.items()},
        python_slice_lines=len(lines), python_parse_lines_per_s=len(lines) / py_parse_s, python_etl_lines_per_s=len(lines) / py_etl_s)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(out, indent=1, sort_keys=True))
    for name in os.listdir(work):
        if not args.dir:
            os.remove(os.path.join(work, name))
    if not args.dir:
        os.rmdir(work)


if __name__ == "__main__":
    main()
