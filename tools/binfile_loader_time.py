"""The MLPerf binary front ends timed alone, tools/dayfile_loader_time.py's three figures for the binary path: batches per
second of the host `BinLoader`, of `DeviceBinLoader`, and of `DeviceDayLoader` over a day file of the same samples beside it;
and the two cutting kernels (`ops.binfile_window`, `ops.dayfile_window`) side by side on the same samples, in one process,
launches alternating, each launch between two device events of its own: the median and the spread of --reps launches after a
warm-up, with the achieved GB/s against the bytes a sample costs either kernel (160 read + 264 written at 13 dense / 26
categorical features).  Writes a synthetic binary file and day file of the asked size to a temporary directory first.  One
JSON line, also written to --out when given.

    python tools/binfile_loader_time.py --batch 8192 --lookahead 256 --batches 1024 --out profiles/binfile_loader_time.json

Needs the MI355X: there is no CPU path to time."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ND, NC = 13, 26
BYTES_PER_SAMPLE = 4 * (ND + NC + 1) + 4 * ND + 8 * NC + 4


def _epoch_rate(ld, dev):
    for _ in ld:                    # warm-up epoch: allocations, code object, files in the page cache
        pass
    torch.cuda.synchronize(dev)
    t0, n = time.perf_counter(), 0
    for _ in ld:
        n += 1
    torch.cuda.synchronize(dev)
    return n, time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8192)
    ap.add_argument("--lookahead", type=int, default=256, help="batches per window of the device loaders")
    ap.add_argument("--batches", type=int, default=1024, help="batches in the generated files")
    ap.add_argument("--host-batches", type=int, default=200, help="batches of the host loader that are timed")
    ap.add_argument("--max-ind-range", type=int, default=-1)
    ap.add_argument("--kernel-batches", type=int, default=256, help="batches of --batch samples per launch of the kernels")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    from cdlrm_amd import _lib, ops
    from cdlrm_amd.data_loader_terabyte import BinLoader, CriteoBinDataset, DeviceBinLoader, DeviceDayLoader
    _lib.require_gpu("tools/binfile_loader_time.py")
    dev = torch.device("cuda", 0)
    B, L = a.batch, a.lookahead
    rows = a.batches * B + 17
    rng = np.random.RandomState(1)
    x_int = rng.randint(0, 1 << 20, size=(rows, ND), dtype=np.int32)
    x_cat = rng.randint(0, 1 << 30, size=(rows, NC), dtype=np.int32)
    y = rng.randint(0, 2, size=rows, dtype=np.int32)
    with tempfile.TemporaryDirectory() as d:
        with open(os.path.join(d, "t_train.bin"), "wb") as f:
            step = 1 << 20
            for r in range(0, rows, step):
                f.write(np.concatenate([y[r:r + step, None], x_int[r:r + step], x_cat[r:r + step]], axis=1).tobytes())
        np.savez(os.path.join(d, "day_fea_count.npz"), counts=np.full(NC, 1 << 30))
        np.savez(os.path.join(d, "day_0_reordered.npz"), X_int=x_int, X_cat=x_cat, y=y)
        np.savez(os.path.join(d, "day_day_count.npz"), total_per_file=np.array([rows]))
        ds = CriteoBinDataset(os.path.join(d, "t_train.bin"), os.path.join(d, "day_fea_count.npz"), B, a.max_ind_range)
        # (a) the host loader alone, as main_no_ddp.Run consumes it without the uploads
        it = iter(BinLoader(ds, drop_last_batch=True))
        for _ in range(8):
            next(it)
        t0, n_host = time.perf_counter(), 0
        for _ in range(a.host_batches):
            if next(it, None) is None:
                break
            n_host += 1
        host_s = time.perf_counter() - t0
        del it
        # (b) the device loaders alone: whole windows, everything they issue finished
        n_bin, bin_s = _epoch_rate(DeviceBinLoader(ds, drop_last_batch=True, device=dev, window=L), dev)
        n_shuf, shuf_s = _epoch_rate(DeviceBinLoader(ds, shuffle=True, drop_last_batch=True, device=dev, window=L), dev)
        n_day, day_s = _epoch_rate(DeviceDayLoader("day", d, [0], B, a.max_ind_range, "train", True, device=dev, window=L), dev)
    # (c) the two kernels on the same samples, alternating
    n = a.kernel_batches * B
    xi, xc, yy = (torch.from_numpy(v[:n]).to(dev) for v in (x_int, x_cat, y))
    rec = torch.cat([yy[:, None], xi, xc], dim=1).contiguous()
    X, I, T = (torch.empty(n, ND, device=dev), torch.empty(NC, n, dtype=torch.int64, device=dev), torch.empty(n, 1, device=dev))
    kernel = {}
    for mir in sorted({-1, a.max_ind_range if a.max_ind_range > 0 else 40000000}):
        launch = dict(binfile=lambda: ops.binfile_window(rec, ND, mir, X, I, T),
                      dayfile=lambda: ops.dayfile_window(xi, xc, yy, mir, X, I, T))
        for _ in range(5):
            for fn in launch.values():
                fn()
        ms = {k: [] for k in launch}
        for _ in range(a.reps):
            for k, fn in launch.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                ms[k].append(e0.elapsed_time(e1))
        kernel["max_ind_range=%d" % mir] = {
            k: dict(ms_median=round(statistics.median(v), 4), ms_min=round(min(v), 4), ms_max=round(max(v), 4),
                    GBps_median=round(BYTES_PER_SAMPLE * n / statistics.median(v) / 1e6, 1)) for k, v in ms.items()}
    line = json.dumps(dict(tool="binfile_loader_time", batch=B, lookahead=L, batches=a.batches,
                           host_bin_loader_batches_per_s=round(n_host / host_s, 1), host_batches_timed=n_host,
                           device_bin_loader_batches_per_s=round(n_bin / bin_s, 1),
                           device_bin_loader_shuffled_batches_per_s=round(n_shuf / shuf_s, 1),
                           device_day_loader_batches_per_s=round(n_day / day_s, 1), device_batches_timed=n_bin,
                           kernel_rows=n, kernel_reps=a.reps, bytes_per_sample=BYTES_PER_SAMPLE, kernel=kernel))
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
