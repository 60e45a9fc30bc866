"""Day-file front ends timed alone: batches per second of the host `DataLoader`, of `DeviceDayLoader`, and the cutting kernel
(`ops.dayfile_window`) by itself with its achieved GB/s against the bytes it has to move per sample (160 read + 264 written at
13 dense / 26 categorical features).  Writes synthetic day files of the asked size to a temporary directory first.  One JSON
line.

    python tools/dayfile_loader_time.py --batch 8192 --lookahead 256 --batches 1024

Every figure is a host clock around work that ends in a device synchronise, after a warm-up pass over the same shapes; the
kernel's is the mean of --reps launches between two device events.  Needs the MI355X: there is no CPU path to time."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ND, NC = 13, 26
BYTES_PER_SAMPLE = 4 * (ND + NC + 1) + 4 * ND + 8 * NC + 4


def write_day_files(d, rows_per_file, seed=1, name="day"):
    rng = np.random.RandomState(seed)
    for day, n in enumerate(rows_per_file):
        np.savez(os.path.join(d, "%s_%d_reordered.npz" % (name, day)),
                 X_int=rng.randint(0, 1 << 20, size=(n, ND), dtype=np.int32),
                 X_cat=rng.randint(0, 1 << 30, size=(n, NC), dtype=np.int32), y=rng.randint(0, 2, size=n, dtype=np.int32))
    np.savez(os.path.join(d, "%s_day_count.npz" % name), total_per_file=np.array(rows_per_file))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8192)
    ap.add_argument("--lookahead", type=int, default=256, help="batches per window of the device loader")
    ap.add_argument("--batches", type=int, default=1024, help="batches in the generated day file")
    ap.add_argument("--host-batches", type=int, default=200, help="batches of the host loader that are timed")
    ap.add_argument("--max-ind-range", type=int, default=-1)
    ap.add_argument("--kernel-rows", type=int, default=1 << 22, help="samples per launch of the kernel-alone timing")
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    from cdlrm_amd import _lib, ops
    from cdlrm_amd.data_loader_terabyte import DataLoader, DeviceDayLoader
    _lib.require_gpu("tools/dayfile_loader_time.py")
    dev = torch.device("cuda", 0)
    B, L = a.batch, a.lookahead
    rows = a.batches * B
    with tempfile.TemporaryDirectory() as d:
        # ONE day file: both loaders np.load whole files alike (the host loader on the training thread, the device loader on
        # its helper thread); with one file the load lies outside both timed regions and the figures are the loaders' own
        write_day_files(d, [rows + 17])
        # (a) the host loader alone, as main_no_ddp.Run consumes it without the uploads
        it = iter(DataLoader("day", d, [0], B, a.max_ind_range, "train", True))
        for _ in range(8):
            next(it)
        t0, n_host = time.perf_counter(), 0
        for _ in range(a.host_batches):
            if next(it, None) is None:
                break
            n_host += 1
        host_s = time.perf_counter() - t0
        del it
        # (b) the device loader alone: whole windows, everything it issues finished
        ld = DeviceDayLoader("day", d, [0], B, a.max_ind_range, "train", True, device=dev, window=L)
        for _ in ld:                    # warm-up epoch: allocations, code object, day files in the page cache
            pass
        torch.cuda.synchronize(dev)
        t0, n_dev = time.perf_counter(), 0
        for _ in ld:
            n_dev += 1
        torch.cuda.synchronize(dev)
        dev_s = time.perf_counter() - t0
    # (c) the kernel alone
    n = a.kernel_rows
    g = torch.Generator(device=dev)
    g.manual_seed(3)
    xi = torch.randint(0, 1 << 20, (n, ND), dtype=torch.int32, device=dev, generator=g)
    xc = torch.randint(0, 1 << 30, (n, NC), dtype=torch.int32, device=dev, generator=g)
    y = torch.randint(0, 2, (n,), dtype=torch.int32, device=dev, generator=g)
    X, I, T = (torch.empty(n, ND, device=dev), torch.empty(NC, n, dtype=torch.int64, device=dev), torch.empty(n, 1, device=dev))
    kernel = {}
    for mir in sorted({-1, a.max_ind_range if a.max_ind_range > 0 else 40000000}):
        for _ in range(3):
            ops.dayfile_window(xi, xc, y, mir, X, I, T)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.reps):
            ops.dayfile_window(xi, xc, y, mir, X, I, T)
        e1.record()
        e1.synchronize()
        ms = e0.elapsed_time(e1) / a.reps
        kernel["max_ind_range=%d" % mir] = dict(ms=round(ms, 4), GBps=round(BYTES_PER_SAMPLE * n / ms / 1e6, 1))
    print(json.dumps(dict(tool="dayfile_loader_time", batch=B, lookahead=L, batches=a.batches,
                          host_loader_batches_per_s=round(n_host / host_s, 1), host_batches_timed=n_host,
                          device_loader_batches_per_s=round(n_dev / dev_s, 1), device_batches_timed=n_dev,
                          kernel_rows=n, bytes_per_sample=BYTES_PER_SAMPLE, kernel=kernel)))


if __name__ == "__main__":
    main()
