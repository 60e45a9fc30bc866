"""The processed-file front ends timed alone, tools/dayfile_loader_time.py's figures for the resident path, at the Kaggle shape
(13 dense / 26 categorical features, batches of 2048, windows of 200 batches, a few million resident rows):

  * the permuted cut (`ops.rows_window`) alone, with its achieved GB/s against the bytes it has to move per sample (160 read +
    264 written) -- for a random permutation of the resident rows and, for comparison, for the identity order;
  * the consecutive cut (`ops.dayfile_window`) on the same number of consecutive rows of the same arrays, alternating with it
    in the same process: that kernel is the yardstick, the gap is what scattered 52 / 104-byte rows cost;
  * batches per second of `ProcessedLoader` and of `DeviceProcessedLoader` over a synthetic processed file.

One JSON line; --out also writes it to a file (profiles/processed_loader.json).

    python tools/processed_loader_time.py --out profiles/processed_loader.json

Every loader figure is a host clock around work that ends in a device synchronise, after a warm-up pass over the same shapes;
a kernel's is the mean of --reps launches between two device events, the two kernels alternating over --rounds rounds (the
smallest and the largest round are reported beside the mean).  Needs the MI355X: there is no CPU path to time."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=2048)
    ap.add_argument("--lookahead", type=int, default=200, help="batches per window of the device loader")
    ap.add_argument("--rows", type=int, default=4 << 20, help="resident rows (the Kaggle set has 45.8 M)")
    ap.add_argument("--host-batches", type=int, default=200, help="batches of the host loader that are timed")
    ap.add_argument("--max-ind-range", type=int, default=-1)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", type=str, default="")
    a = ap.parse_args()
    from cdlrm_amd import _lib, ops
    from cdlrm_amd.data_loader_processed import DeviceProcessedLoader, ProcessedDataset, ProcessedLoader, processed_order
    _lib.require_gpu("tools/processed_loader_time.py")
    dev = torch.device("cuda", 0)
    B, L, n_rows = a.batch, a.lookahead, a.rows
    rng = np.random.RandomState(1)
    # seven days; the last one (its halves test and validate) is an eighth of the file
    sizes = [n_rows // 8] * 7
    sizes[0] += n_rows - sum(sizes)
    with tempfile.TemporaryDirectory() as d:
        pro = os.path.join(d, "kaggleAdDisplayChallenge_processed.npz")
        np.savez(pro, X_int=rng.randint(0, 1 << 20, size=(n_rows, ND), dtype=np.int32),
                 X_cat=rng.randint(0, 1 << 30, size=(n_rows, NC), dtype=np.int32), y=rng.randint(0, 2, size=n_rows, dtype=np.int32),
                 counts=np.full(NC, 1 << 30))
        ds = ProcessedDataset(pro, sizes)
    np.random.seed(1)
    order = processed_order(sizes, "train", "total")
    # (a) the host loader alone, as main_no_ddp.Run consumes it without the uploads
    it = iter(ProcessedLoader(ds, order, B, a.max_ind_range, True))
    for _ in range(8):
        next(it)
    t0, n_host = time.perf_counter(), 0
    for _ in range(a.host_batches):
        if next(it, None) is None:
            break
        n_host += 1
    host_s = time.perf_counter() - t0
    del it
    # (b) the device loader alone: whole windows, everything it issues finished (the warm-up epoch uploads the rows)
    ld = DeviceProcessedLoader(ds, order, B, a.max_ind_range, True, device=dev, window=L)
    t0 = time.perf_counter()
    for _ in ld:
        pass
    torch.cuda.synchronize(dev)
    first_epoch_s = time.perf_counter() - t0
    t0, n_dev = time.perf_counter(), 0
    for _ in ld:
        n_dev += 1
    torch.cuda.synchronize(dev)
    dev_s = time.perf_counter() - t0
    # (c) the kernels alone, on the resident arrays: one window's worth of samples per launch, as the loader launches them.
    # Launch r cuts window r of the epoch (the windows wrap around): every launch reads other rows, so the reads of a round come
    # from HBM unless the whole file fits the Infinity Cache; the outputs go to a ring of three windows.
    xi, xc, y = ds.resident(dev, torch.cuda.current_stream(dev))
    n = min(L * B, order.shape[0])
    nw = max(1, order.shape[0] // n)
    orders = dict(permuted=torch.from_numpy(order).to(dev), identity=torch.arange(order.shape[0], dtype=torch.int64, device=dev))
    ring = [(torch.empty(n, ND, device=dev), torch.empty(NC, n, dtype=torch.int64, device=dev), torch.empty(n, 1, device=dev))
            for _ in range(3)]
    mir = a.max_ind_range

    def sl(r):
        return slice((r % nw) * n, (r % nw + 1) * n)

    runs = dict(rows_window_permuted=lambda r: ops.rows_window(xi, xc, y, orders["permuted"][sl(r)], mir, *ring[r % 3]),
                rows_window_identity=lambda r: ops.rows_window(xi, xc, y, orders["identity"][sl(r)], mir, *ring[r % 3]),
                dayfile_window_consecutive=lambda r: ops.dayfile_window(xi[sl(r)], xc[sl(r)], y[sl(r)], mir, *ring[r % 3]))
    times = {k: [] for k in runs}
    for fn in runs.values():
        for r in range(3):
            fn(r)
    for _ in range(a.rounds):
        for k, fn in runs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for r in range(a.reps):
                fn(r)
            e1.record()
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1) / a.reps)
    kernel = {k: dict(ms=round(float(np.mean(v)), 4), ms_min=round(min(v), 4), ms_max=round(max(v), 4),
                      GBps=round(BYTES_PER_SAMPLE * n / float(np.mean(v)) / 1e6, 1)) for k, v in times.items()}
    res = dict(tool="processed_loader_time", batch=B, lookahead=L, resident_rows=n_rows, train_rows=int(order.shape[0]),
               max_ind_range=mir, host_loader_batches_per_s=round(n_host / host_s, 1), host_batches_timed=n_host,
               device_loader_batches_per_s=round(n_dev / dev_s, 1), device_batches_timed=n_dev,
               device_loader_first_epoch_s=round(first_epoch_s, 3), kernel_rows=n, kernel_windows=nw,
               bytes_per_sample=BYTES_PER_SAMPLE,
               kernel=kernel,
               permuted_over_consecutive=round(float(np.mean(times["rows_window_permuted"]))
                                               / float(np.mean(times["dayfile_window_consecutive"])), 3))
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
