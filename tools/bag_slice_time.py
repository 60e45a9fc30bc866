"""Per-step cost of building a rank's multi-hot inputs: the device path (engine.BagWindows: one window copy, then
cdlrm_bags_rank_slice per step) against the host path (engine.square_bags per step, pad_window per window) on the same
ragged batches.  Wall time per step / window including the host work and the transfer, device synchronised at the end of
each timed loop.

    python tools/bag_slice_time.py [--tables 26] [--batch 2048] [--per-bag 10] [--world 2] [--lookahead 4] [--reps 20]
"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cdlrm_amd.engine import BagWindows, pad_window, rank_bag_slice, square_bags  # noqa: E402


def batches(T, B, npl, L, seed=0):
    """L ragged batches in the random front end's layout: 1 .. npl lookups per bag, lS_o [T, B], T lists."""
    rng = np.random.RandomState(seed)
    out = []
    for _ in range(L):
        off, lists = [], []
        for _k in range(T):
            sizes = rng.randint(1, npl + 1, size=B)
            off.append(np.concatenate([[0], np.cumsum(sizes)[:-1]]))
            lists.append(torch.from_numpy(rng.randint(0, 1 << 20, size=int(sizes.sum())).astype(np.int64)))
        out.append((torch.rand(B, 13), torch.from_numpy(np.stack(off).astype(np.int64)), lists, torch.ones(B, 1)))
    return out


def timed(fn, reps, dev):
    fn()
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize(dev)
    return 1e3 * (time.perf_counter() - t0) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tables", type=int, default=26)
    ap.add_argument("--batch", type=int, default=2048)
    ap.add_argument("--per-bag", type=int, default=10)
    ap.add_argument("--world", type=int, default=2)
    ap.add_argument("--lookahead", type=int, default=4)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    T, B, W, L = a.tables, a.batch, a.world, a.lookahead
    win = batches(T, B, a.per_bag, L)
    lbs = math.ceil(B / W)
    res = dict(tables=T, batch=B, per_bag=a.per_bag, world=W, lookahead=L)

    # host: the world-1 step (square_bags of the global batch) and the same on the rank's host-sliced lists
    def host_global():
        for X, off, lists, _ in win:
            square_bags([off[k] for k in range(T)], lists, dev)

    def host_rank():
        for X, off, lists, _ in win:
            lens = torch.tensor([x.numel() for x in lists])
            s0, s1, lo, hi, _n = rank_bag_slice(off, lens, lbs, 0)
            square_bags([off[k, s0:s1] - lo[k] for k in range(T)], [lists[k][int(lo[k]):int(hi[k])] for k in range(T)], dev)

    def host_window():
        pad_window([torch.cat([b[2][k] for b in win]) for k in range(T)], dev)

    holder = BagWindows(T, dev, lbs, world_size=W, rank=0)
    bw = holder.load(win)

    def dev_steps():
        for j in range(L):
            bw.rank_batch(j)

    def dev_window():
        holder.load(win).window_indices()

    res["host_square_bags_global_ms_per_step"] = timed(host_global, a.reps, dev) / L
    res["host_square_bags_rank_slice_ms_per_step"] = timed(host_rank, a.reps, dev) / L
    res["device_rank_batch_ms_per_step"] = timed(dev_steps, a.reps, dev) / L
    res["host_pad_window_ms_per_window"] = timed(host_window, a.reps, dev)
    res["device_load_and_window_ms_per_window"] = timed(dev_window, a.reps, dev)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
