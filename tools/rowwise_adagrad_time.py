"""The embedding backward's apply alone at c3's step shape (T = 26, D = 128, n = 8192 lookups per table), plain SGD over all
slots (cdlrm_embbag_bwd_apply_sorted, rest = 0: the route a step takes with fuse_once off) against row-wise Adagrad
(cdlrm_embbag_bwd_apply_sorted_opt) on the SAME sorted lists, beside their byte floors.

Device events around one apply (its chunk kernel + k_bwd_long), the two variants alternated inside every repetition, medians
reported.  Slots: Zipf(alpha) ranks scattered over a cache of `sets` x `ways` slots per table far larger than the Infinity Cache
(tools/qr_cached_time.py's geometry; that tool draws its slots uniformly, which would leave no repeated slot to sum).
Byte floors: per lookup the gradient row and the sorted key and run distance (4 D + 12), per distinct slot the row read and
written (8 D); Adagrad adds the tag read and the accumulator read and written, distinct * (8 + 8).

    python tools/rowwise_adagrad_time.py [--batch 8192] [--tables 26] [--dim 128] [--alpha 1.05] [--reps 30]
                                         [--out profiles/rowwise_adagrad_c3.json]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cdlrm_amd import ops  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8192)
    ap.add_argument("--tables", type=int, default=26)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--sets", type=int, default=32771)
    ap.add_argument("--ways", type=int, default=4)
    ap.add_argument("--alpha", type=float, default=1.05)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", type=str, default=os.path.join("profiles", "rowwise_adagrad_c3.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("ERROR: tools/rowwise_adagrad_time.py measures on the MI355X and found no HIP device")
    dev = torch.device("cuda", 0)
    n, T, D, P, ways = a.batch, a.tables, a.dim, a.sets, a.ways
    rows_per_table = P * 64
    ctx = ops.CacheCtx([rows_per_table] * T, [P] * T, D, ways, n, dev, aux_phases=2)
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    # every slot holds a valid index of its set: tags[set, way] = set + P * way
    tags = (torch.arange(P, device=dev).view(P, 1) + P * torch.arange(ways, device=dev).view(1, ways)).reshape(-1).repeat(T)
    W = torch.rand(ctx.total_rows, D, device=dev, generator=g)
    ctx.bind_cache(tags.contiguous(), W)
    rng = np.random.RandomState(3)
    slots = np.stack([(rng.zipf(a.alpha, size=n).astype(np.uint64) * np.uint64(2654435761 + 2 * t)) % np.uint64(ways * P)
                      for t in range(T)]).astype(np.int32)
    distinct = int(sum(len(np.unique(s)) for s in slots))
    longest = int(max(np.unique(s, return_counts=True)[1].max() for s in slots))
    d_slots = torch.from_numpy(slots).to(dev)
    state = torch.rand(T * rows_per_table, device=dev, generator=g)
    state_base = torch.arange(T, device=dev, dtype=torch.int64) * rows_per_table
    dfeat = torch.rand(n, T + 1, D, device=dev, generator=g) - 0.5
    sbuf = ops.embbag_bwd_sorted(ctx, 1, n, dev)
    ops.embbag_bwd_prepare_window(ctx, d_slots, n, 1, n, sbuf)
    keys, meta, _ = ops.embbag_bwd_sorted_views(ctx, sbuf, 1, n, 0)
    work = ops.embbag_bwd_work(ctx, n, dev)
    lr, ld = 1e-4, dfeat.stride(0)
    calls = {
        "sgd_all_slots": lambda: ops.embbag_bwd_apply_sorted(ctx, n, dfeat[:, 1:, :], ld, D, lr, work, keys, meta, n, 0, False),
        "rowwise_adagrad": lambda: ops.embbag_bwd_apply_sorted_opt(ctx, n, dfeat[:, 1:, :], ld, D, lr, work, keys, meta, n, 0, False,
                                                                  opt="rowwise_adagrad", eps=1e-10, state=state,
                                                                  state_base=state_base),
    }
    sgd_floor = T * n * (4 * D + 12) + distinct * 8 * D
    floors = {"sgd_all_slots": sgd_floor, "rowwise_adagrad": sgd_floor + distinct * (8 + 8)}
    times = {k: [] for k in calls}
    torch.cuda.synchronize()
    for rep in range(a.reps + 3):
        for name, fn in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if rep >= 3:                                # three warm-up rounds of either variant
                times[name].append(e0.elapsed_time(e1) * 1e3)
    ctx.check()
    route = ops.embbag_bwd_route(T, D, n, False, "sorted")
    res = dict(shape=dict(lookups_per_table=n, tables=T, dim=D, distinct_slots=distinct, longest_run=longest, zipf_alpha=a.alpha,
                          cache_rows=int(ctx.total_rows), cache_gb=ctx.total_rows * D * 4 / 1e9,
                          state_mb=state.numel() * 4 / 1e6),
               route=dict(apply=route["apply"], lpr=route["lpr"], column_chunks_per_lane=-(-(D // 4) // route["lpr"]),
                          grid=[route["apply_grid_x"], route["apply_grid_y"]], long_grid=route["long_grid"]),
               reps=a.reps, method="device events around one apply (chunk kernel + long runs) on the same sorted lists; the two "
                                   "variants alternated per repetition; median / min / max in us", kernels={})
    for name, ts in times.items():
        med = statistics.median(ts)
        res["kernels"][name] = dict(us_median=med, us_min=min(ts), us_max=max(ts), floor_bytes=floors[name],
                                    tb_per_s_at_median=floors[name] / med / 1e6)
    res["adagrad_over_sgd"] = res["kernels"]["rowwise_adagrad"]["us_median"] / res["kernels"]["sgd_all_slots"]["us_median"]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
