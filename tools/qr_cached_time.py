"""The three kernels of the cached quotient-remainder path (csrc/qr_cached.hip) alone, at c4's step shape (B = 8192, T = 26,
D = 256, c = 4), against their byte floors and against cdlrm_embbag_fwd on the same slots.

Device events around single launches, the variants alternated inside every repetition, medians reported.  The rows come from
a cache far larger than the Infinity Cache (slots uniform over it); the feature block (226 MB) is the step's own.  Byte floors
count the rows, the feature / gradient rows and nothing else (slot ids, remainders and Wr are < 1 % of them).

    python tools/qr_cached_time.py [--batch 8192] [--tables 26] [--dim 256] [--collisions 4] [--sets 32771] [--reps 30]
                                   [--out profiles/qr_cached_c4.json]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cdlrm_amd import ops  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8192)
    ap.add_argument("--tables", type=int, default=26)
    ap.add_argument("--dim", type=int, default=256)
    ap.add_argument("--collisions", type=int, default=4)
    ap.add_argument("--sets", type=int, default=32771)
    ap.add_argument("--ways", type=int, default=4)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", type=str, default=os.path.join("profiles", "qr_cached_c4.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("ERROR: tools/qr_cached_time.py measures on the MI355X and found no HIP device")
    dev = torch.device("cuda", 0)
    B, T, D, c = a.batch, a.tables, a.dim, a.collisions
    ctx = ops.CacheCtx([a.sets * 64] * T, [a.sets] * T, D, a.ways, B, dev, aux_phases=2)
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    tags = torch.full((ctx.total_tags,), -1, dtype=torch.int64, device=dev)
    W = torch.rand(ctx.total_rows, D, device=dev, generator=g)
    ctx.bind_cache(tags, W)
    slots = torch.randint(0, a.ways * a.sets, (T, B), device=dev, generator=g, dtype=torch.int32)
    r = torch.randint(0, c, (T, B), device=dev, generator=g).to(torch.uint8)
    coll = torch.full((T,), c, dtype=torch.int32, device=dev)
    Wr0 = torch.rand(T, c, D, device=dev, generator=g)
    Wr = Wr0.clone()
    feat = torch.zeros(B + 1, T + 1, D, device=dev)[:B]
    dfeat0 = torch.rand(B, T + 1, D, device=dev, generator=g)
    dfeat = dfeat0.clone()
    work = ops.qr_cached_bwd_work(ctx, B, c)
    ld = feat.stride(0)

    calls = {
        "embbag_fwd": lambda: ops.embbag_fwd(ctx, slots, None, feat[:, 1:, :], ld, D),
        "qr_cached_fwd_mult": lambda: ops.qr_cached_fwd(ctx, slots, r, Wr, coll, 0, feat[:, 1:, :], ld, D),
        "qr_cached_fwd_add": lambda: ops.qr_cached_fwd(ctx, slots, r, Wr, coll, 1, feat[:, 1:, :], ld, D),
        "qr_cached_bwd_mult": lambda: ops.qr_cached_bwd(ctx, slots, r, Wr, coll, 0, dfeat[:, 1:, :], ld, D, work),
        "qr_cached_bwd_add": lambda: ops.qr_cached_bwd(ctx, slots, r, Wr, coll, 1, dfeat[:, 1:, :], ld, D, work),
        "qr_cached_bwd_finish": lambda: ops.qr_cached_bwd_finish(ctx, coll, B, work, 0.0, Wr),
    }
    rows = T * B * D * 4
    floors = {      # bytes the algorithm has to move
        "embbag_fwd": 2 * rows, "qr_cached_fwd_mult": 2 * rows, "qr_cached_fwd_add": 2 * rows,
        "qr_cached_bwd_mult": 3 * rows,                 # gradient rows read and written, cache rows read
        "qr_cached_bwd_add": rows,                      # gradient rows read
        "qr_cached_bwd_finish": work.numel() * 4 + 2 * Wr.numel() * 4,
    }
    times = {k: [] for k in calls}
    for rep in range(a.reps + 3):
        for name, fn in calls.items():
            if name.startswith("qr_cached_bwd_m"):     # (the in-place product would shrink the gradient rows towards denormals)
                dfeat.copy_(dfeat0)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if rep >= 3:                                # three warm-up rounds of every variant
                times[name].append(e0.elapsed_time(e1) * 1e3)
    ctx.check()
    res = dict(shape=dict(batch=B, tables=T, dim=D, collisions=c, cache_rows=int(ctx.total_rows), cache_gb=ctx.total_rows * D * 4 / 1e9),
               reps=a.reps, method="device events around one launch; variants alternated per repetition; median / min / max in us",
               kernels={})
    for name, ts in times.items():
        med = statistics.median(ts)
        res["kernels"][name] = dict(us_median=med, us_min=min(ts), us_max=max(ts), floor_bytes=floors[name],
                                    tb_per_s_at_median=floors[name] / med / 1e6)
    res["qr_fwd_over_embbag_fwd"] = res["kernels"]["qr_cached_fwd_mult"]["us_median"] / res["kernels"]["embbag_fwd"]["us_median"]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
