"""Multi-hot bags pooled inside the interaction kernels (csrc/bag_interact.hip) against the two operators they replace, alone,
at B = 8192, T = 26, D = 128: (a) embbag_fwd + interact_fwd, (b) bag_interact_fwd, (c) interact_bwd on the pooled block,
(d) bag_interact_bwd -- once with seeded bag lengths uniform in 1..8, once with every bag one lookup long.

Device events around each version after three warm-up rounds, the versions alternated inside every repetition, median / min /
max reported.  The rows come from a cache far larger than the Infinity Cache (slots uniform over it).  Algorithmic bytes: the
looked-up rows + slot ids + offsets + dense feature + output row (forward), the same + the dR row read with dfeat as the
output (backward); the two-operator path moves the pooled block on top of them, which is not counted.

    python tools/bag_interact_time.py [--batch 8192] [--tables 26] [--dim 128] [--sets 32771] [--reps 30]
                                      [--out profiles/bag_interact_times.json]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cdlrm_amd import ops  # noqa: E402

HBM_TB_S = 8.0


def measure(ctx, B, T, D, ways, sets, lens, reps, dev, g):
    # tables are ragged against each other: squared off with one scratch bag behind the batch (engine.square_bags' layout)
    off = torch.zeros(T, B + 1, dtype=torch.int64)
    off[:, 1:] = torch.cumsum(lens, dim=1)
    n = int(off[:, B].max())
    off = off.to(dev)
    slots = torch.randint(0, ways * sets, (T, n), device=dev, generator=g, dtype=torch.int32)
    F = T + 1
    width = D + F * (F - 1) // 2
    ld_r = (width + 3) & ~3
    feat = torch.zeros(B + 1, F, D, device=dev)[:B]
    feat[:, 0, :] = torch.rand(B, D, device=dev, generator=g)
    x = feat[:, 0, :]
    R, R2 = torch.zeros(B, ld_r, device=dev), torch.zeros(B, ld_r, device=dev)
    dR = torch.rand(B, ld_r, device=dev, generator=g)
    dfeat, dfeat2 = torch.zeros(B, F, D, device=dev), torch.zeros(B, F, D, device=dev)
    ld = feat.stride(0)

    def two_fwd():
        ops.embbag_fwd(ctx, slots, off, feat[:, 1:, :], ld, D, n_bags=B + 1)
        ops.interact_fwd(feat, False, R)

    calls = {
        "two_operators_fwd": two_fwd,
        "bag_interact_fwd": lambda: ops.bag_interact_fwd(ctx, slots, off, x, False, R2),
        "interact_bwd": lambda: ops.interact_bwd(feat, dR, False, dfeat, x_act=1),
        "bag_interact_bwd": lambda: ops.bag_interact_bwd(ctx, slots, off, x, dR, False, dfeat2, x_act=1),
    }
    times = {k: [] for k in calls}
    for rep in range(reps + 3):
        for name, fn in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if rep >= 3:
                times[name].append(e0.elapsed_time(e1) * 1e3)
    ctx.check()
    assert torch.equal(R, R2) and torch.equal(dfeat, dfeat2), "the fused kernels are bit-identical to the two operators"
    lookups = int(lens.sum())
    common = lookups * D * 4 + lookups * 4 + T * (B + 1) * 8 + B * D * 4
    bytes_of = {"fwd": common + B * ld_r * 4, "bwd": common + B * ld_r * 4 + B * F * D * 4}
    out = dict(lookups=lookups, longest_bag=int(lens.max()), algorithmic_bytes=bytes_of, kernels={})
    for name, ts in times.items():
        med = statistics.median(ts)
        by = bytes_of["fwd" if name.endswith("fwd") else "bwd"]
        out["kernels"][name] = dict(us_median=med, us_min=min(ts), us_max=max(ts), share_of_8_tb_s=by / med / 1e6 / HBM_TB_S)
    k = out["kernels"]
    out["fused_over_two_operators_fwd"] = k["bag_interact_fwd"]["us_median"] / k["two_operators_fwd"]["us_median"]
    out["fused_over_interact_bwd"] = k["bag_interact_bwd"]["us_median"] / k["interact_bwd"]["us_median"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8192)
    ap.add_argument("--tables", type=int, default=26)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--sets", type=int, default=32771)
    ap.add_argument("--ways", type=int, default=4)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", type=str, default=os.path.join("profiles", "bag_interact_times.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("ERROR: tools/bag_interact_time.py measures on the MI355X and found no HIP device")
    dev = torch.device("cuda", 0)
    B, T, D = a.batch, a.tables, a.dim
    ctx = ops.CacheCtx([a.sets * 64] * T, [a.sets] * T, D, a.ways, B, dev)
    if not ops.bag_interact_supported(ctx):
        sys.exit("ERROR: no fused bag kernel at D = %d, T = %d" % (D, T))
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    tags = torch.full((ctx.total_tags,), -1, dtype=torch.int64, device=dev)
    W = torch.rand(ctx.total_rows, D, device=dev, generator=g)
    ctx.bind_cache(tags, W)
    hg = torch.Generator()
    hg.manual_seed(2)
    res = dict(shape=dict(batch=B, tables=T, dim=D, cache_rows=int(ctx.total_rows), cache_gb=ctx.total_rows * D * 4 / 1e9),
               reps=a.reps, unroll=ops.BAG_INTERACT_U,
               method="device events around each version; versions alternated per repetition; median / min / max in us",
               lengths_1_to_8=measure(ctx, B, T, D, a.ways, a.sets, torch.randint(1, 9, (T, B), generator=hg), a.reps, dev, g),
               length_1=measure(ctx, B, T, D, a.ways, a.sets, torch.ones(T, B, dtype=torch.int64), a.reps, dev, g))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
