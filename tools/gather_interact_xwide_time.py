"""The fused gather at 65 to 128 features (cdlrm_gather_interact_xwide_fwd / _bwd) against the two operators it
replaces, alone, at B = 8192, D = 128, F = 96 and F = 128:
  fused_fwd                     ops.gather_interact_xwide_fwd: the rows read straight into the interaction
  embbag_fwd, xwide_fwd         ops.embbag_fwd (writes the [B, T, D] block) and ops.interact_fwd on it: single launches
  two_fwd                       the two of them behind each other inside one event pair
  fused_bwd / xwide_bwd         ops.gather_interact_xwide_bwd against ops.interact_bwd on the block (x_act = 1, as the step calls them)
The two-operator rows are unchanged code -- the path a run without --fuse-gather-wide takes -- and the first times taken of the
kernels of DESIGN.md 4.12.

The cache holds 4 x 16384 + B rows per table (4.8 GB at 127 tables of D = 128) and every launch draws its slot ids from one of five
id sets in turn, so that a launch does not find its rows where the launch before it left them.  One process, device events
around each version after three warm-up rounds, the versions alternated inside every repetition, median (min - max) reported.
Before anything is timed the fused results are compared bit for bit with the two operators' at the timed size.
Bytes the fusion does not move: B T 4 D written by the gather and read back by the forward, B T 4 D read back by the backward.
NOT measured here: the kernels inside a training step.

    python tools/gather_interact_xwide_time.py [--batch 8192] [--dim 128] [--reps 30] [--out profiles/gather_interact_xwide_times.json]
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
SETS, WAYS, ID_SETS = 16384, 4, 5


def versions(F, B, D, dev, g):
    """{name: (fn(slot ids), bytes it moves)} of one F, and the id sets the launches draw from in turn."""
    T = F - 1
    ctx = ops.CacheCtx([1 << 22] * T, [SETS] * T, D, WAYS, B, dev)
    assert ops.gather_interact_xwide_supported(ctx)
    weight = torch.randn(ctx.total_rows, D, device=dev, generator=g)
    ctx.bind_cache(torch.full((ctx.total_tags,), -1, dtype=torch.int64, device=dev), weight)
    ids = [torch.randint(0, SETS * WAYS + B, (T, B), dtype=torch.int32, device=dev, generator=g) for _ in range(ID_SETS)]
    ld = (D + F * (F - 1) // 2 + 3) & ~3
    feat = torch.rand(B, F, D, device=dev, generator=g)
    R, dR, dfeat = torch.zeros(B, ld, device=dev), torch.rand(B, ld, device=dev, generator=g), torch.zeros(B, F, D, device=dev)
    x, block = feat[:, 0, :], feat[:, 1:, :]
    rows, out = B * T * 4 * D, B * 4 * ld

    def gather(s):
        ops.embbag_fwd(ctx, s, None, block, F * D, D)

    def two(s):
        gather(s)
        ops.interact_fwd(feat, False, R)

    def fused_fwd(s):
        ops.gather_interact_xwide_fwd(ctx, s, x, False, R)

    def fused_bwd(s):
        ops.gather_interact_xwide_bwd(ctx, s, x, dR, False, dfeat, x_act=1)

    def xwide_bwd(s):
        ops.interact_bwd(feat, dR, False, dfeat, x_act=1)
    # results must not differ: the same ids through both paths at the timed size
    two(ids[0])
    R2 = R.clone()
    xwide_bwd(ids[0])
    df2 = dfeat.clone()
    R.zero_()
    dfeat.zero_()
    fused_fwd(ids[0])
    fused_bwd(ids[0])
    assert torch.equal(R, R2) and torch.equal(dfeat, df2), "F = %d: the fused pair differs from the two operators" % F
    return {
        "fused_fwd": (fused_fwd, rows + B * 4 * D + out),
        "embbag_fwd": (gather, 2 * rows),
        "xwide_fwd": (lambda s: ops.interact_fwd(feat, False, R), rows + B * 4 * D + out),
        "two_fwd": (two, 3 * rows + B * 4 * D + out),
        "fused_bwd": (fused_bwd, 2 * (rows + B * 4 * D) + out),
        "xwide_bwd": (xwide_bwd, 2 * (rows + B * 4 * D) + out),
    }, ids


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8192)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", type=str, default=os.path.join("profiles", "gather_interact_xwide_times.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("ERROR: tools/gather_interact_xwide_time.py measures on the MI355X and found no HIP device")
    dev = torch.device("cuda", 0)
    B, D = a.batch, a.dim
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    calls, meta = {}, {}
    for F in (96, 128):
        vs, ids = versions(F, B, D, dev, g)
        for name, (fn, by) in vs.items():
            calls["%s_f%d" % (name, F)] = (fn, ids)
            meta["%s_f%d" % (name, F)] = by
    times = {k: [] for k in calls}
    turn = 0
    for rep in range(a.reps + 3):
        for name, (fn, ids) in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s = ids[turn % ID_SETS]
            turn += 1
            e0.record()
            fn(s)
            e1.record()
            e1.synchronize()
            if rep >= 3:
                times[name].append(e0.elapsed_time(e1) * 1e3)
    res = dict(shape=dict(batch=B, dim=D, cache_rows_per_table=SETS * WAYS + B, id_sets=ID_SETS), reps=a.reps,
               method="device events around each version; versions alternated per repetition; median / min / max in us; two_fwd is "
                      "two launches inside one event pair; fused results compared bit for bit with the two operators' first",
               not_measured=["the kernels inside a training step"], kernels={})
    for name, ts in times.items():
        med = statistics.median(ts)
        res["kernels"][name] = dict(us_median=med, us_min=min(ts), us_max=max(ts), bytes_moved=meta[name],
                                    floor_us_at_8_tb_s=meta[name] / HBM_TB_S / 1e6, share_of_8_tb_s=meta[name] / med / 1e6 / HBM_TB_S)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
