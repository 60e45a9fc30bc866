"""The quotient-remainder compose inside the interaction kernels (csrc/qr_interact.hip) against the operators it replaces, alone,
at c4's step shape (B = 8192, T = 26, D = 256, c = 4), for both operations:
  (a) qr_cached_fwd + interact_fwd            (b) qr_interact_fwd
  (c) gather_interact_fwd on the same slots -- the plain fused forward: the yardstick for what the compose costs
  (d) interact_bwd with the composed block at hand        (e) qr_interact_bwd

Device events around each version after three warm-up rounds, the versions alternated inside every repetition, median / min /
max reported.  The rows come from a cache far larger than the Infinity Cache (slots uniform over it; the cache of
tools/qr_cached_time.py).  Byte floors: forward lookups * (4 D + 5) + B * 4 D + the output rows; backward the same + the dR rows
read, with dfeat as the output.  The two-operator path moves the composed block on top of them, which is not counted.
NOT measured here: the kernels inside a training step, and a full-size c4 run.

    python tools/qr_interact_time.py [--batch 8192] [--tables 26] [--dim 256] [--collisions 4] [--sets 32771] [--reps 30]
                                     [--out profiles/qr_interact_c4.json]
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


def measure(ctx, B, T, D, c, op, slots, reps, dev, g):
    F = T + 1
    width = D + F * (F - 1) // 2
    ld_R = (width + 3) & ~3
    r = torch.randint(0, c, (T, B), device=dev, generator=g).to(torch.uint8)
    coll = torch.full((T,), c, dtype=torch.int32, device=dev)
    Wr = torch.rand(T, c, D, device=dev, generator=g) + 0.5
    feat = torch.zeros(B + 1, F, D, device=dev)[:B]
    feat[:, 0, :] = torch.rand(B, D, device=dev, generator=g)
    x = feat[:, 0, :]
    R, R2, R3 = (torch.zeros(B, ld_R, device=dev) for _ in range(3))
    dR = torch.rand(B, ld_R, device=dev, generator=g)
    dfeat, dfeat2 = torch.zeros(B, F, D, device=dev), torch.zeros(B, F, D, device=dev)
    ld = feat.stride(0)

    def two_fwd():
        ops.qr_cached_fwd(ctx, slots, r, Wr, coll, op, feat[:, 1:, :], ld, D)
        ops.interact_fwd(feat, False, R)

    calls = {
        "two_operators_fwd": two_fwd,
        "qr_interact_fwd": lambda: ops.qr_interact_fwd(ctx, slots, r, Wr, coll, op, x, False, R2),
        "gather_interact_fwd": lambda: ops.gather_interact_fwd(ctx, slots, x, False, R3),
        "interact_bwd": lambda: ops.interact_bwd(feat, dR, False, dfeat, x_act=1),
        "qr_interact_bwd": lambda: ops.qr_interact_bwd(ctx, slots, r, Wr, coll, op, x, dR, False, dfeat2, x_act=1),
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
    lookups = T * B
    fwd = lookups * (4 * D + 5) + B * 4 * D + B * ld_R * 4
    floors = {"fwd": fwd, "bwd": fwd + B * F * D * 4}
    out = dict(floor_bytes=floors, composed_block_bytes=lookups * 4 * D, kernels={})
    for name, ts in times.items():
        med = statistics.median(ts)
        by = floors["fwd" if name.endswith("fwd") else "bwd"]
        out["kernels"][name] = dict(us_median=med, us_min=min(ts), us_max=max(ts), share_of_8_tb_s=by / med / 1e6 / HBM_TB_S)
    k = out["kernels"]
    out["b_over_a"] = k["qr_interact_fwd"]["us_median"] / k["two_operators_fwd"]["us_median"]
    out["b_over_c"] = k["qr_interact_fwd"]["us_median"] / k["gather_interact_fwd"]["us_median"]
    out["e_over_d"] = k["qr_interact_bwd"]["us_median"] / k["interact_bwd"]["us_median"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8192)
    ap.add_argument("--tables", type=int, default=26)
    ap.add_argument("--dim", type=int, default=256)
    ap.add_argument("--collisions", type=int, default=4)
    ap.add_argument("--sets", type=int, default=32771)
    ap.add_argument("--ways", type=int, default=4)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", type=str, default=os.path.join("profiles", "qr_interact_c4.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("ERROR: tools/qr_interact_time.py measures on the MI355X and found no HIP device")
    dev = torch.device("cuda", 0)
    B, T, D, c = a.batch, a.tables, a.dim, a.collisions
    ctx = ops.CacheCtx([a.sets * 64] * T, [a.sets] * T, D, a.ways, B, dev, aux_phases=2)
    if not ops.qr_interact_supported(ctx):
        sys.exit("ERROR: no fused QR kernel at D = %d, T = %d" % (D, T))
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    tags = torch.full((ctx.total_tags,), -1, dtype=torch.int64, device=dev)
    W = torch.rand(ctx.total_rows, D, device=dev, generator=g)
    ctx.bind_cache(tags, W)
    slots = torch.randint(0, a.ways * a.sets, (T, B), device=dev, generator=g, dtype=torch.int32)
    res = dict(shape=dict(batch=B, tables=T, dim=D, collisions=c, cache_rows=int(ctx.total_rows), cache_gb=ctx.total_rows * D * 4 / 1e9),
               reps=a.reps, method="device events around each version; versions alternated per repetition; median / min / max in us",
               not_measured=["the kernels inside a training step", "a full-size c4 run"],
               mult=measure(ctx, B, T, D, c, 0, slots, a.reps, dev, g), add=measure(ctx, B, T, D, c, 1, slots, a.reps, dev, g))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
