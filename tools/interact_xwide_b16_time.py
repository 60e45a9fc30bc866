"""The bf16 / bf16x3 dot interaction at 65 to 128 features (cdlrm_interact_xwide_b16_fwd / _bwd) against the fp32
kernels it stands in for (cdlrm_interact_xwide_fwd / _bwd, unchanged code), alone, at B = 8192, D = 128, F = 96 and F = 128: each
of the two kernels in fp32, bf16 and bf16x3 through ops.interact_fwd / ops.interact_bwd (x_act = 1, as the step calls them).

The method of tools/gather_interact_xwide_time.py: one process, device events around single launches, the versions alternated
inside every repetition, three warm-up rounds, median (min - max) reported.  The [B, F, D] block (403 / 537 MB) is larger than the
256 MB the last-level cache holds, so no launch finds its rows where the launch before it left them.  Before anything is timed the
results of both modes are compared with the fp32 kernels' at the timed size: the largest |difference| over the largest |fp32
value| is recorded (bf16x3 must stay below 2^-12, bf16 below 2^-4: a wrong kernel, not rounding, is what this stops).
Beside each time: the bytes the kernel moves and their floor at 8 TB/s, and its MFMA count per sample -- matrix time is arithmetic
from these, not a measurement.  NOT measured here: the kernels inside a training step, other D or B.

    python tools/interact_xwide_b16_time.py [--batch 8192] [--dim 128] [--reps 30] [--out profiles/interact_xwide_b16_times.json]
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
PRECISIONS = ("fp32", "bf16", "bf16x3")


def mfmas_per_sample(kernel, prec, F, D):
    """Matrix instructions one sample costs: v_mfma_f32_32x32x2_f32 (fp32) or v_mfma_f32_32x32x16_bf16, by the kernels' tile walks."""
    nb, slabs = (F + 31) // 32, (D + 31) // 32
    blocks = nb * (nb + 1) // 2 if kernel == "fwd" else nb          # 32 x 32 output blocks per slab
    depth = 32 if kernel == "fwd" else 32 * nb                      # contraction indices per slab
    steps = depth // 2 if prec == "fp32" else depth // 16
    return blocks * slabs * steps * (3 if prec == "bf16x3" else 1)


def versions(F, B, D, dev, g):
    ld = (D + F * (F - 1) // 2 + 3) & ~3
    feat = torch.rand(B, F, D, device=dev, generator=g) - 0.25
    dR = torch.rand(B, ld, device=dev, generator=g) - 0.5
    R = {p: torch.zeros(B, ld, device=dev) for p in PRECISIONS}
    dfeat = {p: torch.zeros(B, F, D, device=dev) for p in PRECISIONS}
    block, out = B * F * D * 4, B * ld * 4
    calls, err = {}, {}
    for p in PRECISIONS:
        calls["fwd_" + p] = (lambda p=p: ops.interact_fwd(feat, False, R[p], precision=p), block + out)
        calls["bwd_" + p] = (lambda p=p: ops.interact_bwd(feat, dR, False, dfeat[p], x_act=1, precision=p), 2 * block + out)
    for fn, _ in calls.values():
        fn()
    torch.cuda.synchronize()
    for p, lim in (("bf16", 2.0 ** -4), ("bf16x3", 2.0 ** -12)):
        for k, bufs in (("fwd", R), ("bwd", dfeat)):
            e = float((bufs[p] - bufs["fp32"]).abs().max() / bufs["fp32"].abs().max())
            assert e < lim, "F = %d: %s %s differs from fp32 by %g of the largest value" % (F, k, p, e)
            err["%s_%s" % (k, p)] = e
    return calls, err


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8192)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", type=str, default=os.path.join("profiles", "interact_xwide_b16_times.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("ERROR: tools/interact_xwide_b16_time.py measures on the MI355X and found no HIP device")
    dev = torch.device("cuda", 0)
    B, D = a.batch, a.dim
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    calls, meta, errs = {}, {}, {}
    for F in (96, 128):
        vs, err = versions(F, B, D, dev, g)
        for name, (fn, by) in vs.items():
            calls["%s_f%d" % (name, F)] = fn
            kernel, prec = name.split("_")
            meta["%s_f%d" % (name, F)] = (by, mfmas_per_sample(kernel, prec, F, D))
        errs.update({"%s_f%d" % (k, F): v for k, v in err.items()})
    times = {k: [] for k in calls}
    for rep in range(a.reps + 3):
        for name, fn in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if rep >= 3:
                times[name].append(e0.elapsed_time(e1) * 1e3)
    res = dict(shape=dict(batch=B, dim=D), reps=a.reps,
               method="device events around single launches; versions alternated per repetition; three warm-up rounds; median / min / "
                      "max in us; both modes compared with the fp32 results at the timed size first",
               not_measured=["the kernels inside a training step", "other D or B"], max_diff_over_max_fp32=errs, kernels={})
    for name, ts in times.items():
        med = statistics.median(ts)
        by, mf = meta[name]
        res["kernels"][name] = dict(us_median=med, us_min=min(ts), us_max=max(ts), bytes_moved=by, floor_us_at_8_tb_s=by / HBM_TB_S / 1e6,
                                    share_of_8_tb_s=by / med / 1e6 / HBM_TB_S, mfmas_per_sample=mf)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
