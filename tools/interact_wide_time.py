"""The dot interaction at 33 to 64 features (csrc/interact_wide.hip) alone, at B = 8192, D = 128, F = 40 and F = 64:
  wide_fwd / wide_bwd           ops.interact_fwd / interact_bwd on the wide kernels (x_act = 1, as the step calls them)
  wide_fwd_1wg                  the forward with ONE workgroup per CU (development key 4) instead of two
  narrow_fwd / narrow_bwd       k_interact_fwd_s / k_interact_bwd_s at F = 32 on the same D: the yardstick per MFMA of useful work
  torch_fwd / torch_fwd_bwd     torch.bmm + tril gather and its autograd backward: a yardstick only (the vendor GEMM; tools only)

One process, device events around single launches after three warm-up rounds, the versions alternated inside every repetition,
median (min - max) reported.  Byte floor: B * (4 F D + 4 ld_r) forward, + B * 4 F D (dfeat) backward, at 8 TB/s.  Useful matrix
work: the lower triangle's 32x32x2 blocks -- 3 x D / 2 forward at 32 < F <= 64 (96 of the 16x16x4 form = 48 of these at F = 32),
F-independent; backward 2 x 32 x D / 32 (F = 32: 16 x D / 32).
NOT measured here: the kernels inside a training step.

    python tools/interact_wide_time.py [--batch 8192] [--dim 128] [--reps 30] [--out profiles/interact_wide_times.json]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cdlrm_amd import _lib, ops  # noqa: E402

HBM_TB_S = 8.0


def operands(B, F, D, dev, g):
    width = D + F * (F - 1) // 2
    ld = (width + 3) & ~3
    feat = torch.rand(B, F, D, device=dev, generator=g)
    return dict(F=F, ld=ld, feat=feat, R=torch.zeros(B, ld, device=dev), dR=torch.rand(B, ld, device=dev, generator=g),
                dfeat=torch.zeros(B, F, D, device=dev))


def torch_interact(feat, li, lj):
    Z = torch.bmm(feat, feat.transpose(1, 2))
    return torch.cat([feat[:, 0], Z[:, li, lj]], dim=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8192)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", type=str, default=os.path.join("profiles", "interact_wide_times.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("ERROR: tools/interact_wide_time.py measures on the MI355X and found no HIP device")
    dev = torch.device("cuda", 0)
    B, D = a.batch, a.dim
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    L = _lib.raw()
    L.cdlrm_debug_set.argtypes = [ctypes.c_int32, ctypes.c_int32]
    calls, meta = {}, {}
    for F in (32, 40, 64):
        o = operands(B, F, D, dev, g)
        tag = "narrow" if F == 32 else "wide"
        fwd_bytes = B * (4 * F * D + 4 * o["ld"])
        mfma_fwd = 48 * D // 128 if F == 32 else 3 * D // 2       # 32x32x2 equivalents per sample (F = 32: 3 D / 4 steps of 16x16x4)
        mfma_bwd = (16 if F == 32 else 64) * D // 32
        calls["%s_fwd_f%d" % (tag, F)] = lambda o=o: ops.interact_fwd(o["feat"], False, o["R"])
        meta["%s_fwd_f%d" % (tag, F)] = (fwd_bytes, mfma_fwd)
        calls["%s_bwd_f%d" % (tag, F)] = lambda o=o: ops.interact_bwd(o["feat"], o["dR"], False, o["dfeat"], x_act=1)
        meta["%s_bwd_f%d" % (tag, F)] = (fwd_bytes + B * 4 * F * D, mfma_bwd)
        if F == 32:
            continue

        def one_wg(o=o):
            L.cdlrm_debug_set(4, 1)
            ops.interact_fwd(o["feat"], False, o["R"])
            L.cdlrm_debug_set(4, 0)
        calls["wide_fwd_1wg_f%d" % F] = one_wg
        meta["wide_fwd_1wg_f%d" % F] = (fwd_bytes, mfma_fwd)
        li, lj = torch.tril_indices(F, F, -1, device=dev)
        ft = o["feat"].clone().requires_grad_(True)
        calls["torch_fwd_f%d" % F] = lambda o=o, li=li, lj=lj: torch_interact(o["feat"], li, lj)
        meta["torch_fwd_f%d" % F] = (fwd_bytes, mfma_fwd)

        def torch_fb(ft=ft, o=o, li=li, lj=lj, F=F):
            ft.grad = None
            torch_interact(ft, li, lj).backward(o["dR"][:, :D + F * (F - 1) // 2])
        calls["torch_fwd_bwd_f%d" % F] = torch_fb
        meta["torch_fwd_bwd_f%d" % F] = (2 * fwd_bytes + B * 4 * F * D, mfma_fwd + mfma_bwd)
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
               method="device events around each version; versions alternated per repetition; median / min / max in us; the torch "
                      "rows are several launches each",
               not_measured=["the kernels inside a training step"], kernels={})
    for name, ts in times.items():
        med = statistics.median(ts)
        by, mf = meta[name]
        res["kernels"][name] = dict(us_median=med, us_min=min(ts), us_max=max(ts), floor_bytes=by, floor_us_at_8_tb_s=by / HBM_TB_S / 1e6,
                                    share_of_8_tb_s=by / med / 1e6 / HBM_TB_S, mfma_32x32x2_per_sample=mf,
                                    ns_per_useful_mfma=med * 1e3 / (B * mf))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
