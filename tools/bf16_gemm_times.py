"""Per-GEMM times of the bf16 mode (CDLRM_GEMM_BF16) and the bf16x3 mode (CDLRM_GEMM_BF16X3) against the fp32 route the
training step takes, at the c3 (M = 8192) and c5 (M = 65536) layer shapes: forward (bias + ReLU), dgrad (x_act ReLU),
weight gradient + bias gradient with its slab reduction (ops.mlp_wgrad, one layer).  Torch events around 50 back-to-back
launches after 5 warm-up ones, microseconds.  alone: the CDLRM_GEMM_ALONE hint the step gives the top MLP's forward and
dgrad chain.  Run from the repository root on the GPU:
    python tools/bf16_gemm_times.py"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cdlrm_amd import ops  # noqa: E402

dev = "cuda:0"


def t(fn, reps=50):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1000 / reps


for M in (8192, 65536):
    for (N, K, alone) in [(512, 480, True), (512, 512, True), (256, 512, True), (256, 512, False), (128, 256, False)]:
        X = torch.randn(M, K, device=dev)
        W = torch.randn(N, K, device=dev) / 20
        b = torch.randn(N, device=dev)
        Y = torch.empty(M, N, device=dev)
        dY = torch.randn(M, N, device=dev)
        dX = torch.empty(M, K, device=dev)
        dW = torch.empty(N, K, device=dev)
        db = torch.empty(N, device=dev)
        work = ops.linear_bwd_work(M, N, K, dev)
        plan = {p: ops.WgradPlan([X], [dY], [dW], [db], ops.mlp_wgrad_work(M, [N], [K], dev, precision=p), precision=p)
                for p in ("fp32", "bf16", "bf16x3")}
        row = []
        for p in ("fp32", "bf16", "bf16x3"):
            f = t(lambda: ops.linear_fwd(X, W, b, Y, 1, alone=alone, precision=p))
            d = t(lambda: ops.linear_bwd(X, W, None, dY, dX, None, None, 0, work, x_act=1, alone=alone, precision=p))
            w = t(lambda: ops.mlp_wgrad(plan[p]))
            row.append((f, d, w))
        print("M=%d %dx%d alone=%d  fwd %.1f / %.1f / %.1f  dgrad %.1f / %.1f / %.1f  wgrad+db %.1f / %.1f / %.1f  "
              "(fp32 / bf16 / bf16x3 us)" % ((M, N, K, alone) + tuple(row[p][g] for g in range(3) for p in range(3))), flush=True)
