"""Row-wise Adagrad on the cached embedding rows, restated on the oracle's functions.

The contract, per step and per table, for every CACHE-PROPER slot s the batch looks up:

    G [D]  = sum of the gradient rows of all lookups of s, in ascending position order
    i      = the table index resident in s (the oracle's occupancy table: slot = P * way + set, i = occ[set, way])
    S[i]  += (1/D) sum_d G_d^2
    W[s]  -= lr_embeds * G / (sqrt(S[i]) + eps)

Aux slots (the batch's misses) are skipped: no row write, no state update -- their rows are rewritten by the next forward, and the
reference semantics already drop a missed row's update.  S is one fp32 per TABLE row, starts at zero, and is keyed by index: a row
that is evicted and re-inserted finds its accumulator where it left it.

`RowwiseAdagradTrainer` is `OracleTrainer` with one phase of its step replaced: `update_table`, the step of rank r's table k,
which is `rowwise_adagrad_update` here; nothing here imports the package under test.  `kernel_reference` / `kernel_bounds` are the float64 reference and the bounds the kernel tests hold
the HIP kernels to (and the host tests hold wrong variants of the update to: they must fail them).
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from oracle import cdlrm_oracle as O  # noqa: E402

U = 2.0 ** -24


def slot_index(occ: torch.Tensor, P: int, slots: torch.Tensor) -> torch.Tensor:
    """Table index resident in each cache-proper slot (slot = P * way + set; probe_table, model_no_ddp.py:174)."""
    return occ[slots % P, slots // P]


def rowwise_adagrad_update(weight, state, occ, P, slots, offsets, grad_out, lr, eps, *, variant="rowwise"):
    """The update of one table, fp32, duplicates summed in ascending position order (index_add_, as the oracle's SGD).
    variant: "rowwise" is the contract; the others are the WRONG updates the host tests use as controls --
    "sum" (S += sum instead of mean), "no_accumulate" (S = this step's mean alone), "elementwise" (needs state [n, D])."""
    slots = slots.to(torch.int64)
    ways = occ.shape[1]
    b = O.bag_ids(offsets, slots.shape[0])
    g = grad_out[b]
    u, inv = torch.unique(slots, return_inverse=True)
    acc = torch.zeros(u.shape[0], weight.shape[1], dtype=weight.dtype)
    acc.index_add_(0, inv, g)
    keep = u < P * ways                     # aux slots: skipped
    u, acc = u[keep], acc[keep]
    if u.numel() == 0:
        return
    i = slot_index(occ, P, u)
    assert bool((i >= 0).all()) and i.unique().numel() == i.numel(), "a looked-up slot holds one index, an index one slot"
    if variant == "elementwise":
        S = state[i] + acc * acc
        state[i] = S
        weight[u] = weight[u] - lr * acc / (S.sqrt() + eps)
        return
    sq = (acc * acc).sum(dim=1) if variant == "sum" else (acc * acc).mean(dim=1)
    S = sq if variant == "no_accumulate" else state[i] + sq
    state[i] = S
    weight[u] = weight[u] - lr * acc / (S.sqrt() + eps).unsqueeze(1)


class RowwiseAdagradTrainer(O.OracleTrainer):
    """OracleTrainer (one rank, no victim write-back: as the engine refuses) whose update_table phase is row-wise Adagrad;
    `state[k]`: table k's n_k accumulators, in the trainer's dtype."""

    def __init__(self, *a, adagrad_eps=1e-10, variant="rowwise", **kw):
        super().__init__(*a, **kw)
        assert self.W == 1 and not self.evict_victim
        self.eps, self.variant = float(adagrad_eps), variant
        D = self.weights[0][0].shape[1]
        self.state = [torch.zeros((n, D) if variant == "elementwise" else (n,), dtype=self.dtype) for n in self.ln_emb]

    def update_table(self, r, k, slots, offsets, grad_out):
        rowwise_adagrad_update(self.weights[r][k], self.state[k], self.occ[k], int(self.cache_sizes[k]), slots, offsets, grad_out,
                               self.lr_embeds, self.eps, variant=self.variant)


# ---- what the kernel tests compare with -------------------------------------------------------------------------------------

def kernel_reference(W0, S0, G, lr, eps):
    """float64: (S, W, step) of rows W0 [R, D] with accumulators S0 [R] and run sums G [R, D]."""
    G = G.astype(np.float64)
    S = S0.astype(np.float64) + (G * G).mean(axis=1)
    step = lr * G / (np.sqrt(S) + eps)[:, None]
    return S, W0.astype(np.float64) - step, step


def kernel_bounds(S64, W64, step64, D):
    """|S - S64| <= (D + 4) u S64: a sum of D + 1 non-negative terms in any order, the squares, the division by D.
    |W - W64| <= (D/2 + 16) u |step| + u |W64|: the sqrt halves the sum's relative error; 16 u covers sqrt, add, divide,
    multiply and the final fma, hardware approximations included."""
    return (D + 4) * U * S64, (D / 2 + 16) * U * np.abs(step64) + U * np.abs(W64)


def kernel_check(S, W, S0, W0, G, lr, eps, what=""):
    """Raises AssertionError unless accumulators S [R] and rows W [R, D] are within kernel_bounds of the reference."""
    D = W0.shape[1]
    S64, W64, step = kernel_reference(W0, S0, G, lr, eps)
    bS, bW = kernel_bounds(S64, W64, step, D)
    dS, dW = np.abs(S.astype(np.float64) - S64), np.abs(W.astype(np.float64) - W64)
    if not (dS <= bS).all():
        r = int(np.argmax(dS - bS))
        raise AssertionError("%s accumulator %d: got %r, float64 %r, |diff| %.3g > bound %.3g" % (what, r, S[r], S64[r], dS[r], bS[r]))
    if not (dW <= bW).all():
        r, c = np.unravel_index(int(np.argmax(dW - bW)), dW.shape)
        raise AssertionError("%s row %d col %d: got %r, float64 %r, |diff| %.3g > bound %.3g"
                             % (what, r, c, W[r, c], W64[r, c], dW[r, c], bW[r, c]))
    return float((dS / np.maximum(bS, 1e-300)).max()), float((dW / np.maximum(bW, 1e-300)).max())


def criteo_batches(ln_emb, n_dense, B, nbatch, seed, heavy=(), alpha=1.2):
    """[(X [B, n_dense], idx int64 [T, B], T [B, 1])]: Zipf(alpha) indices scattered over each table; tables in `heavy` draw
    from five indices only (long runs of one slot).  The stream the host and the GPU tests of a mode share."""
    rng = np.random.RandomState(seed)
    out = []
    for _ in range(nbatch):
        X = torch.from_numpy(rng.rand(B, n_dense).astype(np.float32))
        cols = []
        for k, n in enumerate(ln_emb):
            z, n = rng.zipf(alpha, size=B).astype(np.int64), int(n)
            cols.append(torch.from_numpy((z % 5) * 7 % n if k in heavy else z * 2654435761 % n))
        T = torch.from_numpy(np.round(rng.rand(B, 1)).astype(np.float32))
        out.append((X, torch.stack(cols), T))
    return out
