"""Element-wise Adagrad on the MLP parameters, restated on the oracle's functions.

The contract, per step and per dense parameter element, with g the gradient the SGD path would apply (weights: averaged over
the ranks; biases: the rank's own, un-reduced):

    S += g * g
    p -= lr * g / (sqrt(S) + eps)

torch.optim.Adagrad with lr_decay = 0, weight_decay = 0, initial_accumulator_value = 0.  S is one fp32 per parameter, per rank,
zero at the start.  g = 0 on S = 0 leaves p unchanged (0 / eps).

`DenseAdagradTrainer` is `OracleTrainer` with one phase of its step replaced: `dense_step`, the update of one dense parameter
behind the weight-only gradient average.  `BothAdagradTrainer` composes it with the row-wise Adagrad of the cached embedding
rows (tests/rowwise_adagrad_restated.py), the engine's dense_optimizer="adagrad" with embed_optimizer="rowwise_adagrad".
Nothing here imports the package under test.  `kernel_reference` / `kernel_bounds` are the float64 reference and the bounds
the kernel tests hold the HIP kernels to (and the host tests hold the wrong variants to: they must fail them).
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from oracle import cdlrm_oracle as O  # noqa: E402
from rowwise_adagrad_restated import RowwiseAdagradTrainer, criteo_batches  # noqa: E402

U = 2.0 ** -24
VARIANTS = ("contract", "no_accumulate", "eps_inside", "rowwise_mean")


def adagrad_update(p, S, g, lr, eps, variant="contract"):
    """(p, S) after one step, in p's dtype.  variant: "contract", or one of the WRONG updates the host tests use as controls --
    "no_accumulate" (S = this step's g * g alone), "eps_inside" (sqrt(S + eps)), "rowwise_mean" (one accumulator value per row
    of a matrix: the mean of the row's g * g)."""
    sq = g * g
    if variant == "rowwise_mean" and g.dim() == 2:
        sq = sq.mean(dim=1, keepdim=True).expand_as(g)
    S = sq if variant == "no_accumulate" else S + sq
    std = (S + eps).sqrt() if variant == "eps_inside" else S.sqrt() + eps
    return p - lr * g / std, S


class DenseAdagradTrainer(O.OracleTrainer):
    """OracleTrainer whose MLP parameters take Adagrad steps: the dense_step phase replaced, with rank r's accumulators beside
    the parameters (dense_state).  dtype=torch.float64 runs the same sequence in double precision."""

    def __init__(self, *a, dense_adagrad_eps=1e-10, dense_variant="contract", **kw):
        super().__init__(*a, **kw)
        assert dense_variant in VARIANTS
        self._dense_eps, self._dense_variant = float(dense_adagrad_eps), dense_variant
        # [r][part][li] like the parameters: part 0..3 = bot W, bot b, top W, top b
        self._dense_S = [[[torch.zeros_like(t) for t in ts] for ts in self.bot[r] + self.top[r]] for r in range(self.W)]

    def dense_step(self, r, part, li, p):
        p2, S2 = adagrad_update(p.detach(), self._dense_S[r][part][li], p.grad, self.lr, self._dense_eps, self._dense_variant)
        self._dense_S[r][part][li] = S2.detach()
        return p2.detach()

    def dense_params(self, r=0):
        """Rank r's dense parameters as one flat vector: all weights (bottom, then top), then all biases."""
        return torch.cat([t.reshape(-1) for t in self.bot[r][0] + self.top[r][0] + self.bot[r][1] + self.top[r][1]])

    def dense_state(self, r=0):
        s = self._dense_S[r]
        return torch.cat([t.reshape(-1) for t in s[0] + s[2] + s[1] + s[3]])


class BothAdagradTrainer(RowwiseAdagradTrainer, DenseAdagradTrainer):
    """Row-wise Adagrad on the cached rows (update_table) and element-wise Adagrad on the MLPs (dense_step) in one step; one rank."""


# ---- what the kernel tests compare with -------------------------------------------------------------------------------------

def kernel_reference(p0, S0, g, lr, eps):
    """float64: (S, p, step) of parameters p0 with accumulators S0 and fp32 gradients g (arrays of one shape)."""
    g = np.asarray(g).astype(np.float64)
    S = np.asarray(S0).astype(np.float64) + g * g
    step = lr * g / (np.sqrt(S) + eps)
    return S, np.asarray(p0).astype(np.float64) - step, step


def kernel_bounds(S64, p64, step64):
    """|S - S64| <= 4 u S64: the square, the add, one spare ulp each.
    |p - p64| <= 18 u |step| + u |p64|: the project's 16 u for sqrt / add / divide / multiply / fma, hardware approximations
    included (rowwise_adagrad_restated.kernel_bounds), plus 2 u for the accumulator's error through the square root."""
    return 4 * U * S64, 18 * U * np.abs(step64) + U * np.abs(p64)


def kernel_check(S, p, S0, p0, g, lr, eps, what=""):
    """Raises AssertionError unless accumulators S and parameters p are within kernel_bounds of the reference; returns the
    largest (error / bound) of each."""
    S64, p64, step = kernel_reference(p0, S0, g, lr, eps)
    bS, bp = kernel_bounds(S64, p64, step)
    S, p = np.asarray(S), np.asarray(p)
    assert np.isfinite(S).all() and np.isfinite(p).all(), "%s: not finite" % what
    dS, dp = np.abs(S.astype(np.float64) - S64), np.abs(p.astype(np.float64) - p64)
    if not (dS <= bS).all():
        i = int(np.argmax(dS - bS))
        raise AssertionError("%s accumulator %d: got %r, float64 %r, |diff| %.3g > bound %.3g"
                             % (what, i, S.flat[i], S64.flat[i], dS.flat[i], bS.flat[i]))
    if not (dp <= bp).all():
        i = int(np.argmax(dp - bp))
        raise AssertionError("%s parameter %d: got %r, float64 %r, |diff| %.3g > bound %.3g"
                             % (what, i, p.flat[i], p64.flat[i], dp.flat[i], bp.flat[i]))
    return float((dS / np.maximum(bS, 1e-300)).max()), float((dp / np.maximum(bp, 1e-300)).max())


# ---- the engine tests' inputs (tests/test_dense_adagrad.py; self-checked in tests/test_dense_adagrad_host.py) -----------------

LN_EMB = [5000, 30, 2000, 900]          # the small table set of tests/test_rowwise_adagrad.py (table 2: five indices, heavy repeats)
ENGINE_CASE = dict(m_spa=16, B=64, L=3, ways=4, cache_size=40, seed=13, lr=0.05, lr_embeds=0.01, steps=9, batch_seed=93)


def engine_shapes(ln_emb=LN_EMB, m_spa=ENGINE_CASE["m_spa"]):
    nf = len(ln_emb) + 1
    return np.array([13, 32, m_spa]), np.array([m_spa + nf * (nf - 1) // 2, 32, 1])


def engine_batches(ln_emb=LN_EMB, B=ENGINE_CASE["B"], nbatch=ENGINE_CASE["steps"], seed=ENGINE_CASE["batch_seed"]):
    """[(X [B, 13], idx int64 [T, B], T [B, 1])]: Zipf indices scattered over each table, table 2 drawing from five indices."""
    return criteo_batches(ln_emb, 13, B, nbatch, seed, heavy=(2,) if len(ln_emb) > 2 else ())


def run_restated(batches, *, dtype=torch.float32, world_size=1, variant="contract", eps=1e-10, ln_emb=LN_EMB, refill_seed=900,
                 embed="sgd", **over):
    """The restated trainer over `batches` as the engine tests drive the engine: a refill every L batches (torch seed
    refill_seed + j in front of each), one step per batch.  embed="rowwise_adagrad": the composed trainer, the rows' eps
    1e-10.  Returns the trainer."""
    c = dict(ENGINE_CASE)
    c.update(over)
    ln_bot, ln_top = engine_shapes(ln_emb, c["m_spa"])
    assert embed in ("sgd", "rowwise_adagrad")
    cls, kw = (DenseAdagradTrainer, {}) if embed == "sgd" else (BothAdagradTrainer, dict(adagrad_eps=1e-10))
    tr = cls(ln_emb, c["m_spa"], ln_bot, ln_top, cache_size=c["cache_size"], num_ways=c["ways"],
             mini_batch_size=c["B"], world_size=world_size, lr=c["lr"], lr_embeds=c["lr_embeds"],
             lookahead=c["L"], table_agg_freq=c.get("table_agg_freq", 10 ** 9), seed=c["seed"],
             dense_adagrad_eps=eps, dense_variant=variant, dtype=dtype, **kw)
    B = c["B"]
    lS_o = torch.arange(B).repeat(len(ln_emb), 1)
    torch.set_num_threads(1)
    for j, (X, idx, T) in enumerate(batches):
        if j % c["L"] == 0:
            torch.manual_seed(refill_seed + j)
            tr.refill(torch.cat([b[1] for b in batches[j:j + c["L"]]], dim=1))
        tr.step(j, X, lS_o, idx, T)
    return tr
