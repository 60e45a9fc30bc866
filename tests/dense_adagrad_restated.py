"""Element-wise Adagrad on the MLP parameters, restated on the oracle's functions.

The contract, per step and per dense parameter element, with g the gradient the SGD path would apply (weights: averaged over
the ranks; biases: the rank's own, un-reduced):

    S += g * g
    p -= lr * g / (sqrt(S) + eps)

torch.optim.Adagrad with lr_decay = 0, weight_decay = 0, initial_accumulator_value = 0.  S is one fp32 per parameter, per rank,
zero at the start.  g = 0 on S = 0 leaves p unchanged (0 / eps).

`DenseAdagradTrainer` is `OracleTrainer` whose `step` is the oracle's own sequence -- cache_forward, dlrm_forward, loss_fn,
embbag_bwd_sgd, the weight-only gradient average, table_aggregate -- with the dense update replaced; nothing here imports the
package under test.  `kernel_reference` / `kernel_bounds` are the float64 reference and the bounds the kernel tests hold the HIP
kernels to (and the host tests hold the wrong variants to: they must fail them).
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
    """OracleTrainer whose MLP parameters take Adagrad steps; `state[r]`: rank r's accumulators, (bot W, bot b, top W, top b)
    lists shaped like the parameters.  dtype=torch.float64 runs the same sequence in double precision."""

    def __init__(self, *a, dense_adagrad_eps=1e-10, variant="contract", dtype=torch.float32, **kw):
        super().__init__(*a, **kw)
        assert variant in VARIANTS
        self.eps, self.variant, self.dtype = float(dense_adagrad_eps), variant, dtype
        cast = lambda ts: [t.to(dtype) for t in ts]
        self.host = cast(self.host)
        self.weights = [cast(w) for w in self.weights]
        self.bot = [(cast(w), cast(b)) for w, b in self.bot]
        self.top = [(cast(w), cast(b)) for w, b in self.top]
        zeros = lambda ts: [torch.zeros_like(t) for t in ts]
        self.state = [(zeros(self.bot[r][0]), zeros(self.bot[r][1]), zeros(self.top[r][0]), zeros(self.top[r][1]))
                      for r in range(self.W)]

    def step(self, j, X, lS_o, lS_i, T):
        Wn, lbs, nt = self.W, self.lbs, len(self.ln_emb)
        X, T = X.to(self.dtype), T.to(self.dtype)
        rank_loss, params = [], []
        for r in range(Wn):
            Xr = X[r * lbs:(r + 1) * lbs]
            if Wn == 1:
                Ir = [lS_i[k] for k in range(nt)]
                Or = [lS_o[k] for k in range(nt)]
            else:
                Ir = [lS_i[k][r * lbs:(r + 1) * lbs] for k in range(nt)]
                Or = [lS_o[k][:Ir[k].numel()] for k in range(nt)]
            Tr = T[r * lbs:(r + 1) * lbs]
            ly, cg = O.cache_forward(self.occ, self.weights[r], self.cache_sizes, Or, Ir, self.host)
            ly = [v.detach().requires_grad_(True) for v in ly]
            leaf = lambda ts: [t.detach().requires_grad_(True) for t in ts]
            bw, bb, tw, tb = leaf(self.bot[r][0]), leaf(self.bot[r][1]), leaf(self.top[r][0]), leaf(self.top[r][1])
            Z = O.dlrm_forward(Xr, ly, (bw, bb), (tw, tb), self.op, self.itself, self.loss_threshold)
            E = O.loss_fn(Z, Tr, self.loss_kind, self.loss_ws)
            E.backward()
            rank_loss.append(float(E.detach()))
            params.append((bw, bb, tw, tb))
            for k in range(nt):
                O.embbag_bwd_sgd(self.weights[r][k], cg[k].long(), Or[k], ly[k].grad, self.lr_embeds)
            self.touched[r].append(list(cg))
            if self.evict_victim:
                for k in range(nt):
                    first_aux = int(self.cache_sizes[k]) * self.ways
                    sl = cg[k].long()
                    for p in torch.nonzero(sl >= first_aux).flatten().tolist():
                        self.host[k][int(Ir[k][p])] = self.weights[r][k][int(sl[p])]
        # weight gradients averaged over the ranks, bias gradients not reduced
        for part in (0, 2):
            for li in range(len(params[0][part])):
                g = sum(params[r][part][li].grad / Wn for r in range(Wn))
                for r in range(Wn):
                    params[r][part][li].grad = g.clone()
        # the dense update: Adagrad, per rank, on that rank's accumulators
        for r in range(Wn):
            new = []
            for part in range(4):
                ps, Ss = [], []
                for p, S in zip(params[r][part], self.state[r][part]):
                    p2, S2 = adagrad_update(p.detach(), S, p.grad, self.lr, self.eps, self.variant)
                    ps.append(p2.detach())
                    Ss.append(S2.detach())
                new.append((ps, Ss))
            self.bot[r] = (new[0][0], new[1][0])
            self.top[r] = (new[2][0], new[3][0])
            self.state[r] = tuple(n[1] for n in new)
        if j > 0 and j % self.agg_freq == 0:
            for k in range(nt):
                touched = [torch.cat([t[k] for t in self.touched[r]]) for r in range(Wn)]
                O.table_aggregate([self.weights[r][k] for r in range(Wn)], touched, self.agg_op)
            self.touched = [[] for _ in range(Wn)]
        self.losses.append(rank_loss)
        return rank_loss

    def dense_params(self, r=0):
        """Rank r's dense parameters as one flat vector: all weights (bottom, then top), then all biases."""
        return torch.cat([t.reshape(-1) for t in self.bot[r][0] + self.top[r][0] + self.bot[r][1] + self.top[r][1]])

    def dense_state(self, r=0):
        s = self.state[r]
        return torch.cat([t.reshape(-1) for t in s[0] + s[2] + s[1] + s[3]])


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
    from rowwise_adagrad_restated import criteo_batches
    return criteo_batches(ln_emb, 13, B, nbatch, seed, heavy=(2,) if len(ln_emb) > 2 else ())


def run_restated(batches, *, dtype=torch.float32, world_size=1, variant="contract", eps=1e-10, ln_emb=LN_EMB, refill_seed=900,
                 **over):
    """The restated trainer over `batches` as the engine tests drive the engine: a refill every L batches (torch seed
    refill_seed + j in front of each), one step per batch.  Returns the trainer."""
    c = dict(ENGINE_CASE)
    c.update(over)
    ln_bot, ln_top = engine_shapes(ln_emb, c["m_spa"])
    tr = DenseAdagradTrainer(ln_emb, c["m_spa"], ln_bot, ln_top, cache_size=c["cache_size"], num_ways=c["ways"],
                             mini_batch_size=c["B"], world_size=world_size, lr=c["lr"], lr_embeds=c["lr_embeds"],
                             lookahead=c["L"], table_agg_freq=c.get("table_agg_freq", 10 ** 9), seed=c["seed"],
                             dense_adagrad_eps=eps, variant=variant, dtype=dtype)
    B = c["B"]
    lS_o = torch.arange(B).repeat(len(ln_emb), 1)
    torch.set_num_threads(1)
    for j, (X, idx, T) in enumerate(batches):
        if j % c["L"] == 0:
            torch.manual_seed(refill_seed + j)
            tr.refill(torch.cat([b[1] for b in batches[j:j + c["L"]]], dim=1))
        tr.step(j, X, lS_o, idx, T)
    return tr
