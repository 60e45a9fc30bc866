#!/usr/bin/env python3
"""One sha256 per case over everything the oracle's trainers leave behind, to compare two trees bit for bit on one machine.

    python tools/oracle_trainer_digests.py > digests.txt        (in either tree; the outputs must be identical)

Covers OracleTrainer (oracle/cdlrm_oracle.py) and the four trainers built on it (tests/dense_adagrad_restated.py,
tests/rowwise_adagrad_restated.py, tests/qr_cached_restated.py, BagRangeOracle of tests/test_multihot_ranks.py) through the
surface their callers use: the constructors, refill / step / losses, weights / host / bot / top / occ, `state` of the row-wise
trainer, dense_params() / dense_state() of the dense one, Wr of the quotient-remainder one.  CPU only, one thread, fixed
seeds; all cases are small (B <= 64, at most 9 steps, four tables or fewer).  The digests are only comparable between runs
on the same machine and torch build."""
import hashlib
import os
import sys
from types import SimpleNamespace

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import cdlrm_oracle as O  # noqa: E402
import dense_adagrad_restated as DA  # noqa: E402
import qr_cached_restated as QR  # noqa: E402
import rowwise_adagrad_restated as RA  # noqa: E402

LN_EMB = [5000, 30, 2000, 900]
L = 3


def digest(tr, extra=()):
    h = hashlib.sha256()

    def add(t):
        t = torch.as_tensor(t).detach().contiguous()
        h.update(("%s%s" % (t.dtype, tuple(t.shape))).encode())
        h.update(t.numpy().tobytes())

    add(np.array(tr.losses, dtype=np.float64))
    for r in range(tr.W):
        for t in tr.weights[r] + tr.bot[r][0] + tr.bot[r][1] + tr.top[r][0] + tr.top[r][1]:
            add(t)
    for t in list(tr.host) + list(tr.occ) + list(extra):
        add(t)
    return h.hexdigest()


def mlps(D, n_tables, n_dense=13):
    nf = n_tables + 1
    return np.array([n_dense, 32, D]), np.array([D + nf * (nf - 1) // 2, 32, 1])


def drive(tr, batches, lS_o, seed0=900):
    for j, (X, idx, T) in enumerate(batches):
        if j % L == 0:
            torch.manual_seed(seed0 + j)
            tr.refill(torch.cat([b[1] for b in batches[j:j + L]], dim=1))
        tr.step(j, X, lS_o, idx, T)
    return tr


def base_kw(B, **over):
    kw = dict(cache_size=40, num_ways=4, mini_batch_size=B, lr=0.1, lr_embeds=0.3, lookahead=L, table_agg_freq=1, seed=13)
    kw.update(over)
    return kw


def oracle_case(B=64, D=16, nbatch=9, **over):
    ln_bot, ln_top = mlps(D, len(LN_EMB))
    if over.get("op") == "cat":
        ln_top = np.array([D * (len(LN_EMB) + 1), 32, 1])
    tr = O.OracleTrainer(LN_EMB, D, ln_bot, ln_top, **base_kw(B, **over))
    batches = RA.criteo_batches(LN_EMB, 13, B, nbatch, 31, heavy=(2,))
    return digest(drive(tr, batches, torch.arange(B).repeat(len(LN_EMB), 1)))


def multihot_case():
    B, D, hot = 64, 16, 3
    rng = np.random.RandomState(99)
    batches = []
    for _ in range(9):
        X = torch.from_numpy(rng.rand(B, 13).astype(np.float32))
        idx = torch.stack([torch.from_numpy(rng.zipf(1.2, size=hot * B).astype(np.int64) * 2654435761 % n) for n in LN_EMB])
        batches.append((X, idx, torch.from_numpy(np.round(rng.rand(B, 1)).astype(np.float32))))
    ln_bot, ln_top = mlps(D, len(LN_EMB))
    tr = O.OracleTrainer(LN_EMB, D, ln_bot, ln_top, **base_kw(hot * B))
    return digest(drive(tr, batches, torch.arange(0, hot * B, hot).repeat(len(LN_EMB), 1)))


def dense_case(dtype, W, variant):
    tr = DA.run_restated(DA.engine_batches(), dtype=dtype, world_size=W, variant=variant, table_agg_freq=2)
    return digest(tr, [f(r) for r in range(W) for f in (tr.dense_params, tr.dense_state)])


def rowwise_case(D, variant):
    ln_bot, ln_top = mlps(D, len(LN_EMB))
    tr = RA.RowwiseAdagradTrainer(LN_EMB, D, ln_bot, ln_top, variant=variant, adagrad_eps=1e-10,
                                  **base_kw(64, lr_embeds=0.01, table_agg_freq=10 ** 9))
    batches = RA.criteo_batches(LN_EMB, 13, 64, 9, 77 + D, heavy=(2,))
    drive(tr, batches, torch.arange(64).repeat(len(LN_EMB), 1))
    return digest(tr, tr.state)


def qr_case(op, W):
    ln_emb, m, B, c, thr, seed = [900, 150, 1300], 8, 32, 4, 200, 3
    host, wr = QR.init_tables(ln_emb, m, c, thr, seed)
    tr = QR.QRCachedTrainer(ln_emb, m, [13, 16, m], np.array([m + 4 * 3 // 2, 16, 1]), qr_collisions=c, qr_threshold=thr,
                            qr_operation=op, host_tables=[h.clone() for h in host], weight_r=wr, cache_size=20, num_ways=2,
                            mini_batch_size=B, world_size=W, lr=0.1, lr_embeds=0.3, lookahead=L, table_agg_freq=2, seed=seed)
    batches = QR.criteo_batches(ln_emb, 13, B, 9, seed + 1)
    drive(tr, batches, torch.arange(B).repeat(3, 1))
    return digest(tr, [w for r in range(W) for w in tr.Wr[r] if w is not None])


def bag_range_case(world, agg_op):
    """The inputs of tests/test_multihot_ranks.py::test_ragged_bags_ranks_vs_oracle."""
    import test_multihot_ranks as MR
    from cdlrm_amd import dlrm_data_pytorch as DP
    ln_emb, m_spa, B, ways, cache_size, seed, aux = [900, 40, 6, 2500], 16, 29, 4, 300, 23, 256
    nf = len(ln_emb) + 1
    ln_bot, ln_top = [5, 32, m_spa], [m_spa + nf * (nf - 1) // 2, 24, 1]
    args = SimpleNamespace(data_size=255, num_batches=0, mini_batch_size=B, num_indices_per_lookup=7,
                           num_indices_per_lookup_fixed=False, round_targets=True, data_generation="random",
                           numpy_rand_seed=seed)
    _, loader = DP.make_random_data_and_loader(args, np.array(ln_emb), 5)
    batches = [(X, lS_o, [x.clone() for x in lS_i], Tt) for X, lS_o, lS_i, Tt in loader]
    tr = MR._ragged_oracle_class()(ln_emb, m_spa, np.array(ln_bot), np.array(ln_top), cache_size=cache_size, num_ways=ways,
                                   mini_batch_size=aux, batch_size=B, world_size=world, lr=0.1, lr_embeds=0.3, lookahead=L,
                                   table_agg_freq=1, table_agg_op=agg_op, seed=seed)
    for j, (X, lS_o, lS_i, Tt) in enumerate(batches):
        if j % L == 0:
            torch.manual_seed(800 + j)
            tr.refill([torch.cat([b[2][k] for b in batches[j:j + L]]) for k in range(len(ln_emb))])
        tr.step(j, X, lS_o, lS_i, Tt)
    return digest(tr)


def cases():
    for W, B in ((1, 64), (2, 64), (3, 29)):
        yield "oracle W=%d B=%d" % (W, B), lambda W=W, B=B: oracle_case(B=B, world_size=W)
    for op in ("mean", "max", "sum"):
        for freq in (1, 2):
            yield "oracle W=2 agg=%s freq=%d" % (op, freq), lambda op=op, freq=freq: oracle_case(
                world_size=2, table_agg_op=op, table_agg_freq=freq)
    yield "oracle loss=bce", lambda: oracle_case(loss="bce")
    yield "oracle loss=mse", lambda: oracle_case(loss="mse")
    yield "oracle loss=wbce threshold=0.05", lambda: oracle_case(loss="wbce", loss_weights=[0.4, 1.7], loss_threshold=0.05)
    yield "oracle op=dot", lambda: oracle_case(op="dot")
    yield "oracle op=cat W=2", lambda: oracle_case(op="cat", world_size=2)
    yield "oracle evict_victim_cache W=1", lambda: oracle_case(evict_victim_cache=True)
    yield "oracle multi-hot W=1", multihot_case
    for dtype in (torch.float32, torch.float64):
        for W in (1, 2):
            for v in DA.VARIANTS:
                yield "dense_adagrad %s W=%d %s" % (str(dtype).split(".")[1], W, v), lambda d=dtype, W=W, v=v: dense_case(d, W, v)
    for D in (16, 128):
        for v in ("rowwise", "elementwise", "no_accumulate", "sum"):
            yield "rowwise_adagrad D=%d %s" % (D, v), lambda D=D, v=v: rowwise_case(D, v)
    for op in ("mult", "add"):
        for W in (1, 2):
            yield "qr_cached %s W=%d" % (op, W), lambda op=op, W=W: qr_case(op, W)
    for W, agg in ((2, "mean"), (3, "mean"), (3, "max")):
        yield "bag_range W=%d agg=%s" % (W, agg), lambda W=W, agg=agg: bag_range_case(W, agg)


def main():
    torch.set_num_threads(1)
    for name, run in cases():
        print("%s  %s" % (run(), name), flush=True)


if __name__ == "__main__":
    main()
