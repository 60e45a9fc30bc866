"""Quotient-remainder tables trained through the embedding cache, restated on the oracle's own functions.

Contract:
  * a table with n_k > qr_threshold is a QR table: quotient rows Wq_k [ceil(n_k / c), D], remainder rows Wr_k [c, D];
  * r = idx % c; q = (int64)((float32)idx / (float32)c), and for 0 <= idx < n_k a quotient >= rows_q is rows_q - 1;
  * the cache holds quotient rows keyed by q: refill, probe, aux rows, eviction, table aggregation all run on the q stream
    over tables of rows_q rows (a plain table: q = idx);
  * forward E[b, k] = row(slot[b, k]) * Wr_k[r[b, k]] (mult) or + (add); a plain table passes its row through;
  * backward: the cache row's gradient goes through embbag_bwd_sgd as ever; Wr_k -= lr_embeds * dL/dWr_k (local SGD);
  * at every table aggregation Wr is merged over the ranks like a table every rank touched all rows of.
Gradients come from torch autograd on the CPU.  Nothing here reads the GPU code or the reference tree."""
import numpy as np
import torch

from oracle import cdlrm_oracle as O
from rowwise_adagrad_restated import criteo_batches  # noqa: F401  (the batch stream the host and the GPU tests share)


def collisions_of(ln_emb, c, threshold):
    """c for a QR table, 0 for a plain one."""
    return [int(c) if int(n) > int(threshold) else 0 for n in ln_emb]


def rows_q_of(ln_emb, coll):
    return [-(-int(n) // c) if c else int(n) for n, c in zip(ln_emb, coll)]


def split(idx, n_rows, c):
    """One table's lookups -> (q int64, r uint8).  c = 0: a plain table."""
    idx = np.asarray(idx, dtype=np.int64)
    if idx.size and (idx.min() < 0 or idx.max() >= n_rows):
        raise IndexError("index outside the table")
    if c == 0:
        return idx.copy(), np.zeros(idx.shape, dtype=np.uint8)
    q = (idx.astype(np.float32) / np.float32(c)).astype(np.int64)
    q = np.minimum(q, -(-int(n_rows) // c) - 1)
    return q, (idx % c).astype(np.uint8)


def split_tables(idx, ln_emb, coll):
    """idx [T, n] (tensor or array) -> (q int64 tensor [T, n], r uint8 tensor [T, n])."""
    idx = np.asarray(idx)
    qs, rs = zip(*[split(idx[k], int(ln_emb[k]), coll[k]) for k in range(len(ln_emb))])
    return torch.from_numpy(np.stack(qs)), torch.from_numpy(np.stack(rs))


def init_tables(ln_emb, m_spa, c, threshold, seed):
    """-> (host rows per table: Wq of a QR table, W of a plain one; Wr per table, None for a plain one).  QR tables are
    U(sqrt(1/n), 1) from the torch generator, plain ones U(-sqrt(1/n), sqrt(1/n)) from numpy's."""
    np.random.seed(seed)
    torch.manual_seed(seed)
    coll = collisions_of(ln_emb, c, threshold)
    rq = rows_q_of(ln_emb, coll)
    host, wr = [], []
    for k, n in enumerate(ln_emb):
        n = int(n)
        if coll[k]:
            host.append(torch.empty(rq[k], m_spa).uniform_(float(np.sqrt(1 / n)), 1.0))
            wr.append(torch.empty(coll[k], m_spa).uniform_(float(np.sqrt(1 / n)), 1.0))
        else:
            host.append(torch.tensor(np.random.uniform(-np.sqrt(1 / n), np.sqrt(1 / n), size=(n, m_spa)).astype(np.float32)))
            wr.append(None)
    return host, wr


def compose(row, wr, r, operation):
    if wr is None:
        return row
    y = wr[torch.as_tensor(np.asarray(r)).long()]
    if operation == "mult":
        return row * y
    if operation == "add":
        return row + y
    raise ValueError(operation)


class QRCachedTrainer(O.OracleTrainer):
    """OracleTrainer over the quotient tables; step / evaluate / refill take the UNSPLIT indices."""

    def __init__(self, ln_emb, m_spa, ln_bot, ln_top, *, qr_collisions, qr_threshold, qr_operation, host_tables, weight_r, **kw):
        self.ln_full = [int(n) for n in ln_emb]
        self.coll = collisions_of(ln_emb, qr_collisions, qr_threshold)
        self.qr_op = qr_operation
        assert qr_operation in ("mult", "add")
        super().__init__(rows_q_of(ln_emb, self.coll), m_spa, ln_bot, ln_top, host_tables=host_tables, **kw)
        self.Wr = [[None if w is None else w.clone() for w in weight_r] for _ in range(self.W)]

    def split(self, idx):
        return split_tables(idx, self.ln_full, self.coll)

    def refill(self, window_idx, q_source=None):
        q, _ = self.split(window_idx)
        return super().refill(q, q_source)

    def evaluate(self, X, lS_o, lS_i):
        T = len(self.ln_full)
        q, rem = self.split(lS_i)
        with torch.no_grad():
            ly, _ = O.cache_forward(self.occ, self.weights[0], self.cache_sizes, [lS_o[k] for k in range(T)],
                                    [q[k] for k in range(T)], self.host)
            E = [compose(ly[k], self.Wr[0][k], rem[k], self.qr_op) for k in range(T)]
            return O.dlrm_forward(X, E, self.bot[0], self.top[0], self.op, self.itself, self.loss_threshold)


    # the phases of OracleTrainer.step that differ: the slice carries the remainders, the pooled quotient rows are composed
    # with Wr, Wr takes its local SGD step beside the cache rows and is merged with them

    def rank_slice(self, r, X, lS_o, lS_i, T):
        nt = len(self.ln_full)
        sl = slice(r * self.lbs, (r + 1) * self.lbs)
        q, rem = self.split(lS_i)
        Ir = [q[k][sl] for k in range(nt)]
        Or = [lS_o[k][:Ir[k].numel()] for k in range(nt)]
        for k in range(nt):     # one lookup per bag
            assert torch.equal(Or[k].long(), torch.arange(Ir[k].numel()))
        return X[sl], Or, Ir, T[sl], [rem[k][sl] for k in range(nt)]

    def features(self, r, rows, Rr):
        wr = [None if w is None else w.detach().requires_grad_(True) for w in self.Wr[r]]
        return [compose(rows[k], wr[k], Rr[k], self.qr_op) for k in range(len(rows))], wr

    def update_embeddings(self, r, cg, Or, rows, wr):
        super().update_embeddings(r, cg, Or, rows, wr)
        for k, w in enumerate(wr):
            if w is not None:
                self.Wr[r][k] = (w - self.lr_embeds * w.grad).detach()

    def merge_rows(self):
        super().merge_rows()
        for k, c in enumerate(self.coll):
            if c:               # Wr: a table all of whose rows every rank touched
                every = [torch.arange(c, dtype=torch.int32) for _ in range(self.W)]
                O.table_aggregate([self.Wr[r][k] for r in range(self.W)], every, self.agg_op)
