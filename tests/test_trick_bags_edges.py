"""The stand-alone bag operators of csrc/qr.hip against float64 at their edges: k_qr_fwd<LPR> / k_qr_bwd<LPR> behind
tricks.QREmbeddingBag, k_bag_fwd / k_bag_bwd behind tricks.PrEmbeddingBag.

tests/trick_bags_restated.py holds each contract as plain numpy in float64, the inputs and the comparator.  Every comparison
is |got - want| <= a bound computed per element from the inputs (the docstring there derives it); no tolerance is chosen by
hand.  Buffers handed to an entry point directly start as a sentinel bit pattern with PAD more elements behind them, and the
padding has to come back unchanged; inputs have to come back unchanged; every test ends on torch.cuda.synchronize().

Which shape reaches which path:

    QR, D = 4 .. 256        lanes per row 4 (3 idle, 1 idle, full), 8, 16, 32, 64, each once with idle lanes and once full
    QR, D = 260, 512        a second trip of the column loop (63 lanes idle on it at D = 260)
    QR, 32769 bags, D = 132 8192 blocks x 4 bags + 1: the grid-stride trip of the 64-lane instance;  524289 bags, D = 4: 4-lane
    bag, 699051 bags, D = 3 699051 x 3 = 8192 blocks x 256 threads + 1: the grid-stride trip of both bag kernels
    ragged bags             an empty first bag, two empty bags in a row, 1000 lookups in one bag, an empty last bag whose offset is
                            n; closed_by_n: a last bag that n closes

The unmarked tests run anywhere: the inputs hold these edges, the comparator rejects seven wrong answers, and the
restatement agrees with the reference's modules (tests/golden/trick_bag_edges.npz, tools/make_golden.py: g_qr_edges, g_md_edges)
within twice the bounds -- the reference adds in fp32 too."""
import types

import numpy as np
import pytest
import torch

import trick_bags_restated as R
from trick_bags_restated import PAD, same_bits, sentinel, within

gpu = pytest.mark.gpu
DEV = "cuda:0"
NCAT = 103                                                  # categories of the small tables: 26 quotient rows at c = 4


def ids(values, fmt="%s"):
    return [fmt % v for v in values]


def grad_for(op, G2, D):
    """mult and add take the first D columns of the [n_bags, 2 D] gradient, concat all of it."""
    return G2 if op == "concat" else np.ascontiguousarray(G2[:, :D])


def qr_case(kind, n_bags, D, seed=0):
    """Small tables (NCAT categories, c = 4) under `ragged` / `closed_by_n` / one-lookup / contention bags."""
    if kind == "contention":
        idx, off, n = R.contention_input()
        G = R.contention_grad(2 * D, "spread")
    else:
        if kind == "ones":                                         # the last bag alone names quotient row 25 (ids 100 .. 102)
            off, n = np.arange(n_bags, dtype=np.int64), n_bags
            idx = R.cap_ids(n, 100, (101,), 400 + seed)
        else:
            off, n = R.bags(kind, n_bags)
            idx = R.small_ids(n, NCAT, 400 + seed)
        G = np.random.RandomState(410 + D).randn(off.size, 2 * D).astype(np.float32)
    return types.SimpleNamespace(idx=idx, off=off, n=n, c=R.C4, D=D, ncat=NCAT, rows_q=-(-NCAT // R.C4), G=G,
                                 Wq=R.weights(-(-NCAT // R.C4), D, 420 + D), Wr=R.weights(R.C4, D, 430 + D))


# ---- on any machine: the inputs hold their edges ----------------------------------------------------------------------

def test_inputs_hold_their_edges():
    for n_bags, long in ((R.QR_BAGS, 1000), (R.BAG_BAGS, 1000), (R.FIX_BAGS, R.FIX_LONG)):
        for kind in ("ragged", "closed_by_n"):
            off, n = R.bags(kind, n_bags, long)
            L = R.bag_ends(off, n) - off
            assert off.size == n_bags and L.sum() == n and (L >= 0).all()
            assert set(L[:-1].tolist()) == {0, 1, 2, 7, long}, "every bag-length class"
            assert L[0] == 0 and ((L[1:-1] == 0) & (L[2:] == 0)).any(), "an empty first bag, two empty bags in a row"
            if kind == "ragged":
                assert L[-1] == 0 and off[-1] == n, "an empty last bag whose offset equals n"
            else:
                assert L[-1] > 0 and off[-1] < n, "a last bag that only n closes"
    # the float32 quotient differs from the integer one on at least a tenth of every list that is meant to show it
    lists = [R.quirk_ids(R.bags("ragged", R.QR_BAGS)[1])] + [R.fixture_qr_inputs("quirk", D)["idx"] for D in R.FIX_DIMS]
    for idx in lists:
        assert R.quirk_share(idx, R.C4) >= 0.1, R.quirk_share(idx, R.C4)
        assert set(R.QUIRK_IDS) <= set(idx.tolist()) and idx.max() < R.N_C4
    off, n = R.bags("ragged", R.QR_BAGS)
    pos, bag = R.lookups(off, R.bag_ends(off, n))
    L = (R.bag_ends(off, n) - off)[bag]
    differs = R.quotient(lists[0], R.C4) != lists[0] // R.C4
    assert (differs & (L == 2)).any() and (differs & (L == 7)).any() and (differs & (L == 1000)).any()
    assert R.quotient(np.array([39884403, 16777217, 33554433]), 4).tolist() == [9971101, 4194304, 8388608]
    # the lane count of every width, idle and full
    lanes = {4: 4, 12: 4, 16: 4, 20: 8, 32: 8, 36: 16, 64: 16, 68: 32, 128: 32, 132: 64, 256: 64, 260: 64, 512: 64}
    assert set(lanes) == set(R.QR_DIMS + R.QR_DIMS_TWO_TRIPS)
    for D, want in lanes.items():
        assert R.qr_lanes(D) == want == min(64, max(4, R.pow2ceil(D / 4))), D
    for lpr in (4, 8, 16, 32, 64):
        d4 = [D // 4 for D in R.QR_DIMS if R.qr_lanes(D) == lpr]
        assert lpr in d4 and min(d4) < lpr, "lane count %d: once full, once with idle lanes" % lpr
    assert [D // 4 for D in R.QR_DIMS[:3]] == [1, 3, 4]
    assert all(D // 4 > 64 for D in R.QR_DIMS_TWO_TRIPS) and R.QR_DIMS_TWO_TRIPS[0] // 4 == 65
    # the bag counts pass the grid caps by one
    for D, n_bags in (R.QR_CAP_64, R.QR_CAP_4):
        assert n_bags == R.QR_GRID_CAP * (256 // R.qr_lanes(D)) + 1
    assert R.BAG_CAP[1] * R.BAG_CAP[0] == R.QR_GRID_CAP * 256 + 1
    off, n = R.cycle_bags(R.BAG_CAP[1])
    assert n == R.BAG_CAP[1] and (R.bag_ends(off, n) - off)[:4].tolist() == [1, 0, 2, 1]
    # the top id, once
    t = R.top_ids(4044, 17)
    q = R.quotient(t, R.C4)
    assert -(-R.N_TOP // R.C4) == q.max() == q[17] and np.count_nonzero(q == q.max()) == 1 and t.max() == R.N_TOP - 1
    # contention: one quotient row, two of the four remainder rows
    idx, off, n = R.contention_input()
    assert n == idx.size == 8192 and off.size == 64 and set(R.quotient(idx, R.C4).tolist()) == {5}
    assert set((idx % R.C4).tolist()) == {0, 3}
    assert R.BAG_DIMS == (1, 2, 3, 5, 7, 8, 13, 64)


def bag_cap_ids(n):
    """The plain bag's grid-cap ids: the last bag's two lookups alone name rows 101 and 102."""
    return R.cap_ids(n, 101, (101, 102), 480)


# ---- on any machine: the comparator rejects the plausible wrong answers ---------------------------------------------

def rejects(got, want, bound, what):
    with pytest.raises(AssertionError):
        within(got, want, bound, what)


def test_comparator_rejects_integer_quotient():
    off, n = R.bags("ragged", R.QR_BAGS)
    idx = R.quirk_ids(n)
    rows_q = -(-R.N_C4 // R.C4)
    for D, Wq in ((4, R.RowIsIndex(rows_q, 4)), (12, R.FormulaTable(rows_q, 12, 5))):
        Wr = R.weights(R.C4, D, 430 + D)
        good, wrong = R.QR(idx, off, n, Wq, Wr, R.C4), R.QR(idx, off, n, Wq, Wr, R.C4, q=idx // R.C4)
        for op in R.OPS:
            want, bound = good.forward(op)
            within(want.astype(np.float32), want, bound, op)
            rejects(wrong.forward(op)[0].astype(np.float32), want, bound, op)
    # the formula table shows it in every bag that holds such an id, the long one too
    want, bound = good.forward("concat")
    miss = np.abs(wrong.forward("concat")[0] - want) > bound
    L = R.bag_ends(off, n) - off
    assert miss[L == 1000].any() and miss[L == 7].any()


def test_comparator_rejects_last_bag_closed_by_offsets():
    c = qr_case("closed_by_n", R.QR_BAGS, 12)
    good = R.QR(c.idx, c.off, c.n, c.Wq, c.Wr, c.c)
    ends = R.bag_ends(c.off, c.n)
    ends[-1] = c.off[-1]
    wrong = R.QR(c.idx, c.off, c.n, c.Wq, c.Wr, c.c, ends=ends)
    for op in R.OPS:
        want, bound = good.forward(op)
        within(want.astype(np.float32), want, bound, op)
        rejects(wrong.forward(op)[0].astype(np.float32), want, bound, op)
        if op == "mult":        # (a row's gradient holds the 1000-lookup bags' operands: three lookups more or less sit in its bound)
            continue
        G = grad_for(op, c.G, c.D)
        gq, bq, gr, br = good.backward(op, G)
        wq, _, wr, _ = wrong.backward(op, G)
        rejects(wq.astype(np.float32), gq, bq, op)
        rejects(wr.astype(np.float32), gr, br, op)
    b = R.Bag(c.idx, c.off, c.n, (NCAT, 5))
    W = R.weights(NCAT, 5, 440)
    want, bound = b.forward(W)
    got = want.astype(np.float32)
    got[-1] = 0
    rejects(got, want, bound, "bag")


def test_comparator_rejects_dropped_column_and_swapped_halves():
    c = qr_case("ragged", R.QR_BAGS, 12)
    good = R.QR(c.idx, c.off, c.n, c.Wq, c.Wr, c.c)
    for op in R.OPS:
        want, bound = good.forward(op)
        for stale in (0.0, float("nan")):
            got = want.astype(np.float32)
            got[:, 8:12] = stale                                   # the last float4 column of the first half never stored
            rejects(got, want, bound, op)
    want, bound = good.forward("concat")
    got = want.astype(np.float32)
    rejects(np.concatenate([got[:, 12:], got[:, :12]], axis=1), want, bound, "concat")
    gq, bq, gr, br = good.backward("concat", c.G)
    wq, _, wr, _ = good.backward("concat", np.concatenate([c.G[:, 12:], c.G[:, :12]], axis=1))
    rejects(wq.astype(np.float32), gq, bq, "concat gWq")
    rejects(wr.astype(np.float32), gr, br, "concat gWr")


def test_comparator_rejects_mult_backward_from_own_operand():
    for kind in ("ragged", "contention"):
        c = qr_case(kind, R.QR_BAGS, 16)
        good = R.QR(c.idx, c.off, c.n, c.Wq, c.Wr, c.c)
        G = grad_for("mult", c.G, c.D)
        gq, bq, gr, br = good.backward("mult", G)
        within(gq.astype(np.float32), gq, bq, "gWq")
        within(gr.astype(np.float32), gr, br, "gWr")
        rejects(good.backward("mult", G, mult_dq_from_eq=True)[0].astype(np.float32), gq, bq, "gWq")


def test_comparator_rejects_dropped_contribution_under_contention():
    """8192 adds on one element: the any-order bound is 4.3 times the mean contribution, so the comparator can show only a
    missing contribution well above the mean -- `spread` gradients have them.  With `integers` every partial sum is exact, the
    kernel's answer is the float64 one, and any missing contribution shows."""
    idx, off, n = R.contention_input()
    D = 16
    Wq, Wr = R.weights(26, D, 420 + D), R.weights(R.C4, D, 430 + D)
    good = R.QR(idx, off, n, Wq, Wr, R.C4)
    G = R.contention_grad(2 * D, "spread")[:, :D]
    b = int(np.argmax(np.abs(G).max(axis=1)))
    drop = np.delete(idx, off[b])                                  # the first lookup of the bag with the largest gradient
    off2 = np.where(np.arange(off.size) > b, off - 1, off)
    wrong = R.QR(drop, off2, n - 1, Wq, Wr, R.C4)
    for op in ("add", "mult"):
        gq, bq, gr, br = good.backward(op, G)
        within(gq.astype(np.float32), gq, bq, op)
        rejects(wrong.backward(op, G)[0].astype(np.float32), gq, bq, op)
        assert not gq[[r for r in range(26) if r != 5]].any() and not gr[[1, 2]].any() and not br[[1, 2]].any()
    Gi = R.contention_grad(2 * D, "integers")[:, :D]
    for b in range(off.size):
        drop, off2 = np.delete(idx, off[b]), np.where(np.arange(off.size) > b, off - 1, off)
        a = good.backward("add", Gi)[0]
        w = R.QR(drop, off2, n - 1, Wq, Wr, R.C4).backward("add", Gi)[0]
        assert (a[5] != w[5])[Gi[b] != 0].all()
    assert np.abs(good.backward("add", np.abs(Gi))[0]).max() < 2 ** 24


def test_comparator_rejects_skipped_bag_behind_the_grid():
    D, n_bags = R.QR_CAP_64
    c = qr_case("ones", n_bags, D)
    good = R.QR(c.idx, c.off, c.n, c.Wq, c.Wr, c.c)
    for op in ("add", "mult"):
        want, bound = good.forward(op)
        got = want.astype(np.float32)
        within(got, want, bound, op)
        got[n_bags - 1] = 0                                        # bag 32768 of 32769: the one the grid-stride trip takes
        rejects(got, want, bound, op)
        G = grad_for(op, c.G, D)
        gq, bq, gr, br = good.backward(op, G)
        within(gq.astype(np.float32), gq, bq, op)
        short = R.QR(c.idx[:-1], c.off[:-1], c.n - 1, c.Wq, c.Wr, c.c).backward(op, G[:-1])
        rejects(short[0].astype(np.float32), gq, bq, op)           # that bag's row of gWq is its own
    D, n_bags = R.BAG_CAP
    off, n = R.cycle_bags(n_bags)
    idx, G = bag_cap_ids(n), np.random.RandomState(482).randn(n_bags, D).astype(np.float32)
    assert (R.bag_ends(off, n) - off)[-1] == 2 and set(idx[-2:].tolist()).isdisjoint(idx[:-2].tolist())
    gW, bW = R.Bag(idx, off, n, (NCAT, D)).backward(G)
    within(gW.astype(np.float32), gW, bW, "bag gW")
    got = gW.astype(np.float32)
    got[idx[-2:], D - 1] = 0                                       # element 8192 x 256 of the [bags, D] grid: the last bag's last column
    rejects(got, gW, bW, "bag gW")


# ---- on any machine: the restatement against the reference's modules ------------------------------------------------

@pytest.mark.parametrize("D", R.FIX_DIMS, ids=ids(R.FIX_DIMS, "D%d"))
@pytest.mark.parametrize("kind", ["ragged", "quirk"])
def test_restatement_agrees_with_reference_qr(golden, kind, D):
    """Twice the bound: both sides are fp32 sums of the same terms.  The quotient rows the reference addressed (the fixture's
    wq_rows: the distinct values of its (idx / c).long()) have to be the restated quotients."""
    g = golden("trick_bag_edges")
    key = "qr_%s_D%d_" % (kind, D)
    inp = R.fixture_qr_inputs(kind, D)
    same_bits(g[key + "idx"], inp["idx"], "idx")
    same_bits(g[key + "offs"], inp["off"], "offsets")
    same_bits(g[key + "G"], inp["G"], "grad_out")
    idx, off, n, c = inp["idx"], inp["off"], inp["n"], int(g[key + "c"])
    rows = g[key + "wq_rows"]
    q = R.quotient(idx, c)
    same_bits(np.unique(q), rows, "the quotient rows the reference addressed")
    if kind == "quirk":
        assert (q != idx // c).mean() >= 0.1
    ref = R.QR(idx, off, n, g[key + "wq"], g[key + "wr"], c, q=np.searchsorted(rows, q))
    for op in R.OPS:
        want, bound = ref.forward(op)
        within(g[key + op + "_V"], want, 2 * bound, "%s V" % op)
        gq, bq, gr, br = ref.backward(op, grad_for(op, inp["G"], D))
        within(g[key + op + "_gq"], gq, 2 * bq, "%s gWq" % op)
        within(g[key + op + "_gr"], gr, 2 * br, "%s gWr" % op)


@pytest.mark.parametrize("D", R.FIX_WIDTHS, ids=ids(R.FIX_WIDTHS, "D%d"))
def test_restatement_agrees_with_reference_bag(golden, D):
    g = golden("trick_bag_edges")
    key = "bag_D%d_" % D
    inp = R.fixture_bag_inputs(D)
    same_bits(g[key + "idx"], inp["idx"], "idx")
    same_bits(g[key + "offs"], inp["off"], "offsets")
    W = g[key + "W"]
    ref = R.Bag(inp["idx"], inp["off"], inp["n"], W.shape)
    want, bound = ref.forward(W)
    within(g[key + "V"], want, 2 * bound, "V")
    gW, b = ref.backward(g[key + "G"])
    within(g[key + "gW"], gW, 2 * b, "gW")


def test_fixture_is_small(golden):
    import os
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "trick_bag_edges.npz")
    assert os.path.getsize(path) < 100 * 1024


def test_null_idx_is_refused_when_there_are_lookups():
    """idx == NULL passes only with n == 0 (an empty index tensor has no address).  The argument check comes before any device
    call, so this runs anywhere; the other pointers are never followed."""
    import ctypes as C
    from cdlrm_amd import _lib
    L = _lib.lib()
    buf = (C.c_char * 256)()
    p = (C.addressof(buf) + 15) & ~15
    calls = (lambda n: L.cdlrm_qr_embbag_fwd(None, p, n, 5, p, p, 26, 4, 16, 1, p, None, None, p, None),
             lambda n: L.cdlrm_qr_embbag_bwd(None, p, n, 5, None, None, p, 26, 4, 16, 1, p, p, None),
             lambda n: L.cdlrm_bag_fwd(None, p, n, 5, p, 103, 3, p, p, None),
             lambda n: L.cdlrm_bag_bwd(None, p, n, 5, p, 103, 3, p, None))
    for call in calls:
        assert call(3) != 0
        assert b"idx || n == 0" in L.cdlrm_last_error()


# ---- device side --------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def lib():
    from cdlrm_amd import _lib
    _lib.lib()
    return _lib


def dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)


def host(t):
    return t.detach().cpu().numpy()


def stream():
    return torch.cuda.current_stream().cuda_stream


def out_buffer(elems, zeros=False):
    """Device floats: `elems` the entry point may write (sentinels, or the zeros a gradient starts from), PAD sentinels behind."""
    a = sentinel(elems + PAD)
    if zeros:
        a[:elems] = 0
    return dev(a)


def take(buf, rows, cols, what):
    """The [rows, cols] an entry point wrote at the head of `buf`; the padding behind it has to be untouched."""
    a = host(buf)
    same_bits(a[rows * cols:], sentinel(PAD), "behind " + what)
    return a[:rows * cols].reshape(rows, cols)


def qr_direct(lib, c, op, d, G=None, operands=True):
    """cdlrm_qr_embbag_fwd (and _bwd for grad_out G) on device inputs d = (idx, off, Wq, Wr).  -> (out, eq, er, gq, gr, err)."""
    L, code, nb, D = lib.lib(), R.OP_CODE[op], c.off.size, c.D
    width = 2 * D if op == "concat" else D
    o, eq, er = out_buffer(nb * width), out_buffer(nb * D), out_buffer(nb * D)
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    lib.check(L.cdlrm_qr_embbag_fwd(lib.ptr(d[0]), d[1].data_ptr(), c.n, nb, d[2].data_ptr(), d[3].data_ptr(), c.rows_q, c.c, D,
                                    code, o.data_ptr(), eq.data_ptr() if operands else None,
                                    er.data_ptr() if operands else None, err.data_ptr(), stream()))
    res = [take(o, nb, width, "out")]
    for name, b in (("eq_out", eq), ("er_out", er)):
        res.append(take(b, nb, D, name) if operands else same_bits(host(b), sentinel(nb * D + PAD), name + " = NULL"))
    if G is not None:
        gq, gr, dG = out_buffer(c.rows_q * D, zeros=True), out_buffer(c.c * D, zeros=True), dev(G)
        lib.check(L.cdlrm_qr_embbag_bwd(lib.ptr(d[0]), d[1].data_ptr(), c.n, nb, eq.data_ptr() if operands else None,
                                        er.data_ptr() if operands else None, dG.data_ptr(), c.rows_q, c.c, D, code,
                                        gq.data_ptr(), gr.data_ptr(), stream()))
        res += [take(gq, c.rows_q, D, "gWq"), take(gr, c.c, D, "gWr")]
        same_bits(host(dG), G, "grad_out")
    else:
        res += [None, None]
    return tuple(res) + (int(err.item()),)


def check_qr(lib, c, ops, module=True, direct=True, operands=True):
    """Forward and backward of one case through QREmbeddingBag and through the entry points, against the restatement."""
    from cdlrm_amd.tricks.qr_embedding_bag import QREmbeddingBag
    ref = R.QR(c.idx, c.off, c.n, c.Wq, c.Wr, c.c)
    d = (dev(c.idx), dev(c.off), dev(c.Wq), dev(c.Wr))
    for op in ops:
        G = grad_for(op, c.G, c.D)
        want, bound = ref.forward(op)
        gq, bq, gr, br = ref.backward(op, G)
        if direct:
            out, eq, er, dq, dr, err = qr_direct(lib, c, op, d, G, operands)
            assert err == 0
            within(out, want, bound, "%s out" % op)
            if operands:
                within(eq, ref.Eq, R.SLACK * ref.bEq, "%s eq_out" % op)
                within(er, ref.Er, R.SLACK * ref.bEr, "%s er_out" % op)
            within(dq, gq, bq, "%s gWq" % op)
            within(dr, gr, br, "%s gWr" % op)
        if module:
            E = QREmbeddingBag(c.ncat, c.D, c.c, operation=op, mode="sum", sparse=True, _weight=[d[2], d[3]])
            dG = dev(G)
            V = E(d[0], d[1])
            assert tuple(V.shape) == want.shape
            within(host(V), want, bound, "%s module out" % op)
            V.backward(dG)
            within(host(E.weight_q.grad), gq, bq, "%s module gWq" % op)
            within(host(E.weight_r.grad), gr, br, "%s module gWr" % op)
            same_bits(host(dG), G, "grad_out")
            if direct:
                same_bits(host(V), out, "%s: the module's forward and the entry point's" % op)
    for t, a, what in zip(d, (c.idx, c.off, c.Wq, c.Wr), ("idx", "offsets", "weight_q", "weight_r")):
        same_bits(host(t), a, what)
    torch.cuda.synchronize()
    return ref


@gpu
@pytest.mark.parametrize("kind", ["ragged", "closed_by_n"])
@pytest.mark.parametrize("D", R.QR_DIMS, ids=ids(R.QR_DIMS, "D%d"))
def test_qr_every_lane_instance(lib, D, kind):
    check_qr(lib, qr_case(kind, R.QR_BAGS, D), R.OPS)


@gpu
@pytest.mark.parametrize("D", R.QR_DIMS_TWO_TRIPS, ids=ids(R.QR_DIMS_TWO_TRIPS, "D%d"))
def test_qr_two_column_trips(lib, D):
    check_qr(lib, qr_case("ragged", R.QR_BAGS, D), ("mult", "concat"))


@gpu
@pytest.mark.parametrize("D,n_bags,ops", [R.QR_CAP_64 + (("add", "mult"),), R.QR_CAP_4 + (("add",),)], ids=["lanes64", "lanes4"])
def test_qr_grid_cap(lib, D, n_bags, ops):
    check_qr(lib, qr_case("ones", n_bags, D), ops)


def device_table(kind, rows, D, salt=5):
    """RowIsIndex / FormulaTable on the device."""
    if kind == "index":
        return torch.arange(rows, dtype=torch.float32, device=DEV).view(-1, 1).repeat(1, D).contiguous()
    out = torch.empty(rows, D, dtype=torch.float32, device=DEV)
    d = torch.arange(D, dtype=torch.int64, device=DEV).view(1, -1)
    for r0 in range(0, rows, 1 << 20):
        i = torch.arange(r0, min(rows, r0 + (1 << 20)), dtype=torch.int64, device=DEV).view(-1, 1)
        out[r0:r0 + i.shape[0]] = ((i * 37 + d * 11 + salt) & 1023).to(torch.float32) / 1024.0 - 0.5
    return out


@gpu
@pytest.mark.parametrize("table,D", [("index", 4), ("formula", 64)], ids=["row-is-index-D4", "formula-D64"])
def test_qr_float32_quotient_in_ragged_bags(lib, table, D):
    """Ids of the 39 884 406-category table, c = 4, through the entry point: the quotient table holds max(q) + 1 rows whose
    contents are a function of the row number (Wq[i] = i at dim 4; at D = 64 the formula table, whose neighbouring rows
    differ by far more than a 1000-lookup bag's bound)."""
    off, n = R.bags("ragged", R.QR_BAGS)
    idx = R.quirk_ids(n)
    rows_q = int(R.quotient(idx, R.C4).max()) + 1
    assert rows_q == -(-R.N_C4 // R.C4)
    Wq = R.RowIsIndex(rows_q, D) if table == "index" else R.FormulaTable(rows_q, D, 5)
    c = types.SimpleNamespace(idx=idx, off=off, n=n, c=R.C4, D=D, rows_q=rows_q, Wq=Wq, Wr=R.weights(R.C4, D, 430 + D))
    ref = R.QR(idx, off, n, Wq, c.Wr, R.C4)
    d = (dev(idx), dev(off), device_table(table, rows_q, D), dev(c.Wr))
    probe = np.array([0, 1, rows_q // 2, rows_q - 1])
    same_bits(host(d[2][dev(probe)]), Wq[probe].astype(np.float32), "the device table is the restated one")
    for op in R.OPS:
        out, eq, er, _, _, err = qr_direct(lib, c, op, d)
        assert err == 0
        want, bound = ref.forward(op)
        within(out, want, bound, op)
        within(eq, ref.Eq, R.SLACK * ref.bEq, "eq_out")
    same_bits(host(d[0]), idx, "idx")
    same_bits(host(d[1]), off, "offsets")
    torch.cuda.synchronize()


@gpu
def test_qr_quotient_reaches_rows_q(lib):
    """N_TOP = 2^24 + 4 categories, c = 4: rows_q = 2^22 + 1, and the top id's float32 quotient is rows_q.  The kernel sets the
    error word and reads row 0 for that lookup; every other bag is the restatement's; the module raises IndexError."""
    from cdlrm_amd.tricks.qr_embedding_bag import QREmbeddingBag
    off, n = R.bags("ragged", R.QR_BAGS)
    L = R.bag_ends(off, n) - off
    b = int(np.flatnonzero(L == 7)[0])
    idx = R.top_ids(n, int(off[b]) + 3)
    rows_q, D = -(-R.N_TOP // R.C4), 4
    assert rows_q == int(R.quotient(idx, R.C4).max())
    Wq = R.RowIsIndex(rows_q, D)
    c = types.SimpleNamespace(idx=idx, off=off, n=n, c=R.C4, D=D, rows_q=rows_q, Wq=Wq, Wr=R.weights(R.C4, D, 430 + D))
    ref = R.QR(idx, off, n, Wq, c.Wr, R.C4, oob_row0=True)
    assert ref.outside.sum() == 1 and ref.bag[ref.outside][0] == b
    d = (dev(idx), dev(off), device_table("index", rows_q, D), dev(c.Wr))
    for op in ("add", "concat"):
        out, eq, er, _, _, err = qr_direct(lib, c, op, d)
        assert err == 1
        want, bound = ref.forward(op)
        within(out, want, bound, op)
        kept = R.QR(idx, off, n, R.RowIsIndex(rows_q + 1, D), c.Wr, R.C4).forward(op)
        assert abs(out[b, 0] - kept[0][b, 0]) > bound[b, 0] + kept[1][b, 0], "row 0, not row rows_q, went into the bag"
    E = QREmbeddingBag(R.N_TOP, D, R.C4, operation="add", mode="sum", _weight=[d[2], d[3]])
    with pytest.raises(IndexError):
        E(d[0], d[1])
    E(d[0][:int(off[b])], d[1][:b])                                # the lookups in front of it pass
    same_bits(host(d[0]), idx, "idx")
    torch.cuda.synchronize()


@gpu
@pytest.mark.parametrize("D", [16, 256], ids=["D16", "D256"])
def test_qr_contention(lib, D):
    """8192 float atomics on every element of one quotient row; remainder rows 1 and 2 get nothing and stay exactly 0.0."""
    c = qr_case("contention", 0, D)
    check_qr(lib, c, ("mult", "add"))
    d = (dev(c.idx), dev(c.off), dev(c.Wq), dev(c.Wr))
    for op in ("mult", "add"):
        _, _, _, gq, gr, _ = qr_direct(lib, c, op, d, grad_for(op, c.G, D))
        same_bits(gr[[1, 2]], np.zeros((2, D), np.float32), "the absent remainder rows")
        same_bits(np.delete(gq, 5, axis=0), np.zeros((c.rows_q - 1, D), np.float32), "the quotient rows nothing names")
    Gi = R.contention_grad(2 * D, "integers")[:, :D]               # every partial sum is an integer below 2^24: no rounding
    ref = R.QR(c.idx, c.off, c.n, c.Wq, c.Wr, c.c)
    want_q, _, want_r, _ = ref.backward("add", Gi)
    _, _, _, gq, gr, _ = qr_direct(lib, c, "add", d, Gi)
    same_bits(gq, want_q.astype(np.float32), "gWq of integer gradients")
    same_bits(gr, want_r.astype(np.float32), "gWr of integer gradients")
    torch.cuda.synchronize()


@gpu
def test_qr_without_pooled_operands(lib):
    """eq_out = er_out = NULL (and eq = er = NULL into the add backward): the guarded stores."""
    check_qr(lib, qr_case("ragged", R.QR_BAGS, 32), ("add",), module=False, operands=False)


@gpu
def test_offsets_none_for_2d_input(lib):
    from cdlrm_amd.tricks.md_embedding_bag import PrEmbeddingBag
    from cdlrm_amd.tricks.qr_embedding_bag import QREmbeddingBag
    B, Lb = 33, 3
    idx = R.small_ids(B * Lb, NCAT, 450)
    off = np.arange(0, B * Lb, Lb, dtype=np.int64)
    D = 20
    c = qr_case("ragged", R.QR_BAGS, D)
    G = np.random.RandomState(451).randn(B, 2 * D).astype(np.float32)
    ref = R.QR(idx, off, B * Lb, c.Wq, c.Wr, R.C4)
    d_idx = dev(idx.reshape(B, Lb))
    for op in R.OPS:
        E = QREmbeddingBag(NCAT, D, R.C4, operation=op, mode="sum", _weight=[dev(c.Wq), dev(c.Wr)])
        V = E(d_idx)
        want, bound = ref.forward(op)
        assert tuple(V.shape) == want.shape
        within(host(V), want, bound, op)
        V.backward(dev(grad_for(op, G, D)))
        gq, bq, gr, br = ref.backward(op, grad_for(op, G, D))
        within(host(E.weight_q.grad), gq, bq, "%s gWq" % op)
        within(host(E.weight_r.grad), gr, br, "%s gWr" % op)
    W = R.weights(NCAT, 5, 440)
    E = PrEmbeddingBag(NCAT, 5, 5).to(DEV)
    with torch.no_grad():
        E.embs.weight.copy_(dev(W))
    V = E(d_idx)
    bag = R.Bag(idx, off, B * Lb, W.shape)
    want, bound = bag.forward(W)
    assert tuple(V.shape) == want.shape
    within(host(V), want, bound, "bag")
    V.backward(dev(G[:, :5].copy()))
    gW, b = bag.backward(G[:, :5])
    within(host(E.embs.weight.grad), gW, b, "bag gW")
    same_bits(host(d_idx), idx.reshape(B, Lb), "idx")
    torch.cuda.synchronize()


@gpu
@pytest.mark.parametrize("what", ["qr-D16", "bag-D3"])
def test_five_empty_bags(lib, what):
    """No lookups at all: the index tensor has no address.  The reference returns zero rows; so do the modules, and the
    gradients are zero."""
    from cdlrm_amd.tricks.md_embedding_bag import PrEmbeddingBag
    from cdlrm_amd.tricks.qr_embedding_bag import QREmbeddingBag
    idx = torch.empty(0, dtype=torch.int64, device=DEV)
    off = torch.zeros(5, dtype=torch.int64, device=DEV)
    if what == "qr-D16":
        c = qr_case("ragged", R.QR_BAGS, 16)
        for op in R.OPS:
            E = QREmbeddingBag(NCAT, 16, R.C4, operation=op, mode="sum", _weight=[dev(c.Wq), dev(c.Wr)])
            V = E(idx, off)
            same_bits(host(V), np.zeros((5, 32 if op == "concat" else 16), np.float32), op)
            V.backward(torch.ones_like(V))
            same_bits(host(E.weight_q.grad), np.zeros_like(c.Wq), "gWq")
            same_bits(host(E.weight_r.grad), np.zeros_like(c.Wr), "gWr")
    else:
        E = PrEmbeddingBag(NCAT, 3, 3).to(DEV)
        V = E(idx, off)
        same_bits(host(V), np.zeros((5, 3), np.float32), "bag")
        V.backward(torch.ones_like(V))
        same_bits(host(E.embs.weight.grad), np.zeros((NCAT, 3), np.float32), "gW")
    torch.cuda.synchronize()


def bag_direct(lib, idx, off, n, W, G, d=None):
    """cdlrm_bag_fwd / cdlrm_bag_bwd on padded buffers -> (out, gW, err)."""
    L, nb, (rows, D) = lib.lib(), off.size, W.shape
    d = d or (dev(idx), dev(off), dev(W), dev(G))
    o, gW = out_buffer(nb * D), out_buffer(rows * D, zeros=True)
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    lib.check(L.cdlrm_bag_fwd(d[0].data_ptr(), d[1].data_ptr(), n, nb, d[2].data_ptr(), rows, D, o.data_ptr(), err.data_ptr(),
                              stream()))
    lib.check(L.cdlrm_bag_bwd(d[0].data_ptr(), d[1].data_ptr(), n, nb, d[3].data_ptr(), rows, D, gW.data_ptr(), stream()))
    for t, a, what in zip(d, (idx, off, W, G), ("idx", "offsets", "weight", "grad_out")):
        same_bits(host(t), a, what)
    return take(o, nb, D, "out"), take(gW, rows, D, "gW"), int(err.item())


def check_bag(lib, idx, off, n, D, seed):
    from cdlrm_amd.tricks.md_embedding_bag import PrEmbeddingBag
    W = R.weights(NCAT, D, seed)
    G = np.random.RandomState(seed + 1).randn(off.size, D).astype(np.float32)
    assert np.abs(G).min() > 0
    ref = R.Bag(idx, off, n, W.shape)
    want, bound = ref.forward(W)
    gW, bW = ref.backward(G)
    out, got_gW, err = bag_direct(lib, idx, off, n, W, G)
    assert err == 0
    within(out, want, bound, "out")
    within(got_gW, gW, bW, "gW")
    E = PrEmbeddingBag(NCAT, D, D).to(DEV)
    with torch.no_grad():
        E.embs.weight.copy_(dev(W))
    V = E.embs(dev(idx), dev(off))
    same_bits(host(V), out, "the module's forward and the entry point's")
    V.backward(dev(G))
    within(host(E.embs.weight.grad), gW, bW, "module gW")
    torch.cuda.synchronize()


@gpu
@pytest.mark.parametrize("kind", ["ragged", "closed_by_n"])
@pytest.mark.parametrize("D", R.BAG_DIMS, ids=ids(R.BAG_DIMS, "D%d"))
def test_bag_every_width(lib, D, kind):
    off, n = R.bags(kind, R.BAG_BAGS)
    assert R.BAG_BAGS * D > 256, "more than one 256-thread block"
    check_bag(lib, R.small_ids(n, NCAT, 460 + D), off, n, D, 470 + D)


@gpu
def test_bag_grid_cap(lib):
    D, n_bags = R.BAG_CAP
    off, n = R.cycle_bags(n_bags)
    check_bag(lib, bag_cap_ids(n), off, n, D, 481)


@gpu
def test_bag_backward_skips_ids_outside_the_table(lib):
    from cdlrm_amd.tricks.md_embedding_bag import PrEmbeddingBag
    D = 5
    off, n = R.bags("closed_by_n", R.QR_BAGS)
    idx = R.small_ids(n, NCAT, 490).copy()
    idx[[0, 5, n // 2, n - 1]] = [-1, NCAT, NCAT + 7, -(1 << 40)]
    W = R.weights(NCAT, D, 491)
    G = np.random.RandomState(492).randn(off.size, D).astype(np.float32)
    out, gW, err = bag_direct(lib, idx, off, n, W, G)
    assert err == 1
    want, bound = R.Bag(idx, off, n, W.shape, skip_outside=True).backward(G)
    within(gW, want, bound, "gW")
    E = PrEmbeddingBag(NCAT, D, D).to(DEV)
    with pytest.raises(IndexError):
        E(dev(idx), dev(off))
    torch.cuda.synchronize()


@gpu
@pytest.mark.parametrize("ed", [1, 2, 4], ids=["K1", "K2", "K4"])
def test_projection_of_pooled_rows(lib, ed):
    """PrEmbeddingBag(n, ed, 16): the pooled rows into the Linear kernels at K = ed.  The pooled rows against the restatement;
    the projection, its input gradient and its weight gradient against float64 products of the device's own operands within
    the fp32-route bound of tests/test_gemm_routes.py at that depth; the table gradient against the restated backward of the
    device's input gradient."""
    from cdlrm_amd import ops
    from cdlrm_amd.tricks.md_embedding_bag import PrEmbeddingBag
    from test_gemm_routes import assert_within
    base = 16
    off, n = R.bags("ragged", R.BAG_BAGS)
    idx = R.small_ids(n, NCAT, 500 + ed)
    nb = off.size
    rng = np.random.RandomState(510 + ed)
    W = R.weights(NCAT, ed, 520 + ed)
    P = (rng.randn(base, ed) / np.sqrt(ed)).astype(np.float32)
    G = rng.randn(nb, base).astype(np.float32)
    E = PrEmbeddingBag(NCAT, ed, base).to(DEV)
    with torch.no_grad():
        E.embs.weight.copy_(dev(W))
        E.proj.weight.copy_(dev(P))
    d_idx, d_off, dG = dev(idx), dev(off), dev(G)
    x = E.embs(d_idx, d_off)
    x.retain_grad()
    y = E.proj(x)
    y.backward(dG)
    bag = R.Bag(idx, off, n, W.shape)
    want, bound = bag.forward(W)
    within(host(x), want, bound, "pooled rows")
    x64, P64, G64 = host(x).astype(np.float64), P.astype(np.float64), G.astype(np.float64)
    assert_within(host(y), x64 @ P64.T, np.abs(x64) @ np.abs(P64).T, ed + 1, "projection")
    assert_within(host(x.grad), G64 @ P64, np.abs(G64) @ np.abs(P64), base + 5, "dX")
    routes = ops.linear_bwd_route(x.detach(), E.proj.weight.detach(), None, dG, torch.empty_like(x), torch.empty_like(E.proj.weight),
                                  None, ops.ACT["none"], n_cu=torch.cuda.get_device_properties(0).multi_processor_count)
    splits = routes[1]["splits"]
    k_eff = (nb if splits == 1 else -(-nb // splits) + 32 + splits) + 3
    assert_within(host(E.proj.weight.grad), G64.T @ x64, np.abs(G64).T @ np.abs(x64), k_eff, "dW")
    gW, bW = bag.backward(host(x.grad))
    within(host(E.embs.weight.grad), gW, bW, "table gradient")
    whole = E(d_idx, d_off)
    same_bits(host(whole), host(y), "the module's forward in one piece")
    same_bits(host(dG), G, "grad_out")
    torch.cuda.synchronize()
