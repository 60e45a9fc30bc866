"""Every kernel of the pairwise-dot interaction against a plain float64 reference, at its F, B and pitch edges.

interact_plan (csrc/dense.hip) sends cdlrm_interact_fwd / _bwd and the three fused gather + interaction calls to one of 29 kernel
instances by D, F, the row pitch of R / dR and the 16-byte alignment of R / dR and dfeat.  tests/test_interact_plan.py pins that
decision; this file checks the numbers.  One table of cases, each with the route it is meant to reach ("<family> <d4>"), serves

  * CPU: ops.interact_route on the case's facts gives the declared route for every `itself` and batch size, and a batch size the
    case declares as past the grid has grid < ceil(B / 4) -- some wave walks a second sample;
  * CPU: the table holds every instance with itself 0 / 1, x_act 0 / 1 / 2 (backward ops), B = 1, 3 and 4 * cap + 3 (8 * cap + 3 too
    for the gather kernels, which load slot ids two samples ahead);
  * CPU: one TrainEngine step per configuration (c2, c3; itself False / True; tests/fake_ops.py) records the step's interaction
    calls; every (op, route, itself, x_act, pad, alignment) they and their fused replacements resolve to is in the table;
  * GPU: each case runs its kernel at every batch size and compares EVERY element:
      R[:, :D]        feature 0, bit for bit
      pairs           |got - Z_ij| <= C * D * 2^-24 * sum_k |T_ik| |T_jk|             (an fp32 fma chain of length D)
      dfeat           |got - ref| <= C * (F + 2) * 2^-24 * mag * |act'| + 8 * 2^-24 * |ref|,  mag = sum_j |S_ij| |T_jc| (+ |dR_c| in
                      row 0): F products, the direct path, the activation factor; 8 ulp for the three roundings of v * ((1 - y) * y);
                      where the ReLU mask is 0 the bound is TINY: the kernel must give 0
    with S = G + G^T exact in fp32 (an entry of S is one gradient, or twice one on the diagonal under `itself`).  dR holds NaN in
    every column behind the pairs, the feature block handed to a gather kernel NaN outside feature 0, R and dfeat a sentinel that
    must survive wherever no output belongs.  No tolerance here is a measured number.

The comparator is checked on the CPU: a plain fp32 emulation passes, seven ways of being subtly wrong fail.
"""
import os
import sys
import zlib

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import test_gemm_routes as R      # noqa: E402
from test_gemm_routes import assert_within, U, C_BOUND, TINY, SENTINEL, _dev_operand, _gap_ok      # noqa: E402

ops = R.ops
DEV = R.DEV
NAN = float("nan")
FWD_OPS = ("fwd", "gather_fwd")
BWD_OPS = ("bwd", "gather_bwd", "gather_bwd_sgd")
GATHER_OPS = ("gather_fwd", "gather_bwd", "gather_bwd_sgd")
LR = float(np.float32(0.37))        # gather_bwd_sgd's learning rate, as the kernel receives it
WAYS, AUX, SETS = 4, 512, 61        # cache geometry of the gather cases: 61 sets x 4 ways + 512 auxiliary rows per table


def npairs_of(F, itself):
    return F * (F + 1) // 2 if itself else F * (F - 1) // 2


def pad4(w):
    return (w + 3) & ~3


def grid_cap(op, route):
    """Workgroups a launch is capped at (interact_plan at its default debug keys)."""
    fam, d4 = route.split()
    if fam == "generic":
        return 2048
    if fam == "row":
        return 512
    if op in FWD_OPS:
        return 256
    return 256 if d4 == "64" else 512


# ---- the case table -------------------------------------------------------------------------------------------------------

class Case:
    """One interaction call and the route it must take.  pad: ld_r - (D + npairs), or "p4" (the pitch rounded up to 4: the
    engine's) / "p4+4"; off_r / off_df: element offsets of R (forward) / dR (backward) and of dfeat from a 256-byte aligned base;
    Bs: the batch sizes, `past` those of them at which a wave must walk a second sample."""

    def __init__(self, cid, op, F, D, route, Bs=(1, 3), past=(), itselfs=(0, 1), x_acts=(0, 1, 2), pad="p4", off_r=0, off_df=0):
        assert set(past) <= set(Bs)
        self.id, self.op, self.F, self.D, self.route, self.Bs, self.past = cid, op, F, D, route, Bs, past
        self.itselfs, self.x_acts = itselfs, (x_acts if op in BWD_OPS else (None,))
        self.pad, self.off_r, self.off_df = pad, off_r, off_df

    def __repr__(self):
        return self.id

    def width(self, itself):
        return self.D + npairs_of(self.F, itself)

    def ld_r(self, itself):
        w = self.width(itself)
        return pad4(w) if self.pad == "p4" else pad4(w) + 4 if self.pad == "p4+4" else w + self.pad

    def aligned(self):
        return self.off_r % 4 == 0, self.off_df % 4 == 0

    def instance(self):
        return self.op, ("generic" if self.route.startswith("generic") else self.route)

    def keys(self):
        """(op, route, itself, x_act, pad, aligned) of every variant: what the step's calls are matched with."""
        return [(self.op, self.route, i, xa, self.ld_r(i) - self.width(i), self.aligned()) for i in self.itselfs for xa in self.x_acts]


def _cases():
    out = []

    def add(cid, op, F, D, route, Bs=(1, 3), **kw):
        past = tuple(b for b in Bs if b > 4 * grid_cap(op, route))
        out.append(Case(cid, op, F, D, route, Bs, past, **kw))

    # ---- cdlrm_interact_fwd, column slabs: whole-float4 output rows ----
    add("fwd_slab8_c2", "fwd", 27, 32, "slab 8", (1, 3, 1027))
    add("fwd_slab32_c3", "fwd", 27, 128, "slab 32", (1, 3, 1027))
    add("fwd_slab16_f32", "fwd", 32, 64, "slab 16", (1, 3, 1027), pad="p4+4")       # width % 4 == 0; itself: the full staging row
    add("fwd_slab64_f17", "fwd", 17, 256, "slab 64", (1, 3, 33, 1027))              # itself: width % 4 == 1
    add("fwd_slab8_f1", "fwd", 1, 32, "slab 8", (1, 3, 1027))                       # itself 0: no pairs at all
    add("fwd_slab16_f2", "fwd", 2, 64, "slab 16")                                   # itself 0: width % 4 == 1
    add("fwd_slab32_f16", "fwd", 16, 128, "slab 32", (1, 3, 1027))                  # acc10 / acc11 store nothing
    add("fwd_slab64_f32", "fwd", 32, 256, "slab 64")
    # ---- ... whole-row staging: by pitch, by a 4-byte offset of R on a pitch that is a multiple of 4 ----
    add("fwd_row32_pitch", "fwd", 27, 128, "row 32", (1, 3, 2051), pad=0)           # ld_r = 479 / 506
    add("fwd_row8_off", "fwd", 27, 32, "row 8", (1, 3, 2051), off_r=1)
    add("fwd_row16_off", "fwd", 17, 64, "row 16", (1, 3, 2051), off_r=1)
    add("fwd_row64_off", "fwd", 20, 256, "row 64", (1, 3, 2051), off_r=1)
    add("fwd_row32_f32", "fwd", 32, 128, "row 32", pad=1)
    add("fwd_row8_f1", "fwd", 1, 32, "row 8", off_r=2)
    add("fwd_row16_f16", "fwd", 16, 64, "row 16", pad=1)
    # ---- ... generic ----
    add("fwd_generic_d16", "fwd", 4, 16, "generic 4", (1, 3, 8195), pad=0)
    add("fwd_generic_d48", "fwd", 27, 48, "generic 12", (1, 3, 257))
    add("fwd_generic_d4", "fwd", 32, 4, "generic 1", (1, 3, 5), pad=0)
    add("fwd_generic_d316", "fwd", 2, 316, "generic 79", (1, 3, 9))                 # 162,816 B of LDS: the largest inside 160 KiB
    # ---- cdlrm_interact_bwd, column slabs: F > 16, whole-float4 dR rows, aligned dfeat ----
    for d4 in (8, 16, 32, 64):
        add("bwd_slab%d_f17" % d4, "bwd", 17, 4 * d4, "slab %d" % d4)               # the second half has one valid row
        add("bwd_slab%d_f32" % d4, "bwd", 32, 4 * d4, "slab %d" % d4, itselfs=(1,), pad="p4+4" if d4 == 16 else "p4")
    add("bwd_slab8_c2", "bwd", 27, 32, "slab 8", (1, 3, 2051))
    add("bwd_slab32_c3", "bwd", 27, 128, "slab 32")
    add("bwd_slab32_c3_loop", "bwd", 27, 128, "slab 32", (2051,), x_acts=(1, 2))
    add("bwd_slab64_loop", "bwd", 27, 256, "slab 64", (33, 1027))
    add("bwd_slab16_loop", "bwd", 20, 64, "slab 16", (2051,))
    # ---- ... whole-row staging: F <= 16, or an unaligned dfeat ----
    add("bwd_row8_f1", "bwd", 1, 32, "row 8")
    add("bwd_row32_f16", "bwd", 16, 128, "row 32", (1, 3, 2051))
    add("bwd_row32_f17_off", "bwd", 17, 128, "row 32", off_df=1)                     # rows 16..31 of the 32x32 tile
    add("bwd_row32_f32_off", "bwd", 32, 128, "row 32", off_df=1)
    add("bwd_row32_f32_loop", "bwd", 32, 128, "row 32", (2051,), itselfs=(1,), x_acts=(1, 2), off_df=1)
    add("bwd_row8", "bwd", 9, 32, "row 8", (1, 3, 2051))
    add("bwd_row16", "bwd", 12, 64, "row 16", (1, 3, 2051))
    add("bwd_row16_f2", "bwd", 2, 64, "row 16")
    # ---- ... generic ----
    add("bwd_generic_d16", "bwd", 4, 16, "generic 4", (1, 3, 8195), pad=0)
    add("bwd_generic_d48", "bwd", 27, 48, "generic 12", (1, 3, 257))
    add("bwd_generic_d256_f16", "bwd", 16, 256, "generic 64")
    add("bwd_generic_d256_f27_off", "bwd", 27, 256, "generic 64", off_df=1)
    add("bwd_generic_d128_f32_off", "bwd", 32, 128, "generic 32", itselfs=(1,), off_r=1)
    add("bwd_generic_d128_pitch", "bwd", 27, 128, "generic 32", pad=0)
    add("bwd_generic_d316", "bwd", 2, 316, "generic 79", (1, 3, 9))                 # 162,880 B of LDS: the budget's edge
    # ---- the fused gather + interaction calls: every width at F = 17 and F = 32, the step's F = 27 ----
    for op in GATHER_OPS:
        fwd = op == "gather_fwd"
        for d4 in (8, 16, 32, 64):
            route = ("slab_db %d" if fwd and d4 > 8 else "slab %d") % d4
            cap = grid_cap(op, route)
            add("%s_%d_f17" % (op, d4), op, 17, 4 * d4, route)
            add("%s_%d_f32" % (op, d4), op, 32, 4 * d4, route, pad="p4+4")
            # two, then three samples per wave
            loop = dict(itselfs=(0, 1) if d4 in (8, 64) else (d4 // 32,), x_acts=(1, 2))
            if d4 in (8, 32):
                add("%s_%d_c%d" % (op, d4, 2 if d4 == 8 else 3), op, 27, 4 * d4, route)
                add("%s_%d_loop" % (op, d4), op, 27, 4 * d4, route, (4 * cap + 3, 8 * cap + 3), **loop)
            else:
                add("%s_%d_loop" % (op, d4), op, 17 if d4 == 64 else 20, 4 * d4, route, (4 * cap + 3, 8 * cap + 3), **loop)
    add("gather_fwd_32_five_samples", "gather_fwd", 27, 128, "slab_db 32", (4099,), itselfs=(0,))
    return out


CASES = _cases()

INSTANCES = ([("fwd", "generic")] + [("fwd", "%s %d" % (f, d4)) for f in ("row", "slab") for d4 in (8, 16, 32, 64)]
             + [("bwd", "generic")] + [("bwd", "row %d" % d4) for d4 in (8, 16, 32)] + [("bwd", "slab %d" % d4) for d4 in (8, 16, 32, 64)]
             + [("gather_fwd", "slab 8")] + [("gather_fwd", "slab_db %d" % d4) for d4 in (16, 32, 64)]
             + [(op, "slab %d" % d4) for op in GATHER_OPS[1:] for d4 in (8, 16, 32, 64)])


# ---- the float64 reference -------------------------------------------------------------------------------------------------

def pair_ij(F, itself):
    """(i, j) of the pair columns in their order in R: row i of the lower triangle after row i - 1, the diagonal with `itself`."""
    return np.tril_indices(F, 0 if itself else -1)


def ref_fwd(T, itself):
    """Pair columns Z_ij = sum_k T_ik T_jk of a float64 [B, F, D] block, and sum_k |T_ik| |T_jk|."""
    i, j = pair_ij(T.shape[1], itself)
    A = np.abs(T)
    return (T @ T.transpose(0, 2, 1))[:, i, j], (A @ A.transpose(0, 2, 1))[:, i, j]


def ref_bwd(T, dR, itself, x_act):
    """dfeat of the float64 block T [B, F, D] and gradient rows dR [B, >= D + npairs] in the explicit form -- S = G + G^T
    (diagonal 2 G under itself), dT = S T, dT[0] += dR[:, :D], row 0 times act'(y) -- and the magnitudes of its sums."""
    B, F, D = T.shape
    i, j = pair_ij(F, itself)
    G = np.zeros((B, F, F))
    G[:, i, j] = dR[:, D:D + len(i)]
    S = G + G.transpose(0, 2, 1)
    dT, mag = S @ T, np.abs(S) @ np.abs(T)
    dT[:, 0] += dR[:, :D]
    mag[:, 0] += np.abs(dR[:, :D])
    m = R.act_grad(T[:, 0], x_act or 0)
    dT[:, 0] *= m
    mag[:, 0] *= np.abs(m)
    return dT, mag


def check_fwd(rows, T32, itself, what, route):
    """rows [B, >= width] as a forward kernel left them against the float32 block T32."""
    B, F, D = T32.shape
    width = D + npairs_of(F, itself)
    same = np.ascontiguousarray(rows[:, :D]).view(np.uint32) == np.ascontiguousarray(T32[:, 0]).view(np.uint32)
    assert same.all(), "%s: R[:, :D] is not feature 0 bit for bit (%d of %d elements)" % (what, int((~same).sum()), same.size)
    Z, mag = ref_fwd(T32.astype(np.float64), itself)
    assert_within(rows[:, D:width], Z, mag, D, what + " pairs", route, act_ulps=0.0)


def check_bwd(got, T32, dR32, itself, x_act, what, route):
    """dfeat [B, F, D] against the float64 reference; reported rows are sample * F + feature."""
    B, F, D = T32.shape
    ref, mag = ref_bwd(T32.astype(np.float64), dR32.astype(np.float64), itself, x_act)
    assert_within(np.asarray(got).reshape(B * F, D), ref.reshape(B * F, D), mag.reshape(B * F, D), F + 2, what + " dfeat", route)


def draw_block(rng, B, F, D):
    return rng.standard_normal((B, F, D), dtype=np.float32)


def draw_row0(rng, B, D, x_act):
    """Feature 0 as a valid output of the activation under test: relu(randn) -- half the entries exact zeros --, sigmoid(randn)."""
    v = rng.standard_normal((B, D), dtype=np.float32)
    return {0: v, 1: np.maximum(v, np.float32(0)), 2: (1 / (1 + np.exp(-v.astype(np.float64)))).astype(np.float32)}[x_act or 0]


def seed_of(*parts):
    return zlib.crc32(" ".join(str(p) for p in parts).encode())


# ---- CPU: the reference and the comparator ---------------------------------------------------------------------------------

def test_explicit_reference_equals_autograd_on_the_oracle():
    """ref_fwd / ref_bwd are the oracle's interact_features and its autograd gradient (float64, x_act through sigmoid / relu)."""
    from oracle import cdlrm_oracle as O
    rng = np.random.default_rng(5)
    for F, D, itself in ((1, 8, 0), (1, 8, 1), (5, 12, 0), (17, 8, 1)):
        for x_act in (0, 1, 2):
            B = 3
            pre = torch.from_numpy(rng.standard_normal((B, D))).requires_grad_(True)
            rest = torch.from_numpy(rng.standard_normal((B, F - 1, D))).requires_grad_(True)
            x = {0: pre, 1: torch.relu(pre), 2: torch.sigmoid(pre)}[x_act]
            out = O.interact_features(x, [rest[:, k, :] for k in range(F - 1)], "dot", bool(itself))
            width = D + npairs_of(F, itself)
            assert out.shape == (B, width)
            dR = rng.standard_normal((B, width + 2))
            out.backward(torch.from_numpy(dR[:, :width].copy()))
            T = np.concatenate([x.detach().numpy()[:, None, :], rest.detach().numpy()], axis=1)
            Z, _ = ref_fwd(T, itself)
            np.testing.assert_allclose(out.detach().numpy()[:, D:], Z, rtol=1e-13, atol=1e-13)
            assert np.array_equal(out.detach().numpy()[:, :D], T[:, 0])
            dT, _ = ref_bwd(T, dR, itself, x_act)
            np.testing.assert_allclose(dT[:, 0], pre.grad.numpy(), rtol=1e-12, atol=1e-13)
            if F > 1:
                np.testing.assert_allclose(dT[:, 1:], rest.grad.numpy(), rtol=1e-12, atol=1e-13)


def emu_fwd(T32, itself):
    """A correct un-fused fp32 forward: sequential multiply-add over the contraction index (test_gemm_routes._seq_fp32)."""
    B, F, D = T32.shape
    acc = np.zeros((B, F, F), dtype=np.float32)
    for k in range(D):
        acc = (acc + T32[:, :, None, k] * T32[:, None, :, k]).astype(np.float32)
    i, j = pair_ij(F, itself)
    return np.concatenate([T32[:, 0], acc[:, i, j]], axis=1)


def emu_bwd(T32, dR32, itself, x_act, direct=True, mask_row=0, mask_act=None, diagonal_twice=True):
    """A correct un-fused fp32 backward -- and, through the keywords, the ways of being wrong the controls try."""
    B, F, D = T32.shape
    i, j = pair_ij(F, itself)
    G = np.zeros((B, F, F), dtype=np.float32)
    G[:, i, j] = dR32[:, D:D + len(i)]
    S = G + G.transpose(0, 2, 1)
    if not diagonal_twice:
        d = np.arange(F)
        S[:, d, d] = G[:, d, d]
    acc = np.zeros((B, F, D), dtype=np.float32)
    for jj in range(F):
        acc = (acc + S[:, :, jj, None] * T32[:, jj, None, :]).astype(np.float32)
    v = acc[:, 0] + dR32[:, :D] if direct else acc[:, 0]
    y = T32[:, mask_row]
    a = x_act if mask_act is None else mask_act
    if a == 1:
        v = np.where(y > 0, v, np.float32(0))
    elif a == 2:
        v = v * ((np.float32(1) - y) * y)
    acc[:, 0] = v
    return acc


def _control_inputs(rng, B, F, D, itself, x_act):
    T32 = draw_block(rng, B, F, D)
    T32[:, 0] = draw_row0(rng, B, D, x_act)
    dR32 = rng.standard_normal((B, D + npairs_of(F, itself)), dtype=np.float32)
    return T32, dR32


CONTROL_SHAPES = ((1, 32), (2, 316), (16, 64), (17, 128), (27, 128), (32, 48), (32, 256))


def test_comparator_passes_a_plain_fp32_emulation():
    """Sequential fp32 multiply-add, forward and backward, is inside the bound at seven shapes, F 1..32 and D 32..316."""
    rng = np.random.default_rng(11)
    for F, D in CONTROL_SHAPES:
        for itself in (0, 1):
            for x_act in (0, 1, 2):
                T32, dR32 = _control_inputs(rng, 3, F, D, itself, x_act)
                if x_act == 0:
                    check_fwd(emu_fwd(T32, itself), T32, itself, "emulated forward", "slab")
                check_bwd(emu_bwd(T32, dR32, itself, x_act), T32, dR32, itself, x_act, "emulated backward", "slab")


def test_comparator_negative_controls():
    """Each of these fails the bound: two pair columns swapped, the direct path left out of row 0, x_act ignored, the sigmoid
    factor used for ReLU, the mask taken from row 1, the diagonal of S counted once under itself, a NaN anywhere."""
    rng = np.random.default_rng(12)
    B, F, D = 3, 27, 128
    for itself in (0, 1):
        T32, dR32 = _control_inputs(rng, B, F, D, itself, 1)
        rows = emu_fwd(T32, itself)
        check_fwd(rows, T32, itself, "correct", "slab")
        bad = rows.copy()
        bad[:, [D + 40, D + 41]] = bad[:, [D + 41, D + 40]]
        with pytest.raises(AssertionError, match="pairs"):
            check_fwd(bad, T32, itself, "pair columns swapped", "slab")
        bad = rows.copy()
        bad[1, 5] = np.nextafter(bad[1, 5], np.float32(9))
        with pytest.raises(AssertionError, match="bit for bit"):
            check_fwd(bad, T32, itself, "feature 0 off by one ulp", "slab")
        for col in (D - 1, D, rows.shape[1] - 1):
            bad = rows.copy()
            bad[2, col] = np.nan
            with pytest.raises(AssertionError):
                check_fwd(bad, T32, itself, "NaN", "slab")
        for x_act in (0, 1, 2):
            T32[:, 0] = draw_row0(rng, B, D, x_act)
            check_bwd(emu_bwd(T32, dR32, itself, x_act), T32, dR32, itself, x_act, "correct", "slab")
            # (mask_act: the activation the emulation applies instead of x_act; 0 is "x_act ignored")
            wrong = [dict(direct=False)] + [dict(mask_act=a) for a in (0, 1, 2) if a != x_act]
            if x_act:
                wrong.append(dict(mask_row=1))
            if itself:
                wrong.append(dict(diagonal_twice=False))
            for kw in wrong:
                with pytest.raises(AssertionError, match="dfeat"):
                    check_bwd(emu_bwd(T32, dR32, itself, x_act, **kw), T32, dR32, itself, x_act, repr(kw), "slab")
            bad = emu_bwd(T32, dR32, itself, x_act)
            bad[2, F - 1, D - 1] = np.nan
            with pytest.raises(AssertionError, match="row %d, col %d" % (2 * F + F - 1, D - 1)):
                check_bwd(bad, T32, dR32, itself, x_act, "NaN", "slab")
    # where the ReLU mask is 0 the kernel must give 0: the smallest float fails
    T32, dR32 = _control_inputs(rng, B, F, D, 0, 1)
    bad = emu_bwd(T32, dR32, 0, 1)
    b, c = np.argwhere(T32[:, 0] == 0)[0]
    bad[b, 0, c] = np.float32(1e-20)
    with pytest.raises(AssertionError, match="dfeat"):
        check_bwd(bad, T32, dR32, 0, 1, "masked element not 0", "slab")


# ---- CPU: the table --------------------------------------------------------------------------------------------------------

def _route(ops, case, B, itself, aligned=None):
    a_r, a_df = case.aligned() if aligned is None else aligned
    return ops.interact_route(case.op, B, case.F, case.D, bool(itself), case.ld_r(itself), a_r, a_df)


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.id)
def test_declared_route(ops, case):
    """The library's plan for the case's facts is the declared route at every itself and B; a B declared past the grid is."""
    for itself in case.itselfs:
        for B in case.Bs:
            r = _route(ops, case, B, itself)
            assert "%s %d" % (r["family"], r["d4"]) == case.route, (case.id, itself, B, r)
            assert r["lds_bytes"] <= 160 * 1024
            if B in case.past:
                assert r["grid"] < -(-B // 4), (case.id, B, r)
            else:
                assert r["grid"] == -(-B // 4), (case.id, B, r)


def test_table_holds_every_instance_at_every_edge():
    """All 29 kernel instances, each with itself 0 and 1, the backward ones with x_act 0, 1 and 2, each at B = 1, 3 and 4 * cap + 3
    (the gather kernels at 8 * cap + 3 too); B = 8195 only on the generic kernels at D = 16, F = 4; nothing above B = 4099 at
    F = 27, D = 128 otherwise."""
    assert len(INSTANCES) == len(set(INSTANCES)) == 29
    assert {c.instance() for c in CASES} == set(INSTANCES)
    assert len({c.id for c in CASES}) == len(CASES)
    for inst in INSTANCES:
        mine = [c for c in CASES if c.instance() == inst]
        assert {i for c in mine for i in c.itselfs} == {0, 1}, inst
        if inst[0] in BWD_OPS:
            assert {x for c in mine for x in c.x_acts} == {0, 1, 2}, inst
        cap = grid_cap(inst[0], mine[0].route)
        Bs = {b for c in mine for b in c.Bs}
        past = {b for c in mine for b in c.past}
        assert {1, 3} <= Bs and 4 * cap + 3 in past, (inst, Bs)
        if inst[0] in GATHER_OPS:
            assert 8 * cap + 3 in past, (inst, Bs)
    for c in CASES:
        big = max(c.Bs)
        if big > 4099:
            assert big == 8195 and (c.F, c.D) == (4, 16) and c.route == "generic 4", c.id
        assert big * c.F * c.D <= 4099 * 27 * 128, c.id
    assert {c.D for c in CASES if c.route.startswith("generic")} >= {4, 16, 48, 316}


@pytest.mark.parametrize("config", sorted(R.STEP_CONFIGS))
@pytest.mark.parametrize("itself", [False, True])
def test_training_step_interactions_are_in_the_table(ops, config, itself):
    """The interaction calls of one training step (c2 / c3, 26 tables), and the fused calls the GPU engine makes in their place
    wherever gather_interact_supported holds, each with its own route, itself, x_act, pad and alignment: a variant of some case."""
    calls = []
    R._record_step(config, 1024, itself=itself, interactions=calls)
    assert [c[0] for c in calls] == ["fwd", "bwd"], calls
    table = set()
    for c in CASES:
        table.update(c.keys())
    missing = []
    for op0, F, D, its, x_act, ld_r, a_r, a_df in calls:
        assert its == int(itself) and (F, D) == (27, R.STEP_CONFIGS[config]["D"])
        assert x_act == (None if op0 == "fwd" else 1), "the step's bottom MLP ends in ReLU"
        for op in ((op0, "gather_fwd") if op0 == "fwd" else (op0, "gather_bwd", "gather_bwd_sgd")):
            r = ops.interact_route(op, 1024, F, D, bool(its), ld_r, a_r, a_df)
            key = (op, "%s %d" % (r["family"], r["d4"]), its, x_act, ld_r - (D + npairs_of(F, its)), (a_r, a_df))
            if key not in table:
                missing.append(key)
    assert not missing, "step calls the table lacks: %r" % missing


# ---- the gather cases' cache geometry, slot ids and once flags (numpy: the same on the CPU and the GPU) ----------------------

def gather_geometry(case):
    rng = np.random.RandomState(seed_of(case.id))
    ln = [int(v) for v in rng.randint(50, 90000, size=case.F - 1)]
    cs = [min(SETS, v) for v in ln]
    return ln, cs, [c * WAYS + AUX for c in cs]            # (cache rows + the auxiliary rows behind them: all are slot targets)


def gather_slots(case, B, itself):
    """slots int32 [T, n = B + 3] -- valid ids in the pitch gap too -- drawn per table from a window of min(B, rows) ids, so that
    about a third of a batch's lookups are the only one of their slot (fewer once B exceeds a table's rows); once uint8
    [T, n + 5]: the count of the slot id within its table and batch is 1."""
    rows_of = gather_geometry(case)[2]
    rng = np.random.RandomState(seed_of(case.id, B, itself))
    T, n = case.F - 1, B + 3
    slots = np.zeros((T, n), dtype=np.int32)
    once = np.zeros((T, n + 5), dtype=np.uint8)
    for k in range(T):
        span = max(2, min(B, rows_of[k]))
        slots[k] = rng.randint(0, rows_of[k] - span + 1) + rng.randint(0, span, size=n)
        cnt = np.bincount(slots[k, :B], minlength=rows_of[k])
        once[k, :B] = cnt[slots[k, :B]] == 1
    return slots, once


@pytest.mark.parametrize("case", [c for c in CASES if c.op in GATHER_OPS], ids=lambda c: c.id)
def test_gather_slots_are_valid_and_both_classes_occur(case):
    rows_of = gather_geometry(case)[2]
    for itself in case.itselfs:
        for B in case.Bs:
            slots, once = gather_slots(case, B, itself)
            assert (slots >= 0).all() and (slots < np.array(rows_of)[:, None]).all()
            assert not once[:, B:].any()
            if B >= 64:
                assert once[:, :B].any() and not once[:, :B].all(), (case.id, B)
                assert (slots >= np.array(rows_of)[:, None] - AUX).any(), "auxiliary rows are slot targets"


# ---- GPU: every case against float64 -----------------------------------------------------------------------------------------

def _check_R(buf, case, B, itself):
    """The whole allocation behind R: rows [B, ld_r] at off_r.  Returns the rows.  Nothing outside pad4(width) columns is written;
    the pad word (columns width .. pad4(width) - 1) is 0 on the slab routes, 0 or untouched on the others."""
    ld, width, off = case.ld_r(itself), case.width(itself), case.off_r
    rows = buf[off:off + B * ld].reshape(B, ld)
    assert (buf[:off] == SENTINEL).all() and (buf[off + B * ld:] == SENTINEL).all(), "%s: written outside R" % case.id
    w4 = pad4(width)
    padw = rows[:, width:min(w4, ld)]
    if case.route.startswith("slab"):
        assert ld >= w4 and (padw == 0).all(), "%s B=%d: the pad word of a slab route is not 0" % (case.id, B)
    else:
        assert ((padw == 0) | (padw == SENTINEL)).all(), "%s B=%d: pad word" % (case.id, B)
    assert (rows[:, w4:] == SENTINEL).all(), "%s B=%d: R written behind pad4(width)" % (case.id, B)
    return rows


class _Gather:
    """Context, cache rows and slot ids of a gather case on the device; w0: the rows as float32 numpy."""

    def __init__(self, ops, case):
        self.ops, self.case = ops, case
        ln, cs, self.rows_of = gather_geometry(case)
        self.ctx = ops.CacheCtx(ln, cs, case.D, WAYS, AUX, torch.device(DEV))
        assert ops.gather_interact_supported(self.ctx)
        assert self.ctx.rows == self.rows_of
        rng = np.random.default_rng(seed_of(case.id, "rows"))
        self.w0 = rng.standard_normal((self.ctx.total_rows, case.D), dtype=np.float32)
        self.weight = torch.from_numpy(self.w0).to(DEV)
        self.w0_dev = self.weight.clone()
        tags = torch.full((self.ctx.total_tags,), -1, dtype=torch.int64, device=DEV)
        self.ctx.bind_cache(tags, self.weight)
        self.row_base = np.array(self.ctx.row_base[:case.F - 1], dtype=np.int64)

    def batch(self, B, itself):
        """Slot ids and flags on the device; global row [B, T] of every lookup; the gathered rows [B, T, D] (CPU gather)."""
        slots, once = gather_slots(self.case, B, itself)
        self.once = once[:, :B].T.astype(bool)                      # [B, T]
        self.rows = (slots[:, :B] + self.row_base[:, None]).T       # [B, T]
        self.slots_d = torch.from_numpy(slots).to(DEV)
        self.once_d = torch.from_numpy(once).to(DEV)
        self.ld_once = once.shape[1]
        return self.w0[self.rows]

    def x_view(self, row0):
        """Feature 0 as row 0 of a [B, F, D] block whose other features hold NaN."""
        block = torch.full((row0.shape[0], self.case.F, self.case.D), NAN, device=DEV)
        block[:, 0, :] = torch.from_numpy(row0).to(DEV)
        return block[:, 0, :]


def _real_route(ops, case, B, itself, r_op, dfeat):
    r = _route(ops, case, B, itself, (r_op.data_ptr() % 16 == 0, dfeat is None or dfeat.data_ptr() % 16 == 0))
    got = "%s %d" % (r["family"], r["d4"])
    assert got == case.route, "%s B=%d itself=%d: the library takes %r, the case is meant for %r" % (case.id, B, itself, got, case.route)


def _run_forward(ops, case, g, B, itself, zero):
    rng = np.random.default_rng(seed_of(case.id, B, itself, "feat"))
    F, D = case.F, case.D
    T32 = draw_block(rng, B, F, D)
    if g is not None:
        T32[:, 1:] = g.batch(B, itself)
        x = g.x_view(T32[:, 0])
    else:
        fd = torch.from_numpy(T32).to(DEV)
    Rv, Rbuf = _dev_operand(B, case.width(itself), case.ld_r(itself), case.off_r, None, SENTINEL)
    _real_route(ops, case, B, itself, Rv, None)

    def call():
        if g is not None:
            ops.gather_interact_fwd(g.ctx, g.slots_d, x, bool(itself), Rv)
        else:
            ops.interact_fwd(fd, bool(itself), Rv)
        torch.cuda.synchronize()

    if zero:        # B = 0 with the operands' real addresses (an empty tensor has none): straight to the C entry point
        from cdlrm_amd import _lib
        if g is not None:
            _lib.check(_lib.lib().cdlrm_gather_interact_fwd(g.ctx.handle, g.slots_d.data_ptr(), g.slots_d.stride(0), x.data_ptr(),
                                                            x.stride(0), 0, itself, Rv.data_ptr(), Rv.stride(0), None))
        else:
            _lib.check(_lib.lib().cdlrm_interact_fwd(fd.data_ptr(), 0, F, D, itself, Rv.data_ptr(), Rv.stride(0), None))
        torch.cuda.synchronize()
        assert bool((Rbuf == SENTINEL).all()), "%s: B = 0 wrote R" % case.id
    call()
    first = Rbuf.clone()
    call()
    assert torch.equal(first, Rbuf), "%s B=%d itself=%d: two calls differ" % (case.id, B, itself)
    rows = _check_R(Rbuf.cpu().numpy(), case, B, itself)
    check_fwd(rows, T32, itself, "%s B=%d itself=%d" % (case.id, B, itself), case.route)


def _run_backward(ops, case, g, B, itself, zero):
    rng = np.random.default_rng(seed_of(case.id, B, itself, "feat"))
    F, D, width, ld = case.F, case.D, case.width(itself), case.ld_r(itself)
    T32 = draw_block(rng, B, F, D)
    if g is not None:
        T32[:, 1:] = g.batch(B, itself)
    dR32 = rng.standard_normal((B, width), dtype=np.float32)
    dR_src = torch.from_numpy(dR32).to(DEV)
    sgd = case.op == "gather_bwd_sgd"
    for x_act in case.x_acts:
        what = "%s B=%d itself=%d x_act=%d" % (case.id, B, itself, x_act)
        T32[:, 0] = draw_row0(rng, B, D, x_act)
        if g is not None:
            x = g.x_view(T32[:, 0])
        else:
            fd = torch.from_numpy(T32).to(DEV)
        dRv, _ = _dev_operand(B, width, ld, case.off_r, dR_src, NAN)            # NaN in every column >= D + npairs
        dfbuf = torch.full((case.off_df + B * F * D + 4,), SENTINEL, dtype=torch.float32, device=DEV)
        dfeat = dfbuf[case.off_df:case.off_df + B * F * D].view(B, F, D)
        _real_route(ops, case, B, itself, dRv, dfeat)

        def call():
            if sgd:
                g.weight.copy_(g.w0_dev)
                ops.gather_interact_bwd_sgd(g.ctx, g.slots_d, x, dRv, bool(itself), dfeat, g.once_d.data_ptr(), g.ld_once, LR,
                                            x_act=x_act)
            elif g is not None:
                ops.gather_interact_bwd(g.ctx, g.slots_d, x, dRv, bool(itself), dfeat, x_act=x_act)
            else:
                ops.interact_bwd(fd, dRv, bool(itself), dfeat, x_act=x_act)
            torch.cuda.synchronize()

        if zero and x_act == case.x_acts[0]:        # B = 0 with the operands' real addresses: straight to the C entry point
            from cdlrm_amd import _lib
            L = _lib.lib()
            if g is not None:
                head = (g.ctx.handle, g.slots_d.data_ptr(), g.slots_d.stride(0), x.data_ptr(), x.stride(0), dRv.data_ptr(), ld, 0,
                        itself, x_act, dfeat.data_ptr())
                _lib.check(L.cdlrm_gather_interact_bwd_sgd(*head, g.once_d.data_ptr(), g.ld_once, LR, None) if sgd
                           else L.cdlrm_gather_interact_bwd(*head, None))
            else:
                _lib.check(L.cdlrm_interact_bwd(fd.data_ptr(), dRv.data_ptr(), ld, 0, F, D, itself, x_act, dfeat.data_ptr(), None))
            torch.cuda.synchronize()
            assert bool((dfbuf == SENTINEL).all()), "%s: B = 0 wrote dfeat" % case.id
            assert g is None or torch.equal(g.weight, g.w0_dev), "%s: B = 0 wrote cache rows" % case.id
        call()
        first = dfbuf.clone()
        w_first = g.weight.clone() if sgd else None
        call()
        assert torch.equal(first, dfbuf), what + ": two calls differ"
        assert _gap_ok(dRv, ld, width, NAN) and torch.equal(dRv, dR_src), what + ": dR was written"
        buf = dfbuf.cpu().numpy()
        n_out = B * F * D
        assert (buf[:case.off_df] == SENTINEL).all() and (buf[case.off_df + n_out:] == SENTINEL).all(), what + ": written outside dfeat"
        got = buf[case.off_df:case.off_df + n_out].reshape(B, F, D)
        if not sgd:
            assert g is None or torch.equal(g.weight, g.w0_dev), what + ": cache rows were written"
            check_bwd(got, T32, dR32, itself, x_act, what, case.route)
            continue
        # ---- gather_bwd_sgd: once-only lookups update their cache row instead of leaving a gradient row ----
        assert torch.equal(w_first, g.weight), what + ": two calls leave different cache rows"
        T = F - 1
        ref, mag = ref_bwd(T32.astype(np.float64), dR32.astype(np.float64), itself, x_act)
        once = g.once
        assert (got[:, 1:T][once[:, :T - 1]] == SENTINEL).all(), what + ": gradient row of a once-only lookup written"
        # (the last table's once-only rows: the store's spare lanes may repeat the row's last word of a 32-column block, which
        #  is its gradient; every element is the sentinel or inside the bound)
        chk = got.copy()
        skip = once[:, :, None] & (chk[:, 1:] == SENTINEL)
        chk[:, 1:][skip] = ref[:, 1:][skip]
        assert_within(chk.reshape(B * F, D), ref.reshape(B * F, D), mag.reshape(B * F, D), F + 2, what + " dfeat", case.route)
        W1 = g.weight.cpu().numpy()
        hit = g.rows[once]                                          # [K] global rows, each named by exactly one lookup
        assert len(set(hit.tolist())) == hit.size
        g_ref, g_mag = ref[:, 1:][once], mag[:, 1:][once]           # [K, D]
        w_ref = g.w0[hit].astype(np.float64) - LR * g_ref
        bound = LR * (C_BOUND * (F + 2) * U * g_mag + 8 * U * np.abs(g_ref) + TINY) + 2 * U * np.abs(w_ref) + TINY
        err = np.abs(W1[hit].astype(np.float64) - w_ref)
        bad = ~(err <= bound)
        assert not bad.any(), "%s: %d of %d cache-row elements outside the bound, worst %.3g x" % (
            what, int(bad.sum()), bad.size, float(np.where(np.isnan(err), np.inf, err / bound).max()))
        rest = np.ones(W1.shape[0], dtype=bool)
        rest[hit] = False
        assert np.array_equal(W1[rest].view(np.uint32), g.w0[rest].view(np.uint32)), what + ": another cache row changed"


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=lambda c: c.id)
def test_route_vs_float64(ops, case):
    g = _Gather(ops, case) if case.op in GATHER_OPS else None
    run = _run_forward if case.op in FWD_OPS else _run_backward
    first = True
    for itself in case.itselfs:
        for B in case.Bs:
            run(ops, case, g, B, itself, zero=first)
            first = False
