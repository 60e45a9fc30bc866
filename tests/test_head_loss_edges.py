"""The output head and the loss kernels against plain float64 references, at their B, K, alignment and stride edges.

head_plan (csrc/dense.hip) sends cdlrm_head_fwd_bwd to one of four k_head<VEC, TAIL> instances and, inside them, to one of three inner
paths -- "one" (a float4 per lane, K <= 256), "multi" (float4 trips of 256 columns), "scalar" -- by K, the two row pitches and the
16-byte alignment of Y, w and dY; the grid is capped at 1024 workgroups of 16 rows (B > 16384: several passes with clamped rows) and
the loss is finished in the launch ("tail": finish and B <= 2048), by a k_head_finish launch ("finish"), or left as partial sums
("partials": finish=False, the training step's form).  One table of cases, each with the route it is meant to reach, serves

  * CPU: ops.head_route on the case's integer alignment facts gives the declared route, with finish and without;
  * CPU: one TrainEngine step per configuration (tests/fake_ops.py) records the real head_fwd_bwd arguments; every (route, x_act,
    kind, thr > 0) they resolve to is a variant of some case;
  * GPU: each case asks the route with its real pointers, asserts it, runs the kernel and compares EVERY element in two stages:
      1. Z against float64 sigmoid(Y w + b):  |dp| <= p (1 - p) C L 2^-24 (|Y| |w| + |b|)_row + A 2^-24 p,  L the longest fp32 chain
         of the path (ceil(K / 64) or 4 ceil(K / 256) fmas, 6 butterfly adds, the bias add), C = 2, A = 8 (test_gemm_routes');
      2. everything downstream against float64 evaluated on the kernel's OWN Z (read back as fp32): Zc the bit-exact clamp,
         loss[1] the exact count of rint(Zc) == t, dZ within DZ_ULPS = 10 roundings (z - t, 1 - z, the product, the division, w / n
         -- two for wbce's fp32 weight --, the product, 1 - p, its product, the last product), dY = dZ w act'(Y) within 3 more and
         exactly 0 where the mask is 0, loss[0] within (D + A) 2^-24 sum|l_i| / B of the float64 mean (D = passes + 4 waves +
         ceil(grid / 64) + 6: the summation depth), loss[2] == fl32(fl32(loss[0]) * B), and the tail / finish form of a case bit for
         bit the head_finish form.
    Y's and w's surroundings hold NaN, every output's a sentinel that must survive.

The other loss entry points -- cdlrm_bce_fwd_bwd on both sides of its switch to k_bce_partial (whose partial sums, found in
loss_buf[1:65] or not, prove the route), cdlrm_loss_fwd_bwd at z == thr, 1 - thr and their fp32 neighbours, cdlrm_act_bwd with pitches
and past its grid cap, cdlrm_scale_div bit for bit against float32 division -- are held to the same stage-2 reference.

No tolerance here is a measured number.  Largest error / bound seen on the MI355X (every case of this file; the GPU tests print
them per case):
    head Z 0.18, dZ 0.37, dY 0.44, loss 0.14;  bce dZ 0.38, loss 0.045, a partial sum 0.091;
    loss_fwd_bwd dZ 0.35, loss 0.075;  act_bwd (sigmoid) 0.82;  scale_div: bit-equal.
The comparator is checked on the CPU: a plain fp32 emulation of the head passes, nine ways of being subtly wrong fail.
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
from test_gemm_routes import U, C_BOUND, TINY, SENTINEL, _dev_operand, _gap_ok      # noqa: E402

ops = R.ops
DEV = R.DEV
NAN = float("nan")
A_ULPS = 8.0            # the activation allowance of test_gemm_routes: expf / logf / log1pf and the roundings around them
DZ_ULPS = 10.0          # roundings between the prediction and dZ (module docstring)
DY_ULPS = 3.0
F32, F64 = np.float32, np.float64
FLOOR = float(F32(1e-12))       # binary_cross_entropy_backward's denominator floor, as an fp32 kernel holds it
KINDS = {"bce": 0, "mse": 1, "wbce": 2}
WS = (0.3, 1.7)
WORST = {}              # quantity -> largest error / bound of the running test (the GPU tests print it)


def seed_of(*parts):
    return zlib.crc32(" ".join(str(p) for p in parts).encode())


def cdiv(a, b):
    return -(-a // b)


def pad4(w):
    return (w + 3) & ~3


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=F32)).view(np.uint32)


# ---- comparator -----------------------------------------------------------------------------------------------------------

def within(got, ref, bound, what, q):
    """|got - ref| <= bound element by element (NaN fails); notes the largest error / bound under quantity `q`."""
    got = np.asarray(got, dtype=F64)
    ref = np.asarray(ref, dtype=F64)
    bound = np.broadcast_to(np.asarray(bound, dtype=F64), ref.shape)
    err = np.abs(got - ref)
    ratio = np.where(np.isnan(err), np.inf, err / bound)
    worst = float(ratio.max()) if ratio.size else 0.0
    WORST[q] = max(WORST.get(q, 0.0), worst)
    ok = err <= bound
    if ok.all():
        return worst
    i = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
    raise AssertionError("%s %s: %d of %d elements outside the bound; worst at %r: got %r, want %r, |err| %.3g > bound %.3g" % (
        what, q, int((~ok).sum()), ok.size, tuple(int(x) for x in i), float(got[i]), float(ref[i]), float(err[i]), float(bound[i])))


def chain_len(path, K):
    """The kernel's longest fp32 chain of one logit: the lane's fmas, 6 butterfly adds, the bias add."""
    return (cdiv(K, 64) if path == "scalar" else 4 * cdiv(K, 256)) + 6 + 1


def ref_logits(Y32, w32, b32):
    Y, w = Y32.astype(F64), w32.astype(F64)
    b = 0.0 if b32 is None else float(b32)
    return Y @ w + b, np.abs(Y) @ np.abs(w) + abs(b)


def check_Z(Z, Y32, w32, b32, path, what):
    """Stage 1: the prediction against float64 sigmoid(Y w + b)."""
    x, mag = ref_logits(Y32, w32, b32)
    p, q = 1.0 / (1.0 + np.exp(-x)), 1.0 / (1.0 + np.exp(x))
    bound = p * q * C_BOUND * chain_len(path, Y32.shape[1]) * U * mag + A_ULPS * U * p + TINY
    return within(Z, p, bound, what, "Z")


def clamp_of(p32, thr):
    """(clamped prediction fp32, pass mask) as torch.clamp(z, min=thr, max=1.0 - thr) and its backward on a float32 tensor."""
    p32 = np.asarray(p32, dtype=F32)
    if not 0.0 < thr < 1.0:
        return p32, np.ones(p32.shape, dtype=bool)
    lo, hi = F32(thr), F32(1.0 - thr)
    return np.minimum(np.maximum(p32, lo), hi), (p32 >= lo) & (p32 <= hi)


def loss_terms(zc, t, kind, n, ws=WS):
    """float64 loss terms l_i (before the mean) and dL/dzc of the torch formulas: binary_cross_entropy's log clamp at -100, its
    backward's denominator floor, weights[t] * BCE for wbce with w / n, mse_loss."""
    zc, t = np.asarray(zc, dtype=F64), np.asarray(t, dtype=F64)
    if kind == 1:
        return (zc - t) ** 2, 2.0 * (zc - t) / n
    with np.errstate(divide="ignore", invalid="ignore"):
        l1, l0 = np.maximum(np.log(zc), -100.0), np.maximum(np.log1p(-zc), -100.0)
    wt = np.where(t == 0, ws[0], ws[1]) if kind == 2 else np.ones_like(t)
    return ((t - 1.0) * l0 - t * l1) * wt, (zc - t) / np.maximum((1.0 - zc) * zc, FLOOR) * (wt / n)


def check_loss_side(p32, t32, kind, thr, out, depth, what, sigmoid_bwd=True, count=True, q=""):
    """Stage 2 on the prediction p32 the kernel itself used: out = dict(Zc, dZ, loss) as numpy (Zc / dZ may be None).  Returns the
    float64 dZ."""
    p32, t32 = np.asarray(p32, dtype=F32).ravel(), np.asarray(t32, dtype=F32).ravel()
    n = p32.size
    zc32, passm = clamp_of(p32, thr)
    if out.get("Zc") is not None:
        same = bits(out["Zc"]).ravel() == bits(zc32)
        assert same.all(), "%s: Zc is not the clamp of Z bit for bit (%d of %d elements)" % (what, int((~same).sum()), n)
    l, g = loss_terms(zc32, t32, kind, n)
    p = p32.astype(F64)
    dz = np.where(passm, g, 0.0) * ((1.0 - p) * p if sigmoid_bwd else 1.0)
    if out.get("dZ") is not None:
        got = np.asarray(out["dZ"], dtype=F32).ravel()
        assert (got[~passm] == 0).all(), "%s: a gradient outside [thr, 1 - thr] is not exactly 0" % what
        within(got, dz, DZ_ULPS * U * np.abs(dz) + TINY, what, q + "dZ")
    loss = np.asarray(out["loss"], dtype=F32)
    within(loss[:1], [l.sum() / n], (depth + A_ULPS) * U * np.abs(l).sum() / n + TINY, what, q + "loss")
    if count:
        want = int((np.rint(zc32) == t32).sum())
        assert float(loss[1]) == want, "%s: loss[1] = %r, %d predictions round to their target" % (what, float(loss[1]), want)
        assert bits(loss[2]) == bits(F32(loss[0]) * F32(n)), "%s: loss[2] is not fl32(loss[0] * n)" % what
    return dz


def check_head(out, Y32, w32, b32, t32, kind, thr, x_act, route, what):
    """Both stages on everything one head call wrote: out = dict(Z, Zc, dZ, dY, loss)."""
    B, K = Y32.shape
    check_Z(out["Z"], Y32, w32, b32, route["path"], what)
    depth = route["passes"] + 4 + cdiv(route["grid"], 64) + 6
    dz = check_loss_side(out["Z"], t32, kind, thr, out, depth, what)
    if out.get("dY") is not None:
        m = R.act_grad(Y32.astype(F64), x_act)
        ref = dz[:, None] * w32.astype(F64)[None, :] * m
        got = np.asarray(out["dY"], dtype=F32)
        dead = (m == 0) | (dz == 0)[:, None]
        assert (got[dead] == 0).all(), "%s: dY is not exactly 0 where its mask is 0" % what
        within(got, ref, (DZ_ULPS + DY_ULPS) * U * np.abs(ref) + TINY, what, "dY")


# ---- the case table ---------------------------------------------------------------------------------------------------------

DEFAULT_VARIANT = ("bce", 0.0, 1, True)         # (kind, thr, x_act, Zc given): the training step's
ROTATION = (DEFAULT_VARIANT, ("wbce", 0.2, 2, False), ("mse", 0.0, 0, True))
SATURATED = (30.0, -30.0, 120.0, -120.0, 0.0)   # logits of the engineered rows, each with target 0 and 1


class Case:
    """One head call and the route it must take with finish=True: "<path> <tail|finish>[ x<passes>]" (finish=False: "partials" in
    place of the mode).  off*: element offsets of Y, w, dY from a 256-byte aligned base; ldy / lddy: row pitches (default: 4 and 8
    words wider than pad4(K)); variants: (kind, thr, x_act, Zc given); sat: the engineered saturated rows lead the batch."""

    def __init__(self, cid, B, K, route, variants=(DEFAULT_VARIANT,), offy=0, offw=0, offdy=0, ldy=None, lddy=None, has_dY=True,
                 bias=True, sat=False):
        self.id, self.B, self.K, self.route, self.variants = cid, B, K, route, tuple(variants)
        self.offy, self.offw, self.offdy = offy, offw, offdy
        self.ldy, self.lddy = ldy or pad4(K) + 4, lddy or pad4(K) + 8
        self.has_dY, self.bias, self.sat = has_dY, bias, sat

    def __repr__(self):
        return self.id

    def aligned(self):
        return int(self.offy % 4 == 0) | int(self.offw % 4 == 0) << 1 | int(self.offdy % 4 == 0) << 2

    def routes(self):
        """(finish, declared route) of the two forms every case runs."""
        words = self.route.split()
        return [(True, self.route), (False, " ".join([words[0], "partials"] + words[2:]))]

    def keys(self):
        """(route with the pass count reduced to "multipass", x_act, kind, thr > 0): what the step's calls are matched with."""
        return [(key_route(r), xa, KINDS[kind], thr > 0) for _, r in self.routes() for kind, thr, xa, _ in self.variants]


def route_str(r):
    mode = "tail" if r["tail"] else "finish" if r["finish_launch"] else "partials"
    return "%s %s" % (r["path"], mode) + (" x%d" % r["passes"] if r["passes"] > 1 else "")


def key_route(route):
    words = route.split()
    return " ".join(words[:2] + (["multipass"] if len(words) > 2 else []))


B_EDGES = (1, 3, 4, 5, 15, 16, 17, 2048, 2049, 16384, 16385, 40000)
K_SCALAR, K_ONE, K_MULTI = (1, 5, 479), (4, 24, 32, 64, 252, 256), (260, 512, 516, 1024)


def path_of_k(K):
    return "scalar" if K in K_SCALAR else "one" if K in K_ONE else "multi"


def mode_of_b(B):
    """What finish=True does at B, and the passes: a workgroup is 4 waves x 4 rows, the tail serves 128 workgroups, the grid 1024."""
    return ("tail" if B <= 2048 else "finish") + ("" if B <= 16384 else " x2" if B <= 32768 else " x3")


def _cases():
    out, seen = [], set()

    def add(cid, B, K, route, **kw):
        if (B, K) in seen and not kw:
            return
        if not kw:
            seen.add((B, K))
        out.append(Case(cid, B, K, route, **kw))

    # ---- B edges: one workgroup and its neighbours, tail | finish launch, one pass | a second of one live row, three passes ----
    for K in (256, 260, 5):
        for B in B_EDGES:
            add("b%d_k%d" % (B, K), B, K, "%s %s" % (path_of_k(K), mode_of_b(B)))
    # ---- K edges: scalar with one trip and several, one float4 trip with idle lanes and full, several with a last trip of one lane
    for i, K in enumerate(K_SCALAR + K_ONE + K_MULTI):
        for B in (17, 2049):
            if (B, K) in seen:
                continue
            seen.add((B, K))
            out.append(Case("b%d_k%d" % (B, K), B, K, "%s %s" % (path_of_k(K), mode_of_b(B)), variants=(ROTATION[i % 3],)))
    # ---- alignment: every one of these sends a K % 4 == 0 call to the scalar path; dY = None keeps the vector path ----
    for K in (256, 512):
        add("k%d_y_off" % K, 17, K, "scalar tail", offy=1)
        add("k%d_w_off" % K, 17, K, "scalar tail", offw=1)
        add("k%d_dy_off" % K, 17, K, "scalar tail", offdy=1)
        add("k%d_ldy_odd" % K, 17, K, "scalar tail", ldy=K + 1)
        add("k%d_lddy_odd" % K, 17, K, "scalar tail", lddy=K + 2)
        add("k%d_no_dy" % K, 17, K, "%s tail" % path_of_k(K), has_dY=False, lddy=K + 1, offdy=1)
        add("k%d_no_dy_finish" % K, 2049, K, "%s finish" % path_of_k(K), has_dY=False)
    # ---- loss and activation: kind x thr x x_act x Zc, on the vector path past the tail and on the scalar path inside it ----
    for B, K in ((2049, 256), (17, 5)):
        for kind in KINDS:
            add("b%d_k%d_%s" % (B, K, kind), B, K, "%s %s" % (path_of_k(K), mode_of_b(B)),
                variants=[(kind, thr, xa, zc) for thr in (0.0, 0.2) for xa in (0, 1, 2) for zc in (True, False)])
    # ---- engineered rows: p exactly 1, 9.36e-14, exactly 1 and 0, exactly 0.5 (no bias), each with both targets ----
    for K in (64, 260, 5):
        add("saturated_k%d" % K, 32, K, "%s tail" % path_of_k(K), bias=False, sat=True,
            variants=[(kind, thr, 0, True) for kind in KINDS for thr in (0.0, 0.2)])
    return out


CASES = _cases()


# ---- the cases' data (numpy: the same on the CPU and the GPU) ---------------------------------------------------------------

_DATA = {}


def head_data(case, x_act):
    """Y [B, K], w [K], b or None, t [B] as float32.  Y: a third exact zeros among normals (the ReLU mask sees negatives too), or
    sigmoid outputs with exact 0 and 1 (x_act 2); w scaled so that the logits spread over a few units and stay within +-12."""
    key = (case.id, x_act)
    if key in _DATA:
        return _DATA[key]
    rng = np.random.default_rng(seed_of(case.id, x_act))
    B, K = case.B, case.K
    v, u = rng.standard_normal((B, K), dtype=F32), rng.random((B, K))
    if x_act == 2:
        Y = (1.0 / (1.0 + np.exp(-v.astype(F64)))).astype(F32)
        Y[u < 0.05], Y[u > 0.95] = 0.0, 1.0
    else:
        Y = v.copy()
        Y[u < 0.3] = 0.0
    w = rng.standard_normal(K)
    if x_act == 2 and K > 1:
        w -= w.mean()                   # (no common offset of the logits: both clamps are reached)
    b = F32(0.3) if case.bias else None
    x = Y.astype(F64) @ w
    rms = float(np.sqrt(np.mean(x * x)))
    w *= 2.5 / rms if rms > 0 else 1.0
    top = float(np.abs(Y.astype(F64) @ w).max())
    if top > 11.0:
        w *= 11.0 / top
    w32 = w.astype(F32)
    t = (rng.random(B) < 0.5).astype(F32)
    if B >= 2:
        t[:2] = (0.0, 1.0)
    if case.sat:
        w64 = w32.astype(F64)
        for i, s in enumerate(SATURATED):
            Y[2 * i:2 * i + 2] = (s * w64 / (w64 @ w64)).astype(F32)
            t[2 * i:2 * i + 2] = (0.0, 1.0)
    _DATA[key] = (Y, w32, b, t)
    if len(_DATA) > 8:
        _DATA.pop(next(iter(_DATA)))
    return _DATA[key]


# ---- CPU: the expectations at saturation rest on torch, the float64 formulas on torch's ----------------------------------------

def test_torch_fp32_saturation_facts():
    """binary_cross_entropy in torch fp32 on the CPU: terms 0 / 100 / 100 / 0 at (p, t) = (0, 0), (1, 0), (0, 1), (1, 1), gradient
    +-1e12 / n, pre-activation gradient exactly 0; sigmoid(+-30) = 1 and a normal 9.36e-14, sigmoid(+-120) = 1 and 0; 0.5 rounds
    to 0.  loss_terms gives the same numbers."""
    pre = torch.tensor([-120.0, 120.0, -120.0, 120.0], requires_grad=True)
    t = torch.tensor([0.0, 0.0, 1.0, 1.0])
    p = torch.sigmoid(pre)
    p.retain_grad()
    assert p.tolist() == [0.0, 1.0, 0.0, 1.0]
    assert torch.nn.functional.binary_cross_entropy(p, t, reduction="none").tolist() == [0.0, 100.0, 100.0, 0.0]
    torch.nn.functional.binary_cross_entropy(p, t).backward()
    assert p.grad.tolist() == [0.0, float(F32(1.0) / F32(1e-12) / F32(4.0)), -float(F32(1.0) / F32(1e-12) / F32(4.0)), 0.0]
    np.testing.assert_allclose(p.grad.abs().numpy()[1:3], 1e12 / 4, rtol=1e-6)
    assert pre.grad.tolist() == [0.0, 0.0, 0.0, 0.0]
    l, g = loss_terms(p.detach().numpy(), t.numpy(), 0, 4)
    assert l.tolist() == [0.0, 100.0, 100.0, 0.0]
    np.testing.assert_allclose(g, p.grad.numpy().astype(F64), rtol=1e-7)
    s = torch.sigmoid(torch.tensor([30.0, -30.0]))
    assert float(s[0]) == 1.0 and abs(float(s[1]) / 9.3576e-14 - 1) < 1e-4 and float(s[1]) > 1.2e-38
    assert float(torch.round(torch.tensor(0.5))) == 0.0 and np.rint(F32(0.5)) == 0.0 and np.rint(F32(1.5)) == 2.0
    # the clamp's upper end in fp32 arithmetic (1.0f - thr) is the float32 of the double 1.0 - thr at the thresholds used here
    for thr in (0.2, 0.45, 0.48):
        assert F32(1.0) - F32(thr) == F32(1.0 - thr)


@pytest.mark.parametrize("kind", sorted(KINDS))
@pytest.mark.parametrize("thr", [0.0, 0.2])
def test_float64_formulas_equal_torch_autograd(kind, thr):
    """clamp_of + loss_terms + the sigmoid backward restate the oracle's loss_fn under autograd (float64)."""
    from oracle import cdlrm_oracle as O
    rng = np.random.default_rng(3)
    n = 40
    p32 = rng.random(n).astype(F32)
    p32[:6] = (0.2, 0.8, np.nextafter(F32(0.2), F32(0)), np.nextafter(F32(0.8), F32(1)), 1e-9, 1.0 - 2.0 ** -24)
    t = np.round(rng.random(n))
    z = torch.from_numpy(p32.astype(F64)).requires_grad_(True)
    zc = torch.clamp(z, min=float(F32(thr)), max=float(F32(1.0 - thr))) if thr > 0 else z
    E = O.loss_fn(zc.view(-1, 1), torch.from_numpy(t).view(-1, 1), kind, torch.tensor(WS, dtype=torch.float64))
    E.backward()
    zc32, passm = clamp_of(p32, thr)
    l, g = loss_terms(zc32, t, KINDS[kind], n)
    np.testing.assert_allclose(l.sum() / n, float(E.detach()), rtol=1e-13)
    np.testing.assert_allclose(np.where(passm, g, 0.0), z.grad.numpy(), rtol=1e-6, atol=0)     # (FLOOR is the fp32 1e-12)
    assert np.array_equal(zc32.astype(F64), zc.detach().numpy())
    if thr > 0:
        assert passm[:2].all() and not passm[2:4].any()


# ---- CPU: the comparator's controls -----------------------------------------------------------------------------------------

def emu_head(Y, w, b, t, kind, thr, x_act, drop_k=None, no_bias=False, mask_shift=0, n_off=0, count_off=0, drop_group=None):
    """A plain fp32 head: sequential multiply-add over k, the kernel's element formulas, the loss summed by groups of 16 rows --
    and, through the keywords, the ways of being wrong the controls try."""
    B, K = Y.shape
    one = F32(1.0)
    acc = np.zeros(B, dtype=F32)
    for k in range(K):
        if k != drop_k:
            acc = (acc + Y[:, k] * w[k]).astype(F32)
    if b is not None and not no_bias:
        acc = (acc + b).astype(F32)
    with np.errstate(over="ignore", divide="ignore", invalid="ignore"):
        p = (one / (one + np.exp(-acc))).astype(F32)
        zc, passm = clamp_of(p, thr)
        n = F32(B + n_off)
        if kind == 1:
            df = zc - t
            l, g = df * df, F32(2.0) * df * (one / n)
        else:
            l1, l0 = np.maximum(np.log(zc), F32(-100.0)), np.maximum(np.log1p(-zc), F32(-100.0))
            l = (t - one) * l0 - t * l1
            go = np.full(B, one / n, dtype=F32)
            if kind == 2:
                wt = np.where(t == 0, F32(WS[0]), F32(WS[1])).astype(F32)
                l, go = l * wt, (wt.astype(F64) / F64(n)).astype(F32)
            g = (zc - t) / np.maximum((one - zc) * zc, F32(1e-12)) * go
        dz = (np.where(passm, g, F32(0.0)) * ((one - p) * p)).astype(F32)
    Ym = np.roll(Y, mask_shift, axis=0)
    m = {0: np.ones_like(Y), 1: (Ym > 0).astype(F32), 2: (one - Ym) * Ym}[x_act]
    dY = (dz[:, None] * w[None, :] * m).astype(F32)
    parts = [l[i:i + 16].astype(F32).sum(dtype=F32) for i in range(0, B, 16)]
    tot = F32(sum(x for i, x in enumerate(parts) if i != drop_group))
    loss0 = F32(tot / F32(B))
    cnt = int((np.rint(zc) == t).sum()) + count_off
    return dict(Z=p, Zc=zc, dZ=dz, dY=dY, loss=np.array([loss0, cnt, loss0 * F32(B)], dtype=F32))


def _control_case(B, K, path, x_act):
    case = Case("control_%d_%d" % (B, K), B, K, path + " finish")
    Y, w, b, t = head_data(case, x_act)
    route = dict(path=path, grid=min(cdiv(B, 16), 1024), passes=cdiv(B, 16 * min(cdiv(B, 16), 1024)))
    return Y, w, b, t, route


@pytest.mark.parametrize("B,K,path", [(2049, 256, "one"), (300, 260, "multi"), (300, 479, "scalar"), (17, 5, "scalar")])
def test_comparator_passes_a_plain_fp32_emulation(B, K, path):
    for kind in (0, 1, 2):
        for thr in (0.0, 0.2):
            for x_act in (0, 1, 2):
                Y, w, b, t, route = _control_case(B, K, path, x_act)
                check_head(emu_head(Y, w, b, t, kind, thr, x_act), Y, w, b, t, kind, thr, x_act, route, "emulated head")


def test_comparator_negative_controls():
    """Each of these fails: one dropped y_k w_k term of typical magnitude, a missing bias, the mask of the neighbouring row,
    1 / (B + 1) for 1 / B, a count off by one, a loss without one workgroup's partial, a clamped prediction one ulp off, a masked
    dY element that is not 0, a NaN."""
    B, K = 2049, 256
    for x_act in (1, 2):
        Y, w, b, t, route = _control_case(B, K, "one", x_act)
        args = (Y, w, b, t, 0, 0.2, x_act)

        def run(what, **kw):
            check_head(emu_head(*args, **kw), Y, w, b, t, 0, 0.2, x_act, route, what)

        run("correct")
        k = int(np.argsort(np.abs(w))[K // 2])          # the weight of median magnitude
        with pytest.raises(AssertionError, match=" Z:"):
            run("a k term dropped", drop_k=k)
        with pytest.raises(AssertionError, match=" Z:"):
            run("no bias", no_bias=True)
        with pytest.raises(AssertionError, match="dY"):
            run("mask of the neighbouring row", mask_shift=1)
        with pytest.raises(AssertionError, match=" dZ:"):
            run("1 / (B + 1)", n_off=1)
        with pytest.raises(AssertionError, match=r"loss\[1\]"):
            run("count off by one", count_off=1)
        with pytest.raises(AssertionError, match=" loss:"):
            run("a workgroup's partial missing", drop_group=7)
        good = emu_head(*args)
        bad = dict(good, Zc=good["Zc"].copy())
        bad["Zc"][5] = np.nextafter(bad["Zc"][5], F32(2))
        with pytest.raises(AssertionError, match="bit for bit"):
            check_head(bad, Y, w, b, t, 0, 0.2, x_act, route, "Zc one ulp off")
        bad = dict(good, dY=good["dY"].copy())
        r, c = np.argwhere(R.act_grad(Y.astype(F64), x_act) == 0)[0]
        bad["dY"][r, c] = F32(1e-20)
        with pytest.raises(AssertionError, match="exactly 0"):
            check_head(bad, Y, w, b, t, 0, 0.2, x_act, route, "masked element not 0")
        for q in ("Z", "dZ", "dY", "loss"):
            bad = dict(good, **{q: good[q].copy()})
            bad[q].reshape(-1)[0] = np.nan
            with pytest.raises(AssertionError):
                check_head(bad, Y, w, b, t, 0, 0.2, x_act, route, "NaN in " + q)
    # at the largest batch the 1 / (B + 1) control still fails
    Y, w, b, t, route = _control_case(40000, 5, "scalar", 1)
    with pytest.raises(AssertionError, match=" dZ:"):
        check_head(emu_head(Y, w, b, t, 0, 0.0, 1, n_off=1), Y, w, b, t, 0, 0.0, 1, route, "1 / (B + 1)")


# ---- CPU: the table -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", CASES, ids=lambda c: c.id)
def test_declared_route(ops, case):
    """The library's plan for the case's integer facts is the declared route, with finish and without."""
    for finish, want in case.routes():
        r = ops.head_route(case.B, case.K, case.ldy, case.lddy, case.aligned(), case.has_dY, finish)
        assert route_str(r) == want, (case.id, finish, r)
        assert r["grid"] == min(cdiv(case.B, 16), 1024) and r["passes"] == cdiv(case.B, 16 * r["grid"])
        assert r["vec"] == (r["path"] != "scalar")


def test_table_holds_every_path_at_every_edge():
    ids = [c.id for c in CASES]
    assert len(ids) == len(set(ids))
    for K in (256, 260, 5):
        assert {c.B for c in CASES if c.K == K and len(c.variants) == 1 and c.has_dY and c.aligned() == 7} >= set(B_EDGES), K
    for B in (17, 2049):
        assert {c.K for c in CASES if c.B == B} >= set(K_SCALAR + K_ONE + K_MULTI), B
    routes = {c.route for c in CASES}
    assert routes >= {"%s %s" % (p, m) for p in ("one", "multi", "scalar") for m in ("tail", "finish", "finish x2", "finish x3")}
    for K in (256, 512):        # every alignment fact alone sends the call to the scalar path
        facts = {(c.offy, c.offw, c.offdy, c.ldy % 4, c.lddy % 4) for c in CASES if c.K == K and c.route == "scalar tail"}
        assert facts >= {(1, 0, 0, 0, 0), (0, 1, 0, 0, 0), (0, 0, 1, 0, 0), (0, 0, 0, 1, 0), (0, 0, 0, 0, 2)}, K
        assert {c.route for c in CASES if c.K == K and not c.has_dY} == {path_of_k(K) + " tail", path_of_k(K) + " finish"}
    for B, K in ((2049, 256), (17, 5)):
        got = {v for c in CASES if (c.B, c.K) == (B, K) for v in c.variants}
        assert got >= {(k, thr, xa, zc) for k in KINDS for thr in (0.0, 0.2) for xa in (0, 1, 2) for zc in (True, False)}
    assert max(c.B * c.K for c in CASES) == 40000 * 260


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.id)
def test_fixture_classes_are_present(case):
    """What the GPU test relies on is in the data of every case that claims it: logits within +-12 (the engineered rows aside),
    zero-mask elements, both targets, rows clamped low and high under a threshold, the saturated rows at their logits."""
    for x_act in sorted({v[2] for v in case.variants}):
        Y, w, b, t = head_data(case, x_act)
        assert Y.shape == (case.B, case.K) and w.shape == (case.K,) and Y.dtype == w.dtype == t.dtype == F32
        x, _ = ref_logits(Y, w, b)
        free = x[2 * len(SATURATED):] if case.sat else x
        assert np.abs(free).max() <= 12.0
        if case.B * case.K >= 64:
            if x_act:
                assert (R.act_grad(Y.astype(F64), x_act) == 0).any() and (R.act_grad(Y.astype(F64), x_act) != 0).any()
            if x_act == 1:
                assert (Y < 0).any()
            if x_act == 2:
                assert (Y == 0).any() and (Y == 1).any() and Y.min() >= 0 and Y.max() <= 1
        if case.B >= 2:
            assert set(t.tolist()) == {0.0, 1.0}
        if case.B >= 17 and any(v[1] > 0 for v in case.variants):
            p = 1.0 / (1.0 + np.exp(-x))
            assert (p < 0.19).any() and (p > 0.81).any() and ((p > 0.21) & (p < 0.79)).any(), case.id
        if case.sat:
            assert b is None
            for i, s in enumerate(SATURATED):
                assert np.abs(x[2 * i:2 * i + 2] - s).max() <= 1e-4 and t[2 * i:2 * i + 2].tolist() == [0.0, 1.0]


# ---- CPU: the training step's head calls are in the table -------------------------------------------------------------------

STEP_SHAPES = {     # bench.py's layer shapes (test_gemm_routes.STEP_CONFIGS) and the small models of tests/test_engine_parity.py
    "c2": dict(R.STEP_CONFIGS["c2"], T=26),
    "c3": dict(R.STEP_CONFIGS["c3"], T=26),
    "top24": dict(D=16, bot=[13, 32, 16], top=[24, 1], T=4),
    "top64": dict(D=16, bot=[13, 32, 16], top=[64, 1], T=4),
}
STEP_RUNS = ([(c, b, "dot", "bce", None, 0.0) for c in ("c2", "c3") for b in (1024, 2048, 4096, 8192, 65536)]
             + [("top24", 48, "cat", "bce", None, 0.0), ("top24", 48, "dot", "mse", None, 0.0),
                ("top24", 48, "dot", "wbce", (0.4, 2.5), 0.0), ("top24", 48, "cat", "wbce", (1.5, 0.7), 0.45),
                ("top24", 48, "dot", "bce", None, 0.48), ("top64", 48, "dot", "bce", None, 0.0)])


def _record_head_calls(shape, Bsz, op, loss, ws, thr):
    """One TrainEngine step on the CPU test double (tests/fake_ops.py, as test_gemm_routes._record_step) with head_fwd_bwd
    wrapped: its real arguments."""
    import fake_ops
    import cdlrm_amd.engine as engine
    import cdlrm_amd.model_no_ddp as Mo
    from oracle import cdlrm_oracle as O
    cfg = STEP_SHAPES[shape]
    calls = []

    def head(Y, w, bias, target, Z, dZ, dY, loss_buf, scratch, *, x_act=0, kind=0, weights=(1.0, 1.0), threshold=0.0, Zc=None,
             finish=True, stream=None):
        aligned = (int(Y.data_ptr() % 16 == 0) | int(w.data_ptr() % 16 == 0) << 1
                   | int(dY is None or dY.data_ptr() % 16 == 0) << 2)
        calls.append(dict(B=Y.shape[0], K=Y.shape[1], ldy=Y.stride(0), lddy=0 if dY is None else dY.stride(0), aligned=aligned,
                          has_dY=dY is not None, x_act=int(x_act), kind=int(kind), thr=float(threshold), finish=bool(finish),
                          bias=bias is not None))
        return fake_ops.head_fwd_bwd(Y, w, bias, target, Z, dZ, dY, loss_buf, scratch, x_act=x_act, kind=kind, weights=weights,
                                     threshold=threshold, Zc=Zc, finish=finish, stream=stream)

    class Ops:
        pass

    shim = Ops()
    shim.__dict__.update({k: getattr(fake_ops, k) for k in dir(fake_ops) if not k.startswith("__")})
    shim.head_fwd_bwd = head
    saved = (engine.ops, Mo.ops, Mo.Embedding_Table_Group.__dict__.get("device_pointers"))
    engine.ops, Mo.ops = shim, shim
    Mo.Embedding_Table_Group.device_pointers = lambda self: self._fake_ptrs
    try:
        T, rows, D = cfg["T"], 40, cfg["D"]
        ln_emb = np.array([rows] * T)
        nf = T + 1
        ln_top = np.array([D + nf * (nf - 1) // 2 if op == "dot" else nf * D] + cfg["top"])
        host = O.init_host_tables([int(x) for x in ln_emb], D)
        eg = Mo.Embedding_Table_Group(D, ln_emb, init="empty_meta")
        for k in range(T):
            eg.emb_l[k].weight.data = host[k]
        eg._fake_ptrs = fake_ops.register_host(host)
        eg._pinned = True
        np.random.seed(1)
        torch.manual_seed(1)
        cg = Mo.Embedding_Table_Cache_Group(D, ln_emb, 64, Bsz, 4)
        dl = Mo.DLRM_Net(np.array(cfg["bot"]), ln_top, op, False, True, -1, ln_top.size - 2, thr)
        eng = engine.TrainEngine(cg, dl, eg, lr=0.1, lr_embeds=0.1, loss=loss, loss_weights=ws or (1.0, 1.0))
        assert eng.fused_head
        pipe = engine.WindowPipeline(cg, eg, Bsz, parity_rng=True)
        rng = np.random.RandomState(0)
        X = torch.from_numpy(rng.rand(Bsz, cfg["bot"][0]).astype(F32))
        idx = torch.from_numpy(rng.randint(0, rows, size=(T, Bsz)).astype(np.int64))
        Tt = torch.from_numpy(np.round(rng.rand(Bsz, 1)).astype(F32))
        pipe.plan_window(idx)
        pipe.commit()
        pipe.wait_writeback()
        eng.step(X, idx, Tt, j=0)
        eng.finish()
    finally:
        engine.ops, Mo.ops = saved[0], saved[1]
        if saved[2] is None:
            del Mo.Embedding_Table_Group.device_pointers
        else:
            Mo.Embedding_Table_Group.device_pointers = saved[2]
    return calls


@pytest.mark.parametrize("run", STEP_RUNS, ids=lambda r: "%s_b%d_%s_%s_thr%g" % (r[0], r[1], r[2], r[3], r[5]))
def test_training_step_head_calls_are_in_the_table(ops, run):
    """The head call of one training step, resolved with ops.head_route on its real pitches and alignment: a variant of some case."""
    shape, Bsz, op, loss, ws, thr = run
    calls = _record_head_calls(shape, Bsz, op, loss, ws, thr)
    assert len(calls) == 1, calls
    c = calls[0]
    assert (c["B"], c["K"]) == (Bsz, STEP_SHAPES[shape]["top"][-2]) and c["kind"] == KINDS[loss] and c["thr"] == thr
    assert c["has_dY"] and c["bias"] and c["x_act"] == 1, "the step's top MLP runs ReLU in front of its 1-wide layer"
    r = ops.head_route(c["B"], c["K"], c["ldy"], c["lddy"], c["aligned"], c["has_dY"], c["finish"])
    assert r["vec"], "the step's head call is meant for the float4 paths: %r -> %r" % (c, r)
    table = set()
    for case in CASES:
        if case.has_dY and case.bias:
            table.update(case.keys())
    key = (key_route(route_str(r)), c["x_act"], c["kind"], c["thr"] > 0)
    assert key in table, "a head call the table lacks: %r <- %r" % (key, c)


# ---- GPU: every head case against float64 ----------------------------------------------------------------------------------

def _guarded(n, gap=SENTINEL):
    """[n] view of a fresh allocation with four guard words behind it."""
    buf = torch.full((n + 4,), gap, dtype=torch.float32, device=DEV)
    return buf[:n], buf


def _guard_ok(buf, n, gap=SENTINEL):
    g = buf[n:].cpu()
    return bool(torch.isnan(g).all()) if np.isnan(gap) else bool((g == gap).all())


def _report(what):
    """Largest error / bound per quantity of the test that ends here."""
    print("error/bound %s: %s" % (what, ", ".join("%s %.3g" % (q, v) for q, v in sorted(WORST.items()))))


def _run_head_variant(ops, case, variant):
    kind_name, thr, x_act, with_zc = variant
    kind = KINDS[kind_name]
    what = "%s %s thr=%g x_act=%d" % (case.id, kind_name, thr, x_act)
    Y, w, b, t = head_data(case, x_act)
    B, K = case.B, case.K
    Yd, _ = _dev_operand(B, K, case.ldy, case.offy, torch.from_numpy(Y), NAN)
    wd = _dev_operand(1, K, K, case.offw, torch.from_numpy(w)[None], NAN)[0][0]
    bd = None if b is None else torch.full((1,), float(b), dtype=torch.float32, device=DEV)
    td = torch.from_numpy(t).to(DEV)
    Z, Zbuf = _guarded(B)
    dZ, dZbuf = _guarded(B)
    Zc, Zcbuf = _guarded(B) if with_zc else (None, None)
    dYd, dYbuf = _dev_operand(B, K, case.lddy, case.offdy, None, SENTINEL) if case.has_dY else (None, None)
    lb = torch.full((70,), SENTINEL, dtype=torch.float32, device=DEV)
    scratch = ops.head_scratch(DEV)
    aligned = (int(Yd.data_ptr() % 16 == 0) | int(wd.data_ptr() % 16 == 0) << 1
               | int(dYd is None or dYd.data_ptr() % 16 == 0) << 2)
    if case.has_dY:
        assert aligned == case.aligned(), (what, aligned)
    routes = {}
    for finish, want in case.routes():
        routes[finish] = ops.head_route(B, K, Yd.stride(0), 0 if dYd is None else dYd.stride(0), aligned, dYd is not None, finish)
        got = route_str(routes[finish])
        assert got == want, "%s finish=%r: the library takes %r, the case is meant for %r" % (what, finish, got, want)
    kw = dict(x_act=x_act, kind=kind, weights=WS, threshold=thr, Zc=Zc)
    outs = [t_ for t_ in (Zbuf, dZbuf, Zcbuf, dYbuf, lb) if t_ is not None]

    # finish=True, twice in a row on one scratch: the same bits, the arrival counter left at zero
    ops.head_fwd_bwd(Yd, wd, bd, td, Z, dZ, dYd, lb, scratch, finish=True, **kw)
    torch.cuda.synchronize()
    first = [o.clone() for o in outs]
    assert int(scratch[2048:].view(torch.int32)[0]) == 0, what + ": the arrival counter is not left at zero"
    ops.head_fwd_bwd(Yd, wd, bd, td, Z, dZ, dYd, lb, scratch, finish=True, **kw)
    torch.cuda.synchronize()
    assert all(torch.equal(a, o) for a, o in zip(first, outs)), what + ": two calls differ"
    assert int(scratch[2048:].view(torch.int32)[0]) == 0, what + ": the arrival counter is not left at zero"
    assert _guard_ok(Zbuf, B) and _guard_ok(dZbuf, B) and (Zcbuf is None or _guard_ok(Zcbuf, B)), what + ": written behind Z / dZ / Zc"
    assert bool((lb[3:] == SENTINEL).all()), what + ": loss_buf written behind its three words"
    if dYd is not None:
        assert _gap_ok(dYd, case.lddy, K, SENTINEL), what + ": dY's pitch gap was written"
        assert bool((dYbuf[:case.offdy] == SENTINEL).all()) and bool((dYbuf[case.offdy + B * case.lddy:] == SENTINEL).all())
    out = dict(Z=Z.cpu().numpy(), Zc=None if Zc is None else Zc.cpu().numpy(), dZ=dZ.cpu().numpy(),
               dY=None if dYd is None else dYd.cpu().numpy(), loss=lb[:3].cpu().numpy())
    check_head(out, Y, w, b, t, kind, thr, x_act, routes[True], what)
    if case.sat:
        p = out["Z"]
        want = {30.0: 1.0, 120.0: 1.0, -120.0: 0.0, 0.0: 0.5}
        for i, s in enumerate(SATURATED):
            rows = p[2 * i:2 * i + 2]
            if s in want:
                assert (rows == F32(want[s])).all(), "%s: p at logit %g is %r" % (what, s, rows.tolist())
            else:
                assert (np.abs(rows / 9.3576e-14 - 1) < 1e-3).all(), "%s: p at logit -30 is %r" % (what, rows.tolist())
            if abs(s) == 120.0:
                assert (out["dZ"][2 * i:2 * i + 2] == 0).all(), what + ": the gradient at a saturated prediction is not 0"

    # finish=False: loss_buf untouched until head_finish runs; twice with acc: exactly twice the first float64 sums
    lb2 = torch.full((70,), SENTINEL, dtype=torch.float32, device=DEV)
    ops.head_fwd_bwd(Yd, wd, bd, td, Z, dZ, dYd, lb2, scratch, finish=False, **kw)
    torch.cuda.synchronize()
    assert bool((lb2 == SENTINEL).all()), what + ": finish=False wrote loss_buf"
    assert all(torch.equal(a, o) for a, o in zip(first[:-1], outs[:-1])), what + ": the finish=False call's outputs differ"
    acc = torch.zeros(2, dtype=torch.float64, device=DEV)
    ops.head_finish(scratch, B, lb2, acc=acc)
    torch.cuda.synchronize()
    assert torch.equal(lb2.view(torch.int32), lb.view(torch.int32)), what + ": head_finish and the one-call form differ"
    assert acc.tolist() == [float(lb[1]), float(lb[2])]
    ops.head_finish(scratch, B, lb2, acc=acc)
    torch.cuda.synchronize()
    assert acc.tolist() == [2.0 * float(lb[1]), 2.0 * float(lb[2])] and torch.equal(lb2.view(torch.int32), lb.view(torch.int32))
    assert torch.equal(Yd.cpu(), torch.from_numpy(Y)) and torch.equal(wd.cpu(), torch.from_numpy(w)), what + ": an input was written"


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=lambda c: "%s-%s" % (c.id, c.route.replace(" ", "_")))
def test_head_vs_float64(ops, case):
    WORST.clear()
    try:
        for variant in case.variants:
            _run_head_variant(ops, case, variant)
    finally:
        _report(case.id)


# ---- GPU: cdlrm_bce_fwd_bwd on both sides of its switch -------------------------------------------------------------------------

SPECIAL_Z = (0.0, 1.0, 1e-9, 1.0 - 2.0 ** -24)
BCE_N = (1, 1023, 1024, 1025, 8191, 8192, 8193, 32768, 32769, 49152, 49153, 100000)


def bce_route(n):
    """k_bce_one: a workgroup of 1024 lanes in rounds of 8 x 1024; above 32768 elements k_bce_partial (64 x 256 lanes) + k_bce_final."""
    return "one" if n <= 32768 else "partial"


def bce_depth(n):
    if bce_route(n) == "one":
        return 8 * cdiv(n, 8192) + 6 + 16           # a lane's adds, the butterfly, the 16 waves
    return cdiv(n, 64 * 256) + 6 + 4 + 1 + 6        # a lane's adds, the butterfly, 4 waves; k_bce_final: one partial per lane, the butterfly


def specials_data(n, specials, seed):
    """z [n] in (0, 1) with every special value under both targets at the head and (n >= 64) at the tail; t [n]."""
    rng = np.random.default_rng(seed)
    z = rng.random(n).astype(F32)
    z[z == 0] = 0.5
    t = (rng.random(n) < 0.5).astype(F32)
    sz = np.array([s for s in specials for _ in (0, 1)], dtype=F32)
    st = np.array([k for _ in specials for k in (0, 1)], dtype=F32)
    m = len(sz)
    if n >= m:
        z[:m], t[:m] = sz, st
    if n >= 64:
        z[n - m:], t[n - m:] = sz, st
    return z, t


def test_bce_routes_and_specials():
    assert [bce_route(n) for n in BCE_N] == ["one"] * 8 + ["partial"] * 4
    assert F32(1.0 - 2.0 ** -24) < 1 and F32(1e-9) > 0
    for n in BCE_N[1:]:
        z, t = specials_data(n, SPECIAL_Z, n)
        for s in SPECIAL_Z:
            assert {0.0, 1.0} <= set(t[z == F32(s)].tolist()), (n, s)


@pytest.mark.gpu
@pytest.mark.parametrize("n", BCE_N, ids=lambda n: "n%d_%s" % (n, bce_route(n)))
def test_bce_vs_float64(ops, n):
    """Loss, gradient, the 65 words of the loss buffer and nothing behind them; the partial sums in loss_buf[1:65] -- each within
    its bound of the float64 sum of its 64 x 256 strided elements, or untouched -- prove the route."""
    WORST.clear()
    if n == 1:
        inputs = [(np.array([s], dtype=F32), np.array([k], dtype=F32)) for s in SPECIAL_Z + (0.3,) for k in (0, 1)]
    else:
        inputs = [specials_data(n, SPECIAL_Z, n)]
    try:
        for z, t in inputs:
            zd, td = torch.from_numpy(z).to(DEV), torch.from_numpy(t).to(DEV)
            for sb in (False, True):
                for with_dz in (True, False):
                    what = "bce n=%d sigmoid_bwd=%d dZ=%d" % (n, sb, with_dz)
                    lb = torch.full((70,), SENTINEL, dtype=torch.float32, device=DEV)
                    dZ, dZbuf = _guarded(n) if with_dz else (None, None)
                    ops.bce_fwd_bwd(zd, td, lb, dZ, sigmoid_bwd=sb)
                    torch.cuda.synchronize()
                    got = lb.cpu().numpy()
                    assert (got[65:] == SENTINEL).all(), what + ": written behind the 65 words"
                    assert dZbuf is None or _guard_ok(dZbuf, n), what + ": written behind dZ"
                    out = dict(dZ=None if dZ is None else dZ.cpu().numpy(), loss=got[:1])
                    check_loss_side(z, t, 0, 0.0, out, bce_depth(n), what, sigmoid_bwd=sb, count=False, q="bce ")
                    if bce_route(n) == "one":
                        assert (got[1:65] == SENTINEL).all(), what + ": partial sums written: not the one-workgroup route"
                    else:
                        l, _ = loss_terms(z, t, 0, n)
                        pad = np.zeros(cdiv(n, 16384) * 16384)
                        pad[:n] = l
                        ref = pad.reshape(-1, 64, 256).sum(axis=(0, 2))
                        mag = np.abs(pad).reshape(-1, 64, 256).sum(axis=(0, 2))
                        within(got[1:65], ref, (cdiv(n, 16384) + 6 + 4 + A_ULPS) * U * mag + TINY, what, "bce partial")
                    assert torch.equal(zd.cpu(), torch.from_numpy(z))
    finally:
        _report("bce n=%d" % n)


# ---- GPU: cdlrm_loss_fwd_bwd at the ends of the pass interval ---------------------------------------------------------------------

THR = 0.2
LOSS_SPECIALS = (float(F32(THR)), float(F32(1.0 - THR)), float(np.nextafter(F32(THR), F32(0))),
                 float(np.nextafter(F32(1.0 - THR), F32(1))), 0.0, 1.0, 0.5)
LOSS_N = (1, 1023, 1024, 1025, 5000)


def test_loss_specials_sit_on_and_just_outside_the_interval():
    for thr in (0.0, THR):
        z = np.array(LOSS_SPECIALS, dtype=F32)
        zc, passm = clamp_of(z, thr)
        assert passm.tolist() == ([True, True, False, False, False, False, True] if thr else [True] * 7)
        _, g = loss_terms(zc, np.ones(7), 0, 7)
        assert (g[:2] != 0).all()
    for n in LOSS_N[1:]:
        z, t = specials_data(n, LOSS_SPECIALS, n)
        for s in LOSS_SPECIALS:
            assert {0.0, 1.0} <= set(t[z == F32(s)].tolist()), (n, s)


@pytest.mark.gpu
@pytest.mark.parametrize("n", LOSS_N)
def test_loss_kernel_vs_float64(ops, n):
    """Every kind, thr 0 and 0.2, sigmoid_bwd both ways: Zc bit-exact, loss[1] exact, the gradient inside the bound at z == thr and
    z == 1 - thr and exactly 0 at their fp32 neighbours outside."""
    WORST.clear()
    if n == 1:
        inputs = [(np.array([s], dtype=F32), np.array([k], dtype=F32)) for s in LOSS_SPECIALS for k in (0, 1)]
    else:
        inputs = [specials_data(n, LOSS_SPECIALS, n)]
    depth = cdiv(n, 1024) + 6 + 16
    try:
        for z, t in inputs:
            zd, td = torch.from_numpy(z).to(DEV), torch.from_numpy(t).to(DEV)
            for kind_name, kind in sorted(KINDS.items()):
                for thr in (0.0, THR):
                    for sb in (False, True):
                        what = "loss n=%d %s thr=%g sigmoid_bwd=%d" % (n, kind_name, thr, sb)
                        lb = torch.full((70,), SENTINEL, dtype=torch.float32, device=DEV)
                        dZ, dZbuf = _guarded(n)
                        Zc, Zcbuf = _guarded(n)
                        ops.loss_fwd_bwd(zd, td, lb, dZ, kind=kind, weights=WS, threshold=thr, Zc=Zc, sigmoid_bwd=sb)
                        torch.cuda.synchronize()
                        assert bool((lb[3:] == SENTINEL).all()) and _guard_ok(dZbuf, n) and _guard_ok(Zcbuf, n), what
                        out = dict(Zc=Zc.cpu().numpy(), dZ=dZ.cpu().numpy(), loss=lb[:3].cpu().numpy())
                        check_loss_side(z, t, kind, thr, out, depth, what, sigmoid_bwd=sb, q="loss_fwd_bwd ")
                        if thr and n >= 14:
                            d = out["dZ"]
                            assert (d[4:8] == 0).all(), what + ": gradient just outside the interval"
                            assert (d[[1, 2]] != 0).all(), what + ": no gradient at z == thr (t = 1) / z == 1 - thr (t = 0)"
    finally:
        _report("loss_fwd_bwd n=%d" % n)


# ---- GPU: cdlrm_act_bwd ---------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("M,N,ldx,lddx", [(1, 1, 1, 1), (7, 129, 133, 140), (4100, 129, 129, 129)],
                         ids=["1x1", "7x129_pitched", "4100x129_past_the_grid"])
def test_act_bwd_vs_float64(ops, M, N, ldx, lddx):
    """dX *= act'(X) in place: act 0 and M = 0 leave dX bit-identical, ReLU is exact, the sigmoid within 3 roundings of float64;
    X's pitch gap holds NaN, dX's a sentinel; 4100 x 129 is past 2048 x 256 elements (the grid strides)."""
    from cdlrm_amd import _lib
    assert (M * N > 2048 * 256) == (M == 4100)
    WORST.clear()
    rng = np.random.default_rng(seed_of("act_bwd", M, N))
    d0 = rng.standard_normal((M, N), dtype=F32)
    for act in (0, 1, 2):
        X = head_like_activation(rng, M, N, act)
        Xd, _ = _dev_operand(M, N, ldx, 0, torch.from_numpy(X), NAN)
        dXd, dXbuf = _dev_operand(M, N, lddx, 0, torch.from_numpy(d0), SENTINEL)
        start = dXbuf.clone()
        _lib.check(_lib.lib().cdlrm_act_bwd(dXd.data_ptr(), lddx, Xd.data_ptr(), ldx, 0, N, act, None))      # M = 0
        torch.cuda.synchronize()
        assert torch.equal(start.view(torch.int32), dXbuf.view(torch.int32)), "act_bwd M=0 act=%d wrote dX" % act
        ops.act_bwd(dXd, Xd, act)
        torch.cuda.synchronize()
        assert _gap_ok(dXd, lddx, N, SENTINEL) and bool((dXbuf[M * lddx:] == SENTINEL).all()), "act_bwd act=%d: written outside dX" % act
        assert _gap_ok(Xd, ldx, N, NAN) and torch.equal(Xd.cpu(), torch.from_numpy(X))
        got = dXd.cpu().numpy()
        if act == 0:
            assert np.array_equal(bits(got), bits(d0))
        elif act == 1:
            assert np.array_equal(bits(got), bits(np.where(X > 0, d0, F32(0.0))))
        else:
            ref = d0.astype(F64) * ((1.0 - X.astype(F64)) * X.astype(F64))
            within(got, ref, 3 * U * np.abs(ref) + TINY, "act_bwd %dx%d" % (M, N), "act_bwd sigmoid")
            assert (got[(X == 0) | (X == 1)] == 0).all()
    _report("act_bwd %dx%d" % (M, N))


def head_like_activation(rng, M, N, act):
    """An activation output: normals with exact zeros and negatives (act 0 / 1), sigmoid outputs with exact 0 and 1 (act 2)."""
    v, u = rng.standard_normal((M, N), dtype=F32), rng.random((M, N))
    if act == 2:
        X = (1.0 / (1.0 + np.exp(-v.astype(F64)))).astype(F32)
        X[u < 0.05], X[u > 0.95] = 0.0, 1.0
        return X
    v[u < 0.3] = 0.0
    return v


# ---- GPU: cdlrm_scale_div -------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, 524288, 524289, 1000003])
def test_scale_div_is_a_true_division(ops, n):
    """x /= divisor bit for bit numpy's float32 division, for world sizes that are no power of two as well; 524288 = 2048 x 256 is
    the grid cap, past it a lane walks a second element; nothing behind x[n - 1] is written."""
    from cdlrm_amd import _lib
    rng = np.random.default_rng(seed_of("scale_div", n))
    x = (rng.standard_normal(n) * 10.0 ** rng.uniform(-30, 30, size=n)).astype(F32)
    x[np.abs(x) < 1e-35] = 1.0
    for div in (2.0, 3.0, 7.0, 8.0):
        xd, buf = _guarded(n)
        xd.copy_(torch.from_numpy(x))
        if n == 0:      # with the buffer's real address (an empty tensor has none): straight to the C entry point
            _lib.check(_lib.lib().cdlrm_scale_div(buf.data_ptr(), 0, div, None))
        else:
            ops.scale_div(xd, div)
        torch.cuda.synchronize()
        assert _guard_ok(buf, n), "scale_div n=%d: written behind x" % n
        want = x / F32(div)
        assert np.isfinite(want).all() and (n == 0 or np.abs(want).min() > 1.2e-38)
        same = bits(xd.cpu().numpy()) == bits(want)
        assert same.all(), "scale_div n=%d / %g: %d of %d elements differ from float32 division" % (n, div, int((~same).sum()), n)
