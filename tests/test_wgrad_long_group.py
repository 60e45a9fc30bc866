"""The grouped long-batch weight-gradient launch (k_wgrad_long, csrc/gemm_glds.h; the rule: wgrad_long_group, csrc/dense.hip).

Above a batch of 2048 a cdlrm_mlp_wgrad* call used to launch one split-M GEMM per layer; a call whose layers are all on the
LDS-DMA kernel or the LDS-free kernel now launches them as ONE grid, and cdlrm_debug_set(7, 2) brings the per-layer launches
back.  Over layer sets x batches x operand variants:
  1. the two forms give the same bits: dW, db, the stepped W and b (cdlrm_mlp_wgrad_sgd) and, in one case, the Adagrad state
     (cdlrm_mlp_wgrad_opt_ex);
  2. each result is within test_gemm_routes' weight-gradient bound of the float64 result (its comparator, its K_eff);
  3. a call the rule takes issues two kernel launches -- the group and the reduction -- where the per-layer form issues one per
     layer and the reduction; a call it does not take issues the same launches in both forms (torch.profiler kernel names).
Which calls the rule takes is worked out here from the route query, as the rule states it: every layer gemm2 (tn = 1) or
direct on the aligned loader in mode 0, at least one of each, at most eight layers per family, LDS-DMA workgroups <= 4 per CU,
LDS-free workgroups <= 2 per CU.
"""
import functools
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import test_gemm_routes as R      # noqa: E402  (the module fixture that builds the library; the comparator)
import test_wgrad_plan as P       # noqa: E402  (the declared layer sets)

ops = R.ops
DEV = R.DEV
LR = 0.05
PER_LAYER = 2           # cdlrm_debug_set(7, PER_LAYER)

SETS = {
    "c3_bot": P.C3_BOT,
    "mini": ((64, 13), (128, 64), (64, 128)),
    "head_first": ((1, 64), (128, 64)),
    "group9": P.SETS["group9"],         # nine layers, two of them register-staged / LDS-staged: per-layer launches
}
# just above the short path (multiple of 32, ragged last slab); 4096; 8192 (the only one at which c3's 128x64 body is reached);
# 2049 (no multiple of 32: no LDS-DMA route, nothing to group)
BATCHES = (2080, 4096, 8192, 2049)
VARIANTS = ("aligned", "xpitch", "dbnull")
CASES = [(s, m, v) for s in SETS for m in BATCHES for v in VARIANTS]
IDS = ["%s-%d-%s" % c for c in CASES]


class _debug7:
    def __init__(self, value):
        self.value = value

    def __enter__(self):
        from cdlrm_amd import _lib
        torch.cuda.synchronize()
        assert _lib.raw().cdlrm_debug_set(7, self.value) == 0

    def __exit__(self, *exc):
        from cdlrm_amd import _lib
        torch.cuda.synchronize()
        assert _lib.raw().cdlrm_debug_set(7, 0) == 0


@functools.lru_cache(maxsize=None)
def _host(set_name, M):
    """The inputs of one (layer set, batch) and their float64 results, computed once and shared by every test and variant."""
    rng = np.random.RandomState(1000 * len(set_name) + M)
    out = []
    for N, K in SETS[set_name]:
        X = rng.randn(M, K).astype(np.float32)
        dZ = rng.randn(M, N).astype(np.float32)
        W = (rng.randn(N, K) / np.sqrt(K)).astype(np.float32)
        b = rng.randn(N).astype(np.float32)
        X64, dZ64 = X.astype(np.float64), dZ.astype(np.float64)
        out.append(dict(X=X, dZ=dZ, W=W, b=b, dW64=dZ64.T @ X64, dWmag=np.abs(dZ64).T @ np.abs(X64), db64=dZ64.sum(0),
                        dbmag=np.abs(dZ64).sum(0)))
    return out


class Call:
    """The device operands of one case (fresh outputs and parameters) and its ops.WgradPlan."""

    def __init__(self, ops, set_name, M, variant, adagrad=False):
        layers = SETS[set_name]
        n = len(layers)
        host = _host(set_name, M)
        self.Xs, self.dZs, self.dWs, self.dbs, self.Ws, self.bs = [], [], [], [], [], []
        for i, ((N, K), h) in enumerate(zip(layers, host)):
            if variant == "xpitch" and i == min(1, n - 1):       # a row pitch of K + 1 elements: not 16-byte loadable
                buf = torch.full((M, K + 1), float("nan"), device=DEV)
                buf[:, :K] = torch.from_numpy(h["X"])
                self.Xs.append(buf[:, :K])
            else:
                self.Xs.append(torch.from_numpy(h["X"]).to(DEV))
            self.dZs.append(torch.from_numpy(h["dZ"]).to(DEV))
            self.dWs.append(torch.full((N, K), R.SENTINEL, device=DEV))
            nodb = variant == "dbnull" and i == min(2, n - 1)
            self.dbs.append(None if nodb else torch.full((N,), R.SENTINEL, device=DEV))
            self.Ws.append(torch.from_numpy(h["W"]).to(DEV))
            self.bs.append(None if nodb else torch.from_numpy(h["b"]).to(DEV))
        Ns, Ks = [l[0] for l in layers], [l[1] for l in layers]
        self.work = ops.mlp_wgrad_work(M, Ns, Ks, DEV)
        self.plan = ops.WgradPlan(self.Xs, self.dZs, self.dWs, self.dbs, self.work)
        self.plan.set_params(self.Ws, self.bs)
        self.SWs = self.Sbs = None
        if adagrad:
            self.SWs = [torch.zeros_like(w) for w in self.Ws]
            self.Sbs = [None if b is None else torch.zeros_like(b) for b in self.bs]
            self.plan.set_state(self.SWs, self.Sbs)

    def results(self):
        torch.cuda.synchronize()
        out = {}
        for name, ts in (("dW", self.dWs), ("db", self.dbs), ("W", self.Ws), ("b", self.bs), ("SW", self.SWs), ("Sb", self.Sbs)):
            for i, t in enumerate(ts or ()):
                if t is not None:
                    out["%s[%d]" % (name, i)] = t.clone()
        return out


def n_cu():
    return torch.cuda.get_device_properties(0).multi_processor_count


def rule_takes(routes, cus):
    """wgrad_long_group's rule, from the per-layer routes of the call."""
    direct = [r for r in routes if r["family"] == "direct" and r["aligned"] and r["mode"] == 0]
    dma = [r for r in routes if r["family"] == "gemm2" and r["tn"] == 1]
    if len(direct) + len(dma) != len(routes) or not direct or not dma or len(direct) > 8 or len(dma) > 8:
        return False
    return sum(r["wgs"] for r in dma) <= 4 * cus and sum(r["wgs"] for r in direct) <= 2 * cus


def call_routes(ops, call, set_name):
    routes = ops.mlp_wgrad_route(call.plan, n_cu=n_cu())
    for r, (N, K) in zip(routes, SETS[set_name]):       # workgroups: (64 tm) x 64 tiles, or the LDS-free kernel's 32 x 32, per slab
        bm, bn = (64 * r["tm"], 64) if r["tm"] else (32, 32)
        r["wgs"] = -(-N // bm) * -(-K // bn) * r["splits"]
    return routes


def run_both(ops, set_name, M, variant, entry):
    """The call with the switch at 0 and at PER_LAYER on the same inputs: (results, results, routes)."""
    got = []
    for value in (0, PER_LAYER):
        c = Call(ops, set_name, M, variant, adagrad=entry == "adagrad")
        with _debug7(value):
            if entry == "plain":
                ops.mlp_wgrad(c.plan)
            elif entry == "sgd":
                ops.mlp_wgrad(c.plan, lr=LR)
            else:
                ops.mlp_wgrad(c.plan, lr=LR, opt=("adagrad", 1e-8))
            got.append(c.results())
    return got[0], got[1], call_routes(ops, c, set_name)


def assert_identical(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        assert torch.equal(a[k], b[k]), "%s: %s differs between the grouped and the per-layer launches" % (what, k)


def assert_fp64(res, set_name, M, routes, what, stepped):
    """dW / db (and, stepped, W - LR dW / b - LR db) against float64 with test_gemm_routes' bound: K_eff of a split-M weight
    gradient as its _run_bwd has it; the step adds one product and one difference, two more roundings of the same magnitude."""
    for i, (h, r) in enumerate(zip(_host(set_name, M), routes)):
        splits = r["splits"]
        k_eff = (M if splits == 1 else -(-M // splits) + 32 + splits) + 3
        route = R.route_str(r)
        for g, p, ref, mag, p0 in (("dW", "W", h["dW64"], h["dWmag"], h["W"]), ("db", "b", h["db64"], h["dbmag"], h["b"])):
            key = "%s[%d]" % (g, i)
            if key not in res:
                continue
            R.assert_within(res[key].cpu().numpy(), ref, mag, k_eff, "%s %s" % (what, key), route)
            if stepped:
                R.assert_within(res["%s[%d]" % (p, i)].cpu().numpy(), p0.astype(np.float64) - LR * ref, LR * mag, k_eff + 2,
                                "%s %s[%d]" % (what, p, i), route)


@pytest.mark.gpu
@pytest.mark.parametrize("set_name,M,variant", CASES, ids=IDS)
def test_grouped_equals_per_layer_and_fp64(ops, set_name, M, variant):
    for entry in ("plain", "sgd"):
        grouped, per_layer, routes = run_both(ops, set_name, M, variant, entry)
        what = "%s M=%d %s %s" % (set_name, M, variant, entry)
        if entry == "plain":        # the parameters are not touched
            host = _host(set_name, M)
            assert all(torch.equal(grouped["W[%d]" % i].cpu(), torch.from_numpy(h["W"])) for i, h in enumerate(host)), what
        assert_identical(grouped, per_layer, what)
        assert_fp64(grouped, set_name, M, routes, what, stepped=entry == "sgd")


@pytest.mark.gpu
def test_adagrad_grouped_equals_per_layer(ops):
    """cdlrm_mlp_wgrad_opt_ex, c3's bottom call at 8192: the accumulators and the stepped parameters too are the same bits; dW and
    db against float64 (the Adagrad step itself is test_dense_adagrad's subject)."""
    grouped, per_layer, routes = run_both(ops, "c3_bot", 8192, "aligned", "adagrad")
    assert rule_takes(routes, n_cu())
    assert any(k.startswith("SW[") for k in grouped) and any(k.startswith("Sb[") for k in grouped)
    assert_identical(grouped, per_layer, "c3_bot adagrad")
    assert_fp64(grouped, "c3_bot", 8192, routes, "c3_bot adagrad", stepped=False)


def kernel_launches(fn):
    """Names of the kernels fn() launches."""
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    names = [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA and "k_" in e.name]
    return names


@pytest.mark.gpu
@pytest.mark.parametrize("set_name,M,variant", CASES, ids=IDS)
def test_launch_count(ops, set_name, M, variant):
    names = {}
    for value in (0, PER_LAYER):
        c = Call(ops, set_name, M, variant)
        with _debug7(value):
            names[value] = kernel_launches(lambda: ops.mlp_wgrad(c.plan, lr=LR))
    routes = call_routes(ops, c, set_name)
    n_red = -(-sum(r["splits"] > 1 for r in routes) // 8)       # one grouped reduction per eight slabbed layers
    n_step = sum((1 + (b is not None)) * (r["splits"] == 1) for r, b in zip(routes, c.bs))      # un-slabbed layers step elementwise
    assert len(names[PER_LAYER]) == len(routes) + n_red + n_step, names[PER_LAYER]
    assert not any("k_wgrad_long" in n for n in names[PER_LAYER])
    if rule_takes(routes, n_cu()):
        assert len(names[0]) == 1 + n_red + n_step and "k_wgrad_long" in names[0][0], names[0]
    else:
        assert [n.split("(")[0] for n in names[0]] == [n.split("(")[0] for n in names[PER_LAYER]]


@pytest.mark.gpu
def test_the_flagship_call_is_grouped_and_its_neighbours_are_not(ops):
    """c3's bottom call at 8192 is the call the launch was built for: three GEMM launches + a reduction become two launches.  The
    same set at 2049 has no LDS-DMA layer, group9 has nine layers on four kernel families: both keep their per-layer launches."""
    for set_name, M, want in (("c3_bot", 8192, True), ("c3_bot", 2049, False), ("group9", 8192, False)):
        c = Call(ops, set_name, M, "aligned")
        assert rule_takes(call_routes(ops, c, set_name), n_cu()) == want, (set_name, M)
    c = Call(ops, "c3_bot", 8192, "aligned")
    names = kernel_launches(lambda: ops.mlp_wgrad(c.plan, lr=LR))
    assert len(names) == 2 and "k_wgrad_long" in names[0] and "k_reduce_group" in names[1], names
    with _debug7(PER_LAYER):
        names = kernel_launches(lambda: ops.mlp_wgrad(c.plan, lr=LR))
    assert len(names) == 4 and "k_reduce_group" in names[3], names
