"""What a training step issues, written down call by call -- a helper for tests/test_step_path.py that also runs as a script
(`python tests/step_trace.py cpu|gpu OUT.json` makes the fixtures tests/golden/step_traces_*.json).

A `Tracer` wraps `engine.rec` (the step's stream / event calls) and every function of the `engine.ops` module, and logs one
entry per call made inside `TrainEngine.step()`: the name, the streams and events by label, every scalar argument and keyword
by value, every tensor as (shape, strides).  No addresses: an integer that can only be one (>= 2^32: the sorted lists'
addresses) is logged as "addr".  Streams are labelled by identity against the engine's side / prefetch / weight-gradient
streams, anything else is "main"; events by their name in `eng._events`, "ring" for the resolver's ring events.  Classes of
the ops module are left alone (constructing a plan or an event object issues nothing), and so are the two host-side queries a
step asks (QUERIES: do the fused kernels take this shape; where do batch j's sorted lists lie): they issue nothing, and what
they answer reaches the log through the calls that use it.

It reads nothing of the engine but `rec`, `ops`, `side`, `pref`, `wst`, `_events`, `_bufs`, `_tapes`, the schedule knobs and
`step()`, so it runs unchanged on any commit that has those.  Distinct entries and distinct traces are stored once; a run is
the list of its steps' trace numbers."""
import json
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

QUERIES = ("gather_interact_supported", "embbag_bwd_sorted_views")


class Pool:
    """Distinct entries and distinct traces of any number of runs (what a fixture file holds beside the runs)."""

    def __init__(self):
        self.entries, self.traces = [], []
        self._e, self._t = {}, {}

    def trace(self, entries) -> int:
        ids = []
        for e in entries:
            s = json.dumps(e, sort_keys=True)
            if s not in self._e:
                self._e[s] = len(self.entries)
                self.entries.append(json.loads(s))
            ids.append(self._e[s])
        ids = tuple(ids)
        if ids not in self._t:
            self._t[ids] = len(self.traces)
            self.traces.append(list(ids))
        return self._t[ids]


class Tracer:
    def __init__(self, engine_module, eng, pool=None):
        self.E, self.eng = engine_module, eng
        self.pool = pool if pool is not None else Pool()
        self.steps = []             # per step: its trace's number in the pool
        self._log = None

    # ---- labels ----
    def _stream(self, st):
        eng = self.eng
        for name in ("side", "pref", "wst"):
            x = getattr(eng, name)
            if st is x or (hasattr(st, "cuda_stream") and hasattr(x, "cuda_stream") and st.cuda_stream == x.cuda_stream):
                return "stream:" + name
        return "stream:main"

    def _event(self, ev):
        for name, x in self.eng._events.items():
            if isinstance(x, dict):
                for k, y in x.items():
                    if ev is y:
                        return "event:%s[%s]" % (name, k)
            elif ev is x:
                return "event:" + name
        for key, ring in self.eng._bufs.items():
            if isinstance(key, tuple) and key and key[0] in ("wres_ev", "wsorted_ev"):
                if any(ev is y for row in ring for y in (row if isinstance(row, list) else [row])):
                    return "event:ring"
        return "event"

    def _desc(self, a):
        if a is None or isinstance(a, (bool, float, str)):
            return a
        if isinstance(a, int):
            return a if abs(a) < (1 << 32) else "addr"
        if isinstance(a, torch.Tensor):
            return ["T", list(a.shape), list(a.stride())]
        if hasattr(a, "wait_stream"):
            return self._stream(a)
        if hasattr(a, "record") and hasattr(a, "synchronize"):
            return self._event(a)
        if isinstance(a, (list, tuple)):
            return [self._desc(x) for x in a]
        return "<%s>" % type(a).__name__

    # ---- wrapping ----
    def _wrap_op(self, name, fn):
        def call(*args, **kw):
            if self._log is not None:
                self._log.append([name, [self._desc(a) for a in args], {k: self._desc(v) for k, v in kw.items()}])
            return fn(*args, **kw)
        call.__name__ = name
        return call

    def _rec(self, fn, *args):
        if self._log is not None:
            self._log.append(["rec:" + fn.__name__, [self._desc(getattr(fn, "__self__", None))] + [self._desc(a) for a in args], {}])
        return self._rec0(fn, *args)

    def __enter__(self):
        E = self.E
        self._ops0, self._rec0 = E.ops, E.rec
        shim = types.SimpleNamespace()
        for k in dir(E.ops):
            if k.startswith("__"):
                continue
            v = getattr(E.ops, k)
            plain = isinstance(v, (types.FunctionType, types.BuiltinFunctionType)) and k not in QUERIES
            setattr(shim, k, self._wrap_op(k, v) if plain else v)
        E.ops, E.rec = shim, self._rec
        return self

    def __exit__(self, *exc):
        self.E.ops, self.E.rec = self._ops0, self._rec0

    def step(self, *args, **kw):
        self._log = []
        try:
            out = self.eng.step(*args, **kw)
        finally:
            log, self._log = self._log, None
        self.steps.append(self.pool.trace(log))
        return out


def tape_names(eng):
    """Per recorded tape, in the order they were recorded, the names of its entries."""
    return [[getattr(fn, "__name__", type(fn).__name__) for fn, _, _ in t["prog"]] for t in eng._tapes.values()]


# ---- the CPU runs: tests/fake_ops.py behind the engine ----------------------------------------------------------------
CPU_CASES = [dict(aux=aux, alone=alone, defer=defer, op=op) for aux in (1, 2) for alone in (None, 1) for defer in (False, True)
             for op in ("dot", "cat")] + [dict(aux=2, alone=None, defer=False, op="dot", bags=True)]


def cpu_case_name(c):
    return "aux%d_%s_%s_%s%s" % (c["aux"], "alone1" if c["alone"] else "aloneD", "defer" if c["defer"] else "plain", c["op"],
                                 "_bags" if c.get("bags") else "")


def _bag_shim(fake_ops):
    """fake_ops with the scratch bag of squared-off ragged inputs (square_bags: offsets [T, B + 1]): the stand-ins pool into /
    read gradients of a block of exactly as many rows as there are bags; the scratch bag's row lies behind the block."""
    shim = types.ModuleType("fake_ops_bags")
    shim.__dict__.update({k: getattr(fake_ops, k) for k in dir(fake_ops) if not k.startswith("__")})

    def embbag_fwd(ctx, slots, offsets, out, ld_bag, ld_table, n_bags=None, stream=None):
        if offsets is None or offsets.shape[1] == out.shape[0]:
            return fake_ops.embbag_fwd(ctx, slots, offsets, out, ld_bag, ld_table, n_bags, stream)
        tmp = torch.zeros(offsets.shape[1], out.shape[1], out.shape[2])
        fake_ops.embbag_fwd(ctx, slots, offsets, tmp, ld_bag, ld_table, n_bags, stream)
        out.copy_(tmp[:out.shape[0]])

    def embbag_bwd_apply(ctx, n, offsets, grad, ld_bag, ld_table, lr, work, touched=None, stream=None):
        if offsets is not None and offsets.shape[1] != grad.shape[0]:
            grad = torch.cat([grad, torch.zeros(offsets.shape[1] - grad.shape[0], grad.shape[1], grad.shape[2])])
        return fake_ops.embbag_bwd_apply(ctx, n, offsets, grad, ld_bag, ld_table, lr, work, touched, stream)

    shim.embbag_fwd, shim.embbag_bwd_apply = embbag_fwd, embbag_bwd_apply
    return shim


def cpu_run(case, pool, after_step=None, before_step=None, steps=6):
    """One case of CPU_CASES: 6 steps in windows of 3 (the last step of a window hands no next batch over) at B 64, D 16, four
    small tables.  before_step(eng, j, next_idx) / after_step(eng, j, next_idx): hooks of the caller.  Returns the Tracer."""
    import fake_ops
    import cdlrm_amd.engine as E
    import cdlrm_amd.model_no_ddp as Mo
    from oracle import cdlrm_oracle as O
    ln_emb, D, B, L, ways = np.array([300, 50, 7, 120]), 16, 64, 3, 4
    bags = bool(case.get("bags"))
    aux_rows = 256 if bags else B
    nf = len(ln_emb) + 1
    ln_bot = np.array([5, 24, D])
    ln_top = np.array([(D + nf * (nf - 1) // 2) if case["op"] == "dot" else nf * D, 24, 1])
    saved = (E.ops, Mo.ops, Mo.Embedding_Table_Group.__dict__.get("device_pointers"))
    E.ops = Mo.ops = _bag_shim(fake_ops)
    Mo.Embedding_Table_Group.device_pointers = lambda self: self._fake_ptrs
    try:
        np.random.seed(3)
        torch.manual_seed(3)
        host = O.init_host_tables([int(x) for x in ln_emb], D)
        eg = Mo.Embedding_Table_Group(D, ln_emb, init="empty_meta")
        for k in range(len(ln_emb)):
            eg.emb_l[k].weight.data = host[k]
        eg._fake_ptrs = fake_ops.register_host(host)
        eg._pinned = True
        cg = Mo.Embedding_Table_Cache_Group(D, ln_emb, 24, aux_rows, ways, aux_phases=case["aux"])
        dl = Mo.DLRM_Net(ln_bot, ln_top, case["op"], False, True, -1, ln_top.size - 2, 0.0)
        eng = E.TrainEngine(cg, dl, eg, lr=0.1, lr_embeds=0.2, defer_top_update=case["defer"])
        if case["alone"]:
            eng.gather_alone_min = case["alone"]
        eng.use_tape = False
        pipe = E.WindowPipeline(cg, eg, 4096, parity_rng=True)
        rng = np.random.RandomState(7)
        batches = []
        for j in range(steps):
            X = torch.from_numpy(rng.rand(B, 5).astype(np.float32))
            Tt = torch.from_numpy(np.round(rng.rand(B, 1)).astype(np.float32))
            if bags:
                lens = [[int(x) for x in rng.randint(1, 4, size=B)] for _ in ln_emb]
                lists = [torch.from_numpy(rng.randint(0, n, size=sum(l)).astype(np.int64)) for n, l in zip(ln_emb, lens)]
                offs = [torch.from_numpy(np.cumsum([0] + l[:-1]).astype(np.int64)) for l in lens]
                off, idx = E.square_bags(offs, lists)
                batches.append((X, idx, Tt, off, lists))
            else:
                idx = torch.from_numpy(np.stack([rng.randint(0, n, size=B) for n in ln_emb]).astype(np.int64))
                batches.append((X, idx, Tt, None, None))
        with Tracer(E, eng, pool) as tr:
            for j, (X, idx, Tt, off, _) in enumerate(batches):
                if j % L == 0:
                    torch.manual_seed(100 + j)
                    if bags:
                        win = E.pad_window([torch.cat([b[4][k] for b in batches[j:j + L]]) for k in range(len(ln_emb))])
                    else:
                        win = torch.cat([b[1] for b in batches[j:j + L]], dim=1)
                    pipe.plan_window(win)
                    pipe.commit()
                    pipe.wait_writeback()
                nxt = batches[j + 1][1] if (j + 1) % L != 0 and j + 1 < steps and not bags else None
                if before_step is not None:
                    before_step(eng, j, nxt)
                tr.step(X, idx, Tt, lS_o=off, j=j, next_idx=nxt)
                if after_step is not None:
                    after_step(eng, j, nxt)
        eng.finish()
        return tr
    finally:
        E.ops, Mo.ops = saved[0], saved[1]
        if saved[2] is None:
            del Mo.Embedding_Table_Group.device_pointers
        else:
            Mo.Embedding_Table_Group.device_pointers = saved[2]


# ---- the GPU runs: the golden runs of tests/test_engine_parity.py on a WindowResolver with chunks of 3 -----------------
GPU_VARIANTS = ("default", "gather_alone_min_1", "fuse_gather_off", "fuse_once_off", "attach_events_off", "loss_async",
                "place_resolve")


class _Run(dict):
    """A run description with the golden files' surface (g[name], g.files)."""
    files = property(lambda self: list(self.keys()))


def gpu_shapes(golden):
    """name -> run description.  The two golden runs are the smallest at which the chained take, the placed resolve (train_c1:
    windows of 32 batches) and the slice sorts occur; their tables (4 x D 8, 8 x D 16) are outside what the fused gather +
    interaction kernels take, so a third run at the smoke test's shape (17 tables, D 32) reaches those kernels."""
    fused = _Run(ln_emb=np.array([3000, 50, 7, 1200, 40000, 90, 2500, 13, 700, 15000, 333, 41, 8000, 5, 1900, 620, 27000]),
                 m_spa=32, ln_bot=np.array([13, 32, 32]), top=np.array([32, 1]), cache_size=40, ways=4, B=64, L=8, nbatch=16,
                 seed=11, lr=0.1, lr_emb=0.3, alpha=1.2)
    return {"train_small": golden("train_small"), "train_c1": golden("train_c1"), "fused_shape": fused}


def _apply_variant(eng, variant):
    if variant == "gather_alone_min_1":
        eng.gather_alone_min = 1
    elif variant == "fuse_gather_off":
        eng.fuse_gather = False
    elif variant == "fuse_once_off":
        eng.fuse_once = False
    elif variant == "attach_events_off":
        eng.attach_events = False
    elif variant == "place_resolve":
        eng.place_resolve_min = 1
    else:
        assert variant in ("default", "loss_async"), variant


def gpu_run(g, variant, taped, pool=None, after_step=None):
    """One golden run under one variant.  Returns (Tracer or None when taped, eng, losses [nbatch, 3] on the host)."""
    import test_engine_parity as P
    import cdlrm_amd.engine as E
    DEV = P.DEV
    host, cg, dl, eng, pipe = P.build(g, aux_phases=2)
    _apply_variant(eng, variant)
    eng.use_tape = bool(taped)
    L = int(g["L"])
    batches = P.make_batches(g)
    dev = [(X.to(DEV), idx.to(DEV), Tt.to(DEV)) for X, idx, Tt in batches]
    losses = []
    tr = None if taped else Tracer(E, eng, pool)
    if tr is not None:
        tr.__enter__()
    try:
        for j, (X, idx, Tt) in enumerate(dev):
            if j % L == 0:
                win = torch.cat([b[1] for b in batches[j:j + L]], dim=1).to(DEV)
                torch.manual_seed(5000 + j)
                pipe.plan_window(win)
                pipe.commit()
                pipe.wait_writeback()
                rs = E.WindowResolver(eng, win, int(g["B"]), chunk=3)
            jl = j % L
            nxt = dev[j + 1][1] if j + 1 < len(dev) and jl + 1 < L else None
            kw = dict(j=j, next_idx=nxt, res=rs.batch(jl), next_res=rs.batch(jl + 1) if nxt is not None else None,
                      loss_sync=variant != "loss_async")
            loss = tr.step(X, idx, Tt, **kw) if tr is not None else eng.step(X, idx, Tt, **kw)
            if after_step is not None:
                after_step(eng, j)
            rs.ensure(jl + rs.CH + 2)
            if variant == "loss_async":
                eng.finish()
            losses.append(loss[0:3].clone())
    finally:
        if tr is not None:
            tr.__exit__(None, None, None)
    eng.finish()
    torch.cuda.synchronize()
    cg.ctx.check()
    return tr, eng, torch.stack(losses).cpu()


def expand(pool, steps):
    """The steps' traces written out: per step the list of its entries (pool: a Pool or a loaded fixture)."""
    entries, traces = (pool["entries"], pool["traces"]) if isinstance(pool, dict) else (pool.entries, pool.traces)
    return [[entries[e] for e in traces[t]] for t in steps]


def has_entry(pool, trace_ids, name, *, stream=None, first=None):
    """Does any of the traces hold a call `name` (on `stream`: its stream= keyword; with first positional argument `first`)?"""
    for t in set(trace_ids):
        for e in pool.traces[t]:
            n, args, kw = pool.entries[e]
            if n == name and (stream is None or kw.get("stream") == stream) and (first is None or (args and args[0] == first)):
                return True
    return False


def make_cpu():
    pool = Pool()
    runs = {cpu_case_name(c): dict(steps=cpu_run(c, pool).steps) for c in CPU_CASES}
    return dict(entries=pool.entries, traces=pool.traces, runs=runs)


def make_gpu():
    def golden(name):
        return np.load(os.path.join(ROOT, "tests", "golden", name + ".npz"))
    pool, runs = Pool(), {}
    for sname, g in gpu_shapes(golden).items():
        for v in GPU_VARIANTS:
            tr, _, l0 = gpu_run(g, v, False, pool)
            _, eng, l1 = gpu_run(g, v, True)
            assert torch.equal(l0, l1), (sname, v)
            runs["%s/%s" % (sname, v)] = dict(steps=tr.steps, tapes=tape_names(eng))
    return dict(entries=pool.entries, traces=pool.traces, runs=runs)


def dump(fix, path):
    with open(path, "w") as f:
        f.write("{\n\"entries\": [\n" + ",\n".join(json.dumps(e, sort_keys=True) for e in fix["entries"]) + "\n],\n")
        f.write("\"traces\": [\n" + ",\n".join(json.dumps(t) for t in fix["traces"]) + "\n],\n")
        f.write("\"runs\": {\n" + ",\n".join("%s: %s" % (json.dumps(k), json.dumps(v, sort_keys=True))
                                             for k, v in sorted(fix["runs"].items())) + "\n}\n}\n")


if __name__ == "__main__":
    fix = make_cpu() if sys.argv[1] == "cpu" else make_gpu()
    dump(fix, sys.argv[2])
    ids = [t for r in fix["runs"].values() for t in r["steps"]]
    print("%d runs, %d steps, %d distinct traces, %d distinct entries" % (len(fix["runs"]), len(ids), len(fix["traces"]),
                                                                         len(fix["entries"])))
    if sys.argv[1] == "gpu":
        pool = Pool()
        pool.entries, pool.traces = fix["entries"], fix["traces"]
        for what in (("gather_interact_bwd_sgd", {}), ("embbag_take", dict(stream="stream:pref")),
                     ("embbag_take", dict(stream="stream:side")), ("event_attach_next", dict(first="event:fwd_mark")),
                     ("embbag_bwd_apply_sorted", {})):
            print(what, has_entry(pool, ids, what[0], **what[1]))
