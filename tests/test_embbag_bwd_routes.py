"""Every route of the embedding backward + sparse SGD (K8, csrc/embbag_bwd.hip) against a plain float64 reference.

The sort (bwd_sort_plan / bwd_sort_launch: k_sort_chunks at 1024 / 2048 / 8192 keys per workgroup, k_merge_pass, k_seg_meta) and
the apply (bwd_apply_plan / bwd_apply_launch: k_bwd_chunks, the full and the lean k_bwd_blocks, k_bwd_long) have many branches, and
K8 writes the cache rows that persist from step to step: a lookup summed twice or dropped at a chunk edge is never overwritten.  One table of
cases below, each a deterministic RUN-LENGTH SCRIPT (how many lookups each slot gets, in sorted order; positions scattered by a
fixed permutation) with the route it is meant to reach, serves three checks:

  * CPU: ops.embbag_bwd_route (the plans and layouts the launching calls read, nothing launched) gives the declared route, the
    table reaches every kernel instantiation the dispatch can launch, and the offsets it reports lie inside the buffer in the
    layout's order;
  * CPU: one TrainEngine step per configuration (c1 ... c5 embedding widths, per-rank batches 1024 ... 65536, tests/fake_ops.py)
    records the step's embbag_bwd_prepare / embbag_bwd_apply arguments; every sort and apply route they resolve to, with its
    layout and grad pitches, is in the table;
  * GPU: each case checks the sort's keys, run distances and once-only flags exactly, every updated row against
    |W - W_ref| <= C (u |W_ref| + lr gamma_k sum |g|), k = min(L, 32) - 1 + ceil(L / 32) - 1 (in-chunk sums in position order,
    chunk partials in chunk order, one fma), every other row bit for bit, and the touched flags exactly.  Gaps of the gradient
    pitches and the gradient rows of empty bags hold NaN.

The comparators are checked on the CPU with negative controls: each bug a kernel could have, made in numpy, is rejected.
"""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
U = 2.0 ** -24
C_BOUND = 2.0           # safety factor over the rigorous bound of the kernel's summation
SEG = 32                # SEG_CH: lookups one chunk head sums
TILE = 256              # positions per k_seg_meta tile
LR = 0.25
WAYS = 2

# ---- run-length scripts ----------------------------------------------------------------------------------------------------

FILL = (1, 2, 1, 3, 1, 1, 5, 2, 9, 1, 4)        # what fills the gaps between anchored runs (cut to fit)
EDGE_RUNS = (1, 2, 31, 32, 33, 63, 64, 65)
LOOP_RUNS = (4 * SEG, 15 * SEG, 16 * SEG, 16 * SEG + 1, 17 * SEG + 5)   # k_bwd_long: 4-wide only, 4-wide x 3 + 3 tail, 16-wide x 1,
                                                                         # 16-wide + 1 tail, 16-wide + 1 tail of a 5-lookup chunk


def seq(start, lengths):
    """Anchors of consecutive runs from sorted position `start` on."""
    out = []
    for L in lengths:
        out.append((start, L))
        start += L
    return out


def SHARED_BUCKET(s):
    """A 40-lookup run from s (s % 32 == 0: its second chunk's head at s + 32) and a 70-lookup run from s + 40, whose head falls
    in the same 32-position bucket of chunk partials (2 * (p / 32) + head)."""
    assert s % SEG == 0
    return [(s, 40), (s + 40, 70)]


def script(n, anchors=()):
    """Run lengths in sorted order covering n positions: each (start, length) anchor placed at its start, the gaps filled by FILL."""
    runs, p, fi = [], 0, 0
    for st, L in sorted(anchors) + [(n, 0)]:
        assert st >= p, "overlapping anchors at %d" % st
        while p < st:
            l = min(FILL[fi % len(FILL)], st - p)
            runs.append(l)
            p += l
            fi += 1
        if L:
            runs.append(L)
            p += L
    assert p == n and all(r >= 1 for r in runs)
    return runs


TILE_EDGES = [(TILE - 1, 2), (2 * TILE, 300), (4 * TILE - 14, 15), (4 * TILE + 1, 3)]
# (255: a run starting one before a k_seg_meta tile; 512: one starting exactly at a tile and covering the whole next tile, whose
#  positions all find their run start by the tile's left search; 1010 .. 1024: a run straddling sort chunk / tile 1024, and 1025:
#  one starting one after it)


def _bags_of(n, rot=0):
    """Bag offsets (the first lookup of every bag) of a multi-hot layout over n lookups: empty bags, single-lookup bags, one
    huge bag and an empty last bag.  rot: the bag lengths (all but the empty last bag) rotated by that many bags -- the layout
    of another table, with as many bags but other offsets (its empty bags and its huge bag elsewhere)."""
    off, p = [], 0
    pattern = [0, 1, 3, 0, 0, 1, 2, 7, 1]
    i = 0
    huge = max(1, (2 * n) // 5)
    while p < n:
        if i == 5:
            L = huge
        else:
            L = pattern[i % len(pattern)]
        L = min(L, n - p)
        off.append(p)
        p += L
        i += 1
    off.append(n)           # the empty last bag
    lens = np.diff(off)
    if rot:
        lens = np.roll(lens, rot)
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)


def _table_bags(n, t):
    return _bags_of(n, 7 * t)


class Case:
    def __init__(self, id, n, D, entry, route, anchors=(), T=1, layout="arange", debug6=0, debug1=0, pitch="tight", whole=False,
                 nb=1, j0=0, count=1, batch_len=None, aux_phase=0, ld_off_pad=0):
        self.id, self.n, self.D, self.entry, self.route = id, n, D, entry, route
        self.T, self.layout, self.debug6, self.debug1, self.pitch = T, layout, debug6, debug1, pitch
        self.runs = [n] if whole else script(n, anchors)
        self.nb, self.j0, self.count = nb, j0, count
        self.batch_len = n if batch_len is None else batch_len
        self.aux_phase, self.ld_off_pad = aux_phase, ld_off_pad
        self.window = entry in ("sorted", "sorted_rest")
        self.rest = entry in ("rest", "sorted_rest")
        assert not (self.window and layout != "arange")
        assert self.window or aux_phase == 0

    @property
    def query_entry(self):
        return "apply" if self.entry == "sgd" else self.entry

    def route_args(self):
        return dict(T=self.T, D=self.D, n=self.n, offsets=self.layout == "bags", entry=self.query_entry, nb=self.nb, j0=self.j0,
                    count=self.count)


def route_str(r):
    """ops.embbag_bwd_route's dict -> '8192x8 c3 m2 seg A / chunks ar l64'."""
    return "%dx%d c%d m%d %s %s / %s %s l%d" % (r["sort_chunk"], r["sort_e"], r["sort_chunks"], r["merge_passes"],
                                                 "seg" if r["seg_meta"] else "sort", "B" if r["keys_in_b"] else "A", r["apply"],
                                                 "ar" if r["arange"] else "bag", r["lpr"])


def sort_part(route):
    return route.split(" / ")[0]


def apply_part(route):
    return route.split(" / ")[1]


# engine.py TrainEngine.step, the window-sorted path (WindowResolver.ensure_sorted / sorted_views):
#   ops.embbag_bwd_prepare_window(self.ctx, ws[:, self.col0:], self.B, nbc, self.width, ..., j0=j0, count=cnt)   (engine.py:643)
#     batch_len = self.B (the global batch), n = self.width (this rank's slice of it; the whole batch at world 1)
#     j0 / count: slices of SL = max(1, min(max(2, 2 * 8192 // width), CH)) batches of the chunk's nbc          (engine.py:524-525)
#   ops.embbag_bwd_apply_sorted(ctx, n, dfeat[:, 1:, :], dfeat.stride(0), D, lr, emb_work, sv[0], sv[1], sv[3],
#                               self._phase, once, ...)                                                          (engine.py:1521-1522)
#     n = width (the step's batch on this rank, B there), tstride = sv[3] = nbc * width, aux_phase = self._phase in {0, 1},
#     rest = once = fuse_once
# The CPU test double cannot take this path (WindowPipeline.sort_chunks needs HIP), so its arguments are cases of the table
# (the "win_engine_*" cases).
CASES = [
    # --- k_bwd_chunks, one lookup per bag (the Criteo layout): LPR 4 / 8 / 16 / 32 / 64, every sort shape
    Case("n1_d4_sgd", 1, 4, "sgd", "1024x1 c1 m0 sort A / chunks ar l4"),
    Case("n31_d8_whole", 31, 8, "apply", "1024x1 c1 m0 sort A / chunks ar l4", whole=True),
    Case("n1024_d16_edges", 1024, 16, "apply", "1024x1 c1 m0 sort A / chunks ar l4", pitch="engine",
         anchors=seq(0, EDGE_RUNS) + SHARED_BUCKET(512) + [(700, 32 * 4)]),
    Case("n1025_d32_edges", 1025, 32, "apply", "2048x2 c1 m0 sort A / chunks ar l8", pitch="engine",
         anchors=seq(640, EDGE_RUNS)),
    Case("n2048_d64_loops", 2048, 64, "sgd", "2048x2 c1 m0 sort A / chunks ar l16", pitch="gap",
         anchors=seq(3, LOOP_RUNS[:4])),
    Case("n2049_d128_t2_tiles", 2049, 128, "apply", "2048x2 c2 m1 seg B / chunks ar l32", T=2, pitch="engine",
         anchors=TILE_EDGES + SHARED_BUCKET(1536) + [(2040, 9)]),
    Case("n4097_d48_loops", 4097, 48, "apply", "2048x2 c3 m2 seg A / chunks ar l16",
         anchors=seq(0, LOOP_RUNS) + [(4095, 2)]),
    Case("n4097_d8_whole", 4097, 8, "sgd", "2048x2 c3 m2 seg A / chunks ar l4", whole=True),
    Case("n16384_d256", 16384, 256, "apply", "2048x2 c8 m3 seg B / chunks ar l64", pitch="engine",
         anchors=seq(0, LOOP_RUNS) + [(12 * TILE + 1, 3), (8180, 30)] + SHARED_BUCKET(12288) + [(16383, 1)]),
    Case("n16385_d384_cc2", 16385, 384, "apply", "8192x8 c3 m2 seg A / chunks ar l64", pitch="gap",
         anchors=seq(32, EDGE_RUNS) + [(8190, 549), (16384, 1)]),
    Case("n1025_d1024_cc4", 1025, 1024, "apply", "2048x2 c1 m0 sort A / chunks ar l64",
         anchors=seq(0, EDGE_RUNS) + seq(512, LOOP_RUNS[:1])),
    Case("n65536_d16", 65536, 16, "sgd", "8192x8 c8 m3 seg B / chunks ar l4", pitch="engine",
         anchors=seq(0, LOOP_RUNS) + [(8180, 30), (16380, 10), (32768 - 1, 2)] + SHARED_BUCKET(40000) + [(10 * TILE - 1, 2)]
         + [(65536 - 65, 65)]),
    # --- k_bwd_chunks over bags: empty bags, one-lookup bags, one huge bag, an empty last bag, ld_off > n_bags; the T = 2 cases
    #     give every table its own offsets (a table's offsets read at a stride other than ld_off are another table's bags)
    Case("bags_n1024_d4", 1024, 4, "apply", "1024x1 c1 m0 sort A / chunks bag l4", layout="bags", ld_off_pad=3,
         anchors=seq(0, EDGE_RUNS)),
    Case("bags_n2049_d32", 2049, 32, "sgd", "2048x2 c2 m1 seg B / chunks bag l8", layout="bags", anchors=TILE_EDGES),
    Case("bags_n1025_d64", 1025, 64, "apply", "2048x2 c1 m0 sort A / chunks bag l16", layout="bags", ld_off_pad=5, T=2,
         anchors=seq(500, LOOP_RUNS[:1]) + SHARED_BUCKET(800)),
    Case("bags_n4097_d128", 4097, 128, "apply", "2048x2 c3 m2 seg A / chunks bag l32", layout="bags", pitch="gap", ld_off_pad=1,
         T=2,
         anchors=seq(1000, LOOP_RUNS[2:])),
    Case("bags_n31_d256", 31, 256, "apply", "1024x1 c1 m0 sort A / chunks bag l64", layout="bags", anchors=[(3, 20)]),
    # --- the full k_bwd_blocks: cdlrm_debug_set(6, 64), apply_rest over bags, and the 4x4 / 16 form of the rest (6, 128)
    Case("blk_n1024_d16", 1024, 16, "apply", "1024x1 c1 m0 sort A / blocks ar l4", debug6=64, anchors=seq(0, EDGE_RUNS)),
    Case("blk_n2049_d32", 2049, 32, "apply", "2048x2 c2 m1 seg B / blocks ar l8", debug6=64,
         anchors=TILE_EDGES + SHARED_BUCKET(1536)),
    Case("blk_n4097_d64", 4097, 64, "rest", "2048x2 c3 m2 seg A / blocks ar l16", debug6=128, anchors=seq(7, LOOP_RUNS)),
    Case("blk_n1025_d128", 1025, 128, "apply", "2048x2 c1 m0 sort A / blocks ar l32", debug6=64, debug1=1,
         anchors=seq(0, EDGE_RUNS) + SHARED_BUCKET(640)),
    Case("blk_n16385_d256", 16385, 256, "apply", "8192x8 c3 m2 seg A / blocks ar l64", debug6=64, debug1=-1,
         anchors=seq(8100, LOOP_RUNS[3:]) + [(16380, 5)]),
    Case("blkbag_n1024_d8", 1024, 8, "rest", "1024x1 c1 m0 sort A / blocks bag l4", layout="bags", ld_off_pad=2, T=2,
         anchors=seq(0, EDGE_RUNS)),
    Case("blkbag_n2049_d32", 2049, 32, "apply", "2048x2 c2 m1 seg B / blocks bag l8", layout="bags", debug6=64, T=2,
         ld_off_pad=3, anchors=TILE_EDGES),
    Case("blkbag_n1025_d48", 1025, 48, "rest", "2048x2 c1 m0 sort A / blocks bag l16", layout="bags", pitch="gap",
         anchors=seq(200, LOOP_RUNS[1:2]) + SHARED_BUCKET(768)),
    Case("blkbag_n4097_d128", 4097, 128, "rest", "2048x2 c3 m2 seg A / blocks bag l32", layout="bags", debug1=1,
         anchors=seq(0, LOOP_RUNS[3:])),
    Case("blkbag_n31_d384", 31, 384, "apply", "1024x1 c1 m0 sort A / blocks bag l64", layout="bags", debug6=64, whole=True),
    # --- the lean k_bwd_blocks: apply_rest without offsets (runs of one lookup only flag their rows)
    Case("lean_n1024_d4", 1024, 4, "rest", "1024x1 c1 m0 sort A / blocks_lean ar l4", anchors=seq(0, EDGE_RUNS)),
    Case("lean_n2049_d32", 2049, 32, "rest", "2048x2 c2 m1 seg B / blocks_lean ar l8", pitch="engine",
         anchors=TILE_EDGES + SHARED_BUCKET(1536)),
    Case("lean_n4097_d64", 4097, 64, "rest", "2048x2 c3 m2 seg A / blocks_lean ar l16", debug1=-1, anchors=seq(0, LOOP_RUNS)),
    Case("lean_n16384_d128_t2", 16384, 128, "rest", "2048x2 c8 m3 seg B / blocks_lean ar l32", T=2, pitch="engine",
         anchors=seq(8000, LOOP_RUNS[2:]) + [(16000, 384)]),
    Case("lean_n1025_d256", 1025, 256, "rest", "2048x2 c1 m0 sort A / blocks_lean ar l64", anchors=seq(1, EDGE_RUNS)),
    # --- the window-sorted path: prepare_window (nb / j0 / count, batch_len > n) + apply_sorted (tstride = nb * n, aux_phase)
    Case("win_engine_c3_rest", 8192, 128, "sorted_rest", "2048x2 c4 m2 seg A / blocks_lean ar l32", pitch="engine",
         nb=4, j0=2, count=2, aux_phase=1, anchors=seq(0, EDGE_RUNS) + seq(4000, LOOP_RUNS[:2])),
    Case("win_engine_c1_p0", 1024, 16, "sorted", "1024x1 c1 m0 sort A / chunks ar l4", pitch="engine",
         nb=3, j0=0, count=2, aux_phase=0, anchors=seq(0, EDGE_RUNS)),
    Case("win_engine_c2_p1", 2048, 32, "sorted", "2048x2 c1 m0 sort A / chunks ar l8", pitch="engine",
         nb=2, j0=0, count=2, aux_phase=1, anchors=seq(100, LOOP_RUNS[:3])),
    Case("win_engine_c4_rest", 8192, 256, "sorted_rest", "2048x2 c4 m2 seg A / blocks_lean ar l64", pitch="engine",
         nb=2, j0=0, count=2, aux_phase=0, anchors=seq(5000, LOOP_RUNS[3:])),
    Case("win_engine_c5_rest", 65536, 128, "sorted_rest", "8192x8 c8 m3 seg B / blocks_lean ar l32", pitch="engine",
         nb=1, j0=0, count=1, aux_phase=1, anchors=seq(8150, LOOP_RUNS)),
    Case("win_engine_c5_once0", 65536, 128, "sorted", "8192x8 c8 m3 seg B / chunks ar l32", pitch="engine",
         nb=1, j0=0, count=1, aux_phase=0, anchors=seq(16350, LOOP_RUNS[:2])),
    Case("win_split_n2049", 2049, 64, "sorted", "2048x2 c2 m1 seg B / chunks ar l16", nb=3, j0=1, count=1, batch_len=2100,
         aux_phase=1, pitch="gap", anchors=TILE_EDGES),
    Case("win_rest128_n1025", 1025, 256, "sorted_rest", "2048x2 c1 m0 sort A / blocks ar l64", debug6=128, nb=2, j0=1, count=1,
         batch_len=1100, aux_phase=1, anchors=seq(0, EDGE_RUNS)),
    Case("win_n4097_d8_t2", 4097, 8, "sorted", "2048x2 c3 m2 seg A / chunks ar l4", T=2, nb=2, j0=0, count=2, aux_phase=1,
         anchors=seq(0, LOOP_RUNS)),
]


# ---- fixtures and switches -------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def ops():
    from cdlrm_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        sys.path.insert(0, ROOT)
        import __graft_entry__ as g
        g.build()
    _lib.lib()
    from cdlrm_amd import ops as _ops
    return _ops


class debug:
    """cdlrm_debug_set(6, bits) and (1, cap) for the block; both back to 0 (their defaults) in a finally."""

    def __init__(self, d6=0, d1=0):
        self.d6, self.d1 = d6, d1

    def __enter__(self):
        from cdlrm_amd import _lib
        try:
            assert _lib.raw().cdlrm_debug_set(6, self.d6) == 0
            assert _lib.raw().cdlrm_debug_set(1, self.d1) == 0
        except BaseException:
            self.__exit__(None, None, None)
            raise

    def __exit__(self, *a):
        from cdlrm_amd import _lib
        _lib.raw().cdlrm_debug_set(6, 0)
        _lib.raw().cdlrm_debug_set(1, 0)


def query(ops, c, **over):
    a = c.route_args()
    a.update(over)
    with debug(c.debug6, c.debug1):
        return ops.embbag_bwd_route(**a)


# ---- the data of a case: slots, bags, gradients --------------------------------------------------------------------------

class Table:
    """One table (and batch) of a case: slot ids by position, the expected sort, bags."""

    def __init__(self, runs, n, main, aux, aux_regions, seed):
        rng = np.random.RandomState(seed)
        R = len(runs)
        n_aux = min(aux, max(1, R // 8)) if R > 1 else 0
        # distinct slots in increasing order: the sorted layout is exactly the script; the last n_aux runs on aux slots
        main_slots = np.sort(rng.choice(main, R - n_aux, replace=False))
        aux_slots = np.sort(rng.choice(aux * aux_regions, n_aux, replace=False)) + main
        self.run_slot = np.concatenate([main_slots, aux_slots]).astype(np.int64)
        self.runs = np.array(runs, dtype=np.int64)
        sorted_slots = np.repeat(self.run_slot, self.runs)
        perm = np.random.RandomState(1000 + n).permutation(n)       # a fixed scatter: the sort has to gather every run
        self.slots = np.empty(n, dtype=np.int64)
        self.slots[perm] = sorted_slots
        self.keys = np.sort((self.slots.astype(np.uint64) << np.uint64(32)) | np.arange(n, dtype=np.uint64))
        self.pos_sorted = (self.keys & np.uint64(0xffffffff)).astype(np.int64)
        self.starts = np.concatenate([[0], np.cumsum(self.runs)[:-1]])
        self.meta = np.arange(n) - np.repeat(self.starts, self.runs)
        self.once = (np.repeat(self.runs, self.runs) == 1)[np.argsort(self.pos_sorted)].astype(np.uint8)


class Geo:
    """Cache geometry of a case: WAYS ways, P_t sets (different per table: different row bases), two aux regions."""

    def __init__(self, c):
        R = max(len(c.runs), 1)
        self.aux = max(8, R // 8 + 2)
        self.P = [R // WAYS + 5 + 7 * t for t in range(c.T)]
        self.main = [WAYS * p for p in self.P]
        self.rows = [m + 2 * self.aux for m in self.main]
        self.row_base = list(np.concatenate([[0], np.cumsum(self.rows)]).astype(np.int64))


def build(c):
    """Slots [T][batches] (Table), offsets, gradients [T, n_bags, D] of a case (host numpy), deterministic."""
    g = Geo(c)
    batches = list(range(c.j0, c.j0 + c.count)) if c.window else [0]
    regions = 1 if c.window else 2          # window slots are phase-0 aux slots; a batch's own slots may be in either region
    tabs = [{j: Table(c.runs, c.n, g.main[t], g.aux, regions, 7 * t + 131 * j + c.n) for j in batches} for t in range(c.T)]
    off = [_table_bags(c.n, t) for t in range(c.T)] if c.layout == "bags" else [None] * c.T
    n_bags = c.n if off[0] is None else len(off[0])
    assert all(o is None or len(o) == n_bags for o in off)
    rng = np.random.RandomState(c.n + c.D)
    grads = {j: rng.randn(c.T, n_bags, c.D).astype(np.float32) for j in batches}
    return g, tabs, off, n_bags, grads, batches


def bags_of_positions(off, pos):
    """bag_of: the last bag whose offset is <= the position (empty bags in front of it skipped)."""
    return pos if off is None else np.searchsorted(off, pos, side="right") - 1


def grad_layout(c, n_bags):
    """(ld_bag, ld_table, column offset, total columns) of the gradient buffer: tight [n_bags, T*D]; gap: 8 NaN columns after
    every bag row; engine: dfeat[:, 1:, :] of a [n_bags, T + 1, D] buffer (ld_bag = (T + 1) * D, ld_table = D, column 0 NaN)."""
    TD = c.T * c.D
    if c.pitch == "tight":
        return TD, c.D, 0, TD
    if c.pitch == "gap":
        return TD + 8, c.D, 0, TD + 8
    return TD + c.D, c.D, c.D, TD + c.D


# ---- the float64 reference and the comparators ----------------------------------------------------------------------------

def reference(W0, tab, G, off, row_base, main, lr, rest=False, aux_add=0, drop=None, dup_chunk=None, bag_shift=None,
              lr_twice=False, no_aux_shift=False):
    """float64 rows after one SGD step of one table: (rows, ref [R, D], bound [R, D], once-only rows left alone).
    The keyword arguments after aux_add make the reference WRONG the way a kernel bug would (negative controls only)."""
    pos = tab.pos_sorted
    bag = bags_of_positions(off, pos)
    G64 = G.astype(np.float64)
    gs = G64[bag]
    w = np.ones(len(pos))
    if drop is not None:
        w[drop] = 0.0
    if bag_shift is not None:
        gs[bag_shift] = G64[bag[bag_shift] + 1]
    gs = gs * w[:, None]
    sums = np.add.reduceat(gs, tab.starts, axis=0)
    mags = np.add.reduceat(np.abs(G64[bag]), tab.starts, axis=0)
    if dup_chunk is not None:
        r, ch = dup_chunk
        s = tab.starts[r] + ch * SEG
        sums[r] += gs[s:s + SEG].sum(0)
    L = tab.runs
    k = np.minimum(L, SEG) - 1 + (L + SEG - 1) // SEG - 1
    gamma = k * U / (1 - k * U)
    slot = tab.run_slot.copy()
    if not no_aux_shift:
        slot = np.where(slot >= main, slot + aux_add, slot)
    rows = row_base + slot
    step = lr * sums * (2.0 if lr_twice else 1.0)
    ref = W0[rows].astype(np.float64) - step
    bound = C_BOUND * (U * np.abs(ref) + lr * gamma[:, None] * mags)
    keep = np.ones(len(rows), dtype=bool) if not rest else L > 1
    return rows[keep], ref[keep], bound[keep], rows[~keep]


def check_rows(got, W0, updated, ref, bound, what):
    """Rows `updated` within the bound of `ref`; every other row of `got` bit for bit W0's."""
    d = np.abs(got[updated].astype(np.float64) - ref)
    bad = ~(d <= bound)         # NaN fails
    if bad.any():
        i, j = np.argwhere(bad)[0]
        raise AssertionError("%s: row %d col %d: got %r, float64 %r, bound %.3g (%d elements out)" %
                             (what, updated[i], j, got[updated[i], j], ref[i, j], bound[i, j], int(bad.sum())))
    other = np.ones(got.shape[0], dtype=bool)
    other[updated] = False
    same = got[other].view(np.int32) == W0[other].view(np.int32)
    if not same.all():
        r = np.flatnonzero(other)[np.argwhere(~same)[0][0]]
        raise AssertionError("%s: row %d is not in the batch's update and changed" % (what, r))


def check_sort(keys, meta, once, tab, what):
    if not np.array_equal(keys, tab.keys):
        i = int(np.flatnonzero(keys != tab.keys)[0])
        raise AssertionError("%s: sorted key %d is %#x, numpy %#x" % (what, i, int(keys[i]), int(tab.keys[i])))
    if not np.array_equal(meta, tab.meta):
        i = int(np.flatnonzero(meta != tab.meta)[0])
        raise AssertionError("%s: run distance at sorted position %d is %d, numpy %d" % (what, i, meta[i], tab.meta[i]))
    if not np.array_equal(once, tab.once):
        i = int(np.flatnonzero(once != tab.once)[0])
        raise AssertionError("%s: once-only flag of position %d is %d, numpy %d" % (what, i, once[i], tab.once[i]))


def check_touched(touched, expect, what):
    if not np.array_equal(touched.astype(bool), expect):
        i = int(np.flatnonzero(touched.astype(bool) != expect)[0])
        raise AssertionError("%s: touched[%d] is %d, expected %d" % (what, i, touched[i], expect[i]))


def expected_touched(total_rows, run_slots, row_base, main):
    """Every non-aux slot of the batch (aux slots already moved to their region) -- under rest also the once-only ones, which
    the rest kernels still flag."""
    e = np.zeros(total_rows, dtype=bool)
    for t, s in enumerate(run_slots):
        e[row_base[t] + s[s < main[t]]] = True
    return e


# ---- CPU: the comparators reject each bug they are there to catch --------------------------------------------------------

def _emulate_fp32(W0, tab, G, off, row_base, main, lr, aux_add=0):
    """The kernel's arithmetic in float32: in-chunk sums in position order, chunk partials in chunk order, one fma."""
    W = W0.copy()
    bag = bags_of_positions(off, tab.pos_sorted)
    for r, (s0, L) in enumerate(zip(tab.starts, tab.runs)):
        parts = []
        for c0 in range(0, L, SEG):
            acc = np.zeros(G.shape[1], dtype=np.float32)
            for q in range(s0 + c0, s0 + min(L, c0 + SEG)):
                acc = (acc + G[bag[q]]).astype(np.float32)
            parts.append(acc)
        tot = parts[0]
        if L > SEG:
            tot = np.zeros(G.shape[1], dtype=np.float32)
            for p in parts:
                tot = (tot + p).astype(np.float32)
        slot = tab.run_slot[r] + (aux_add if tab.run_slot[r] >= main else 0)
        row = row_base + slot
        W[row] = (W0[row].astype(np.float64) - np.float64(lr) * tot.astype(np.float64)).astype(np.float32)
    return W


def test_comparator_negative_controls():
    """The kernel's own float32 order passes; a dropped lookup of a 33-run, a chunk partial of a 513-run counted twice, the last
    lookup of a bag given to the next bag, an aux slot not shifted by aux_add, -lr applied twice, a touched flag on an aux row and
    a run distance one off at a k_seg_meta tile start each fail."""
    n, D = 1200, 8
    runs = script(n, [(0, 33), (40, 513), (TILE * 3 - 1, 40)])
    main, aux = 300, 40
    tab = Table(runs, n, main, aux, 1, 5)
    off = _bags_of(n)
    n_bags = len(off)
    rng = np.random.RandomState(2)
    G = rng.randn(n_bags, D).astype(np.float32)
    W0 = rng.randn(main + 2 * aux, D).astype(np.float32)
    aux_add = aux
    rows, ref, bound, _ = reference(W0, tab, G, off, 0, main, LR, aux_add=aux_add)
    assert (tab.run_slot >= main).any() and 33 in tab.runs and 513 in tab.runs
    good = _emulate_fp32(W0, tab, G, off, 0, main, LR, aux_add=aux_add)
    check_rows(good, W0, rows, ref, bound, "kernel order")

    def bad(**kw):
        r2, ref2, _, _ = reference(W0, tab, G, off, 0, main, LR, aux_add=aux_add, **kw)
        W = W0.copy()
        W[r2] = ref2.astype(np.float32)
        with pytest.raises(AssertionError):
            check_rows(W, W0, rows, ref, bound, repr(kw))

    r33 = int(np.flatnonzero(tab.runs == 33)[0])
    bad(drop=int(tab.starts[r33]) + 17)
    r513 = int(np.flatnonzero(tab.runs == 513)[0])
    bad(dup_chunk=(r513, 9))
    # the last lookup of a bag with a lookup after it (a bag of >= 2 lookups, not the last bag) attributed to the next bag
    bag = bags_of_positions(off, tab.pos_sorted)
    end = np.append(off[1:], n)
    last = [q for q in range(n) if bag[q] + 1 < n_bags and end[bag[q]] - 1 == tab.pos_sorted[q]
            and end[bag[q]] - off[bag[q]] >= 2 and end[bag[q] + 1] > off[bag[q] + 1]]
    bad(bag_shift=last[0])
    # a second table's offsets found at another stride than ld_off = n_bags + 3: at n_bags (the padding's zeros in front of
    # them), and at 0 (the first table's offsets)
    off1 = _table_bags(n, 1)
    assert len(off1) == n_bags and not np.array_equal(off1, off)
    tab1 = Table(runs, n, main, aux, 1, 6)
    rows1, ref1, bound1, _ = reference(W0, tab1, G, off1, 0, main, LR)
    check_rows(_emulate_fp32(W0, tab1, G, off1, 0, main, LR), W0, rows1, ref1, bound1, "second table, its own offsets")
    for wrong in (np.concatenate([np.zeros(3, dtype=np.int64), off1])[:n_bags], off):
        r2, ref2, _, _ = reference(W0, tab1, G, wrong, 0, main, LR)
        W = W0.copy()
        W[r2] = ref2.astype(np.float32)
        with pytest.raises(AssertionError):
            check_rows(W, W0, rows1, ref1, bound1, "offsets at a wrong stride")
    bad(no_aux_shift=True)
    bad(lr_twice=True)
    # touched: a flag on an aux row
    exp = expected_touched(main + 2 * aux, [tab.run_slot], [0], [main])
    check_touched(exp.astype(np.uint8), exp, "correct flags")
    t2 = exp.copy()
    t2[main + aux + 1] = True
    with pytest.raises(AssertionError, match="touched"):
        check_touched(t2.astype(np.uint8), exp, "aux row flagged")
    # meta one off at a tile start
    check_sort(tab.keys, tab.meta, tab.once, tab, "correct sort")
    m2 = tab.meta.copy()
    assert m2[3 * TILE] > 0          # the 40-run from 767 reaches into the tile at 768: its positions there search leftwards
    m2[3 * TILE] -= 1
    with pytest.raises(AssertionError, match="run distance"):
        check_sort(tab.keys, m2, tab.once, tab, "meta off by one")


@pytest.mark.parametrize("case", [c for c in CASES if c.layout == "bags" and c.T >= 2], ids=lambda c: c.id)
def test_bag_cases_see_a_wrong_offsets_stride(case):
    """The multi-hot cases over two tables would fail a kernel that finds table 1's offsets at another stride than ld_off: at
    n_bags (the padding of table 0's row in front of them) or at 0 (table 0's offsets) -- from the same [T, ld_off] array and
    the same NaN rows of empty bags the GPU test hands the kernel."""
    c = case
    g, tabs, off, n_bags, grads, _ = build(c)
    ld_off = n_bags + c.ld_off_pad
    flat = np.zeros(c.T * ld_off, dtype=np.int64)
    for t in range(c.T):
        flat[t * ld_off:t * ld_off + n_bags] = off[t]
    W0 = np.random.RandomState(4).randn(g.row_base[-1], c.D).astype(np.float32)
    t = 1
    G = grads[0][t].copy()
    G[~(np.diff(np.append(off[t], c.n)) > 0)] = np.nan
    args = (W0, tabs[t][0], G)
    rows, ref, bound, _ = reference(*args, off[t], g.row_base[t], g.main[t], LR, rest=c.rest)
    assert np.isfinite(ref).all()
    for stride in (n_bags, 0):
        r2, ref2, _, _ = reference(*args, flat[t * stride:t * stride + n_bags], g.row_base[t], g.main[t], LR, rest=c.rest)
        W = W0.copy()
        W[r2] = ref2.astype(np.float32)
        with pytest.raises(AssertionError):
            check_rows(W, W0, rows, ref, bound, "%s: offsets at stride %d" % (c.id, stride))


# ---- CPU: the declared routes hold and the table covers the dispatch -----------------------------------------------------

@pytest.mark.parametrize("case", CASES, ids=lambda c: c.id)
def test_declared_route(ops, case):
    r = query(ops, case)
    assert route_str(r) == case.route, "%s: routed to %r, the table declares %r" % (case.id, route_str(r), case.route)
    if not case.window:
        # per batch, the apply finds the keys on its own (bwd_sort_plan's keys_in_b) while the sort leaves them where its merge
        # passes end: the two must agree.  (The window entries hand the apply the views' keys: equal by construction, nothing to check.)
        assert r["apply_keys_off"] == r["keys_off"], "the apply reads other keys than the sort leaves"


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.id)
def test_offsets_lie_inside_the_buffer(ops, case):
    """The sorted keys, run distances and once-only flags the query reports: regions that start 256-byte aligned, distinct, in the
    order of the layout comment (keys A | keys B | meta | ... | once), the last one ending inside the byte count the library
    reports.  (Batch j0 of a window chunk lies j0 * n elements inside its region: it is the region's start that is aligned.)"""
    from cdlrm_amd import _lib
    c, r = case, query(ops, case)
    j = c.j0 if c.window else 0
    offs = (r["keys_off"], r["meta_off"], r["once_off"])
    for off, size in zip(offs, (8, 4, 1)):
        assert off >= 0 and (off - j * c.n * size) % 256 == 0, (offs, size)
    assert offs[0] < offs[1] < offs[2], offs
    assert offs[0] + c.n * 8 <= offs[1] and offs[1] + c.n * 4 <= offs[2], offs
    if c.window:
        assert offs[2] + c.T * c.nb * c.n - c.j0 * c.n <= _lib.raw().cdlrm_embbag_bwd_sorted_bytes(c.T, c.nb, c.n)
    else:
        assert offs[2] + c.T * c.n <= _lib.raw().cdlrm_embbag_bwd_work_bytes(c.T, c.n, c.D)


def test_table_reaches_every_instantiation(ops):
    """Each (apply kernel x ARANGE x LPR) the dispatch can launch, each sort E (the chunk rule never makes 4096-key chunks: E = 4
    is compiled, never launched), odd and even merge-pass counts, both meta writers, and k_bwd_long at every LPR (a run > 32)."""
    applies, sorts, longs = set(), set(), set()
    for c in CASES:
        r = query(ops, c)
        applies.add((r["apply"], r["arange"], r["lpr"]))
        sorts.add(("E", r["sort_e"]))
        sorts.add(("passes", r["merge_passes"] % 2 if r["merge_passes"] else "none"))
        sorts.add(("meta", r["seg_meta"]))
        if max(c.runs) > SEG:
            longs.add(r["lpr"])
    lprs = (4, 8, 16, 32, 64)
    want = {(k, a, l) for k in ("chunks", "blocks") for a in (0, 1) for l in lprs} | {("blocks_lean", 1, l) for l in lprs}
    assert want <= applies, sorted(want - applies)
    assert {("E", 1), ("E", 2), ("E", 8), ("passes", 0), ("passes", 1), ("passes", "none"), ("meta", 0), ("meta", 1)} <= sorts
    assert set(lprs) <= longs
    # the lean form is reachable only without offsets: apply_rest over bags takes the full form
    assert query(ops, Case("x", 100, 16, "rest", "", layout="bags"))["apply"] == "blocks"


def test_table_covers_every_edge():
    """The scripts and sizes the issue of these tests names are all in the table."""
    runs, ns, Ds = set(), set(), set()
    whole = shared = aux = two_tables = False
    tile_starts, straddles = set(), set()
    for c in CASES:
        runs.update(c.runs)
        ns.add(c.n)
        Ds.add(c.D)
        whole |= c.runs == [c.n] and c.n > SEG
        starts = np.concatenate([[0], np.cumsum(c.runs)[:-1]])
        ends = starts + np.array(c.runs)
        for s, L in zip(starts, c.runs):
            for b in range(TILE, c.n, TILE):
                for d in (-1, 0, 1):
                    if s == b + d and c.n > 2048:
                        tile_starts.add(d)
            for b in (1024, 2048, 8192):
                if s < b < s + L:
                    straddles.add(b)
        # a long run whose last chunk head lies in the 32-position bucket where the next long run's head falls
        for i in range(len(c.runs) - 1):
            last_head = starts[i] + ((c.runs[i] - 1) // SEG) * SEG
            if c.runs[i] > SEG and c.runs[i + 1] > SEG and last_head // SEG == starts[i + 1] // SEG:
                shared = True
        aux |= len(c.runs) > 1
        two_tables |= c.T > 1
    need_runs = set(EDGE_RUNS) | set(LOOP_RUNS)
    assert need_runs <= runs, sorted(need_runs - runs)
    assert whole and shared and aux and two_tables
    assert tile_starts == {-1, 0, 1}
    assert straddles == {1024, 2048, 8192}
    assert {1, 31, 1024, 1025, 2048, 2049, 4097, 16384, 16385, 65536} <= ns
    assert {4, 8, 16, 32, 48, 64, 128, 256, 384} <= Ds
    assert {c.debug1 for c in CASES} >= {-1, 0, 1} and {c.debug6 for c in CASES} >= {0, 64, 128}
    assert {c.aux_phase for c in CASES if c.window} == {0, 1} and any(c.batch_len > c.n for c in CASES)
    assert {c.pitch for c in CASES} == {"tight", "gap", "engine"}
    # multi-hot over several tables, each with its own offsets, ld_off > n_bags: table t's row found at t * ld_off, in both
    # apply kernels that read offsets
    strided = {apply_part(c.route).split()[0] for c in CASES if c.layout == "bags" and c.T >= 2 and c.ld_off_pad > 0
               and not np.array_equal(_table_bags(c.n, 0), _table_bags(c.n, 1))}
    assert {"chunks", "blocks"} <= strided


def test_grid_caps(ops):
    """cdlrm_debug_set(1, n): n workgroups per CU (256 CUs) over the tables, -1 uncapped, 0 the default 12 -- for both apply forms;
    k_bwd_long's grid is capped at 1024 regardless."""
    def cdiv(a, b):
        return -(-a // b)

    T, n, D = 26, 65536, 128
    gpb = 256 // 32
    for entry, per in (("apply", cdiv(n, gpb)), ("rest", cdiv(cdiv(n, SEG), gpb))):
        for d1, want in ((-1, per), (1, cdiv(256, T)), (0, cdiv(256 * 12, T)), (20, cdiv(256 * 20, T))):
            with debug(0, d1):
                r = ops.embbag_bwd_route(T, D, n, False, entry)
            assert (r["apply_grid_x"], r["apply_grid_y"]) == (min(want, 65535), T), (entry, d1, r)
            assert r["long_grid"] == 1024


# ---- CPU: every K8 call of a training step is in the table ------------------------------------------------------------------

STEP_D = {"c1": 16, "c2": 32, "c3": 128, "c4": 256, "c5": 128}      # bench.py CONFIGS' embedding widths


def _record_step(D, Bsz):
    """One TrainEngine step on the CPU test double (tests/fake_ops.py, world 1, 26 small tables) with embbag_bwd_prepare /
    embbag_bwd_apply wrapped: their real arguments."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import fake_ops
    import cdlrm_amd.engine as engine
    import cdlrm_amd.model_no_ddp as Mo
    from oracle import cdlrm_oracle as O
    calls = []

    def prep(ctx, slots, work, stream=None):
        calls.append(("prepare", ctx.T, ctx.D, slots.shape[1]))
        return fake_ops.embbag_bwd_prepare(ctx, slots, work, stream)

    def app(ctx, n, offsets, grad, ld_bag, ld_table, lr, work, touched=None, stream=None):
        calls.append(("apply", ctx.T, ctx.D, n, offsets is not None, ld_bag, ld_table, tuple(grad.stride())))
        return fake_ops.embbag_bwd_apply(ctx, n, offsets, grad, ld_bag, ld_table, lr, work, touched, stream)

    class Ops:
        pass

    shim = Ops()
    shim.__dict__.update({k: getattr(fake_ops, k) for k in dir(fake_ops) if not k.startswith("__")})
    shim.embbag_bwd_prepare, shim.embbag_bwd_apply = prep, app
    saved = (engine.ops, Mo.ops, Mo.Embedding_Table_Group.__dict__.get("device_pointers"))
    engine.ops, Mo.ops = shim, shim
    Mo.Embedding_Table_Group.device_pointers = lambda self: self._fake_ptrs
    try:
        T, rows = 26, 40
        ln_emb = np.array([rows] * T)
        nf = T + 1
        bot, top = [13, 64, D], [64, 1]
        ln_top = np.array([D + nf * (nf - 1) // 2] + top)
        host = O.init_host_tables([int(x) for x in ln_emb], D)
        eg = Mo.Embedding_Table_Group(D, ln_emb, init="empty_meta")
        for k in range(T):
            eg.emb_l[k].weight.data = host[k]
        eg._fake_ptrs = fake_ops.register_host(host)
        eg._pinned = True
        np.random.seed(1)
        torch.manual_seed(1)
        cg = Mo.Embedding_Table_Cache_Group(D, ln_emb, 64, Bsz, 4)
        dl = Mo.DLRM_Net(np.array(bot), ln_top, "dot", False, True, -1, ln_top.size - 2, 0.0)
        eng = engine.TrainEngine(cg, dl, eg, lr=0.1, lr_embeds=0.1)
        pipe = engine.WindowPipeline(cg, eg, Bsz, parity_rng=True)
        rng = np.random.RandomState(0)
        X = torch.from_numpy(rng.rand(Bsz, bot[0]).astype(np.float32))
        idx = torch.from_numpy(rng.randint(0, rows, size=(T, Bsz)).astype(np.int64))
        Tt = torch.from_numpy(np.round(rng.rand(Bsz, 1)).astype(np.float32))
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


def _pitch(T, D, ld_bag, ld_table):
    if ld_table != D:
        return "other"
    return {T * D: "tight", (T + 1) * D: "engine"}.get(ld_bag, "gap" if ld_bag > T * D else "other")


@pytest.mark.parametrize("config,batch", [(c, b) for c in ("c1", "c2", "c3", "c4") for b in (1024, 2048, 4096, 8192, 65536)])
def test_training_step_routes_are_in_the_table(ops, config, batch):
    """Every K8 call one training step makes (c1 ... c5 widths -- c5 is c3's at 65536 --, per-rank batches 1024 ... 65536) is a
    case of the table: its sort (which depends on n alone) and its apply (on D, the layout and the entry point), with the
    layout and the grad pitches.  The route query is asked at the step's own T = 26."""
    sorts, applies = set(), set()
    for c in CASES:
        sorts.add(sort_part(c.route))
        applies.add((c.query_entry, apply_part(c.route), c.pitch))
    calls = _record_step(STEP_D[config], batch)
    assert any(k[0] == "prepare" for k in calls) and any(k[0] == "apply" for k in calls), calls
    missing = []
    for call in calls:
        if call[0] == "prepare":
            _, T, D, n = call
            s = sort_part(route_str(ops.embbag_bwd_route(T, D, n, False, "apply")))
            if s not in sorts:
                missing.append(("sort", s, call))
        else:
            _, T, D, n, has_off, ld_bag, ld_table, gstride = call
            assert gstride[0] == ld_bag and gstride[1] == ld_table, call      # dfeat[:, 1:, :]: the pitches are the view's
            key = ("apply", apply_part(route_str(ops.embbag_bwd_route(T, D, n, has_off, "apply"))), _pitch(T, D, ld_bag, ld_table))
            if key not in applies:
                missing.append(key + (call,))
    assert not missing, "step routes the table lacks:\n" + "\n".join(map(repr, missing))


# ---- GPU ------------------------------------------------------------------------------------------------------------------

class Dev:
    """Device state of a case: context, weights, touched flags, slot / offset / gradient buffers."""

    def __init__(self, ops, c, seed=0):
        self.c = c
        self.g, self.tabs, self.off, self.n_bags, self.grads, self.batches = build(c)
        g = self.g
        self.ctx = ops.CacheCtx([10 ** 6] * c.T, g.P, c.D, WAYS, g.aux, torch.device(DEV), aux_phases=2)
        assert self.ctx.row_base == g.row_base and self.ctx.rows == g.rows
        self.tags = torch.full((self.ctx.total_tags,), -1, dtype=torch.int64, device=DEV)
        rng = np.random.RandomState(17 + c.n)
        self.W0 = rng.randn(self.ctx.total_rows, c.D).astype(np.float32)
        self.weight = torch.from_numpy(self.W0).to(DEV)
        self.ctx.bind_cache(self.tags, self.weight)
        self.touched = torch.zeros(self.ctx.total_rows, dtype=torch.uint8, device=DEV)
        self.ld_bag, self.ld_table, self.col0, cols = grad_layout(c, self.n_bags)
        self.gbuf = {}
        for j in self.batches:
            # 8 spare NaN rows behind the last bag: an offset read past n_bags (a wrong bag) stays inside the buffer and poisons
            buf = np.full((self.n_bags + 8, cols), np.nan, dtype=np.float32)
            for t in range(c.T):
                # (each table's own empty bags hold NaN: a lookup given a bag of another table's layout lands on one of them)
                nonempty = np.ones(self.n_bags, dtype=bool) if self.off[t] is None else np.diff(np.append(self.off[t], c.n)) > 0
                c0 = self.col0 + t * self.ld_table
                buf[np.flatnonzero(nonempty), c0:c0 + c.D] = self.grads[j][t][nonempty]
                self.grads[j][t][~nonempty] = np.nan            # an empty bag's gradient row is never read
            self.gbuf[j] = torch.from_numpy(buf).to(DEV)
        if self.off[0] is not None:
            # [T, ld_off] rows of each table's own offsets; the padding behind n_bags is never read (if it were, or a row were
            # found at another stride than ld_off: zeros among the offsets, wrong bags)
            o = np.zeros((c.T, self.n_bags + c.ld_off_pad), dtype=np.int64)
            for t in range(c.T):
                o[t, :self.n_bags] = self.off[t]
            self.offs = torch.from_numpy(o).to(DEV)[:, :self.n_bags]
            assert self.offs.stride(0) == self.n_bags + c.ld_off_pad
        else:
            self.offs = None

    def grad(self, j):
        return self.gbuf[j][:, self.col0:]

    def reset(self):
        self.weight.copy_(torch.from_numpy(self.W0).to(DEV))
        self.touched.zero_()

    def slots_dev(self, j):
        return torch.from_numpy(np.stack([self.tabs[t][j].slots for t in range(self.c.T)]).astype(np.int32)).to(DEV)

    def window_slots(self):
        """The resolver's [T, ld_w] slot ids of the chunk: batch j's n ids at column j * batch_len (other columns: junk that is
        never read -- a valid main slot no batch uses, whose row would show a read)."""
        c = self.c
        ld_w = (c.nb - 1) * c.batch_len + c.n + 3
        ws = np.zeros((c.T, ld_w), dtype=np.int32)
        for t in range(c.T):
            used = np.concatenate([self.tabs[t][j].run_slot for j in self.batches])
            ws[t] = np.setdiff1d(np.arange(self.g.main[t]), used)[-1]
        for j in self.batches:
            for t in range(c.T):
                ws[t, j * c.batch_len:j * c.batch_len + c.n] = self.tabs[t][j].slots
        return torch.from_numpy(ws).to(DEV)

    def expect(self, j, aux_add=None, rest=None, steps=1):
        c = self.c
        aux_add = (c.aux_phase * self.g.aux if c.window else 0) if aux_add is None else aux_add
        rest = c.rest if rest is None else rest
        rows, refs, bounds = [], [], []
        assert steps in (1, 2)
        for t in range(c.T):
            args = (self.W0, self.tabs[t][j], self.grads[j][t], self.off[t], self.g.row_base[t], self.g.main[t])
            r, ref, b, _ = reference(*args, LR * steps, rest=rest, aux_add=aux_add)
            if steps == 2:
                # two SGD steps of the same gradient: 2 lr in the reference, and the first step's rounding of the row, u |W_1|
                b = b + C_BOUND * U * np.abs(reference(*args, LR, rest=rest, aux_add=aux_add)[1])
            rows.append(r); refs.append(ref); bounds.append(b)
        return np.concatenate(rows), np.concatenate(refs), np.concatenate(bounds)


def _u8(buf, off, count, dtype):
    """`count` elements of `dtype` at byte offset `off` of a device uint8 buffer, on the host."""
    nbytes = count * np.dtype(dtype).itemsize
    return buf[off:off + nbytes].cpu().numpy().view(dtype)


def _run(ops, d, j=None):
    """The case's entry point once, from a fresh prepare; returns (route, sort views: [(keys, meta, once) per table])."""
    c = d.c
    j = d.batches[-1] if j is None else j
    with debug(c.debug6, c.debug1):
        r = ops.embbag_bwd_route(**c.route_args())
        if not c.window:
            work = ops.embbag_bwd_work(d.ctx, c.n, DEV)
            sl = d.slots_dev(0)
            if c.entry == "sgd":
                ops.embbag_bwd_sgd(d.ctx, sl, d.offs, d.grad(0), d.ld_bag, d.ld_table, LR, work, d.touched)
            else:
                ops.embbag_bwd_prepare(d.ctx, sl, work)
                f = ops.embbag_bwd_apply_rest if c.rest else ops.embbag_bwd_apply
                f(d.ctx, c.n, d.offs, d.grad(0), d.ld_bag, d.ld_table, LR, work, d.touched)
            torch.cuda.synchronize()
            views = [{0: (_u8(work, r["keys_off"] + t * c.n * 8, c.n, np.uint64), _u8(work, r["meta_off"] + t * c.n * 4, c.n, np.int32),
                          _u8(work, r["once_off"] + t * c.n, c.n, np.uint8))} for t in range(c.T)]
            return r, views, work
        sbuf = ops.embbag_bwd_sorted(d.ctx, c.nb, c.n, DEV)
        ws = d.window_slots()
        ops.embbag_bwd_prepare_window(d.ctx, ws, c.batch_len, c.nb, c.n, sbuf, j0=c.j0, count=c.count)
        work = ops.embbag_bwd_work(d.ctx, c.n, DEV)
        k, m, o = ops.embbag_bwd_sorted_views(d.ctx, sbuf, c.nb, c.n, j)
        ops.embbag_bwd_apply_sorted(d.ctx, c.n, d.grad(j), d.ld_bag, d.ld_table, LR, work, k, m, c.nb * c.n, c.aux_phase, c.rest,
                                    d.touched)
        torch.cuda.synchronize()
        base = sbuf.data_ptr()
        views = [dict() for _ in range(c.T)]
        for jj in range(c.nb):
            k, m, o = ops.embbag_bwd_sorted_views(d.ctx, sbuf, c.nb, c.n, jj)
            if jj == c.j0:
                assert (k - base, m - base, o - base) == (r["keys_off"], r["meta_off"], r["once_off"])
            for t in range(c.T):
                views[t][jj] = (_u8(sbuf, k - base + t * c.nb * c.n * 8, c.n, np.uint64),
                                _u8(sbuf, m - base + t * c.nb * c.n * 4, c.n, np.int32),
                                _u8(sbuf, o - base + t * c.nb * c.n, c.n, np.uint8))
        return r, views, work


@pytest.mark.gpu
@pytest.mark.parametrize("case", [c for c in CASES if c.window], ids=lambda c: c.id)
def test_sorted_views_are_the_query_offsets(ops, case):
    """embbag_bwd_sorted_views needs a context, a context a device; nothing is launched."""
    c = case
    ctx = ops.CacheCtx([10 ** 6] * c.T, Geo(c).P, c.D, WAYS, Geo(c).aux, torch.device(DEV), aux_phases=2)
    sbuf = ops.embbag_bwd_sorted(ctx, c.nb, c.n, DEV)
    r = query(ops, c)
    k, m, o = ops.embbag_bwd_sorted_views(ctx, sbuf, c.nb, c.n, c.j0)
    base = sbuf.data_ptr()
    assert (k - base, m - base, o - base) == (r["keys_off"], r["meta_off"], r["once_off"])


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=lambda c: c.id)
def test_case_vs_float64(ops, case):
    """Sort output exactly, updated rows within the float64 bound, every other row bit for bit, touched exactly, and the same bits
    from a second run."""
    c = case
    d = Dev(ops, c)
    j = d.batches[-1]
    r, views, _ = _run(ops, d)
    assert route_str(r) == c.route
    for t in range(c.T):
        for jj, (k, m, o) in views[t].items():
            if jj in d.tabs[t]:
                check_sort(k, m, o, d.tabs[t][jj], "%s table %d batch %d" % (c.id, t, jj))
            else:       # a window batch outside the slice: its lists are left alone (the buffer's zero fill)
                assert not k.any() and not m.any() and not o.any(), "%s: batch %d outside the slice was written" % (c.id, jj)
    got = d.weight.cpu().numpy()
    rows, ref, bound = d.expect(j)
    check_rows(got, d.W0, rows, ref, bound, c.id)
    aux_add = c.aux_phase * d.g.aux if c.window else 0
    shifted = [np.where(d.tabs[t][j].run_slot >= d.g.main[t], d.tabs[t][j].run_slot + aux_add, d.tabs[t][j].run_slot)
               for t in range(c.T)]
    check_touched(d.touched.cpu().numpy(), expected_touched(len(got), shifted, d.g.row_base, d.g.main), c.id)
    first = d.weight.clone()
    d.reset()
    _run(ops, d)
    assert torch.equal(first, d.weight), "%s: two runs differ" % c.id


XROUTE = [c for c in CASES if c.id in ("n1024_d16_edges", "n2049_d128_t2_tiles", "n4097_d48_loops", "n16385_d384_cc2",
                                       "bags_n1025_d64", "blkbag_n4097_d128", "lean_n2049_d32")]


@pytest.mark.gpu
@pytest.mark.parametrize("case", XROUTE, ids=lambda c: c.id)
def test_apply_kernels_and_grids_same_bits(ops, case):
    """One prepare, then every apply form over it: k_bwd_chunks, the full k_bwd_blocks (6, 64), the lean rest and the full rest
    (6, 128), each at grid caps -1 / 1 / default -- the same bits over the rows each one updates (the rest forms leave the
    once-only rows alone)."""
    c = case
    d = Dev(ops, c)
    work = ops.embbag_bwd_work(d.ctx, c.n, DEV)
    ops.embbag_bwd_prepare(d.ctx, d.slots_dev(0), work)
    results = {}
    forms = [("chunks", 0, False), ("blocks", 64, False), ("rest", 128, True)]
    if c.layout == "arange":
        forms.append(("rest_lean", 0, True))
    for name, d6, rest in forms:
        for d1 in (-1, 1, 0):
            d.reset()
            with debug(d6, d1):
                f = ops.embbag_bwd_apply_rest if rest else ops.embbag_bwd_apply
                f(d.ctx, c.n, d.offs, d.grad(0), d.ld_bag, d.ld_table, LR, work, d.touched)
                torch.cuda.synchronize()
            results[(name, d1)] = d.weight.cpu().numpy().view(np.int32).copy()
    base = results[("chunks", 0)]
    once_rows = np.concatenate([d.g.row_base[t] + d.tabs[t][0].run_slot[d.tabs[t][0].runs == 1] for t in range(c.T)])
    multi = np.ones(base.shape[0], dtype=bool)
    multi[once_rows] = False
    for key, w in results.items():
        if key[0].startswith("rest"):
            assert np.array_equal(w[multi], base[multi]), "%s %r: rows of runs >= 2 differ from k_bwd_chunks" % (c.id, key)
            assert np.array_equal(w[once_rows], d.W0.view(np.int32)[once_rows]), "%s %r: a once-only row changed" % (c.id, key)
        else:
            assert np.array_equal(w, base), "%s %r: differs from k_bwd_chunks at the default grid" % (c.id, key)


@pytest.mark.gpu
@pytest.mark.parametrize("case", [c for c in CASES if c.id in ("n4097_d48_loops", "lean_n4097_d64", "bags_n4097_d128",
                                                                 "blk_n2049_d32")], ids=lambda c: c.id)
def test_repeated_apply(ops, case):
    """Two applies on one prepare are two SGD steps (k_bwd_long's last workgroup empties the long-run list for the second)."""
    c = case
    d = Dev(ops, c)
    work = ops.embbag_bwd_work(d.ctx, c.n, DEV)
    with debug(c.debug6, c.debug1):
        ops.embbag_bwd_prepare(d.ctx, d.slots_dev(0), work)
        f = ops.embbag_bwd_apply_rest if c.rest else ops.embbag_bwd_apply
        for _ in range(2):
            f(d.ctx, c.n, d.offs, d.grad(0), d.ld_bag, d.ld_table, LR, work, d.touched)
        torch.cuda.synchronize()
    rows, ref, bound = d.expect(0, steps=2)
    check_rows(d.weight.cpu().numpy(), d.W0, rows, ref, bound, c.id + " x2")


@pytest.mark.gpu
@pytest.mark.parametrize("case", [c for c in CASES if c.window], ids=lambda c: c.id)
def test_window_equals_batch_sort(ops, case):
    """A window-sorted apply gives the bits of the per-batch prepare + apply of the same slots (aux slots moved to the batch's
    aux region, as cdlrm_embbag_take does)."""
    c = case
    d = Dev(ops, c)
    j = d.batches[-1]
    _run(ops, d)
    win = d.weight.clone()
    win_t = d.touched.clone()
    d.reset()
    with debug(c.debug6, c.debug1):
        aux_add = c.aux_phase * d.g.aux
        sl = np.stack([np.where(d.tabs[t][j].slots >= d.g.main[t], d.tabs[t][j].slots + aux_add, d.tabs[t][j].slots)
                       for t in range(c.T)]).astype(np.int32)
        work = ops.embbag_bwd_work(d.ctx, c.n, DEV)
        ops.embbag_bwd_prepare(d.ctx, torch.from_numpy(sl).to(DEV), work)
        f = ops.embbag_bwd_apply_rest if c.rest else ops.embbag_bwd_apply
        f(d.ctx, c.n, None, d.grad(j), d.ld_bag, d.ld_table, LR, work, d.touched)
        torch.cuda.synchronize()
    assert torch.equal(win, d.weight), "%s: window-sorted and per-batch results differ" % c.id
    assert torch.equal(win_t, d.touched)
