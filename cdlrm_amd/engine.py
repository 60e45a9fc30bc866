"""The fused per-GPU training engine behind `main_no_ddp.Run` and bench.py.

`TrainEngine.step()` is the reference's loop body (main_no_ddp.py:401-423) as one fixed sequence of
libcdlrm_hip.so launches on preallocated buffers -- no autograd graph, no per-table Python loop:

    bottom MLP -> gather (slots probed one step ahead) -> interaction -> top MLP -> BCE -> top dgrad chain
          -> interaction bwd -> fused embedding bwd + sparse SGD || bottom dgrad chain || weight gradients
          -> grad all-reduce (RCCL) -> dense SGD -> every table_agg_freq steps: touched-row merge across ranks

Four HIP streams: main (the chain above), side (embedding backward; the slot sort of batches without sorted lists; under
the chained take the next batch's take), pref (with two aux regions the NEXT batch's take / tag probe and aux-row fill into
the other aux region; the look-ahead chunks' resolve; the slot sorts `WindowResolver` issues slice by slice, batches ahead of
their steps -- the embedding backward's sort, off every queue a step waits for, whose once-only flags let the interaction
backward update the slots a batch reads once; at long batches also the top MLP's weight gradients) and the window plan's.
The launch sequence of a step is recorded once per control path and replayed (`_step_taped`).

`WindowPipeline` is the look-ahead side: it plans window w+1 (unique scan, tag probe, way choice, winners-
only pinned-host -> HBM row fetch) on a side HIP stream while window w trains, and commits it at the
boundary (main_no_ddp.py:393-399, 148-209; cache_manager.py:66-115).
"""
from __future__ import annotations

import itertools
import math
import os
from typing import List, NamedTuple, Optional

import numpy as np
import torch
import torch.distributed as dist

from . import _lib
from . import _streams as S
from . import ops
from ._lib import record as rec
from .lr_schedule import RateCell, effective_rate
from .model_no_ddp import DLRM_Net, Embedding_Table_Cache_Group, Embedding_Table_Group, _linears


# serial numbers of the slice sorts (WindowResolver.ensure_sorted), unique in the process: the slice events are a ring shared by
# every resolver of an engine and re-recorded every RING chunks, so a step tells one slice's sort from the next by its serial
_SORT_SERIAL = itertools.count(1)


def square_bags(lS_o, lS_i, device=None, multiple: int = 256):
    """Ragged multi-hot bags (the reference's random front end: T index lists of different lengths + T offset lists,
    dlrm_data_pytorch.py:763-805) -> the rectangular layout the kernels take: (offsets int64 [T, n_bags + 1],
    indices int64 [T, n]).  Tables are squared off with ONE extra bag: the padding lookups of table k repeat its first
    index of the batch (no new row is touched, no new window index appears) and are pooled into bag n_bags, a scratch row
    behind the batch whose gradient is zero -- adding lr * 0 leaves the cache rows bit-identical.  n is rounded up to
    `multiple` so that a stream of batches reuses a few buffer shapes.  Rectangular inputs pass through unchanged."""
    if isinstance(lS_i, torch.Tensor) and lS_i.dim() == 2:
        off = lS_o if isinstance(lS_o, torch.Tensor) or lS_o is None else torch.stack(list(lS_o))
        return (None if off is None else off.to(device) if device is not None else off,
                lS_i.to(device) if device is not None else lS_i)
    idx_l = [torch.as_tensor(x).reshape(-1).to(torch.int64) for x in lS_i]
    off_l = [torch.as_tensor(x).reshape(-1).to(torch.int64) for x in lS_o]
    T, nb = len(idx_l), int(off_l[0].numel())
    lens = [int(x.numel()) for x in idx_l]
    assert min(lens) >= 1 and all(int(o.numel()) == nb for o in off_l), "every table needs >= 1 lookup and n_bags offsets"
    n = (max(lens) + multiple - 1) // multiple * multiple
    idx = torch.empty(T, n, dtype=torch.int64)
    off = torch.empty(T, nb + 1, dtype=torch.int64)
    for k in range(T):
        idx[k, :lens[k]] = idx_l[k]
        idx[k, lens[k]:] = idx_l[k][0]
        off[k, :nb] = off_l[k]
        off[k, nb] = lens[k]
    if device is not None:
        idx, off = idx.to(device), off.to(device)
    return off, idx


def pad_window(lists, device=None):
    """A look-ahead window of ragged per-table index lists -> int64 [T, n]: the plan only needs each table's SET of
    indices, so short tables are padded with their own first index."""
    lists = [torch.as_tensor(x).reshape(-1).to(torch.int64) for x in lists]
    n = max(int(x.numel()) for x in lists)
    out = torch.empty(len(lists), n, dtype=torch.int64)
    for k, x in enumerate(lists):
        out[k, :x.numel()] = x
        out[k, x.numel():] = x[0]
    return out.to(device) if device is not None else out


def rank_bag_slice(off: torch.Tensor, lens: torch.Tensor, lbs: int, rank: int, multiple: int = 256):
    """The rank slice of one batch of ragged multi-hot bags.  off: int64 [T, B] global offsets, lens:
    int64 [T] lengths of the batch's table lists, both on the host; lbs: the local batch size ceil(mini_batch_size / world)
    -- of the run, not of this batch: a short last batch (--data-size not a multiple of the batch) is cut where the
    reference and the one-lookup path cut it, X[r * lbs:(r + 1) * lbs] (main_no_ddp.py:344, 388-391).  Rank r trains
    samples [s0, s1) = [min(B, r * lbs), min(B, (r + 1) * lbs)); of table k it takes the lookups of exactly those bags,
    [a_k, e_k) = [off[k, s0], off[k, s1]) (e_k = lens[k] when s1 = B).  With one lookup per bag this is the reference's
    lS_i[:, s0:s1].  Returns (s0, s1, a [T], e [T], n); n = the squared width of the rank's lists, max(e - a) rounded up to
    `multiple` as square_bags() rounds.  O(T) tensor ops, no loop over the tables.  Raises ValueError when the rank has no
    sample or a table slice holds no lookup: padding such a table would need an index the rank never looked up, which would
    add an untouched row to its merge set."""
    T, B = off.shape
    s0, s1 = min(B, rank * lbs), min(B, (rank + 1) * lbs)
    if s0 >= s1:
        raise ValueError("multi-hot bags: rank %d has no sample of a batch of %d (local batch %d): every rank needs >= 1 "
                         "sample per batch" % (rank, B, lbs))
    a = off[:, s0]
    e = off[:, s1] if s1 < B else lens
    m = e - a
    if int(m.min()) < 1:
        k = int(torch.argmin(m))
        raise ValueError("multi-hot bags: rank %d's slice [%d, %d) of table %d holds no lookup (every table needs >= 1 "
                         "lookup per rank slice)" % (rank, s0, s1, k))
    n = (int(m.max()) + multiple - 1) // multiple * multiple
    return s0, s1, a, e, n


class BagWindow:
    """One look-ahead window of ragged multi-hot batches in HBM (BagWindows.load): the plan's rectangle and every step's
    per-rank squared lists, each one launch on the current stream."""

    def __init__(self, owner, buf, bpos, dev_off, host_off, lens, n_win):
        self._o, self.buf, self.bpos = owner, buf, bpos
        self.dev_off, self.host_off, self.lens = dev_off, host_off, lens
        self.L, self.n_win = len(dev_off), n_win

    def window_indices(self) -> torch.Tensor:
        """int64 [T, n_win]: pad_window() of the window's global lists."""
        return ops.bags_window(self.buf, self.bpos, self.L, self.n_win)

    def rank_batch(self, b: int):
        """(off int64 [T, nb + 1], idx int64 [T, n], samples) of batch b for this rank: square_bags() of the rank's rebased
        lookups, and slice(s0, s1) -- the rows of the batch's X and T they belong to."""
        o = self._o
        s0, s1, _, _, n = rank_bag_slice(self.host_off[b], self.lens[b], o.lbs, o.rank, o.multiple)
        off, idx = ops.bags_rank_slice(self.buf, self.bpos, self.L, b, self.dev_off[b], s0, s1, n)
        return off, idx, slice(s0, s1)


class BagWindows:
    """Ragged multi-hot batches on the device for the rank slices at world_size > 1.  load(win) packs a window's global
    lists -- per table the window's batches concatenated, then the list positions, then every batch's offsets -- into
    pinned staging and moves them with ONE host-to-device copy into the next buffer of a ring of two: with --device-rng
    the next window is loaded and planned while the current one trains.  Every launch (copy, slices) is on the current
    stream, so a buffer is refilled two windows later behind every slice cut from it.  local_batch_size: ceil(mini_batch_size
    / world_size), the run's rank slice width (rank_bag_slice).  At world_size 1 the host path (square_bags / pad_window)
    stays."""

    RING = 2

    def __init__(self, num_tables: int, device, local_batch_size: int, world_size: int = 1, rank: int = 0, multiple: int = 256):
        self.T, self.dev = int(num_tables), torch.device(device)
        self.lbs, self.world, self.rank, self.multiple = int(local_batch_size), int(world_size), int(rank), int(multiple)
        self._stage = [None] * self.RING       # pinned int64 staging
        self._buf = [None] * self.RING         # int64 device buffer
        self._copied = [None] * self.RING      # event behind the copy out of the staging buffer
        self._next = 0

    def load(self, win) -> BagWindow:
        """win: the window's batches (X, lS_o, lS_i, T) as the loader hands them out -- lS_o [T, B] (or T lists of B), lS_i T
        ragged lists.  Checks every rank's slices (the same decision on every rank), then stages and copies."""
        T, L = self.T, len(win)
        host_off = [torch.as_tensor(b[1]).to(torch.int64).reshape(T, -1) if isinstance(b[1], torch.Tensor) else
                    torch.stack([torch.as_tensor(o).reshape(-1).to(torch.int64) for o in b[1]]) for b in win]
        lists = [[torch.as_tensor(b[2][k]).reshape(-1) for b in win] for k in range(T)]     # table-major
        lens = torch.tensor([[int(lists[k][j].numel()) for k in range(T)] for j in range(L)], dtype=torch.int64)  # [L, T]
        if int(lens.min()) < 1:
            raise ValueError("multi-hot bags: every table needs >= 1 lookup per batch")
        for j in range(L):
            for r in range(self.world):
                rank_bag_slice(host_off[j], lens[j], self.lbs, r, self.multiple)
        tab_len = lens.sum(0)                                           # [T]
        tab_start = torch.cumsum(tab_len, 0) - tab_len
        bpos = torch.cat([tab_start.view(1, T), tab_start.view(1, T) + torch.cumsum(lens, 0)])   # [L + 1, T]
        total = int(tab_len.sum())
        n_pos, n_off = (L + 1) * T, sum(int(o.numel()) for o in host_off)
        N = total + n_pos + n_off
        i = self._next
        self._next = (i + 1) % self.RING
        if self._copied[i] is not None:
            self._copied[i].synchronize()           # the previous copy out of this staging buffer has been read
        if self._stage[i] is None or self._stage[i].numel() < N:
            cap = 1 << max(16, (N - 1).bit_length())
            self._stage[i] = S.pinned(torch.empty(cap, dtype=torch.int64), self.dev)
            self._buf[i] = torch.empty(cap, dtype=torch.int64, device=self.dev)
        st, buf = self._stage[i], self._buf[i]
        torch.cat([x.to(torch.int64) for row in lists for x in row] + [bpos.reshape(-1)] + [o.reshape(-1) for o in host_off],
                  out=st[:N])
        buf[:N].copy_(st[:N], non_blocking=True)
        ev = S.new_event(self.dev)
        ev.record(S.current_stream(self.dev))
        self._copied[i] = ev
        dev_off, p = [], total + n_pos
        for o in host_off:
            dev_off.append(buf[p:p + o.numel()].view(o.shape))
            p += o.numel()
        return BagWindow(self, buf[:total], buf[total:total + n_pos], dev_off, host_off, lens, int(tab_len.max()))


class WindowPipeline:
    def __init__(self, cache_group: Embedding_Table_Cache_Group, host_tables: Embedding_Table_Group, max_window: int,
                 *, parity_rng: bool = False, seed: int = 0, average_on_writeback: bool = False, rank: int = 0,
                 world_size: int = 1, cap_uniq: Optional[int] = None, cap_win: Optional[int] = None,
                 victim_rows: Optional[int] = None, host_gather: bool = False, gather_threads: int = 16,
                 shard_fetch: Optional[bool] = None, process_group=None, write_back: bool = True,
                 force_collectives: bool = False, insert_policy: str = "reference"):
        """victim_rows: capacity (rows) of each of the two HBM buffers that hold the host rows of a window's
        non-cached indices (None: every unique index of a window, at most 8 GiB per buffer; 0: off -- every miss
        reads the host table over PCIe as the reference does).
        host_gather: move the plan's bulk rows (winners, victims) the way the reference's Prefetcher does -- CPU threads
        gather them from the host tables into pinned staging, ONE DMA copy brings them to HBM -- from a background
        thread, instead of GPU waves reading host memory (which slows every kernel beside them ~2x while they run;
        a DMA copy costs the training ~2 %).  Not with parity_rng (that path draws its random numbers in-line).
        shard_fetch (host_gather plans at world_size > 1; default on): every rank's plan is the same list of rows, so
        each rank fetches only its 1/world slice from the host tables (CPU gather + DMA over ITS PCIe link) and the
        slices are exchanged over xGMI with one all-gather per list at the window boundary (commit(), main thread,
        same point of the step sequence on every rank).  Host-DRAM and PCIe traffic per window drop from
        world x (winners + victims) to 1 x; the reference instead broadcasts whole cache tables from rank 0
        (main_no_ddp.py:318-319).
        write_back=False: evicted rows are dropped instead of written to the host tables (repeatability tests that must
        leave the host tables as they found them; never in training).
        force_collectives: take the multi-rank code paths (sharded fetch + in-place all-gather, barrier) at world_size 1
        too -- a 1-rank communicator executes every collective the N-rank run issues (tests/test_rccl_one_rank.py).
        insert_policy: which of a window's new indices get a slot.  "reference": every claimant picks a random unprotected
        way, a contested slot goes to the claimant latest in index order (main_no_ddp.py:171-204).  "fill": the
        collision-free, frequency-ranked policy (cdlrm_plan_assign_fill) -- a count pass over the window's lookups
        runs between the probe and the assignment (a streamed window is iterated a second time for it), every set inserts
        min(claimants, free ways) rows, and no random number is drawn: with parity_rng the fill policy takes nothing from
        the torch CPU generator (and ignores q_source), with the device RNG the seed has no effect on the plan."""
        if insert_policy not in ("reference", "fill"):
            raise ValueError("insert_policy must be 'reference' or 'fill', not %r" % (insert_policy,))
        self.insert_policy = insert_policy
        self.cg, self.host = cache_group, host_tables
        self.write_back = bool(write_back)
        self.ctx = cache_group.ctx
        self.plan = ops.WindowPlan(self.ctx, max_window, cap_uniq, cap_win)
        # Each of the two victim buffers starts at <= 8 GiB and GROWS when a window's plan lists more non-cached indices than it
        # holds (host-gather plans: the count is on the host before any row moves), up to a fifth of the device's memory per
        # buffer: a Zipf window at c3 leaves 9-10 M victims (5 GB), a UNIFORM one 76 M (39 GB) -- cut at 8 GiB, four of five
        # misses of every step read the host table over PCIe inside the step (0.90 instead of 0.70 ms/step).  288 GB of HBM are
        # there to be used; what does not fit even then is still served from the host table, as the reference serves all of it.
        self.victim_limit = 0
        if victim_rows is None:
            victim_rows = min(self.plan.cap_uniq, (8 << 30) // (4 * self.ctx.D))
            if S.is_hip(cache_group.weight.device):
                total = torch.cuda.get_device_properties(cache_group.weight.device).total_memory
                self.victim_limit = min(self.plan.cap_uniq, int(total * 0.2) // (4 * self.ctx.D))
        self.victims = [ops.Victims(self.ctx, victim_rows) for _ in range(2)] if victim_rows > 0 else None
        self._vnext = 0
        self.dev = cache_group.weight.device
        # the plan's stream: least urgent priority -- the window scan shares the GPU with the training step, which goes first
        self.side = S.background_stream(self.dev)
        self.parity_rng, self.seed, self.avg = parity_rng, int(seed), average_on_writeback
        self.rank, self.world = rank, world_size
        self.multi = self.world > 1 or bool(force_collectives)
        self.host_ptrs = host_tables.device_pointers()
        self.ctx.bind_host_tables(self.host_ptrs)
        # every rank holds a private copy of the host tables (hostmem.make_host_tables "replicas"): every rank writes its evictions
        # back -- identical rows on every rank at a commit (sync_touched_to_rank0 precedes it), so the copies stay identical
        self.replicated_host = bool(getattr(host_tables, "_replicated", False))
        self.window_no = 0
        self._commits = 0
        self.planned = None          # event: plan of the next window is ready
        self.written_back = None     # event: evictions of the last commit are in the host tables
        self.last_offsets = None
        self.host_gather = bool(host_gather) and not parity_rng and S.is_hip(self.dev)
        self.gather_threads = int(gather_threads)
        if shard_fetch is None:
            shard_fetch = True
        self.shard = bool(shard_fetch) and self.host_gather and self.multi
        self.pg = process_group
        self._exchange = []          # (buffer, chunk rows) all-gathers commit() owes for the plan in flight
        self._worker = None          # background thread of a host-gather plan
        self._worker_err = None
        self._pin = {}               # pinned host staging, grown on demand
        # where the last host-gather plan's time went (ms, host clock of the plan thread; `dma` from events at commit()):
        # the GPU half (window scan, tag probe, way choice, victim list), list copies to the host, first-touch allocation of
        # pinned staging (first window only, or when a list outgrows it), the CPU threads' row gather, the DMA copies
        self._breakdown = None
        self._bd = None

    @property
    def breakdown(self):
        """Itemised cost of the last committed host-gather plan (None before the first).  Reading it waits for that plan's
        DMA copies (instrumentation: commit() itself never blocks the host for it)."""
        return self.resolve_breakdown(self._breakdown)

    def breakdown_deferred(self):
        """The same record WITHOUT waiting for anything: hand it to resolve_breakdown() later (bench.py: after the timed region)."""
        return self._breakdown

    @staticmethod
    def resolve_breakdown(bd):
        if bd is not None and "_dma_events" in bd:
            evs = bd.pop("_dma_events")
            if evs and isinstance(evs[0][0], torch.cuda.Event):
                evs[-1][1].synchronize()
                bd["dma"] = float(sum(a.elapsed_time(b) for a, b in evs))
        return bd

    def _pinned(self, key, shape, dtype):
        t = self._pin.get(key)
        if t is None or t.shape[0] < shape[0]:
            import time as _time
            t0 = _time.perf_counter()
            rows = int(shape[0] * 1.25) + 1024
            t = torch.empty((rows,) + tuple(shape[1:]), dtype=dtype, pin_memory=True)
            self._pin[key] = t
            if self._bd is not None:
                self._bd["pinned_alloc"] += (_time.perf_counter() - t0) * 1e3
        return t

    def reserve_staging(self, win_rows: int, victim_rows: int):
        """Allocate the pinned host staging of a host-gather plan up front (rows of the winners' / victims' lists a window
        may produce): pinning GBs of host memory costs ~1 s the first time a plan needs it; a trainer that knows its window
        size pays it at set-up, not inside its first window."""
        D = self.ctx.D
        for key, rows in (("win", win_rows), ("vic", victim_rows)):
            if rows > 0:
                self._pinned(key + "_idx", (int(rows),), torch.int64)
                self._pinned(key + "_rows", (int(rows), D), torch.float32)

    def _shard_range(self, n, cap_rows):
        """This rank's slice of a list of n rows that travels as `world` equal chunks: (chunk, lo, hi), or None when the
        list is fetched whole (sharding off, empty list, or the padded length would not fit the buffer)."""
        if not self.shard or n == 0:
            return None
        chunk = -(-n // self.world)
        if chunk * self.world > cap_rows:
            return None
        lo = min(self.rank * chunk, n)
        return chunk, lo, min(lo + chunk, n)

    def _fetch_list(self, key, idx_dev, off, n, dst_dev, D):
        """Rows of one plan list (n entries, `off` = per-table offsets into it) -> dst_dev[:n]: CPU-thread gather into
        pinned staging + one DMA copy, of the whole list or of this rank's slice (the exchange is queued for commit())."""
        import time as _time
        side, bd = self.side, self._bd
        sh = self._shard_range(n, dst_dev.shape[0])
        chunk, lo, hi = sh if sh is not None else (0, 0, n)
        m = hi - lo
        alloc0 = bd["pinned_alloc"] if bd is not None else 0.0
        t0 = _time.perf_counter()
        idx_h = self._pinned(key + "_idx", (max(m, 1),), torch.int64)
        idx_h[:m].copy_(idx_dev[lo:hi], non_blocking=True)
        side.synchronize()
        t1 = _time.perf_counter()
        if bd is not None:          # (a first-touch allocation of the index staging is itemised as pinned_alloc, not here)
            bd["lists_to_host"] -= bd["pinned_alloc"] - alloc0
        if m > 0:
            rows_h = self._pinned(key + "_rows", (m, D), torch.float32)
            t2 = _time.perf_counter()
            off_r = [min(max(int(o), lo), hi) - lo for o in off]
            ops.host_gather_rows(self.host_ptrs, idx_h, off_r, D, rows_h, self.gather_threads)
            t3 = _time.perf_counter()
            ev0, ev1 = S.new_event(self.dev, timing=True), S.new_event(self.dev, timing=True)
            ev0.record(side)
            dst_dev[lo:hi].copy_(rows_h[:m], non_blocking=True)
            ev1.record(side)
            if bd is not None:
                bd["cpu_gather"] += (t3 - t2) * 1e3
                bd["_dma_events"].append((ev0, ev1))
                bd["rows"][key] = m
        if bd is not None:
            bd["lists_to_host"] += (t1 - t0) * 1e3
        if sh is not None:
            self._exchange.append((dst_dev, chunk))

    def _plan_host_gather(self, window_idx, lists_ready, t_launch):
        """Background half of a host-gather plan: wait for the winner / victim lists, copy them down, gather the rows on
        the CPU, issue the two DMA copies and the `planned` event on the plan stream."""
        try:
            import time as _time
            torch.cuda.set_device(self.dev)
            plan, side, T, D = self.plan, self.side, self.ctx.T, self.ctx.D
            vic = self.victims[self._vnext] if self.victims is not None else None
            bd = self._bd = dict(gpu_scan_probe_assign=0.0, lists_to_host=0.0, pinned_alloc=0.0, cpu_gather=0.0, dma=None,
                                 rows={}, threads=self.gather_threads, sharded=self.shard, _dma_events=[])
            lists_ready.synchronize()
            bd["gpu_scan_probe_assign"] = (_time.perf_counter() - t_launch) * 1e3
            t0 = _time.perf_counter()
            _, _, wo = plan.offsets(stream=side)
            W = wo[T]
            bd["lists_to_host"] += (_time.perf_counter() - t0) * 1e3
            with torch.cuda.stream(side):
                self._fetch_list("win", plan.win_idx, wo, W, plan.stage, D)
                if vic is not None:
                    t0 = _time.perf_counter()
                    voff = vic.off.cpu().tolist()
                    bd["lists_to_host"] += (_time.perf_counter() - t0) * 1e3
                    need = voff[T + 1]               # what the window has; voff[T] = what the buffer holds of it
                    if need > vic.cap and self.victim_limit > vic.cap:
                        # more victims than this buffer holds: a larger one (this is the buffer of the window being planned:
                        # nothing reads it yet), and the list again
                        t0 = _time.perf_counter()
                        side.synchronize()
                        old_cap, vic = vic.cap, None        # (no reference of ours keeps the old buffer alive)
                        grown = self._grow_victims(old_cap, min(self.victim_limit, int(need * 1.1) + 4096), self._commits == 0)
                        vic = self.victims[self._vnext]
                        if grown:
                            plan.victims(vic, stream=side, list_only=True)
                            voff = vic.off.cpu().tolist()
                        bd["victims_regrown_ms"] = (_time.perf_counter() - t0) * 1e3
                    bd["victims_in_window"], bd["victim_capacity"] = int(voff[T + 1]), int(vic.cap)
                    V = min(voff[T], vic.cap)
                    voff = [min(o, V) for o in voff[:T + 1]]
                    self._fetch_list("vic", vic.idx, voff, V, vic.rows, D)
                bd["host_total"] = (_time.perf_counter() - t_launch) * 1e3
                if isinstance(window_idx, torch.Tensor) and window_idx.is_cuda:
                    window_idx.record_stream(side)
                self.planned = S.new_event(self.dev)
                self.planned.record(side)
        except BaseException as e:          # surfaced by commit()
            self._worker_err = e

    def _grow_victims(self, old_cap: int, want: int, both: bool) -> bool:
        """Replace the victim buffer of the window being planned (both: the other one too -- the very first plan, when neither is
        bound: sized now, beside a plan nobody trains next to, instead of inside the second window; a 40 GB allocation holds the
        device for ~1 s) by one of `want` rows -- or of what the device has FREE right now, less 4 GiB of headroom for the
        trainer's own later allocations: this runs in the plan's background thread in the middle of training, where an
        out-of-memory error would surface windows after set-up.  True: the buffers are new objects (the list has to be made
        again); False: the old ones stay -- the misses that do not fit read the host table, as the reference serves all of them."""
        n_buf = 2 if both else 1
        row = 4 * self.ctx.D + 12                     # row + index + position per entry (ops.Victims)
        if self.multi:
            # Several ranks: the capacity has to come out THE SAME on every rank -- with the sharded fetch V = min(victims,
            # capacity) sets the chunk sizes (and the number) of commit()'s all-gathers, and the bound victim set has to be one
            # set.  So nothing rank-local enters: `want` derives from the window's victim count (the replicated plan: equal
            # everywhere) and victim_limit (a fifth of the device's TOTAL memory); this rank's free memory does not, and there is
            # no smaller-size fallback -- a rank that cannot allocate what the others allocate stops the job here, loudly,
            # instead of training on a different victim set.
            cap = int(want)
            if cap <= old_cap:
                return False
            slots = [self._vnext, self._vnext ^ 1][:n_buf]
            for i in slots:
                self.victims[i] = None
            try:
                for i in slots:
                    self.victims[i] = ops.Victims(self.ctx, cap)
            except torch.OutOfMemoryError as e:
                raise RuntimeError("rank %d: victim buffers of %d rows (the capacity every rank allocates) do not fit this "
                                   "device: lower --lookahead or pass victim_rows" % (self.rank, cap)) from e
            return True
        free = torch.cuda.mem_get_info(self.dev)[0] if S.is_hip(self.dev) else (1 << 62)
        free += n_buf * old_cap * row                 # what releasing the old buffer(s) gives back
        cap = int(min(want, (free - (4 << 30)) // (n_buf * row)))
        if cap <= old_cap:
            return False
        slots = [self._vnext, self._vnext ^ 1][:n_buf]
        for c in (cap, old_cap):
            try:
                for i in slots:
                    self.victims[i] = None
                for i in slots:
                    self.victims[i] = ops.Victims(self.ctx, c)
                return True
            except torch.OutOfMemoryError:          # (the allocator's view and the driver's can differ): the old size again
                for i in slots:
                    self.victims[i] = None
                torch.cuda.empty_cache()
        raise RuntimeError("victim buffers: not even the previous capacity could be allocated again")

    def _unique(self, window_idx, side):
        """K1 on the plan stream: one [T, n] tensor, or a window streamed as chunks (a callable returning an iterator
        of [T, n_c] tensors, produced on the plan stream: a window that does not fit HBM in one piece)."""
        plan = self.plan
        if callable(window_idx):
            for chunk in window_idx():
                plan.unique_add(chunk, stream=side)
                del chunk
            plan.unique_finish(stream=side)
        else:
            plan.unique(window_idx, stream=side)

    def _assign_fill(self, window_idx, side):
        """The "fill" policy's half of a plan, between probe and fetch: count the window's lookups per unique index, then
        the ranked way assignment."""
        plan = self.plan
        plan.count_reset(stream=side)
        if callable(window_idx):
            for chunk in window_idx():
                plan.count_add(chunk, stream=side)
                del chunk
        else:
            plan.count_add(window_idx, stream=side)
        plan.assign_fill(stream=side)

    def plan_window(self, window_idx, q_source=None):
        """Launch the plan of one window on the side stream.  window_idx: [T, n] int64 on the device, or a callable
        that yields the window's chunks (called under the plan stream; see _unique)."""
        plan, side = self.plan, self.side
        side.wait_stream(S.current_stream(self.dev))          # window_idx may have been produced there
        if self.host_gather:
            import threading
            import time as _time
            assert self._worker is None, "the previous plan was never committed"
            t_launch = _time.perf_counter()
            with S.on_stream(side):
                self._unique(window_idx, side)
                plan.probe(stream=side)
                if self.insert_policy == "fill":
                    self._assign_fill(window_idx, side)
                else:
                    plan.assign(None, seed=self.seed * 1000003 + self.window_no, stream=side)
                if self.victims is not None:
                    plan.victims(self.victims[self._vnext], stream=side, list_only=True)
                lists_ready = S.new_event(self.dev)
                lists_ready.record(side)
            self.planned = None
            self._worker_err = None
            self._exchange = []
            self._worker = threading.Thread(target=self._plan_host_gather, args=(window_idx, lists_ready, t_launch),
                                            daemon=True)
            self._worker.start()
            self.window_no += 1
            return
        with S.on_stream(side):
            self._unique(window_idx, side)
            plan.probe(stream=side)
            if self.insert_policy == "fill":
                self._assign_fill(window_idx, side)
            elif self.parity_rng:
                # Categorical.sample() draws from the torch CPU generator, table by table (main_no_ddp.py:184-185)
                uo, ko, _ = plan.offsets(stream=side)
                T, ways = self.ctx.T, self.ctx.ways
                src = q_source if q_source is not None else (lambda M, w: torch.empty(M, w).exponential_(1) if M else torch.empty(0, w))
                qs = [src(ko[k + 1] - ko[k], ways) for k in range(T)]
                q = torch.cat(qs).contiguous().to(self.dev, non_blocking=False) if ko[T] else None
                self.last_offsets = (uo, ko)
                plan.assign(q if q is not None else torch.empty(1, ways, device=self.dev), stream=side)
            else:
                plan.assign(None, seed=self.seed * 1000003 + self.window_no, stream=side)
            plan.fetch(self.host_ptrs, False, stream=side)
            if self.victims is not None:
                plan.victims(self.victims[self._vnext], stream=side)
            if isinstance(window_idx, torch.Tensor) and window_idx.is_cuda:
                window_idx.record_stream(side)
            self.planned = S.new_event(self.dev)
            self.planned.record(side)
        self.window_no += 1

    def commit(self):
        """At the window boundary: swap the fetched rows in, write the tags, write the evicted rows back."""
        main = S.current_stream(self.dev)
        if self._worker is not None:            # host-gather plan: the background half has to have issued its copies
            self._worker.join()
            self._worker = None
            if self._worker_err is not None:
                raise self._worker_err
        assert self.planned is not None, "plan_window() first"
        main.wait_event(self.planned)
        if self._bd is not None:
            # (the DMA copies' own duration is read from their timing events when `breakdown` is QUERIED, not here: a commit
            #  keeps the host free to issue the next steps -- on a late plan the wait above is the GPU's, not the host's)
            self._breakdown, self._bd = self._bd, None
        # sharded fetch: every rank holds its slice of each list in place; one in-place all-gather per list (RCCL over
        # xGMI) completes them.  Issued here, on the main thread and stream, at the same point of the step sequence on
        # every rank, so it orders with the per-step gradient exchanges on the same communicator.
        for buf, chunk in self._exchange:
            full = buf[:chunk * self.world]
            dist.all_gather_into_tensor(full, full[self.rank * chunk:(self.rank + 1) * chunk], group=self.pg)
        self._exchange = []
        self.plan.commit(stream=main)
        self._commits += 1
        if self.victims is not None:
            # from here on the per-iteration probe serves misses from this window's resident victim rows (the buffer
            # of the previous window is free for the next plan: every probe that read it is ordered before this point)
            self.ctx.bind_victims(self.victims[self._vnext])
            self._vnext ^= 1
        done = S.new_event(self.dev)
        done.record(main)
        with S.on_stream(self.side):
            self.side.wait_event(done)
            # evictions come from rank 0's copy only (main_no_ddp.py:208, 312-315); with private host-table copies every rank
            # applies them to its own
            if (self.rank == 0 or self.replicated_host) and self.write_back:
                self.plan.writeback(self.host_ptrs, self.avg, stream=self.side)
            self.written_back = S.new_event(self.dev)
            self.written_back.record(self.side)
        self.planned = None

    def close(self):
        """Wait for a plan that is still in flight (its background thread runs C++ threads of its own; a process that exits
        under them aborts in teardown).  Call before the process ends; the plan's result is dropped."""
        w, self._worker = self._worker, None
        if w is not None:
            w.join()
        if S.is_hip(self.dev):
            self.side.synchronize()

    def plan_in_flight(self) -> bool:
        """Is the plan of the next window running right now (its kernels / DMA copies / CPU gather)?  bench.py flags the
        roofline-kernel samples taken beside one."""
        if self._worker is not None and self._worker.is_alive():
            return True
        return self.planned is not None and S.is_hip(self.dev) and not self.planned.query()

    def wait_writeback(self):
        """Host-side: the evicted rows are in the host tables (all ranks may read them afterwards)."""
        if self.written_back is not None:
            self.written_back.synchronize()
        if self.multi:
            dist.barrier(group=self.pg)

    def eviction_data(self):
        """(idx, rows) per table, as the reference queues them (main_no_ddp.py:199); synchronises."""
        _, _, wo = self.plan.offsets()
        out = []
        for k in range(self.ctx.T):
            tag = self.plan.ev_tag[wo[k]:wo[k + 1]]
            valid = tag != -1
            out.append((tag[valid], self.plan.stage[wo[k]:wo[k + 1]][valid]))
        return out


class Resolved(NamedTuple):
    """What WindowResolver.batch(j) hands a step: this rank's lookups of batch j as views into the chunk's ring slot, the
    chunk's ready event and where the batch sits (resolver, j) -- the row merge looks AHEAD from there (lookahead()).  step()
    also takes a plain (slots, src, ready) tuple: a batch without a position."""
    slots: torch.Tensor
    src: torch.Tensor
    ready: object
    pos: Optional[tuple] = None


class SortedViews(NamedTuple):
    """WindowResolver.sorted_views(j): the addresses of batch j's sorted lists (keys, meta, once-only flags), the elements
    between two tables' lists, the slice's event and the slice sort's serial."""
    keys: int
    meta: int
    once: int
    stride: int
    event: object
    serial: int


class Handover(NamedTuple):
    """What a step leaves for the next one when it has issued that batch's take: which index tensor it took (ptr, shape), the
    aux region the misses went to, the probe buffers and the event behind the take, and what rode along -- the wait for the
    deferred top-MLP update (chained_top), the batch's slot sort (prepared), and whether the take was ordered behind its
    slice's sort (sorted_ok).  A launch tape keeps stored(); every replay hands it on with handed()."""
    ptr: int
    shape: tuple
    phase: int
    out: tuple
    probed: object
    chained_top: bool = False
    prepared: bool = False
    sorted_ok: bool = False

    def matches(self, lS_i) -> bool:
        """Was this batch's take issued by the previous step?"""
        return self.ptr == lS_i.data_ptr() and self.shape == tuple(lS_i.shape)

    def stored(self) -> "Handover":
        return self._replace(ptr=0)

    def handed(self, next_idx) -> "Handover":
        return self._replace(ptr=next_idx.data_ptr())


class StepPath(NamedTuple):
    """Every decision one training step makes, settled once by TrainEngine._step_path before anything is issued: _wait_slices,
    _fwd_bwd, _issue_resolve and step()'s gradient exchange read them here, a launch tape is keyed by (path, layout) and
    _tape_ptrs names its cells from it.  Two steps with equal paths issue the same calls with the same arguments up to the
    addresses and strides of the layout.  What is fixed when the engine is built -- defer_top, cat, multi, the fused head, the
    layer lists, the loss, quotient-remainder mode, the device -- is a constant and not part of it."""
    B: int
    n: int
    n_bags: int                 # bags per table: B, or B + 1 for squared-off ragged bags
    offsets: bool               # multi-hot bags (lS_o given)
    next_n: int                 # lookups per table of the batch handed over (0: none)
    hit: bool                   # this batch's take was issued by the previous step
    phase: int                  # aux region of the batch being trained
    top_waited: bool            # ... and that take was recorded behind the deferred top-MLP update
    prepared: bool              # ... and sorted this batch's slots right behind itself
    nxt: bool                   # a next batch is handed over
    resolved: bool              # an in-line take reads the window's resolved views (else: a tag probe)
    next_resolved: bool
    two_phase: bool             # the next batch's take at the head of the step, into the other aux region
    chain: bool                 # ... or chained behind this step's embedding update
    side_gather: bool           # the gather on the side stream, beside the bottom MLP
    gather_alone: bool          # B >= gather_alone_min: a two-phase take starts behind the gather
    fused: bool                 # the gather rides in the interaction kernels
    sorted: Optional[int]       # this batch's lists were sorted with its slice: their stride (None: the step sorts)
    once: bool                  # the once-only slots are updated by the interaction backward
    next_sorted: bool
    chain_sort: bool            # the chained take sorts the next batch's slots
    chained_top: bool           # ... and waits for this step's top-MLP update
    next_bufs: int              # the probe buffers a next take writes
    emb_done_seen: bool         # emb_done has been recorded before
    timed: bool                 # the gather's launch carries timing events
    loss_sync: bool
    resolve_cols: Optional[int]  # a look-ahead chunk's resolve is placed behind the interaction forward: its columns
    fwd_marked: bool            # ... and its event completes with the fused forward's launch
    attach: bool                # cross-stream events complete with the launch they follow
    join: str                   # what the training queue waits for at the end: "full", "emb_done" or "none"
    lanes: int                  # issuing threads of a native tape
    wide_gemm: bool
    matmul_precision: str
    lr: float
    lr_embeds: float
    lr_cells: bool = False          # the rate arguments are the engine's two rate cells, not literals
    embed_optimizer: str = "sgd"    # the cache rows' update: "sgd" or "rowwise_adagrad" 
    adagrad_eps: float = 0.0
    dense_optimizer: str = "sgd"    # the MLP parameters' update: "sgd" or "adagrad" 
    dense_adagrad_eps: float = 0.0


EMBED_OPTIMIZERS = ("sgd", "rowwise_adagrad")
DENSE_OPTIMIZERS = ("sgd", "adagrad")


def check_dense_optimizer(dense_optimizer: str, dense_adagrad_eps: float):
    """What the dense optimizer refuses, as one ValueError -- raised by TrainEngine before it touches the GPU and
    turned into the one ERROR: line by the command line: an unknown name, and an eps that is not > 0.  Nothing else: the
    accumulators live beside the parameters, so every world size, either embedding optimizer, quotient-remainder tables and the
    victim write-back are all served."""
    if dense_optimizer not in DENSE_OPTIMIZERS:
        raise ValueError("dense_optimizer=%r: one of %s" % (dense_optimizer, ", ".join(DENSE_OPTIMIZERS)))
    if dense_optimizer == "sgd":
        return
    if not float(dense_adagrad_eps) > 0.0:
        raise ValueError("dense_adagrad_eps=%r: Adagrad divides by sqrt(S) + eps and S starts at zero: eps > 0" % (dense_adagrad_eps,))


def check_embed_optimizer(embed_optimizer: str, adagrad_eps: float, *, world_size: int = 1, qr: bool = False,
                          evict_victim: bool = False):
    """What row-wise Adagrad refuses, as one ValueError -- raised by TrainEngine before it touches the GPU and
    turned into the one ERROR: line by the command line."""
    if embed_optimizer not in EMBED_OPTIMIZERS:
        raise ValueError("embed_optimizer=%r: one of %s" % (embed_optimizer, ", ".join(EMBED_OPTIMIZERS)))
    if embed_optimizer == "sgd":
        return
    if not float(adagrad_eps) > 0.0:
        raise ValueError("adagrad_eps=%r: row-wise Adagrad divides by sqrt(S) + eps and S starts at zero: eps > 0" % (adagrad_eps,))
    if int(world_size) > 1:
        raise ValueError("row-wise Adagrad runs on one rank: how the accumulators of rows that the ranks' row merge averages "
                         "are merged is not defined yet (world_size=%d)" % int(world_size))
    if qr:
        raise ValueError("row-wise Adagrad with quotient-remainder tables is not defined: the remainder tables take plain SGD steps")
    if evict_victim:
        raise ValueError("row-wise Adagrad skips the aux rows of a batch's misses; --evict-victim-cache writes those rows back")


class WindowResolver:
    """The look-ahead window's lookups resolved ONCE (tags only change at a refill, main_no_ddp.py:393-399): tag match,
    ordered miss numbering per batch and the place of every miss in the window's victim rows (cdlrm_window_resolve), in
    chunks of `chunk` batches issued on the engine's prefetch stream ahead of the training position.  `batch(j)` hands the
    engine the views of batch j; what is left per iteration is cdlrm_embbag_take (copy the slot ids, copy the miss rows).
    Create it right after the window's commit(); call ensure() after every step.

    Chunk results live in a fixed RING of three buffers owned by the engine (chunk c in slot c % 3), not in per-chunk
    allocations: the resolve writes them on the prefetch stream while takes read them on the side stream, streams the
    caching allocator knows nothing about -- a block freed on the host while queued takes still read it would be handed
    straight to the next chunk's resolve.  A slot is recycled behind an event recorded on the side stream when the recycling
    resolve is issued, and chunk c is only issued once batch() has been asked for the SECOND batch of chunk c - 2 (the step
    of that chunk's first batch is then on the queues): every take of chunk c - 3, the slot's previous holder, has been
    ISSUED by then, so the event covers them all however far the host runs ahead of the GPU."""

    RING = 3

    def __init__(self, engine: "TrainEngine", window_idx: torch.Tensor, global_batch: int, *, chunk: int = 16):
        self.eng, self.ctx = engine, engine.ctx
        self.idx = window_idx
        self.B = int(global_batch)
        self.lbs = -(-self.B // engine.world)
        self.rank = engine.rank
        # this rank's slice of a global batch (main_no_ddp.py:388-391): the last rank's is shorter when world does not divide B
        self.col0 = min(self.rank * self.lbs, self.B)
        self.width = max(0, min(self.lbs, self.B - self.col0))
        n = int(window_idx.shape[1])
        assert n % self.B == 0, "a window is a whole number of batches"
        self.nb = n // self.B
        self.CH = max(1, int(chunk))
        self.chunks = {}            # chunk number -> (wslots, wsrc, ready event)
        self.done = 0               # chunks issued
        self.maxj = -1              # highest batch handed out by batch()
        key = ("wres", self.CH * self.B)
        if key not in engine._bufs:
            T = self.ctx.T
            engine._bufs[key] = [tuple(torch.empty(T * self.CH * self.B, dtype=torch.int32, device=window_idx.device)
                                       for _ in range(2)) for _ in range(self.RING)]
        self._ring = engine._bufs[key]
        if ("wres_ev",) not in engine._bufs:        # one persistent event per ring slot (a launch tape keeps its handle in a cell)
            evs = [S.new_event(engine.dev) for _ in range(self.RING)]
            if S.is_hip(engine.dev):
                for e in evs:
                    e.record(S.current_stream(engine.dev))
            engine._bufs[("wres_ev",)] = evs
        self._ring_ev = engine._bufs[("wres_ev",)]
        # The embedding backward's slot sort, per CHUNK instead of per step (round 6): a window's slot ids are final once its
        # chunk is resolved, so the lists of SL batches x T tables are sorted by ONE set of launches (four launches for four
        # batches instead of four per batch, 416 instead of 104 sorting workgroups each), on the side stream behind a step's
        # embedding update, batches ahead of their use.  A step whose batch has its lists sorted issues no sort, and its
        # interaction backward finds the once-only flags there (TrainEngine.fuse_once) without waiting for anything: the
        # slice's event is waited for by the stream that runs the batch's take, which the step's gather waits for anyway.
        self.sort_chunks = bool(getattr(engine, "sort_chunks", False)) and S.is_hip(engine.dev) and self.width > 0
        # (short batches: the slice's four runtime calls are host time the issuing thread does not have every other step --
        #  per-rank 1024: 0.1852 ms with slices of 2 against 0.1824 with the per-step sort on the launch tape -- and its kernels
        #  are small: as many batches as make ~16 k lookups per table)
        sl = int(getattr(engine, "sort_slice", 2))
        self.SL = max(1, min(max(sl, (sl * 8192) // max(self.width, 1)), self.CH))
        self.sorted_upto = 0        # batches [0, sorted_upto) of the window have had their slice's turn
        # first batch of a slice whose sort was issued -> (batches in it, the sort's serial: _SORT_SERIAL)
        self._sorted_at = {}
        if self.sort_chunks:
            skey = ("wsorted", self.CH, self.width)
            if skey not in engine._bufs:
                engine._bufs[skey] = [ops.embbag_bwd_sorted(self.ctx, self.CH, self.width, window_idx.device)
                                      for _ in range(self.RING)]
            self._sorted_ring = engine._bufs[skey]
            nsl = -(-self.CH // self.SL)
            ekey = ("wsorted_ev", self.CH, self.SL)
            if ekey not in engine._bufs:
                engine._bufs[ekey] = [[S.new_event(engine.dev) for _ in range(nsl)] for _ in range(self.RING)]
            self._sorted_ev = engine._bufs[ekey]
        self._armed = None          # chunk handed to the engine, to be placed by its next step
        if getattr(engine, "_pending_resolve", None) is not None:
            # a chunk of the window this one replaces that no step has placed: its ring slot belongs to this window now
            engine._pending_resolve, engine.mark_next = None, False
        self._started = False       # the first chunks of a window are issued at once (no step of the window is in flight)
        self.ensure(self.CH + 2)
        self._started = True

    def _long_batch(self) -> bool:
        """Long local batches on a HIP device with an engine that can place a resolve inside its step (TrainEngine.
        place_resolve_min): a chunk's resolve issued at once lands on whatever the training queue runs then -- one interaction
        forward in sixteen took 60 us instead of 23 -- so the step places it behind its interaction forward."""
        eng = self.eng
        return (hasattr(eng, "_issue_resolve") and S.is_hip(eng.dev)
                and (self.width >= getattr(eng, "place_resolve_min", 1 << 62) or not eng._side_gather(self.width)))

    def _prepare(self, c: int):
        ctx = self.ctx
        self.chunks.pop(c - self.RING, None)
        last = getattr(self.eng, "_last_sort_ev", None)
        if last is not None and c < self.RING:
            # The slice sorts read the ring slots' slot ids on TrainEngine.sort_st (the prefetch stream, where this resolve runs
            # behind them in order; tools/race_check.py also puts them on a stream of their own).  Inside a window the slot's
            # previous holder is chunk c - 3, whose slices were all waited for by the takes of its batches, long ago; the first
            # chunks of a window recycle slots of the PREVIOUS window, which may have been left early -- a sort whose batches
            # were never trained has no take behind it: this resolve (prefetch stream, issued after this call) is ordered behind
            # every sort issued so far, on whichever stream
            self.eng.pref.wait_event(last)
        b0, b1 = c * self.CH, min(self.nb, (c + 1) * self.CH)
        cols = self.idx[:, b0 * self.B:b1 * self.B]
        w = int(cols.shape[1])
        ring_ws, ring_src = self._ring[c % self.RING]
        ws, wsrc = ring_ws[:ctx.T * w].view(ctx.T, w), ring_src[:ctx.T * w].view(ctx.T, w)
        ev = self._ring_ev[c % self.RING]
        self.chunks[c] = (ws, wsrc, ev)
        return dict(cols=cols, lbs=self.lbs, ws=ws, wsrc=wsrc, ev=ev, B=self.B, first=(c == 0))

    def ensure(self, upto_batch: int, urgent: bool = False):
        """Issue the resolve of every chunk that holds a batch < upto_batch (prefetch stream; no host wait).  Called after every
        step.  At long batches a chunk that falls due is handed to the engine, whose NEXT step issues it behind its interaction
        forward (TrainEngine._issue_resolve); urgent (batch() needs the chunk now), the first chunks of a window, short batches
        and engines without that hook: at once."""
        eng = self.eng
        if self._armed is not None:
            if eng._pending_resolve is None:
                self._armed = None                      # the step issued since has placed it
            elif urgent and self._armed * self.CH < int(upto_batch):
                self._armed = None
                eng.flush_pending_resolve()             # needed before a step could place it
        nchunks = -(-self.nb // self.CH)
        want = min(nchunks, -(-min(int(upto_batch), self.nb) // self.CH))
        while self.done < want and self._armed is None:
            c = self.done
            if c >= self.RING and self.maxj < (c - 2) * self.CH + 1:
                break               # the slot's previous chunk may still have takes to issue: a later ensure() / batch() issues it
            self.done += 1
            pr = self._prepare(c)
            if not urgent and c > 0 and self._started and self._long_batch() and eng._pending_resolve is None:
                eng._pending_resolve, eng.mark_next = pr, True
                self._armed = c
                break               # one chunk per step
            if hasattr(eng, "_issue_resolve"):
                eng._issue_resolve(pr, lambda fn, *a: fn(*a), S.current_stream(eng.dev), placed=None)
            else:                   # (host-logic tests: a bare engine stand-in)
                ops.window_resolve(self.ctx, pr["cols"], self.lbs, pr["ws"], pr["wsrc"], stream=eng.pref, batch_len=self.B)
        if not urgent:
            # (callers pass the batch just trained + CH + 2) the slice that holds the batch after next: the next step issues that
            # batch's take, and the take's stream waits for the slice
            self.ensure_sorted(int(upto_batch) - self.CH - 2 + 3)

    def _chunk_nb(self, c: int) -> int:
        return min(self.nb, (c + 1) * self.CH) - c * self.CH

    def ensure_sorted(self, upto_batch: int):
        """Issue the slot sort of every slice that holds a batch < upto_batch (side stream, behind whatever the last step put
        there; no host wait).  A slice of a chunk whose resolve has not been ISSUED yet stays for a later call."""
        if not self.sort_chunks:
            return
        eng = self.eng
        upto = min(int(upto_batch), self.nb)
        while self.sorted_upto < upto:
            b0 = self.sorted_upto
            c = b0 // self.CH
            if c >= self.done or c not in self.chunks:
                break
            if self._armed is not None and c >= self._armed and getattr(eng, "_pending_resolve", None) is not None:
                break               # handed to the engine, not yet issued
            ws, _, ev = self.chunks[c]
            nbc = self._chunk_nb(c)
            j0 = b0 - c * self.CH
            cnt = min(self.SL, nbc - j0)
            if getattr(eng, "sort_chunks", True):       # (switched per slice by tools/ab_step.py)
                st = getattr(eng, "sort_st", eng.pref)     # (host-logic stand-ins: the prefetch stream)
                st.wait_event(ev)                       # the chunk's resolve (prefetch stream)
                # the ring slot's previous lists were read by embedding updates three chunks back; what the wait really picks is
                # WHERE in the step the sort runs: behind the last step's embedding update = in that step's tail
                if eng._emb_done is not None:
                    st.wait_event(eng._emb_done)
                if getattr(eng, "sort_delay", 0):       # (tools/race_check.py: a late sort shows a consumer that is not ordered behind it)
                    with torch.cuda.stream(st):
                        torch.cuda._sleep(int(eng.sort_delay))
                ops.embbag_bwd_prepare_window(self.ctx, ws[:, self.col0:], self.B, nbc, self.width,
                                              self._sorted_ring[c % self.RING], stream=st, j0=j0, count=cnt)
                sev = self._sorted_ev[c % self.RING][j0 // self.SL]
                sev.record(st)
                eng._last_sort_ev = sev
                self._sorted_at[b0] = (cnt, next(_SORT_SERIAL))
            self.sorted_upto = b0 + cnt
            self._sorted_at.pop(b0 - self.RING * self.CH, None)

    def sorted_views(self, j: int) -> Optional[SortedViews]:
        """Batch j's sorted lists -- or None: not sorted (yet)."""
        if not self.sort_chunks or j >= self.sorted_upto:
            return None
        c = j // self.CH
        nbc = self._chunk_nb(c)
        jl = j - c * self.CH
        at = self._sorted_at.get(j - jl % self.SL)
        if at is None:
            return None
        k, m, o = ops.embbag_bwd_sorted_views(self.ctx, self._sorted_ring[c % self.RING], nbc, self.width, jl)
        return SortedViews(k, m, o, nbc * self.width, self._sorted_ev[c % self.RING][jl // self.SL], at[1])

    def batch(self, j: int) -> Resolved:
        """This rank's lookups of batch j of the window."""
        c = j // self.CH
        self.maxj = max(self.maxj, j)
        self.ensure(j + 1, urgent=True)
        ws, wsrc, ev = self.chunks[c]
        col = (j - c * self.CH) * self.B + self.col0
        if c >= 2 and (c - 2) in self.chunks:       # chunks far behind the training position are not needed any more
            del self.chunks[c - 2]
        return Resolved(ws[:, col:col + self.width], wsrc[:, col:col + self.width], ev, (self, j))

    def lookahead(self, j: int, kmax: int):
        """[(k, slot ids of GLOBAL batch j + k -- every rank's lookups --, ready event)] for k = 1, 2, ... while the batch
        belongs to this window and its chunk's resolve has been issued (at most kmax): the rows the next steps will use."""
        out = []
        eng = self.eng
        for k in range(1, int(kmax) + 1):
            b = j + k
            if b >= self.nb:
                break
            c = b // self.CH
            if c >= self.done or c not in self.chunks:
                break
            if self._armed is not None and c >= self._armed and getattr(eng, "_pending_resolve", None) is not None:
                break               # handed to the engine, not yet issued
            ws, _, ev = self.chunks[c]
            col = (b - c * self.CH) * self.B
            out.append((k, ws[:, col:col + self.B], ev))
        return out


# ---- the touched-row merge in deadline order -----------------------------------------------------------------------------
# broadcast_and_aggregate (main_no_ddp.py:250-292) replaces every row any rank touched since the last merge by its mean
# (max, sum) over the ranks, at step j, before step j + 1 runs.  What step j + 1 can observe of that is the rows IT uses;
# a row nobody uses before step j + d may be merged any time before step j + d -- it does not change in between on any
# rank.  The window's resolved slot ids (WindowResolver.lookahead: every rank's lookups of the next batches) say which
# rows the next K steps use: the merge's row list is sorted by the first batch that needs a row (classes: batch 1, 2, 3-4,
# 5-8, 9-16, 17-32, 33-64, later = "cold", due at batch K + 1) and exchanged in that order on the exchange stream -- gather, all-
# reduce, scatter per chunk -- a few chunks per step, while the training steps run; a step waits for the chunk that holds
# the last row it needs.  At c3 (100 steps x 8192 lookups x 26 tables, Zipf 1.05: 1.86 M rows, 0.95 GB) the next batch
# needs 2.3 % of the merge's rows, the next 16 batches 13 %.  Same values as the merge in one piece: every rank builds the
# same list from the same flags and the same window, and a row's gather reads what the one-piece merge would have read.
#
# Every rank has to cut the exchange into the same pieces in the same order (a mismatch is a hang, not a failed assert): the
# arithmetic that decides the pieces is MergeSchedule + merge_pieces, no torch and no streams (tests/test_merge_schedule_host.py);
# MergePump holds the buffers and the in-flight state and issues what the schedule says.
MERGE_CLASS_FIRST = (1, 2, 3, 5, 9, 17, 33)     # first batch (after the merge step) of each deadline class; then: cold
MERGE_LOOKAHEAD = 64                            # batches ahead the classes reach (the resolver decides how many are known)


class MergeSchedule(NamedTuple):
    """One merge's deadlines.  off: the class offsets into the merge's row list (cdlrm_agg_split: len(MERGE_CLASS_FIRST) + 2
    entries, rows of class c at [off[c], off[c + 1]), the cold class last); K: how many batches ahead were known; U: rows in
    the merge; budget: rows issued per step beyond what the next step needs."""
    off: tuple
    K: int
    U: int
    budget: int

    def need(self, d: int) -> int:
        """Rows that have to have landed before the d-th step after the merge."""
        if d > self.K:
            return self.U
        need = 0
        for c, f in enumerate(MERGE_CLASS_FIRST):
            if f <= d:
                need = self.off[c + 1]
        return need

    def target(self, d_next: int, issued: int, everything: bool = False) -> int:
        """Rows to have issued once a step is done: what the NEXT step (the d_next-th after the merge) needs, plus the budget."""
        return self.U if everything else max(self.need(d_next), min(self.U, issued + self.budget))


def merge_pieces(issued: int, target: int, chunk: int):
    """The (lo, hi) cuts that take a merge from `issued` rows to `target`, at most `chunk` rows each."""
    ch, cuts = max(1, int(chunk)), []
    while issued < target:
        cuts.append((issued, min(target, issued + ch)))
        issued = cuts[-1][1]
    return cuts


class MergePump:
    """The touched-row merge of a multi-rank engine (TrainEngine.merge): its buffers -- allocated at the first merge, grown by
    doubling, none in a steady-state merge -- and the one merge that may be on its way across steps.  Everything here is
    COLLECTIVE: every rank makes the same calls at the same steps."""

    def __init__(self, engine: "TrainEngine"):
        self.eng = engine
        self.list_rows = None       # the union's sorted row list; with it: count, count_host, flags, counted, xbuf, tier
        self._clear()

    def _clear(self):
        self.sched = None           # MergeSchedule of the merge in flight
        self.rows = self.buf = self.rop = self.ready = self.rs = None
        self.scale = 1.0
        self.j0 = self.step0 = 0    # the merge step's batch in its window (rs), and its engine iteration
        self.issued = self.waited = 0
        self.chunks = []            # (hi, event) per piece issued

    @property
    def pending(self) -> bool:
        return self.sched is not None

    def _alloc(self):
        if self.list_rows is None:
            dev, n = self.eng.dev, self.eng.ctx.total_rows
            self.list_rows = torch.empty(n, dtype=torch.int64, device=dev)
            self.count = torch.zeros(1, dtype=torch.int64, device=dev)
            self.count_host = S.pinned(torch.zeros(1, dtype=torch.int64), dev)
            self.flags = torch.zeros(n, dtype=torch.uint8, device=dev)
            self.counted = S.new_event(dev)
            self.xbuf = self.tier = None

    def _list(self, flags) -> int:
        """flags -> sorted row list (device) and its length on the host.  The host waits for THIS copy only (an event
        behind the compaction), not for the stream: kernels queued behind it keep the GPU busy meanwhile."""
        ops.agg_compact(self.eng.ctx, flags, self.list_rows, self.count)
        self.count_host.copy_(self.count, non_blocking=True)
        self.counted.record(S.current_stream(self.eng.dev))
        self.counted.synchronize()
        return int(self.count_host[0])

    def _buffer(self, U: int) -> torch.Tensor:
        """[>= U, D] exchange buffer, kept between merges (grown by doubling: no allocation in a steady-state merge)."""
        if self.xbuf is None or self.xbuf.shape[0] < U:
            cap = 1 << max(12, (U - 1).bit_length())
            self.xbuf = torch.empty(min(cap, self.eng.ctx.total_rows), self.eng.D, dtype=torch.float32, device=self.eng.dev)
        return self.xbuf[:U]

    def sync_to_rank0(self):
        """The reference refills rank 0's cache and then broadcasts EVERY cache table from rank 0
        (main_no_ddp.py:318-319), which also overwrites whatever the other ranks changed since the last
        table-agg merge.  Same result without moving 10.9 GB: only the rows some rank touched since that merge can
        differ, so broadcast exactly those (union of the touched flags), leaving the flags set for the next merge."""
        eng = self.eng
        self.drain()                # the refill that follows reads and evicts cache rows: the last merge lands first
        self._alloc()
        self.flags.copy_(eng.cg.touched)
        dist.all_reduce(self.flags, op=dist.ReduceOp.MAX, group=eng.pg)
        U = self._list(self.flags)
        if U == 0:
            return
        buf = self._buffer(U)
        ops.agg_gather(eng.ctx, self.list_rows, self.count, 1.0, buf, U)
        dist.broadcast(buf, src=0, group=eng.pg)
        ops.agg_scatter(eng.ctx, self.list_rows, self.count, buf, U)

    def aggregate(self, pos, it: int):
        """The merge of engine iteration `it`, whose batch is pos = (resolver, batch number) of its window (None: unknown).
        Slot ids are global, so the union of touched rows is an all-reduce(MAX) of the flag bytes (the reference all-gathers
        the slot lists and takes torch.unique per table); the rows then travel as ONE compacted [U, D] buffer: in deadline
        order over the next steps (lazy_merge, _start), or at once, in chunks -- while chunk i is reduced over xGMI on the
        exchange stream, chunk i+1 is gathered and chunk i-1 scattered back on the main stream.  The host waits only for
        the row count (and the class offsets)."""
        eng = self.eng
        ctx, main, comm = eng.ctx, S.current_stream(eng.dev), eng.comm
        touched = eng.cg.touched
        dist.all_reduce(touched, op=dist.ReduceOp.MAX, group=eng.pg)
        self._alloc()
        U = self._list(touched)                       # consumes (clears) the flags
        if U == 0:
            return
        buf = self._buffer(U)
        if eng.agg_op == "mean":
            scale, rop = float(eng.world), dist.ReduceOp.SUM
        elif eng.agg_op == "sum":
            scale, rop = 1.0, dist.ReduceOp.SUM
        elif eng.agg_op == "max":
            scale, rop = 1.0, dist.ReduceOp.MAX
        else:
            raise ValueError(eng.agg_op)
        if eng.lazy_merge and self._start(pos, it, U, buf, scale, rop):
            return
        rows, count, ch = self.list_rows, self.count, eng.agg_chunk_rows
        nch = (U + ch - 1) // ch
        if nch == 1 or not S.is_hip(eng.dev):
            ops.agg_gather(ctx, rows, count, scale, buf, U)
            dist.all_reduce(buf, op=rop, group=eng.pg)
            ops.agg_scatter(ctx, rows, count, buf, U)
            return
        gathered = [S.new_event(eng.dev) for _ in range(nch)]
        reduced = [S.new_event(eng.dev) for _ in range(nch)]

        def gather(i):
            lo, hi = i * ch, min(U, (i + 1) * ch)
            ops.agg_gather(ctx, rows[lo:], count, scale, buf[lo:hi], hi - lo, first=lo)
            gathered[i].record(main)

        def reduce(i):
            lo, hi = i * ch, min(U, (i + 1) * ch)
            with S.on_stream(comm):
                comm.wait_event(gathered[i])
                dist.all_reduce(buf[lo:hi], op=rop, group=eng.pg)
                reduced[i].record(comm)

        def scatter(i):
            lo, hi = i * ch, min(U, (i + 1) * ch)
            main.wait_event(reduced[i])
            ops.agg_scatter(ctx, rows[lo:], count, buf[lo:hi], hi - lo, first=lo)

        gather(0)
        for i in range(nch):
            reduce(i)
            if i + 1 < nch:
                gather(i + 1)
            if i >= 1:
                scatter(i - 1)
        scatter(nch - 1)

    def _start(self, pos, it, U, buf, scale, rop) -> bool:
        """Sort the merge's rows by their deadline and begin the exchange; False: nothing known about the next batches."""
        if pos is None:
            return False
        rs, j = pos
        la = rs.lookahead(j, MERGE_LOOKAHEAD)
        if not la:
            return False            # nothing known about the next batch (end of the window): the merge in one piece
        eng = self.eng
        ctx, main = eng.ctx, S.current_stream(eng.dev)
        first = MERGE_CLASS_FIRST
        C = len(first) + 1
        K = la[-1][0]
        if self.tier is None:
            self.tier = (torch.empty(ctx.total_rows, dtype=torch.uint8, device=eng.dev),
                         torch.empty(ctx.total_rows, dtype=torch.int64, device=eng.dev),
                         torch.zeros(C + 1, dtype=torch.int64, device=eng.dev),
                         S.pinned(torch.zeros(C + 1, dtype=torch.int64), eng.dev))
        tier, rows_sorted, off_dev, off_host = self.tier
        tier.fill_(C - 1)
        seen = set()
        for k, ws, ev in la:
            if id(ev) not in seen:
                main.wait_event(ev)
                seen.add(id(ev))
        for c in reversed(range(C - 1)):        # latest deadline first: the earliest class that names a row wins
            hi = first[c + 1] if c + 1 < len(first) else MERGE_LOOKAHEAD + 1
            for k, ws, ev in la:
                if first[c] <= k < hi:
                    ops.agg_mark_tier(ctx, ws, c, tier)
        ops.agg_split(ctx, self.list_rows, U, tier, C, rows_sorted, off_dev)
        eng._events["tier_marked"].record(main)
        off_host.copy_(off_dev, non_blocking=True)
        self.counted.record(main)
        self.counted.synchronize()
        ready = S.new_event(eng.dev)
        ready.record(main)
        # (the budget cuts the exchange into pieces: it has to be the same number on every rank -- the resolver's lbs =
        #  ceil(B / world), not this rank's slice width, which is shorter on the last rank when world does not divide B)
        budget = int(eng.merge_budget_rows)
        if eng.merge_budget_auto:
            budget = max(budget, int(rs.lbs) * eng.T)
        sched = MergeSchedule(tuple(int(x) for x in off_host.tolist()), K, U, budget)
        self.start(sched, rows_sorted, buf, scale, rop, ready, rs, j, it)
        return True

    def start(self, sched: MergeSchedule, rows, buf, scale, rop, ready, rs, j0: int, it: int):
        """A merge is on its way from here: rows [U] in deadline order, buf [U, D]; `ready`: rows and buf may be read."""
        self._clear()
        self.sched, self.rows, self.buf, self.scale, self.rop, self.ready = sched, rows, buf, scale, rop, ready
        self.rs, self.j0, self.step0 = rs, j0, it
        self.after_step(it)

    def issue(self, lo: int, hi: int):
        """Rows [lo, hi) of the merge in flight on the exchange stream; returns the event behind their scatter."""
        eng, comm = self.eng, self.eng.comm
        with S.on_stream(comm):
            if not self.chunks:
                comm.wait_event(self.ready)
            ops.agg_gather(eng.ctx, self.rows[lo:], self.count, self.scale, self.buf[lo:hi], hi - lo, first=lo)
            dist.all_reduce(self.buf[lo:hi], op=self.rop, group=eng.pg)
            ops.agg_scatter(eng.ctx, self.rows[lo:], self.count, self.buf[lo:hi], hi - lo, first=lo)
            ev = S.new_event(eng.dev)
            ev.record(comm)
        return ev

    def before_step(self, pos, it: int):
        """In front of engine iteration `it`, whose batch is `pos`: the rows of a pending merge that this step uses have landed.
        The deadlines were computed for the batches FOLLOWING the merge step in its window: a step that is not the expected
        next batch of that window (another resolver, a jump) gets the whole merge first."""
        if self.sched is None:
            return
        if pos is None or pos[0] is not self.rs or pos[1] != self.j0 + (it - self.step0):
            self.drain()
        else:
            self.wait(it)

    def after_step(self, it: int, everything: bool = False):
        """Issue the pieces the NEXT step needs, plus the budget's share of the rest (everything: all of it)."""
        s = self.sched
        if s is None:
            return
        target = s.target(it + 1 - self.step0, self.issued, everything)
        for lo, hi in merge_pieces(self.issued, target, self.eng.agg_chunk_rows):
            self.chunks.append((hi, self.issue(lo, hi)))
            self.issued = hi

    def wait(self, it: int, everything: bool = False):
        """The training (and the side) stream wait for the piece that holds the last row iteration `it` needs."""
        s, eng = self.sched, self.eng
        need = s.U if everything else s.need(it - self.step0)
        if need > self.waited:
            assert self.issued >= need, "merge rows this step needs were never issued"
            for hi, ev in self.chunks:
                if hi >= need:
                    S.current_stream(eng.dev).wait_event(ev)
                    eng.side.wait_event(ev)
                    self.waited = hi
                    break
        if self.waited >= s.U:
            self._clear()

    def drain(self):
        """Land every row of the merge in flight (nothing to do without one)."""
        if self.sched is not None:
            self.after_step(self.step0, everything=True)
            self.wait(self.step0, everything=True)
            self._clear()


class TrainEngine:
    def __init__(self, cache_group: Embedding_Table_Cache_Group, dlrm: DLRM_Net, host_tables: Embedding_Table_Group,
                 *, lr: float, lr_embeds: float, world_size: int = 1, rank: int = 0, table_agg_freq: int = 1,
                 table_agg_op: str = "mean", process_group=None, loss: str = "bce", loss_weights=(1.0, 1.0),
                 defer_top_update: bool = False, force_collectives: bool = False, matmul_precision: str = "fp32",
                 embed_optimizer: str = "sgd", adagrad_eps: float = 1e-10, dense_optimizer: str = "sgd",
                 dense_adagrad_eps: float = 1e-10):
        """loss / loss_weights: --loss-function / --loss-weights (main_no_ddp.py:364-372); the --loss-threshold clamp
        is read from `dlrm.loss_threshold`.
        defer_top_update: the top MLP's weight gradients, their all-reduce and their SGD update leave the critical
        path -- they run on a side stream beside the interaction backward, the bottom MLP's backward and the HEAD of the
        next step (gather, bottom MLP forward), which only waits for them in front of its interaction.  Same values,
        different schedule; readers of the top MLP's weights outside step()/evaluate() call finish() first.
        force_collectives: run the multi-rank control flow (gradient all-reduce, touched-row flags and merge, exchange
        stream) at world_size 1 as well: over a 1-rank RCCL communicator every collective of the N-rank step executes and is
        the identity, so the result must equal the one-rank fast path bit for bit (tests/test_rccl_one_rank.py).
        matmul_precision: "fp32" (default: the reference's arithmetic) or "bf16" -- every MLP layer with K >= 32 and N >= 32
        runs its forward, dgrad and weight-gradient GEMMs on the bf16 matrix cores (operands rounded once to bf16 inside the
        kernels, fp32 accumulation, storage and epilogues: DESIGN.md section 4, "bf16 mode") -- or "bf16x3": the same layers
        with every operand split into two bf16 values and three exact products per product, near-fp32 results (DESIGN.md
        section 4.2).  A plain attribute: set it between steps and the next step / evaluate() follows it.
        embed_optimizer: "sgd" (default: the reference's sparse SGD on the cache rows) or "rowwise_adagrad" with adagrad_eps
        (DESIGN.md section 4.5): one fp32 accumulator per table row in `emb_state`, indexed by table index; one rank, plain
        tables, no --evict-victim-cache.
        dense_optimizer: "sgd" (default: the reference's optim.SGD on the MLP parameters) or "adagrad" with dense_adagrad_eps
        (DESIGN.md section 4.6): element-wise Adagrad, one fp32 accumulator per parameter in `dense_state` (param_flat's layout),
        stepped where the SGD step runs; every world size.  A plain attribute like matmul_precision."""
        check_embed_optimizer(embed_optimizer, adagrad_eps, world_size=world_size,
                              qr=getattr(cache_group, "qr", None) is not None)
        check_dense_optimizer(dense_optimizer, dense_adagrad_eps)
        self.embed_optimizer, self.adagrad_eps = embed_optimizer, float(adagrad_eps)
        self.dense_optimizer, self.dense_adagrad_eps = dense_optimizer, float(dense_adagrad_eps)
        self.cg, self.dlrm, self.host = cache_group, dlrm, host_tables
        self.ctx = cache_group.ctx
        self.dev = cache_group.weight.device
        self.lr, self.lr_embeds = float(lr), float(lr_embeds)
        # A learning-rate schedule: lr / lr_embeds stay the BASE rates and part of the step's path; the factor
        # is not.  Until a factor is first set every rate argument is the literal base rate; from then on (lr_cells) it is one of
        # these two shared cells, which step() sets to the effective rates and a launch tape reads at every replay.
        self.lr_cells = False
        self._lr_factor = 1.0
        self._lr_cell, self._lr_embeds_cell = RateCell(self.lr), RateCell(self.lr_embeds)
        self.world, self.rank = int(world_size), int(rank)
        self.multi = self.world > 1 or bool(force_collectives)      # the multi-rank control flow is on
        self.agg_freq, self.agg_op = int(table_agg_freq), table_agg_op
        self.pg = process_group
        self.T, self.D = self.ctx.T, self.ctx.D
        self.F = self.T + 1
        self.itself = bool(dlrm.arch_interaction_itself)
        assert dlrm.arch_interaction_op in ("dot", "cat"), "--arch-interaction-op: dot or cat (model_no_ddp.py:272-304)"
        self.cat = dlrm.arch_interaction_op == "cat"
        self.loss_kind = ops.LOSS[loss]
        self.loss_weights = (float(loss_weights[0]), float(loss_weights[1]))
        thr = float(getattr(dlrm, "loss_threshold", 0.0) or 0.0)
        self.loss_threshold = thr if 0.0 < thr < 1.0 else 0.0
        self.defer_top = bool(defer_top_update)
        self.matmul_precision = matmul_precision
        self.bot = dlrm._acts(dlrm.bot_l, dlrm.sigmoid_bot)
        self.top = dlrm._acts(dlrm.top_l, dlrm.sigmoid_top)
        self._flatten_params()
        self.ctx.bind_host_tables(host_tables.device_pointers())
        self._bufs = {}
        # quotient-remainder mode: the cache holds quotient rows keyed by q -- everything above the gather runs
        # unchanged on the q stream --, the remainder tables Wr [T, c, D] live whole in HBM and are composed with the rows by
        # cdlrm_qr_cached_fwd / _bwd.  None: plain tables, no Wr, no r columns, the launch sequence of a plain run.
        self.qr = getattr(cache_group, "qr", None)
        self.Wr = self._r = None
        if self.qr is not None:
            self._init_qr(host_tables)
        # row-wise Adagrad's accumulators: one fp32 per TABLE row, table k's n_k from state_base[k] on; zero at the start, in HBM
        # for the whole run.  Plain SGD allocates nothing
        # (embed_optimizer is a plain attribute like matmul_precision -- tools/ab_step.py switches it between rounds --: a step
        #  that finds it set without a state allocates one, _step_path)
        self.emb_state = self.state_base = None
        if self.embed_optimizer != "sgd":
            self._alloc_emb_state()
        # the dense Adagrad's accumulators: param_flat's layout, zero at the start; allocated in that mode only, here or by the
        # first step that finds the attribute set (_step_path)
        self.dense_state = None
        if self.dense_optimizer != "sgd":
            self._alloc_dense_state()
        self.iter = 0
        self.comm = S.new_stream(self.dev) if self.multi else None
        self.side = S.new_stream(self.dev)
        self.pref = S.new_stream(self.dev)          # next batch's tag probe + aux-row fill
        # rows per chunk of the touched-row merge (32 MB at D = 128: large enough for xGMI bandwidth, small enough that
        # the gather of chunk i+1 hides under the reduction of chunk i)
        self.agg_chunk_rows = 1 << 16
        # The merge of step j is due, row by row, before the first later step that USES the row (on any rank) -- the look-ahead
        # window knows those steps --, so only the rows the very next batch needs are exchanged at step j; the others follow in
        # deadline order over the next steps, `merge_budget_rows` per step beyond what the next step needs (MergePump).
        self.lazy_merge = True
        # per step, beyond what the next step needs: max(this, the rank's lookups per step) rows -- 32 MB at c3's per-rank batch,
        # 109 MB at c5's: about one step's length of xGMI time at ring rates, so that the next step's gradient exchange (same
        # communicator stream) finds the stream free; a c3 merge drains in ~29 steps, a c5 merge in ~41 (look-ahead: 34-65)
        self.merge_budget_rows = 1 << 16
        self.merge_budget_auto = True           # (tests switch the per-step-lookups floor off to keep rows on their way)
        self.merge = MergePump(self) if self.multi else None
        self._pref = None
        self._phase = 0                             # aux region of the batch being trained
        self._emb_done = None
        ne = lambda: S.new_event(self.dev)
        self._events = dict(probed={k: ne() for k in range(4)}, probed_inline=ne(), gathered=ne(), interacted=ne(),
                            emb_done=ne(), wgrad_done=ne(), top_dz=ne(), top_updated=ne(), fwd_mark=ne(), res_slot=ne(),
                            tier_marked=ne())
        if S.is_hip(self.dev):
            # torch creates the HIP event at the first record: give every engine event its handle now (a launch tape stores
            # handles; a wait recorded before the event's first real record would otherwise push that tape back to Python)
            cur = S.current_stream(self.dev)
            for e in list(self._events["probed"].values()) + [v for k, v in self._events.items() if k != "probed"]:
                e.record(cur)
        self._head_scratch = ops.head_scratch(self.dev)
        # running print statistics [correct predictions, loss * mbs] summed over steps in float64 on the device
        # (main_no_ddp.py:427-433 keeps them on the host and synchronises twice per step for it): the head's finish launch adds
        # to them; readers call finish() first and zero them when they start a new interval
        self.stat_acc = torch.zeros(2, dtype=torch.float64, device=self.dev)
        self.loss_sync = True                   # see step()
        # output head in one launch (last layer + loss + its input gradient) when the last top layer is 1-wide + sigmoid
        l_last, a_last = self.top[-1]
        self.fused_head = l_last.out_features == 1 and a_last == 2
        # top-MLP weight gradients at long local batches: the SAME stream as the prefetch (their work never overlaps in
        # time: probe/fill right after the gather, weight gradients late in the backward) -- four streams in all
        # (main, side, pref, the window plan's), one per default hardware queue
        self.wst = self.pref
        # measured (c3 shapes): the split loses ~3 % at B <= 2048 (two more launches on a latency-bound step), gains
        # 8 % at 4096 (0.580 -> 0.534 ms) and at 8192 (0.853 -> 0.782 ms)
        self.split_wgrad_min = 2049
        # Local batches below this take the TWO-AUX-REGION schedule (the next batch's take on the prefetch stream at the head of
        # the step, into the other aux region; its slot sort at the head of the next step; stand-alone gather, where there is one,
        # on the side stream beside the bottom MLP's forward), from it on the CHAINED take (one aux region; take and sort of the
        # next batch behind this batch's embedding update, the gather / fused interaction forward alone on the training queue).
        # Decided by samples/s on the fused build (round 5, tools/ab_step.py, one box, six rounds each, three sessions): at 8192
        # the two-region schedule is 0.8-1.3 % faster (0.5588 / 0.5591 / 0.5593 against 0.5662 / 0.5636 / 0.5651 ms; the driver's
        # 20 steps 0.5737 against 0.5797, a whole window 0.5865 against 0.5906) although the fused kernel -- the HBM-roofline
        # kernel -- then runs beside the next batch's take and this batch's sort: 28.3 us in the step against 23.9 alone (0.57
        # against 0.68 of 8 TB/s; bench.py reports both, roofline.frac and roofline.alone).  At 65536 the chained take stays
        # (3.718 against 3.741 ms), 4096 is a tie, 2048 / 1024 keep two regions (0.2422 / 0.2433, 0.1798 / 0.1845 the other way).
        self.gather_alone_min = 16384
        # The top MLP's forward and its input-gradient chain run with no other GEMM beside them in every schedule of the step
        # (the weight gradients start behind the chain): these launches carry CDLRM_GEMM_ALONE and, where their 128x128 tiles
        # fill the chip (local batch 8192 x 512-wide layers: 256 tiles on 256 CUs; c5), take the one-workgroup-per-CU kernel
        # (csrc/gemm_wide.h).  The bottom MLP's backward runs beside the weight gradients and never does (round 6: with the hint
        # on every GEMM the c3 step took 0.5790 ms against 0.5580 without, with it on these 0.5562).  The bottom MLP's forward
        # carries it too (it runs at the end of the previous step, beside the next batch's take and slot sort: small kernels
        # that fit beside a wide workgroup): its 512 -> 256 layer on 64x128 tiles, c3 0.5495 against 0.5522 ms
        self.wide_gemm = True
        # the SGD step of the slots a batch reads ONCE rides in the fused interaction backward (cdlrm_gather_interact_bwd_sgd):
        # those lookups' gradient rows are never written or read back, the sorted path is left with the repeated slots.
        # Bit-identical (a single addend has no order); costs the training queue one wait for the slot sort
        self.fuse_once = True
        # the slot sort of the embedding backward per look-ahead chunk slice instead of per step (WindowResolver.ensure_sorted);
        # steps of batches without sorted lists (no resolver, multi-hot bags) sort their own
        self.sort_chunks = True
        # batches per slice.  tools/ab_step.py, one box, c3, against the per-step sort: slices of 1 / 2 / 4 batches -2.7 / -3.3 /
        # -2.7 %: what pays is the sort OFF the queues a step waits for and the folded once-only update it allows, not the
        # batching -- a long slice is a long visitor in one step's tail
        self.sort_slice = 2
        # The stream of the slice sorts: issued behind a step, they follow that step's top-MLP weight gradients (and its
        # `top_updated` record) on the prefetch stream and run in the step's tail; the next take on that stream is behind them in
        # order, the one after needs them.  (The side stream and a stream of their own measured no better: DESIGN.md, "Which
        # stream".)
        self.sort_st = self.pref
        self._cur_sorted = self._next_sorted = None
        self._next_waited = self._cur_waited = 0    # serial of the last slice each take path waited for (_wait_slices)
        self.slice_wait = True      # (False: tools/race_check.py --negative -- nobody waits for the slices: the check must notice)
        self._last_sort_ev = None
        # --evict-victim-cache (main_no_ddp.py:96, parsed and unused by the reference): behind every step's embedding update
        # the trained aux rows of the batch's misses go back to their host rows and to their copies among the window's victim
        # rows (ops.victim_writeback).  One rank only; the step then runs un-pipelined (no take of the next batch ahead of
        # this batch's write-back, no launch tape) -- an optional mode, not the timed path.  Run() also plans the next window
        # at the boundary instead of in the background: the plan's row gather has to see the window's last write-back.
        self.evict_victim = False
        self._vwb_work = {}
        self._gslot = None
        self._res = self._next_res = None
        self._tapes = {}
        self.tape_fallbacks = []                # why a recorded step could not become a native tape (should stay empty)
        # schedule knobs (attributes, not environment switches: tests/test_engine_parity.py runs each of them both ways)
        self.use_tape = S.is_hip(self.dev)      # replay recorded launch sequences (_step_taped)
        self.native_tape = True                 # ... from the C side (csrc/tape.hip) instead of from Python
        # ... in lanes: the training queue's calls by this thread, each side queue's by a helper thread of the library.  At a
        # per-rank batch of 1024 the thread that issues a step's ~45 runtime calls, not the GPU, sets the step time
        self.tape_lanes = 3
        # ... below this local batch only: from it on the GPU needs several times the host's issue time per step and a
        # single issuing thread keeps the program order of the tape (A / B at c3: 0.6331 one lane, 0.6396 three)
        self.tape_lanes_below = 4096
        # cross-stream events of the step complete WITH the kernel they follow (attached to its launch) instead of being
        # recorded behind it: no marker packet, no bubble on the training queue
        self.attach_events = True
        # Criteo layout + dot interaction: the gather IS the interaction's operand load (cdlrm_gather_interact_fwd / _bwd) -- the
        # [B, T, D] block between cached EmbeddingBag and interact_features is neither written nor read back (c3: 109 MB + 113 MB
        # per step), the backward reads the rows again from the cache, in front of the batch's embedding update.  Bit-identical
        # to the two operators (False: gather + interaction as two launches; multi-hot bags and "cat" always take those).
        self.fuse_gather = True
        # (Where the sort of a batch's own slot ids and the top MLP's weight gradients start, the fold of the top-update wait
        #  and the take schedules were measured as knobs, rounds 1-6, and the losers removed: DESIGN_HISTORY.md.)
        # WindowResolver hands the NEXT step a look-ahead chunk to resolve (`_pending_resolve`, taken when `mark_next` is set): the
        # step issues it on the prefetch stream right behind its interaction forward -- in front of its own weight gradients on that
        # stream --, so the resolve (random 128-B tag reads) runs beside the top MLP's GEMMs, which leave HBM idle, instead of
        # behind the weight gradients at the end of the step, where it lands on the next step's gather (the roofline kernel)
        # local batches from this size on PLACE the resolve (either take schedule); below it a chunk is small and is issued at once
        self.place_resolve_min = 8192
        self.mark_next = False
        self._mark_this = False
        self._pending_resolve = None
        self._step_key = None                   # (StepPath, layout) of the last step

    # ---- quotient-remainder mode -------------------------------------------------------------------------------------
    def _init_qr(self, host_tables):
        q = self.qr
        c = int(q["c"])
        assert host_tables.qr_layout() == q, "the cache group's quotient-remainder layout is not the host group's"
        if q["operation"] not in ops.QR_OPS:
            raise ValueError("--qr-operation=%s changes the row width: the cached path composes mult / add" % q["operation"])
        if not 2 <= c <= 16:
            raise ValueError("--qr-collisions=%d: the cached path takes 2 .. 16" % c)
        if not ops.qr_cached_shape_ok(self.D, c):
            raise ValueError("embedding dim %d x %d collisions: the backward's remainder accumulators exceed 64 KB of LDS"
                             % (self.D, c))
        self.qr_op = ops.QR_OPS[q["operation"]]
        self.qr_coll = torch.tensor(q["collisions"], dtype=torch.int32, device=self.dev)
        self.qr_rows = torch.tensor(q["rows"], dtype=torch.int64, device=self.dev)
        self.Wr = torch.zeros(self.T, c, self.D, dtype=torch.float32, device=self.dev)
        self.load_wr(host_tables)

    def load_wr(self, host_tables):
        """Wr <- the host group's weight_r (construction, --load-model)."""
        for k, E in enumerate(host_tables.emb_l):
            if self.qr["collisions"][k]:
                self.Wr[k].copy_(E.weight_r.data)

    def flush_wr(self, host_tables):
        """The host group's weight_r <- Wr: call it wherever the cache is flushed (beside Embedding_Table_Cache_Group.flush_to_host;
        Run does at --save-model).  Not collective: it waits for this rank's last embedding update only."""
        if self._emb_done is not None:
            S.current_stream(self.dev).wait_event(self._emb_done)
        wr = self.Wr.cpu()
        for k, E in enumerate(host_tables.emb_l):
            if self.qr["collisions"][k]:
                E.weight_r.data.copy_(wr[k])

    # ---- row-wise Adagrad's state ---------------------------------------------------------------------------------------
    def _alloc_emb_state(self):
        check_embed_optimizer(self.embed_optimizer, self.adagrad_eps, world_size=self.world, qr=self.qr is not None,
                              evict_victim=bool(getattr(self, "evict_victim", False)))
        rows = [int(n) for n in self.ctx.table_rows]
        self._state_off = [sum(rows[:k]) for k in range(len(rows) + 1)]
        self.emb_state = torch.zeros(self._state_off[-1], dtype=torch.float32, device=self.dev)
        self.state_base = torch.tensor(self._state_off[:-1], dtype=torch.int64, device=self.dev)

    def emb_state_views(self):
        """Table k's accumulators: a view of n_k elements of emb_state."""
        return [self.emb_state[a:b] for a, b in zip(self._state_off[:-1], self._state_off[1:])]

    def emb_state_to_host(self):
        """[T] CPU tensors, table k's n_k accumulators (--save-model); waits for this rank's last embedding update."""
        if self._emb_done is not None:
            S.current_stream(self.dev).wait_event(self._emb_done)
        return [v.cpu() for v in self.emb_state_views()]

    def load_emb_state(self, per_table):
        """emb_state <- a list of per-table accumulators (--load-model); None: zeros."""
        if self._emb_done is not None:
            S.current_stream(self.dev).wait_event(self._emb_done)
        if per_table is None:
            self.emb_state.zero_()
            return
        views = self.emb_state_views()
        if len(per_table) != len(views):
            raise ValueError("emb_state: %d tables, the model has %d" % (len(per_table), len(views)))
        for k, (v, h) in enumerate(zip(views, per_table)):
            h = torch.as_tensor(h, dtype=torch.float32).reshape(-1)
            if h.numel() != v.numel():
                raise ValueError("emb_state[%d]: %d accumulators, the table has %d rows" % (k, h.numel(), v.numel()))
            v.copy_(h)

    # ---- the dense Adagrad's state ----------------------------------------------------------------------------------------
    def _alloc_dense_state(self):
        check_dense_optimizer(self.dense_optimizer, self.dense_adagrad_eps)
        self.dense_state = torch.zeros_like(self.param_flat)
        base = self.param_flat.data_ptr()
        es = self.param_flat.element_size()

        def beside(t):          # the accumulators of a parameter view: the same elements of dense_state
            off = (t.data_ptr() - base) // es
            return self.dense_state[off:off + t.numel()].view(t.shape)

        # per layer, as self.W / l.bias.data name the parameters (the padded weight storage included)
        self.SW = {l: beside(W) for l, W in self.W.items()}
        self.Sb = {l: beside(l.bias.data) for l in self.W}

    # ---- the learning-rate factor -----------------------------------------------------------------------------------------
    def set_lr_factor(self, f: float):
        """Scale both rates of the steps that follow by f (cdlrm_amd.lr_schedule): the rates handed to the library become
        effective_rate(lr, f) and effective_rate(lr_embeds, f).  The first call switches the engine's rate arguments from
        literals to cells for good -- one re-recording per control path --; no later call, whatever its value, changes a path."""
        f = float(f)
        if not (f >= 0.0 and f != float("inf")):
            raise ValueError("lr factor %r: a finite number >= 0" % (f,))
        self._lr_factor = f
        self.lr_cells = True        # (step() writes the cells: lr / lr_embeds may still be assigned before it)

    lr_factor = property(lambda self: self._lr_factor, set_lr_factor)

    def effective_rates(self):
        """(dense, embedding) rates of the next step as float32: the base rates without a factor."""
        if not self.lr_cells:
            return np.float32(self.lr), np.float32(self.lr_embeds)
        return effective_rate(self.lr, self._lr_factor), effective_rate(self.lr_embeds, self._lr_factor)

    def _set_rate_cells(self):
        self._lr_cell.value, self._lr_embeds_cell.value = self.effective_rates()

    def _rate(self, path: StepPath):
        """The dense rate argument of this step's calls, in a tape or outside one."""
        return self._lr_cell if path.lr_cells else self.lr

    def _rate_embeds(self, path: StepPath):
        return self._lr_embeds_cell if path.lr_cells else self.lr_embeds

    def _dense_step(self, path: StepPath):
        """The dense optimizer's step over the whole flat buffer, on the current stream."""
        if path.dense_optimizer == "sgd":
            ops.sgd_step(self.param_flat, self.grad_flat, self._rate(path))
        else:
            ops.dense_opt_step(self.param_flat, self.grad_flat, self.dense_state, self._rate(path), *self._dense_opt(path))

    def _dense_step2(self, path: StepPath, rng, **kw):
        """... over one sub-network's weights and biases (rng_bot / rng_top); kw: stream."""
        if path.dense_optimizer == "sgd":
            ops.sgd_step2(self.param_flat, self.grad_flat, *rng, self._rate(path), **kw)
        else:
            ops.dense_opt_step2(self.param_flat, self.grad_flat, self.dense_state, *rng, self._rate(path), *self._dense_opt(path), **kw)

    def _dense_opt(self, path: StepPath):
        """ops.mlp_wgrad's `opt` for this step."""
        return (path.dense_optimizer, path.dense_adagrad_eps)

    def dense_state_to_host(self):
        """One flat CPU tensor, param_flat's layout (--save-model); behind a deferred top-MLP update."""
        if self.defer_top and self.iter > 0:
            S.current_stream(self.dev).wait_event(self._events["top_updated"])
        return self.dense_state.cpu()

    def load_dense_state(self, flat):
        """dense_state <- a flat tensor of param_flat's layout (--load-model); None: zeros."""
        if self.defer_top and self.iter > 0:
            S.current_stream(self.dev).wait_event(self._events["top_updated"])
        if self.dense_state is None:
            self._alloc_dense_state()
        if flat is None:
            self.dense_state.zero_()
            return
        h = torch.as_tensor(flat, dtype=torch.float32).reshape(-1)
        if h.numel() != self.dense_state.numel():
            raise ValueError("dense_state: %d accumulators, the MLPs have %d parameters" % (h.numel(), self.dense_state.numel()))
        self.dense_state.copy_(h)

    def qr_split(self, idx, q=None, r=None, stream=None):
        """idx [T, n] -> (q, r) (ops.qr_split; q=idx splits a window rectangle in place): what plan_window / WindowResolver /
        step() / evaluate() take in this mode."""
        return ops.qr_split(self.ctx, idx, self.qr_coll, self.qr_rows, q, r, stream=stream)

    def _qr_work(self, n):
        key = ("qr", n)
        if key not in self._bufs:
            self._bufs[key] = ops.qr_cached_bwd_work(self.ctx, n, int(self.qr["c"]))
        return self._bufs[key]

    def _merge_wr(self):
        """Wr over the ranks with --table-agg-op, as oracle.table_aggregate merges a table every rank touched all rows of."""
        if self.agg_op == "mean":
            ops.scale_div(self.Wr.view(-1), float(self.world))
            dist.all_reduce(self.Wr, op=dist.ReduceOp.SUM, group=self.pg)
        elif self.agg_op == "sum":
            dist.all_reduce(self.Wr, op=dist.ReduceOp.SUM, group=self.pg)
        elif self.agg_op == "max":
            dist.all_reduce(self.Wr, op=dist.ReduceOp.MAX, group=self.pg)
        else:
            raise ValueError(self.agg_op)

    # all Linear weights in one flat buffer (one all-reduce, main_no_ddp.py:234-247), biases behind them
    def _flatten_params(self):
        """All Linear weights in one flat buffer, biases behind them.  The first top-MLP layer reads the interaction
        output R, whose width D + npairs (479 at c3) is not a multiple of 4: its weight is stored with the row pitch
        rounded up to 4 (zero pad column, R gets a matching zero column) so that layer runs on the 16-byte-load GEMM
        path; `layer.weight` stays a [out, in] view of that storage."""
        lin = _linears(self.dlrm.bot_l) + _linears(self.dlrm.top_l)
        top0 = _linears(self.dlrm.top_l)[0]
        kp = {l: ((l.in_features + 3) // 4 * 4 if l is top0 else l.in_features) for l in lin}
        nw = sum(l.out_features * kp[l] for l in lin)
        nb = sum(l.bias.numel() for l in lin)
        self.param_flat = torch.zeros(nw + nb, dtype=torch.float32, device=self.dev)
        self.grad_flat = torch.zeros(nw + nb, dtype=torch.float32, device=self.dev)
        self.n_weight = nw
        nbot = len(_linears(self.dlrm.bot_l))
        nw_bot = sum(l.out_features * kp[l] for l in lin[:nbot])
        nb_bot = sum(l.bias.numel() for l in lin[:nbot])
        # (weights offset, count, biases offset, count) of the bottom / top MLP inside the flat buffers
        self.rng_bot = (0, nw_bot, nw, nb_bot)
        self.rng_top = (nw_bot, nw - nw_bot, nw + nb_bot, nb - nb_bot)
        # the weight-gradient ranges the two exchanges at world > 1 carry (top MLP's, bottom MLP's)
        self._grad_views = (self.grad_flat[nw_bot:nw], self.grad_flat[0:nw_bot])
        off_w, off_b = 0, nw
        self.W, self.gW, self.gb = {}, {}, {}
        for l in lin:
            n = l.out_features * kp[l]
            Wp = self.param_flat[off_w:off_w + n].view(l.out_features, kp[l])
            Wp[:, :l.in_features].copy_(l.weight.data)
            self.W[l] = Wp                                          # what the kernels see: [out, kp] contiguous
            l.weight.data = Wp[:, :l.in_features]
            self.gW[l] = self.grad_flat[off_w:off_w + n].view(l.out_features, kp[l])
            l.weight.grad = self.gW[l][:, :l.in_features]
            off_w += n
            m = l.bias.numel()
            self.param_flat[off_b:off_b + m].copy_(l.bias.data)
            l.bias.data = self.param_flat[off_b:off_b + m]
            self.gb[l] = self.grad_flat[off_b:off_b + m]
            l.bias.grad = self.gb[l]
            off_b += m
        self.r_width = kp[top0]

    def _issue_resolve(self, pr, rec, main, placed: Optional[StepPath]):
        """One look-ahead chunk's resolve on the prefetch stream (WindowResolver prepares `pr`).  placed: the path of the step
        that issues it behind its interaction forward (an event recorded on the training queue: one marker packet per chunk, i.e.
        per 16 steps); None: issued at once."""
        pst, ev = self.pref, self._events
        if placed is not None:
            if not placed.fwd_marked:            # (else: fwd_mark completes with the interaction forward's launch)
                rec(ev["fwd_mark"].record, main)
            rec(pst.wait_event, ev["fwd_mark"])
        elif pr["first"]:
            pst.wait_stream(main)               # the commit (tags, victims) is on the main stream
        # the ring slot's previous chunk (this window's c - 3, or a chunk of the previous window): its takes are all issued, on
        # the side stream (chained / in-line takes) or on this very stream (two-phase takes: in order)
        rec(ev["res_slot"].record, self.side)
        rec(pst.wait_event, ev["res_slot"])
        if self.multi:
            # ... and the row merge's deadline pass (main stream, MergePump.aggregate) has read the slot ids it wanted from it
            rec(pst.wait_event, ev["tier_marked"])
        ops.window_resolve(self.ctx, pr["cols"], pr["lbs"], pr["ws"], pr["wsrc"], stream=pst, batch_len=pr["B"])
        if S.is_hip(self.dev):
            ops.event_record(pr["ev"], pst)       # (a library call: on a launch tape the slot's event handle is a cell)
        else:
            pr["ev"].record(pst)

    def flush_pending_resolve(self):
        """Issue a handed-over chunk at once (its batches are needed before a step could place it)."""
        pr, self._pending_resolve = self._pending_resolve, None
        self.mark_next = False
        if pr is not None:
            self._issue_resolve(pr, lambda fn, *a: fn(*a), S.current_stream(self.dev), placed=None)

    def _fused_gather(self, lS_o) -> bool:
        """This step's gather rides in the interaction kernels (fuse_gather)."""
        # (quotient-remainder mode composes the rows with Wr in the stand-alone gather: the fused kernels are a later step)
        return bool(self.fuse_gather and lS_o is None and not self.cat and S.is_hip(self.dev) and self.qr is None
                    and ops.gather_interact_supported(self.ctx))

    def _side_gather(self, B: int) -> bool:
        """Short local batches run the gather on the side stream (see _fwd_bwd)."""
        return B < self.gather_alone_min and not (self.defer_top and self.cat)

    def _chain(self, B: int, next_idx, lS_o) -> bool:
        """Long batches on the window-resident probe: the next batch's take rides behind this step's embedding update on
        the side stream (see _fwd_bwd)."""
        return not self._side_gather(B) and next_idx is not None and self._next_res is not None and lS_o is None

    def _step_path(self, X, lS_i, lS_o, next_idx) -> StepPath:
        """The decisions of the step step() is about to issue (StepPath), from the batch, the hand-over of the previous step, the
        resolver's views and the schedule knobs.  The one place that evaluates them."""
        B, n = X.shape[0], lS_i.shape[1]
        if self.embed_optimizer != "sgd" and self.emb_state is None:
            self._alloc_emb_state()
        if self.dense_optimizer != "sgd" and self.dense_state is None:
            self._alloc_dense_state()
        pf = self._pref
        hit = pf is not None and pf.matches(lS_i)
        phase = pf.phase if hit else self._phase
        nxt = next_idx is not None
        side_gather = self._side_gather(B)
        # Long batches with the window-resident probe: the next batch's take costs ~10 us stand-alone, so it no longer needs
        # a stream and an aux region of its own (that pipeline hid 250 us of PCIe reads).  It follows this step's embedding
        # update in order on the side stream, and ONE event recorded there -- after the take and, on one rank, after the
        # deferred top-MLP update -- is all the next step's gather waits for: the main queue carries one wait per step
        # instead of three (probe, top update, embedding update) plus a record, each a 6-8 us bubble (measured).
        chain = self._chain(B, next_idx, lS_o)
        two_phase = self.ctx.aux_phases >= 2 and not chain
        fused = self._fused_gather(lS_o)
        # this batch's slot lists were sorted with its look-ahead chunk (WindowResolver.ensure_sorted): no sort in the step, and
        # the once-only slots can be updated by the interaction backward (it reads the sort's flags)
        # (the flags of a batch's OWN sort would cost the training queue a wait for the side stream in front of the interaction
        #  backward: measured 21 us, three times what the folding saves)
        sv = self._cur_sorted if (lS_o is None and n == B) else None
        attach = bool(self.attach_events and S.is_hip(self.dev))
        # the next step's gather runs on the side stream, in order behind this embedding update, and its probe waits for emb_done
        # on its own stream -- nothing on the main stream reads the cache rows before the next full join (window boundary, row
        # merge, evaluate(), finish()), so the main queue is spared one more wait (6-8 us bubble)
        spared = nxt and side_gather and two_phase
        if self.multi:          # step() joins AFTER it has issued the gradient all-reduce: the exchange overlaps the embedding update
            join = "none" if (self.defer_top and spared) else "emb_done"
        elif not nxt:
            join = "full"
        elif chain or spared:   # (chain: the next gather waits for the take's event, recorded behind emb_done)
            join = "none"
        else:                   # cache rows are updated; the prefetched probe keeps running
            join = "emb_done"
        pr = self._pending_resolve if self._mark_this else None
        return StepPath(
            B=B, n=n, n_bags=B if lS_o is None else lS_o.shape[1], offsets=lS_o is not None,
            next_n=next_idx.shape[1] if nxt else 0, hit=hit, phase=phase, top_waited=bool(hit and pf.chained_top),
            prepared=bool(hit and pf.prepared), nxt=nxt, resolved=self._res is not None and lS_o is None,
            next_resolved=self._next_res is not None, two_phase=two_phase, chain=chain, side_gather=side_gather,
            gather_alone=B >= self.gather_alone_min, fused=fused, sorted=None if sv is None else sv.stride,
            # (row-wise Adagrad: the once-only fold is an SGD step -- the sorted apply takes every slot)
            once=bool(self.fuse_once and fused and sv is not None and self.embed_optimizer == "sgd"), next_sorted=self._next_sorted is not None,
            chain_sort=chain and self._next_sorted is None, chained_top=chain and self.defer_top and not self.multi,
            next_bufs=(1 - phase) if two_phase else 2 + (self.iter & 1), emb_done_seen=self._emb_done is not None,
            timed=self._gslot is not None, loss_sync=self.loss_sync, resolve_cols=None if pr is None else int(pr["cols"].shape[1]),
            fwd_marked=bool(pr is not None and attach and fused), attach=attach, join=join,
            lanes=self.tape_lanes if B < self.tape_lanes_below else 1, wide_gemm=bool(self.wide_gemm),
            matmul_precision=self.matmul_precision, lr=self.lr, lr_embeds=self.lr_embeds,
            embed_optimizer=self.embed_optimizer, adagrad_eps=self.adagrad_eps if self.embed_optimizer != "sgd" else 0.0,
            dense_optimizer=self.dense_optimizer,
            dense_adagrad_eps=self.dense_adagrad_eps if self.dense_optimizer != "sgd" else 0.0, lr_cells=bool(self.lr_cells))

    def _take(self, idx, res, phase: int, which, st):
        """A batch's (slots, miss_pos, miss_count) into the probe buffers `which`, misses into aux region `phase`, on stream st:
        its take when the window resolved it (res: WindowResolver.batch), else its tag probe."""
        out = self._probe_bufs(idx.shape[1], which)
        if res is None:
            return ops.embbag_probe(self.ctx, idx, stream=st, aux_phase=phase, out=out)
        ops.embbag_take(self.ctx, idx, res.slots, res.src, out[0], aux_phase=phase, stream=st)
        return out

    def _hand_over(self, path: StepPath, next_idx, phase: int, st):
        """The next batch's take (or tag probe) on stream st, misses into aux region `phase`; returns what the next step needs
        of it.  The caller records `probed` behind whatever else it puts between the take and the next step."""
        out = self._take(next_idx, self._next_res, phase, path.next_bufs, st)
        return Handover(ptr=next_idx.data_ptr(), shape=tuple(next_idx.shape), phase=phase, out=(out[0], out[1], out[2]),
                        probed=self._events["probed"][path.next_bufs], chained_top=path.chained_top, prepared=path.chain_sort,
                        sorted_ok=path.next_sorted)

    def _wait_slices(self, path: StepPath, cur, nxt):
        """The streams of this batch's and the next batch's takes wait for their slices' sorts (cur / nxt: sorted_views() of
        the two batches, or None) -- once per slice sort, told apart by its serial: the slice events are a ring, and an event
        that comes round again has been recorded by another sort."""
        if not self.slice_wait:
            return
        if nxt is not None and nxt.serial != self._next_waited:
            # the next batch's take (two aux regions: prefetch stream; chained / single region: side stream) waits for its
            # slice's sort: this step's successor -- gather, interaction backward (the once-only flags), embedding update -- is
            # ordered behind that take.  (Not on both: with two aux regions the `gathered` record THIS step's fused forward
            # waits for sits on the side stream -- a wait for a sort that is still running would hold the training queue.)
            (self.pref if path.two_phase else self.side).wait_event(nxt.event)
            self._next_waited = nxt.serial
        if cur is not None and cur.serial != self._cur_waited:
            # this batch's take, if no earlier step issued it, runs in line on the side stream; its gather follows that stream
            self.side.wait_event(cur.event)
            self._cur_waited = cur.serial

    def _reduce_avg(self) -> bool:
        """grad /= W followed by all-reduce(SUM) (main_no_ddp.py:239-244) as ONE all-reduce(AVG): on RCCL, for a
        power-of-two world size -- dividing by 2, 4, 8 is exact in fp32 and commutes with every rounding of the sum, so the
        result is bit-identical while one kernel launch per exchange disappears.  Other sizes / backends (gloo in the
        tests) keep the reference's two steps."""
        r = getattr(self, "_avg_ok", None)
        if r is None:
            W = self.world
            r = (W & (W - 1)) == 0 and dist.get_backend(self.pg) == "nccl"
            self._avg_ok = r
        return r

    def _mm(self, l) -> dict:
        """The extra keyword of layer l's linear_fwd / linear_bwd calls: {} in fp32 mode (the calls stay what they were),
        {"bf16": True} in bf16 mode and {"precision": "bf16x3"} in bf16x3 mode for a layer the shape rule admits
        (ops.bf16_eligible)."""
        if self.matmul_precision == "fp32":
            return {}
        assert self.matmul_precision in ("bf16", "bf16x3"), \
            "matmul_precision: 'fp32', 'bf16' or 'bf16x3', not %r" % (self.matmul_precision,)
        if not ops.bf16_eligible(l.out_features, self.W[l].shape[1]):
            return {}
        return {"bf16": True} if self.matmul_precision == "bf16" else {"precision": self.matmul_precision}

    def _wplans(self, buf):
        """(whole-network plan, (bottom plan, top plan) or None) of the weight gradients at the current matmul precision: the
        fp32 plans of _buffers, or bf16 / bf16x3 plans built on first use."""
        if self.matmul_precision != "fp32":
            self._mm(self.bot[0][0])            # validates the attribute
        key = "wgrad_" + self.matmul_precision
        if key not in buf:
            buf[key] = self._build_wplans(buf, self.matmul_precision)
        split = buf[key][1]
        if self.dense_state is not None and split is not None and not hasattr(split[0], "S_w"):
            # the accumulators beside the parameters _build_wplans set; once per plan (a tape holds the arrays' addresses)
            layers, nb = buf["wgrad_args"][2], len(self.bot)
            split[0].set_state([self.SW[l] for l in layers[:nb]], [self.Sb[l] for l in layers[:nb]])
            split[1].set_state([self.SW[l] for l in layers[nb:]], [self.Sb[l] for l in layers[nb:]])
        return buf[key]

    def _build_wplans(self, buf, precision):
        """(whole, split) for _wplans.  split: (bottom plan, top plan), each with scratch of its own and the layers' parameters
        set, where the step takes the two sub-networks' weight gradients apart -- None otherwise.  whole: all layers in one call;
        in fp32 on the scratch the layers' backward calls use (lin_work), in bf16 / bf16x3 on scratch of its own and so only where
        the step has no split plans (None otherwise)."""
        xs, dzs, layers, B, split = buf["wgrad_args"]
        gw = [self.gW[l] for l in layers]
        gb = [self.gb[l] for l in layers]
        kw = {} if precision == "fp32" else {"precision": precision}       # (fp32: the calls stay what they were, as _mm)

        def plan(lo, hi, work=None):
            ls = layers[lo:hi]
            if work is None:
                work = ops.mlp_wgrad_work(B, [l.out_features for l in ls], [self.W[l].shape[1] for l in ls], self.dev, **kw)
            return ops.WgradPlan(xs[lo:hi], dzs[lo:hi], gw[lo:hi], gb[lo:hi], work, **kw)

        fp32 = precision == "fp32"
        whole = plan(0, len(layers), buf["lin_work"] if fp32 else None) if fp32 or not split else None
        if not split:
            return whole, None
        nb = len(self.bot)
        parts = (plan(0, nb), plan(nb, len(layers)))
        # one rank: nothing sits between a sub-network's weight gradients and its SGD step, so the step rides in the
        # gradients' reduction pass (cdlrm_mlp_wgrad_sgd) -- one launch less per sub-network and step
        parts[0].set_params([self.W[l] for l in layers[:nb]], [l.bias.data for l in layers[:nb]])
        parts[1].set_params([self.W[l] for l in layers[nb:]], [l.bias.data for l in layers[nb:]])
        return whole, parts

    def _buffers(self, B):
        if B in self._bufs:
            return self._bufs[B]
        dev, D, F = self.dev, self.D, self.F
        f32 = torch.float32
        npairs = F * (F + 1) // 2 if self.itself else F * (F - 1) // 2
        b = dict()
        # one scratch row behind the batch in the feature blocks: the extra bag of squared-off ragged inputs
        # (square_bags) pools into it; its gradient row stays zero
        if self.cat:
            # "cat" interaction (model_no_ddp.py:297-299): R = cat([x] + ly) IS the feature block the bottom MLP and
            # the gather write into -- no interaction kernel, no copy
            assert self.r_width >= F * D
            b["R"] = torch.zeros(B + 1, self.r_width, dtype=f32, device=dev)[:B]
            b["dR"] = torch.zeros(B + 1, self.r_width, dtype=f32, device=dev)[:B]
            b["feat"] = b["R"].as_strided((B, F, D), (self.r_width, D, 1))
            b["dfeat"] = b["dR"].as_strided((B, F, D), (self.r_width, D, 1))
        else:
            b["feat"] = torch.zeros(B + 1, F, D, dtype=f32, device=dev)[:B]
            b["dfeat"] = torch.zeros(B + 1, F, D, dtype=f32, device=dev)[:B]
            assert self.r_width >= D + npairs
            b["R"] = torch.zeros(B, self.r_width, dtype=f32, device=dev)      # pad column (if any) stays zero
            b["dR"] = torch.zeros(B, self.r_width, dtype=f32, device=dev)
        b["Zc"] = torch.empty(B, 1, dtype=f32, device=dev) if self.loss_threshold > 0.0 else None
        # activations / gradients of the hidden layers
        b["bot_y"] = [torch.empty(B, l.out_features, dtype=f32, device=dev) for l, _ in self.bot[:-1]]
        b["bot_dy"] = [torch.empty(B, l.out_features, dtype=f32, device=dev) for l, _ in self.bot[:-1]]
        b["top_y"] = [torch.empty(B, l.out_features, dtype=f32, device=dev) for l, _ in self.top]
        b["top_dy"] = [torch.empty(B, l.out_features, dtype=f32, device=dev) for l, _ in self.top]
        b["loss"] = torch.zeros(65, dtype=f32, device=dev)
        work = 0
        for l, _ in self.bot + self.top:
            work = max(work, ops.linear_bwd_work(B, l.out_features, self.W[l].shape[1], dev).numel())
        work = max(work, ops.mlp_wgrad_work(B, [l.out_features for l, _ in self.bot + self.top],
                                            [self.W[l].shape[1] for l, _ in self.bot + self.top], dev).numel())
        b["lin_work"] = torch.empty(work, dtype=torch.uint8, device=dev)
        # weight/bias gradients of all layers are taken at the end of the backward, from the pre-activation
        # gradients the dgrad chain leaves in these buffers (one grouped launch at small batches)
        layers = [l for l, _ in self.bot + self.top]
        x0 = torch.empty(B, self.W[layers[0]].shape[1], dtype=f32, device=dev)   # stand-in: re-pointed at X every step
        xs = [x0] + b["bot_y"] + [b["R"]] + b["top_y"][:-1]
        dzs = b["bot_dy"] + [b["dfeat"][:, 0, :]] + b["top_dy"]
        # long local batches: the top MLP's weight gradients run on their own stream beside the interaction backward
        # and the bottom MLP's backward -- (bottom plan, top plan) instead of one plan of all layers
        split = bool(self.defer_top or (S.is_hip(dev) and B >= self.split_wgrad_min))
        b["wgrad_args"] = (xs, dzs, layers, B, split)
        b["wgrad_fp32"] = self._build_wplans(b, "fp32")
        self._bufs[B] = b
        return b

    def _probe_bufs(self, n, which):
        """(slots, miss_pos, miss_count) of one pipeline stage, allocated once: they are written and read on side
        streams, where the caching allocator's per-stream reuse rules would not protect per-call temporaries."""
        key = ("probe", n, which)
        if key not in self._bufs:
            i32 = torch.int32
            self._bufs[key] = (torch.empty(self.T, n, dtype=i32, device=self.dev),
                               torch.empty(self.T, n, dtype=i32, device=self.dev),
                               torch.empty(self.T, dtype=i32, device=self.dev))
        return self._bufs[key]

    def _emb_work(self, n):
        key = ("emb", n)
        if key not in self._bufs:
            self._bufs[key] = ops.embbag_bwd_work(self.ctx, n, self.dev)
        return self._bufs[key]

    # ----------------------------------------------------------------------------------------------
    def sync_touched_to_rank0(self):
        """Rank 0's copy of every row some rank touched since the last merge, on all ranks (MergePump.sync_to_rank0): call it
        on every rank in front of a window's refill.  Nothing to do on one rank."""
        if self.merge is not None:
            self.merge.sync_to_rank0()

    def table_aggregate(self):
        """broadcast_and_aggregate (main_no_ddp.py:250-292): average the rows any rank touched since the last merge
        (MergePump.aggregate).  A merge that is still on its way lands first (a merge period shorter than the look-ahead), then
        the remainder tables of quotient-remainder mode are merged whole, one small all-reduce."""
        if self.merge is None:
            self.cg.touched.zero_()
            return
        self.merge.drain()
        if self.Wr is not None:
            self._merge_wr()
        self.merge.aggregate(self._res.pos if self._res is not None else None, self.iter)

    def _exchange(self, g, stream=None):
        """aggregate_gradients (main_no_ddp.py:239-244) on the current stream: g /= world, all-reduce(SUM) -- or the one
        all-reduce(AVG) where that gives the same bits (_reduce_avg).  stream: passed on to the scaling launch."""
        if self._reduce_avg():
            dist.all_reduce(g, op=dist.ReduceOp.AVG, group=self.pg)
            return
        kw = {} if stream is None else {"stream": stream}
        ops.scale_div(g, float(self.world), **kw)       # layer.weight.grad /= world (:239); biases untouched
        dist.all_reduce(g, op=dist.ReduceOp.SUM, group=self.pg)

    def step(self, X: torch.Tensor, lS_i: torch.Tensor, T: torch.Tensor, lS_o: Optional[torch.Tensor] = None,
             j: Optional[int] = None, gather_events: Optional[list] = None, next_idx: Optional[torch.Tensor] = None,
             res=None, next_res=None, loss_sync: bool = True, r: Optional[torch.Tensor] = None):
        """One training iteration on this rank's slice (next_idx: the NEXT batch's indices, if it belongs to the same
        window: its tag probe and aux fill are then issued behind this step's embedding backward).  X [B, m_den] fp32, lS_i [T, n] int64, T [B, 1] fp32, all
        on the device; lS_o None = Criteo layout (one lookup per bag), else int64 [T, B] offsets -- or [T, B + 1] from
        square_bags() for ragged multi-hot tables; j = batch number inside the epoch (table-agg schedule).
        res / next_res: WindowResolver.batch(j) / .batch(j + 1) -- the window-resident probe: this batch's (the next
        batch's) slot ids and miss sources were resolved once for the whole window, the per-step tag probe shrinks to
        cdlrm_embbag_take.
        loss_sync=False: the loss buffer is completed OFF the training queue -- the head kernel leaves per-workgroup partial
        sums, and the one-workgroup launch that adds them up (and accumulates `stat_acc`) runs on the side stream in front of
        the embedding backward instead of holding the training queue for ~6 us; the returned buffer and `stat_acc` are then
        valid after finish() (bench.py, Run), not right behind step() on the current stream.
        r: quotient-remainder mode only -- lS_i (and next_idx, the window, the resolver's chunks) are QUOTIENTS and r uint8
        [T, n] holds this batch's remainders (qr_split; columns of a window's r rectangle are fine).
        Returns the device loss buffer (element 0 = the loss, 1 = correct predictions, 2 = loss * batch)."""
        B, n = X.shape[0], lS_i.shape[1]
        if self.qr is not None:
            if lS_o is not None:
                raise ValueError("quotient-remainder mode takes one lookup per bag (the operator pools before it combines)")
            assert r is not None and r.dtype == torch.uint8 and tuple(r.shape) == (self.T, n) and r.stride(1) == 1
        else:
            assert r is None, "r columns belong to quotient-remainder mode"
        self._r = r
        if res is not None and not isinstance(res, Resolved):
            res = Resolved(*res)
        if next_res is not None and not isinstance(next_res, Resolved):
            next_res = Resolved(*next_res)
        if self.evict_victim:
            check_embed_optimizer(self.embed_optimizer, self.adagrad_eps, evict_victim=True)
            assert not self.multi, "--evict-victim-cache is defined for one rank (every rank would write its own misses' rows)"
            next_idx = next_res = None          # the next batch's take follows this batch's write-back
        self.loss_sync = bool(loss_sync) or not self.fused_head
        self._mark_this = bool(self.mark_next and self._pending_resolve is not None and lS_o is None)
        self.mark_next = False
        self._res, self._next_res = res, (next_res if next_idx is not None else None)
        if lS_o is not None:
            # [T, B + 1]: squared-off ragged bags (square_bags, BagWindow.rank_batch).  Their padding lookups go through the
            # embedding backward like any lookup and set the touched flag of their slot, which decides what the row merge
            # averages at world > 1.  They repeat the first index of THIS rank's lookups of the table: a slot this rank's
            # own lookups flag anyway (a hit) or an aux row (never flagged), so the merge set is the rank's real lookups'.
            assert lS_o.shape[1] in (B, B + 1)
        if j is None:
            j = self.iter
        # (the row merge at the end of a table-agg step leaves aux rows alone -- the backward never flags them --, so the
        #  next batch's probe / aux fill may run ahead across it like across any other step)
        sgd_done = False
        # bench.py: HIP timing events of the roofline kernel -- a pre-created (start, stop) pair of ops.TimingEvent, or a list
        # that receives a new pair.  They are attached to the gather's launch (cdlrm_ctx_time_next_gather); on a tape the
        # pair's handles are cells.
        if gather_events is None:
            self._gslot = None
        elif isinstance(gather_events, tuple):
            self._gslot = gather_events
        else:
            self._gslot = (ops.TimingEvent(), ops.TimingEvent())
            gather_events.append(self._gslot)
        if self.merge is not None:
            self.merge.before_step(res.pos if res is not None else None, self.iter)     # rows of an earlier merge this step uses
        self._cur_sorted = self._next_sorted = None
        sliced = lS_o is None and not self.evict_victim
        if sliced:
            if res is not None and res.pos is not None:
                self._cur_sorted = res.pos[0].sorted_views(res.pos[1])
            if self._next_res is not None and next_res.pos is not None:
                self._next_sorted = next_res.pos[0].sorted_views(next_res.pos[1])
            pf = self._pref
            if self._cur_sorted is not None and pf is not None and pf.matches(lS_i) and not pf.sorted_ok:
                # this batch's take was issued by the previous step, BEFORE its slice's sort (a chunk resolved late: short chunks):
                # nothing orders this step behind that sort -- it sorts its own slots
                self._cur_sorted = None
        main = S.current_stream(self.dev)
        if self.lr_cells:
            self._set_rate_cells()          # (lr / lr_embeds may have been assigned since the factor was set)
        path = self._step_path(X, lS_i, lS_o, next_idx)
        # the addresses-and-strides half of a tape's key: no decision, but baked into the recorded arguments
        pr = self._pending_resolve if self._mark_this else None
        layout = (getattr(main, "cuda_stream", 0), X.stride(0), lS_i.stride(0), next_idx.stride(0) if path.nxt else 0,
                  res.slots.stride(0) if (path.resolved and not path.hit) else 0,
                  self._next_res.slots.stride(0) if path.next_resolved else 0, r.stride(0) if r is not None else 0,
                  0 if pr is None else pr["cols"].stride(0))
        self._step_key = (path, layout)
        if sliced:
            self._wait_slices(path, self._cur_sorted, self._next_sorted)
        if res is not None:
            # an in-line take (no prefetched result for this batch) runs on the side stream: behind the chunk's resolve
            self.side.wait_event(res.ready)
        if self._next_res is not None and next_res.ready is not (res.ready if res is not None else None):
            # the next batch's take may run on the side stream too (single aux region / chained take): behind ITS chunk
            self.side.wait_event(next_res.ready)
        if self.use_tape and sliced:
            sgd_done = self._step_taped(path, layout, X, lS_i, T, next_idx)
        else:
            sgd_done = self._fwd_bwd(path, X, lS_i, T, lS_o, next_idx)
        if self.evict_victim:
            # on the side stream, behind the embedding update _fwd_bwd issued there and in front of the next step's take
            if n not in self._vwb_work:
                self._vwb_work[n] = ops.victim_writeback_work(self.ctx, n)
            ops.victim_writeback(self.ctx, lS_i, self._last_slots, res.src if (res is not None and lS_o is None) else None,
                                 self._last_phase, self._vwb_work[n], stream=self.side)
        if self._mark_this:
            self._pending_resolve = None        # issued by this step
        # ---- dense gradient exchange + SGD ----
        if self.multi and self.defer_top:
            # two exchanges, issued in the same order on every rank: the top MLP's (its weight gradients were launched
            # on the side stream right after the top dgrad chain) runs beside the rest of this step's backward and the
            # head of the next step; the bottom MLP's is the only one on the critical path
            wst = self.wst
            gt, gb = self._grad_views
            with S.on_stream(wst):
                self._exchange(gt, stream=wst)
                self._dense_step2(path, self.rng_top, stream=wst)
                self._events["top_updated"].record(wst)
            self._exchange(gb)
            if path.join == "emb_done":
                S.current_stream(self.dev).wait_event(self._events["emb_done"])
            self._dense_step2(path, self.rng_bot)
            sgd_done = True
        elif self.multi:
            self._exchange(self.grad_flat[:self.n_weight])
            # the join _fwd_bwd left out: the embedding backward / sparse SGD on the side stream ran beside the
            # all-reduce (the reference overlaps optimizer_embeds.step() with it the same way, :412-414)
            S.current_stream(self.dev).wait_event(self._events["emb_done"])
        if not sgd_done:
            self._dense_step(path)
        # ---- periodic cache-row merge (main_no_ddp.py:417-423) ----
        if j is None:
            j = self.iter
        if self.multi and j > 0 and j % self.agg_freq == 0:
            # (one rank averages with itself, W[u] = W[u] / 1: nothing to do, and no flags are kept at world == 1)
            if self._emb_done is not None:      # the merge reads (and the flag reset races with) this step's row updates
                S.current_stream(self.dev).wait_event(self._emb_done)
            self.table_aggregate()
            # the next step's gather may run on the side stream: it has to see the merged rows
            self.side.wait_stream(S.current_stream(self.dev))
        elif self.merge is not None:
            self.merge.after_step(self.iter)    # the rows the NEXT step needs, and this step's share of the rest
        self.iter += 1
        return self._buffers(B)["loss"]

    def _fwd_bwd(self, path: StepPath, X, lS_i, T, lS_o, next_idx=None):
        """Forward + backward of one iteration up to: all dense gradients in grad_flat, cache rows updated.  Every branch that
        depends on the step reads `path`."""
        ctx, cg = self.ctx, self.cg
        B = X.shape[0]
        n = lS_i.shape[1]
        buf = self._buffers(B)
        feat, dfeat, R, dR = buf["feat"], buf["dfeat"], buf["R"], buf["dR"]
        F, D = self.F, self.D
        # ---- forward ----
        # tag probe + aux-row fill (PCIe) on the side stream, under the bottom MLP -- or already done: the previous
        # step issues them for this batch behind its embedding backward (software-pipelined across iterations)
        # Stream/event calls go through `rec` so that a recorded step (see _step_taped) replays them too; the events
        # are persistent engine objects (a wait always sees the latest record, whichever tape issued it).
        main = S.current_stream(self.dev)
        side = self.side
        ev = self._events
        if self.defer_top and self.cat:
            # the previous step's top weight gradients read R = the feature block this step's first kernels overwrite
            rec(main.wait_event, ev["top_updated"])
        pref, self._pref = self._pref, None
        top_waited = path.top_waited
        self._phase = path.phase
        if path.hit:
            (slots, miss_pos, miss_count), probed = pref.out, pref.probed
        else:
            rec(side.wait_stream, main)
            slots, miss_pos, miss_count = self._take(lS_i, self._res if path.resolved else None, self._phase, self._phase, side)
            probed = ev["probed_inline"]
            rec(probed.record, side)
        self._last_slots, self._last_phase = slots, self._phase          # (ops.victim_writeback reads them behind the step)

        fused = path.fused

        def gather(st):
            if fused:       # the rows are the interaction kernel's operand loads: nothing to launch here
                return
            if self.qr is not None:
                ops.qr_cached_fwd(ctx, slots, self._r, self.Wr, self.qr_coll, self.qr_op, feat[:, 1:, :], feat.stride(0), D, stream=st)
                return
            if path.timed:                      # bench.py: the roofline kernel's own start / stop timestamps
                ops.time_next_gather(ctx, self._gslot[0], self._gslot[1])
            ops.embbag_fwd(ctx, slots, lS_o, feat[:, 1:, :], feat.stride(0), D, n_bags=path.n_bags, stream=st)

        # Short local batches: the gather (6 us at 1024) goes to the SIDE stream, beside the bottom MLP's forward -- it
        # needs the probe result and the previous step's embedding update, which ran on that very stream (in order: no
        # event), not the bottom MLP.  Long batches: it is the HBM-roofline kernel and runs alone on the main stream.
        side_gather = path.side_gather
        if side_gather:
            rec(side.wait_event, probed)
            if self.defer_top and not self.cat and not top_waited:
                # the previous step's deferred top-MLP update is waited for HERE, on the side stream in front of the gather:
                # the one wait the training queue has in front of the interaction (`gathered`) then covers it too -- one
                # barrier packet less on that queue.  (The update has landed long before the embedding update the gather
                # follows in order.)
                rec(side.wait_event, ev["top_updated"])
                top_waited = True
            gather(side)
            rec(ev["gathered"].record, side)
        cur = X
        bot_acts = [X]
        for i, (l, act) in enumerate(self.bot):
            y = feat[:, 0, :] if i == len(self.bot) - 1 else buf["bot_y"][i]
            ops.linear_fwd(cur, self.W[l], l.bias.data, y, act, alone=self.wide_gemm, **self._mm(l))
            bot_acts.append(y)
            cur = y
        if side_gather:
            rec(main.wait_event, ev["gathered"])
        else:
            # the gather runs alone on the main stream (it is the HBM-roofline kernel: nothing competes for bandwidth)
            rec(main.wait_event, probed)
            gather(main)
        if path.nxt and path.two_phase:
            # Software pipelining across iterations: the NEXT batch's tag probe and aux-row fill (~0.25 ms of PCIe
            # reads at c3) start right behind this batch's gather, on their own stream, into the OTHER aux region
            # (this batch still reads and updates its own aux rows).  The other region was last used by the previous
            # batch: its embedding update must have landed (emb_done).
            pst = self.pref
            if path.gather_alone:
                # long batches: the gather is the HBM-roofline kernel and runs alone; the probe starts behind it
                ev_g = ev["gathered"]
                rec(ev_g.record, main)
                rec(pst.wait_event, ev_g)
            # short batches: every event recorded on the main queue costs a ~6 us bubble there (measured), more than the
            # probe could take from a 6 us gather -- it starts as soon as the other aux region is free
            if path.emb_done_seen:
                rec(pst.wait_event, ev["emb_done"])
            self._pref = self._hand_over(path, next_idx, 1 - self._phase, pst)
            rec(self._pref.probed.record, pst)
        # the backward's sort of the slot ids needs nothing but the probe result: run it on the side, under the MLPs
        emb_work = self._emb_work(n)
        if not side_gather:
            rec(side.wait_event, probed)
        attach = path.attach
        sv = self._cur_sorted if path.sorted is not None else None      # (path.sorted: no sort here)
        once = path.once
        if sv is None and not path.prepared:     # (prepared: a chained take sorted this batch's slots right behind itself)
            ops.embbag_bwd_prepare(ctx, slots, emb_work, stream=side)
        if self.defer_top and not self.cat and not top_waited:
            # the previous step's top-MLP update (weight gradients read R / top_y / top_dy, then all-reduce and SGD on
            # the side stream) has to have landed before this step overwrites those buffers and reads the weights
            # (top_waited: the event this step's gather waited for was recorded behind that update)
            rec(main.wait_event, ev["top_updated"])
        if fused:
            if path.timed:                      # bench.py: the kernel that does the gather, timed by its own launch
                ops.time_next_gather(ctx, self._gslot[0], self._gslot[1])
            if path.fwd_marked:
                # the placed resolve (prefetch stream) waits for an event that completes WITH this launch
                ops.event_attach_next(ev["fwd_mark"], main)
            ops.gather_interact_fwd(ctx, slots, feat[:, 0, :], self.itself, R)
        elif not self.cat:
            ops.interact_fwd(feat, self.itself, R)
        if path.resolve_cols is not None:
            self._issue_resolve(self._pending_resolve, rec, main, placed=path)
        cur = R
        top_acts = [R]
        fused_head = self.fused_head
        for i, (l, act) in enumerate(self.top):
            y = buf["top_y"][i]
            if not (fused_head and i == len(self.top) - 1):
                ops.linear_fwd(cur, self.W[l], l.bias.data, y, act, alone=self.wide_gemm, **self._mm(l))
            top_acts.append(y)
            cur = y
        Z = cur
        # ---- backward ----
        # No stand-alone activation-backward pass: every gradient buffer holds the PRE-activation gradient of its
        # layer.  The loss kernel applies the last sigmoid's derivative, each dgrad GEMM applies the derivative of
        # the activation that produced its input (x_act) in its epilogue, the interaction backward does the same
        # for the bottom MLP's output, and the bias gradients are column sums taken inside the wgrad GEMMs.
        last_act = self.top[-1][1]
        whole_plan, split = self._wplans(buf)
        wst = self.wst
        sgd_in_wgrad = self.defer_top and not self.multi      # one rank: the dense SGD rides in the weight gradients' reduction pass
        # ... or the dense Adagrad's step does, at the same places (cdlrm_mlp_wgrad_opt_ex); SGD: the calls stay what they were
        dopt = {"opt": self._dense_opt(path)} if (sgd_in_wgrad and path.dense_optimizer != "sgd") else {}

        n_top = len(self.top)
        if fused_head:
            # last layer + loss + the layer's input gradient in one launch
            l = self.top[-1][0]
            dX = dR if n_top == 1 else buf["top_dy"][-2]
            ops.head_fwd_bwd(top_acts[-2][:, :l.in_features], self.W[l], l.bias.data, T, Z, buf["top_dy"][-1],
                             dX[:, :l.in_features], buf["loss"], self._head_scratch,
                             x_act=(self.top[-2][1] if n_top > 1 else 0), kind=self.loss_kind,
                             weights=self.loss_weights, threshold=self.loss_threshold, Zc=buf["Zc"], finish=False)
            if path.loss_sync:      # partial sums -> loss, running statistics: here, or on the side stream below
                ops.head_finish(self._head_scratch, B, buf["loss"], acc=self.stat_acc)
            dY = dX
        else:
            ops.loss_fwd_bwd(Z, T, buf["loss"], buf["top_dy"][-1], kind=self.loss_kind, weights=self.loss_weights,
                             threshold=self.loss_threshold, Zc=buf["Zc"], sigmoid_bwd=(last_act == 2))
            rec(self.stat_acc.add_, buf["loss"][1:3])
            dY = buf["top_dy"][-1]
        for i in reversed(range(n_top - 1 if fused_head else n_top)):
            l, act = self.top[i]
            if i == len(self.top) - 1 and act == 2:
                act = 0                                      # already applied by the loss kernel
            elif i < len(self.top) - 1:
                act = 0                                      # applied by the dgrad epilogue of layer i+1
            dX = dR if i == 0 else buf["top_dy"][i - 1]
            if i == 0 and attach and split is not None:
                # `top_dz` (every top-layer dZ is final: the weight gradients may start) completes WITH the chain's last GEMM
                # -- attached to its launch instead of recorded behind it: a record is a marker packet of its own and left
                # a 6-8 us bubble on the training queue
                ops.event_attach_next(ev["top_dz"], main)
            ops.linear_bwd(top_acts[i], self.W[l], top_acts[i + 1], dY, dX, None, None, act,
                           buf["lin_work"], x_act=(self.top[i - 1][1] if i > 0 else 0), alone=self.wide_gemm, **self._mm(l))
            dY = dX
        # (One event on the main queue for both side streams -- recorded behind the interaction backward -- instead of one in
        #  front of it for the weight gradients and one behind it for the embedding backward measured slower at c3, 0.698 vs
        #  0.675 ms: the saved bubble is worth less than the 57 us the weight gradients start later.  The interaction backward
        #  split by rows -- the dense feature's row as its own launch, the rest on the side queue -- measured slower too, 0.718
        #  vs 0.663 ms.  Both schedules were removed in round 3.)
        if split is not None:
            # Every top-layer dZ is final: the top MLP's weight gradients run on their own stream, beside the interaction
            # backward and the bottom MLP's backward.  (Launching each layer's weight gradient as soon as ITS dZ exists -- beside
            # the dgrad chain itself -- measured slower: 0.810 vs 0.782 ms at B=8192; the chain is the critical path and loses CUs
            # to them.  Later starts measured slower too: DESIGN_HISTORY.md.)
            if not (attach and n_top - (1 if fused_head else 0) > 0):
                rec(ev["top_dz"].record, main)
            rec(wst.wait_event, ev["top_dz"])
            ops.mlp_wgrad(split[1], stream=wst, lr=self._rate(path) if sgd_in_wgrad else None, **dopt)
            if not self.defer_top:
                rec(ev["wgrad_done"].record, wst)
            elif not self.multi:
                rec(ev["top_updated"].record, wst)
        if self.cat:
            # dR is the gradient of the feature block itself; only the bottom MLP's output needs its activation's
            # derivative (the dot path applies it in the interaction backward's epilogue)
            ops.act_bwd(dfeat[:, 0, :], feat[:, 0, :], self.bot[-1][1])
        else:
            if attach:
                ops.event_attach_next(ev["interacted"], main)      # completes with the interaction backward's launch
            if once:
                ops.gather_interact_bwd_sgd(ctx, slots, feat[:, 0, :], dR, self.itself, dfeat, sv.once, sv.stride, self._rate_embeds(path),
                                            x_act=self.bot[-1][1])
            elif fused:
                ops.gather_interact_bwd(ctx, slots, feat[:, 0, :], dR, self.itself, dfeat, x_act=self.bot[-1][1])
            else:
                ops.interact_bwd(feat, dR, self.itself, dfeat, x_act=self.bot[-1][1])
        # embedding backward + sparse SGD on a side stream, overlapped with the bottom-MLP backward and the
        # gradient all-reduce (the reference overlaps optimizer_embeds.step() with the all-reduce, :412-414)
        if not attach or self.cat:
            rec(ev["interacted"].record, main)
        rec(side.wait_event, ev["interacted"])
        if fused_head and not path.loss_sync:
            # the head's partial sums -> loss buffer + running statistics, off the training queue.  The next head kernel
            # overwrites the partials only behind the next gather, which is ordered behind this stream's embedding update
            ops.head_finish(self._head_scratch, B, buf["loss"], stream=side, acc=self.stat_acc)
        if self.qr is not None:
            # dL/dE -> the quotient rows' gradient, in place, and the remainder tables' sums and SGD step: both factors are read
            # here, in front of the row update below (same stream) and of Wr's own
            qw = self._qr_work(n)
            ops.qr_cached_bwd(ctx, slots, self._r, self.Wr, self.qr_coll, self.qr_op, dfeat[:, 1:, :], dfeat.stride(0), D, qw,
                              stream=side)
            ops.qr_cached_bwd_finish(ctx, self.qr_coll, n, qw, self._rate_embeds(path), self.Wr, stream=side)
        if path.embed_optimizer != "sgd":
            # the same plan, the Adagrad epilogue: S[tags[slot]] and the row, once per looked-up cache-proper slot
            opt = dict(opt=path.embed_optimizer, eps=path.adagrad_eps, state=self.emb_state, state_base=self.state_base, stream=side)
            if sv is not None:
                ops.embbag_bwd_apply_sorted_opt(ctx, n, dfeat[:, 1:, :], dfeat.stride(0), D, self._rate_embeds(path), emb_work, sv.keys,
                                                sv.meta, sv.stride, self._phase, False, cg.touched if self.multi else None, **opt)
            else:
                ops.embbag_bwd_apply_opt(ctx, n, lS_o, dfeat[:, 1:, :], dfeat.stride(0), D, self._rate_embeds(path), emb_work,
                                         cg.touched if self.multi else None, **opt)
        elif sv is not None:
            ops.embbag_bwd_apply_sorted(ctx, n, dfeat[:, 1:, :], dfeat.stride(0), D, self._rate_embeds(path), emb_work, sv.keys, sv.meta, sv.stride,
                                        self._phase, once, cg.touched if self.multi else None, stream=side)
        else:
            ops.embbag_bwd_apply(ctx, n, lS_o, dfeat[:, 1:, :], dfeat.stride(0), D, self._rate_embeds(path), emb_work,
                                 cg.touched if self.multi else None, stream=side)
        emb_done = ev["emb_done"]
        rec(emb_done.record, side)
        self._emb_done = emb_done
        if path.nxt and not path.two_phase:
            # single aux region: the next batch's fill can only follow this batch's embedding update
            self._pref = self._hand_over(path, next_idx, 0, side)
            if path.chain_sort:
                # ... and the sort of the next batch's slot ids for ITS backward: here it ends well before the step does; issued
                # at the head of the next step it shared HBM with that step's gather (the roofline kernel)
                ops.embbag_bwd_prepare(ctx, self._pref.out[0], emb_work, stream=side)
            if path.chained_top:
                rec(side.wait_event, ev["top_updated"])     # recorded above, behind this step's top-MLP SGD
            rec(self._pref.probed.record, side)
        dY = dfeat[:, 0, :]
        for i in reversed(range(1, len(self.bot))):         # layer 0 has no input gradient
            l, act = self.bot[i]
            dX = buf["bot_dy"][i - 1]
            ops.linear_bwd(bot_acts[i], self.W[l], bot_acts[i + 1], dY, dX, None, None, 0,
                           buf["lin_work"], x_act=self.bot[i - 1][1], **self._mm(l))
            dY = dX
        if split is not None:
            split[0].set_x(0, X)
            ops.mlp_wgrad(split[0], lr=self._rate(path) if sgd_in_wgrad else None, **dopt)
            if not self.defer_top:
                rec(main.wait_event, ev["wgrad_done"])
        else:
            plan = whole_plan
            plan.set_x(0, X)
            ops.mlp_wgrad(plan)
        if self.multi:
            return False        # step() joins behind the gradient all-reduce it issues
        if path.join == "full":
            rec(main.wait_stream, side)
        elif path.join == "emb_done":
            rec(main.wait_event, emb_done)
        return split is not None and sgd_in_wgrad

    # ----------------------------------------------------------------------------------------------
    def evaluate(self, X: torch.Tensor, lS_i: torch.Tensor, lS_o: Optional[torch.Tensor] = None,
                 r: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Forward only (the test loop of main_no_ddp.py:479-494: `cache_group(lS_o, lS_i, emb_tables, rank)` then
        `dlrm(X, lookups)` under no_grad): tag probe with the aux-miss path (test indices outside the cache read their
        host rows -- into the aux region of the batch trained last, whose rows are dead), cached gather, bottom MLP,
        interaction, top MLP.  Returns Z [B, 1] (a buffer reused by the next call)."""
        ctx = self.ctx
        B, n = X.shape[0], lS_i.shape[1]
        assert n <= ctx.aux, "test batch larger than the aux table (test_mini_batch_size <= aux_table_size)"
        if self.merge is not None and self.merge.pending:
            # Rows of the last merge are still on their way, and landing them means COLLECTIVES.  The test loop runs on rank 0
            # only (main_no_ddp.py:478-494): a rank that issued the remaining exchanges from here would issue them alone, in
            # other pieces and at another place of the communicator's order than its peers (a hang, or other ranks' gradients
            # reduced into rows).  Every rank calls drain_merge() at the same step first -- Run does, in front of its rank-0
            # test block.
            raise RuntimeError("evaluate(): a row merge is still draining; every rank has to call drain_merge() first")
        self.finish()
        pend = self._pref
        if pend is not None and pend.phase == self._phase:
            # the next training batch's take already filled THIS aux region (single-region / chained take: the long-batch
            # default): wait for it, let the test batch overwrite the region, and drop the prefetched result -- the next
            # step() then takes (and sorts) its batch again in line
            S.current_stream(self.dev).wait_event(pend.probed)
            self._pref = None
        buf = self._buffers(B)
        feat, R = buf["feat"], buf["R"]
        F, D = self.F, self.D
        slots, _, _ = ops.embbag_probe(ctx, lS_i, aux_phase=self._phase, out=self._probe_bufs(n, "eval"))
        cur = X
        for i, (l, act) in enumerate(self.bot):
            y = feat[:, 0, :] if i == len(self.bot) - 1 else buf["bot_y"][i]
            ops.linear_fwd(cur, self.W[l], l.bias.data, y, act, **self._mm(l))
            cur = y
        if self._fused_gather(lS_o):
            ops.gather_interact_fwd(ctx, slots, feat[:, 0, :], self.itself, R)
        else:
            if self.qr is not None:         # (lS_i: quotients, r: the batch's remainders -- qr_split)
                if lS_o is not None:
                    raise ValueError("quotient-remainder mode takes one lookup per bag")
                assert r is not None and r.dtype == torch.uint8 and tuple(r.shape) == (self.T, n) and r.stride(1) == 1
                ops.qr_cached_fwd(ctx, slots, r, self.Wr, self.qr_coll, self.qr_op, feat[:, 1:, :], feat.stride(0), D)
            else:
                ops.embbag_fwd(ctx, slots, lS_o, feat[:, 1:, :], feat.stride(0), D, n_bags=(B if lS_o is None else lS_o.shape[1]))
            if not self.cat:
                ops.interact_fwd(feat, self.itself, R)
        cur = R
        for i, (l, act) in enumerate(self.top):
            y = buf["top_y"][i]
            ops.linear_fwd(cur, self.W[l], l.bias.data, y, act, alone=self.wide_gemm, **self._mm(l))
            cur = y
        if self.loss_threshold > 0.0:       # DLRM_Net.forward returns the clamped prediction (model_no_ddp.py:311-314)
            cur = torch.clamp(cur, min=self.loss_threshold, max=1.0 - self.loss_threshold)
        return cur

    def drain_merge(self):
        """Land every row of a merge that is still travelling in deadline order (MergePump).  COLLECTIVE: call it on every rank
        at the same step, or on none -- in front of anything only some ranks do next (the rank-0 test loop, a checkpoint)."""
        if self.merge is not None:
            self.merge.drain()

    def finish(self):
        """Order the current stream behind a deferred top-MLP update (defer_top_update): call before reading the top
        MLP's weights, gradients or activation buffers outside step() / evaluate().  Collective while a row merge is
        draining (drain_merge): every rank calls it at the same step, as Run does at print boundaries and at the end."""
        if self.defer_top:
            S.current_stream(self.dev).wait_event(self._events["top_updated"])
        if self._emb_done is not None:          # a pipelined short-batch step leaves the embedding update un-joined
            S.current_stream(self.dev).wait_event(self._emb_done)
        self.drain_merge()                      # rows of the last merge that are still on their way

    def prediction(self, B: int) -> torch.Tensor:
        """Z of the last step at batch size B as DLRM_Net.forward returns it (clamped under --loss-threshold)."""
        buf = self._buffers(B)
        return buf["Zc"] if buf["Zc"] is not None else buf["top_y"][-1]

    def _step_taped(self, path: StepPath, layout, X, lS_i, T, next_idx):
        """The same launch sequence as _fwd_bwd, replayed from a recording.  At small local batches the ~30 launches
        of a step take less GPU time than the Python around them (argument marshalling, stream lookups): the first
        step of each control path (StepPath) at each layout runs _fwd_bwd under `_lib.start_recording`, later ones re-issue
        the recorded (function, arguments) list.  Pointers that change from step to step (X, T, the index tensors) are shared
        ctypes cells patched before each replay; everything else the step touches is a preallocated buffer with a fixed address."""
        import ctypes as C
        B = path.B
        main = S.current_stream(self.dev)
        key = (path, layout)
        tape = self._tapes.get(key)
        if tape is None:
            calls = []
            _lib.start_recording(calls)
            try:
                included = self._fwd_bwd(path, X, lS_i, T, None, next_idx)
                if not self.multi and not included:   # no gradient exchange in between: the dense SGD rides on the tape too
                    self._dense_step(path)
            finally:
                _lib.stop_recording()
            # pointer arguments equal to one of the per-step tensors become shared cells
            cells = {k: C.c_void_p(v) for k, v in self._tape_ptrs(path, X, T, lS_i, next_idx).items()}
            by_value = {c.value: c for c in cells.values()}
            if len(by_value) != len(cells):
                return not self.multi      # aliased inputs: stay on the untaped path
            if path.lr_cells:
                # the rate cells are on the recording already (ops passes them through); named here for the native tape, which
                # finds a float argument's cell by the object's identity
                cells["lr"], cells["lr_embeds"] = self._lr_cell, self._lr_embeds_cell
            prog = []
            for fn, args in calls:
                if getattr(fn, "argtypes", None) is not None:
                    args = tuple(by_value.get(a, a) if isinstance(a, int) and not isinstance(a, bool) else a for a in args)
                    prog.append((fn, args, True))
                else:
                    prog.append((fn, args, False))
            post = self._pref
            native = None
            if self.native_tape and _lib.native_tape_ok():
                # the same calls as a C-side tape: one library call per step instead of ~45 interpreted ones (0.22 ms of
                # host time per step, more than the GPU needs at a per-rank batch of 1024)
                try:
                    native = _lib.NativeTape(prog, cells, main_stream=main.cuda_stream if path.lanes > 1 else None,
                                             max_lanes=path.lanes)
                except _lib.TapeUnsupported as e:
                    native = None
                    self.tape_fallbacks.append(str(e))      # this control path replays from Python (bench.py reports it)
            self._tapes[key] = dict(prog=prog, cells=cells, native=native, pref=None if post is None else post.stored())
            return not self.multi
        cells = tape["cells"]
        for k, v in self._tape_ptrs(path, X, T, lS_i, next_idx).items():
            cells[k].value = v
        bufs = self._buffers(B)
        whole_plan, split = self._wplans(bufs)
        (split[0] if split is not None else whole_plan).set_x(0, X)
        if tape["native"] is not None:
            rc = tape["native"].replay()
            if rc:
                _lib.check(rc)
        else:
            for fn, args, is_lib in tape["prog"]:
                rc = fn(*args)
                if is_lib and rc:
                    _lib.check(rc)
        # the state _fwd_bwd leaves behind
        self._phase = path.phase
        self._emb_done = self._events["emb_done"]
        self._pref = None if tape["pref"] is None else tape["pref"].handed(next_idx)
        return not self.multi

    def _tape_ptrs(self, path: StepPath, X, T, lS_i, next_idx) -> dict:
        """The per-step pointers a recorded step reads, by cell name (_step_taped): the path says which of them exist."""
        p = {"X": X.data_ptr(), "T": T.data_ptr(), "idx": lS_i.data_ptr()}
        if path.nxt:
            p["next"] = next_idx.data_ptr()
        if path.resolved and not path.hit:
            p["ws"], p["wsrc"] = self._res.slots.data_ptr(), self._res.src.data_ptr()
        if path.next_resolved:
            p["nws"], p["nwsrc"] = self._next_res.slots.data_ptr(), self._next_res.src.data_ptr()
        if path.sorted is not None:
            sv = self._cur_sorted
            p["skeys"], p["smeta"], p["sonce"] = sv.keys, sv.meta, sv.once
        if path.timed:
            p["g0"], p["g1"] = self._gslot[0].handle, self._gslot[1].handle
        if self._r is not None:         # quotient-remainder mode (a constant of the engine): the batch's remainder columns
            p["r"] = self._r.data_ptr()
        if path.resolve_cols is not None:       # the placed resolve's chunk: index columns, ring slot, the slot's event
            pr = self._pending_resolve
            p["rcols"], p["rws"] = pr["cols"].data_ptr(), pr["ws"].data_ptr()
            p["rwsrc"], p["rev"] = pr["wsrc"].data_ptr(), int(pr["ev"].cuda_event)
        return p
