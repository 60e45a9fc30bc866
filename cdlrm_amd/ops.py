"""Thin functional layer over the C ABI (include/cdlrm_hip.h) on torch tensors.

Torch is plumbing here (device memory, streams); every computation is a libcdlrm_hip.so call.
"""
from __future__ import annotations

import ctypes as C
from typing import List, Optional, Sequence

import torch

from . import _lib
from ._lib import Geometry, Plan, check, ptr, stream_ptr
from ._lib import Victims as _VictimsStruct
from .lr_schedule import rate_arg as _rate     # a learning rate: a number by value, or the engine's rate cell passed through


def _require_cuda(t: torch.Tensor, name: str):
    if not t.is_cuda:
        raise RuntimeError("cdlrm_amd: %s must live on the MI355X (got %s); there is no CPU path" % (name, t.device))


class CacheCtx:
    """Opaque library context of one cache group (geometry + bound cache state)."""

    def __init__(self, table_rows: Sequence[int], cache_sets: Sequence[int], dim: int, num_ways: int,
                 aux_rows: int, device: torch.device, aux_phases: int = 1):
        self.T = len(table_rows)
        self.D, self.ways, self.aux = int(dim), int(num_ways), int(aux_rows)
        self.aux_phases = max(1, int(aux_phases))
        self.table_rows = [int(x) for x in table_rows]
        self.cache_sets = [int(x) for x in cache_sets]
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("cdlrm_amd: a HIP device is required (no CPU fallback)")
        _lib.require_gpu("cdlrm_amd.ops.CacheCtx")
        _lib.warn_hw_queues()
        self.rows = [self.ways * p + self.aux * self.aux_phases for p in self.cache_sets]
        self.row_base, self.tag_base, self.set_base = [0], [0], [0]
        for k in range(self.T):
            self.row_base.append(self.row_base[-1] + self.rows[k])
            self.tag_base.append(self.tag_base[-1] + self.cache_sets[k] * self.ways)
            self.set_base.append(self.set_base[-1] + self.cache_sets[k])
        self.total_rows, self.total_tags, self.total_sets = self.row_base[-1], self.tag_base[-1], self.set_base[-1]
        self.bm_words = [((n + 63) // 64 + 1023) // 1024 * 1024 for n in self.table_rows]
        self.total_bm_words = sum(self.bm_words)
        tr = (C.c_int64 * self.T)(*self.table_rows)
        cs = (C.c_int64 * self.T)(*self.cache_sets)
        geo = Geometry(self.T, self.D, self.ways, self.aux, tr, cs, self.device.index or 0, self.aux_phases)
        h = C.c_void_p()
        with torch.cuda.device(self.device):
            check(_lib.lib().cdlrm_ctx_create(C.byref(geo), C.byref(h)))
        self.handle = h
        self._host_ptrs = None
        self._keep = None

    def __del__(self):
        try:
            if getattr(self, "handle", None):
                # straight to the library: the garbage collector may run this while a step is being recorded
                _lib.raw().cdlrm_ctx_destroy(self.handle)
                self.handle = None
        except Exception:
            pass

    def bind_cache(self, tags: torch.Tensor, weight: torch.Tensor):
        _require_cuda(tags, "tags"); _require_cuda(weight, "weight")
        assert tags.dtype == torch.int64 and tags.numel() == self.total_tags and tags.is_contiguous()
        assert weight.dtype == torch.float32 and tuple(weight.shape) == (self.total_rows, self.D) and weight.is_contiguous()
        check(_lib.lib().cdlrm_ctx_bind_cache(self.handle, tags.data_ptr(), weight.data_ptr()))
        self._keep = (tags, weight)

    def bind_host_tables(self, ptrs: Sequence[int]):
        ptrs = [int(p) for p in ptrs]
        if ptrs == self._host_ptrs:
            return
        arr = (C.c_void_p * self.T)(*ptrs)
        check(_lib.lib().cdlrm_ctx_bind_host_tables(self.handle, arr))
        self._host_ptrs = ptrs

    def bind_victims(self, victims: Optional["Victims"]):
        """Serve the aux-row fill of the per-iteration probe from the window's HBM-resident victim rows (None:
        from the host tables again)."""
        check(_lib.lib().cdlrm_ctx_bind_victims(self.handle, C.byref(victims.c) if victims is not None else None))
        self._victims = victims

    def check(self, stream=None):
        """Raise if a kernel flagged out-of-range input (synchronises the stream)."""
        check(_lib.lib().cdlrm_ctx_check_sync(self.handle, stream_ptr(stream)))


# ---- per-iteration path --------------------------------------------------------------------------

def embbag_probe(ctx: CacheCtx, idx: torch.Tensor, stream=None, aux_phase: int = 0, out=None):
    """idx int64 [T, n] on device -> (slots int32 [T, n], miss_pos int32 [T, n], miss_count int32 [T]).
    aux_phase: which of the ctx's aux regions receives the misses' rows (double-buffered aux, see engine.py)."""
    _require_cuda(idx, "idx")
    assert idx.dtype == torch.int64 and idx.dim() == 2 and idx.shape[0] == ctx.T and idx.stride(1) == 1
    n = idx.shape[1]
    if out is not None:
        slots, miss_pos, miss_count = out
        assert slots.shape == (ctx.T, n) and slots.dtype == torch.int32 and slots.is_contiguous()
        assert miss_pos.shape == (ctx.T, n) and miss_pos.dtype == torch.int32 and miss_pos.is_contiguous()
        assert miss_count.numel() == ctx.T and miss_count.dtype == torch.int32
    else:
        slots = torch.empty((ctx.T, n), dtype=torch.int32, device=idx.device)
        miss_pos = torch.empty((ctx.T, n), dtype=torch.int32, device=idx.device)
        miss_count = torch.empty((ctx.T,), dtype=torch.int32, device=idx.device)
    check(_lib.lib().cdlrm_embbag_probe(ctx.handle, idx.data_ptr(), n, idx.stride(0) if n else 0, slots.data_ptr(),
                                        miss_pos.data_ptr(), miss_count.data_ptr(), int(aux_phase),
                                        stream_ptr(stream)))
    return slots, miss_pos, miss_count


def window_resolve(ctx: CacheCtx, idx: torch.Tensor, seg_len: int, wslots: torch.Tensor, wsrc: torch.Tensor, stream=None,
                   batch_len: int = 0):
    """Resolve every lookup of idx [T, n] (consecutive global batches of batch_len lookups, each cut into rank slices of
    seg_len; batch_len 0 = one run of seg_len-long segments) against the CURRENT tags and the bound victim list, once:
    wslots / wsrc int32 [T, n] contiguous (see include/cdlrm_hip.h)."""
    _require_cuda(idx, "idx")
    assert idx.dtype == torch.int64 and idx.dim() == 2 and idx.shape[0] == ctx.T and idx.stride(1) == 1
    n = idx.shape[1]
    for w in (wslots, wsrc):
        assert w.dtype == torch.int32 and tuple(w.shape) == (ctx.T, n) and w.is_contiguous()
    check(_lib.lib().cdlrm_window_resolve(ctx.handle, idx.data_ptr(), n, idx.stride(0), int(batch_len), int(seg_len), wslots.data_ptr(),
                                          wsrc.data_ptr(), stream_ptr(stream)))


def embbag_take(ctx: CacheCtx, idx: torch.Tensor, wslots: torch.Tensor, wsrc: torch.Tensor, slots_out: torch.Tensor,
                aux_phase: int = 0, stream=None):
    """One batch out of a resolved window: idx / wslots / wsrc are [T, n] column VIEWS of the window's tensors."""
    n = idx.shape[1]
    assert idx.dtype == torch.int64 and idx.stride(1) == 1 and wslots.stride(1) == 1 and wsrc.stride(1) == 1
    assert wslots.shape == (ctx.T, n) and wsrc.shape == (ctx.T, n) and wslots.stride(0) == wsrc.stride(0)
    assert slots_out.dtype == torch.int32 and slots_out.shape == (ctx.T, n) and slots_out.is_contiguous()
    check(_lib.lib().cdlrm_embbag_take(ctx.handle, idx.data_ptr(), n, idx.stride(0), wslots.data_ptr(), wsrc.data_ptr(),
                                       wslots.stride(0), slots_out.data_ptr(), int(aux_phase), stream_ptr(stream)))


def victim_writeback_work(ctx: CacheCtx, n: int) -> torch.Tensor:
    nbytes = int(_lib.lib().cdlrm_victim_writeback_work_bytes(ctx.T, n))
    return torch.empty((nbytes + 255) // 256 * 256, dtype=torch.uint8, device=ctx.device)


def victim_writeback(ctx: CacheCtx, idx: torch.Tensor, slots: torch.Tensor, wsrc: Optional[torch.Tensor], aux_phase: int,
                     work: torch.Tensor, stream=None):
    """--evict-victim-cache: the batch's trained aux rows (its misses) back to their host rows and to their copies among the
    window's resident victim rows; behind the step's embedding update, in front of the next batch's take."""
    n = idx.shape[1]
    assert idx.dtype == torch.int64 and idx.stride(1) == 1 and slots.dtype == torch.int32 and slots.shape == (ctx.T, n) \
        and slots.is_contiguous()
    check(_lib.lib().cdlrm_victim_writeback(ctx.handle, idx.data_ptr(), n, idx.stride(0), slots.data_ptr(),
                                            0 if wsrc is None else wsrc.data_ptr(), 0 if wsrc is None else wsrc.stride(0),
                                            int(aux_phase), work.data_ptr(), stream_ptr(stream)))


class TimingEvent:
    """A HIP timing event of the library's own (its handle exists from creation on, so a launch tape can hold it)."""

    def __init__(self):
        h = _lib.raw().cdlrm_event_create(1)
        if not h:
            raise _lib.CdlrmError(-22, _lib.raw().cdlrm_last_error().decode("utf-8", "replace"))
        self.handle = int(h)

    def elapsed_us(self, stop: "TimingEvent") -> float:
        """Microseconds from this event to `stop` (waits for `stop`)."""
        us = C.c_float(0.0)
        check(_lib.raw().cdlrm_event_elapsed_us(self.handle, stop.handle, C.byref(us)))
        return float(us.value)

    def __del__(self):
        h, self.handle = getattr(self, "handle", None), None
        if h:
            try:
                _lib.raw().cdlrm_event_destroy(h)
            except Exception:
                pass


def event_attach_next(event: "torch.cuda.Event", stream):
    """`event` completes with the next linear_bwd / interact_bwd launched on `stream` (attached to the launch: no marker
    packet on the queue).  The event must have been recorded once before (torch creates the HIP event lazily)."""
    h = event.cuda_event
    assert h, "record the event once before attaching it"
    check(_lib.lib().cdlrm_event_attach_next(int(h), stream.cuda_stream))


def event_record(event: "torch.cuda.Event", stream):
    """event.record(stream) as a library call (the handle is an argument a launch tape can keep in a cell)."""
    h = event.cuda_event
    assert h, "record the event once through torch first (it creates the HIP event lazily)"
    check(_lib.lib().cdlrm_event_record(int(h), stream.cuda_stream))


def time_next_gather(ctx: CacheCtx, start: TimingEvent, stop: TimingEvent):
    """The next embbag_fwd on this context leaves its own start / stop timestamps in the two events (attached to the
    launch: nothing is added to the queue)."""
    check(_lib.lib().cdlrm_ctx_time_next_gather(ctx.handle, start.handle, stop.handle))


def embbag_fwd(ctx: CacheCtx, slots: torch.Tensor, offsets: Optional[torch.Tensor], out: torch.Tensor,
               ld_bag: int, ld_table: int, n_bags: Optional[int] = None, stream=None):
    n = slots.shape[1]
    nb = n if offsets is None else offsets.shape[1]
    if n_bags is not None:
        nb = n_bags
    check(_lib.lib().cdlrm_embbag_fwd(ctx.handle, slots.data_ptr(), ptr(offsets), n, nb,
                                      0 if offsets is None else offsets.stride(0), out.data_ptr(), ld_bag, ld_table,
                                      stream_ptr(stream)))


# ---- the quotient-remainder trick on the cached step (csrc/qr_cached.hip) ----------

QR_OPS = {"mult": 0, "add": 1}


def qr_cached_shape_ok(dim: int, c: int) -> bool:
    """The backward keeps one [c, D] accumulator per lane group of a 256-thread workgroup in LDS: 64 KB at the most."""
    d4 = max(1, int(dim) // 4)
    lpr = min(64, max(4, 1 << (d4 - 1).bit_length()))
    return (256 // lpr) * int(c) * d4 * 16 <= 65536


def qr_split(ctx: CacheCtx, idx: torch.Tensor, collisions: torch.Tensor, table_rows: torch.Tensor,
             q: Optional[torch.Tensor] = None, r: Optional[torch.Tensor] = None, stream=None):
    """idx int64 [T, n] (any row pitch) -> (q int64, r uint8), both [T, n]; q=idx splits in place.  collisions int32 [T]
    (0 = a plain table), table_rows int64 [T] (rows of the unsplit tables), both on the device."""
    _require_cuda(idx, "idx")
    assert idx.dtype == torch.int64 and idx.dim() == 2 and idx.shape[0] == ctx.T and idx.stride(1) == 1
    assert collisions.dtype == torch.int32 and collisions.numel() == ctx.T and collisions.is_cuda
    assert table_rows.dtype == torch.int64 and table_rows.numel() == ctx.T and table_rows.is_cuda
    n = idx.shape[1]
    if q is None:
        q = torch.empty((ctx.T, n), dtype=torch.int64, device=idx.device)
    if r is None:
        r = torch.empty((ctx.T, n), dtype=torch.uint8, device=idx.device)
    assert q.dtype == torch.int64 and tuple(q.shape) == (ctx.T, n) and q.stride(1) == 1
    assert r.dtype == torch.uint8 and tuple(r.shape) == (ctx.T, n) and r.stride(1) == 1
    ld = lambda t: t.stride(0) if ctx.T > 1 else max(n, 1)
    check(_lib.lib().cdlrm_qr_split(ctx.handle, idx.data_ptr(), n, ld(idx), collisions.data_ptr(), table_rows.data_ptr(),
                                    q.data_ptr(), ld(q), r.data_ptr(), ld(r), stream_ptr(stream)))
    return q, r


def _qr_args(ctx: CacheCtx, slots, r, Wr, collisions):
    n = slots.shape[1]
    assert slots.dtype == torch.int32 and tuple(slots.shape) == (ctx.T, n) and slots.is_contiguous()
    assert r.dtype == torch.uint8 and tuple(r.shape) == (ctx.T, n) and r.stride(1) == 1
    assert Wr.dtype == torch.float32 and Wr.dim() == 3 and Wr.shape[0] == ctx.T and Wr.shape[2] == ctx.D and Wr.is_contiguous()
    assert collisions.dtype == torch.int32 and collisions.numel() == ctx.T
    return n, (r.stride(0) if ctx.T > 1 else max(n, 1)), int(Wr.shape[1])


def qr_cached_fwd(ctx: CacheCtx, slots: torch.Tensor, r: torch.Tensor, Wr: torch.Tensor, collisions: torch.Tensor, op: int,
                  out: torch.Tensor, ld_bag: int, ld_table: int, stream=None):
    """cdlrm_embbag_fwd's gather composed with the remainder rows in one pass: out[b, k] = row(slot) (*|+) Wr[k][r]."""
    n, ld_r, c = _qr_args(ctx, slots, r, Wr, collisions)
    check(_lib.lib().cdlrm_qr_cached_fwd(ctx.handle, slots.data_ptr(), r.data_ptr(), ld_r, Wr.data_ptr(), collisions.data_ptr(),
                                         c, int(op), n, out.data_ptr(), ld_bag, ld_table, stream_ptr(stream)))


def qr_cached_bwd_work(ctx: CacheCtx, n: int, c: int) -> torch.Tensor:
    nbytes = int(_lib.lib().cdlrm_qr_cached_bwd_work_bytes(ctx.T, n, ctx.D, int(c)))
    return torch.empty(max(nbytes, 16) // 4, dtype=torch.float32, device=ctx.device)


def qr_cached_bwd(ctx: CacheCtx, slots: torch.Tensor, r: torch.Tensor, Wr: torch.Tensor, collisions: torch.Tensor, op: int,
                  grad: torch.Tensor, ld_bag: int, ld_table: int, work: torch.Tensor, stream=None):
    """grad (dL/dE, addressed like the forward's out) -> the cache rows' gradient, in place; the remainder tables' partial sums
    into `work` (qr_cached_bwd_work)."""
    n, ld_r, c = _qr_args(ctx, slots, r, Wr, collisions)
    check(_lib.lib().cdlrm_qr_cached_bwd(ctx.handle, slots.data_ptr(), r.data_ptr(), ld_r, Wr.data_ptr(), collisions.data_ptr(),
                                         c, int(op), n, grad.data_ptr(), ld_bag, ld_table, work.data_ptr(), stream_ptr(stream)))


def qr_cached_bwd_finish(ctx: CacheCtx, collisions: torch.Tensor, n: int, work: torch.Tensor, lr: float, Wr: torch.Tensor,
                         gWr: Optional[torch.Tensor] = None, stream=None):
    """Wr -= lr * gWr, gWr = the partial sums of qr_cached_bwd in ascending order (optionally stored)."""
    assert Wr.dtype == torch.float32 and Wr.is_contiguous() and (gWr is None or (gWr.shape == Wr.shape and gWr.is_contiguous()))
    check(_lib.lib().cdlrm_qr_cached_bwd_finish(ctx.handle, collisions.data_ptr(), int(Wr.shape[1]), n, work.data_ptr(), _rate(lr),
                                                Wr.data_ptr(), ptr(gWr), stream_ptr(stream)))


def embbag_bwd_work(ctx: CacheCtx, n: int, device) -> torch.Tensor:
    """(zero-filled: embbag_bwd_apply_sorted uses the buffer's scratch without a prepare in front)"""
    nbytes = int(_lib.lib().cdlrm_embbag_bwd_work_bytes(ctx.T, n, ctx.D))
    work = torch.zeros((nbytes + 255) // 256 * 256, dtype=torch.uint8, device=device)
    # the fill runs on the CURRENT stream, the buffer's first user (a prepare) on a side stream of the caller's: it has to have
    # landed before anything else touches the buffer (once per buffer)
    torch.cuda.current_stream(device).synchronize()
    return work


def embbag_bwd_sgd(ctx: CacheCtx, slots: torch.Tensor, offsets: Optional[torch.Tensor], grad: torch.Tensor,
                   ld_bag: int, ld_table: int, lr: float, work: torch.Tensor, touched: Optional[torch.Tensor] = None,
                   stream=None):
    n = slots.shape[1]
    nb = n if offsets is None else offsets.shape[1]
    check(_lib.lib().cdlrm_embbag_bwd_sgd(ctx.handle, slots.data_ptr(), ptr(offsets), n, nb,
                                          0 if offsets is None else offsets.stride(0), grad.data_ptr(), ld_bag,
                                          ld_table, _rate(lr), work.data_ptr(), ptr(touched), stream_ptr(stream)))


def embbag_bwd_prepare(ctx: CacheCtx, slots: torch.Tensor, work: torch.Tensor, stream=None):
    check(_lib.lib().cdlrm_embbag_bwd_prepare(ctx.handle, slots.data_ptr(), slots.shape[1], work.data_ptr(),
                                              stream_ptr(stream)))


def embbag_bwd_apply(ctx: CacheCtx, n: int, offsets: Optional[torch.Tensor], grad: torch.Tensor, ld_bag: int,
                     ld_table: int, lr: float, work: torch.Tensor, touched: Optional[torch.Tensor] = None, stream=None):
    nb = n if offsets is None else offsets.shape[1]
    check(_lib.lib().cdlrm_embbag_bwd_apply(ctx.handle, ptr(offsets), n, nb, 0 if offsets is None else offsets.stride(0),
                                            grad.data_ptr(), ld_bag, ld_table, _rate(lr), work.data_ptr(), ptr(touched),
                                            stream_ptr(stream)))


def embbag_bwd_apply_rest(ctx: CacheCtx, n: int, offsets: Optional[torch.Tensor], grad: torch.Tensor, ld_bag: int,
                          ld_table: int, lr: float, work: torch.Tensor, touched: Optional[torch.Tensor] = None, stream=None):
    """embbag_bwd_apply behind gather_interact_bwd_sgd: the once-only slots are done, the runs of >= 2 lookups are left."""
    nb = n if offsets is None else offsets.shape[1]
    check(_lib.lib().cdlrm_embbag_bwd_apply_rest(ctx.handle, ptr(offsets), n, nb, 0 if offsets is None else offsets.stride(0),
                                                 grad.data_ptr(), ld_bag, ld_table, _rate(lr), work.data_ptr(), ptr(touched),
                                                 stream_ptr(stream)))


def embbag_bwd_once_flags(ctx: CacheCtx, work: torch.Tensor, n: int) -> int:
    """Address of the once-only flags (uint8 [T, n]) a prepare left in `work`."""
    import ctypes as C
    out = C.c_void_p()
    check(_lib.lib().cdlrm_embbag_bwd_once_flags(ctx.handle, work.data_ptr(), n, C.byref(out)))
    return int(out.value)


def embbag_bwd_sorted(ctx: CacheCtx, nb: int, n: int, device) -> torch.Tensor:
    """Caller-owned buffer for the sorted slot lists of a look-ahead chunk of nb batches of n lookups per table."""
    nbytes = int(_lib.lib().cdlrm_embbag_bwd_sorted_bytes(ctx.T, nb, n))
    # zero-filled: lists nobody has sorted yet are still lists of valid (slot 0, position 0) keys
    buf = torch.zeros((nbytes + 255) // 256 * 256, dtype=torch.uint8, device=device)
    torch.cuda.current_stream(device).synchronize()
    return buf


def embbag_bwd_prepare_window(ctx: CacheCtx, wslots: torch.Tensor, batch_len: int, nb: int, n: int, sorted_buf: torch.Tensor,
                              stream=None, j0: int = 0, count: Optional[int] = None):
    """Sort the slot ids of batches [j0, j0 + count) of a chunk of nb (default: all of them), every table, at once: wslots int32
    [T, >= (nb - 1) * batch_len + n] (the resolver's chunk, or a view starting at this rank's first column)."""
    assert wslots.dtype == torch.int32 and wslots.stride(1) == 1
    check(_lib.lib().cdlrm_embbag_bwd_prepare_window(ctx.handle, wslots.data_ptr(), wslots.stride(0), batch_len, nb, n, int(j0),
                                                     int(nb - j0 if count is None else count), sorted_buf.data_ptr(),
                                                     stream_ptr(stream)))


def embbag_bwd_sorted_views(ctx: CacheCtx, sorted_buf: torch.Tensor, nb: int, n: int, j: int):
    """(keys, meta, once) addresses of batch j inside a sorted chunk; table t's lists lie t * nb * n elements further."""
    import ctypes as C
    k, m, o = C.c_void_p(), C.c_void_p(), C.c_void_p()
    check(_lib.lib().cdlrm_embbag_bwd_sorted_views(ctx.handle, sorted_buf.data_ptr(), nb, n, j, C.byref(k), C.byref(m), C.byref(o)))
    return int(k.value), int(m.value), int(o.value)


def embbag_bwd_apply_sorted(ctx: CacheCtx, n: int, grad: torch.Tensor, ld_bag: int, ld_table: int, lr: float, work: torch.Tensor,
                            keys: int, meta: int, tstride: int, aux_phase: int, rest: bool,
                            touched: Optional[torch.Tensor] = None, stream=None):
    """embbag_bwd_apply / _apply_rest over a sorted chunk's lists (addresses from embbag_bwd_sorted_views)."""
    check(_lib.lib().cdlrm_embbag_bwd_apply_sorted(ctx.handle, n, grad.data_ptr(), ld_bag, ld_table, _rate(lr), work.data_ptr(),
                                                   keys, meta, tstride, int(aux_phase), int(bool(rest)), ptr(touched),
                                                   stream_ptr(stream)))


EMB_OPTS = {"sgd": 0, "rowwise_adagrad": 1}          # include/cdlrm_hip.h: CDLRM_EMB_OPT_*


def embbag_bwd_apply_opt(ctx: CacheCtx, n: int, offsets: Optional[torch.Tensor], grad: torch.Tensor, ld_bag: int,
                         ld_table: int, lr: float, work: torch.Tensor, touched: Optional[torch.Tensor] = None, *,
                         opt: str = "sgd", eps: float = 0.0, state: Optional[torch.Tensor] = None,
                         state_base: Optional[torch.Tensor] = None, stream=None):
    """embbag_bwd_apply with an optimizer for the cache rows: opt "sgd" (the sibling's launches) or "rowwise_adagrad" (state:
    fp32, one accumulator per table row, table t's from state_base[t] on; state_base: int64 [T] on the device)."""
    nb = n if offsets is None else offsets.shape[1]
    _check_emb_state(ctx, state, state_base)
    check(_lib.lib().cdlrm_embbag_bwd_apply_opt(ctx.handle, ptr(offsets), n, nb, 0 if offsets is None else offsets.stride(0),
                                                grad.data_ptr(), ld_bag, ld_table, _rate(lr), work.data_ptr(), ptr(touched),
                                                EMB_OPTS[opt], float(eps), ptr(state), ptr(state_base), stream_ptr(stream)))


def embbag_bwd_apply_sorted_opt(ctx: CacheCtx, n: int, grad: torch.Tensor, ld_bag: int, ld_table: int, lr: float,
                                work: torch.Tensor, keys: int, meta: int, tstride: int, aux_phase: int, rest: bool,
                                touched: Optional[torch.Tensor] = None, *, opt: str = "sgd", eps: float = 0.0,
                                state: Optional[torch.Tensor] = None, state_base: Optional[torch.Tensor] = None, stream=None):
    """embbag_bwd_apply_sorted with an optimizer for the cache rows (embbag_bwd_apply_opt); rest=True takes "sgd" only."""
    _check_emb_state(ctx, state, state_base)
    check(_lib.lib().cdlrm_embbag_bwd_apply_sorted_opt(ctx.handle, n, grad.data_ptr(), ld_bag, ld_table, _rate(lr), work.data_ptr(),
                                                       keys, meta, tstride, int(aux_phase), int(bool(rest)), ptr(touched),
                                                       EMB_OPTS[opt], float(eps), ptr(state), ptr(state_base),
                                                       stream_ptr(stream)))


def _check_emb_state(ctx: CacheCtx, state, state_base):
    """The kernels index `state` by table index without knowing its length: it must hold every table's rows."""
    if state is None:
        return
    assert state.dtype == torch.float32 and state.is_contiguous() and state.numel() >= sum(int(r) for r in ctx.table_rows)
    assert state_base is not None and state_base.dtype == torch.int64 and state_base.numel() == ctx.T and state_base.is_contiguous()


BWD_ENTRIES = {"apply": 0, "rest": 1, "sorted": 2, "sorted_rest": 3}          # include/cdlrm_hip.h: CDLRM_BWD_ENTRY_*
BWD_APPLY_KERNELS = {0: None, 1: "chunks", 2: "blocks", 3: "blocks_lean"}      # CDLRM_BWD_APPLY_*


def embbag_bwd_route(T: int, D: int, n: int, offsets: bool, entry: str, nb: int = 1, j0: int = 0,
                     count: Optional[int] = None) -> dict:
    """The kernels one embedding backward launches, from the same plan, without launching them: entry "apply"
    (embbag_bwd_prepare + embbag_bwd_apply), "rest" (+ embbag_bwd_apply_rest), "sorted" / "sorted_rest"
    (embbag_bwd_prepare_window(nb, j0, count) + embbag_bwd_apply_sorted(rest = 0 / 1)) on T tables of D columns with n lookups
    each, offsets given or not.  Sort (sort_chunk, sort_e, sort_chunks, merge_passes, seg_meta, keys_in_b), apply kernel
    (BWD_APPLY_KERNELS), arange, lpr, grids under the current cdlrm_debug_set values, and the byte offsets of table 0's sorted
    keys / run distances / once-only flags in the work buffer (window entries: in the sorted buffer, batch j0).  No device is
    touched."""
    out = _lib.EmbBwdRoute()
    check(_lib.raw().cdlrm_embbag_bwd_route(int(T), int(D), int(n), int(bool(offsets)), BWD_ENTRIES[entry], int(nb), int(j0),
                                            int(nb - j0 if count is None else count), C.byref(out)))
    r = {f: getattr(out, f) for f, _ in _lib.EmbBwdRoute._fields_ if f != "reserved"}
    r["apply"] = BWD_APPLY_KERNELS[r["apply"]]
    return r


# ---- look-ahead window plan -------------------------------------------------------------------------

class WindowPlan:
    """Caller-owned buffers of one insert plan (cdlrm_plan in the header) + the call sequence."""

    def __init__(self, ctx: CacheCtx, max_window: int, cap_uniq: Optional[int] = None, cap_win: Optional[int] = None):
        dev = ctx.device
        self.ctx = ctx
        per_table = [min(int(max_window), n) for n in ctx.table_rows]
        self.cap_uniq = int(cap_uniq) if cap_uniq is not None else max(16, sum(per_table))
        slots_cap = [min(u, ctx.ways * p) for u, p in zip(per_table, ctx.cache_sets)]
        self.cap_win = int(cap_win) if cap_win is not None else max(16, sum(slots_cap))
        i64, i32, u8 = torch.int64, torch.int32, torch.uint8
        z = lambda n, dt: torch.zeros(max(int(n), 1), dtype=dt, device=dev)
        e = lambda n, dt: torch.empty(max(int(n), 1), dtype=dt, device=dev)
        T = ctx.T
        self.bitmap = z(ctx.total_bm_words, i64)
        self.uniq = e(self.cap_uniq, i64)
        self.uniq_off = z(T + 1, i64)
        self.prot = z(ctx.total_sets, i64)
        self.hit = e((self.cap_uniq + 15) // 16 * 16, u8)
        self.kept = e(self.cap_uniq, i32)
        self.kept_off = z(T + 1, i64)
        self.way = e((self.cap_uniq + 15) // 16 * 16, u8)
        self.flags = z((self.cap_uniq + 15) // 16 * 16, u8)
        self.winner = torch.full((ctx.total_rows,), -1, dtype=i32, device=dev)
        self.win_claim = e(self.cap_win, i32)
        self.win_idx = e(self.cap_win, i64)
        self.win_row = e(self.cap_win, i64)
        self.win_tag = e(self.cap_win, i64)
        self.win_off = z(T + 1, i64)
        self.stage = torch.empty((self.cap_win, ctx.D), dtype=torch.float32, device=dev)
        self.ev_tag = torch.full((self.cap_win,), -1, dtype=i64, device=dev)
        self.count = self.claim = None         # the "fill" insert policy's buffers (_fill_buffers)
        self.c = Plan(self.bitmap.data_ptr(), self.uniq.data_ptr(), self.uniq_off.data_ptr(), self.cap_uniq,
                      self.prot.data_ptr(), self.hit.data_ptr(), self.kept.data_ptr(), self.kept_off.data_ptr(),
                      self.way.data_ptr(), self.flags.data_ptr(), self.winner.data_ptr(), self.win_claim.data_ptr(),
                      self.win_idx.data_ptr(), self.win_row.data_ptr(), self.win_tag.data_ptr(),
                      self.win_off.data_ptr(), self.cap_win, self.stage.data_ptr(), self.ev_tag.data_ptr())

    # K1
    def unique(self, idx: torch.Tensor, stream=None):
        _require_cuda(idx, "window indices")
        assert idx.dtype == torch.int64 and idx.dim() == 2 and idx.shape[0] == self.ctx.T and idx.stride(1) == 1
        check(_lib.lib().cdlrm_window_unique(self.ctx.handle, C.byref(self.c), idx.data_ptr(), idx.shape[1],
                                             idx.stride(0), stream_ptr(stream)))

    def unique_add(self, idx: torch.Tensor, stream=None):
        """Streamed K1: fold one chunk [T, n] of the window into the bitmap (any number of chunks, then unique_finish)."""
        _require_cuda(idx, "window indices")
        assert idx.dtype == torch.int64 and idx.dim() == 2 and idx.shape[0] == self.ctx.T and idx.stride(1) == 1
        check(_lib.lib().cdlrm_window_unique_add(self.ctx.handle, C.byref(self.c), idx.data_ptr(), idx.shape[1],
                                                 idx.stride(0), stream_ptr(stream)))

    def unique_finish(self, stream=None):
        check(_lib.lib().cdlrm_window_unique_finish(self.ctx.handle, C.byref(self.c), stream_ptr(stream)))

    def set_unique(self, uniqs: Sequence[torch.Tensor]):
        """CacheEmbeddings drop-in entry: the caller already has the sorted unique lists."""
        off = [0]
        for u in uniqs:
            off.append(off[-1] + int(u.numel()))
        if off[-1] > self.cap_uniq:
            raise RuntimeError("plan capacity %d < %d unique indices" % (self.cap_uniq, off[-1]))
        if off[-1]:
            self.uniq[:off[-1]] = torch.cat([u.reshape(-1).to(self.uniq.device, torch.int64) for u in uniqs])
        self.uniq_off.copy_(torch.tensor(off, dtype=torch.int64))

    # K2
    def probe(self, stream=None):
        check(_lib.lib().cdlrm_plan_probe(self.ctx.handle, C.byref(self.c), stream_ptr(stream)))

    def offsets(self, stream=None):
        """(uniq_off, kept_off, win_off) as python lists; synchronises the stream."""
        T = self.ctx.T
        bufs = [(C.c_int64 * (T + 1))() for _ in range(3)]
        check(_lib.lib().cdlrm_plan_offsets_sync(self.ctx.handle, C.byref(self.c), bufs[0], bufs[1], bufs[2],
                                                 stream_ptr(stream)))
        return [list(b) for b in bufs]

    # K3
    def assign(self, q: Optional[torch.Tensor] = None, seed: int = 0, stream=None):
        if q is not None:
            _require_cuda(q, "q")
            assert q.dtype == torch.float32 and q.is_contiguous()
        check(_lib.lib().cdlrm_plan_assign(self.ctx.handle, C.byref(self.c), ptr(q), int(seed) & (2 ** 64 - 1),
                                           stream_ptr(stream)))

    # K3, "fill" insert policy (cdlrm_plan_assign_fill in the header): its two extra buffers exist from the first use on
    def _fill_buffers(self):
        if self.count is None:
            dev = self.ctx.device
            self.count = torch.zeros(max(self.cap_uniq, 1), dtype=torch.int32, device=dev)
            self.claim = torch.zeros(max(int(self.ctx.total_sets), 1), dtype=torch.int64, device=dev)
            torch.cuda.current_stream(dev).synchronize()       # (zeroed on the current stream, used on the plan's)

    def count_reset(self, stream=None):
        self._fill_buffers()
        check(_lib.lib().cdlrm_plan_count_reset(self.ctx.handle, C.byref(self.c), self.count.data_ptr(), stream_ptr(stream)))

    def count_add(self, idx: torch.Tensor, stream=None):
        """Add the lookups of one chunk [T, n] of the window to the per-unique counters (after unique / unique_finish)."""
        _require_cuda(idx, "window indices")
        assert idx.dtype == torch.int64 and idx.dim() == 2 and idx.shape[0] == self.ctx.T and idx.stride(1) == 1
        self._fill_buffers()
        check(_lib.lib().cdlrm_plan_count_add(self.ctx.handle, C.byref(self.c), idx.data_ptr(), idx.shape[1], idx.stride(0),
                                              self.count.data_ptr(), stream_ptr(stream)))

    def assign_fill(self, use_counts: bool = True, stream=None):
        """Instead of assign(): the collision-free, frequency-ranked policy (use_counts=False: index order)."""
        self._fill_buffers()
        check(_lib.lib().cdlrm_plan_assign_fill(self.ctx.handle, C.byref(self.c), self.count.data_ptr() if use_counts else None,
                                                self.claim.data_ptr(), stream_ptr(stream)))

    # K5a
    def fetch(self, src_ptrs: Sequence[int], by_position: bool, stream=None):
        arr = (C.c_void_p * self.ctx.T)(*[int(p) for p in src_ptrs])
        check(_lib.lib().cdlrm_plan_fetch(self.ctx.handle, C.byref(self.c), arr, 1 if by_position else 0,
                                          stream_ptr(stream)))

    def victims(self, victims: "Victims", stream=None, list_only: bool = False):
        """After assign(): list the window's indices that stay outside the cache and fetch their host rows
        (list_only: the caller moves the rows itself -- host_gather_rows + one DMA copy)."""
        fn = _lib.lib().cdlrm_plan_victims_list if list_only else _lib.lib().cdlrm_plan_victims
        check(fn(self.ctx.handle, C.byref(self.c), C.byref(victims.c), stream_ptr(stream)))

    # K4 + K5b
    def commit(self, stream=None):
        check(_lib.lib().cdlrm_plan_commit(self.ctx.handle, C.byref(self.c), stream_ptr(stream)))

    # K14
    def writeback(self, dst_ptrs: Sequence[int], average: bool, stream=None):
        arr = (C.c_void_p * self.ctx.T)(*[int(p) for p in dst_ptrs])
        check(_lib.lib().cdlrm_plan_writeback(self.ctx.handle, C.byref(self.c), arr, 1 if average else 0,
                                              stream_ptr(stream)))


class Victims:
    """Caller-owned buffers of one window's victim rows (cdlrm_victims in the header)."""

    def __init__(self, ctx: CacheCtx, cap: int):
        dev = ctx.device
        self.cap = max(1, int(cap))
        self.pos = torch.empty(self.cap, dtype=torch.int32, device=dev)
        self.idx = torch.zeros(self.cap, dtype=torch.int64, device=dev)
        self.off = torch.zeros(ctx.T + 2, dtype=torch.int64, device=dev)     # [T + 1] offsets + the un-capped list length
        self.rows = torch.empty((self.cap, ctx.D), dtype=torch.float32, device=dev)
        self.c = _VictimsStruct(self.pos.data_ptr(), self.idx.data_ptr(), self.off.data_ptr(), self.rows.data_ptr(),
                                self.cap)


def host_gather_rows(table_ptrs: Sequence[int], idx: torch.Tensor, off: Sequence[int], dim: int, dst: torch.Tensor,
                     threads: int = 16):
    """HOST-side gather (CPU threads, releases the GIL): dst[j] = table_{t(j)}[idx[j]] for j < off[-1].  idx: CPU int64,
    dst: CPU fp32 [>= off[-1], dim] (pinned for the DMA that follows)."""
    T = len(table_ptrs)
    assert idx.device.type == "cpu" and idx.dtype == torch.int64 and idx.is_contiguous()
    assert dst.device.type == "cpu" and dst.dtype == torch.float32 and dst.is_contiguous() and dst.shape[1] == dim
    assert len(off) == T + 1 and off[-1] <= idx.numel() and off[-1] <= dst.shape[0]
    tp = (C.c_void_p * T)(*[int(p) for p in table_ptrs])
    oa = (C.c_int64 * (T + 1))(*[int(o) for o in off])
    check(_lib.lib().cdlrm_host_gather_rows(tp, idx.data_ptr(), oa, T, int(dim), dst.data_ptr(), int(threads)))


def gather_rows(src_ptr: int, index: torch.Tensor, dim: int, stream=None) -> torch.Tensor:
    _require_cuda(index, "index")
    out = torch.empty((index.numel(), dim), dtype=torch.float32, device=index.device)
    check(_lib.lib().cdlrm_gather_rows(int(src_ptr), index.data_ptr(), index.numel(), dim, out.data_ptr(),
                                       stream_ptr(stream)))
    return out


# ---- table aggregation -------------------------------------------------------------------------------

def agg_compact(ctx: CacheCtx, touched: torch.Tensor, rows_out: torch.Tensor, count_out: torch.Tensor, stream=None):
    check(_lib.lib().cdlrm_agg_compact(ctx.handle, touched.data_ptr(), touched.numel(), rows_out.data_ptr(),
                                       rows_out.numel(), count_out.data_ptr(), stream_ptr(stream)))


def agg_gather(ctx: CacheCtx, rows: torch.Tensor, count: torch.Tensor, scale: float, buf: torch.Tensor, cap: int,
               stream=None, first: int = 0):
    """buf[i] = weight[rows[i]] / scale for i < min(count - first, cap): `rows` points at entry `first` of the list
    whose length is the device word `count` (chunked merges pass slices)."""
    check(_lib.lib().cdlrm_agg_gather(ctx.handle, rows.data_ptr(), count.data_ptr(), float(scale), buf.data_ptr(),
                                      int(cap), int(first), stream_ptr(stream)))


def agg_scatter(ctx: CacheCtx, rows: torch.Tensor, count: torch.Tensor, buf: torch.Tensor, cap: int, stream=None,
                first: int = 0):
    check(_lib.lib().cdlrm_agg_scatter(ctx.handle, rows.data_ptr(), count.data_ptr(), buf.data_ptr(), int(cap),
                                       int(first), stream_ptr(stream)))


def agg_mark_tier(ctx: CacheCtx, slots: torch.Tensor, value: int, tier: torch.Tensor, stream=None):
    """tier[row] = value for every cache slot the [T, n] view of resolved slot ids names (cdlrm_agg_mark_tier)."""
    assert slots.dtype == torch.int32 and slots.dim() == 2 and slots.shape[0] == ctx.T and slots.stride(1) == 1
    assert tier.dtype == torch.uint8 and tier.numel() == ctx.total_rows
    check(_lib.lib().cdlrm_agg_mark_tier(ctx.handle, slots.data_ptr(), slots.shape[1], slots.stride(0), int(value),
                                         tier.data_ptr(), stream_ptr(stream)))


def agg_split(ctx: CacheCtx, rows: torch.Tensor, count: int, tier: torch.Tensor, n_classes: int, rows_out: torch.Tensor,
              class_off: torch.Tensor, stream=None):
    """Stable counting sort of the merge's row list by tier byte (cdlrm_agg_split); class_off: int64 [n_classes + 1] on the device."""
    assert rows.dtype == torch.int64 and rows_out.dtype == torch.int64 and rows_out.numel() >= count
    assert class_off.dtype == torch.int64 and class_off.numel() >= n_classes + 1
    check(_lib.lib().cdlrm_agg_split(ctx.handle, rows.data_ptr(), int(count), tier.data_ptr(), int(n_classes), rows_out.data_ptr(),
                                     class_off.data_ptr(), stream_ptr(stream)))


# ---- dense model -------------------------------------------------------------------------------------

def interact_fwd(feat: torch.Tensor, itself: bool, R: torch.Tensor, stream=None):
    B, F, D = feat.shape
    check(_lib.lib().cdlrm_interact_fwd(feat.data_ptr(), B, F, D, int(bool(itself)), R.data_ptr(), R.stride(0),
                                        stream_ptr(stream)))


def interact_bwd(feat: torch.Tensor, dR: torch.Tensor, itself: bool, dfeat: torch.Tensor, stream=None, x_act: int = 0):
    """x_act: activation that produced feature 0 (the bottom MLP's output); its gradient row then leaves as the
    pre-activation gradient."""
    B, F, D = feat.shape
    check(_lib.lib().cdlrm_interact_bwd(feat.data_ptr(), dR.data_ptr(), dR.stride(0), B, F, D, int(bool(itself)),
                                        int(x_act), dfeat.data_ptr(), stream_ptr(stream)))


def gather_interact_supported(ctx: CacheCtx) -> bool:
    """Shapes the fused gather + interaction kernels take (D in 32 / 64 / 128 / 256, 16 < T + 1 <= 32)."""
    return bool(_lib.raw().cdlrm_gather_interact_supported(ctx.handle))      # (a query: never on a step's tape)


def gather_interact_fwd(ctx: CacheCtx, slots: torch.Tensor, x: torch.Tensor, itself: bool, R: torch.Tensor, stream=None):
    """Cached EmbeddingBag forward (Criteo layout) + dot interaction in one launch: x [B, D] (any row pitch) is feature 0,
    features 1 .. T are the cache rows `slots` [T, n] names.  Bit-identical to embbag_fwd + interact_fwd."""
    B = x.shape[0]
    assert slots.dtype == torch.int32 and slots.stride(1) == 1 and x.stride(1) == 1
    check(_lib.lib().cdlrm_gather_interact_fwd(ctx.handle, slots.data_ptr(), slots.stride(0), x.data_ptr(), x.stride(0), B,
                                               int(bool(itself)), R.data_ptr(), R.stride(0), stream_ptr(stream)))


def gather_interact_bwd(ctx: CacheCtx, slots: torch.Tensor, x: torch.Tensor, dR: torch.Tensor, itself: bool,
                        dfeat: torch.Tensor, stream=None, x_act: int = 0):
    """interact_bwd with the rows read again from the cache (before the batch's embedding update rewrites them)."""
    B = x.shape[0]
    assert slots.dtype == torch.int32 and slots.stride(1) == 1 and x.stride(1) == 1 and dfeat.is_contiguous()
    check(_lib.lib().cdlrm_gather_interact_bwd(ctx.handle, slots.data_ptr(), slots.stride(0), x.data_ptr(), x.stride(0),
                                               dR.data_ptr(), dR.stride(0), B, int(bool(itself)), int(x_act),
                                               dfeat.data_ptr(), stream_ptr(stream)))


def gather_interact_bwd_sgd(ctx: CacheCtx, slots: torch.Tensor, x: torch.Tensor, dR: torch.Tensor, itself: bool,
                            dfeat: torch.Tensor, once: int, ld_once: int, lr: float, stream=None, x_act: int = 0):
    """gather_interact_bwd + the SGD step of the slots the batch reads once (their gradient rows are not written).  once: address
    of the sort's flags (embbag_bwd_once_flags, ld_once = n; embbag_bwd_sorted_views, ld_once = nb * n).  embbag_bwd_apply_rest /
    embbag_bwd_apply_sorted(rest=True) does the other slots."""
    B = x.shape[0]
    assert slots.dtype == torch.int32 and slots.stride(1) == 1 and x.stride(1) == 1 and dfeat.is_contiguous()
    check(_lib.lib().cdlrm_gather_interact_bwd_sgd(ctx.handle, slots.data_ptr(), slots.stride(0), x.data_ptr(), x.stride(0),
                                                   dR.data_ptr(), dR.stride(0), B, int(bool(itself)), int(x_act),
                                                   dfeat.data_ptr(), int(once), int(ld_once), _rate(lr), stream_ptr(stream)))


IA_OPS = {"fwd": 0, "bwd": 1, "gather_fwd": 2, "gather_bwd": 3, "gather_bwd_sgd": 4}
IA_FAMILIES = {1: "generic", 2: "row", 3: "slab", 4: "slab_db"}


def interact_route(op: str, B: int, F: int, D: int, itself: bool, ld_r: int, aligned_r: bool = True,
                   aligned_dfeat: bool = True) -> dict:
    """The kernel one interaction call launches, from the same decision code, without launching it: op of IA_OPS on B samples
    of F features (T + 1 for the gather ops) of D columns, ld_r the row pitch of R (forward) / dR (backward), aligned_r /
    aligned_dfeat whether R / dR and dfeat are 16-byte aligned.  family (IA_FAMILIES), d4, ns, grid (under the current
    cdlrm_debug_set values) and lds_bytes; a shape the call refuses raises its error.  No device is touched."""
    out = _lib.InteractRoute()
    check(_lib.raw().cdlrm_interact_route(IA_OPS[op], int(B), int(F), int(D), int(bool(itself)), int(ld_r),
                                          int(bool(aligned_r)) | int(bool(aligned_dfeat)) << 1, C.byref(out)))
    return {"family": IA_FAMILIES[out.family], "d4": out.d4, "ns": out.ns, "grid": out.grid, "lds_bytes": out.lds_bytes}


ACT = {"none": 0, "relu": 1, "sigmoid": 2}


GEMM_ALONE = 0x100        # include/cdlrm_hip.h: CDLRM_GEMM_ALONE
GEMM_BF16 = 0x200         # include/cdlrm_hip.h: CDLRM_GEMM_BF16
GEMM_BF16X3 = 0x400       # include/cdlrm_hip.h: CDLRM_GEMM_BF16X3
PRECISIONS = {"fp32": 0, "bf16": GEMM_BF16, "bf16x3": GEMM_BF16X3}


def bf16_eligible(N: int, K: int) -> bool:
    """The shape rule of the bf16 and bf16x3 modes (CDLRM_GEMM_BF16 / CDLRM_GEMM_BF16X3): a layer with N outputs and K inputs
    runs its GEMMs in the mode when K >= 32 and N >= 32; other layers keep their fp32 routes."""
    return int(N) >= 32 and int(K) >= 32


def _flags(alone: bool = False, bf16: bool = False, precision: Optional[str] = None) -> int:
    assert precision is None or not bf16, "bf16= and precision= are two spellings of one choice: pass one"
    return (GEMM_ALONE if alone else 0) | (GEMM_BF16 if bf16 else 0) | (PRECISIONS[precision] if precision else 0)


def linear_fwd(X: torch.Tensor, W: torch.Tensor, b: Optional[torch.Tensor], Y: torch.Tensor, act: int, stream=None,
               alone: bool = False, bf16: bool = False, precision: Optional[str] = None):
    """alone: no other GEMM runs beside this launch (scheduling hint, CDLRM_GEMM_ALONE).  bf16: the opt-in bf16 matrix-core
    mode (CDLRM_GEMM_BF16: X and W rounded once to bf16 inside the kernel, fp32 accumulation; eligible shapes only).
    precision: a key of PRECISIONS instead of bf16= ("bf16" is bf16=True; "bf16x3": CDLRM_GEMM_BF16X3, X and W split into two
    bf16 planes each, three exact products per product, near-fp32 results)."""
    M, K = X.shape
    N = W.shape[0]
    assert W.shape[1] == K and W.is_contiguous() and X.stride(1) == 1 and Y.stride(1) == 1
    check(_lib.lib().cdlrm_linear_fwd(X.data_ptr(), X.stride(0), W.data_ptr(), ptr(b), Y.data_ptr(), Y.stride(0), M, N,
                                      K, act | _flags(alone, bf16, precision), stream_ptr(stream)))


def linear_bwd_work(M: int, N: int, K: int, device) -> torch.Tensor:
    nbytes = int(_lib.lib().cdlrm_linear_bwd_work_bytes(M, N, K))
    return torch.empty((nbytes + 255) // 256 * 256, dtype=torch.uint8, device=device)


def linear_bwd(X, W, Y, dY, dX, dW, db, act: int, work: torch.Tensor, stream=None, x_act: int = 0, alone: bool = False,
               bf16: bool = False, precision: Optional[str] = None):
    """act: this layer's activation, applied backward to dY in place (0: dY already is the pre-activation
    gradient).  x_act: the activation that produced X; dX then leaves as the layer below's pre-activation gradient.
    bf16, precision: as linear_fwd (dgrad operands dZ and W, weight-gradient operands dZ and X)."""
    M, K = X.shape
    N = W.shape[0]
    check(_lib.lib().cdlrm_linear_bwd(X.data_ptr(), X.stride(0), W.data_ptr(), ptr(Y), 0 if Y is None else Y.stride(0),
                                      dY.data_ptr(), dY.stride(0), ptr(dX), 0 if dX is None else dX.stride(0),
                                      ptr(dW), ptr(db), M, N, K, act | _flags(alone, bf16, precision), int(x_act), work.data_ptr(),
                                      stream_ptr(stream)))


ROUTE_FAMILIES = {0: None, 1: "smallk_rows", 2: "smallk", 3: "direct", 4: "staged", 5: "gemm2", 6: "gemm3", 7: "gemm",
                  8: "bf16", 9: "bf16x3"}


def _route(r: _lib.GemmRoute) -> Optional[dict]:
    fam = ROUTE_FAMILIES[r.family]
    if fam is None:
        return None
    return dict(family=fam, tm=r.tm, tn=r.tn, mode=r.mode, aligned=r.aligned, splits=r.splits, vec_a=r.vec_a, vec_b=r.vec_b,
                fast=r.fast)


def linear_fwd_route(X, W, b, Y, act: int, alone: bool = False, n_cu: int = 256, bf16: bool = False,
                     precision: Optional[str] = None) -> dict:
    """The kernel linear_fwd(X, W, b, Y, act, alone=alone) launches, from the same decision code, without launching it:
    family (ROUTE_FAMILIES), tile (tm, tn), direct mode / aligned, splits, vec_a / vec_b, fast (the full-tile epilogue).
    X, W, b, Y: tensors or anything with .shape, .stride(0) and .data_ptr() -- addresses are looked at for their alignment
    only, no device is touched.  n_cu: the compute-unit count of the device the rule is evaluated for (MI355X: 256)."""
    M, K = X.shape
    N = W.shape[0]
    out = _lib.GemmRoute()
    check(_lib.raw().cdlrm_linear_fwd_route(X.data_ptr(), X.stride(0), W.data_ptr(), ptr(b), Y.data_ptr(), Y.stride(0), M, N, K,
                                            act | _flags(alone, bf16, precision), None, int(n_cu), C.byref(out)))
    return _route(out)


def linear_bwd_route(X, W, Y, dY, dX, dW, db, act: int, x_act: int = 0, alone: bool = False, n_cu: int = 256,
                     bf16: bool = False, precision: Optional[str] = None):
    """(dgrad, wgrad): the kernels linear_bwd with the same arguments launches for dX and for dW / db (None where it launches
    none), as linear_fwd_route."""
    M, K = X.shape
    N = W.shape[0]
    out = (_lib.GemmRoute * 2)()
    check(_lib.raw().cdlrm_linear_bwd_route(X.data_ptr(), X.stride(0), W.data_ptr(), ptr(Y), 0 if Y is None else Y.stride(0),
                                            dY.data_ptr(), dY.stride(0), ptr(dX), 0 if dX is None else dX.stride(0), ptr(dW),
                                            ptr(db), M, N, K, act | _flags(alone, bf16, precision), int(x_act), 256, None,
                                            int(n_cu), out))
    return _route(out[0]), _route(out[1])


def _wgrad_work_bytes(M: int, Ns, Ks, precision: str) -> int:
    n = len(Ns)
    NA = C.c_int32 * n
    N, K = NA(*[int(x) for x in Ns]), NA(*[int(x) for x in Ks])
    return int(_lib.lib().cdlrm_mlp_wgrad_work_bytes_ex(n, int(M), N, K, PRECISIONS[precision]))


def mlp_wgrad_work(M: int, Ns: Sequence[int], Ks: Sequence[int], device, precision: str = "fp32") -> torch.Tensor:
    """Scratch for mlp_wgrad over layers with output widths Ns and input widths Ks at batch M (precision: that of the plan)."""
    nbytes = _wgrad_work_bytes(M, Ns, Ks, precision)
    return torch.empty((nbytes + 255) // 256 * 256, dtype=torch.uint8, device=device)


class WgradPlan:
    """Host-side argument block of cdlrm_mlp_wgrad for a fixed set of layers and buffers (built once per batch shape;
    `set_x` re-points one layer's input, e.g. the dense features of the current batch).  precision: "fp32", or "bf16" /
    "bf16x3" for the opt-in modes of the eligible layers (K >= 32 and N >= 32; work from mlp_wgrad_work(..., precision=...))."""

    def __init__(self, Xs, dZs, dWs, dbs, work: torch.Tensor, precision: str = "fp32"):
        import ctypes as C
        assert precision in PRECISIONS, precision
        self.precision = precision
        n = len(Xs)
        assert len(dZs) == n and len(dWs) == n and len(dbs) == n
        self.n = n
        self.M = int(dZs[0].shape[0])
        self._keep = (list(Xs), list(dZs), list(dWs), list(dbs), work)
        PA, IA, NA = C.c_void_p * n, C.c_int64 * n, C.c_int32 * n
        self.X = PA(*[x.data_ptr() for x in Xs])
        self.ld_x = IA(*[x.stride(0) for x in Xs])
        self.dZ = PA(*[d.data_ptr() for d in dZs])
        self.ld_dz = IA(*[d.stride(0) for d in dZs])
        self.dW = PA(*[w.data_ptr() for w in dWs])
        self.db = PA(*[ptr(b) for b in dbs])
        self.N = NA(*[int(w.shape[0]) for w in dWs])
        self.K = NA(*[int(w.shape[1]) for w in dWs])
        for x, d, w in zip(Xs, dZs, dWs):
            assert x.shape[0] == self.M and d.shape[0] == self.M and x.stride(1) == 1 and d.stride(1) == 1
            assert w.is_contiguous() and d.shape[1] == w.shape[0] and x.shape[1] <= w.shape[1] <= x.stride(0)
        need = _wgrad_work_bytes(self.M, list(self.N), list(self.K), precision)
        assert work.numel() * work.element_size() >= need and work.data_ptr() % 256 == 0, "work too small: ops.mlp_wgrad_work"
        self.work = work

    def set_x(self, i: int, x: torch.Tensor):
        assert x.shape[0] == self.M and x.stride(1) == 1
        self.X[i] = x.data_ptr()
        self.ld_x[i] = x.stride(0)
        self._keep[0][i] = x

    def set_params(self, Ws, bs):
        """The layers' parameters (W[i] [N, K] contiguous, b[i] [N] or None), for mlp_wgrad(..., lr=): the SGD step then
        happens in the weight-gradient launches."""
        import ctypes as C
        assert len(Ws) == self.n and len(bs) == self.n
        for i, w in enumerate(Ws):
            assert w.is_contiguous() and tuple(w.shape) == (int(self.N[i]), int(self.K[i]))
        PA = C.c_void_p * self.n
        self.P_w = PA(*[w.data_ptr() for w in Ws])
        self.P_b = PA(*[ptr(b) for b in bs])
        self._params = (list(Ws), list(bs))

    def set_state(self, SWs, Sbs):
        """The accumulators of the parameters set_params named (same shapes), for mlp_wgrad(..., lr=, opt=("adagrad", eps))."""
        import ctypes as C
        assert len(SWs) == self.n and len(Sbs) == self.n
        for i, (s, w) in enumerate(zip(SWs, self._params[0])):
            assert s.is_contiguous() and s.shape == w.shape and s.dtype == torch.float32
        for s, b in zip(Sbs, self._params[1]):
            assert (s is None) == (b is None) and (s is None or s.numel() == b.numel())
        PA = C.c_void_p * self.n
        self.S_w = PA(*[s.data_ptr() for s in SWs])
        self.S_b = PA(*[ptr(s) for s in Sbs])
        self._state = (list(SWs), list(Sbs))


DENSE_OPTS = {"sgd": 0, "adagrad": 1}     # CDLRM_DENSE_OPT_*


def mlp_wgrad(plan: WgradPlan, stream=None, lr: Optional[float] = None, opt=None):
    """dW[i] = dZ[i]^T X[i], db[i] = column sums of dZ[i] for every layer of the plan (one grouped launch at small M).
    lr given (and plan.set_params called): W[i] -= lr * dW[i], b[i] -= lr * db[i] in the same launches.
    opt = (name, eps) with lr (and plan.set_state called): the step of that dense optimizer (DENSE_OPTS) in their place."""
    flags = PRECISIONS[plan.precision]          # 0: exactly cdlrm_mlp_wgrad / cdlrm_mlp_wgrad_sgd
    if opt is not None:
        assert lr is not None, "the optimizer's step rides with lr"
        name, eps = opt
        adagrad = DENSE_OPTS[name] != 0
        check(_lib.lib().cdlrm_mlp_wgrad_opt_ex(plan.n, plan.X, plan.ld_x, plan.dZ, plan.ld_dz, plan.dW, plan.db, plan.P_w,
                                                plan.P_b, _rate(lr), plan.M, plan.N, plan.K, flags, DENSE_OPTS[name], float(eps),
                                                plan.S_w if adagrad else None, plan.S_b if adagrad else None,
                                                plan.work.data_ptr(), stream_ptr(stream)))
    elif lr is None:
        check(_lib.lib().cdlrm_mlp_wgrad_ex(plan.n, plan.X, plan.ld_x, plan.dZ, plan.ld_dz, plan.dW, plan.db, plan.M, plan.N,
                                            plan.K, flags, plan.work.data_ptr(), stream_ptr(stream)))
    else:
        check(_lib.lib().cdlrm_mlp_wgrad_sgd_ex(plan.n, plan.X, plan.ld_x, plan.dZ, plan.ld_dz, plan.dW, plan.db, plan.P_w,
                                                plan.P_b, _rate(lr), plan.M, plan.N, plan.K, flags, plan.work.data_ptr(),
                                                stream_ptr(stream)))


def mlp_wgrad_route(plan: WgradPlan, n_cu: int = 256, precision: Optional[str] = None) -> list:
    """One route per layer of the plan (as linear_fwd_route's dict): the weight-gradient GEMM mlp_wgrad(plan) launches for it,
    from the same decision code, without launching.  precision: the plan's unless given."""
    out = (_lib.GemmRoute * max(plan.n, 1))()
    flags = PRECISIONS[precision or plan.precision]
    check(_lib.raw().cdlrm_mlp_wgrad_route(plan.n, plan.X, plan.ld_x, plan.dZ, plan.ld_dz, plan.dW, plan.db, plan.M, plan.N,
                                           plan.K, flags, int(n_cu), out))
    return [_route(out[i]) for i in range(plan.n)]


def bce_fwd_bwd(Z: torch.Tensor, target: torch.Tensor, loss_buf: torch.Tensor, dZ: Optional[torch.Tensor], stream=None,
                sigmoid_bwd: bool = False):
    assert loss_buf.numel() >= 65
    check(_lib.lib().cdlrm_bce_fwd_bwd(Z.data_ptr(), target.data_ptr(), Z.numel(), loss_buf.data_ptr(), ptr(dZ),
                                       1 if sigmoid_bwd else 0, stream_ptr(stream)))


LOSS = {"bce": 0, "mse": 1, "wbce": 2}


def loss_fwd_bwd(Z: torch.Tensor, target: torch.Tensor, loss_buf: torch.Tensor, dZ: Optional[torch.Tensor], *,
                 kind: int = 0, weights=(1.0, 1.0), threshold: float = 0.0, Zc: Optional[torch.Tensor] = None,
                 sigmoid_bwd: bool = False, stream=None):
    """loss_fn_wrap (main_no_ddp.py:212-221) with every arm + the --loss-threshold clamp (model_no_ddp.py:311-314)."""
    check(_lib.lib().cdlrm_loss_fwd_bwd(Z.data_ptr(), target.data_ptr(), Z.numel(), int(kind), float(weights[0]),
                                        float(weights[1]), float(threshold), loss_buf.data_ptr(), ptr(dZ), ptr(Zc),
                                        1 if sigmoid_bwd else 0, stream_ptr(stream)))


def head_scratch(device) -> torch.Tensor:
    return torch.zeros(int(_lib.lib().cdlrm_head_scratch_floats()), dtype=torch.float32, device=device)


def head_fwd_bwd(Y: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor], target: torch.Tensor, Z: torch.Tensor,
                 dZ: torch.Tensor, dY: Optional[torch.Tensor], loss_buf: torch.Tensor, scratch: torch.Tensor, *,
                 x_act: int = 0, kind: int = 0, weights=(1.0, 1.0), threshold: float = 0.0,
                 Zc: Optional[torch.Tensor] = None, finish: bool = True, stream=None):
    """Last top layer (out_features 1, sigmoid) + loss + the layer's input gradient in one launch.  finish=False leaves
    the loss as partial sums in `scratch`: head_finish() on a stream ordered behind this call completes loss_buf."""
    B, K = Y.shape
    assert Y.stride(1) == 1 and w.numel() >= K and Z.numel() == B and dZ.numel() == B and target.numel() == B
    assert dY is None or (dY.shape == Y.shape and dY.stride(1) == 1)
    check(_lib.lib().cdlrm_head_fwd_bwd(Y.data_ptr(), Y.stride(0), w.data_ptr(), ptr(bias), target.data_ptr(), B, K,
                                        int(kind), float(weights[0]), float(weights[1]), float(threshold), int(x_act),
                                        Z.data_ptr(), ptr(Zc), dZ.data_ptr(), ptr(dY), 0 if dY is None else dY.stride(0),
                                        loss_buf.data_ptr(), scratch.data_ptr(), 1 if finish else 0, stream_ptr(stream)))


def head_route(B: int, K: int, ldy: int, lddy: int, aligned: int = 7, has_dY: bool = True, finish: bool = True) -> dict:
    """What one head_fwd_bwd call launches, from the same decision code, without launching it.  aligned: bit 0 = Y is 16-byte
    aligned, bit 1 = w, bit 2 = dY (has_dY False: lddy and bit 2 are not looked at).  path: "one" (a float4 per lane, K <= 256),
    "multi" (float4 trips of 256 columns) or "scalar"; tail: the launch completes loss_buf itself; finish_launch: head_finish is
    launched behind it; grid workgroups of 16 rows, passes = ceil(B / (16 * grid)).  No device is touched."""
    out = _lib.HeadRoute()
    check(_lib.raw().cdlrm_head_route(int(B), int(K), int(ldy), int(lddy), int(aligned), int(bool(has_dY)), int(bool(finish)),
                                      C.byref(out)))
    return {"path": "one" if out.one else "multi" if out.vec else "scalar", "vec": bool(out.vec), "tail": bool(out.tail),
            "finish_launch": bool(out.finish_launch), "grid": out.grid, "passes": out.passes}


def head_finish(scratch: torch.Tensor, B: int, loss_buf: torch.Tensor, stream=None, acc: Optional[torch.Tensor] = None):
    """acc: float64 [2] on the device, += [correct predictions, loss * B] of this batch."""
    assert acc is None or (acc.dtype == torch.float64 and acc.numel() >= 2 and acc.is_contiguous())
    check(_lib.lib().cdlrm_head_finish(scratch.data_ptr(), int(B), loss_buf.data_ptr(), ptr(acc), stream_ptr(stream)))


def act_bwd(dX: torch.Tensor, X: torch.Tensor, act: int, stream=None):
    """dX *= act'(X) in place over a 2-D block (views with row pitches allowed)."""
    assert dX.shape == X.shape and dX.dim() == 2 and dX.stride(1) == 1 and X.stride(1) == 1
    check(_lib.lib().cdlrm_act_bwd(dX.data_ptr(), dX.stride(0), X.data_ptr(), X.stride(0), X.shape[0], X.shape[1],
                                   int(act), stream_ptr(stream)))


def sgd_step2(param: torch.Tensor, grad: torch.Tensor, off0: int, n0: int, off1: int, n1: int, lr: float, stream=None):
    assert param.is_contiguous() and grad.is_contiguous() and param.numel() == grad.numel()
    assert 0 <= off0 and off0 + n0 <= param.numel() and 0 <= off1 and off1 + n1 <= param.numel()
    check(_lib.lib().cdlrm_sgd_step2(param.data_ptr(), grad.data_ptr(), int(off0), int(n0), int(off1), int(n1), _rate(lr),
                                     stream_ptr(stream)))


def _check_dense_state(param, grad, state, opt):
    assert param.is_contiguous() and grad.is_contiguous() and param.numel() == grad.numel()
    if DENSE_OPTS[opt] != 0:
        assert state is not None and state.is_contiguous() and state.dtype == torch.float32 and state.numel() == param.numel()


def dense_opt_step(param: torch.Tensor, grad: torch.Tensor, state: Optional[torch.Tensor], lr: float, opt: str, eps: float,
                   stream=None):
    """sgd_step with the dense optimizer named (DENSE_OPTS): "adagrad" steps `state` (param's layout) and param."""
    _check_dense_state(param, grad, state, opt)
    check(_lib.lib().cdlrm_dense_opt_step(param.data_ptr(), grad.data_ptr(), ptr(state), param.numel(), _rate(lr),
                                          DENSE_OPTS[opt], float(eps), stream_ptr(stream)))


def dense_opt_step2(param: torch.Tensor, grad: torch.Tensor, state: Optional[torch.Tensor], off0: int, n0: int, off1: int,
                    n1: int, lr: float, opt: str, eps: float, stream=None):
    """sgd_step2 with the dense optimizer named: two disjoint ranges of the flat buffers in one launch."""
    _check_dense_state(param, grad, state, opt)
    assert 0 <= off0 and off0 + n0 <= param.numel() and 0 <= off1 and off1 + n1 <= param.numel()
    check(_lib.lib().cdlrm_dense_opt_step2(param.data_ptr(), grad.data_ptr(), ptr(state), int(off0), int(n0), int(off1),
                                           int(n1), _rate(lr), DENSE_OPTS[opt], float(eps), stream_ptr(stream)))


def scale_div(x: torch.Tensor, divisor: float, stream=None):
    assert x.is_contiguous()
    check(_lib.lib().cdlrm_scale_div(x.data_ptr(), x.numel(), float(divisor), stream_ptr(stream)))


def scatter_rows(dst_ptr: int, index: torch.Tensor, rows: torch.Tensor, average: bool, stream=None,
                 distinct: bool = True):
    """dst[index[i]] = rows[i] (or the average with the old row).  distinct=False: the list may repeat an index (the
    reference's eviction lists do): the averaging arm then blends every entry against the OLD destination row first
    (cdlrm_blend_rows) and scatters the blended rows -- repeats carry identical rows, so the result is defined."""
    _require_cuda(index, "index"); _require_cuda(rows, "rows")
    assert rows.is_contiguous() and index.is_contiguous() and index.dtype == torch.int64
    if average and not distinct:
        out = torch.empty_like(rows)
        check(_lib.lib().cdlrm_blend_rows(int(dst_ptr), index.data_ptr(), rows.data_ptr(), index.numel(), rows.shape[1],
                                          out.data_ptr(), stream_ptr(stream)))
        rows, average = out, False
    check(_lib.lib().cdlrm_scatter_rows(int(dst_ptr), index.data_ptr(), rows.data_ptr(), index.numel(), rows.shape[1],
                                        1 if average else 0, stream_ptr(stream)))


def bags_window(buf: torch.Tensor, bpos: torch.Tensor, L: int, n_win: int, out: Optional[torch.Tensor] = None,
                stream=None) -> torch.Tensor:
    """int64 [T, n_win] window rectangle (engine.pad_window's contract) of a device window buffer: buf int64 [total], bpos
    int64 [(L + 1) * T] (include/cdlrm_hip.h: cdlrm_bags_window)."""
    _require_cuda(buf, "buf"); _require_cuda(bpos, "bpos")
    assert buf.dtype == torch.int64 and bpos.dtype == torch.int64 and buf.is_contiguous() and bpos.is_contiguous()
    T = bpos.numel() // (L + 1)
    assert bpos.numel() == (L + 1) * T
    if out is None:
        out = torch.empty(T, n_win, dtype=torch.int64, device=buf.device)
    assert out.shape == (T, n_win) and out.is_contiguous() and out.dtype == torch.int64
    check(_lib.lib().cdlrm_bags_window(buf.data_ptr(), buf.numel(), bpos.data_ptr(), L, T, n_win, out.data_ptr(),
                                       stream_ptr(stream)))
    return out


def bags_rank_slice(buf: torch.Tensor, bpos: torch.Tensor, L: int, b: int, off: torch.Tensor, s0: int, s1: int, n: int,
                    stream=None):
    """Batch b of a device window buffer, a rank's samples [s0, s1) -> (off int64 [T, s1 - s0 + 1], idx int64 [T, n]): the
    layout engine.square_bags() gives the rank's rebased lookups (include/cdlrm_hip.h: cdlrm_bags_rank_slice).  off: the
    batch's global offsets, int64 [T, nbag] on the device (a view of the window buffer may do)."""
    _require_cuda(buf, "buf"); _require_cuda(bpos, "bpos"); _require_cuda(off, "off")
    assert buf.dtype == torch.int64 and bpos.dtype == torch.int64 and off.dtype == torch.int64
    assert buf.is_contiguous() and bpos.is_contiguous() and off.is_contiguous() and off.dim() == 2
    T, nbag = off.shape
    assert bpos.numel() == (L + 1) * T
    idx = torch.empty(T, n, dtype=torch.int64, device=buf.device)
    off_out = torch.empty(T, s1 - s0 + 1, dtype=torch.int64, device=buf.device)
    check(_lib.lib().cdlrm_bags_rank_slice(buf.data_ptr(), buf.numel(), bpos.data_ptr(), L, b, T, off.data_ptr(), nbag, s0, s1,
                                           n, idx.data_ptr(), off_out.data_ptr(), stream_ptr(stream)))
    return off_out, idx


def dayfile_tile() -> int:
    """Samples per workgroup of `dayfile_window`'s kernel."""
    return int(_lib.lib().cdlrm_dayfile_tile())


def dayfile_window(x_int: torch.Tensor, x_cat: torch.Tensor, y: torch.Tensor, max_ind_range: int, X: torch.Tensor,
                   lS_i: torch.Tensor, T: torch.Tensor, col0: int = 0, stream=None) -> None:
    """n raw day-file rows on the device (x_int int32 [n, n_dense], x_cat int32 [n, n_cat], y int32 [n]) -> samples
    [col0, col0 + n) of a window: X fp32 [rows, n_dense] = log(x_int + 1), lS_i int64 [n_cat, pitch] = x_cat^T (floor-mod
    max_ind_range when > 0), T fp32 [rows] or [rows, 1] = y (include/cdlrm_hip.h: cdlrm_dayfile_window).  lS_i may be a
    column range of a wider rectangle (unit column stride); nothing outside the n samples is written."""
    for t, name in ((x_int, "x_int"), (x_cat, "x_cat"), (y, "y"), (X, "X"), (lS_i, "lS_i"), (T, "T")):
        _require_cuda(t, name)
    assert x_int.dtype == torch.int32 and x_cat.dtype == torch.int32 and y.dtype == torch.int32
    assert X.dtype == torch.float32 and T.dtype == torch.float32 and lS_i.dtype == torch.int64
    assert x_int.dim() == 2 and x_cat.dim() == 2 and y.dim() == 1 and X.dim() == 2 and lS_i.dim() == 2
    assert x_int.is_contiguous() and x_cat.is_contiguous() and y.is_contiguous() and X.is_contiguous() and T.is_contiguous()
    n, nd, nc = y.shape[0], x_int.shape[1], x_cat.shape[1]
    col0 = int(col0)
    assert x_int.shape[0] == n and x_cat.shape[0] == n and X.shape[1] == nd and lS_i.shape[0] == nc and nd >= 1 and nc >= 1
    assert col0 >= 0 and col0 + n <= X.shape[0] and col0 + n <= T.numel() and col0 + n <= lS_i.shape[1], \
        "samples [%d, %d) do not fit the window buffers" % (col0, col0 + n)
    assert lS_i.stride(1) == 1 or lS_i.shape[1] == 1
    pitch = lS_i.stride(0) if nc > 1 else lS_i.shape[1]
    assert pitch >= lS_i.shape[1]
    check(_lib.lib().cdlrm_dayfile_window(x_int.data_ptr(), x_cat.data_ptr(), y.data_ptr(), n, nd, nc, int(max_ind_range),
                                          X.data_ptr(), lS_i.data_ptr(), pitch, col0, T.data_ptr(), stream_ptr(stream)))


def rows_tile() -> int:
    """Samples per workgroup of `rows_window`'s kernel."""
    return int(_lib.lib().cdlrm_rows_tile())


def rows_window(x_int: torch.Tensor, x_cat: torch.Tensor, y: torch.Tensor, order: torch.Tensor, max_ind_range: int,
                X: torch.Tensor, lS_i: torch.Tensor, T: torch.Tensor, col0: int = 0, stream=None) -> None:
    """Rows order[0 .. n) of arrays that stay on the device (x_int int32 [n_rows, n_dense], x_cat int32 [n_rows, n_cat], y int32
    [n_rows]; order int64 [n], every entry in [0, n_rows) -- not checked here, nor by the kernel) -> samples [col0, col0 + n) of a
    window, with `dayfile_window`'s outputs and rules (include/cdlrm_hip.h: cdlrm_rows_window)."""
    for t, name in ((x_int, "x_int"), (x_cat, "x_cat"), (y, "y"), (order, "order"), (X, "X"), (lS_i, "lS_i"), (T, "T")):
        _require_cuda(t, name)
    assert x_int.dtype == torch.int32 and x_cat.dtype == torch.int32 and y.dtype == torch.int32 and order.dtype == torch.int64
    assert X.dtype == torch.float32 and T.dtype == torch.float32 and lS_i.dtype == torch.int64
    assert x_int.dim() == 2 and x_cat.dim() == 2 and y.dim() == 1 and order.dim() == 1 and X.dim() == 2 and lS_i.dim() == 2
    assert x_int.is_contiguous() and x_cat.is_contiguous() and y.is_contiguous() and order.is_contiguous()
    assert X.is_contiguous() and T.is_contiguous()
    n_rows, n, nd, nc = y.shape[0], order.shape[0], x_int.shape[1], x_cat.shape[1]
    col0 = int(col0)
    assert x_int.shape[0] == n_rows and x_cat.shape[0] == n_rows and n_rows >= 1
    assert X.shape[1] == nd and lS_i.shape[0] == nc and nd >= 1 and nc >= 1
    assert col0 >= 0 and col0 + n <= X.shape[0] and col0 + n <= T.numel() and col0 + n <= lS_i.shape[1], \
        "samples [%d, %d) do not fit the window buffers" % (col0, col0 + n)
    assert lS_i.stride(1) == 1 or lS_i.shape[1] == 1
    pitch = lS_i.stride(0) if nc > 1 else lS_i.shape[1]
    assert pitch >= lS_i.shape[1]
    check(_lib.lib().cdlrm_rows_window(x_int.data_ptr(), x_cat.data_ptr(), y.data_ptr(), n_rows, order.data_ptr(), n, nd, nc,
                                       int(max_ind_range), X.data_ptr(), lS_i.data_ptr(), pitch, col0, T.data_ptr(),
                                       stream_ptr(stream)))


def binfile_tile() -> int:
    """Samples per workgroup of `binfile_window`'s kernel."""
    return int(_lib.lib().cdlrm_binfile_tile())


def binfile_window(rec: torch.Tensor, n_dense: int, max_ind_range: int, X: torch.Tensor, lS_i: torch.Tensor, T: torch.Tensor,
                   col0: int = 0, stream=None) -> None:
    """n records of the MLPerf binary Criteo file on the device (rec int32 [n, 1 + n_dense + n_cat], a record =
    [y | dense | categorical]) -> samples [col0, col0 + n) of a window, with `dayfile_window`'s outputs and rules
    (include/cdlrm_hip.h: cdlrm_binfile_window)."""
    for t, name in ((rec, "rec"), (X, "X"), (lS_i, "lS_i"), (T, "T")):
        _require_cuda(t, name)
    assert rec.dtype == torch.int32 and X.dtype == torch.float32 and T.dtype == torch.float32 and lS_i.dtype == torch.int64
    assert rec.dim() == 2 and X.dim() == 2 and lS_i.dim() == 2
    assert rec.is_contiguous() and X.is_contiguous() and T.is_contiguous()
    n, nd = rec.shape[0], int(n_dense)
    nc = rec.shape[1] - 1 - nd
    col0 = int(col0)
    assert nd >= 1 and nc >= 1 and X.shape[1] == nd and lS_i.shape[0] == nc
    assert col0 >= 0 and col0 + n <= X.shape[0] and col0 + n <= T.numel() and col0 + n <= lS_i.shape[1], \
        "samples [%d, %d) do not fit the window buffers" % (col0, col0 + n)
    assert lS_i.stride(1) == 1 or lS_i.shape[1] == 1
    pitch = lS_i.stride(0) if nc > 1 else lS_i.shape[1]
    assert pitch >= lS_i.shape[1]
    check(_lib.lib().cdlrm_binfile_window(rec.data_ptr(), n, nd, nc, int(max_ind_range), X.data_ptr(), lS_i.data_ptr(), pitch,
                                          col0, T.data_ptr(), stream_ptr(stream)))


# ---- raw Criteo text (cdlrm_amd/data_utils.py; include/cdlrm_hip.h: cdlrm_etl_*) -----------------------------------

ETL_N_DENSE, ETL_N_CAT = 13, 26
ETL_NO_ERROR = -1          # the error word as int64: all ones = no error
ETL_CODES = {1: "not exactly 40 tab-separated fields", 2: "a decimal field holds a byte outside [0-9] (one leading - allowed)",
             3: "a decimal field does not fit int32", 4: "a hex field holds a byte outside [0-9a-fA-F]",
             5: "a hex field has more than 8 digits", 6: "a value is missing from its column's dictionary",
             7: "a line span outside the text buffer"}


def etl_error_word(device) -> torch.Tensor:
    """A fresh device error word (int64 [1], all ones = no error) for the `etl_*` calls."""
    return torch.full((1,), ETL_NO_ERROR, dtype=torch.int64, device=device)


def etl_error(err: torch.Tensor):
    """None, or (1-based line / row number, code) of the FIRST malformed line the word has seen (synchronises)."""
    w = int(err.item())
    if w == ETL_NO_ERROR:
        return None
    w &= (1 << 64) - 1
    return w >> 8, w & 0xff


def etl_line_index(text: torch.Tensor, length: int = None, starts: torch.Tensor = None, count: torch.Tensor = None, stream=None):
    """text uint8 [>= length] on the device -> (starts int64 [cap + 1], count int64 [1]): starts[j] is the offset of line j,
    starts[count] one past the last newline; count = the lines that END inside text[:length] (cdlrm_etl_line_index)."""
    _require_cuda(text, "text")
    assert text.dtype == torch.uint8 and text.dim() == 1 and text.is_contiguous()
    n = text.numel() if length is None else int(length)
    assert 0 <= n <= text.numel()
    if starts is None:
        starts = torch.empty(n + 1, dtype=torch.int64, device=text.device)
    if count is None:
        count = torch.empty(1, dtype=torch.int64, device=text.device)
    assert starts.dtype == torch.int64 and starts.is_contiguous() and starts.numel() >= 1 and count.dtype == torch.int64
    L = _lib.lib()
    work = torch.empty(int(L.cdlrm_etl_line_index_work_bytes(n)), dtype=torch.uint8, device=text.device)
    check(L.cdlrm_etl_line_index(text.data_ptr(), n, starts.data_ptr(), starts.numel() - 1, count.data_ptr(), work.data_ptr(),
                                 work.numel(), stream_ptr(stream)))
    return starts, count


def etl_parse(text: torch.Tensor, length: int, starts: torch.Tensor, n: int, line0: int, max_ind_range: int, y: torch.Tensor,
              x_int: torch.Tensor, x_cat: torch.Tensor, err: torch.Tensor, row0: int = 0, stream=None) -> None:
    """Lines [0, n) of `etl_line_index`'s starts -> rows [row0, row0 + n) of y [*], x_int [*, 13], x_cat [*, 26] (int32);
    line0: the file's 0-based number of line 0 (cdlrm_etl_parse)."""
    for t, name in ((text, "text"), (starts, "starts"), (y, "y"), (x_int, "x_int"), (x_cat, "x_cat"), (err, "err")):
        _require_cuda(t, name)
        assert t.is_contiguous(), name
    assert text.dtype == torch.uint8 and starts.dtype == torch.int64 and err.dtype == torch.int64 and err.numel() == 1
    assert y.dtype == x_int.dtype == x_cat.dtype == torch.int32
    assert 0 <= length <= text.numel() and 0 <= n and starts.numel() >= n + 1
    assert x_int.dim() == 2 and x_int.shape[1] == ETL_N_DENSE and x_cat.dim() == 2 and x_cat.shape[1] == ETL_N_CAT
    assert row0 >= 0 and row0 + n <= min(y.numel(), x_int.shape[0], x_cat.shape[0]), "rows [%d, %d) do not fit" % (row0, row0 + n)
    check(_lib.lib().cdlrm_etl_parse(text.data_ptr(), int(length), starts.data_ptr(), int(n), int(line0), int(max_ind_range),
                                     y.data_ptr() + 4 * row0, x_int.data_ptr() + 4 * ETL_N_DENSE * row0,
                                     x_cat.data_ptr() + 4 * ETL_N_CAT * row0, err.data_ptr(), stream_ptr(stream)))


def etl_subsample(y: torch.Tensor, x_int: torch.Tensor, x_cat: torch.Tensor, n: int, rand_u: torch.Tensor, line0: int, rate: float,
                  out_y: torch.Tensor, out_x_int: torch.Tensor, out_x_cat: torch.Tensor, rows_in: torch.Tensor,
                  rows_out: torch.Tensor, stream=None) -> None:
    """Rows [0, n) -> the kept ones, in order, behind row rows_in[0] of the out arrays; rows_out[0] = rows_in[0] + kept
    (int64 [1] each, two different tensors).  Row i is dropped iff y[i] == 0 and rand_u[line0 + i] < rate (cdlrm_etl_subsample)."""
    for t, name in ((y, "y"), (x_int, "x_int"), (x_cat, "x_cat"), (rand_u, "rand_u"), (out_y, "out_y"), (out_x_int, "out_x_int"),
                    (out_x_cat, "out_x_cat"), (rows_in, "rows_in"), (rows_out, "rows_out")):
        _require_cuda(t, name)
        assert t.is_contiguous(), name
    assert y.dtype == x_int.dtype == x_cat.dtype == out_y.dtype == out_x_int.dtype == out_x_cat.dtype == torch.int32
    assert rand_u.dtype == torch.float64 and rows_in.dtype == rows_out.dtype == torch.int64
    assert 0 <= n <= min(y.numel(), x_int.shape[0], x_cat.shape[0])
    assert x_int.shape[1] == out_x_int.shape[1] == ETL_N_DENSE and x_cat.shape[1] == out_x_cat.shape[1] == ETL_N_CAT
    out_cap = min(out_y.numel(), out_x_int.shape[0], out_x_cat.shape[0])
    L = _lib.lib()
    work = torch.empty(int(L.cdlrm_etl_subsample_work_bytes(n)), dtype=torch.uint8, device=y.device)
    check(L.cdlrm_etl_subsample(y.data_ptr(), x_int.data_ptr(), x_cat.data_ptr(), int(n), rand_u.data_ptr(), rand_u.numel(),
                                int(line0), float(rate), out_y.data_ptr(), out_x_int.data_ptr(), out_x_cat.data_ptr(), out_cap,
                                rows_in.data_ptr(), rows_out.data_ptr(), work.data_ptr(), work.numel(), stream_ptr(stream)))


def etl_encode(x_cat: torch.Tensor, col: int, keys: torch.Tensor, ids: torch.Tensor, err: torch.Tensor, n: int = None,
               row0: int = 0, stream=None) -> None:
    """Column `col` of x_cat int32 [*, n_cols], rows [0, n), in place: value -> ids[k] with keys[k] == value; keys int32
    ascending, ids int32 beside them (cdlrm_etl_encode)."""
    for t, name in ((x_cat, "x_cat"), (keys, "keys"), (ids, "ids"), (err, "err")):
        _require_cuda(t, name)
        assert t.is_contiguous(), name
    assert x_cat.dtype == keys.dtype == ids.dtype == torch.int32 and err.dtype == torch.int64 and err.numel() == 1
    assert x_cat.dim() == 2 and keys.dim() == 1 and keys.shape == ids.shape
    n = x_cat.shape[0] if n is None else int(n)
    assert 0 <= n <= x_cat.shape[0]
    check(_lib.lib().cdlrm_etl_encode(x_cat.data_ptr(), n, x_cat.shape[1], int(col), keys.data_ptr(), ids.data_ptr(), keys.numel(),
                                      int(row0), err.data_ptr(), stream_ptr(stream)))


def mark_rows(ctx: CacheCtx, slots: torch.Tensor, touched: torch.Tensor, stream=None):
    assert slots.dtype == torch.int32 and slots.is_contiguous() and slots.shape[0] == ctx.T
    check(_lib.lib().cdlrm_mark_rows(ctx.handle, slots.data_ptr(), slots.shape[1], touched.data_ptr(),
                                     stream_ptr(stream)))


def sgd_step(param: torch.Tensor, grad: torch.Tensor, lr: float, stream=None):
    assert param.is_contiguous() and grad.is_contiguous() and param.numel() == grad.numel()
    check(_lib.lib().cdlrm_sgd_step(param.data_ptr(), grad.data_ptr(), param.numel(), _rate(lr), stream_ptr(stream)))


def roc_auc(scores: torch.Tensor, targets: torch.Tensor) -> float:
    """Area under the ROC curve of `scores` against binary `targets`, on the device the scores live on: the Mann-Whitney rank
    sum with average ranks for tied scores (= sklearn.metrics.roc_auc_score), float64 accumulation.  The rank-0 test loop's
    second figure beside the accuracy (the reference parses --mlperf-auc-threshold, main_no_ddp.py:119-120,
    and never computes the AUC).  NaN when only one class is present."""
    s = scores.reshape(-1).to(torch.float32)
    t = targets.reshape(-1).to(s.device) > 0.5
    n = s.numel()
    n_pos = int(t.sum())
    n_neg = n - n_pos
    if n_pos == 0 or n_neg == 0:
        return float("nan")
    order = torch.argsort(s, stable=True)
    ss = s[order]
    # average rank of every run of equal scores: (first + last) / 2 of its 1-based positions
    new = torch.ones(n, dtype=torch.bool, device=s.device)
    new[1:] = ss[1:] != ss[:-1]
    run_id = torch.cumsum(new.to(torch.int64), 0) - 1
    first = torch.nonzero(new).reshape(-1)
    last = torch.cat([first[1:], torch.tensor([n], device=s.device)]) - 1
    avg_rank = ((first + last).to(torch.float64) * 0.5 + 1.0)[run_id]
    rank_sum_pos = avg_rank[t[order]].sum()
    u = rank_sum_pos - n_pos * (n_pos + 1) / 2.0
    return float(u / (float(n_pos) * float(n_neg)))
