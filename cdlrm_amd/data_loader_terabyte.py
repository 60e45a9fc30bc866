"""Reader of the pre-processed Criteo day files, mirroring the reference's `data_loader_terabyte.DataLoader`
(data_loader_terabyte.py:19-172): `<dir>/<name>_<day>_reordered.npz` with X_int [n, 13], X_cat [n, 26], y [n] and
`<dir>/<name>_day_count.npz` with total_per_file.  A batch is the tuple the trainer loop consumes,

    (X fp32 [B, 13] = log(X_int + 1),  lS_o int64 [26, B] = arange(B) per row,  lS_i int64 [26, B] = X_cat^T,  T fp32 [B, 1])

(`_transform_features`, :68-87).  Batching quirks kept: batches run across day-file boundaries (the tail of a file is
carried into the first batch of the next), a file's rows are consumed while `start < rows - batch_size` (strict, :115
-- a tail of exactly batch_size rows is carried over too), "test" reads the first half of each file and "val" the
second half (:107-112), and the last short batch is emitted unless drop_last_batch.  `DataLoader` is host-side only: no GPU
work.

`batch_segments` is the same batch geometry as arithmetic on the file lengths alone, and `DeviceDayLoader` (opt-in:
`--day-file-loader=device`) hands out the same batches from HBM: the raw int32 rows of a whole look-ahead window are uploaded
ahead of their use and cut into (X, lS_i, T) by one kernel (csrc/dayfile.hip), in the layout the synthetic front end hands
out -- a step gets views, no copy, no launch."""
from __future__ import annotations

import math
import os
from concurrent.futures import ThreadPoolExecutor
from typing import Iterator, List, Sequence, Tuple

import numpy as np
import torch

from . import ops

Batch = Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]


def transform_features(x_int: np.ndarray, x_cat: np.ndarray, y: np.ndarray, max_ind_range: int) -> Batch:
    """data_loader_terabyte.py:68-87."""
    if max_ind_range > 0:
        x_cat = x_cat % max_ind_range
    X = torch.log(torch.as_tensor(np.asarray(x_int), dtype=torch.float) + 1)
    cat = torch.as_tensor(np.asarray(x_cat), dtype=torch.long)
    T = torch.as_tensor(np.asarray(y), dtype=torch.float32).view(-1, 1)
    B, F = cat.shape[0], cat.shape[1]
    lS_o = torch.arange(B).reshape(1, -1).repeat(F, 1)
    return X, lS_o, cat.t(), T


class DataLoader:
    def __init__(self, data_filename: str, data_directory: str, days: Sequence[int], batch_size: int,
                 max_ind_range: int = -1, split: str = "train", drop_last_batch: bool = False):
        self.data_filename, self.data_directory = data_filename, data_directory
        self.days, self.batch_size, self.max_ind_range = list(days), int(batch_size), int(max_ind_range)
        with np.load(os.path.join(data_directory, data_filename + "_day_count.npz")) as data:
            total = int(sum(data["total_per_file"][np.array(self.days)]))
        self.length = int(np.ceil(total / 2.)) if split in ("test", "val") else total
        self.split, self.drop_last_batch = split, drop_last_batch

    def __len__(self) -> int:
        return self.length // self.batch_size if self.drop_last_batch else math.ceil(self.length / self.batch_size)

    def __iter__(self) -> Iterator[Batch]:
        B = self.batch_size
        carry = None            # rows left over from the previous file(s): (x_int, x_cat, y)
        for day in self.days:
            path = os.path.join(self.data_directory, "%s_%d_reordered.npz" % (self.data_filename, day))
            with np.load(path) as data:
                x_int, x_cat, y = data["X_int"], data["X_cat"], data["y"]
            end, start = y.shape[0], 0
            if self.split in ("test", "val"):
                half = int(np.ceil(end / 2.))
                if self.split == "test":
                    end = half
                else:
                    start = end - half
            while start < end - B:
                take = B - (carry[2].shape[0] if carry is not None else 0)
                sl = slice(start, start + take)
                xi, xc, yy = x_int[sl], x_cat[sl], y[sl]
                if carry is not None:
                    xi, xc, yy = (np.concatenate([carry[0], xi]), np.concatenate([carry[1], xc]),
                                  np.concatenate([carry[2], yy]))
                    carry = None
                if xi.shape[0] != B:
                    raise ValueError("should not happen")
                yield transform_features(xi, xc, yy, self.max_ind_range)
                start += take
            if start != end:
                sl = slice(start, end)
                carry = (x_int[sl], x_cat[sl], y[sl]) if carry is None else (
                    np.concatenate([carry[0], x_int[sl]]), np.concatenate([carry[1], x_cat[sl]]),
                    np.concatenate([carry[2], y[sl]]))
        if not self.drop_last_batch and carry is not None:
            yield transform_features(carry[0], carry[1], carry[2], self.max_ind_range)


Segment = Tuple[int, int, int]      # (day, first row, row behind the last)


def batch_segments(rows_per_file, days: Sequence[int], batch_size: int, split: str = "train",
                   drop_last_batch: bool = False) -> List[List[Segment]]:
    """The batches `DataLoader.__iter__` yields, as row ranges: for every batch the list of (day, start, stop) it is made of,
    in order.  rows_per_file[day] = rows of that day's file.  Arithmetic on file lengths only, by the rules of
    data_loader_terabyte.py:95-172: the tail of a file is carried into the next file's first batch, a file gives batches
    while `start < end - B` (strict), "test" is the first half of each file and "val" the second, the last short batch is
    kept unless dropped.  Raises where the host loader raises ("should not happen": files whose range is not longer than B
    have let the carry grow past a batch); a carry that is still there at the end is reported as the host loader yields it,
    even when it is longer than B."""
    B = int(batch_size)
    out: List[List[Segment]] = []
    carry: List[Segment] = []
    carry_n = 0
    for day in days:
        end, start = int(rows_per_file[day]), 0
        if split in ("test", "val"):
            half = int(np.ceil(end / 2.))
            if split == "test":
                end = half
            else:
                start = end - half
        while start < end - B:
            take = B - carry_n
            if take < 0:
                raise ValueError("should not happen")
            segs = carry + ([(day, start, start + take)] if take else [])
            carry, carry_n = [], 0
            out.append(segs)
            start += take
        if start != end:
            carry.append((day, start, end))
            carry_n += end - start
    if not drop_last_batch and carry:
        out.append(carry)
    return out


class DeviceBatch(tuple):
    """(X, lS_o, lS_i, T) of `DeviceDayLoader`, every tensor on the device, plus the window it is a part of: `window_rect`
    = the window's whole int64 [n_cat, rows] index rectangle, `win_pos` = this batch's number inside it, `win_batches` = batches
    in the window.  `wait_upload(stream)` orders another stream than the one the batch was handed out on behind the window's
    upload (and keeps the window's buffers from being reused before what that stream has been given by then)."""

    def wait_upload(self, stream) -> None:
        stream.wait_event(self._slot["ev"])
        self._slot["consumers"].add(stream)


class DeviceDayLoader:
    """`DataLoader`'s batches, produced on the device a look-ahead window at a time.  Same constructor arguments plus `device`
    and `window` (batches per upload; the last window of an epoch may be shorter), same `__len__`, same tuples -- as
    `DeviceBatch`es whose tensors are views of their window's buffers: lS_i = columns [j*B, (j+1)*B) of the window's int64
    [n_cat, window*B] rectangle (as `_SyntheticLoader`'s), X / T = rows of its [window*B, n_dense] / [window*B, 1], lS_o one
    shared arange(B).repeat(n_cat, 1).

    Upload: a helper thread copies the raw int32 rows of a window's file segments into pinned staging, `copy_(non_blocking)`s
    them to HBM on the loader's own stream and launches `ops.dayfile_window` there, one launch per piece with its column
    offset, then records the window's event.  A piece is a file segment, cut at STAGE_BATCHES batches (a window of the README
    configuration is 3000 batches = 3.9 GB of raw rows: staging two whole windows would pin 8 GB); the pinned ring is two pieces
    deep, and a piece is refilled only after the host has seen the event behind the kernel that read it -- a wait of the helper
    thread, never of the training thread.  The window after the one being handed out is uploaded ahead: copy and kernel
    overlap training.  The stream a window's first batch is handed out on waits for the window's event once; no device-wide or
    stream synchronise anywhere.

    Ring rule.  The device ring is RING = 3 windows deep, which is what `main_no_ddp.Run` needs: it pulls a whole window of
    batches at once and, with the look-ahead plan, the next window's too before the current one has trained, and one more is
    being uploaded -- training, planned, uploading.  Upload u + 1 is started when the first batch of window u is handed out and
    overwrites window u - 2: a batch, and anything made from its window, may be read until the first batch of the window TWO
    after its own has been asked for.  The reuse is ordered on the device, not by a host wait: when a slot is recycled, an
    event is recorded on every stream that consumed its old window (the hand-out stream, every `wait_upload` stream and the
    current one) and the copy stream waits for them -- by then every step of the old window has been issued.

    Day files are opened with np.load, whole arrays in host memory (as the reference does).  A last batch longer than
    batch_size (files not longer than a batch at the end of the list, which the host loader yields as they are) is refused
    with a ValueError naming the file."""

    RING = 3
    STAGE_BATCHES = 64

    def __init__(self, data_filename: str, data_directory: str, days: Sequence[int], batch_size: int,
                 max_ind_range: int = -1, split: str = "train", drop_last_batch: bool = False, device="cuda", window: int = 1):
        self.data_filename, self.data_directory = data_filename, data_directory
        self.days, self.batch_size, self.max_ind_range = list(days), int(batch_size), int(max_ind_range)
        with np.load(os.path.join(data_directory, data_filename + "_day_count.npz")) as data:
            self.rows_per_file = [int(n) for n in data["total_per_file"]]
        total = int(sum(self.rows_per_file[d] for d in self.days))
        self.length = int(np.ceil(total / 2.)) if split in ("test", "val") else total
        self.split, self.drop_last_batch = split, drop_last_batch
        self.device, self.window = torch.device(device), max(1, int(window))
        self.batches = batch_segments(self.rows_per_file, self.days, self.batch_size, split, drop_last_batch)
        if self.batches and sum(b - a for _, a, b in self.batches[-1]) > self.batch_size:
            raise ValueError("%s: the last batch would hold %d rows, more than the batch size %d (day files not longer than a "
                             "batch at the end of the list)" % (self._path(self.batches[-1][-1][0]),
                                                                sum(b - a for _, a, b in self.batches[-1]), self.batch_size))
        self._slots = None
        self._uploads = 0           # windows uploaded so far, over all epochs: upload u lives in slot u % RING
        self._file = (None, None)   # (day, (X_int, X_cat, y)) of the day file in host memory

    def __len__(self) -> int:
        return self.length // self.batch_size if self.drop_last_batch else math.ceil(self.length / self.batch_size)

    def _path(self, day: int) -> str:
        return os.path.join(self.data_directory, "%s_%d_reordered.npz" % (self.data_filename, day))

    def _day(self, day: int):
        if self._file[0] != day:
            with np.load(self._path(day)) as data:
                arrs = tuple(np.ascontiguousarray(data[k], dtype=np.int32) for k in ("X_int", "X_cat", "y"))
            if arrs[2].shape[0] != self.rows_per_file[day] or arrs[0].shape[0] != arrs[2].shape[0] or \
                    arrs[1].shape[0] != arrs[2].shape[0]:
                raise ValueError("%s holds %d rows, %s_day_count.npz says %d" % (
                    self._path(day), arrs[2].shape[0], self.data_filename, self.rows_per_file[day]))
            self._file = (day, arrs)
        return self._file[1]

    def _setup(self):
        if self.device.type != "cuda":
            raise RuntimeError("cdlrm_amd: DeviceDayLoader needs the MI355X (got %s); the host loader is DataLoader" % self.device)
        xi, xc, _ = self._day(self.batches[0][0][0])
        self.n_dense, self.n_cat = int(xi.shape[1]), int(xc.shape[1])
        B, dev = self.batch_size, self.device
        W = min(self.window, len(self.batches)) * B
        width = self.n_dense + self.n_cat + 1
        self._stage_rows = min(W, self.STAGE_BATCHES * B)
        with torch.cuda.device(dev):
            self._copy = torch.cuda.Stream(device=dev)
            self._slots = [dict(X=torch.empty(W, self.n_dense, dtype=torch.float32, device=dev),
                                I=torch.empty(self.n_cat, W, dtype=torch.int64, device=dev),
                                T=torch.empty(W, 1, dtype=torch.float32, device=dev), ev=torch.cuda.Event(), consumers=set())
                           for _ in range(self.RING)]
            self._stage = [dict(host=torch.empty(self._stage_rows * width, dtype=torch.int32).pin_memory(),
                                dev=torch.empty(self._stage_rows * width, dtype=torch.int32, device=dev), ev=None)
                           for _ in range(2)]
        self._pieces = 0
        self._lS_o = torch.arange(B, device=dev).repeat(self.n_cat, 1)
        self._pool = ThreadPoolExecutor(max_workers=1, thread_name_prefix="dayfile-upload")

    def _submit(self, first_batch: int):
        """Start the upload of the window that begins at batch `first_batch` into the next ring slot (see the ring rule)."""
        slot = self._slots[self._uploads % self.RING]
        self._uploads += 1
        consumers, slot["consumers"] = slot["consumers"] | {torch.cuda.current_stream(self.device)}, set()
        released = []
        for st in consumers:
            e = torch.cuda.Event()
            e.record(st)
            released.append(e)
        return self._pool.submit(self._upload, slot, first_batch, released)

    def _upload(self, slot, first_batch: int, released):
        B, nd, nc = self.batch_size, self.n_dense, self.n_cat
        batches = self.batches[first_batch:first_batch + self.window]
        with torch.cuda.device(self.device), torch.cuda.stream(self._copy):
            for e in released:
                self._copy.wait_event(e)
            col = 0
            for segs in batches:
                for day, a, b in segs:
                    while a < b:
                        n = min(b - a, self._stage_rows)
                        xi, xc, y = self._day(day)
                        st = self._stage[self._pieces % 2]
                        self._pieces += 1
                        if st["ev"] is not None:
                            st["ev"].synchronize()      # (helper thread) the kernel that read this piece's last rows is done
                        h = st["host"].numpy()
                        o1, o2, o3 = n * nd, n * (nd + nc), n * (nd + nc + 1)
                        h[:o1].reshape(n, nd)[...] = xi[a:a + n]
                        h[o1:o2].reshape(n, nc)[...] = xc[a:a + n]
                        h[o2:o3] = y[a:a + n]
                        d = st["dev"]
                        d[:o3].copy_(st["host"][:o3], non_blocking=True)
                        ops.dayfile_window(d[:o1].view(n, nd), d[o1:o2].view(n, nc), d[o2:o3], self.max_ind_range, slot["X"],
                                           slot["I"], slot["T"], col0=col, stream=self._copy)
                        st["ev"] = torch.cuda.Event()
                        st["ev"].record(self._copy)
                        a, col = a + n, col + n
            slot["ev"].record(self._copy)
        return slot, col

    def __iter__(self) -> Iterator[DeviceBatch]:
        if not self.batches:
            return
        if self._slots is None:
            self._setup()
        B, L, nb = self.batch_size, self.window, len(self.batches)
        fut = self._submit(0)
        for w0 in range(0, nb, L):
            slot, rows = fut.result()
            fut = self._submit(w0 + L) if w0 + L < nb else None
            cur = torch.cuda.current_stream(self.device)
            cur.wait_event(slot["ev"])
            slot["consumers"].add(cur)
            nwin = min(L, nb - w0)
            rect = slot["I"][:, :rows]
            for j in range(nwin):
                r0, r1 = j * B, min((j + 1) * B, rows)
                lS_o = self._lS_o if r1 - r0 == B else torch.arange(r1 - r0, device=self.device).repeat(self.n_cat, 1)
                batch = DeviceBatch((slot["X"][r0:r1], lS_o, rect[:, r0:r1], slot["T"][r0:r1]))
                batch._slot, batch.window_rect, batch.win_pos, batch.win_batches = slot, rect, j, nwin
                yield batch
