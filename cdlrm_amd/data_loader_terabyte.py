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
out -- a step gets views, no copy, no launch.

The MLPerf binary files (`--mlperf-bin-loader`; data_loader_terabyte.py:195-275) are read by `CriteoBinDataset` / `BinLoader`
on the host and `DeviceBinLoader` on the device: one file per split, a record = [y, dense, categorical] int32, entry idx =
records [idx * B, (idx + 1) * B).  `bin_extents` is their batch geometry as arithmetic; the device loader shares its ring,
staging and hand-out with `DeviceDayLoader` (`_DeviceWindowLoader`) and cuts with csrc/binfile.hip.

The third dataset arm, the in-memory processed file, is data_loader_processed.py; its device loader takes the ring from here."""
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


Extent = Tuple[int, int]            # (first record, records)


def bin_extents(n_records: int, batch_size: int, order: Sequence[int] = None) -> List[Extent]:
    """The batches of a binary file of n_records records, as record ranges: entry idx = records [idx * B, (idx + 1) * B), cut at
    the end of the file (data_loader_terabyte.py:211, :226-227: ceil(n / B) entries, the last one short when B does not divide
    n).  `order`: the entries to list, in that order (a sampler's permutation); all of them in file order when None."""
    n, B = int(n_records), int(batch_size)
    if n < 0 or B < 1:
        raise ValueError("bin_extents: %d records in batches of %d" % (n, B))
    entries = -(-n // B)
    out = []
    for idx in (range(entries) if order is None else order):
        idx = int(idx)
        if not 0 <= idx < entries:
            raise IndexError("entry %d of a file of %d entries" % (idx, entries))
        out.append((idx * B, min(B, n - idx * B)))
    return out


class CriteoBinDataset:
    """The reference's binary Criteo dataset (data_loader_terabyte.py:195-235): `data_file` holds records [y, 13 dense,
    categorical] of int32 (160 bytes at the 26 categorical features of Criteo; here as many as `counts_file` lists), entry idx
    is the batch of records [idx * batch_size, (idx + 1) * batch_size) and `__getitem__` returns `transform_features` of
    them.  len = ceil(file bytes / bytes per batch): the last entry is short when the file does not divide.  A file that is not
    a whole number of records is refused (the reference would fail in `view` at its last entry)."""

    def __init__(self, data_file: str, counts_file: str, batch_size: int = 1, max_ind_range: int = -1,
                 bytes_per_feature: int = 4):
        if bytes_per_feature != 4:
            raise ValueError("%s: records of int32 only (bytes_per_feature = %d)" % (data_file, bytes_per_feature))
        with np.load(counts_file) as data:
            self.counts = data["counts"]
        self.tar_fea, self.den_fea, self.spa_fea = 1, 13, int(len(self.counts))
        self.tad_fea = self.tar_fea + self.den_fea
        self.tot_fea = self.tad_fea + self.spa_fea
        self.m_den = self.den_fea
        self.data_file, self.batch_size, self.max_ind_range = data_file, int(batch_size), int(max_ind_range)
        if self.batch_size < 1:
            raise ValueError("%s: batch size %d" % (data_file, self.batch_size))
        self.bytes_per_record = bytes_per_feature * self.tot_fea
        self.bytes_per_entry = self.bytes_per_record * self.batch_size
        if not os.path.isfile(data_file):
            raise FileNotFoundError("%s: no such binary Criteo file" % data_file)
        size = os.path.getsize(data_file)
        if size % self.bytes_per_record:
            raise ValueError("%s: %d bytes are not a whole number of %d-byte records (truncated?)"
                             % (data_file, size, self.bytes_per_record))
        self.n_records = size // self.bytes_per_record
        self.num_entries = math.ceil(size / self.bytes_per_entry)
        self.file = open(data_file, "rb", buffering=0)

    def __len__(self) -> int:
        return self.num_entries

    def read_into(self, buf, first_record: int, n_records: int) -> None:
        """Records [first_record, first_record + n_records) of the file into the writable buffer `buf`, which they fill."""
        view = memoryview(buf).cast("B")
        want, off = n_records * self.bytes_per_record, first_record * self.bytes_per_record
        if view.nbytes != want:
            raise ValueError("a buffer of %d bytes for %d records" % (view.nbytes, n_records))
        done = 0
        while done < want:
            got = os.preadv(self.file.fileno(), [view[done:]], off + done)
            if got <= 0:
                raise ValueError("%s ends inside record range [%d, %d)" % (self.data_file, first_record,
                                                                          first_record + n_records))
            done += got

    def __getitem__(self, idx: int) -> Batch:
        if not 0 <= idx < self.num_entries:
            raise IndexError(idx)
        first, n = idx * self.batch_size, min(self.batch_size, self.n_records - idx * self.batch_size)
        rec = np.empty((n, self.tot_fea), dtype=np.int32)
        self.read_into(rec, first, n)
        return transform_features(rec[:, 1:self.tad_fea], rec[:, self.tad_fea:], rec[:, 0], self.max_ind_range)


def _entry_order(dataset: CriteoBinDataset, shuffle: bool, drop_last_batch: bool, generator=None) -> List[int]:
    """The entries of one epoch.  Shuffled: what the reference's `DataLoader(train_data, batch_size=None,
    sampler=RandomSampler(train_data))` (dlrm_data_pytorch.py:411-421) visits, drawn by those very classes of torch over the
    entry numbers -- so the state of torch's generator decides the permutation exactly as it does there."""
    n = len(dataset)
    if shuffle:
        numbers = range(n)
        order = [int(i) for i in torch.utils.data.DataLoader(
            numbers, batch_size=None, sampler=torch.utils.data.RandomSampler(numbers, generator=generator), collate_fn=int)]
    else:
        order = list(range(n))
    if drop_last_batch and n and dataset.n_records % dataset.batch_size:
        order.remove(n - 1)
    return order


class BinLoader:
    """The entries of a `CriteoBinDataset` in file order, or (shuffle: `--mlperf-bin-shuffle`) in the order torch's
    RandomSampler gives, a fresh permutation per epoch (`_entry_order`).  Host-side only.  drop_last_batch leaves the short
    last entry out, wherever the permutation has it (the CLI's training loader: a step's batch is sliced across ranks)."""

    def __init__(self, dataset: CriteoBinDataset, shuffle: bool = False, drop_last_batch: bool = False, generator=None):
        self.dataset, self.shuffle, self.drop_last_batch, self.generator = dataset, bool(shuffle), drop_last_batch, generator

    def __len__(self) -> int:
        ds = self.dataset
        return ds.n_records // ds.batch_size if self.drop_last_batch else len(ds)

    def __iter__(self) -> Iterator[Batch]:
        for idx in _entry_order(self.dataset, self.shuffle, self.drop_last_batch, self.generator):
            yield self.dataset[idx]


class DeviceBatch(tuple):
    """(X, lS_o, lS_i, T) of `DeviceDayLoader`, every tensor on the device, plus the window it is a part of: `window_rect`
    = the window's whole int64 [n_cat, rows] index rectangle, `win_pos` = this batch's number inside it, `win_batches` = batches
    in the window.  `wait_upload(stream)` orders another stream than the one the batch was handed out on behind the window's
    upload (and keeps the window's buffers from being reused before what that stream has been given by then)."""

    def wait_upload(self, stream) -> None:
        stream.wait_event(self._slot["ev"])
        self._slot["consumers"].add(stream)


class _DeviceWindowLoader:
    """The part of the device loaders that does not depend on where the rows come from: the ring of RING window buffers, the
    pinned staging ring two pieces deep, the helper thread's upload of a window piece by piece on the loader's own stream, the
    events that order the reuse, and the hand-out of a window's batches as `DeviceBatch` views (`DeviceDayLoader` documents
    the rules).  A subclass sets batch_size, max_ind_range, device, window, n_dense, n_cat and gives the source:

        _pieces(batches)         the pieces of a window's batches, in order: (rows, source) with rows <= self._stage_rows
        _fill(h, rows, source)   write the piece's raw int32 dwords, rows * (n_dense + n_cat + 1) of them, to h (pinned)
        _cut(d, rows, slot, col) launch the kernel that cuts the piece's dwords d (device) into the slot at column col
        _rows(batch)             samples of one batch

    A loader whose rows are already on the device (data_loader_processed.DeviceProcessedLoader) takes the ring alone
    (`_setup_ring`) and brings an `_upload` of its own: no staging is allocated for it."""

    RING = 3
    STAGE_BATCHES = 64
    THREAD = "window-upload"

    _slots = None
    _uploads = 0                # windows uploaded so far, over all epochs: upload u lives in slot u % RING

    def _setup_ring(self, n_batches: int) -> int:
        """The loader's stream, the ring of window buffers, the shared lS_o and the helper thread; returns a window's rows."""
        B, dev = self.batch_size, self.device
        W = min(self.window, n_batches) * B
        with torch.cuda.device(dev):
            self._copy = torch.cuda.Stream(device=dev)
            self._slots = [dict(X=torch.empty(W, self.n_dense, dtype=torch.float32, device=dev),
                                I=torch.empty(self.n_cat, W, dtype=torch.int64, device=dev),
                                T=torch.empty(W, 1, dtype=torch.float32, device=dev), ev=torch.cuda.Event(), consumers=set())
                           for _ in range(self.RING)]
        self._lS_o = torch.arange(B, device=dev).repeat(self.n_cat, 1)
        self._pool = ThreadPoolExecutor(max_workers=1, thread_name_prefix=self.THREAD)
        return W

    def _setup(self, n_batches: int):
        B, dev = self.batch_size, self.device
        W = self._setup_ring(n_batches)
        width = self.n_dense + self.n_cat + 1
        self._stage_rows = min(W, self.STAGE_BATCHES * B)
        with torch.cuda.device(dev):
            self._stage = [dict(host=torch.empty(self._stage_rows * width, dtype=torch.int32).pin_memory(),
                                dev=torch.empty(self._stage_rows * width, dtype=torch.int32, device=dev), ev=None)
                           for _ in range(2)]
        self._pieces_done = 0

    def _submit(self, batches):
        """Start the upload of the window made of `batches` into the next ring slot (see the ring rule)."""
        slot = self._slots[self._uploads % self.RING]
        self._uploads += 1
        consumers, slot["consumers"] = slot["consumers"] | {torch.cuda.current_stream(self.device)}, set()
        released = []
        for st in consumers:
            e = torch.cuda.Event()
            e.record(st)
            released.append(e)
        return self._pool.submit(self._upload, slot, batches, released)

    def _upload(self, slot, batches, released):
        width = self.n_dense + self.n_cat + 1
        with torch.cuda.device(self.device), torch.cuda.stream(self._copy):
            for e in released:
                self._copy.wait_event(e)
            col = 0
            for n, source in self._pieces(batches):
                st = self._stage[self._pieces_done % 2]
                self._pieces_done += 1
                if st["ev"] is not None:
                    st["ev"].synchronize()      # (helper thread) the kernel that read this piece's last rows is done
                self._fill(st["host"].numpy(), n, source)
                d = st["dev"]
                d[:n * width].copy_(st["host"][:n * width], non_blocking=True)
                self._cut(d, n, slot, col)
                st["ev"] = torch.cuda.Event()
                st["ev"].record(self._copy)
                col += n
            slot["ev"].record(self._copy)
        return slot, col

    def _hand_out(self, batches) -> Iterator[DeviceBatch]:
        """The batches of one epoch (`batches`: the epoch's list, whatever `_pieces` and `_rows` read), window by window."""
        if not batches:
            return
        if self._slots is None:
            self._setup(len(batches))
        B, L, nb = self.batch_size, self.window, len(batches)
        fut = self._submit(batches[:L])
        for w0 in range(0, nb, L):
            slot, rows = fut.result()
            fut = self._submit(batches[w0 + L:w0 + 2 * L]) if w0 + L < nb else None
            cur = torch.cuda.current_stream(self.device)
            cur.wait_event(slot["ev"])
            slot["consumers"].add(cur)
            nwin = min(L, nb - w0)
            rect = slot["I"][:, :rows]
            r0 = 0
            for j in range(nwin):
                r1 = r0 + self._rows(batches[w0 + j])
                lS_o = self._lS_o if r1 - r0 == B else torch.arange(r1 - r0, device=self.device).repeat(self.n_cat, 1)
                batch = DeviceBatch((slot["X"][r0:r1], lS_o, rect[:, r0:r1], slot["T"][r0:r1]))
                batch._slot, batch.window_rect, batch.win_pos, batch.win_batches = slot, rect, j, nwin
                yield batch
                r0 = r1


class DeviceDayLoader(_DeviceWindowLoader):
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

    THREAD = "dayfile-upload"

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
        if self.batches and self._rows(self.batches[-1]) > self.batch_size:
            raise ValueError("%s: the last batch would hold %d rows, more than the batch size %d (day files not longer than a "
                             "batch at the end of the list)" % (self._path(self.batches[-1][-1][0]),
                                                                self._rows(self.batches[-1]), self.batch_size))
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

    @staticmethod
    def _rows(segs) -> int:
        return sum(b - a for _, a, b in segs)

    def _setup(self, n_batches: int):
        if self.device.type != "cuda":
            raise RuntimeError("cdlrm_amd: DeviceDayLoader needs the MI355X (got %s); the host loader is DataLoader" % self.device)
        xi, xc, _ = self._day(self.batches[0][0][0])
        self.n_dense, self.n_cat = int(xi.shape[1]), int(xc.shape[1])
        super()._setup(n_batches)

    def _pieces(self, batches):
        """A piece is a file segment, cut at STAGE_BATCHES batches: (rows, (day, first row))."""
        for segs in batches:
            for day, a, b in segs:
                while a < b:
                    n = min(b - a, self._stage_rows)
                    yield n, (day, a)
                    a += n

    def _fill(self, h, n, source):
        day, a = source
        xi, xc, y = self._day(day)
        nd, nc = self.n_dense, self.n_cat
        o1, o2, o3 = n * nd, n * (nd + nc), n * (nd + nc + 1)
        h[:o1].reshape(n, nd)[...] = xi[a:a + n]
        h[o1:o2].reshape(n, nc)[...] = xc[a:a + n]
        h[o2:o3] = y[a:a + n]

    def _cut(self, d, n, slot, col):
        nd, nc = self.n_dense, self.n_cat
        o1, o2, o3 = n * nd, n * (nd + nc), n * (nd + nc + 1)
        ops.dayfile_window(d[:o1].view(n, nd), d[o1:o2].view(n, nc), d[o2:o3], self.max_ind_range, slot["X"], slot["I"],
                           slot["T"], col0=col, stream=self._copy)

    def __iter__(self) -> Iterator[DeviceBatch]:
        return self._hand_out(self.batches)


class DeviceBinLoader(_DeviceWindowLoader):
    """`BinLoader`'s batches, produced on the device a look-ahead window at a time, with `DeviceDayLoader`'s contract exactly:
    `DeviceBatch` tuples whose tensors are views of their window's buffers, the RING = 3 rule, the pinned ring two pieces deep,
    uploads on the loader's own stream, reuse ordered by events, no device-wide or stream synchronise (the machinery is
    `_DeviceWindowLoader`, shared with the day-file loader).  The source differs: the raw records go from the file straight
    into the pinned stage (`os.preadv`, no array in between) and csrc/binfile.hip cuts them as they lie.

    Unshuffled, a window is ONE contiguous extent of the file, cut into pieces at STAGE_BATCHES batches; the short last batch
    of a file that does not divide is the last batch of the last window.  Shuffled, a window is `window` extents of one batch
    each, in the permutation's order (entries that happen to follow one another in the file are read as one piece).  The short
    last batch may then come anywhere in the epoch: its window holds fewer than window * B columns and the batches behind it
    start where it ends, not at a multiple of B -- `main_no_ddp.Run` resolves lookups per window for "whole batches only", so
    that one window trains without the resolver, as every short window does.  The permutation of an epoch is drawn when its
    first batch is asked for, by `_entry_order` as for `BinLoader`."""

    THREAD = "binfile-upload"

    def __init__(self, dataset: CriteoBinDataset, shuffle: bool = False, drop_last_batch: bool = False, generator=None,
                 device="cuda", window: int = 1):
        self.dataset, self.shuffle, self.drop_last_batch, self.generator = dataset, bool(shuffle), drop_last_batch, generator
        self.batch_size, self.max_ind_range = dataset.batch_size, dataset.max_ind_range
        self.n_dense, self.n_cat = dataset.den_fea, dataset.spa_fea
        self.device, self.window = torch.device(device), max(1, int(window))

    def __len__(self) -> int:
        ds = self.dataset
        return ds.n_records // ds.batch_size if self.drop_last_batch else len(ds)

    @staticmethod
    def _rows(extent) -> int:
        return extent[1]

    def _setup(self, n_batches: int):
        if self.device.type != "cuda":
            raise RuntimeError("cdlrm_amd: DeviceBinLoader needs the MI355X (got %s); the host loader is BinLoader" % self.device)
        super()._setup(n_batches)

    def _pieces(self, batches):
        """Extents that follow one another in the file are one extent; a piece is an extent cut at STAGE_BATCHES batches:
        (records, first record)."""
        k = 0
        while k < len(batches):
            a, b = batches[k][0], batches[k][0] + batches[k][1]
            k += 1
            while k < len(batches) and batches[k][0] == b:
                b += batches[k][1]
                k += 1
            while a < b:
                n = min(b - a, self._stage_rows)
                yield n, a
                a += n

    def _fill(self, h, n, first):
        self.dataset.read_into(h[:n * self.dataset.tot_fea], first, n)

    def _cut(self, d, n, slot, col):
        w = self.dataset.tot_fea
        ops.binfile_window(d[:n * w].view(n, w), self.n_dense, self.max_ind_range, slot["X"], slot["I"], slot["T"], col0=col,
                           stream=self._copy)

    def __iter__(self) -> Iterator[DeviceBatch]:
        ds = self.dataset
        order = _entry_order(ds, self.shuffle, self.drop_last_batch, self.generator)
        yield from self._hand_out(bin_extents(ds.n_records, ds.batch_size, order))
