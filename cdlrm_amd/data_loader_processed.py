"""The in-memory processed Criteo file, the reference's default `--data-generation=dataset` path (`CriteoDataset` without
`--memory-map`, dlrm_data_pytorch.py:47-320; `--data-set=kaggle` takes it): ONE `.npz` with X_int [n, 13], X_cat [n, 26],
y [n] and counts (`kaggleAdDisplayChallenge_processed.npz` / `terabyte_processed.npz`), split by the day counts of
`<dir>/<d_file>_day_count.npz` -- every day but the last trains, the last day's first half tests, its second half validates --
and ordered by `--data-randomize=total|day|none`; a plain torch DataLoader with `collate_wrapper_criteo` batches it (:323-338,
:493-545).  A batch is the tuple the trainer loop consumes, as `data_loader_terabyte` hands it out,

    (X fp32 [B, 13] = log(X_int + 1),  lS_o int64 [26, B] = arange(B) per row,  lS_i int64 [26, B] = X_cat^T,  T fp32 [B, 1]).

The reference re-lists the arrays row by row in the randomised order when the dataset is built.  Here the order is arithmetic
(`processed_order`: an int64 row order per split, drawing from numpy's generator exactly what one reference construction
draws), the file is read once (`ProcessedDataset`), and a loader is the order cut into batches: `ProcessedLoader` gathers each
batch on the host; `DeviceProcessedLoader` (`--day-file-loader=device`) keeps the raw rows resident in HBM -- the whole Kaggle
set is 45 840 617 x 160 B = 7.3 GB -- and cuts a look-ahead window per launch by the order (csrc/dayfile.hip: k_rows_window),
with no host staging and no PCIe traffic after the first upload.  The Criteo pre-processing that writes the file is not part
of this package."""
from __future__ import annotations

import math
from typing import Iterator, Tuple

import numpy as np
import torch

from . import ops
from .data_loader_terabyte import Batch, DeviceBatch, _DeviceWindowLoader, transform_features

RANDOMIZE = ("total", "day", "none")


def processed_paths(data_set: str, raw_data_file: str) -> Tuple[int, str, str]:
    """(days, the processed file's stem, the day-count file) as the reference names them (dlrm_data_pytorch.py:66-86, :119):
    `kaggle` is 7 days and d_file the raw file's name without its extension, `terabyte` 24 days and d_file the raw file's name
    as it is; the day counts (`total_per_file`) are `<dir>/<d_file>_day_count.npz`."""
    if data_set == "kaggle":
        days, out_file = 7, "kaggleAdDisplayChallenge_processed"
    elif data_set == "terabyte":
        days, out_file = 24, "terabyte_processed"
    else:
        raise ValueError("Data set option is not supported: --data-set=%s (kaggle | terabyte)" % data_set)
    lstr = raw_data_file.split("/")
    d_path = "/".join(lstr[0:-1]) + "/"
    d_file = lstr[-1].split(".")[0] if data_set == "kaggle" else lstr[-1]
    return days, out_file, d_path + d_file + "_day_count.npz"


def processed_order(total_per_file, split: str, randomize: str, rng=np.random) -> np.ndarray:
    """The rows of the processed file that make up `split` ("train" | "test" | "val"), in the order the reference's
    `CriteoDataset(split=...)` lists them (dlrm_data_pytorch.py:209-254), int64.  The row numbers are `np.array_split` at the
    day offsets; `day` permutes every day but the last with `rng.permutation`, in day order; the train rows are every day but
    the last, concatenated; the last day is `np.array_split` in two, "test" the first half (it gets the odd row) and "val" the
    second; `total` permutes the train rows once.  The permutations are drawn whatever the split, as one reference construction
    draws them (for "test" it throws them away): build train, then test, from a freshly seeded generator and the generator is
    where the reference leaves it."""
    if randomize not in RANDOMIZE:
        raise ValueError("--data-randomize=%s (total | day | none)" % randomize)
    if split not in ("train", "test", "val"):
        raise ValueError("split %r (train | test | val)" % (split,))
    offsets = np.concatenate([[0], np.cumsum(np.asarray(total_per_file, dtype=np.int64))])
    indices = np.array_split(np.arange(int(offsets[-1]), dtype=np.int64), offsets[1:-1])
    if randomize == "day":
        for i in range(len(indices) - 1):
            indices[i] = rng.permutation(indices[i])
    train = np.concatenate(indices[:-1]) if len(indices) > 1 else np.empty(0, dtype=np.int64)
    test, val = np.array_split(indices[-1], 2)
    if randomize == "total":
        train = rng.permutation(train)
    return np.ascontiguousarray({"train": train, "test": test, "val": val}[split], dtype=np.int64)


class ProcessedDataset:
    """The processed file, opened once: X_int [n, m_den], X_cat [n, n_emb], y [n] held as contiguous int32 (the file may store
    wider integers: a value that does not fit, like row counts that disagree with each other or with total_per_file, is a
    ValueError naming the file), `counts` = the table sizes, `total_per_file` = the day counts.  `resident(device)` is the one
    copy of the raw rows in HBM per process, shared by every `DeviceProcessedLoader` over this dataset."""

    UPLOAD_CHUNK = 8 << 20          # bytes of each of the two pinned buffers the rows go to HBM through

    def __init__(self, processed_file: str, total_per_file):
        self.processed_file = processed_file
        self.total_per_file = np.asarray(total_per_file, dtype=np.int64).reshape(-1)
        with np.load(processed_file) as data:
            arrs = [self._int32(data[k], k) for k in ("X_int", "X_cat", "y")]
            self.counts = np.asarray(data["counts"])
        self.X_int, self.X_cat, self.y = arrs
        self.y = self.y.reshape(-1)
        n = self.y.shape[0]
        if self.X_int.ndim != 2 or self.X_cat.ndim != 2 or self.X_int.shape[0] != n or self.X_cat.shape[0] != n:
            raise ValueError("%s: X_int %s, X_cat %s and y %s do not hold the same rows" % (
                processed_file, self.X_int.shape, self.X_cat.shape, self.y.shape))
        if self.total_per_file.size < 1 or int(self.total_per_file.min()) < 0 or int(self.total_per_file.sum()) != n:
            raise ValueError("%s holds %d rows, the day counts say %d" % (processed_file, n, int(self.total_per_file.sum())))
        self.m_den, self.n_emb = int(self.X_int.shape[1]), int(len(self.counts))
        if self.X_cat.shape[1] != self.n_emb:
            raise ValueError("%s: X_cat has %d columns, counts lists %d tables" % (processed_file, self.X_cat.shape[1], self.n_emb))
        self.uploads = 0            # times the raw rows went to a device (one per process is the rule)
        self._resident = None

    def _int32(self, a: np.ndarray, key: str) -> np.ndarray:
        a = np.asarray(a)
        if a.dtype != np.int32:
            if a.dtype.kind not in "iu":
                raise ValueError("%s: %s is %s, not an integer array" % (self.processed_file, key, a.dtype))
            if a.size and (int(a.min()) < -2 ** 31 or int(a.max()) > 2 ** 31 - 1):
                raise ValueError("%s: %s holds a value that does not fit int32 (%d .. %d)" % (
                    self.processed_file, key, int(a.min()), int(a.max())))
        return np.ascontiguousarray(a, dtype=np.int32)

    def __len__(self) -> int:
        return int(self.y.shape[0])

    @property
    def row_bytes(self) -> int:
        return 4 * (self.m_den + self.n_emb + 1)

    def is_resident(self, device) -> bool:
        return self._resident is not None and self._resident["device"] == torch.device(device)

    def resident(self, device, stream):
        """(x_int, x_cat, y) on `device`, uploaded the first time it is asked for: in chunks through two small pinned buffers,
        on `stream`; any later caller's stream is put behind the upload's event."""
        device = torch.device(device)
        r = self._resident
        if r is not None and r["device"] != device:
            raise RuntimeError("%s is resident on %s: one copy per process" % (self.processed_file, r["device"]))
        if r is None:
            with torch.cuda.device(device), torch.cuda.stream(stream):
                dev = [torch.empty(a.shape, dtype=torch.int32, device=device) for a in (self.X_int, self.X_cat, self.y)]
                pin = [dict(buf=torch.empty(self.UPLOAD_CHUNK // 4, dtype=torch.int32).pin_memory(), ev=None) for _ in range(2)]
                k = 0
                for src, dst in zip((self.X_int, self.X_cat, self.y), dev):
                    flat, out = src.reshape(-1), dst.view(-1)
                    for a in range(0, flat.shape[0], self.UPLOAD_CHUNK // 4):
                        b = min(flat.shape[0], a + self.UPLOAD_CHUNK // 4)
                        p = pin[k % 2]
                        k += 1
                        if p["ev"] is not None:
                            p["ev"].synchronize()       # the copy that read this buffer last is done
                        p["buf"].numpy()[:b - a] = flat[a:b]
                        out[a:b].copy_(p["buf"][:b - a], non_blocking=True)
                        p["ev"] = torch.cuda.Event()
                        p["ev"].record(stream)
                ev = torch.cuda.Event()
                ev.record(stream)
                for p in pin:                           # the pinned buffers go away with this call
                    if p["ev"] is not None:
                        p["ev"].synchronize()
            self.uploads += 1
            r = self._resident = dict(device=device, arrays=tuple(dev), ev=ev)
        else:
            for t in r["arrays"]:                       # (the allocator learns of the second reader)
                t.record_stream(stream)
        stream.wait_event(r["ev"])
        return r["arrays"]


def _n_batches(n: int, B: int, drop_last_batch: bool) -> int:
    return n // B if drop_last_batch else math.ceil(n / B)


def _check_order(dataset: ProcessedDataset, order) -> np.ndarray:
    order = np.ascontiguousarray(order, dtype=np.int64).reshape(-1)
    if order.size and (int(order.min()) < 0 or int(order.max()) >= len(dataset)):
        raise ValueError("%s: an order over rows %d .. %d of a file of %d rows" % (
            dataset.processed_file, int(order.min()), int(order.max()), len(dataset)))
    return order


class ProcessedLoader:
    """The host loader: batch j is rows order[j * B : (j + 1) * B] of the dataset through `transform_features` -- the
    arithmetic of `collate_wrapper_criteo` (dlrm_data_pytorch.py:323-338) over `CriteoDataset.__getitem__`'s rows with their
    `% max_ind_range` (:292-295).  The short last batch is handed out unless drop_last_batch.  No GPU work."""

    def __init__(self, dataset: ProcessedDataset, order, batch_size: int, max_ind_range: int = -1,
                 drop_last_batch: bool = False):
        self.dataset, self.order = dataset, _check_order(dataset, order)
        self.batch_size, self.max_ind_range, self.drop_last_batch = int(batch_size), int(max_ind_range), drop_last_batch
        if self.batch_size < 1:
            raise ValueError("%s: batch size %d" % (dataset.processed_file, self.batch_size))

    def __len__(self) -> int:
        return _n_batches(self.order.shape[0], self.batch_size, self.drop_last_batch)

    def __iter__(self) -> Iterator[Batch]:
        ds, B = self.dataset, self.batch_size
        for j in range(len(self)):
            rows = self.order[j * B:(j + 1) * B]
            yield transform_features(ds.X_int[rows], ds.X_cat[rows], ds.y[rows], self.max_ind_range)


class DeviceProcessedLoader(_DeviceWindowLoader):
    """`ProcessedLoader`'s batches, produced on the device a look-ahead window at a time, with `DeviceDayLoader`'s contract
    exactly: `DeviceBatch` tuples whose tensors are views of their window's buffers (`window_rect`, `win_pos`, `win_batches`,
    `wait_upload`), the RING = 3 rule, uploads on the loader's own stream by the helper thread, reuse ordered by events, no
    device-wide or stream synchronise while batches are handed out (the machinery is `_DeviceWindowLoader`'s).

    Only the upload differs: the raw rows are RESIDENT.  They go to HBM once per process, the first time a loader over the
    dataset iterates (`ProcessedDataset.resident`: chunks through two small pinned buffers); the train and the test loader share
    that copy.  A window is one slice of the order, so ONE launch cuts it: `ops.rows_window` over the slice of the
    device-resident order when the order permutes, `ops.dayfile_window` on offset pointers when it is a run of consecutive
    rows (the `none` order and every test / val split) -- then no order goes to the device at all.  No pinned staging, no
    per-batch launch, no PCIe traffic after the first upload.  The order goes up once: the reference randomises when the dataset
    is built, so every epoch sees the same order.  Its entries are checked against the file's row count here, on the host; the
    kernel trusts them.

    Refusal before any allocation: the raw rows (unless already resident) + the order + the ring of window buffers must fit
    `hbm_fraction` (default 0.5) of the device memory that is free when the loader sets up -- the rest is left to the cache,
    the model and the victim rows, which are sized elsewhere -- or a ValueError names the sizes and `--day-file-loader=host`."""

    THREAD = "processed-upload"

    def __init__(self, dataset: ProcessedDataset, order, batch_size: int, max_ind_range: int = -1,
                 drop_last_batch: bool = False, device="cuda", window: int = 1, hbm_fraction: float = 0.5):
        self.dataset, self.order = dataset, _check_order(dataset, order)
        self.batch_size, self.max_ind_range, self.drop_last_batch = int(batch_size), int(max_ind_range), drop_last_batch
        if self.batch_size < 1:
            raise ValueError("%s: batch size %d" % (dataset.processed_file, self.batch_size))
        self.n_dense, self.n_cat = dataset.m_den, dataset.n_emb
        self.device, self.window, self.hbm_fraction = torch.device(device), max(1, int(window)), float(hbm_fraction)
        n, B = self.order.shape[0], self.batch_size
        # a batch = (its first position in the order, its rows)
        self.batches = [(j * B, min(B, n - j * B)) for j in range(len(self))]
        # a run of consecutive rows is cut as it lies: first row, or None when the order permutes
        self.first_row = None
        if n and int(self.order[-1]) - int(self.order[0]) == n - 1 and bool((np.diff(self.order) == 1).all()):
            self.first_row = int(self.order[0])
        self._order_dev = self._rows_dev = None

    def __len__(self) -> int:
        return _n_batches(self.order.shape[0], self.batch_size, self.drop_last_batch)

    @staticmethod
    def _rows(batch) -> int:
        return batch[1]

    def hbm_bytes(self, n_batches: int) -> Tuple[int, int, int]:
        """(raw rows still to upload, order, window ring) in bytes, as `_setup` would allocate them."""
        W = min(self.window, n_batches) * self.batch_size
        raw = 0 if self.dataset.is_resident(self.device) else len(self.dataset) * self.dataset.row_bytes
        order = 0 if self.first_row is not None else 8 * self.order.shape[0]
        ring = self.RING * W * (4 * self.n_dense + 8 * self.n_cat + 4)
        return raw, order, ring

    def _setup(self, n_batches: int):
        if self.device.type != "cuda":
            raise RuntimeError("cdlrm_amd: DeviceProcessedLoader needs the MI355X (got %s); the host loader is ProcessedLoader"
                               % self.device)
        raw, order, ring = self.hbm_bytes(n_batches)
        free = int(torch.cuda.mem_get_info(self.device)[0])
        if raw + order + ring > self.hbm_fraction * free:
            raise ValueError("%s: %.3f GB of raw rows + %.3f GB of order + %.3f GB of window buffers do not fit %.3g of the %.3f "
                             "GB of device memory that are free (the rest is the cache's, the model's and the victim rows'): "
                             "use --day-file-loader=host" % (self.dataset.processed_file, raw / 1e9, order / 1e9, ring / 1e9,
                                                             self.hbm_fraction, free / 1e9))
        self._setup_ring(n_batches)
        self._rows_dev = self.dataset.resident(self.device, self._copy)
        if self.first_row is None:
            with torch.cuda.device(self.device), torch.cuda.stream(self._copy):
                # (pageable, once: the copy has read the host array when it returns)
                self._order_dev = torch.from_numpy(self.order).to(self.device)

    def _upload(self, slot, batches, released):
        """A window is positions [a, a + n) of the order: one launch."""
        a, n = batches[0][0], sum(r for _, r in batches)
        xi, xc, y = self._rows_dev
        with torch.cuda.device(self.device), torch.cuda.stream(self._copy):
            for e in released:
                self._copy.wait_event(e)
            if self.first_row is not None:
                r0 = self.first_row + a
                ops.dayfile_window(xi[r0:r0 + n], xc[r0:r0 + n], y[r0:r0 + n], self.max_ind_range, slot["X"], slot["I"],
                                   slot["T"], col0=0, stream=self._copy)
            else:
                ops.rows_window(xi, xc, y, self._order_dev[a:a + n], self.max_ind_range, slot["X"], slot["I"], slot["T"],
                                col0=0, stream=self._copy)
            slot["ev"].record(self._copy)
        return slot, n

    def __iter__(self) -> Iterator[DeviceBatch]:
        return self._hand_out(self.batches)
