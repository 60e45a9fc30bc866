"""Raw Criteo text -> the processed files every Criteo loader here starts from, on the device.

The reference's ETL (data_utils.py:876-1121, `getCriteoAdData` with `process_one_file`, `processCriteoAdData` and
`concatCriteoAdData`) is a Python loop per line and per field.  `getCriteoAdData` below keeps its name, its argument list, its
path handling and what it computes (DESIGN.md section 3 has the contract); the text goes to HBM in chunks and the per-line work
is four kernels of csrc/etl.hip (`ops.etl_line_index`, `etl_parse`, `etl_subsample`, `etl_encode`).  The dictionaries are
extended on the device with stable sorts.  One pass over the text: parse -> drop -> extend the dictionary -> encode that day
(a value's id is final as soon as its day is scanned).

Two departures from the reference, both named in DESIGN.md: `X_cat` is written as int32 (the reference writes the same values
as float64, which `ProcessedDataset` refuses), and a hash >= 2^31 keeps its int32 bit pattern (numpy >= 1.24 raises
OverflowError at data_utils.py:998-1006; numpy < 1.24 stored the wrap, and so do the published processed files).

    python -m cdlrm_amd.data_utils --raw-data-file=.../train.txt --processed-data-file=... --data-set=kaggle
"""
from __future__ import annotations

import argparse
import os
import sys
from typing import List, Optional, Tuple

import numpy as np
import torch

from . import ops

N_DENSE, N_CAT = ops.ETL_N_DENSE, ops.ETL_N_CAT
ROW_BYTES = 4 * (1 + N_DENSE + N_CAT)
DEFAULT_CHUNK = 32 << 20        # bytes of text per launch; the pinned ring is two of these
COUNT_BLOCK = 16 << 20          # bytes per read of the line-counting pass
MIN_LINE = 40                   # 39 tabs and a newline: no well-formed line is shorter
_SORT_BYTES_PER_ROW = 40        # a column's dictionary extension: values, sorted values, int64 order, masks, run heads


# ---- the host side of the text: counting, piece boundaries, the chunk ring ------------------------------------------------------

def _count_lines(path: str, block: int = COUNT_BLOCK) -> Tuple[int, List[int]]:
    """(lines, newlines per block): what `for _ in f` counts (data_utils.py:921-923) -- a final line without '\\n' is a line."""
    per_block, last = [], b"\n"
    with open(path, "rb") as f:
        while True:
            buf = f.read(block)
            if not buf:
                break
            per_block.append(buf.count(b"\n"))
            last = buf[-1:]
    return sum(per_block) + (last != b"\n"), per_block


def _offset_after_newline(path: str, per_block: List[int], k: int, block: int = COUNT_BLOCK) -> int:
    """Byte offset one past the k-th newline of the file (k >= 1), from the per-block counts of `_count_lines`."""
    before = 0
    for b, c in enumerate(per_block):
        if before + c >= k:
            with open(path, "rb") as f:
                f.seek(b * block)
                buf = np.frombuffer(f.read(block), dtype=np.uint8)
            return b * block + int(np.flatnonzero(buf == 10)[k - before - 1]) + 1
        before += c
    raise ValueError("%s holds fewer than %d newlines" % (path, k))


def _last_newline(buf: np.ndarray, length: int) -> int:
    """Position of the last '\\n' of buf[:length], -1 if there is none (searched from the end, a window at a time)."""
    hi = length
    while hi > 0:
        lo = max(0, hi - 65536)
        at = np.flatnonzero(buf[lo:hi] == 10)
        if at.size:
            return lo + int(at[-1])
        hi = lo
    return -1


class _Source:
    """One day's text: bytes [begin, end) of a file, `lines` lines, the first of them line `line0` (0-based) of the file."""

    def __init__(self, path: str, begin: int, end: int, lines: int, line0: int):
        self.path, self.begin, self.end, self.lines, self.line0 = path, begin, end, lines, line0


def _sources(datafile: str, npzfile: str, days: int, criteo_kaggle: bool) -> List[_Source]:
    if criteo_kaggle:
        # one train.txt cut into `days` pieces by line count, the first `extras` one line longer (data_utils.py:926-929);
        # the split text files train_day_i are not written: a piece is a byte range
        if not os.path.exists(datafile):
            raise FileNotFoundError("Criteo Kaggle Display Ad Challenge Dataset path is invalid: %s" % datafile)
        total, per_block = _count_lines(datafile)
        per, extras = divmod(total, days)
        sizes = [per + (1 if j < extras else 0) for j in range(days)]
        size = os.path.getsize(datafile)
        out, line0, begin = [], 0, 0
        for n in sizes:
            end = size if line0 + n >= total else _offset_after_newline(datafile, per_block, line0 + n)
            if n == 0:
                end = begin
            out.append(_Source(datafile, begin, end, n, line0))
            line0, begin = line0 + n, end
        return out
    out = []
    for i in range(days):
        path = datafile + "_" + str(i)
        if not os.path.exists(path):
            raise FileNotFoundError("Criteo Terabyte Dataset path is invalid: day file %s is missing" % path)
        out.append(_Source(path, 0, os.path.getsize(path), _count_lines(path)[0], 0))
    return out


def _device_free_bytes(device) -> int:
    """Bytes this process can still place on the device: the driver's free memory plus what the allocator holds unused."""
    free, _ = torch.cuda.mem_get_info(device)
    return int(free) + int(torch.cuda.memory_reserved(device)) - int(torch.cuda.memory_allocated(device))


def _day_bytes(lines: int, chunk_bytes: int, sub_sample: bool, dict_keys: int) -> Tuple[int, int, int]:
    """(parsed rows, text chunk ring, running dictionary + one column's extension) in bytes for a day of `lines` lines."""
    rows = lines * ROW_BYTES
    ring = chunk_bytes + 8 * (chunk_bytes + 1) + 8 * (chunk_bytes // 4096 + 2)
    if sub_sample:
        per_chunk = min(lines, chunk_bytes // MIN_LINE + 1)
        rows += 8 * lines                                       # rand_u
        ring += per_chunk * ROW_BYTES + 8 * (per_chunk // 256 + 2)
    dictionary = 16 * dict_keys + _SORT_BYTES_PER_ROW * (lines + dict_keys)
    return rows, ring, dictionary


class _Dictionary:
    """One column's running dictionary on the device: `keys` int32 ascending, `pos` int64 the global kept-row number of each
    key's first appearance.  A value's id is the rank of its first position (data_utils.py:1080-1082: enumeration order of a
    dict filled in row order)."""

    def __init__(self, device):
        self.keys = torch.empty(0, dtype=torch.int32, device=device)
        self.pos = torch.empty(0, dtype=torch.int64, device=device)

    @staticmethod
    def _run_heads(sorted_vals: torch.Tensor) -> torch.Tensor:
        head = torch.ones(sorted_vals.numel(), dtype=torch.bool, device=sorted_vals.device)
        head[1:] = sorted_vals[1:] != sorted_vals[:-1]
        return head

    def extend(self, vals: torch.Tensor, base: int) -> None:
        """vals: the column's values of one day's kept rows, the first of them global row `base`."""
        if vals.numel() == 0:
            return
        sv, order = torch.sort(vals, stable=True)               # stable: the first position of a run is its smallest
        head = self._run_heads(sv)
        keys = torch.cat([self.keys, sv[head]])                 # the running entries first: stable keeps the older position
        pos = torch.cat([self.pos, order[head] + base])
        sk, order = torch.sort(keys, stable=True)
        head = self._run_heads(sk)
        self.keys, self.pos = sk[head].contiguous(), pos[order][head].contiguous()

    def ids(self) -> torch.Tensor:
        """int32 beside `keys`: the rank of every key's first position."""
        ids = torch.empty(self.keys.numel(), dtype=torch.int32, device=self.keys.device)
        ids[torch.argsort(self.pos)] = torch.arange(self.keys.numel(), dtype=torch.int32, device=self.keys.device)
        return ids

    def unique(self) -> np.ndarray:
        """The keys in first-appearance order (`<d_file>_fea_dict_j.npz`)."""
        return self.keys[torch.argsort(self.pos)].cpu().numpy().astype(np.int32)


class _Ring:
    """Two pinned text buffers and the device side of a chunk.  A chunk is read into one buffer while the kernels of the chunk
    before it run; bytes behind a chunk's last newline are carried in front of the next chunk."""

    def __init__(self, chunk_bytes: int, device):
        if chunk_bytes < 2:
            raise ValueError("chunk_bytes=%d: a chunk holds at least one byte and its newline" % chunk_bytes)
        self.cap = int(chunk_bytes)
        self.pinned = [torch.empty(self.cap, dtype=torch.uint8).pin_memory() for _ in range(2)]
        self.host = [p.numpy() for p in self.pinned]
        self.text = torch.empty(self.cap, dtype=torch.uint8, device=device)
        self.starts = torch.empty(self.cap + 1, dtype=torch.int64, device=device)
        self.count = torch.empty(1, dtype=torch.int64, device=device)


def _raise_malformed(src: _Source, found, what="line") -> None:
    line, code = found
    raise ValueError("%s: %s %d is malformed: %s (code %d)" % (src.path, what, line, ops.ETL_CODES.get(code, "?"), code))


def _parse_day(src: _Source, ring: _Ring, stream, device, max_ind_range: int, rate: float, rand_u: Optional[torch.Tensor],
               err: torch.Tensor):
    """One day's text -> (y, X_int, X_cat, kept) on the device, sub-sampled, not yet encoded."""
    n_max = src.lines
    y = torch.empty(n_max, dtype=torch.int32, device=device)
    x_int = torch.empty((n_max, N_DENSE), dtype=torch.int32, device=device)
    x_cat = torch.empty((n_max, N_CAT), dtype=torch.int32, device=device)
    rows = [torch.zeros(1, dtype=torch.int64, device=device) for _ in range(2)] if rate > 0.0 else None
    seen = kept = k = carry = 0
    remaining = src.end - src.begin
    with open(src.path, "rb", buffering=0) as f:
        f.seek(src.begin)
        buf = ring.host[0]
        while remaining > 0 or carry > 0:
            # ---- host: the next chunk behind the carry (the kernels of the chunk before are running meanwhile)
            length = carry
            want = min(remaining, ring.cap - 1 - length)         # one byte stays free for a final line's missing newline
            while want > 0:
                got = f.readinto(memoryview(buf)[length:length + want])
                if not got:
                    raise ValueError("%s ends before byte %d" % (src.path, src.end))
                length, want, remaining = length + got, want - got, remaining - got
            if remaining == 0 and length > 0 and buf[length - 1] != 10:
                buf[length] = 10                                 # a final line without '\n' counts as a line
                length += 1
            last = _last_newline(buf, length)
            if last < 0:
                # the carry grew until the buffer was full (the end of the text always has its newline) and no line ends in it
                raise ValueError("%s: line %d is longer than the chunk capacity of %d bytes" % (
                    src.path, src.line0 + seen + 1, ring.cap))
            # ---- device: upload, index; the count comes back (the one wait per chunk), then parse and drop are queued
            ring.text[:length].copy_(ring.pinned[k % 2][:length], non_blocking=True)
            ops.etl_line_index(ring.text, length, ring.starts, ring.count, stream=stream)
            n = int(ring.count.item())
            found = ops.etl_error(err)                           # of the chunks before this one: they have finished
            if found:
                _raise_malformed(src, found)
            if n < 1 or seen + n > n_max:
                raise RuntimeError("%s: the line index counts %d lines where the file has %d left" % (src.path, n, n_max - seen))
            if rate > 0.0:
                cy = torch.empty(n, dtype=torch.int32, device=device)
                ci = torch.empty((n, N_DENSE), dtype=torch.int32, device=device)
                cc = torch.empty((n, N_CAT), dtype=torch.int32, device=device)
                ops.etl_parse(ring.text, length, ring.starts, n, src.line0 + seen, max_ind_range, cy, ci, cc, err, stream=stream)
                ops.etl_subsample(cy, ci, cc, n, rand_u, seen, rate, y, x_int, x_cat, rows[k % 2], rows[(k + 1) % 2],
                                  stream=stream)
            else:
                ops.etl_parse(ring.text, length, ring.starts, n, src.line0 + seen, max_ind_range, y, x_int, x_cat, err,
                              row0=seen, stream=stream)
            seen += n
            # ---- the bytes behind the last newline go in front of the next chunk, in the other buffer
            k += 1
            carry = length - (last + 1)
            nxt = ring.host[k % 2]
            if carry:
                nxt[:carry] = buf[last + 1:length]
            buf = nxt
    found = ops.etl_error(err)
    if found:
        _raise_malformed(src, found)
    if seen != n_max:
        raise RuntimeError("%s: %d lines parsed, %d counted" % (src.path, seen, n_max))
    kept = int(rows[k % 2].item()) if rate > 0.0 else seen
    return y, x_int, x_cat, kept


def getCriteoAdData(datafile, o_filename, max_ind_range=-1, sub_sample_rate=0.0, days=7, data_split='train', randomize='total',
                    criteo_kaggle=True, memory_map=False, *, force=False, store=False, chunk_bytes=DEFAULT_CHUNK,
                    device="cuda:0"):
    """The reference's `getCriteoAdData` (data_utils.py:876-1121): raw text -> `<d_file>_day_count.npz`, the 26
    `<d_file>_fea_dict_j.npz`, `<d_file>_fea_count.npz`, a `<npzfile>_i_processed.npz` per day and, unless `memory_map`, the
    concatenation `<d_path><o_filename>.npz` whose path it returns.  `data_split` and `randomize` only matter to the reference's
    `memory_map` reorder, which is not written.  force: overwrite existing outputs; store: np.savez instead of
    np.savez_compressed; chunk_bytes: text per launch."""
    lstr = datafile.split("/")
    d_path = "/".join(lstr[0:-1]) + "/"
    d_file = lstr[-1].split(".")[0] if criteo_kaggle else lstr[-1]
    npzfile = d_path + ((d_file + "_day") if criteo_kaggle else d_file)
    days = int(days)
    if days < 1:
        raise ValueError("days=%d: at least one" % days)
    rate = float(sub_sample_rate)
    if not 0.0 <= rate <= 1.0:
        raise ValueError("sub_sample_rate=%r: a rate in [0, 1]" % (sub_sample_rate,))
    total_file = d_path + d_file + "_day_count.npz"
    count_file = d_path + d_file + "_fea_count.npz"
    dict_files = [d_path + d_file + "_fea_dict_{0}.npz".format(j) for j in range(N_CAT)]
    day_files = [npzfile + "_{0}_processed.npz".format(i) for i in range(days)]
    o_file = d_path + o_filename + ".npz"
    outputs = [total_file, count_file] + dict_files + day_files + ([] if memory_map else [o_file])
    if not force:
        for p in outputs:
            if os.path.exists(p):
                raise FileExistsError("%s exists: the ETL does not reuse earlier outputs (force=True / --force overwrites them)" % p)
    sources = _sources(datafile, npzfile, days, bool(criteo_kaggle))
    save = np.savez if store else np.savez_compressed

    if not torch.cuda.is_available():
        raise RuntimeError("cdlrm_amd.data_utils parses the text on the MI355X; there is no CPU path")
    device = torch.device(device)
    chunk_bytes = int(chunk_bytes)

    def refuse_unless_it_fits(i, src, dict_keys):
        rows, ring_b, dictionary = _day_bytes(src.lines, chunk_bytes, rate > 0.0, dict_keys)
        free = _device_free_bytes(device)
        if rows + ring_b + dictionary > free:
            raise ValueError("day %d of %s does not fit the device: %d bytes of parsed rows (%d lines) + %d of text chunk ring + %d "
                             "of dictionary = %d, %d free" % (i, datafile, rows, src.lines, ring_b, dictionary,
                                                              rows + ring_b + dictionary, free))

    refuse_unless_it_fits(0, max(sources, key=lambda s: s.lines), 0)       # before any allocation
    stream = torch.cuda.Stream(device=device)
    total_per_file, kept_days, base = [], [], 0
    with torch.cuda.device(device), torch.cuda.stream(stream):
        ring = _Ring(chunk_bytes, device)
        dicts = [_Dictionary(device) for _ in range(N_CAT)]
        err = ops.etl_error_word(device)
        for i, src in enumerate(sources):
            if i:
                refuse_unless_it_fits(i, src, max(int(d.keys.numel()) for d in dicts))
            rand_u = None
            if rate > 0.0:
                # one draw per line of the file, in file order (data_utils.py:979); the caller seeds numpy
                rand_u = torch.from_numpy(np.random.uniform(low=0.0, high=1.0, size=src.lines)).to(device)
            y, x_int, x_cat, kept = _parse_day(src, ring, stream, device, int(max_ind_range), rate, rand_u, err)
            for j, d in enumerate(dicts):
                d.extend(x_cat[:kept, j].contiguous(), base)
                ops.etl_encode(x_cat, j, d.keys, d.ids(), err, n=kept, row0=base, stream=stream)
            found = ops.etl_error(err)
            if found:
                _raise_malformed(src, found, what="kept row")
            day = dict(X_cat=x_cat[:kept].cpu().numpy(), X_int=x_int[:kept].cpu().numpy(), y=y[:kept].cpu().numpy())
            del y, x_int, x_cat, rand_u
            save(day_files[i], **day)
            print("Processed %s: %d of %d lines kept" % (day_files[i], kept, src.lines))
            total_per_file.append(kept)
            base += kept
            if not memory_map:
                kept_days.append(day)
        uniques = [d.unique() for d in dicts]
    counts = np.array([u.size for u in uniques], dtype=np.int32)
    np.savez_compressed(total_file, total_per_file=np.array(total_per_file, dtype=np.int64))
    for j, u in enumerate(uniques):
        np.savez_compressed(dict_files[j], unique=u)
    np.savez_compressed(count_file, counts=counts)
    print("Total number of samples:", int(np.sum(total_per_file)))
    print("Divided into days/splits:\n", total_per_file)
    if memory_map:
        print("memory_map: stopping after the per-day processed files (the reordered files of the reference are not written)")
        return o_file
    print("Concatenating multiple days into %s file" % o_file)
    save(o_file, X_cat=np.concatenate([d["X_cat"] for d in kept_days]), X_int=np.concatenate([d["X_int"] for d in kept_days]),
         y=np.concatenate([d["y"] for d in kept_days]), counts=counts)
    return o_file


# ---- command line -------------------------------------------------------------------------------------------------------------

DATA_SETS = {"kaggle": (7, "kaggleAdDisplayChallenge_processed"), "terabyte": (24, "terabyte_processed")}


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(prog="python -m cdlrm_amd.data_utils", description="Pre-process the raw Criteo text on the GPU")
    p.add_argument("--raw-data-file", type=str, default="")
    p.add_argument("--processed-data-file", type=str, default="")
    p.add_argument("--data-set", type=str, default="kaggle")            # or terabyte
    p.add_argument("--max-ind-range", type=int, default=-1)
    p.add_argument("--data-sub-sample-rate", type=float, default=0.0)   # in [0, 1]
    p.add_argument("--data-randomize", type=str, default="total")
    p.add_argument("--numpy-rand-seed", type=int, default=123)
    p.add_argument("--memory-map", action="store_true", default=False)
    p.add_argument("--days", type=int, default=0, help="0: 7 for kaggle, 24 for terabyte")
    p.add_argument("--force", action="store_true", default=False, help="overwrite existing outputs")
    p.add_argument("--store", action="store_true", default=False, help="np.savez without compression")
    p.add_argument("--chunk-bytes", type=int, default=DEFAULT_CHUNK)
    return p


def main(argv=None) -> str:
    args = build_parser().parse_args(argv)
    if args.data_set not in DATA_SETS:
        raise SystemExit("ERROR: Data set option is not supported: --data-set=%s (kaggle | terabyte)" % args.data_set)
    days, o_filename = DATA_SETS[args.data_set]
    if not args.raw_data_file:
        raise SystemExit("ERROR: --raw-data-file is required")
    d_path = "/".join(args.raw_data_file.split("/")[0:-1]) + "/"
    if args.processed_data_file:
        # the reference always writes <dir of the raw file>/<o_filename>.npz (data_utils.py:753); a flag that names another
        # file would be ignored silently
        want = d_path + o_filename + ".npz"
        if os.path.abspath(args.processed_data_file) != os.path.abspath(want):
            raise SystemExit("ERROR: --processed-data-file=%s: the ETL writes %s" % (args.processed_data_file, want))
    np.random.seed(args.numpy_rand_seed)
    try:
        out = getCriteoAdData(args.raw_data_file, o_filename, args.max_ind_range, args.data_sub_sample_rate, args.days or days,
                              "train", args.data_randomize, args.data_set == "kaggle", args.memory_map, force=args.force,
                              store=args.store, chunk_bytes=args.chunk_bytes)
    except (ValueError, OSError) as e:
        raise SystemExit("ERROR: " + " ".join(str(e).split()))
    print("Wrote %s" % out)
    return out


if __name__ == "__main__":
    main(sys.argv[1:])
