"""Differential sweep of the embedding backward's route query: one line per query, for comparing two builds of the library.

    python tools/embbag_bwd_route_sweep.py path/to/libcdlrm_hip.so > routes.txt    (stderr: line count and sha256 of the output)

The library is loaded through plain ctypes; cdlrm_embbag_bwd_route, cdlrm_embbag_bwd_work_bytes and cdlrm_embbag_bwd_sorted_bytes
touch no device and read no pointer.  A refactor of K8's host side (the layouts, bwd_sort_plan and bwd_apply_plan of
csrc/embbag_bwd.hip) must leave every line as it was: run the tool on the library of the parent commit and on the new one and
compare the two outputs.

The walk: every (T, D, n) of TS x DS x NS, offsets given or not, all four entries -- the window entries with every (nb, j0, count)
of WINDOWS, the others once -- under every value of the development keys 1 (workgroups per CU of the apply) and 6 (the apply
form).  A line holds the return code, every field of the route (a refused query leaves the zeros the struct started with) and
the two byte counts.
"""
import ctypes as C
import hashlib
import sys

TS = (1, 2, 26, 40)
DS = (4, 8, 16, 32, 48, 64, 128, 256, 384, 1024)
NS = (0, 1, 31, 32, 33, 1023, 1024, 1025, 2048, 2049, 4096, 4097, 8192, 8193, 16384, 16385, 32768, 65536, 65537, 1 << 20,
      (1 << 31) - 1, 1 << 31)
ENTRIES = ("apply", "rest", "sorted", "sorted_rest")        # CDLRM_BWD_ENTRY_* 0 .. 3
WINDOWS = ((1, 0, 1), (4, 2, 2), (3, 1, 1), (3, 0, 3), (0, 0, 1), (2, 2, 1), (2, 0, 3), (2, -1, 1), (3000, 0, 1))
DEBUG1 = (-1, 0, 1, 20)
DEBUG6 = (0, 64, 128, 192)
I32 = ("sort_chunk", "sort_e", "sort_chunks", "merge_passes", "seg_meta", "keys_in_b", "apply", "arange", "lpr", "reserved")
I64 = ("apply_grid_x", "apply_grid_y", "long_grid", "keys_off", "meta_off", "once_off", "apply_keys_off")


class Route(C.Structure):
    _fields_ = [(n, C.c_int32) for n in I32] + [(n, C.c_int64) for n in I64]

    def __str__(self):
        return " ".join("%d" % getattr(self, n) for n in I32 + I64)


def main(path):
    L = C.CDLL(path)
    i32, i64 = C.c_int32, C.c_int64
    L.cdlrm_embbag_bwd_route.argtypes = [i32, i32, i64, i32, i32, i32, i32, i32, C.POINTER(Route)]
    L.cdlrm_embbag_bwd_work_bytes.argtypes = [i32, i64, i32]
    L.cdlrm_embbag_bwd_work_bytes.restype = C.c_uint64
    L.cdlrm_embbag_bwd_sorted_bytes.argtypes = [i32, i32, i64]
    L.cdlrm_embbag_bwd_sorted_bytes.restype = C.c_uint64
    L.cdlrm_debug_set.argtypes = [i32, i32]
    h, lines = hashlib.sha256(), 0
    try:
        for d1 in DEBUG1:
            for d6 in DEBUG6:
                L.cdlrm_debug_set(1, d1)
                L.cdlrm_debug_set(6, d6)
                for T in TS:
                    for D in DS:
                        for n in NS:
                            work = L.cdlrm_embbag_bwd_work_bytes(T, n, D)
                            for off in (0, 1):
                                for e, entry in enumerate(ENTRIES):
                                    for nb, j0, count in (WINDOWS if e >= 2 else ((1, 0, 1),)):
                                        out = Route()
                                        rc = L.cdlrm_embbag_bwd_route(T, D, n, off, e, nb, j0, count, out)
                                        line = "d%d/%d T%d D%d n%d o%d %s nb%d j%d c%d -> %d %s | %d %d\n" % (
                                            d1, d6, T, D, n, off, entry, nb, j0, count, rc, out, work,
                                            L.cdlrm_embbag_bwd_sorted_bytes(T, nb, n))
                                        sys.stdout.write(line)
                                        h.update(line.encode())
                                        lines += 1
    finally:
        L.cdlrm_debug_set(1, 0)
        L.cdlrm_debug_set(6, 0)
    sys.stderr.write("%d lines, sha256 %s\n" % (lines, h.hexdigest()))


if __name__ == "__main__":
    main(sys.argv[1])
