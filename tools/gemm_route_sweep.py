"""Differential sweep of the dense GEMM route queries: one line per query, for comparing two builds of the library.

    python tools/gemm_route_sweep.py path/to/libcdlrm_hip.so > routes.txt      (stderr: line count and sha256 of the output)

The library is loaded through plain ctypes; cdlrm_linear_fwd_route, cdlrm_linear_bwd_route and cdlrm_mlp_wgrad_route touch no
device and read no pointer, so the operands are made-up addresses.  A refactor of the planning code (csrc/gemm_plan.h) must leave
every line as it was: run the tool on the library of the parent commit and on the new one and compare the two outputs.

The walk: every (M, N, K) of MS x NKS x NKS, under every SETTING -- the default call (pitches equal to the extents, operands
16-byte aligned, ReLU on both sides, 256 compute units, no flag, no development switch) with one axis moved at a time, plus the
pairs that meet in one rule (CDLRM_GEMM_ALONE with each compute-unit count and each bit of development key 6, the bf16 modes on
odd pitches, ...).  Per shape and setting four calls: the forward, and the backward with dX and dW, dX only, dW only.  Then
cdlrm_mlp_wgrad_route on the layer lists of the c2 and c3 configurations (c5 is c3's list at M = 65536), fp32 and both bf16
modes, with each operand variant of tests/test_wgrad_plan.py.
"""
import ctypes as C
import hashlib
import sys

MS = (1, 3, 31, 32, 33, 64, 255, 256, 1000, 1024, 2048, 2049, 4096, 8100, 8192, 16384, 65536)
NKS = (1, 3, 4, 13, 31, 32, 33, 64, 70, 96, 100, 128, 256, 264, 479, 480, 512, 1024)
ALONE, BF16, BF16X3 = 0x100, 0x200, 0x400
FAMILIES = ("none", "smallk_rows", "smallk", "direct", "staged", "gemm2", "gemm3", "gemm", "bf16", "bf16x3")
OPERANDS = ("x", "w", "b", "y", "dx", "dw")      # b: bias / db; y: Y / dY
DEFAULT = dict(pitch=0, off=None, act=1, x_act=1, alone=0, flags=0, n_cu=256, d0=0, d6=0, d7=0)
LAYERS = {
    "c2_bot": ((512, 13), (256, 512), (32, 256)),
    "c2_top": ((512, 384), (256, 512), (1, 256)),
    "c3_bot": ((512, 13), (256, 512), (128, 256)),
    "c3_top": ((512, 480), (512, 512), (256, 512), (1, 256)),
}
LAYERS["c2_all"] = LAYERS["c2_bot"] + LAYERS["c2_top"]
LAYERS["c3_all"] = LAYERS["c3_bot"] + LAYERS["c3_top"]


class Route(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("family", "tm", "tn", "mode", "aligned", "splits", "vec_a", "vec_b", "fast")]

    def __str__(self):
        return "%s %dx%d m%d a%d v%d%d f%d /%d" % (FAMILIES[self.family], self.tm, self.tn, self.mode, self.aligned, self.vec_a,
                                                   self.vec_b, self.fast, self.splits)


def settings():
    S = [{}]
    S += [dict(pitch=p) for p in (1, 4)]
    S += [dict(off=(o, f)) for o in OPERANDS for f in (1, 4)]
    S += [dict(act=a) for a in (0, 2)] + [dict(x_act=a) for a in (0, 2)]
    S += [dict(n_cu=n) for n in (64, 304)]
    S += [dict(alone=1, n_cu=n) for n in (64, 256, 304)]
    S += [dict(alone=a, d6=b) for a in (0, 1) for b in (16, 32, 256, 512, 1024)]
    S += [dict(alone=1, pitch=4), dict(alone=1, act=0, x_act=0), dict(alone=1, off=("b", 1)), dict(alone=1, off=("x", 4))]
    S += [dict(flags=f, pitch=p) for f in (BF16, BF16X3) for p in (0, 1, 4)]
    S += [dict(flags=f, off=("w", 1)) for f in (BF16, BF16X3)]
    S += [dict(d0=1), dict(d7=1), dict(d7=1, alone=1), dict(d7=1, pitch=4)]
    return [dict(DEFAULT, **s) for s in S]


def tag(s):
    return "p%d o%s a%d x%d al%d f%x cu%d d%d/%d/%d" % (s["pitch"], "%s%d" % s["off"] if s["off"] else "-", s["act"], s["x_act"],
                                                          s["alone"], s["flags"], s["n_cu"], s["d0"], s["d6"], s["d7"])


def main(path):
    L = C.CDLL(path)
    vp, i32, i64 = C.c_void_p, C.c_int32, C.c_int64
    L.cdlrm_linear_fwd_route.argtypes = [vp, i64, vp, vp, vp, i64, i64, i32, i32, i32, vp, i32, C.POINTER(Route)]
    L.cdlrm_linear_bwd_route.argtypes = [vp, i64, vp, vp, i64, vp, i64, vp, i64, vp, vp, i64, i32, i32, i32, i32, vp, vp, i32,
                                         C.POINTER(Route)]
    L.cdlrm_mlp_wgrad_route.argtypes = [i32, vp, vp, vp, vp, vp, vp, i64, vp, vp, i32, i32, C.POINTER(Route)]
    L.cdlrm_debug_set.argtypes = [i32, i32]
    base = {o: (1 << 40) + (i << 36) for i, o in enumerate(OPERANDS + ("work", "Y"))}
    out, h, n = (Route * 2)(), hashlib.sha256(), 0

    def emit(line):
        nonlocal n
        line += "\n"
        sys.stdout.write(line)
        h.update(line.encode())
        n += 1

    for s in settings():
        for key, v in ((0, s["d0"]), (6, s["d6"]), (7, s["d7"])):
            L.cdlrm_debug_set(key, v)
        t, p = tag(s), s["pitch"]
        a = dict(base)
        if s["off"]:
            a[s["off"][0]] += 4 * s["off"][1]
        mode = s["flags"] | (ALONE if s["alone"] else 0)
        for M in MS:
            for N in NKS:
                for K in NKS:
                    rc = L.cdlrm_linear_fwd_route(a["x"], K + p, a["w"], a["b"], a["y"], N + p, M, N, K, s["act"] | mode, None,
                                                  s["n_cu"], out)
                    emit("fwd %d %d %d %s -> %d %s" % (M, N, K, t, rc, out[0]))
                    for name, dx, dw in (("bwd", a["dx"], a["dw"]), ("bwd_dx", a["dx"], None), ("bwd_dw", None, a["dw"])):
                        rc = L.cdlrm_linear_bwd_route(a["x"], K + p, a["w"], a["Y"], N + p, a["y"], N + p, dx, K + p, dw,
                                                      a["b"] if dw else None, M, N, K, s["act"] | mode, s["x_act"], a["work"], None,
                                                      s["n_cu"], out)
                        emit("%s %d %d %d %s -> %d %s | %s" % (name, M, N, K, t, rc, out[0], out[1]))
    for key in (0, 6, 7):
        L.cdlrm_debug_set(key, 0)
    for name, layers in sorted(LAYERS.items()):
        nl = len(layers)
        PA, IA, NA = vp * nl, i64 * nl, i32 * nl
        rout = (Route * nl)()
        for variant in ("aligned", "xpitch", "dzoff", "dbnull"):
            X = [(1 << 40) + (i << 32) for i in range(nl)]
            dZ = [(2 << 40) + (i << 32) for i in range(nl)]
            dW = [(3 << 40) + (i << 32) for i in range(nl)]
            db = [(4 << 40) + (i << 32) for i in range(nl)]
            ldx = [k for _, k in layers]
            if variant == "xpitch":
                ldx[min(1, nl - 1)] += 1
            elif variant == "dzoff":
                dZ[nl // 2] += 4
            elif variant == "dbnull":
                db[min(2, nl - 1)] = None
            for flags, n_cu, d6 in [(f, c, d) for f in (0, BF16, BF16X3) for c in (64, 256, 304) for d in (0, 32, 256, 512, 1024)]:
                L.cdlrm_debug_set(6, d6)
                for M in MS:
                    rc = L.cdlrm_mlp_wgrad_route(nl, PA(*X), IA(*ldx), PA(*dZ), IA(*[nn for nn, _ in layers]), PA(*dW), PA(*db), M,
                                                 NA(*[nn for nn, _ in layers]), NA(*[k for _, k in layers]), flags, n_cu, rout)
                    emit("wgrad %s %s f%x cu%d d6=%d %d -> %d %s" % (name, variant, flags, n_cu, d6, M, rc,
                                                                      " | ".join(str(rout[i]) for i in range(nl))))
    L.cdlrm_debug_set(6, 0)
    sys.stderr.write("%d lines, sha256 %s\n" % (n, h.hexdigest()))


if __name__ == "__main__":
    main(sys.argv[1])
