"""The host-side plan of the pairwise-dot interaction (interact_plan, csrc/dense.hip), pinned through cdlrm_interact_route.

What cdlrm_interact_fwd / _bwd and the three fused gather + interaction calls launch -- kernel family, D4, grid, dynamic LDS bytes
-- is a pure function of (op, B, F, D, itself, row pitch, operand alignment) and of the debug keys 4 and 5.  `expect` below restates
that function from the rules the kernels were measured into and from the LDS formulas the host passed before the footprints were
gathered into one place; it never asks the library.  Whoever changes a route, a grid cap or a staging row changes a line here, on
purpose.  No GPU: the query touches no device.
"""
import ctypes as C
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import test_gemm_routes as R      # noqa: E402  (the module fixture that builds the library)

ops = R.ops
EINVAL = -22
OPS = ("fwd", "bwd", "gather_fwd", "gather_bwd", "gather_bwd_sgd")
GENERIC, ROW, SLAB, SLAB_DB = 1, 2, 3, 4
PIPED = (32, 64, 128, 256)

DS = (16, 32, 48, 64, 128, 256, 512)
FS = (1, 4, 16, 17, 27, 32)
BS = (1, 4, 5, 1024, 1025, 2048, 2049, 8192, 8193)


def npairs_of(F, itself):
    return F * (F + 1) // 2 if itself else F * (F - 1) // 2


def pad4(w):
    return (w + 3) & ~3


def expect(op, B, F, D, itself, ld_r, a_r, a_df, knob4=0, knob5=0):
    """(family, d4, ns, grid, lds_bytes) of the call, or None where its entry point refuses it."""
    npairs = npairs_of(F, itself)
    width = D + npairs
    vec = ld_r % 4 == 0 and a_r and ld_r >= pad4(width)
    blocks = (B + 3) // 4
    slab = 16 * (32 * 36 + D + 532)
    if op == "fwd":
        if ld_r < width:
            return None
        if D in PIPED and vec:
            return SLAB, D // 4, D // 32, min(blocks, 256), slab
        if D in PIPED:
            return ROW, D // 4, 0, min(blocks, 512), 16 * 32 * (D + 4)
        lds = 16 * (32 * (D + 1) + 32)
        return (GENERIC, D // 4, 0, min(blocks, 2048), lds) if lds <= 160 * 1024 else None
    if op == "bwd":
        if D in PIPED and vec and F > 16 and a_df:
            return SLAB, D // 4, D // 32, min(blocks, 256 if D == 256 else 512), 16 * (32 * 36 + D + 528)
        if D in (32, 64, 128) and vec:
            return ROW, D // 4, 0, min(blocks, 512), 16 * (32 * (D + 4) + D + 528)
        lds = 16 * (32 * (D + 1) + 32 + pad4(npairs))
        return (GENERIC, D // 4, 0, min(blocks, 2048), lds) if lds <= 160 * 1024 else None
    if not (D in PIPED and 16 < F <= 32 and vec and (op == "gather_fwd" or a_df)):
        return None
    if op == "gather_fwd":
        cap = 256 * (knob4 if knob4 > 0 else 1)
        if D == 32:
            return SLAB, 8, 1, min(blocks, cap), slab
        return SLAB_DB, D // 4, D // 32, min(blocks, cap), 16 * (2 * 32 * 36 + D + 532)
    cap = 256 * (knob5 if knob5 > 0 else (1 if D == 256 else 2))
    return SLAB, D // 4, D // 32, min(blocks, cap), 16 * (32 * 36 + D + 528)


def grid_of_cases():
    for D in DS:
        for F in FS:
            for itself in (0, 1):
                width = D + npairs_of(F, itself)
                for ld_r in (width, pad4(width), pad4(width) + 4):
                    for aligned in range(4):
                        for B in BS:
                            yield B, F, D, itself, ld_r, aligned


def ask(lib, op, B, F, D, itself, ld_r, aligned):
    """The library's answer as expect() writes it."""
    from cdlrm_amd import _lib
    out = _lib.InteractRoute()
    rc = lib.cdlrm_interact_route(OPS.index(op), B, F, D, itself, ld_r, aligned, C.byref(out))
    if rc != 0:
        assert rc == EINVAL
        return None
    return out.family, out.d4, out.ns, out.grid, out.lds_bytes


def table(lib, op):
    return [ask(lib, op, *case) for case in grid_of_cases()]


def check_table(lib, op, knob4=0, knob5=0):
    seen = set()
    for case, got in zip(grid_of_cases(), table(lib, op)):
        B, F, D, itself, ld_r, aligned = case
        want = expect(op, B, F, D, itself, ld_r, bool(aligned & 1), bool(aligned & 2), knob4, knob5)
        assert got == want, (op, case, got, want)
        seen.add(want and want[0])
    return seen


class Knob:
    """cdlrm_debug_set(key, value) for the block; back to 0 (the default) in a finally."""

    def __init__(self, lib, key, value):
        self.lib, self.key, self.value = lib, key, value

    def __enter__(self):
        assert self.lib.cdlrm_debug_set(self.key, self.value) == 0

    def __exit__(self, *exc):
        assert self.lib.cdlrm_debug_set(self.key, 0) == 0


@pytest.fixture()
def lib(ops):
    from cdlrm_amd import _lib
    return _lib.raw()


@pytest.mark.parametrize("op", OPS)
def test_route_table(lib, op):
    """Family, d4, ns, grid and LDS bytes of every case of the grid; each op reaches every family it has, and refuses some case."""
    seen = check_table(lib, op)
    families = {"fwd": {GENERIC, ROW, SLAB, None}, "bwd": {GENERIC, ROW, SLAB, None}, "gather_fwd": {SLAB, SLAB_DB, None}}
    assert seen == families.get(op, {SLAB, None}), seen


def test_ops_wrapper_and_supported_shapes(ops):
    """ops.interact_route names what the raw query numbers; cdlrm_gather_interact_supported is the plan's answer."""
    r = ops.interact_route("gather_fwd", 8192, 27, 128, False, 480)
    assert r == {"family": "slab_db", "d4": 32, "ns": 4, "grid": 256, "lds_bytes": 16 * (2 * 32 * 36 + 128 + 532)}
    r = ops.interact_route("bwd", 8192, 27, 128, False, 480, aligned_dfeat=False)
    assert r["family"] == "row" and r["d4"] == 32 and r["ns"] == 0 and r["grid"] == 512
    with pytest.raises(RuntimeError, match="unsupported shape"):
        ops.interact_route("gather_bwd", 64, 9, 128, False, 164)


def test_refused_shapes(lib):
    """A shape the entry point refuses is refused by the query, with the entry point's error."""
    from cdlrm_amd import _lib
    out = _lib.InteractRoute()

    def refused(op, B, F, D, itself, ld_r, aligned=3):
        assert lib.cdlrm_interact_route(OPS.index(op), B, F, D, itself, ld_r, aligned, C.byref(out)) == EINVAL
        return lib.cdlrm_last_error().decode()

    for op in OPS:
        assert "unsupported shape" in refused(op, 64, 33, 128, 0, 1024)         # F > 32
        assert "unsupported shape" in refused(op, 64, 27, 130, 0, 1024)         # D % 4 != 0
        assert "unsupported shape" in refused(op, 64, 27, 516, 0, 1024)         # D > 512
        assert "unsupported shape" in refused(op, 64, 0, 128, 0, 1024)
    assert "ld_r" in refused("fwd", 64, 27, 128, 0, 128 + 351 - 1)              # ld_r < width
    assert "ld_r" in refused("fwd", 64, 4, 16, 1, 16 + 10 - 1)
    for op in OPS[2:]:
        assert "unsupported shape" in refused(op, 64, 9, 128, 0, 164)           # F <= 16
        assert "unsupported shape" in refused(op, 64, 27, 48, 0, 400)           # no slab kernel at D = 48
        assert "whole-float4" in refused(op, 64, 27, 128, 0, 479)               # ld_r < width, no whole words
        assert "whole-float4" in refused(op, 64, 27, 128, 0, 480, aligned=2)    # R / dR off 16 bytes
    for op in OPS[3:]:
        assert "whole-float4" in refused(op, 64, 27, 128, 0, 480, aligned=1)    # dfeat off 16 bytes
    assert lib.cdlrm_interact_route(2, 64, 27, 128, 0, 480, 1, C.byref(out)) == 0       # (the forward has no dfeat)
    # the generic backward above 160 KiB = 10240 floats per wave: D = 512 always; the edges with no pairs and with all 528
    assert "LDS budget" in refused("bwd", 64, 27, 512, 0, 1024)
    assert "LDS budget" in refused("bwd", 64, 1, 320, 0, 320)                   # 32 * 321 + 32 = 10304
    assert "LDS budget" in refused("bwd", 64, 32, 304, 1, 1024)                 # 32 * 305 + 32 + 528 = 10320
    assert lib.cdlrm_interact_route(1, 64, 1, 316, 0, 316, 3, C.byref(out)) == 0
    assert (out.family, out.lds_bytes) == (GENERIC, 16 * (32 * 317 + 32))       # 10176
    assert lib.cdlrm_interact_route(1, 64, 32, 300, 1, 1024, 3, C.byref(out)) == 0
    assert (out.family, out.lds_bytes) == (GENERIC, 16 * (32 * 301 + 32 + 528))     # 10192
    assert "LDS budget" in refused("fwd", 64, 27, 512, 0, 1024)                 # the forward's generic tile: 32 * 513 + 32 = 16448


def test_knobs_4_and_5_move_the_gather_grids_and_nothing_else(lib):
    """Debug keys 4 / 5: workgroups per CU of the fused forward / the two fused backwards.  Every other answer stays."""
    base = {op: table(lib, op) for op in OPS}
    with Knob(lib, 4, 3):
        assert SLAB_DB in check_table(lib, "gather_fwd", knob4=3)
        assert table(lib, "gather_fwd") != base["gather_fwd"]
        for op in OPS:
            if op != "gather_fwd":
                assert table(lib, op) == base[op], op
    with Knob(lib, 5, 3):
        for op in OPS[3:]:
            check_table(lib, op, knob5=3)
            assert table(lib, op) != base[op]
        for op in OPS[:3]:
            assert table(lib, op) == base[op], op
    for op in OPS:
        assert table(lib, op) == base[op], op


def test_key_7_no_longer_selects_a_single_slice_forward(lib):
    """Bit 2 of debug key 7 used to put the fused forward at D = 64 / 128 / 256 back on one slab slice; that duplicate is gone."""
    base = {op: table(lib, op) for op in OPS}
    with Knob(lib, 7, 2):
        for D in (64, 128, 256):
            got = ask(lib, "gather_fwd", 8192, 27, D, 0, pad4(D + 351), 3)
            assert got == (SLAB_DB, D // 4, D // 32, 256, 16 * (2 * 32 * 36 + D + 532))
        for op in OPS:
            assert table(lib, op) == base[op], op
