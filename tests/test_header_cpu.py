"""The Python binding is derived from include/vppx.h (vppstereo_amd/_header.py): checks of the reader that do not go through the
reader -- the C compiler's struct layout, signatures written out by hand, a call of every entry point that takes a handle -- and
of what it refuses."""
import ctypes as C
import os
import re
import shutil
import subprocess
from types import SimpleNamespace

import pytest

from vppstereo_amd import _header, _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "vppx.h")).read()
STRUCTS = ("VppxVppParams", "VppxRsgmParams", "VppxOccParams", "VppxScaleParams", "VppxEvalParams", "VppxSampleParams", "VppxGruSource",
           "VppxMetrics")
# the test's own view of the header: comments out, then `ret vppx_name(params);`
_CODE = re.sub(r"/\*.*?\*/", " ", HEADER, flags=re.S)
DECLARED = [(ret.strip(), name, [p.strip() for p in params.split(",")])
            for ret, name, params in re.findall(r"([\w \t]+?[ \t*]+)(vppx_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", _CODE)]


def test_struct_layout_is_the_c_compilers(tmp_path):
    structs = {n: getattr(_lib, n) for n in STRUCTS}
    assert set(structs) == set(_lib.ABI.structs) == set(re.findall(r"typedef struct (\w+) \{", HEADER))
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "vppx.h"', 'int main(void) {']
    for n, s in structs.items():
        lines.append(f'    printf("{n} %zu\\n", sizeof({n}));')
        lines += [f'    printf("{n}.{f} %zu\\n", offsetof({n}, {f}));' for f, _ in s._fields_]
    (tmp_path / "layout.c").write_text("\n".join(lines + ["    return 0;", "}", ""]))
    subprocess.check_call([shutil.which("cc") or "gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(tmp_path / "layout.c"),
                           "-o", str(tmp_path / "layout")])
    want = dict(line.split() for line in subprocess.check_output([str(tmp_path / "layout")], text=True).splitlines())
    got = {}
    for n, s in structs.items():
        got[n] = str(C.sizeof(s))
        got.update({f"{n}.{f}": str(getattr(s, f).offset) for f, _ in s._fields_})
    assert got == want and len(got) == 8 + sum(len(s._fields_) for s in structs.values())
    assert C.sizeof(_lib.VppxVppParams) == 104 and C.sizeof(_lib.VppxRsgmParams) == 32 and C.sizeof(_lib.VppxMetrics) == 64
    assert _lib.VppxVppParams() is not None         # the structs exist without the library


class _Is:
    """Equal to a type that is `base` or derives from it."""

    def __init__(self, base):
        self.base = base

    def __eq__(self, other):
        return isinstance(other, type) and issubclass(other, self.base)


def test_pinned_signatures():
    """Written out from the hand-made table this binding replaces, so that the reader is not only checked against itself."""
    lib = _lib.load()
    vp, i, i64, f, d, cp = C.c_void_p, C.c_int, C.c_int64, C.c_float, C.c_double, C.c_char_p
    P = lambda s: _Is(C.POINTER(s))          # a pointer to one of the header's structs: POINTER(struct) or a subclass of it
    want = {
        "vppx_raft_motion_front_dt_dev": (i, [vp, vp, vp, vp, i64, vp, i64, vp, vp, i, vp, vp, i, i, i, i, i, i, i, i, vp, i64, vp, i64,
                                              i, i]),
        "vppx_raft_gru_update_dt_dev": (i, [vp, vp, i64, vp, i64, vp, i64, vp, i64, vp, i64, vp, i64, i, i, i, i, i]),
        "vppx_raft_gru_assemble_dt_dev": (i, [vp, P(_lib.VppxGruSource), i, i, i, i, vp, i, i]),
        "vppx_raft_upsample_dt_dev": (i, [vp, vp, i64, vp, i, i, i, i, i, i, i, i, i, i, i, vp, i]),
        "vppx_png_decode_dev": (i, [vp, i, vp, vp, i, i, i, f, vp, vp, vp, vp]),
        "vppx_fstream_pop_eval": (i, [vp, vp, vp, vp, vp, vp, P(_lib.VppxMetrics), vp]),
        "vppx_virtual_projection_scan_max_dist": (i, [vp, vp, vp, vp, i, i, i, i, i, i, i, i, f, f, vp, i, i]),
        "vppx_guided_visualize_dev": (i, [vp, i, i, i, vp, vp, vp, d, i, C.c_uint, vp]),
        "vppx_occlusion_heuristic_full_dev": (i, [vp, i, i, i, vp, i, i, d, d, d, d, vp, vp]),
        "vppx_raft_corr_pyramid_cells": (i64, [i64, i, i, vp]),
        "vppx_sample_threshold": (C.c_uint32, [d]),
        "vppx_rand_stream": (i, [vp, C.c_uint32, C.c_uint64, i64, vp]),
        "vppx_workspace_bytes": (C.c_size_t, [vp]),
        "vppx_lockstep_failures": (C.c_long, [vp]),
        "vppx_device_name": (cp, [vp]),
        "vppx_last_error": (cp, []),
        "vppx_last_routes": (i, [vp, cp, i]),
        "vppx_create": (i, [vp, i]),
        "vppx_destroy": (None, [vp]),
        "vppx_vpp_params_default": (None, [P(_lib.VppxVppParams)]),
    }
    for name, (restype, argtypes) in want.items():
        fn = getattr(lib, name)
        assert (fn.restype, list(fn.argtypes)) == (restype, argtypes), name


def test_a_struct_pointer_takes_the_struct_and_an_address():
    """`VppxMetrics *metrics_out` is a host record in some calls and device memory in others: the slot takes the instance, byref,
    an array, a pointer and NULL as POINTER(VppxMetrics) does, and an address as c_void_p does; nothing else."""
    M = _lib.VppxMetrics
    slot = _lib.load().vppx_guided_metrics_dev.argtypes[10]
    assert issubclass(slot, C.POINTER(M)) and slot._type_ is M
    rec, arr = M(), (M * 2)()
    for v in (rec, C.byref(rec), C.pointer(rec), arr, None):
        slot.from_param(v)
    for v in (C.addressof(arr), C.c_void_p(C.addressof(arr))):
        p = slot.from_param(v)
        assert C.cast(p, C.c_void_p).value == C.addressof(arr)
    assert not slot.from_param(0) and not slot.from_param(C.c_void_p())
    for v in (1.5, "x", C.c_int(3), _lib.VppxEvalParams(), C.byref(_lib.VppxEvalParams())):
        with pytest.raises((TypeError, C.ArgumentError)):
            slot.from_param(v)


def test_every_prototype_is_bound_with_the_headers_arity():
    lib = _lib.load()
    assert [name for _, name, _ in DECLARED] == _lib.EXPORTS and len(set(_lib.EXPORTS)) == len(DECLARED) >= 120
    for _, name, params in DECLARED:
        fn = getattr(lib, name)
        assert fn.argtypes is not None and len(fn.argtypes) == (0 if params == ["void"] else len(params)), name


def test_constants_are_the_headers():
    k = _lib.ABI.constants
    assert _lib.ERR_NAMES == {-1: "VPPX_E_INVALID_ARG", -2: "VPPX_E_DMAX_MOD8", -3: "VPPX_E_DMAX_GT256", -4: "VPPX_E_UNIQUENESS",
                              -5: "VPPX_E_WIDTH_MOD16", -6: "VPPX_E_METHOD", -7: "VPPX_E_NO_DEVICE", -8: "VPPX_E_HIP", -9: "VPPX_E_OOM",
                              -10: "VPPX_E_UNSUPPORTED"}
    assert (_lib.VPPX_OK, _lib.DT_F32, _lib.DT_BF16, _lib.GRU_MAX_SOURCES) == (0, 0, 1, 4)
    assert (_lib.FS_PATTERNS, _lib.FS_MASK, _lib.FS_GOCC, _lib.FS_GUIDED, _lib.FS_METRICS, _lib.FS_NO_DISP, _lib.FS_SAMPLE) == (1, 2, 4, 8, 16, 32, 64)
    assert (_lib.CORR_MAX_LEVELS, _lib.CORR_MAX_RADIUS, _lib.MOTION_MAX_CH, _lib.MOTION_MAX_KS) == (4, 8, 64, 7)
    assert (_lib.VIZ_ALL, _lib.VIZ_MAX_DILATION) == (63, 31) and _lib.GRU_MODES == {"copy": 0, "pool2x": 1, "interp": 2}
    assert (k["VPPX_VERSION"], k["VPPX_METHOD_RND"], k["VPPX_METHOD_MAXDIST"], k["VPPX_VIZ_RMS"]) == (100, 0, 1, 32)
    assert "VPPX_H" not in k
    # implicit, explicit and derived enumerators
    e = _header.parse("enum { A_X, A_Y, A_Z = 8, A_W, A_ALL = A_X | A_Z | 0x10, A_NEG = -3 };\ntypedef enum T { T_A = 2, T_B } T;").constants
    assert e == dict(A_X=0, A_Y=1, A_Z=8, A_W=9, A_ALL=24, A_NEG=-3, T_A=2, T_B=3)


# entry points that take a handle and return int, by what they answer to a NULL handle with every other argument NULL / zero
ZERO = {"vppx_uses_vert", "vppx_batch_quantum", "vppx_last_call_parts", "vppx_we_last_pieces", "vppx_wsum_last_pieces",
        "vppx_fused_pixels_per_wave", "vppx_time_aggregate_frames", "vppx_stage_marks"}                 # queries: 0 without a context
INVALID_ARG = {"vppx_fstream_push", "vppx_fstream_push_guided", "vppx_fstream_push_eval", "vppx_fstream_push_sampled", "vppx_fstream_flush",
               "vppx_fstream_pop", "vppx_fstream_pop_eval", "vppx_fstream_counts",                       # "stream is NULL"
               "vppx_set_graph_mode", "vppx_enable_stage_timing", "vppx_get_stage_ms", "vppx_last_front_sets",
               "vppx_time_aggregate_part", "vppx_fstream_create_sampled"}                                 # their own message


def test_null_handle_sweep():
    """Every derived signature through ctypes' argument conversion and into the library: nothing crashes, nothing succeeds."""
    lib = _lib.load()
    swept = [(name, params) for ret, name, params in DECLARED
             if ret == "int" and re.fullmatch(r"(const )?vppx_ctx \*\w+|vppx_fstream \*\w+", params[0])]
    assert len(swept) == 101
    seen = {0: set(), -1: set(), -7: set()}
    for name, _ in swept:
        fn = getattr(lib, name)
        rc = fn(*[0.0 if t in (C.c_float, C.c_double) else 0 if t in _header.SCALARS.values() else None for t in fn.argtypes])
        assert rc in seen, (name, rc)
        seen[rc].add(name)
        if rc < 0:
            assert lib.vppx_last_error(), name
            if rc == -7:
                assert b"context is NULL" in lib.vppx_last_error(), name
    assert seen[0] == ZERO and seen[-1] == INVALID_ARG and len(seen[-7]) == 79


def test_a_function_the_library_lacks_is_named(monkeypatch):
    class Lacking:
        def __getattr__(self, name):
            if name == "vppx_create":
                raise AttributeError(name)
            return SimpleNamespace()

    _lib.load()
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(C, "CDLL", lambda path: Lacking())
    with pytest.raises(ImportError, match="does not export vppx_create"):
        _lib.load()


@pytest.mark.parametrize("text, quoted", [
    ("int vppx_f(vppx_ctx *ctx, uint8_t flag);", "int vppx_f(vppx_ctx *ctx, uint8_t flag)"),             # a scalar outside the list
    ("int vppx_f(VppxNoSuch p);", "int vppx_f(VppxNoSuch p)"),                                           # a struct by value
    ("typedef struct S { int32_t a; short b; } S;", "short b"),                                           # an unknown field type
    ("typedef struct S { int (*cb)(int); } S;", "int (*cb)(int)"),                                        # a function pointer
    ("int vppx_f(int (*cb)(int));", "int vppx_f(int (*cb)(int))"),                                       # nested parentheses
    ("int vppx_f(vppx_ctx *, int);", "int vppx_f(vppx_ctx *, int)"),                                     # a parameter without a name
    ("static int g(void) { return vppx_f(0); }", "return vppx_f(0)"),                                     # a call, not a prototype
    ("int other_f(int a);", "int other_f(int a)"),                                                        # not ours
    ("enum { A = 1 << 3 };", "A = 1 << 3"),                                                               # an expression it cannot value
])
def test_the_reader_refuses_and_quotes(text, quoted):
    with pytest.raises(ValueError) as e:
        _header.parse(text)
    assert quoted in str(e.value), str(e.value)


def test_the_reader_on_a_small_header():
    h = _header.parse("""
        /* vppx_foo(int) in a comment is no prototype */   // nor is vppx_bar(void) here
        #define VPPX_N 0x10   /* sixteen */
        #define VPPX_GUARD
        typedef struct P { const void *ptr; int32_t a, b; double w; } P;
        typedef struct vppx_ctx vppx_ctx;
        const char *vppx_name(const vppx_ctx *ctx);
        void vppx_fill(P *p,
                       const P *q, float *out, vppx_ctx **h, unsigned which, size_t n);
        uint32_t vppx_t(double p);   int vppx_v(void);
    """)
    assert h.constants == {"VPPX_N": 16} and list(h.protos) == ["vppx_name", "vppx_fill", "vppx_t", "vppx_v"]
    P = h.structs["P"]
    assert P._fields_ == [("ptr", C.c_void_p), ("a", C.c_int32), ("b", C.c_int32), ("w", C.c_double)] and P.__name__ == "P"
    assert h.protos["vppx_name"] == (C.c_char_p, [C.c_void_p])
    assert h.protos["vppx_fill"] == (None, [_Is(C.POINTER(P)), _Is(C.POINTER(P)), C.c_void_p, C.c_void_p, C.c_uint, C.c_size_t])
    assert h.protos["vppx_t"] == (C.c_uint32, [C.c_double]) and h.protos["vppx_v"] == (C.c_int, [])
