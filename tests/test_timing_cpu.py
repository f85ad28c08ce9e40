"""The timing helpers' refusals that need no device (tests/test_gpu_timing.py holds everything else): what they answer without
a context, and that the header's new queries are bound."""
import ctypes as C

from vppstereo_amd import _lib


def test_helpers_without_a_context_refuse_and_leave_ms_out_alone():
    lib = _lib.load()
    ms, n = C.c_float(-7.0), C.c_int(-7)
    assert lib.vppx_time_aggregate(None, 3, C.byref(ms)) == _lib.ABI.constants["VPPX_E_NO_DEVICE"]
    assert b"context is NULL" in lib.vppx_last_error()
    assert lib.vppx_time_aggregate_part(None, 3, 1, C.byref(ms)) == _lib.ABI.constants["VPPX_E_NO_DEVICE"]
    assert lib.vppx_agg_kernel_ms(None, 4, C.byref(ms), C.byref(n)) == _lib.ABI.constants["VPPX_E_NO_DEVICE"]
    assert lib.vppx_we_kernel_ms(None, 4, C.byref(ms), C.byref(n)) == _lib.ABI.constants["VPPX_E_NO_DEVICE"]
    assert (ms.value, n.value) == (-7.0, -7)
    assert lib.vppx_time_aggregate_frames(None) == 0 and lib.vppx_stage_marks(None) == 0


def test_a_part_other_than_1_or_2_is_refused_before_the_context_is_looked_at():
    lib = _lib.load()
    ms = C.c_float(-7.0)
    for part in (0, 3, -1):
        assert lib.vppx_time_aggregate_part(None, 3, part, C.byref(ms)) == _lib.ABI.constants["VPPX_E_INVALID_ARG"]
        assert lib.vppx_last_error() == b"part must be 1 or 2"
    assert ms.value == -7.0


def test_the_helpers_own_route_list_follows_last_routes_convention():
    lib = _lib.load()
    assert "vppx_timing_last_routes" in _lib.EXPORTS and "vppx_stage_marks" in _lib.EXPORTS
    assert lib.vppx_timing_last_routes.argtypes == lib.vppx_last_routes.argtypes
    assert lib.vppx_timing_last_routes(None, None, 0) == _lib.ABI.constants["VPPX_E_NO_DEVICE"]
    assert lib.vppx_get_stage_ms(None, None, 0) == _lib.ABI.constants["VPPX_E_INVALID_ARG"]
