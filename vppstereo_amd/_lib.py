"""ctypes binding of libvppx.so (C-ABI in include/vppx.h).

There is no CPU fallback anywhere in this package: if the HIP library is missing or no
MI355X is visible, every compute call raises.  PyTorch is used only as plumbing (device
memory, streams, torch.distributed) by the optional tensor front-end.
"""
import ctypes as C
import os
import threading

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("VPPX_LIB") or os.path.join(_HERE, "libvppx.so")  # VPPX_LIB: experiment builds

VPPX_OK = 0
ERR_NAMES = {
    -1: "VPPX_E_INVALID_ARG", -2: "VPPX_E_DMAX_MOD8", -3: "VPPX_E_DMAX_GT256", -4: "VPPX_E_UNIQUENESS",
    -5: "VPPX_E_WIDTH_MOD16", -6: "VPPX_E_METHOD", -7: "VPPX_E_NO_DEVICE", -8: "VPPX_E_HIP", -9: "VPPX_E_OOM",
    -10: "VPPX_E_UNSUPPORTED",
}

# every symbol include/vppx.h declares (tests check that the library exports all of them)
EXPORTS = [
    "vppx_version", "vppx_last_error", "vppx_vpp_params_default", "vppx_rsgm_params_default", "vppx_occ_params_default", "vppx_create",
    "vppx_destroy", "vppx_set_stream", "vppx_set_stream_legacy", "vppx_set_pipeline", "vppx_synchronize", "vppx_status", "vppx_lockstep_failures", "vppx_workspace_bytes", "vppx_device_name", "vppx_srand",
    "vppx_rand_stream", "vppx_rand_state", "vppx_rand_advance", "vppx_virtual_projection_scan_rnd", "vppx_virtual_projection_scan_max_dist", "vppx_vpp_host",
    "vppx_vpp_dev", "vppx_vpp_last_draws", "vppx_census5x5", "vppx_cost_census5x5_xyd", "vppx_aggregate", "vppx_aggregate_img", "vppx_match_wta",
    "vppx_match_wta_right", "vppx_subpixel_refine", "vppx_median3x3", "vppx_rsgm_host", "vppx_rsgm_dev",
    "vppx_vpp_rsgm_dev", "vppx_rsgm_post_dev", "vppx_occ_vpp_rsgm_dev", "vppx_occ_vpp_rsgm_host", "vppx_inputs_ready_event", "vppx_u8_to_nchw_dev", "vppx_psmnet_cost_volume_dev", "vppx_raft_corr_modulate_dev", "vppx_kitti_disp_decode_dev", "vppx_png_decode_dev", "vppx_pfm_decode_dev", "vppx_occlusion_heuristic_host", "vppx_occlusion_heuristic_dev", "vppx_occlusion_heuristic_full_host", "vppx_occlusion_heuristic_full_dev", "vppx_set_graph_mode", "vppx_graph_replays", "vppx_time_aggregate", "vppx_agg_kernel_ms", "vppx_we_kernel_ms", "vppx_time_aggregate_frames", "vppx_time_aggregate_part", "vppx_uses_vert", "vppx_last_call_parts", "vppx_we_last_pieces", "vppx_wsum_last_pieces", "vppx_wsum_default_route", "vppx_last_routes", "vppx_last_front_routes", "vppx_fused_pixels_per_wave", "vppx_batch_quantum",
    "vppx_enable_stage_timing", "vppx_get_stage_ms", "vppx_stage_name",
    "vppx_fstream_create", "vppx_fstream_destroy", "vppx_fstream_push", "vppx_fstream_flush", "vppx_fstream_pop", "vppx_fstream_counts",
    "vppx_occ_vpp_rsgm_guided_dev", "vppx_occ_vpp_rsgm_guided_host", "vppx_fstream_push_guided",
    "vppx_scale_params_default", "vppx_scaled_shape", "vppx_scale_table_builds", "vppx_last_front_sets", "vppx_occ_vpp_rsgm_scaled_dev", "vppx_occ_vpp_rsgm_scaled_host",
    "vppx_fstream_create_scaled",
    "vppx_eval_params_default", "vppx_guided_metrics_dev", "vppx_guided_metrics_host", "vppx_occ_vpp_rsgm_eval_dev",
    "vppx_fstream_create_eval", "vppx_fstream_push_eval", "vppx_fstream_pop_eval",
    "vppx_rsgm_front_dev", "vppx_rsgm_guided_rows_dev", "vppx_rsgm_mid_dev",
    "vppx_error_colors_dev", "vppx_error_colors_host", "vppx_guided_visualize_dev", "vppx_guided_visualize_host",
    "vppx_colorize_dev", "vppx_colorize_host", "vppx_finite_max_dev",
    "vppx_sample_params_default", "vppx_sample_threshold", "vppx_sample_hints_dev", "vppx_sample_hints_host", "vppx_occ_vpp_rsgm_sampled_dev",
    "vppx_fstream_create_sampled", "vppx_fstream_push_sampled",
    "vppx_psmnet_cost_volume_dt_dev", "vppx_raft_corr_modulate_dt_dev",
    "vppx_raft_corr_pyramid_cells", "vppx_raft_corr_pyramid_dt_dev", "vppx_raft_corr_lookup_dt_dev", "vppx_raft_corr_fused_dt_dev",
    "vppx_psmnet_readout_dt_dev", "vppx_raft_upsample_dt_dev",
    "vppx_raft_gru_assemble_dt_dev", "vppx_raft_gru_reset_dt_dev", "vppx_raft_gru_update_dt_dev",
    "vppx_raft_motion_front_dt_dev",
]
CORR_MAX_LEVELS, CORR_MAX_RADIUS = 4, 8
DT_F32, DT_BF16 = 0, 1          # VppxDtype
GRU_MAX_SOURCES = 4
MOTION_MAX_CH, MOTION_MAX_KS = 64, 7
GRU_MODES = {"copy": 0, "pool2x": 1, "interp": 2}      # VppxGruMode
FS_PATTERNS, FS_MASK, FS_GOCC, FS_GUIDED = 1, 2, 4, 8
FS_METRICS, FS_NO_DISP = 16, 32
FS_SAMPLE = 64
VIZ_KEYS = ('bad 1.0', 'bad 2.0', 'bad 3.0', 'bad 4.0', 'avgerr', 'rms')  # utils.guided_visualize's dict keys (utils.py:79), VPPX_VIZ_* bit order
VIZ_ALL = 63
VIZ_MAX_DILATION = 31
METRIC_KEYS = ('bad 1.0', 'bad 2.0', 'bad 3.0', 'bad 4.0', 'avgerr', 'rms')  # the reference's dict keys (losses.py:24), VppxMetrics order


class VppxVppParams(C.Structure):
    _fields_ = [
        ("method", C.c_int32), ("wsize", C.c_int32), ("wsize_agg_x", C.c_int32), ("wsize_agg_y", C.c_int32),
        ("direction", C.c_int32), ("uniform_color", C.c_int32), ("discard_occluded", C.c_int32),
        ("interpolate", C.c_int32), ("c", C.c_float), ("c_occ", C.c_float), ("use_distance_patch", C.c_int32),
        ("use_bilateral_patch", C.c_int32), ("distance_gamma", C.c_double), ("dmin", C.c_float), ("dmax", C.c_float),
        ("seed", C.c_uint32), ("per_frame_range", C.c_uint32), ("rand_offset", C.c_uint64),
        ("bilateral_o_xy", C.c_double), ("bilateral_o_i", C.c_double), ("bilateral_th", C.c_double),
    ]


class VppxRsgmParams(C.Structure):
    _fields_ = [
        ("dmax", C.c_int32), ("p1", C.c_int32), ("p2min", C.c_int32), ("alpha", C.c_float), ("gamma", C.c_int32),
        ("uniqueness", C.c_float), ("subpixel", C.c_int32), ("reserved0", C.c_int32),
    ]


class VppxOccParams(C.Structure):
    _fields_ = [("rx", C.c_int32), ("ry", C.c_int32), ("l", C.c_double), ("g", C.c_double), ("th_conf", C.c_double),
                ("th_filter", C.c_double)]


class VppxScaleParams(C.Structure):
    _fields_ = [("iscale", C.c_int32), ("oscale", C.c_int32)]


class VppxEvalParams(C.Structure):
    _fields_ = [("gt_scale", C.c_int32), ("reserved0", C.c_int32)]


class VppxSampleParams(C.Structure):
    _fields_ = [("probability", C.c_double), ("seed", C.c_uint32), ("reserved0", C.c_uint32), ("reserved1", C.c_uint64)]


class VppxGruSource(C.Structure):
    _fields_ = [("ptr", C.c_void_p), ("frame_stride", C.c_int64), ("C", C.c_int32), ("Hs", C.c_int32), ("Ws", C.c_int32),
                ("mode", C.c_int32)]


class VppxMetrics(C.Structure):
    _fields_ = [("bad1", C.c_double), ("bad2", C.c_double), ("bad3", C.c_double), ("bad4", C.c_double), ("avgerr", C.c_double),
                ("rms", C.c_double), ("n_valid", C.c_double), ("reserved", C.c_double)]


class VppxError(Exception):
    """Raised for every non-zero return of the C-ABI; .code is the VPPX_E_* value.  The
    message is the reference's own exception text where one exists (rsgm.py:19-40)."""

    def __init__(self, code, msg):
        super().__init__(msg)
        self.code = code


_lib = None
_lock = threading.Lock()


def load():
    """Load libvppx.so; raises (never falls back) when it has not been built."""
    global _lib
    with _lock:
        if _lib is not None:
            return _lib
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                f"{LIB_PATH} not found: the HIP library has not been built "
                "(run `python -c 'import __graft_entry__ as g; g.build()'` or `make -C vppstereo_amd/csrc`). "
                "vppstereo_amd has no CPU fallback.")
        # torch bundles its own HIP runtime (same soname as /opt/rocm's): whichever is loaded first
        # serves the whole process, and torch only works with its own -> let torch go first.
        try:
            import torch  # noqa: F401
        except Exception:
            pass
        lib = C.CDLL(LIB_PATH)
        vp = C.c_void_p
        lib.vppx_version.restype = C.c_int
        lib.vppx_last_error.restype = C.c_char_p
        lib.vppx_device_name.restype = C.c_char_p
        lib.vppx_device_name.argtypes = [vp]
        lib.vppx_stage_name.restype = C.c_char_p
        lib.vppx_stage_name.argtypes = [C.c_int]
        lib.vppx_workspace_bytes.restype = C.c_size_t
        lib.vppx_workspace_bytes.argtypes = [vp]
        lib.vppx_create.argtypes = [C.POINTER(vp), C.c_int]
        lib.vppx_destroy.argtypes = [vp]
        lib.vppx_destroy.restype = None
        lib.vppx_set_stream.argtypes = [vp, vp]
        lib.vppx_set_stream_legacy.argtypes = [vp]
        lib.vppx_set_pipeline.argtypes = [vp, C.c_int]
        lib.vppx_synchronize.argtypes = [vp]
        lib.vppx_status.argtypes = [vp]
        lib.vppx_lockstep_failures.argtypes = [vp]
        lib.vppx_lockstep_failures.restype = C.c_long
        lib.vppx_srand.argtypes = [vp, C.c_uint32]
        lib.vppx_rand_state.argtypes = [vp, C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)]
        lib.vppx_rand_advance.argtypes = [vp, C.c_uint64]
        lib.vppx_rand_stream.argtypes = [vp, C.c_uint32, C.c_uint64, C.c_int64, vp]
        i, f, d = C.c_int, C.c_float, C.c_double
        lib.vppx_virtual_projection_scan_rnd.argtypes = [vp, vp, vp, vp, i, i, i, i, i, i, f, f, vp, i, i]
        lib.vppx_virtual_projection_scan_max_dist.argtypes = [vp, vp, vp, vp, i, i, i, i, i, i, i, i, f, f, vp, i, i]
        pv, pr = C.POINTER(VppxVppParams), C.POINTER(VppxRsgmParams)
        lib.vppx_vpp_params_default.argtypes = [pv]
        lib.vppx_vpp_params_default.restype = None
        lib.vppx_rsgm_params_default.argtypes = [pr]
        lib.vppx_rsgm_params_default.restype = None
        lib.vppx_vpp_host.argtypes = [vp, pv, i, i, i, i, vp, vp, vp, vp, vp, vp]
        lib.vppx_vpp_dev.argtypes = [vp, pv, i, i, i, i, vp, vp, vp, vp, vp, vp]
        lib.vppx_vpp_last_draws.argtypes = [vp, i, C.POINTER(C.c_uint64)]
        lib.vppx_census5x5.argtypes = [vp, vp, vp, i, i]
        lib.vppx_cost_census5x5_xyd.argtypes = [vp, vp, vp, vp, i, i, i, i]
        lib.vppx_aggregate.argtypes = [vp, vp, vp, vp, i, i, i, i, i, f, i]
        lib.vppx_aggregate_img.argtypes = [vp, vp, i, vp, vp, i, i, i, i, i, f, i]
        lib.vppx_match_wta.argtypes = [vp, vp, vp, i, i, i, f]
        lib.vppx_match_wta_right.argtypes = [vp, vp, vp, i, i, i, f]
        lib.vppx_subpixel_refine.argtypes = [vp, vp, vp, i, i, i, i]
        lib.vppx_median3x3.argtypes = [vp, vp, vp, i, i]
        lib.vppx_rsgm_host.argtypes = [vp, pr, i, i, i, i, vp, vp, vp, vp, vp, vp]
        lib.vppx_rsgm_dev.argtypes = [vp, pr, i, i, i, i, vp, vp, vp, vp, vp, vp]
        lib.vppx_rsgm_post_dev.argtypes = [vp, i, i, i, vp, vp, i, vp]
        lib.vppx_rsgm_front_dev.argtypes = [vp, i, i, i, i, vp, vp, vp, vp, vp, vp]
        lib.vppx_rsgm_guided_rows_dev.argtypes = [vp, i, i, i, i, vp, vp, vp, vp, vp, vp, vp]
        lib.vppx_rsgm_mid_dev.argtypes = [vp, i, i, i, vp, vp, vp, vp]
        lib.vppx_vpp_rsgm_dev.argtypes = [vp, pv, pr, i, i, i, i, vp, vp, vp, vp, vp, vp, vp]
        po = C.POINTER(VppxOccParams)
        lib.vppx_occ_vpp_rsgm_host.argtypes = [vp, po, pv, pr, i, i, i, i, vp, vp, vp, vp, vp, vp, vp, vp, C.POINTER(C.c_uint64)]
        lib.vppx_occ_params_default.argtypes = [po]
        lib.vppx_occ_params_default.restype = None
        lib.vppx_occ_vpp_rsgm_dev.argtypes = [vp, po, pv, pr, i, i, i, i, vp, vp, vp, vp, vp, vp, vp]
        lib.vppx_occ_vpp_rsgm_guided_dev.argtypes = [vp, po, pv, pr, i, i, i, i, vp, vp, vp, vp, vp, vp, vp, vp, vp]
        lib.vppx_occ_vpp_rsgm_guided_host.argtypes = [vp, po, pv, pr, i, i, i, i, vp, vp, vp, vp, vp, vp, vp, vp, vp,
                                                      C.POINTER(C.c_uint64)]
        lib.vppx_inputs_ready_event.argtypes = [vp, vp]
        lib.vppx_u8_to_nchw_dev.argtypes = [vp, i, i, i, i, i, vp, vp, i]
        lib.vppx_psmnet_cost_volume_dev.argtypes = [vp, vp, vp, vp, vp, i, i, i, i, i, i, i, vp]
        lib.vppx_raft_corr_modulate_dev.argtypes = [vp, vp, vp, vp, i, i, i, i, i, i]
        lib.vppx_psmnet_cost_volume_dt_dev.argtypes = [vp, vp, vp, vp, vp, i, i, i, i, i, i, i, vp, i]
        lib.vppx_raft_corr_modulate_dt_dev.argtypes = [vp, vp, vp, vp, i, i, i, i, i, i, i]
        lib.vppx_raft_corr_pyramid_cells.argtypes = [C.c_int64, i, i, C.POINTER(C.c_int64)]
        lib.vppx_raft_corr_pyramid_cells.restype = C.c_int64
        lib.vppx_raft_corr_pyramid_dt_dev.argtypes = [vp, vp, vp, vp, i, i, i, i, i, i, i, vp, i]
        lib.vppx_raft_corr_fused_dt_dev.argtypes = [vp, vp, vp, vp, vp, i, i, i, i, i, i, i, i, vp, vp, i]
        lib.vppx_raft_corr_lookup_dt_dev.argtypes = [vp, vp, vp, vp, C.c_int64, i, i, i, i, i, i, vp, i]
        lib.vppx_psmnet_readout_dt_dev.argtypes = [vp, vp, i, i, i, i, i, i, i, i, i, i, i, vp, i]
        lib.vppx_raft_upsample_dt_dev.argtypes = [vp, vp, C.c_int64, vp, i, i, i, i, i, i, i, i, i, i, i, vp, i]
        i64 = C.c_int64
        lib.vppx_raft_gru_assemble_dt_dev.argtypes = [vp, C.POINTER(VppxGruSource), i, i, i, i, vp, i, i]
        lib.vppx_raft_gru_reset_dt_dev.argtypes = [vp, vp, i64, vp, i64, vp, i64, vp, i64, i, i, i, i, i, i]
        lib.vppx_raft_gru_update_dt_dev.argtypes = [vp, vp, i64, vp, i64, vp, i64, vp, i64, vp, i64, vp, i64, i, i, i, i, i]
        lib.vppx_raft_motion_front_dt_dev.argtypes = [vp, vp, vp, vp, i64, vp, i64, vp, vp, i, vp, vp, i, i, i, i, i, i, i, i, vp, i64, vp, i64,
                                                      i, i]
        lib.vppx_kitti_disp_decode_dev.argtypes = [vp, vp, C.c_int64, vp, vp]
        lib.vppx_pfm_decode_dev.argtypes = [vp, vp, i, i, i, i, vp]
        lib.vppx_png_decode_dev.argtypes = [vp, i, vp, C.POINTER(C.c_int64), i, i, i, f, vp, vp, vp, vp]
        lib.vppx_occlusion_heuristic_host.argtypes = [vp, i, i, i, vp, i, i, d, d, d, d, vp]
        lib.vppx_occlusion_heuristic_dev.argtypes = [vp, i, i, i, vp, i, i, d, d, d, d, vp]
        lib.vppx_occlusion_heuristic_full_host.argtypes = [vp, i, i, i, vp, i, i, d, d, d, d, vp, vp]
        lib.vppx_occlusion_heuristic_full_dev.argtypes = [vp, i, i, i, vp, i, i, d, d, d, d, vp, vp]
        lib.vppx_set_graph_mode.argtypes = [vp, i]
        lib.vppx_graph_replays.argtypes = [vp]
        lib.vppx_graph_replays.restype = C.c_long
        lib.vppx_time_aggregate.argtypes = [vp, i, C.POINTER(C.c_float)]
        lib.vppx_agg_kernel_ms.argtypes = [vp, i, C.POINTER(C.c_float), C.POINTER(C.c_int)]
        lib.vppx_we_kernel_ms.argtypes = [vp, i, C.POINTER(C.c_float), C.POINTER(C.c_int)]
        lib.vppx_time_aggregate_frames.argtypes = [vp]
        lib.vppx_time_aggregate_part.argtypes = [vp, i, i, C.POINTER(C.c_float)]
        lib.vppx_uses_vert.argtypes = [vp]
        lib.vppx_last_call_parts.argtypes = [vp]
        lib.vppx_we_last_pieces.argtypes = [vp]
        lib.vppx_wsum_last_pieces.argtypes = [vp]
        lib.vppx_wsum_default_route.argtypes = [i, i, i, i, i, i]
        lib.vppx_last_routes.argtypes = [vp, C.c_char_p, i]
        lib.vppx_last_front_routes.argtypes = [vp, C.c_char_p, i]
        lib.vppx_fused_pixels_per_wave.argtypes = [vp]
        lib.vppx_batch_quantum.argtypes = [vp, i, i, i]
        lib.vppx_enable_stage_timing.argtypes = [vp, i]
        lib.vppx_get_stage_ms.argtypes = [vp, C.POINTER(C.c_float), i]
        lib.vppx_fstream_create.argtypes = [vp, po, pv, pr, i, i, i, i, i, i, i, C.POINTER(vp)]
        lib.vppx_fstream_destroy.argtypes = [vp]
        lib.vppx_fstream_destroy.restype = None
        lib.vppx_fstream_push.argtypes = [vp, vp, vp, vp, vp]
        lib.vppx_fstream_push_guided.argtypes = [vp, vp, vp, vp, vp, vp]
        lib.vppx_fstream_flush.argtypes = [vp]
        lib.vppx_fstream_pop.argtypes = [vp, vp, vp, vp, vp, C.POINTER(C.c_uint64), C.POINTER(C.c_int)]
        ps = C.POINTER(VppxScaleParams)
        lib.vppx_scale_params_default.argtypes = [ps]
        lib.vppx_scale_params_default.restype = None
        pi = C.POINTER(C.c_int)
        lib.vppx_scaled_shape.argtypes = [i, i, ps, pi, pi, pi, pi]
        lib.vppx_scale_table_builds.argtypes = [vp]
        lib.vppx_scale_table_builds.restype = C.c_long
        lib.vppx_last_front_sets.argtypes = [vp, pi, pi]
        lib.vppx_occ_vpp_rsgm_scaled_dev.argtypes = [vp, po, pv, pr, ps, i, i, i, i, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
        lib.vppx_occ_vpp_rsgm_scaled_host.argtypes = [vp, po, pv, pr, ps, i, i, i, i, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp,
                                                      C.POINTER(C.c_uint64)]
        lib.vppx_fstream_create_scaled.argtypes = [vp, po, pv, pr, ps, i, i, i, i, i, i, i, C.POINTER(vp)]
        p64 = C.POINTER(C.c_int64)
        lib.vppx_fstream_counts.argtypes = [vp, p64, p64, p64, p64]
        pe = C.POINTER(VppxEvalParams)
        lib.vppx_eval_params_default.argtypes = [pe]
        lib.vppx_eval_params_default.restype = None
        lib.vppx_guided_metrics_dev.argtypes = [vp, pe, i, i, i, vp, i, i, vp, vp, vp, vp]
        lib.vppx_guided_metrics_host.argtypes = [vp, pe, i, i, i, vp, i, i, vp, vp, vp, vp]
        lib.vppx_occ_vpp_rsgm_eval_dev.argtypes = [vp, po, pv, pr, ps, pe, i, i, i, i, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
        lib.vppx_fstream_create_eval.argtypes = [vp, po, pv, pr, ps, pe, i, i, i, i, i, i, i, C.POINTER(vp)]
        lib.vppx_fstream_push_eval.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp]
        lib.vppx_fstream_pop_eval.argtypes = [vp, vp, vp, vp, vp, C.POINTER(C.c_uint64), C.POINTER(VppxMetrics), C.POINTER(C.c_int)]
        u = C.c_uint
        for sfx in ("dev", "host"):
            getattr(lib, "vppx_error_colors_" + sfx).argtypes = [vp, i, i, i, vp, vp, d, i, i, vp]
            getattr(lib, "vppx_guided_visualize_" + sfx).argtypes = [vp, i, i, i, vp, vp, vp, d, i, u, vp]
            getattr(lib, "vppx_colorize_" + sfx).argtypes = [vp, i, i, i, vp, vp, vp, i, vp]
        lib.vppx_finite_max_dev.argtypes = [vp, i, i, i, vp, vp]
        pm = C.POINTER(VppxSampleParams)
        lib.vppx_sample_params_default.argtypes = [pm]
        lib.vppx_sample_params_default.restype = None
        lib.vppx_sample_threshold.argtypes = [d]
        lib.vppx_sample_threshold.restype = C.c_uint32
        lib.vppx_sample_hints_dev.argtypes = [vp, pm, i, i, i, vp, vp, vp, vp]
        lib.vppx_sample_hints_host.argtypes = [vp, pm, i, i, i, vp, vp, vp, vp]
        lib.vppx_occ_vpp_rsgm_sampled_dev.argtypes = [vp, po, pv, pr, ps, pe, pm, i, i, i, i, vp, vp, vp, vp, i, vp, vp, vp, vp, vp, vp, vp, vp,
                                                      vp, vp, vp, vp]
        lib.vppx_fstream_create_sampled.argtypes = [vp, po, pv, pr, ps, pe, pm, i, i, i, i, i, i, i, C.POINTER(vp)]
        lib.vppx_fstream_push_sampled.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp]
        _lib = lib
        return lib


def split_routes(s):
    """Split vppx_last_routes' list at the commas outside <>."""
    out, depth, cur = [], 0, []
    for ch in s:
        if ch == "," and depth == 0:
            out.append("".join(cur))
            cur = []
            continue
        depth += (ch == "<") - (ch == ">")
        cur.append(ch)
    if cur:
        out.append("".join(cur))
    return out


def _route_list(fn, handle):
    n = check(fn(handle, None, 0))
    buf = C.create_string_buffer(n + 1)
    check(fn(handle, buf, n + 1))
    return split_routes(buf.value.decode())


def last_routes(lib, handle):
    return _route_list(lib.vppx_last_routes, handle)


def last_front_routes(lib, handle):
    return _route_list(lib.vppx_last_front_routes, handle)


def check(rc):
    """Turn a negative return code into the reference's `raise Exception(msg)`."""
    if rc is not None and rc < 0:
        msg = load().vppx_last_error().decode("utf-8", "replace")
        raise VppxError(rc, msg or ERR_NAMES.get(rc, f"vppx error {rc}"))
    return rc


def np_ptr(a):
    return C.c_void_p(a.ctypes.data) if a is not None else None


class Context:
    """One vppx_ctx (one GPU, one stream, one workspace arena)."""

    def __init__(self, device=-1):
        self._lib = load()
        self._h = C.c_void_p()
        check(self._lib.vppx_create(C.byref(self._h), int(device)))

    @property
    def handle(self):
        return self._h

    def close(self):
        if self._h:
            self._lib.vppx_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_stream(self, stream_ptr):
        """Bind a hipStream_t handle; 0 / None = the legacy default stream (torch's default stream)."""
        if not stream_ptr:
            check(self._lib.vppx_set_stream_legacy(self._h))
        else:
            check(self._lib.vppx_set_stream(self._h, C.c_void_p(stream_ptr)))

    def use_own_stream(self):
        """Back to the context's private non-blocking stream (what a fresh context uses)."""
        check(self._lib.vppx_set_stream(self._h, None))

    def synchronize(self):
        """Wait for the context's stream; raises VppxError when a fused aggregation launch lost its lock step."""
        check(self._lib.vppx_synchronize(self._h))

    def status(self):
        """Non-blocking health check (vppx_status): raises VppxError for a lost lock step seen so far."""
        check(self._lib.vppx_status(self._h))

    @property
    def lockstep_failures(self):
        return int(self._lib.vppx_lockstep_failures(self._h))

    @property
    def device_name(self):
        return self._lib.vppx_device_name(self._h).decode()

    @property
    def workspace_bytes(self):
        return int(self._lib.vppx_workspace_bytes(self._h))


_default_ctx = None


def default_context():
    """Process-wide context used by the drop-in module-level functions (the reference's
    natives are free functions with global libc rand() state)."""
    global _default_ctx
    if _default_ctx is None:
        dev = -1
        lr = os.environ.get("LOCAL_RANK")
        if lr is not None:
            try:
                import torch
                if torch.cuda.device_count() > int(lr):
                    dev = int(lr)
            except Exception:
                dev = -1
        _default_ctx = Context(dev)
    return _default_ctx


def _fill(p, kw):
    # setattr on a ctypes.Structure silently creates a Python attribute for an unknown name: a misspelt or
    # reference-style keyword (blending=, wsizeAgg_x=) must not be ignored
    names = {f[0] for f in p._fields_ if not f[0].startswith("reserved")}
    for k, v in kw.items():
        if k not in names:
            raise TypeError(f"{type(p).__name__}: unknown parameter {k!r} (fields: {sorted(names)})")
        setattr(p, k, v)
    return p


def vpp_params(**kw):
    p = VppxVppParams()
    load().vppx_vpp_params_default(C.byref(p))
    return _fill(p, kw)


def occ_params(**kw):
    p = VppxOccParams()
    load().vppx_occ_params_default(C.byref(p))
    return _fill(p, kw)


def rsgm_params(**kw):
    p = VppxRsgmParams()
    load().vppx_rsgm_params_default(C.byref(p))
    return _fill(p, kw)


def scale_params(**kw):
    """VppxScaleParams: iscale / oscale of test.py:36-37 (defaults 1, 1)."""
    p = VppxScaleParams()
    load().vppx_scale_params_default(C.byref(p))
    return _fill(p, kw)


def eval_params(**kw):
    """VppxEvalParams: gt_scale = --oscale of test.py:150-152 (default 1)."""
    p = VppxEvalParams()
    load().vppx_eval_params_default(C.byref(p))
    return _fill(p, kw)


def sample_params(**kw):
    """VppxSampleParams: probability = --guideperc (default 0.05), seed (default 1)."""
    p = VppxSampleParams()
    load().vppx_sample_params_default(C.byref(p))
    return _fill(p, kw)


def sample_threshold(p):
    """T of the sampling rule (include/vppx.h): torch's ``rand < p`` on float32 rand = k * 2**-24 is exactly ``k < T`` with
    T = clamp(ceil(float64(float32(p)) * 2**24), 0, 2**24); NaN selects nothing.  Host arithmetic, no library call."""
    pf = float(np.float32(p))
    if not pf > 0.0:
        return 0
    if pf >= 1.0:
        return 1 << 24
    return min(int(np.ceil(pf * 16777216.0)), 1 << 24)


def check_gt_shape(Hg, Wg, gt_scale, Ho, Wo, what="gt"):
    """What the library checks before it launches anything (vppx_guided_metrics_dev): gt_scale takes gt to the map's shape."""
    s = int(gt_scale)
    if s < 1:
        raise ValueError(f"gt_scale {s} (>= 1)")
    if (Hg // s, Wg // s) != (Ho, Wo):
        raise ValueError(f"{what} of {Hg} x {Wg} at gt_scale {s} is {Hg // s} x {Wg // s}, the disparity map is {Ho} x {Wo}")


def metrics_dict(rec):
    """One VppxMetrics record (ctypes struct or a sequence of its 8 doubles) -> the reference's dict (losses.py:24)."""
    v = [rec.bad1, rec.bad2, rec.bad3, rec.bad4, rec.avgerr, rec.rms] if isinstance(rec, VppxMetrics) else [float(x) for x in rec[:6]]
    return dict(zip(METRIC_KEYS, v))


def viz_which(which):
    """`which` of guided_visualize: None (all six), a VPPX_VIZ_* bit mask, one of the reference's keys, or an iterable of keys."""
    if which is None:
        return VIZ_ALL
    if isinstance(which, str):
        which = [which]
    if isinstance(which, int):
        w = which
    else:
        w = 0
        for k in which:
            if k not in VIZ_KEYS:
                raise ValueError(f"which: unknown map {k!r} (one of {VIZ_KEYS})")
            w |= 1 << VIZ_KEYS.index(k)
    if w <= 0 or w & ~VIZ_ALL:
        raise ValueError(f"which: {which!r} selects no map of {VIZ_KEYS}")
    return w


def scaled_shape(H, W, iscale=1, oscale=1):
    """(h, w, Ho, Wo): the shape the matcher runs at and the shape of the returned map (vppx_scaled_shape)."""
    sp = scale_params(iscale=int(iscale), oscale=int(oscale))
    v = [C.c_int(0) for _ in range(4)]
    check(load().vppx_scaled_shape(int(H), int(W), C.byref(sp), *[C.byref(x) for x in v]))
    return tuple(int(x.value) for x in v)


def c_contig(a, dtype):
    a = np.ascontiguousarray(a, dtype=dtype)
    return a
