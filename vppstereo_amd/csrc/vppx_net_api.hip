// vppx_net_api.hip -- C-ABI entry points of the network hand-off (declared in include/vppx.h): the patterned pair to
// PSMNet / RAFT-Stereo, the correlation, read-out, update-block and encoder calls, the convolution and the payload decoders.
// Host-side checks and sequencing only, as vppx_api.hip: every refusal comes before anything is launched.
#include "vppx_internal.h"

#include <math.h>

// ---------------------------------------------------------------------------------------
// hand-off of the patterned pair to PSMNet / RAFT-Stereo (test.py:179-200)
// ---------------------------------------------------------------------------------------
extern "C" int vppx_u8_to_nchw_dev(vppx_ctx *ctx, int B, int H, int W, int C, int pad_multiple, const uint8_t *src,
                                   void *dst, int dst_is_bf16)
{
    int rc;
    VPPX_ENTER(ctx);
    if (!src || !dst || B <= 0 || H <= 0 || W <= 0 || C <= 0 || pad_multiple <= 0) { vppx_set_error("vppx_u8_to_nchw: bad arguments"); return VPPX_E_INVALID_ARG; }
    return rsgm_launch_to_nchw(ctx, B, H, W, C, pad_multiple, src, dst, dst_is_bf16 != 0);
}

// ---------------------------------------------------------------------------------------
// hand-off rows: PSMNet volume, RAFT correlation modulation, payload decoders
// ---------------------------------------------------------------------------------------
static bool handoff_dtype_ok(const char *who, int dtype, const char *what = "dtype")
{
    if (dtype == VPPX_DT_F32 || dtype == VPPX_DT_BF16) return true;
    vppx_set_error("%s: %s %d is neither VPPX_DT_F32 (0) nor VPPX_DT_BF16 (1)", who, what, dtype);
    return false;
}

extern "C" int vppx_psmnet_cost_volume_dt_dev(vppx_ctx *ctx, const void *fea_l, const void *fea_r, const float *hints,
                                              const float *validhints, int B, int C, int H4, int W4, int H, int W,
                                              int maxdisp, void *cost, int dtype)
{
    int rc;
    VPPX_ENTER(ctx);
    if (!fea_l || !fea_r || !cost || B <= 0 || C <= 0 || H4 <= 0 || W4 <= 0 || maxdisp < 4 || (hints && !validhints)) {
        vppx_set_error("vppx_psmnet_cost_volume: bad arguments");
        return VPPX_E_INVALID_ARG;
    }
    if (!handoff_dtype_ok("vppx_psmnet_cost_volume", dtype)) return VPPX_E_INVALID_ARG;
    return handoff_psmnet_cost_volume(ctx, fea_l, fea_r, hints, validhints, B, C, H4, W4, H, W, maxdisp, cost, dtype);
}

extern "C" int vppx_psmnet_cost_volume_dev(vppx_ctx *ctx, const float *fea_l, const float *fea_r, const float *hints,
                                           const float *validhints, int B, int C, int H4, int W4, int H, int W,
                                           int maxdisp, float *cost)
{
    return vppx_psmnet_cost_volume_dt_dev(ctx, fea_l, fea_r, hints, validhints, B, C, H4, W4, H, W, maxdisp, cost, VPPX_DT_F32);
}

extern "C" int vppx_raft_corr_modulate_dt_dev(vppx_ctx *ctx, void *corr, const float *hints, const float *validhints, int B,
                                              int H4, int W2, int W3, int H, int W, int dtype)
{
    int rc;
    VPPX_ENTER(ctx);
    if (!corr || !hints || !validhints || B <= 0 || H4 <= 0 || W2 <= 0 || W3 <= 0) {
        vppx_set_error("vppx_raft_corr_modulate: bad arguments");
        return VPPX_E_INVALID_ARG;
    }
    if (!handoff_dtype_ok("vppx_raft_corr_modulate", dtype)) return VPPX_E_INVALID_ARG;
    return handoff_raft_corr_modulate(ctx, corr, hints, validhints, B, H4, W2, W3, H, W, dtype);
}

extern "C" int vppx_raft_corr_modulate_dev(vppx_ctx *ctx, float *corr, const float *hints, const float *validhints, int B,
                                           int H4, int W2, int W3, int H, int W)
{
    return vppx_raft_corr_modulate_dt_dev(ctx, corr, hints, validhints, B, H4, W2, W3, H, W, VPPX_DT_F32);
}

// CorrBlock1D's pyramid and lookup (corr_kernels.hip).  Every refusal comes before anything is launched.
extern "C" int64_t vppx_raft_corr_pyramid_cells(int64_t N, int W3, int levels, int64_t *offsets)
{
    if (N <= 0 || W3 <= 0 || levels < 1) {
        vppx_set_error("vppx_raft_corr_pyramid_cells: bad arguments");
        return VPPX_E_INVALID_ARG;
    }
    if (levels > VPPX_CORR_MAX_LEVELS) {
        vppx_set_error("vppx_raft_corr_pyramid_cells: %d levels, at most %d are built", levels, VPPX_CORR_MAX_LEVELS);
        return VPPX_E_UNSUPPORTED;
    }
    return corr_pyramid_offsets(N, W3, levels, offsets);
}

static int corr_shape_ok(const char *who, int B, int H4, int W2, int W3, int levels, int radius, int dtype)
{
    if (B <= 0 || H4 <= 0 || W2 <= 0 || W3 <= 0 || levels < 1 || radius < 0) {
        vppx_set_error("%s: bad arguments", who);
        return VPPX_E_INVALID_ARG;
    }
    if (!handoff_dtype_ok(who, dtype)) return VPPX_E_INVALID_ARG;
    if (levels > VPPX_CORR_MAX_LEVELS || radius > VPPX_CORR_MAX_RADIUS) {
        vppx_set_error("%s: %d levels of radius %d, at most %d levels and radius %d are built", who, levels, radius, VPPX_CORR_MAX_LEVELS,
                       VPPX_CORR_MAX_RADIUS);
        return VPPX_E_UNSUPPORTED;
    }
    if ((W3 >> (levels - 1)) < 2) {
        vppx_set_error("%s: level %d of a %d-wide row has %d cells; the lookup divides by that width - 1, so 2 is the least", who,
                       levels - 1, W3, W3 >> (levels - 1));
        return VPPX_E_INVALID_ARG;
    }
    return 0;
}

extern "C" int vppx_raft_corr_pyramid_dt_dev(vppx_ctx *ctx, void *corr, const float *hints, const float *validhints, int B, int H4,
                                             int W2, int W3, int H, int W, int levels, void *pyr, int dtype)
{
    int rc;
    VPPX_ENTER(ctx);
    if (!corr || (hints && !validhints) || (!pyr && levels > 1)) {
        vppx_set_error("vppx_raft_corr_pyramid: bad arguments");
        return VPPX_E_INVALID_ARG;
    }
    if ((rc = corr_shape_ok("vppx_raft_corr_pyramid", B, H4, W2, W3, levels, 0, dtype))) return rc;
    return corr_pyramid(ctx, corr, hints, validhints, B, H4, W2, W3, H, W, levels, pyr, dtype);
}

extern "C" int vppx_raft_corr_fused_dt_dev(vppx_ctx *ctx, const void *fmap2, const void *fmap3, const float *hints,
                                           const float *validhints, int B, int D, int H4, int W2, int W3, int H, int W, int levels,
                                           void *corr, void *pyr, int dtype)
{
    int rc;
    VPPX_ENTER(ctx);
    if (!fmap2 || !fmap3 || !corr || (hints && !validhints) || (!pyr && levels > 1) || D <= 0) {
        vppx_set_error("vppx_raft_corr_fused: bad arguments");
        return VPPX_E_INVALID_ARG;
    }
    if ((rc = corr_shape_ok("vppx_raft_corr_fused", B, H4, W2, W3, levels, 0, dtype))) return rc;
    return corr_fused(ctx, fmap2, fmap3, hints, validhints, B, D, H4, W2, W3, H, W, levels, corr, pyr, dtype);
}

// a frame stride holds at least the frame
static int gru_stride_ok(const char *who, const char *what, int64_t stride, int C, int H, int W)
{
    if (stride < (int64_t)C * H * W) {
        vppx_set_error("%s: %s_frame_stride %lld is less than %d planes of %dx%d", who, what, (long long)stride, C, H, W);
        return VPPX_E_INVALID_ARG;
    }
    return 0;
}

static int coords_stride_ok(const char *who, int64_t stride, int H4, int W2)
{
    if (stride < (int64_t)H4 * W2) {
        vppx_set_error("%s: coords_frame_stride %lld is less than one %dx%d plane", who, (long long)stride, H4, W2);
        return VPPX_E_INVALID_ARG;
    }
    return 0;
}

extern "C" int vppx_raft_corr_lookup_dt_dev(vppx_ctx *ctx, const void *corr, const void *pyr, const float *coords_x,
                                            int64_t coords_frame_stride, int B, int H4, int W2, int W3, int levels, int radius,
                                            float *out, int dtype)
{
    int rc;
    VPPX_ENTER(ctx);
    if (!corr || !coords_x || !out || (!pyr && levels > 1)) {
        vppx_set_error("vppx_raft_corr_lookup: bad arguments");
        return VPPX_E_INVALID_ARG;
    }
    if ((rc = corr_shape_ok("vppx_raft_corr_lookup", B, H4, W2, W3, levels, radius, dtype))) return rc;
    if ((rc = coords_stride_ok("vppx_raft_corr_lookup", coords_frame_stride, H4, W2))) return rc;
    return corr_lookup(ctx, corr, pyr, coords_x, coords_frame_stride, B, H4, W2, W3, levels, radius, out, dtype);
}

// The read-out of the two networks (readout_kernels.hip).  Every refusal comes before anything is launched.
static int readout_window_ok(const char *who, int H, int W, int top, int left, int Hout, int Wout)
{
    if (top < 0 || left < 0 || Hout <= 0 || Wout <= 0 || (int64_t)top + Hout > H || (int64_t)left + Wout > W) {
        vppx_set_error("%s: the window of %dx%d pixels at row %d, column %d is not inside the %dx%d map", who, Hout, Wout, top, left, H, W);
        return VPPX_E_INVALID_ARG;
    }
    return 0;
}

extern "C" int vppx_psmnet_readout_dt_dev(vppx_ctx *ctx, const void *cost, int B, int D4, int H4, int W4, int maxdisp, int H, int W,
                                          int top, int left, int Hout, int Wout, float *out, int dtype)
{
    int rc;
    VPPX_ENTER(ctx);
    if (!cost || !out || B <= 0 || D4 <= 0 || H4 <= 0 || W4 <= 0 || maxdisp <= 0 || H <= 0 || W <= 0) {
        vppx_set_error("vppx_psmnet_readout: bad arguments");
        return VPPX_E_INVALID_ARG;
    }
    if (!handoff_dtype_ok("vppx_psmnet_readout", dtype)) return VPPX_E_INVALID_ARG;
    if ((rc = readout_window_ok("vppx_psmnet_readout", H, W, top, left, Hout, Wout))) return rc;
    return readout_psm(ctx, cost, B, D4, H4, W4, maxdisp, H, W, top, left, Hout, Wout, out, dtype);
}

extern "C" int vppx_raft_upsample_dt_dev(vppx_ctx *ctx, const void *flow, int64_t flow_frame_stride, const void *mask, int B, int C,
                                         int H4, int W4, int f, int mask_channels, int sign, int top, int left, int Hout, int Wout,
                                         float *out, int dtype)
{
    int rc;
    VPPX_ENTER(ctx);
    if (!flow || !mask || !out || B <= 0 || C <= 0 || H4 <= 0 || W4 <= 0 || (sign != 1 && sign != -1)) {
        vppx_set_error("vppx_raft_upsample: bad arguments (sign is +1 or -1)");
        return VPPX_E_INVALID_ARG;
    }
    if (!handoff_dtype_ok("vppx_raft_upsample", dtype)) return VPPX_E_INVALID_ARG;
    if (f != 1 && f != 2 && f != 4 && f != 8) {
        vppx_set_error("vppx_raft_upsample: factor %d is not 1, 2, 4 or 8", f);
        return VPPX_E_INVALID_ARG;
    }
    if (mask_channels != 9 * f * f) {
        vppx_set_error("vppx_raft_upsample: the mask has %d channels, factor %d takes 9*%d*%d = %d", mask_channels, f, f, f, 9 * f * f);
        return VPPX_E_INVALID_ARG;
    }
    if (flow_frame_stride < (int64_t)C * H4 * W4) {
        vppx_set_error("vppx_raft_upsample: flow_frame_stride %lld is less than %d planes of %dx%d", (long long)flow_frame_stride, C, H4, W4);
        return VPPX_E_INVALID_ARG;
    }
    if ((int64_t)f * H4 > 0x7FFFFFFF || (int64_t)f * W4 > 0x7FFFFFFF) {
        vppx_set_error("vppx_raft_upsample: a %dx%d map times %d is more than the call takes", H4, W4, f);
        return VPPX_E_UNSUPPORTED;
    }
    if ((rc = readout_window_ok("vppx_raft_upsample", f * H4, f * W4, top, left, Hout, Wout))) return rc;
    return readout_raft_upsample(ctx, flow, flow_frame_stride, mask, B, C, H4, W4, f, sign, top, left, Hout, Wout, out, dtype);
}

// The update block's glue (gru_kernels.hip).  Every refusal comes before anything is launched.
static int gru_shape_ok(const char *who, int B, int C, int H, int W, int dtype)
{
    if (B <= 0 || C <= 0 || H <= 0 || W <= 0) {
        vppx_set_error("%s: bad arguments (B, C, H and W must be positive)", who);
        return VPPX_E_INVALID_ARG;
    }
    if (!handoff_dtype_ok(who, dtype)) return VPPX_E_INVALID_ARG;
    if ((int64_t)H * W > 0x7FFFFFFF) {
        vppx_set_error("%s: a %dx%d map is more than the call takes", who, H, W);
        return VPPX_E_UNSUPPORTED;
    }
    return 0;
}

// both assemble calls: the strided one's destination is checked by its frame stride, the other's by its channels
static int gru_assemble_call(const char *who, bool strided, vppx_ctx *ctx, const VppxGruSource *sources, int n_sources, int B, int H, int W,
                             void *hx, int hx_channels, int64_t hx_frame_stride, int dtype)
{
    int rc;
    VPPX_ENTER(ctx);
    if (!sources || !hx) {
        vppx_set_error("%s: bad arguments", who);
        return VPPX_E_INVALID_ARG;
    }
    if (n_sources < 1 || n_sources > VPPX_GRU_MAX_SOURCES) {
        vppx_set_error("%s: %d sources, 1 .. %d are taken", who, n_sources, VPPX_GRU_MAX_SOURCES);
        return VPPX_E_INVALID_ARG;
    }
    if ((rc = gru_shape_ok(who, B, 1, H, W, dtype))) return rc;
    int64_t channels = 0;
    for (int k = 0; k < n_sources; k++) {
        const VppxGruSource &s = sources[k];
        if (!s.ptr || s.C <= 0 || s.Hs <= 0 || s.Ws <= 0) {
            vppx_set_error("%s: source %d: bad arguments", who, k);
            return VPPX_E_INVALID_ARG;
        }
        if ((int64_t)s.Hs * s.Ws > 0x7FFFFFFF) {
            vppx_set_error("%s: source %d: a %dx%d map is more than the call takes", who, k, s.Hs, s.Ws);
            return VPPX_E_UNSUPPORTED;
        }
        if (s.mode == VPPX_GRU_COPY) {
            if (s.Hs != H || s.Ws != W) {
                vppx_set_error("%s: source %d is copied and is %dx%d, hx is %dx%d", who, k, s.Hs, s.Ws, H, W);
                return VPPX_E_INVALID_ARG;
            }
        } else if (s.mode == VPPX_GRU_POOL2X) {
            if ((s.Hs - 1) / 2 + 1 != H || (s.Ws - 1) / 2 + 1 != W) {
                vppx_set_error("%s: source %d is %dx%d and pools to %dx%d, hx is %dx%d", who, k, s.Hs, s.Ws, (s.Hs - 1) / 2 + 1,
                               (s.Ws - 1) / 2 + 1, H, W);
                return VPPX_E_INVALID_ARG;
            }
        } else if (s.mode != VPPX_GRU_INTERP) {
            vppx_set_error("%s: source %d: mode %d is not VPPX_GRU_COPY, VPPX_GRU_POOL2X or VPPX_GRU_INTERP", who, k, s.mode);
            return VPPX_E_INVALID_ARG;
        }
        if ((rc = gru_stride_ok(who, "source", s.frame_stride, s.C, s.Hs, s.Ws))) return rc;
        channels += s.C;
    }
    if (strided) {
        if (hx_frame_stride < channels * H * W) {
            vppx_set_error("%s: out_frame_stride %lld is less than the sources' %lld planes of %dx%d", who, (long long)hx_frame_stride,
                           (long long)channels, H, W);
            return VPPX_E_INVALID_ARG;
        }
        return gru_assemble(ctx, sources, n_sources, B, H, W, hx, hx_frame_stride, dtype);
    }
    if (hx_channels < channels) {
        vppx_set_error("%s: hx has %d channels, the sources have %lld", who, hx_channels, (long long)channels);
        return VPPX_E_INVALID_ARG;
    }
    return gru_assemble(ctx, sources, n_sources, B, H, W, hx, (int64_t)hx_channels * H * W, dtype);
}

extern "C" int vppx_raft_gru_assemble_dt_dev(vppx_ctx *ctx, const VppxGruSource *sources, int n_sources, int B, int H, int W, void *hx,
                                             int hx_channels, int dtype)
{
    return gru_assemble_call("vppx_raft_gru_assemble", false, ctx, sources, n_sources, B, H, W, hx, hx_channels, 0, dtype);
}

// the same into a channel slice: the destination's frames out_frame_stride cells apart (PSMNet's 320-channel feature buffer)
extern "C" int vppx_raft_gru_assemble_strided_dt_dev(const VppxGruSource *sources, int n_sources, int B, int H, int W, void *out,
                                                     int64_t out_frame_stride, int dtype, vppx_ctx *ctx)
{
    return gru_assemble_call("vppx_raft_gru_assemble_strided", true, ctx, sources, n_sources, B, H, W, out, 0, out_frame_stride, dtype);
}

extern "C" int vppx_raft_gru_reset_dt_dev(vppx_ctx *ctx, const void *ar, int64_t ar_frame_stride, const void *cr, int64_t cr_frame_stride,
                                          const void *h, int64_t h_frame_stride, void *hx, int64_t hx_frame_stride, int B, int C, int H,
                                          int W, int hx_channels, int dtype)
{
    static const char *who = "vppx_raft_gru_reset";
    int rc;
    VPPX_ENTER(ctx);
    if (!ar || !cr || !h || !hx) {
        vppx_set_error("%s: bad arguments", who);
        return VPPX_E_INVALID_ARG;
    }
    if ((rc = gru_shape_ok(who, B, C, H, W, dtype))) return rc;
    if (hx_channels < C) {
        vppx_set_error("%s: hx has %d channels, h has %d", who, hx_channels, C);
        return VPPX_E_INVALID_ARG;
    }
    if ((rc = gru_stride_ok(who, "ar", ar_frame_stride, C, H, W)) || (rc = gru_stride_ok(who, "cr", cr_frame_stride, C, H, W)) ||
        (rc = gru_stride_ok(who, "h", h_frame_stride, C, H, W)) || (rc = gru_stride_ok(who, "hx", hx_frame_stride, hx_channels, H, W)))
        return rc;
    return gru_reset(ctx, ar, ar_frame_stride, cr, cr_frame_stride, h, h_frame_stride, hx, hx_frame_stride, B, C, H, W, dtype);
}

extern "C" int vppx_raft_gru_update_dt_dev(vppx_ctx *ctx, const void *az, int64_t az_frame_stride, const void *cz, int64_t cz_frame_stride,
                                           const void *aq, int64_t aq_frame_stride, const void *cq, int64_t cq_frame_stride, const void *h,
                                           int64_t h_frame_stride, void *out, int64_t out_frame_stride, int B, int C, int H, int W,
                                           int dtype)
{
    static const char *who = "vppx_raft_gru_update";
    int rc;
    VPPX_ENTER(ctx);
    if (!az || !cz || !aq || !cq || !h || !out) {
        vppx_set_error("%s: bad arguments", who);
        return VPPX_E_INVALID_ARG;
    }
    if ((rc = gru_shape_ok(who, B, C, H, W, dtype))) return rc;
    if ((rc = gru_stride_ok(who, "az", az_frame_stride, C, H, W)) || (rc = gru_stride_ok(who, "cz", cz_frame_stride, C, H, W)) ||
        (rc = gru_stride_ok(who, "aq", aq_frame_stride, C, H, W)) || (rc = gru_stride_ok(who, "cq", cq_frame_stride, C, H, W)) ||
        (rc = gru_stride_ok(who, "h", h_frame_stride, C, H, W)) || (rc = gru_stride_ok(who, "out", out_frame_stride, C, H, W)))
        return rc;
    return gru_update(ctx, az, az_frame_stride, cz, cz_frame_stride, aq, aq_frame_stride, cq, cq_frame_stride, h, h_frame_stride, out,
                      out_frame_stride, B, C, H, W, dtype);
}

// The motion encoder's front (motion_kernels.hip).  Every refusal comes before anything is launched; the lookup's come first.
extern "C" int vppx_raft_motion_front_dt_dev(vppx_ctx *ctx, const void *corr, const void *pyr, const float *coords_x,
                                             int64_t coords_frame_stride, const float *flow, int64_t flow_frame_stride, const float *wc,
                                             const float *bias_c, int Cc, const float *wf, const float *bias_f, int Cf, int ks, int B,
                                             int H4, int W2, int W3, int levels, int radius, void *out_c, int64_t out_c_frame_stride,
                                             void *out_f, int64_t out_f_frame_stride, int dtype, int out_dtype)
{
    static const char *who = "vppx_raft_motion_front";
    int rc;
    VPPX_ENTER(ctx);
    if (!corr || !coords_x || !flow || !wc || !wf || !out_c || !out_f || (!pyr && levels > 1)) {
        vppx_set_error("%s: bad arguments", who);
        return VPPX_E_INVALID_ARG;
    }
    if ((rc = corr_shape_ok(who, B, H4, W2, W3, levels, radius, dtype))) return rc;
    if ((rc = coords_stride_ok(who, coords_frame_stride, H4, W2))) return rc;
    if (!handoff_dtype_ok(who, out_dtype, "out_dtype")) return VPPX_E_INVALID_ARG;
    if (Cc <= 0 || Cf <= 0 || ks < 1 || ks % 2 == 0) {
        vppx_set_error("%s: %d and %d output channels and a %dx%d window: the channels must be positive and the window odd", who, Cc, Cf, ks,
                       ks);
        return VPPX_E_INVALID_ARG;
    }
    if (Cc % 16 || Cf % 16 || Cc > VPPX_MOTION_MAX_CH || Cf > VPPX_MOTION_MAX_CH || ks > VPPX_MOTION_MAX_KS) {
        vppx_set_error("%s: %d and %d output channels and a %dx%d window: multiples of 16 up to %d and windows up to %dx%d are built", who,
                       Cc, Cf, ks, ks, VPPX_MOTION_MAX_CH, VPPX_MOTION_MAX_KS, VPPX_MOTION_MAX_KS);
        return VPPX_E_UNSUPPORTED;
    }
    if ((rc = gru_stride_ok(who, "flow", flow_frame_stride, 2, H4, W2)) || (rc = gru_stride_ok(who, "out_c", out_c_frame_stride, Cc, H4, W2)) ||
        (rc = gru_stride_ok(who, "out_f", out_f_frame_stride, Cf, H4, W2)))
        return rc;
    return motion_front(ctx, corr, pyr, coords_x, coords_frame_stride, flow, flow_frame_stride, wc, bias_c, Cc, wf, bias_f, Cf, ks, B, H4, W2,
                        W3, levels, radius, out_c, out_c_frame_stride, out_f, out_f_frame_stride, dtype, out_dtype);
}

// The encoders' glue (norm_kernels.hip).  Flat arguments with the context last (include/vppx.h says why); every refusal
// comes before anything is launched.
static int norm_stats_stride_ok(const char *who, const char *what, int64_t stride, int C)
{
    if (stride != 0 && stride != 2 * (int64_t)C) {
        vppx_set_error("%s: %s_frame_stride %lld is neither 0 (one set for every frame) nor 2*C = %d", who, what, (long long)stride, 2 * C);
        return VPPX_E_INVALID_ARG;
    }
    return 0;
}

extern "C" int vppx_raft_norm_stats_dt_dev(const void *x, int64_t x_frame_stride, int B, int C, int H, int W, double eps, float *stats,
                                           int dtype, vppx_ctx *ctx)
{
    static const char *who = "vppx_raft_norm_stats";
    int rc;
    VPPX_ENTER(ctx);
    if (!x || !stats) {
        vppx_set_error("%s: bad arguments", who);
        return VPPX_E_INVALID_ARG;
    }
    if ((rc = gru_shape_ok(who, B, C, H, W, dtype)) || (rc = gru_stride_ok(who, "x", x_frame_stride, C, H, W))) return rc;
    if (!(eps > 0.0) || !(eps <= 1.7976931348623157e308)) {
        vppx_set_error("%s: eps %g is not a positive finite number", who, eps);
        return VPPX_E_INVALID_ARG;
    }
    return norm_stats(ctx, x, x_frame_stride, B, C, H, W, eps, stats, dtype);
}

extern "C" int vppx_raft_norm_apply_dt_dev(const void *x, int64_t x_frame_stride, const float *stats, int64_t stats_frame_stride,
                                           const float *weight, const float *bias, int relu_inner, const void *res,
                                           int64_t res_frame_stride, const float *res_stats, int64_t res_stats_frame_stride,
                                           const float *res_weight, const float *res_bias, void *out, int64_t out_frame_stride, int B,
                                           int C, int H, int W, int dtype, vppx_ctx *ctx)
{
    static const char *who = "vppx_raft_norm_apply";
    int rc;
    VPPX_ENTER(ctx);
    if (!x || !stats || !out) {
        vppx_set_error("%s: bad arguments", who);
        return VPPX_E_INVALID_ARG;
    }
    if ((rc = gru_shape_ok(who, B, C, H, W, dtype))) return rc;
    if ((rc = gru_stride_ok(who, "x", x_frame_stride, C, H, W)) || (rc = gru_stride_ok(who, "out", out_frame_stride, C, H, W)) ||
        (res && (rc = gru_stride_ok(who, "res", res_frame_stride, C, H, W))))
        return rc;
    if ((rc = norm_stats_stride_ok(who, "stats", stats_frame_stride, C)) ||
        (res_stats && (rc = norm_stats_stride_ok(who, "res_stats", res_stats_frame_stride, C))))
        return rc;
    if (!weight != !bias || !res_weight != !res_bias) {
        vppx_set_error("%s: a weight goes with its bias (weight %s, bias %s, res_weight %s, res_bias %s)", who, weight ? "given" : "NULL",
                       bias ? "given" : "NULL", res_weight ? "given" : "NULL", res_bias ? "given" : "NULL");
        return VPPX_E_INVALID_ARG;
    }
    if ((res_stats || res_weight) && !res) {
        vppx_set_error("%s: res_stats or res_weight without res", who);
        return VPPX_E_INVALID_ARG;
    }
    if (res_weight && !res_stats) {
        vppx_set_error("%s: res_weight without res_stats", who);
        return VPPX_E_INVALID_ARG;
    }
    return norm_apply(ctx, x, x_frame_stride, stats, stats_frame_stride, weight, bias, relu_inner, res, res_frame_stride, res_stats,
                      res_stats_frame_stride, res_weight, res_bias, out, out_frame_stride, B, C, H, W, dtype);
}

extern "C" int vppx_norm_stats_pieces(int64_t planes, int64_t cells_per_plane) { return norm_stats_pieces(planes, cells_per_plane); }

// The 3x3 convolution and ConvGRU's gates (conv_kernels.hip).  Flat arguments with the context last, as the encoders' glue;
// every refusal comes before anything is launched.
// What is built, by output channels: multiples of 16 (the conv3x3 calls and the gates), or any count from 1 on (vppx_raft_conv_*).
enum ConvRule { CONV_OUT_16, CONV_OUT_ANY };

// who NULL: the answer without a text (the *_packed_bytes calls)
static int conv_channels_ok(const char *who, ConvRule rule, int C0, int C1, int Cout)
{
    if (C0 <= 0 || C1 < 0 || Cout <= 0) {
        if (who) vppx_set_error("%s: %d + %d input and %d output channels: C0 and Cout must be positive, C1 not negative", who, C0, C1, Cout);
        return VPPX_E_INVALID_ARG;
    }
    if (C0 % 16 || C1 % 16 || (rule == CONV_OUT_16 && Cout % 16) || (int64_t)C0 + C1 > VPPX_CONV_MAX_CIN || Cout > VPPX_CONV_MAX_COUT) {
        if (who)
            vppx_set_error("%s: %d + %d input and %d output channels: multiples of 16 up to %d in and %s%d out are built", who, C0, C1, Cout,
                           VPPX_CONV_MAX_CIN, rule == CONV_OUT_ANY ? "1 to " : "", VPPX_CONV_MAX_COUT);
        return VPPX_E_UNSUPPORTED;
    }
    return 0;
}

static int conv_ksize_ok(const char *who, int ksize)
{
    if (ksize == 1 || ksize == 3) return 0;
    if (who) vppx_set_error("%s: a kernel size of %d: 1 and 3 are built", who, ksize);
    return VPPX_E_UNSUPPORTED;
}

// is a convolution of (Cout, Cin, ksize, dtype) built under the rule?
static bool conv_built(ConvRule rule, int Cout, int Cin, int ksize, int dtype)
{
    return !conv_channels_ok(NULL, rule, Cin, 0, Cout) && !conv_ksize_ok(NULL, ksize) && (dtype == VPPX_DT_F32 || dtype == VPPX_DT_BF16);
}

static int conv_packed_aligned(const char *who, const void *packed)
{
    if ((uintptr_t)packed % 16) {
        vppx_set_error("%s: the packed buffer is not 16-byte aligned", who);
        return VPPX_E_INVALID_ARG;
    }
    return 0;
}

static int conv_pack_call(const char *who, ConvRule rule, const float *weight, const float *bias, int Cout, int Cin, int ksize, int dtype,
                          void *packed, vppx_ctx *ctx)
{
    int rc;
    VPPX_ENTER(ctx);
    if (!weight || !packed) {
        vppx_set_error("%s: bad arguments", who);
        return VPPX_E_INVALID_ARG;
    }
    if (!handoff_dtype_ok(who, dtype)) return VPPX_E_INVALID_ARG;
    if ((rc = conv_channels_ok(who, rule, Cin, 0, Cout)) || (rc = conv_ksize_ok(who, ksize)) || (rc = conv_packed_aligned(who, packed))) return rc;
    return conv_pack(ctx, weight, bias, Cout, Cin, ksize, dtype, packed);
}

extern "C" size_t vppx_raft_conv3x3_packed_bytes(int Cout, int Cin, int dtype)
{
    return conv_built(CONV_OUT_16, Cout, Cin, 3, dtype) ? conv_packed_bytes(Cout, Cin, 3, dtype) : 0;
}

extern "C" int vppx_raft_conv3x3_pack_dev(const float *weight, const float *bias, int Cout, int Cin, int dtype, void *packed, vppx_ctx *ctx)
{
    return conv_pack_call("vppx_raft_conv3x3_pack", CONV_OUT_16, weight, bias, Cout, Cin, 3, dtype, packed, ctx);
}

// Any Cout, ksize 3 or 1 and a scale: the motion encoder's tail, the flow head and the mask head (update.py:34-42, :83-87, :113-116).
extern "C" size_t vppx_raft_conv_packed_bytes(int Cout, int Cin, int ksize, int dtype)
{
    return conv_built(CONV_OUT_ANY, Cout, Cin, ksize, dtype) ? conv_packed_bytes(Cout, Cin, ksize, dtype) : 0;
}

extern "C" int vppx_raft_conv_pack_dev(const float *weight, const float *bias, int Cout, int Cin, int ksize, int dtype, void *packed,
                                       vppx_ctx *ctx)
{
    return conv_pack_call("vppx_raft_conv_pack", CONV_OUT_ANY, weight, bias, Cout, Cin, ksize, dtype, packed, ctx);
}

// The stride-1 3x3x3 convolution (vppx_conv3d_*): Cin volume channels are 3 Cin pseudo-channels of the 3x3 kernel.
static int conv3d_channels_ok(const char *who, int Cin, int Cout)
{
    if (Cin <= 0 || Cout <= 0) {
        if (who) vppx_set_error("%s: %d input and %d output channels: Cin and Cout must be positive", who, Cin, Cout);
        return VPPX_E_INVALID_ARG;
    }
    if (Cin % 16 || 3 * (int64_t)Cin > VPPX_CONV_MAX_CIN || Cout > VPPX_CONV_MAX_COUT) {
        if (who)
            vppx_set_error("%s: %d input and %d output channels: multiples of 16 up to %d in (3 x Cin up to %d) and 1 to %d out are built", who,
                           Cin, Cout, VPPX_CONV_MAX_CIN / 3 / 16 * 16, VPPX_CONV_MAX_CIN, VPPX_CONV_MAX_COUT);
        return VPPX_E_UNSUPPORTED;
    }
    return 0;
}

extern "C" size_t vppx_conv3d_packed_bytes(int Cout, int Cin, int dtype)
{
    return !conv3d_channels_ok(NULL, Cin, Cout) && (dtype == VPPX_DT_F32 || dtype == VPPX_DT_BF16) ? conv_packed_bytes(Cout, 3 * Cin, 3, dtype) : 0;
}

extern "C" int vppx_conv3d_pack_dev(const float *weight, const float *bias, int Cout, int Cin, int dtype, void *packed, vppx_ctx *ctx)
{
    static const char *who = "vppx_conv3d_pack";
    int rc;
    VPPX_ENTER(ctx);
    if (!weight || !packed) {
        vppx_set_error("%s: bad arguments", who);
        return VPPX_E_INVALID_ARG;
    }
    if (!handoff_dtype_ok(who, dtype)) return VPPX_E_INVALID_ARG;
    if ((rc = conv3d_channels_ok(who, Cin, Cout)) || (rc = conv_packed_aligned(who, packed))) return rc;
    return conv_pack(ctx, weight, bias, Cout, Cin, 3, dtype, packed, true);
}

// a volume's frame stride holds the frame; C * D * H * W is within int64 (C <= 512, D * H * W < 2^31)
static int vol_stride_ok(const char *who, const char *what, int64_t stride, int C, int D, int H, int W)
{
    if (stride < (int64_t)C * D * H * W) {
        vppx_set_error("%s: %s_frame_stride %lld is less than %d volumes of %dx%dx%d", who, what, (long long)stride, C, D, H, W);
        return VPPX_E_INVALID_ARG;
    }
    return 0;
}

// Everything the launch entry points share, in the order they have always refused in.  The tensors of the epilogue are those the
// call names: each is there and its frame stride holds a frame of the output (the gates': C channels, the plain call's: Cout).
// A volume (c.vol) is refused in the same places: its depth with B, H and W, its size behind theirs, its channels by its own rule.
static int conv_call_ok(const char *who, const ConvCall &c, ConvRule rule)
{
    int rc;
    bool missing = c.epi != CV_PLAIN && c.C <= 0;
    for (const ConvTensor &t : c.in) missing = missing || (t.name && !t.p);
    for (const ConvTensor &t : c.out) missing = missing || (t.name && !t.p);
    if (missing) {
        vppx_set_error("%s: bad arguments", who);
        return VPPX_E_INVALID_ARG;
    }
    if (!std::isfinite(c.scale)) {
        vppx_set_error("%s: the scale is not finite", who);
        return VPPX_E_INVALID_ARG;
    }
    if (c.stride != 1 && c.stride != 2) {
        vppx_set_error("%s: a stride of %d: 1 and 2 are built", who, c.stride);
        return VPPX_E_UNSUPPORTED;
    }
    if ((c.dilation != 1 && c.dilation != 2) || (c.dilation == 2 && c.stride == 2)) {
        vppx_set_error("%s: a dilation of %d at stride %d: dilation 1, and dilation 2 at stride 1, are built", who, c.dilation, c.stride);
        return VPPX_E_UNSUPPORTED;
    }
    if (c.epi == CV_ZR && (c.C % 16 || c.C > VPPX_CONV_MAX_COUT / 2)) {
        vppx_set_error("%s: a hidden size of %d makes 2 x %d output channels: multiples of 16 up to %d in all are built", who, c.C, c.C,
                       VPPX_CONV_MAX_COUT);
        return VPPX_E_UNSUPPORTED;
    }
    if (!c.x0 || !c.packed || (c.C1 > 0 && !c.x1)) {
        vppx_set_error("%s: bad arguments", who);
        return VPPX_E_INVALID_ARG;
    }
    if (c.vol && c.D <= 0) {
        vppx_set_error("%s: bad arguments (B, D, H and W must be positive)", who);
        return VPPX_E_INVALID_ARG;
    }
    if ((rc = gru_shape_ok(who, c.B, 1, c.H, c.W, c.dtype))) return rc;
    if (c.vol && (int64_t)c.D * c.H * c.W > 0x7FFFFFFF) { // H * W <= 2^31 - 1 by now: the product is within int64
        vppx_set_error("%s: a %dx%dx%d volume is more than the call takes", who, c.D, c.H, c.W);
        return VPPX_E_UNSUPPORTED;
    }
    if ((rc = c.vol ? conv3d_channels_ok(who, c.C0, c.Cout) : conv_channels_ok(who, rule, c.C0, c.C1, c.Cout)) ||
        (rc = conv_packed_aligned(who, c.packed)))
        return rc;
    // a frame stride against its tensor of C channels, each an h x w map or, for a volume, D of them
    auto stride_ok = [&](const char *what, int64_t stride, int C, int h, int w) {
        return c.vol ? vol_stride_ok(who, what, stride, C, c.D, h, w) : gru_stride_ok(who, what, stride, C, h, w);
    };
    if ((rc = stride_ok(c.vol ? "x" : "x0", c.s0, c.C0, c.H, c.W)) || (c.C1 > 0 && (rc = stride_ok("x1", c.s1, c.C1, c.H, c.W)))) return rc;
    const int64_t cells = (int64_t)c.B * ((int64_t)(c.vol ? c.D : 1) * c.H * c.W); // B and D * H * W <= 2^31 - 1 each: within int64
    if (cells > 0x7FFFFFFF) {
        if (c.vol) vppx_set_error("%s: B*D*H*W = %lld cells are more than one launch takes", who, (long long)cells);
        else vppx_set_error("%s: B*H*W = %lld pixels are more than one launch takes", who, (long long)c.B * c.H * c.W);
        return VPPX_E_UNSUPPORTED;
    }
    const int Ce = c.epi == CV_PLAIN ? c.Cout : c.C, Ho = (c.H - 1) / c.stride + 1, Wo = (c.W - 1) / c.stride + 1;
    for (const ConvTensor &t : c.in)
        if (t.name && (rc = stride_ok(t.name, t.stride, Ce, Ho, Wo))) return rc;
    for (const ConvTensor &t : c.out)
        if (t.name && (rc = stride_ok(t.name, t.stride, Ce, Ho, Wo))) return rc;
    return conv_ksize_ok(who, c.ksize);
}

// the plain call at stride 1 or 2: H, W are the input's, out is [B,Cout,(H - 1) / stride + 1,(W - 1) / stride + 1]; res, where there
// is one, is of out's shape
static int conv_plain_call(const char *who, ConvRule rule, const void *x0, int64_t x0_frame_stride, int C0, const void *x1,
                           int64_t x1_frame_stride, int C1, const void *packed, int Cout, int ksize, int stride, int B, int H, int W, int relu,
                           float scale, void *out, int64_t out_frame_stride, int dtype, vppx_ctx *ctx, int dilation = 1,
                           const void *res = NULL, int64_t res_frame_stride = 0)
{
    int rc;
    VPPX_ENTER(ctx);
    ConvCall c;
    c.ksize = ksize, c.stride = stride, c.dilation = dilation, c.dtype = dtype, c.B = B, c.H = H, c.W = W;
    c.x0 = x0, c.s0 = x0_frame_stride, c.C0 = C0, c.x1 = x1, c.s1 = x1_frame_stride, c.C1 = C1;
    c.packed = packed, c.Cout = Cout, c.relu = relu != 0, c.scale = scale;
    if (res) c.in[0] = {"res", res, res_frame_stride};
    c.out[0] = {"out", out, out_frame_stride};
    if ((rc = conv_call_ok(who, c, rule))) return rc;
    return conv_run(ctx, who, c);
}

extern "C" int vppx_raft_conv3x3_dt_dev(const void *x0, int64_t x0_frame_stride, int C0, const void *x1, int64_t x1_frame_stride, int C1,
                                        const void *packed, int Cout, int B, int H, int W, int relu, void *out, int64_t out_frame_stride,
                                        int dtype, vppx_ctx *ctx)
{
    return conv_plain_call("vppx_raft_conv3x3", CONV_OUT_16, x0, x0_frame_stride, C0, x1, x1_frame_stride, C1, packed, Cout, 3, 1, B, H, W, relu,
                           1.0f, out, out_frame_stride, dtype, ctx);
}

extern "C" int vppx_raft_conv_dt_dev(const void *x0, int64_t x0_frame_stride, int C0, const void *x1, int64_t x1_frame_stride, int C1,
                                     const void *packed, int Cout, int ksize, int B, int H, int W, int relu, float scale, void *out,
                                     int64_t out_frame_stride, int dtype, vppx_ctx *ctx)
{
    return conv_plain_call("vppx_raft_conv", CONV_OUT_ANY, x0, x0_frame_stride, C0, x1, x1_frame_stride, C1, packed, Cout, ksize, 1, B, H, W, relu,
                           scale, out, out_frame_stride, dtype, ctx);
}

// nn.Conv2d(Cin, Cout, ksize, stride=stride, padding=ksize // 2): the encoders' layerN[0].conv1 and downsample[0] (extractor.py:10-11,45)
extern "C" int vppx_raft_conv_strided_dt_dev(const void *x0, int64_t x0_frame_stride, int C0, const void *x1, int64_t x1_frame_stride,
                                             int C1, const void *packed, int Cout, int ksize, int stride, int B, int H, int W, int relu,
                                             float scale, void *out, int64_t out_frame_stride, int dtype, vppx_ctx *ctx)
{
    return conv_plain_call("vppx_raft_conv_strided", CONV_OUT_ANY, x0, x0_frame_stride, C0, x1, x1_frame_stride, C1, packed, Cout, ksize, stride,
                           B, H, W, relu, scale, out, out_frame_stride, dtype, ctx);
}

// nn.Conv2d(Cin, Cout, ksize, stride=stride, padding=dilation * (ksize / 2), dilation=dilation) with a residual in front of the
// ReLU: PSMNet's feature_extraction (models/psmnet/submodule.py:29-42 convbn, :60-84 BasicBlock) with its BatchNorm folded
extern "C" int vppx_conv2d_dt_dev(const void *x0, int64_t x0_frame_stride, int C0, const void *x1, int64_t x1_frame_stride, int C1,
                                  const void *packed, int Cout, int ksize, int stride, int dilation, int B, int H, int W, const void *res,
                                  int64_t res_frame_stride, int relu, float scale, void *out, int64_t out_frame_stride, int dtype,
                                  vppx_ctx *ctx)
{
    return conv_plain_call("vppx_conv2d", CONV_OUT_ANY, x0, x0_frame_stride, C0, x1, x1_frame_stride, C1, packed, Cout, ksize, stride, B, H, W,
                           relu, scale, out, out_frame_stride, dtype, ctx, dilation, res, res_frame_stride);
}

// nn.Conv3d(Cin, Cout, 3, stride=1, padding=1) with a residual in front of the ReLU: PSMNet's dres0, dres1, the hourglasses' conv2 and
// conv4 and the classif heads (models/psmnet/psmnet.py:24-36, 93-128) with their BatchNorm3d folded.  x [B,Cin,D,H,W]; res, out [B,Cout,D,H,W].
extern "C" int vppx_conv3d_dt_dev(const void *x, int64_t x_frame_stride, int Cin, const void *packed, int Cout, int B, int D, int H, int W,
                                  const void *res, int64_t res_frame_stride, int relu, float scale, void *out, int64_t out_frame_stride,
                                  int dtype, vppx_ctx *ctx)
{
    static const char *who = "vppx_conv3d";
    int rc;
    VPPX_ENTER(ctx);
    ConvCall c;
    c.vol = true, c.D = D, c.dtype = dtype, c.B = B, c.H = H, c.W = W;
    c.x0 = x, c.s0 = x_frame_stride, c.C0 = Cin;
    c.packed = packed, c.Cout = Cout, c.relu = relu != 0, c.scale = scale;
    if (res) c.in[0] = {"res", res, res_frame_stride};
    c.out[0] = {"out", out, out_frame_stride};
    if ((rc = conv_call_ok(who, c, CONV_OUT_ANY))) return rc;
    return conv_run(ctx, who, c);
}

// PSMNet's pyramid pooling (spp_kernels.hip; submodule.py:149-171 the four AvgPool2d).  ks and outs are host arrays.
extern "C" int vppx_psm_spp_pool_dt_dev(const void *x, int64_t x_frame_stride, int B, int C, int H, int W, int n_levels, const int *ks,
                                        void *const *outs, int dtype, vppx_ctx *ctx)
{
    static const char *who = "vppx_psm_spp_pool";
    int rc;
    VPPX_ENTER(ctx);
    if (!x || !ks || !outs) {
        vppx_set_error("%s: bad arguments", who);
        return VPPX_E_INVALID_ARG;
    }
    if (n_levels < 1 || n_levels > VPPX_SPP_MAX_LEVELS) {
        vppx_set_error("%s: %d levels, 1 .. %d are taken", who, n_levels, VPPX_SPP_MAX_LEVELS);
        return VPPX_E_INVALID_ARG;
    }
    if ((rc = gru_shape_ok(who, B, C, H, W, dtype)) || (rc = gru_stride_ok(who, "x", x_frame_stride, C, H, W))) return rc;
    for (int i = 0; i < n_levels; i++) {
        if (!outs[i]) {
            vppx_set_error("%s: level %d: bad arguments", who, i);
            return VPPX_E_INVALID_ARG;
        }
        if (ks[i] < 1 || (ks[i] <= VPPX_SPP_MAX_K && (H / ks[i] == 0 || W / ks[i] == 0))) {
            vppx_set_error("%s: level %d: a window of %d over a %dx%d map leaves no cell", who, i, ks[i], H, W);
            return VPPX_E_INVALID_ARG;
        }
    }
    for (int i = 0; i < n_levels; i++)
        if (ks[i] > VPPX_SPP_MAX_K) {
            vppx_set_error("%s: level %d: a window of %d, up to %d are built", who, i, ks[i], VPPX_SPP_MAX_K);
            return VPPX_E_UNSUPPORTED;
        }
    if ((int64_t)B * C > 0x7FFFFFFF) {
        vppx_set_error("%s: %d frames of %d planes are more workgroups than one launch takes", who, B, C);
        return VPPX_E_UNSUPPORTED;
    }
    return spp_pool(ctx, x, x_frame_stride, B, C, H, W, n_levels, ks, outs, dtype);
}

extern "C" int vppx_raft_gru_zr_dt_dev(const void *x0, int64_t x0_frame_stride, int C0, const void *x1, int64_t x1_frame_stride, int C1,
                                       const void *packed_zr, const void *cz, int64_t cz_frame_stride, const void *cr,
                                       int64_t cr_frame_stride, const void *h, int64_t h_frame_stride, void *z, int64_t z_frame_stride,
                                       void *rh, int64_t rh_frame_stride, int B, int C, int H, int W, int dtype, vppx_ctx *ctx)
{
    static const char *who = "vppx_raft_gru_zr";
    int rc;
    VPPX_ENTER(ctx);
    ConvCall c;
    c.epi = CV_ZR, c.dtype = dtype, c.B = B, c.C = C, c.H = H, c.W = W;
    c.x0 = x0, c.s0 = x0_frame_stride, c.C0 = C0, c.x1 = x1, c.s1 = x1_frame_stride, c.C1 = C1;
    c.packed = packed_zr, c.Cout = C > 0 && C <= VPPX_CONV_MAX_COUT / 2 ? 2 * C : 0; // convz and convr; any other C is refused as such
    c.in[0] = {"cz", cz, cz_frame_stride}, c.in[1] = {"cr", cr, cr_frame_stride}, c.in[2] = {"h", h, h_frame_stride};
    c.out[0] = {"z", z, z_frame_stride}, c.out[1] = {"rh", rh, rh_frame_stride};
    if ((rc = conv_call_ok(who, c, CONV_OUT_16))) return rc;
    return conv_run(ctx, who, c);
}

extern "C" int vppx_raft_gru_q_dt_dev(const void *x0, int64_t x0_frame_stride, int C0, const void *x1, int64_t x1_frame_stride, int C1,
                                      const void *packed_q, const void *cq, int64_t cq_frame_stride, const void *z, int64_t z_frame_stride,
                                      const void *h, int64_t h_frame_stride, void *out, int64_t out_frame_stride, int B, int C, int H, int W,
                                      int dtype, vppx_ctx *ctx)
{
    static const char *who = "vppx_raft_gru_q";
    int rc;
    VPPX_ENTER(ctx);
    ConvCall c;
    c.epi = CV_Q, c.dtype = dtype, c.B = B, c.C = C, c.H = H, c.W = W;
    c.x0 = x0, c.s0 = x0_frame_stride, c.C0 = C0, c.x1 = x1, c.s1 = x1_frame_stride, c.C1 = C1;
    c.packed = packed_q, c.Cout = C;
    c.in[0] = {"cq", cq, cq_frame_stride}, c.in[1] = {"z", z, z_frame_stride}, c.in[2] = {"h", h, h_frame_stride};
    c.out[0] = {"out", out, out_frame_stride};
    if ((rc = conv_call_ok(who, c, CONV_OUT_16))) return rc;
    return conv_run(ctx, who, c);
}

extern "C" int vppx_kitti_disp_decode_dev(vppx_ctx *ctx, const uint16_t *png_u16, int64_t n, float *disp, uint8_t *valid)
{
    int rc;
    VPPX_ENTER(ctx);
    if (!png_u16 || !disp || n < 0) { vppx_set_error("vppx_kitti_disp_decode: bad arguments"); return VPPX_E_INVALID_ARG; }
    if (n == 0) return 0;
    return handoff_kitti_decode(ctx, png_u16, (size_t)n, disp, valid);
}

extern "C" int vppx_pfm_decode_dev(vppx_ctx *ctx, const uint8_t *raw, int H, int W, int channels, int little_endian,
                                   float *out)
{
    int rc;
    VPPX_ENTER(ctx);
    if (!raw || !out || H <= 0 || W <= 0 || (channels != 1 && channels != 3) || ((uintptr_t)raw & 3)) {
        vppx_set_error("vppx_pfm_decode: bad arguments (channels must be 1 or 3, payload 4-byte aligned)");
        return VPPX_E_INVALID_ARG;
    }
    return handoff_pfm_decode(ctx, raw, H, W, channels, little_endian != 0, out);
}

extern "C" int vppx_png_decode_dev(vppx_ctx *ctx, int n_files, const uint8_t *blob, const int64_t *offsets, int H, int W, int C,
                                   float scale, float *disp, uint8_t *valid, uint8_t *out_u8, int32_t *status)
{
    int rc;
    VPPX_ENTER(ctx);
    if (n_files <= 0 || !blob || !offsets || H <= 0 || W <= 0 || (C != 1 && C != 3) || (!disp && !out_u8) || (disp && C != 1)) {
        vppx_set_error("vppx_png_decode: bad arguments (C must be 1 or 3; the disparity output needs C = 1)");
        return VPPX_E_INVALID_ARG;
    }
    for (int i = 0; i < n_files; i++)
        if (offsets[i + 1] < offsets[i]) { vppx_set_error("vppx_png_decode: offsets must be non-decreasing"); return VPPX_E_INVALID_ARG; }
    if (1 + (size_t)W * C * 2 > 16384) { vppx_set_error("vppx_png_decode: scanlines longer than 16 KB are not supported"); return VPPX_E_UNSUPPORTED; }
    // scratch for the concatenated IDAT payloads: file i's zlib stream starts 16-byte aligned at zoffs[i] (<= its file size)
    ctx->png_offs_host.assign(offsets, offsets + n_files + 1);
    size_t ztot = 0;
    for (int i = 0; i < n_files; i++) {
        ctx->png_offs_host.push_back((long long)ztot);
        ztot += (((size_t)(offsets[i + 1] - offsets[i])) + 15 + 16) & ~(size_t)15;
    }
    u8 *zcat;
    long long *offs_d;
    int *st_d;
    if ((rc = ws_get(ctx, WS_PNG_RAW, ztot + 16, &zcat))) return rc;
    if ((rc = ws_get(ctx, WS_PNG_OFFS, (size_t)2 * n_files + 1, &offs_d))) return rc;
    if (!status && (rc = ws_get(ctx, WS_PNG_STATUS, (size_t)n_files, &st_d))) return rc;
    VPPX_HIP(hipMemcpyAsync(offs_d, ctx->png_offs_host.data(), ((size_t)2 * n_files + 1) * sizeof(long long), hipMemcpyHostToDevice, ctx->stream));
    return handoff_png_decode(ctx, n_files, blob, offs_d, H, W, C, zcat, offs_d + n_files + 1, scale, disp, valid, out_u8, status ? status : st_d);
}
