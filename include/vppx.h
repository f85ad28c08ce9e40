/*
 * vppx.h -- C-ABI of libvppx.so: MI355X-native (gfx950) virtual-pattern-projection +
 * rSGM hot path.  Drop-in boundary for the reference's native entry points:
 *
 *   reference native (file:line)                                   replaced by
 *   ------------------------------------------------------------   ---------------------------
 *   vpp_core_opt.init_rand              vpp_core_opt.pyx:33-35      vppx_srand
 *   vpp_core_opt.virtual_projection_scan_rnd       .pyx:53-54       vppx_virtual_projection_scan_rnd
 *   vpp_core_opt.virtual_projection_scan_max_dist  .pyx:133-134     vppx_virtual_projection_scan_max_dist
 *   numba twins + wrapper vpp()         vpp_standalone.py:243,14,396 vppx_vpp_host / vppx_vpp_dev
 *   pyrSGM.census5x5_SSE                call site rsgm.py:25        vppx_census5x5
 *   pyrSGM.costMeasureCensus5x5_xyd_SSE call site rsgm.py:44        vppx_cost_census5x5_xyd
 *   pyrSGM.aggregate_SSE                call site rsgm.py:61        vppx_aggregate
 *   pyrSGM.matchWTA_SSE                 call site rsgm.py:141       vppx_match_wta
 *   pyrSGM.subPixelRefine               call site rsgm.py:142       vppx_subpixel_refine
 *   pyrSGM.median3x3_SSE                call site rsgm.py:145,173   vppx_median3x3
 *   pyrSGM.matchWTARight_SSE            call site rsgm.py:170       vppx_match_wta_right
 *   compute_rsgm()                      rsgm.py:250-294             vppx_rsgm_host / vppx_rsgm_dev
 *   occlusion_heuristic()               filter.py:246-292           vppx_occlusion_heuristic_host/_dev
 *   test.py:158-225 (VPP -> rSGM per frame)                         vppx_vpp_rsgm_dev (fused, batched)
 *   guided_metrics()                    losses.py:13-24             vppx_guided_metrics_host / _dev, vppx_occ_vpp_rsgm_eval_dev
 *   sample_hints()                      losses.py:5-10              vppx_sample_hints_host / _dev, vppx_occ_vpp_rsgm_sampled_dev
 *   color_error_image_kitti()           utils.py:17-36              vppx_error_colors_host / _dev
 *   guided_visualize()                  utils.py:39-79              vppx_guided_visualize_host / _dev
 *   test.py:318, :325-326, :343 (max_val, applyColorMap)            vppx_finite_max_dev, vppx_colorize_host / _dev
 *   CorrBlock1D.corr GEMM + pyramid     raft_stereo/corr.py:116-124,151-155 vppx_raft_corr_fused_dt_dev
 *   CorrBlock1D.__init__ pyramid        raft_stereo/corr.py:116-124 vppx_raft_corr_pyramid_dt_dev
 *   CorrBlock1D.__call__                raft_stereo/corr.py:126-145 vppx_raft_corr_lookup_dt_dev
 *   BasicMotionEncoder convc1 / convf1  raft_stereo/update.py:80,82 vppx_raft_motion_front_dt_dev
 *   ResidualBlock norm / relu / sum     raft_stereo/extractor.py:48-60 vppx_raft_norm_stats_dt_dev, vppx_raft_norm_apply_dt_dev
 *   ConvGRU convz / convr / convq + gates raft_stereo/update.py:19-32 vppx_raft_gru_zr_dt_dev, vppx_raft_gru_q_dt_dev, vppx_raft_conv3x3_dt_dev
 *   BasicMotionEncoder convc2 / convf2 / conv raft_stereo/update.py:81,83,86 vppx_raft_conv_dt_dev
 *   FlowHead conv1 / conv2              raft_stereo/update.py:34-42 vppx_raft_conv_dt_dev
 *   BasicMultiUpdateBlock.mask, .25 *   raft_stereo/update.py:113-116,141 vppx_raft_conv_dt_dev
 *   ResidualBlock conv1 / conv2 / downsample, encoder conv2, output heads -> extractor.py:10-11,45,149,231,240,247 vppx_raft_conv_strided_dt_dev
 *   feature_extraction convbn / BasicBlock  psmnet/submodule.py:29-42,60-84 vppx_conv2d_dt_dev
 *   feature_extraction branches, cat    psmnet/submodule.py:149-171,208-250 vppx_psm_spp_pool_dt_dev, vppx_raft_gru_assemble_strided_dt_dev
 *   dres0 / dres1 / hourglass conv2, conv4 / classif  psmnet/psmnet.py:24-36,93-128 vppx_conv3d_dt_dev
 *
 * Conventions
 *   - plain C, no torch types.  "_host" entry points take host pointers (what a ctypes /
 *     numpy caller has) and are synchronous; "_dev" entry points take device pointers,
 *     enqueue on the context's HIP stream and return without synchronising.
 *   - images are uint8, HWC, C-contiguous, batch outermost: [B,H,W,C]; hint / disparity
 *     maps are float32 [B,H,W]; masks uint8 [B,H,W].  Exactly the reference's layouts
 *     (vpp_core_opt.pyx:53, rsgm.py:42,60) with a leading batch dimension.
 *   - every function returns 0 on success or a negative VPPX_E_* code; the message of
 *     the last error on the calling thread is available from vppx_last_error().  Codes map
 *     one-to-one onto the reference's Python exceptions (rsgm.py:19-20,31-40,157-167).
 *   - there is NO CPU fallback: without a HIP device every compute entry point fails with
 *     VPPX_E_NO_DEVICE.
 */
#ifndef VPPX_H
#define VPPX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VPPX_VERSION 100

enum {
    VPPX_OK = 0,
    VPPX_E_INVALID_ARG = -1,     /* null pointer, bad shape, bad enum                       */
    VPPX_E_DMAX_MOD8 = -2,       /* "Invalid dmax (..): dmax % 8 != 0"      rsgm.py:31-32   */
    VPPX_E_DMAX_GT256 = -3,      /* "Invalid dmax (..): dmax > 256"         rsgm.py:34-35   */
    VPPX_E_UNIQUENESS = -4,      /* "Invalid uniqueness (..) in ]0,1]"      rsgm.py:166-167 */
    VPPX_E_WIDTH_MOD16 = -5,     /* "Invalid width (..): width % 16 != 0"   rsgm.py:19-20   */
    VPPX_E_METHOD = -6,          /* assert method in ["rnd","maxDistance"]  vpp_standalone.py:400 */
    VPPX_E_NO_DEVICE = -7,       /* no HIP device / HIP runtime error at init               */
    VPPX_E_HIP = -8,             /* HIP runtime error (message has the hipError string)     */
    VPPX_E_OOM = -9,             /* workspace allocation failed                             */
    VPPX_E_UNSUPPORTED = -10     /* valid in the reference but outside this build's limits  */
};

enum { VPPX_METHOD_RND = 0, VPPX_METHOD_MAXDIST = 1 };

/* Parameters of the VPP scans.  Field meaning = the same-named argument of
 * vpp_core_opt.pyx:53-54 / :133-134 and vpp_standalone.py:396 (defaults in brackets). */
typedef struct VppxVppParams {
    int32_t method;             /* VPPX_METHOD_*                 ["rnd"]                    */
    int32_t wsize;              /* patch size 2n+1               [3]                        */
    int32_t wsize_agg_x;        /* maxDistance window            [64]                       */
    int32_t wsize_agg_y;        /*                               [3]                        */
    int32_t direction;          /* 1 = left2right scan, 0 = r2l  [1]                        */
    int32_t uniform_color;      /*                               [0]                        */
    int32_t discard_occluded;   /*                               [0]                        */
    int32_t interpolate;        /*                               [1]                        */
    float c;                    /* blending                      [0.4]                      */
    float c_occ;                /*                               [0.0]                      */
    /* numba-twin extras (vpp_standalone.py:93-96,154,315-318,335) */
    int32_t use_distance_patch; /*                               [0]                        */
    int32_t use_bilateral_patch;/* gate on |g - filled_g| < 0.1  [0] (needs filled_g)       */
    double distance_gamma;      /*                               [0.3]                      */
    float dmin, dmax;           /* min / max positive hint of the frame (wrapper :410-411); ignored with per_frame_range */
    /* random stream (libc rand() in the reference, vpp_core_opt.pyx:33-35,93,102):
     * frame f of a batch draws from srand(seed + f) starting rand_offset draws in.        */
    uint32_t seed;              /*                               [1]                        */
    /* use_distance_patch in a batch: 1 = every frame's dmin / dmax are taken from ITS OWN hints on the device (min / max of the
     * positive values), which is what vpp() does per call (vpp_standalone.py:410-411); 0 = dmin / dmax above, one pair for the
     * whole batch.  A frame whose positive hints all have one value -- the reference's _get_patch_size_based_on_distance divides
     * by zero there -- gets the full patch size.                                    [0]     */
    uint32_t per_frame_range;
    uint64_t rand_offset;       /*                               [0]                        */
    /* _bilateral_filling (vpp_standalone.py:372-394, wrapper :419-420): when
     * use_bilateral_patch is set and no filled_g is passed, the library densifies the hints
     * itself from the un-patterned left image (BGR2GRAY of it, as the wrapper does at :415) */
    double bilateral_o_xy;      /*                               [2]                        */
    double bilateral_o_i;       /*                               [1]                        */
    double bilateral_th;        /*                               [0.001]                    */
} VppxVppParams;

/* Parameters of compute_rsgm (rsgm.py:250). */
typedef struct VppxRsgmParams {
    int32_t dmax;        /* [192]  multiple of 8, <= 256 */
    int32_t p1;          /* [11]   */
    int32_t p2min;       /* [17]   */
    float alpha;         /* [0.5]  */
    int32_t gamma;       /* [35]   */
    float uniqueness;    /* [0.95] */
    int32_t subpixel;    /* [1]  (test.py:71 passes False) */
    int32_t reserved0;
} VppxRsgmParams;

/* Parameters of occlusion_heuristic (filter.py:246; defaults in brackets). */
typedef struct VppxOccParams {
    int32_t rx, ry;      /* [9] [7]   */
    double l, g;         /* [2] [0.4375] */
    double th_conf;      /* [1]   */
    double th_filter;    /* [0.1] */
} VppxOccParams;

typedef struct vppx_ctx vppx_ctx; /* opaque: device, stream, workspace arena */

/* ---- library / context ------------------------------------------------------------ */
int vppx_version(void);
const char *vppx_last_error(void);
void vppx_vpp_params_default(VppxVppParams *p);
void vppx_rsgm_params_default(VppxRsgmParams *p);
void vppx_occ_params_default(VppxOccParams *p);

/* Create a context on HIP device `device` (-1 = current device).  One context per
 * process/GPU; not thread-safe (the reference is single-threaded: rsgm.py:44). */
int vppx_create(vppx_ctx **out, int device);
void vppx_destroy(vppx_ctx *ctx);
/* Use an existing hipStream_t (e.g. torch's current side stream); NULL = the context's own (non-blocking) stream.
 * Binding the stream that is already bound costs nothing (no synchronisation). */
int vppx_set_stream(vppx_ctx *ctx, void *hip_stream);
/* Launch on the legacy default ("null") stream itself -- what torch's default stream is (its handle is 0, which
 * vppx_set_stream reads as "own stream").  All work is then ordered with the caller's default-stream work. */
int vppx_set_stream_legacy(vppx_ctx *ctx);

/* Cross-call pipelining for streams of batches through vppx_occ_vpp_rsgm_dev / vppx_vpp_rsgm_dev: with `on`, the front
 * stage of a call (occlusion heuristic, VPP, pad + gray, census) runs on a second stream as soon as the PREVIOUS call's
 * aggregation is done, i.e. next to that call's sum / WTA and post kernels (calls that take the 8-path layout -- fewer than
 * 3 frames -- leave most of the GPU idle during their aggregation: there the next front stage starts as soon as the previous
 * one has delivered its results, next to that aggregation; the gray / census images exist twice for this).  A call of more
 * frames than one batch quantum (vppx_batch_quantum) runs as consecutive parts of one quantum each, pipelined like separate
 * calls; results do not depend on the split.  Safe by construction:
 *   - outputs keep the launch stream's order: the launch stream waits for the front stage, and everything the front stage
 *     produces for the caller (conf_out, l_vpp, r_vpp) is computed into library-owned buffers and copied to the caller's
 *     memory ON THE LAUNCH STREAM -- the front stream never writes caller memory, so buffers allocated per call by a
 *     stream-ordered allocator (torch's) are fine;
 *   - inputs: the front stage waits for an event.  By default the library records it on the launch stream when the call
 *     is made, i.e. the front stage waits for everything queued before the call (correct for any caller; no overlap then).
 *     A caller whose inputs are ready earlier -- resident frames, a loader running on its own stream -- says so with
 *     vppx_inputs_ready_event: the front stage of the NEXT call then waits for that event instead and overlaps the
 *     previous call's tail.
 * Any other entry point called in between uses the same workspace on the launch stream and makes the next front stage
 * wait for the whole launch stream again.  Off by default; ignored during graph capture, stage timing and for sub-stream
 * parts.  (No reference counterpart: test.py handles one pair at a time.) */
int vppx_set_pipeline(vppx_ctx *ctx, int on);
/* One-shot: `hip_event` (a hipEvent_t the caller recorded on the stream that produced them) completes when ALL inputs of
 * the next vppx_occ_vpp_rsgm_dev / vppx_vpp_rsgm_dev / vppx_occ_vpp_rsgm_guided_dev call (left, right, g, g_occ,
 * validhints) are ready.  NULL withdraws it.  Without
 * pipelining the call runs on the launch stream and the event is simply waited for there. */
int vppx_inputs_ready_event(vppx_ctx *ctx, void *hip_event);
/* Wait for everything queued on the context's stream.  Returns VPPX_E_HIP (message in vppx_last_error) when a fused
 * aggregation launch that has finished by then lost its lock step (see vppx_status). */
int vppx_synchronize(vppx_ctx *ctx);
/* Health of the asynchronous hot path, non-blocking.  The fused aggregation kernel (vppx_uses_vert() == 3) hands
 * diagonal path state between neighbouring waves in lock step; every wait is bounded (VPPX_V3_TIMEOUT_MS, default 250 ms
 * of wall clock per wait), and a wave that gives up marks its launch: the disparities of that call are void -- and are
 * overwritten with NaN by a kernel queued behind the call, so that nothing later on the stream can take them for a
 * disparity map.  The mark is reported -- VPPX_E_HIP, once -- by whichever of these looks first: vppx_status,
 * vppx_synchronize, the next vppx_occlusion_heuristic_dev / vppx_vpp_rsgm_dev / vppx_rsgm_dev call, or vppx_rsgm_host, which
 * repeats its OWN aggregation on the line-parallel kernel and returns correct results (a mark left by an earlier
 * asynchronous call is reported, not consumed).  The context then aggregates with the line-parallel kernel for its next 64
 * aggregation launches (doubling with every further loss, at most 4096) and tries the fused layout again.  After the caller
 * has synchronised the stream (by any means) a 0 from vppx_status covers every call made so far.  (No reference
 * counterpart: aggregate_SSE, rsgm.py:61, is synchronous.) */
int vppx_status(vppx_ctx *ctx);
/* Number of fused launches that reported a lost lock step on this context so far. */
long vppx_lockstep_failures(vppx_ctx *ctx);
/* Bytes of device workspace currently held by the context. */
size_t vppx_workspace_bytes(const vppx_ctx *ctx);
/* Name of the HIP device the context runs on (e.g. "AMD Instinct MI355X"). */
const char *vppx_device_name(const vppx_ctx *ctx);

/* ---- libc-style random stream of the single-frame scans ----------------------------- */
/* init_rand(seed) (vpp_core_opt.pyx:33): restart the context's stream; subsequent
 * vppx_virtual_projection_scan_* calls continue it exactly like libc's global state. */
int vppx_srand(vppx_ctx *ctx, uint32_t seed);
/* Position of that stream: the seed of the last vppx_srand and the number of draws consumed since.  A batched
 * caller (vpp_standalone.vpp through vppx_vpp_host) continues the stream by passing these as
 * VppxVppParams.seed / .rand_offset and reporting what it consumed with vppx_rand_advance. */
int vppx_rand_state(vppx_ctx *ctx, uint32_t *seed, uint64_t *consumed);
int vppx_rand_advance(vppx_ctx *ctx, uint64_t draws);
/* Device-generated glibc rand() stream: out[i] = i-th rand() after srand(seed), for
 * i in [offset, offset+n).  Host pointer. */
int vppx_rand_stream(vppx_ctx *ctx, uint32_t seed, uint64_t offset, int64_t n, int32_t *out);

/* ---- VPP: reference native signatures (host pointers, in place, single frame) -------- */
/* vpp_core_opt.pyx:53-54.  Returns the number of hints (>= 0) or a negative error. */
int vppx_virtual_projection_scan_rnd(vppx_ctx *ctx, uint8_t *l, uint8_t *r, const float *g, int width, int height,
                                     int channels, int uniform_color, int wsize, int direction, float c,
                                     float c_occ, const uint8_t *g_occ, int discard_occluded, int interpolate);
/* vpp_core_opt.pyx:133-134. */
int vppx_virtual_projection_scan_max_dist(vppx_ctx *ctx, uint8_t *l, uint8_t *r, const float *g, int width,
                                          int height, int channels, int uniform_color, int wsize, int wsize_agg_x,
                                          int wsize_agg_y, int direction, float c, float c_occ,
                                          const uint8_t *g_occ, int discard_occluded, int interpolate);

/* ---- VPP: batched form ---------------------------------------------------------------- */
/* l, r are updated in place; g_occ / filled_g may be NULL; n_hints (host, [B]) may be NULL
 * for the _dev form (then nothing is copied back). */
int vppx_vpp_host(vppx_ctx *ctx, const VppxVppParams *p, int B, int H, int W, int C, uint8_t *l, uint8_t *r,
                  const float *g, const uint8_t *g_occ, const float *filled_g, int64_t *n_hints);
int vppx_vpp_dev(vppx_ctx *ctx, const VppxVppParams *p, int B, int H, int W, int C, uint8_t *l, uint8_t *r,
                 const float *g, const uint8_t *g_occ, const float *filled_g, int64_t *n_hints_dev);

/* Number of rand() draws each frame of the last vppx_vpp_host / vppx_vpp_dev call consumed (host array [B]);
 * synchronises the stream.  Lets a caller continue the libc-like stream across calls.  Not defined after the fused
 * entry points (vppx_vpp_rsgm_dev / vppx_occ_vpp_rsgm_dev): those may run a batch in parts (vppx_last_call_parts) and keep
 * the counts of the last part only; their frames draw from srand(seed + frame) and never continue a stream. */
int vppx_vpp_last_draws(vppx_ctx *ctx, int B, uint64_t *draws);

/* ---- rSGM: pyrSGM-compatible stage entry points (host pointers, single frame) ---------- */
int vppx_census5x5(vppx_ctx *ctx, const uint8_t *img, uint32_t *out, int w, int h);
int vppx_cost_census5x5_xyd(vppx_ctx *ctx, const uint32_t *cl, const uint32_t *cr, uint16_t *dsi, int w, int h,
                            int dmax, int n_threads_ignored);
int vppx_aggregate(vppx_ctx *ctx, const uint8_t *img, const uint16_t *dsi, uint16_t *dsi_agg, int w, int h,
                   int dmax, int p1, int p2min, float alpha, int gamma);
/* The same with the image as the reference's glue passes it (rsgm.py:258,270: the padded H x W x 3 colour array):
 * channels = 3 converts to gray on the device first, so that this route and vppx_rsgm_* use the same P2 image. */
int vppx_aggregate_img(vppx_ctx *ctx, const uint8_t *img, int channels, const uint16_t *dsi, uint16_t *dsi_agg, int w,
                       int h, int dmax, int p1, int p2min, float alpha, int gamma);
int vppx_match_wta(vppx_ctx *ctx, const uint16_t *dsi, float *disp, int w, int h, int dmax, float uniqueness);
int vppx_match_wta_right(vppx_ctx *ctx, const uint16_t *dsi, float *disp, int w, int h, int dmax,
                         float uniqueness);
int vppx_subpixel_refine(vppx_ctx *ctx, const uint16_t *dsi, float *disp, int w, int h, int dmax, int method);
int vppx_median3x3(vppx_ctx *ctx, const float *src, float *dst, int w, int h);

/* ---- rSGM: whole compute_rsgm (rsgm.py:250-294), batched -------------------------------- */
/* Stage API: the post-processing of compute_rsgm (models/rsgm/rsgm.py:275-292) on device buffers: crop of the padded
 * left / right disparity maps [B][Hp][Wp] (Hp, Wp = H, W rounded up to multiples of 16, the frame centred as rsgm.py:254-260
 * pads it), left/right check (:230-248, threshold 1), astype(uint8), cv2.filterSpeckles(0, 200, 10), astype(float32),
 * sub-pixel values restored where the integer map kept a pixel (subpixel != 0), _interpolate_background (:185-227).
 * disp_out: [B][H][W] float32. */
int vppx_rsgm_post_dev(vppx_ctx *ctx, int B, int H, int W, const float *disp_l_pad, const float *disp_r_pad, int subpixel,
                       float *disp_out);

/* Stage API: three more stages of compute_rsgm on device buffers, each through the very launch the whole call makes (the
 * pyrSGM-style entries above run kernels of their own).  Like vppx_rsgm_post_dev they queue on the context's stream, do not
 * synchronise, use no workspace and leave vppx_last_routes / vppx_last_front_routes as they were.  Hp, Wp = H, W rounded up
 * to multiples of 16, the frame centred as rsgm.py:254-260 pads it (pad_l = (Wp - W) / 2, pad_t = (Hp - H) / 2).
 *
 * vppx_rsgm_front_dev: reflect pad (rsgm.py:258-260), RGB -> gray for C = 3 (the plane itself for C = 1) and the 5x5
 * census (rsgm.py:25-26) of three images in one launch.  left / left_vpp / right_vpp: uint8 [B,H,W,C], H, W >= 5.
 * gray_left: uint8 [B,Hp,Wp], the padded gray image of `left` (the P2 image, rsgm.py:270).  census_l / census_r: uint32
 * [B,Hp,Wp], the census codes of the padded gray images of left_vpp / right_vpp (zero on the 2-pixel border). */
int vppx_rsgm_front_dev(vppx_ctx *ctx, int B, int H, int W, int C, const uint8_t *left, const uint8_t *left_vpp,
                        const uint8_t *right_vpp, uint8_t *gray_left, uint32_t *census_l, uint32_t *census_r);
/* vppx_rsgm_guided_rows_dev: the cost rows of --guided (_guided_dsi, rsgm.py:116-127, on the rows of
 * costMeasureCensus5x5_xyd_SSE) at the hint pixels only.  census_l / census_r: uint32 [B,Hp,Wp]; row x of census_r is read
 * at x - d for d <= x only, never in front of a row, so census_r needs no guard words in front of it.  hints / validhints:
 * float32 [B,H,W], un-padded (rsgm.py:266-267 pads them with zeros: a padding pixel owns no row).  gmap: int32 [B,Hp,Wp],
 * receives the row index of every padded pixel with validhints > 0 and -1 elsewhere; the indices are 0 .. n-1 in no
 * particular order.  rows: uint16 [n][dmax]; n is not known beforehand, so reserve B*H*W rows as the whole call does.
 * count: one uint32, receives n.  dmax: a multiple of 8 in 8 .. 256 (VPPX_E_DMAX_MOD8 / VPPX_E_DMAX_GT256 otherwise). */
int vppx_rsgm_guided_rows_dev(vppx_ctx *ctx, int B, int H, int W, int dmax, const uint32_t *census_l, const uint32_t *census_r,
                              const float *hints, const float *validhints, int32_t *gmap, uint16_t *rows, uint32_t *count);
/* vppx_rsgm_mid_dev: median3x3_SSE -> _linear_interpolate(., 15, 3) -> np.clip(., 0, None) of the left and the right
 * disparity map (rsgm.py:145-151, 173-179) in one launch.  All four: float32 [B,Hp,Wp]; the outputs must not alias the
 * inputs.  Hp, Wp: multiples of 16, at least 16 (VPPX_E_INVALID_ARG otherwise). */
int vppx_rsgm_mid_dev(vppx_ctx *ctx, int B, int Hp, int Wp, const float *disp_l, const float *disp_r, float *out_l,
                      float *out_r);

/* left / left_vpp / right_vpp: uint8 [B,H,W,C] (C = 1 or 3); disp_out: float32 [B,H,W].
 * hints / validhints: float32 [B,H,W] or both NULL; non-NULL = --guided (_guided_dsi, rsgm.py:116-127). */
int vppx_rsgm_host(vppx_ctx *ctx, const VppxRsgmParams *p, int B, int H, int W, int C, const uint8_t *left,
                   const uint8_t *left_vpp, const uint8_t *right_vpp, const float *hints, const float *validhints,
                   float *disp_out);
int vppx_rsgm_dev(vppx_ctx *ctx, const VppxRsgmParams *p, int B, int H, int W, int C, const uint8_t *left,
                  const uint8_t *left_vpp, const uint8_t *right_vpp, const float *hints, const float *validhints,
                  float *disp_out);

/* ---- fused hot path: VPP (in place on copies) + rSGM, batched, device pointers ----------- */
/* left/right: original pair uint8 [B,H,W,C] (not modified); l_vpp/r_vpp: outputs, patterned
 * pair (may be NULL -> internal scratch); disp_out float32 [B,H,W]. */
int vppx_vpp_rsgm_dev(vppx_ctx *ctx, const VppxVppParams *vp, const VppxRsgmParams *rp, int B, int H, int W, int C,
                      const uint8_t *left, const uint8_t *right, const float *g, const uint8_t *g_occ,
                      uint8_t *l_vpp, uint8_t *r_vpp, float *disp_out);

/* The same with the occlusion mask computed on the way (test.py:154 --maskocc, then :158-225): g_occ =
 * occlusion_heuristic(g, op)[1] never leaves the library between the two stages.  conf_out (uint8 [B,H,W], may be NULL)
 * receives the mask.  This is the entry point bench.py times. */
int vppx_occ_vpp_rsgm_dev(vppx_ctx *ctx, const VppxOccParams *op, const VppxVppParams *vp, const VppxRsgmParams *rp, int B,
                          int H, int W, int C, const uint8_t *left, const uint8_t *right, const float *g, uint8_t *conf_out,
                          uint8_t *l_vpp, uint8_t *r_vpp, float *disp_out);
/* The same for HOST arrays, one frame or a batch: test.py:154-225 in one call.  The pair, the hints and a caller's mask go up
 * once, the disparities -- and, where the pointers are not NULL, the mask
 * (op != NULL: computed on the way, test.py:154), and the patterned pair -- come down once; synchronous.  op == NULL: g_occ
 * (may be NULL) is the caller's mask.  draws_out (may be NULL, [B]): rand() draws each frame consumed (0 for maxDistance or
 * when the call ran in parts), for callers that continue a libc-like stream (vppx_rand_advance). */
int vppx_occ_vpp_rsgm_host(vppx_ctx *ctx, const VppxOccParams *op, const VppxVppParams *vp, const VppxRsgmParams *rp, int B, int H,
                           int W, int C, const uint8_t *left, const uint8_t *right, const float *g, const uint8_t *g_occ,
                           uint8_t *conf_out, uint8_t *l_vpp_out, uint8_t *r_vpp_out, float *disp_out, uint64_t *draws_out);
/* --guided with the rSGM matcher (test.py:207-223): as vppx_occ_vpp_rsgm_dev, and the hints g also re-weight the matching
 * costs at every pixel whose validhints (float32 [B,H,W], required) is > 0, whatever its hint (_guided_dsi, rsgm.py:116-127).
 * op != NULL computes the mask on the way; op == NULL: g_occ (may be NULL) is the caller's mask.  With vppx_set_pipeline,
 * validhints is an input like g (vppx_inputs_ready_event).  Never the fused aggregation layout: the 8-path layout on u16
 * volumes; a batch whose eight volumes (16 bytes per cell) would exceed 48 GiB runs in parts (frame f keeps srand(seed + f)). */
int vppx_occ_vpp_rsgm_guided_dev(vppx_ctx *ctx, const VppxOccParams *op, const VppxVppParams *vp, const VppxRsgmParams *rp, int B,
                                 int H, int W, int C, const uint8_t *left, const uint8_t *right, const float *g, const uint8_t *g_occ,
                                 const float *validhints, uint8_t *conf_out, uint8_t *l_vpp, uint8_t *r_vpp, float *disp_out);
/* The same for HOST arrays, as vppx_occ_vpp_rsgm_host. */
int vppx_occ_vpp_rsgm_guided_host(vppx_ctx *ctx, const VppxOccParams *op, const VppxVppParams *vp, const VppxRsgmParams *rp, int B,
                                  int H, int W, int C, const uint8_t *left, const uint8_t *right, const float *g, const uint8_t *g_occ,
                                  const float *validhints, uint8_t *conf_out, uint8_t *l_vpp_out, uint8_t *r_vpp_out, float *disp_out,
                                  uint64_t *draws_out);

/* ---- --iscale / --oscale (test.py:136-148, :247-248): the batched call on frames resized on the device ------------------
 * With s = iscale and (h, w) = (H / s, W / s): the pair is resized as cv2.resize(INTER_LINEAR) does for 8U (DESIGN section 5,
 * rule 1), the hints and validhints are decimated to every s-th row and column (F.interpolate nearest) and the hints divided
 * by s (float32 true division).  Occlusion heuristic, VPP and rSGM then run at (h, w), unchanged.  When iscale != 1 and
 * iscale / oscale != 1 the map is restored to (Ho, Wo) = floor((h, w) * iscale / oscale) (double) by F.interpolate nearest
 * and multiplied by iscale, divided by oscale (two float32 operations); otherwise (Ho, Wo) = (h, w) and the map is returned
 * as computed.  (Ho, Wo) need not be (H, W): H = 375, s = 2 gives 374 rows. */
typedef struct VppxScaleParams {
    int32_t iscale; /* >= 1, default 1: --iscale */
    int32_t oscale; /* >= 1, default 1: --oscale */
} VppxScaleParams;
void vppx_scale_params_default(VppxScaleParams *p);
/* (h, w): the shape the matcher runs at; (Ho, Wo): the shape of the returned map.  VPPX_E_INVALID_ARG for iscale < 1,
 * oscale < 1 or an empty scaled shape. */
int vppx_scaled_shape(int H, int W, const VppxScaleParams *sp, int *h, int *w, int *Ho, int *Wo);
/* Times this context built the resize / restore index tables of a scaled call and uploaded them: once for the first scaled
 * call, once more whenever (H, W, iscale, oscale) differs from the previous scaled call's; a call of the same shape reuses
 * them.  A host counter, for tests and diagnostics: reading it launches and waits for nothing. */
long vppx_scale_table_builds(vppx_ctx *ctx);
/* Which of the two sets of library-owned maps the last resizing call (scale_set) and the last sampling call (sample_set) of this
 * context wrote: 0 or 1, -1 before the first such call.  Without vppx_set_pipeline every call writes set 0; with it consecutive
 * calls alternate, since the next call's front stage may write while this call still reads.  Either pointer may be NULL.  Host
 * stores only, for tests and diagnostics. */
int vppx_last_front_sets(vppx_ctx *ctx, int *scale_set, int *sample_set);
/* As vppx_occ_vpp_rsgm_guided_dev on full-size inputs left / right (uint8 [B,H,W,C]), g and validhints (float32 [B,H,W]):
 * validhints == NULL runs unguided; op != NULL computes the mask on the way, op == NULL takes g_occ (may be NULL) as the
 * caller's mask at (h, w).  conf_out [B,h,w], l_vpp / r_vpp [B,h,w,C] are at the scaled shape (may be NULL), disp_out is
 * float32 [B,Ho,Wo], disp_small (may be NULL) receives the map at [B,h,w] before the restore.  Rejects sp out of range and
 * a scaled shape that fails the frame checks with VPPX_E_INVALID_ARG before anything is launched.  With vppx_set_pipeline
 * the resize runs in the front stage (the scaled buffers alternate between two sets). */
int vppx_occ_vpp_rsgm_scaled_dev(vppx_ctx *ctx, const VppxOccParams *op, const VppxVppParams *vp, const VppxRsgmParams *rp,
                                 const VppxScaleParams *sp, int B, int H, int W, int C, const uint8_t *left, const uint8_t *right,
                                 const float *g, const uint8_t *g_occ, const float *validhints, uint8_t *conf_out, uint8_t *l_vpp,
                                 uint8_t *r_vpp, float *disp_out, float *disp_small);
/* The same for HOST arrays, as vppx_occ_vpp_rsgm_host (draws_out: draws of each frame at the scaled shape). */
int vppx_occ_vpp_rsgm_scaled_host(vppx_ctx *ctx, const VppxOccParams *op, const VppxVppParams *vp, const VppxRsgmParams *rp,
                                  const VppxScaleParams *sp, int B, int H, int W, int C, const uint8_t *left, const uint8_t *right,
                                  const float *g, const uint8_t *g_occ, const float *validhints, uint8_t *conf_out,
                                  uint8_t *l_vpp_out, uint8_t *r_vpp_out, float *disp_out, float *disp_small, uint64_t *draws_out);

/* ---- evaluation metrics (losses.py:13-24 guided_metrics; test.py:150-152, :251-252) ------------------------------------
 * What test.py reports per frame: over the pixels with validgt > 0, with e = |disp - gt| and d2 = (disp - gt)^2 in float32,
 * bad_t = n(e > t) / n_valid for t = 1, 2, 3, 4, avgerr = sum(e) / n_valid, rms = sqrt(sum(d2) / n_valid): exact integer
 * counts, float64 sums of the float32 terms, float64 results (all six NaN when no pixel is valid).  The sums are added in a
 * fixed order that depends on the frame's shape only (no floating-point atomics): a frame's record is the same bytes alone,
 * as frame 17 of 32, or in a flushed part batch of a frame stream.  NaN disparities (vppx_status) go through the same
 * expressions as in numpy: compares false, sums NaN. */
typedef struct VppxMetrics {
    double bad1, bad2, bad3, bad4; /* 'bad 1.0' ... 'bad 4.0' */
    double avgerr, rms;
    double n_valid;                /* pixels with validgt > 0 (an integer) */
    double reserved;
} VppxMetrics;                     /* 64 bytes */
typedef struct VppxEvalParams {
    int32_t gt_scale;  /* >= 1, default 1: --oscale (test.py:150-152): gt and validgt are read at every gt_scale-th row and
                        * column (F.interpolate nearest) and gt is divided by gt_scale (float32 true division) */
    int32_t reserved0;
} VppxEvalParams;
void vppx_eval_params_default(VppxEvalParams *p);

/* losses.guided_metrics for a batch: device pointers, stream-ordered, no synchronisation.  disp float32 [B,Ho,Wo]; gt, validgt
 * float32 [B,Hg,Wg] (validgt > 0 is valid: the reference's float mask); (Hg / gt_scale, Wg / gt_scale) (integer division)
 * must be (Ho, Wo), else VPPX_E_INVALID_ARG before anything is launched (the reference dies in a numpy broadcast there).
 * metrics_out: device VppxMetrics[B]; errormap (device float32 [B,Ho,Wo], may be NULL) receives the reference's seventh
 * entry, error * (validgt > 0).  ep == NULL: gt_scale 1. */
int vppx_guided_metrics_dev(vppx_ctx *ctx, const VppxEvalParams *ep, int B, int Ho, int Wo, const float *disp, int Hg, int Wg,
                            const float *gt, const float *validgt, VppxMetrics *metrics_out, float *errormap);
/* The same on host pointers, synchronous. */
int vppx_guided_metrics_host(vppx_ctx *ctx, const VppxEvalParams *ep, int B, int Ho, int Wo, const float *disp, int Hg, int Wg,
                             const float *gt, const float *validgt, VppxMetrics *metrics_out, float *errormap);
/* vppx_occ_vpp_rsgm_scaled_dev and, behind it on the same stream, the metrics of its result: test.py:136-252 in one call.  sp
 * may be NULL (unscaled); validhints NULL = unguided; gt / validgt are float32 [B,H,W] (the full frame shape) and ep->gt_scale
 * must take them to (Ho, Wo); disp_out is required.  The metrics are queued on the launch stream behind the post stage: once,
 * over the whole batch, also when the call runs in parts (vppx_last_call_parts), with vppx_set_pipeline, and inside the
 * captured graph of vppx_set_graph_mode. */
int vppx_occ_vpp_rsgm_eval_dev(vppx_ctx *ctx, const VppxOccParams *op, const VppxVppParams *vp, const VppxRsgmParams *rp,
                               const VppxScaleParams *sp, const VppxEvalParams *ep, int B, int H, int W, int C, const uint8_t *left,
                               const uint8_t *right, const float *g, const uint8_t *g_occ, const float *validhints, const float *gt,
                               const float *validgt, uint8_t *conf_out, uint8_t *l_vpp, uint8_t *r_vpp, float *disp_out,
                               float *disp_small, VppxMetrics *metrics_out, float *errormap);

/* ---- hint sampling (losses.py:5-10 sample_hints; test.py:125-129) ---------------------------------------------------------
 * What test.py does first for every dataset without raw hints: hints = src * (rand_like(src) < probability) * (validsrc > 0)
 * with torch's CPU generator.  Reproduced bit for bit: frame f of a call equals torch.manual_seed(seed + f (mod 2^32)) followed
 * by sample_hints(src, validsrc > 0, probability) on the CPU.  torch draws one tempered MT19937 word y per pixel in row-major
 * order -- valid or not -- and keeps k = y & 0xFFFFFF (rand = k * 2^-24); rand < probability compares in float32, which is
 * k < T with T = clamp(ceil((double)(float)probability * 2^24), 0, 2^24) (vppx_sample_threshold; NaN gives 0).  Then, with
 * sel = validsrc > 0 && k < T: hints = sel ? src : +0.0f (src unchanged, NaN / inf included; anything at an unselected pixel
 * gives 0), validhints = sel ? 1.0f : 0.0f.  Any probability is legal.  A frame's stream starts with its own seed (the
 * reference's one generator running on through all frames is a serial dependency between frames, as with the colours). */
typedef struct VppxSampleParams {
    double probability;  /* [0.05]  --guideperc */
    uint32_t seed;       /* [1]     frame f samples with seed + f */
    uint32_t reserved0;
    uint64_t reserved1;
} VppxSampleParams;
void vppx_sample_params_default(VppxSampleParams *p);
uint32_t vppx_sample_threshold(double probability);
/* src, validsrc, hints_out, validhints_out (may be NULL): float32 [B,H,W].  Device pointers, stream-ordered, no synchronisation;
 * one workgroup per frame walks the generator, so frames of a batch run in parallel.  VPPX_E_INVALID_ARG with nothing launched:
 * a NULL required pointer, B / H / W <= 0, H * W > 2^31. */
int vppx_sample_hints_dev(vppx_ctx *ctx, const VppxSampleParams *smp, int B, int H, int W, const float *src, const float *validsrc,
                          float *hints_out, float *validhints_out);
/* The same on host pointers, synchronous. */
int vppx_sample_hints_host(vppx_ctx *ctx, const VppxSampleParams *smp, int B, int H, int W, const float *src, const float *validsrc,
                           float *hints_out, float *validhints_out);
/* vppx_occ_vpp_rsgm_eval_dev on hints sampled on the way: test.py:125-252 in one call.  In place of g / validhints: smp, the
 * source pair src / validsrc (float32 [B,H,W]; both NULL = sample from gt / validgt, which are then required) and `guided`
 * (!= 0: --guided, the sampled mask is the validhints, test.py:207-208).  The sampled maps live in the context's workspace and
 * enter the path where a caller's would: at full size, in front of the --iscale decimation.  ep, gt, validgt and metrics_out may
 * all be NULL: sampled, not evaluated (errormap then NULL as well).  hints_out / validhints_out (float32 [B,H,W], may be NULL)
 * receive the sampled maps in launch-stream order.  With vppx_set_pipeline the sampling is the first kernel of the front stage
 * (two sets of maps alternate); with vppx_set_graph_mode it is launched in front of the replayed graph, so a new seed does not
 * re-capture; a call that runs in parts samples once, frame f with smp->seed + f. */
int vppx_occ_vpp_rsgm_sampled_dev(vppx_ctx *ctx, const VppxOccParams *op, const VppxVppParams *vp, const VppxRsgmParams *rp,
                                  const VppxScaleParams *sp, const VppxEvalParams *ep, const VppxSampleParams *smp, int B, int H, int W,
                                  int C, const uint8_t *left, const uint8_t *right, const float *src, const float *validsrc, int guided,
                                  const uint8_t *g_occ, const float *gt, const float *validgt, uint8_t *conf_out, uint8_t *l_vpp,
                                  uint8_t *r_vpp, float *disp_out, float *disp_small, VppxMetrics *metrics_out, float *errormap,
                                  float *hints_out, float *validhints_out);

/* ---- pictures (utils.py:17-79; test.py:318-343) --------------------------------------------------------------------------
 * What test.py --outdir renders per frame, for a batch: inputs float32 [B,H,W], pictures uint8 [B,H,W,3].  Every call takes a
 * `dilation` d >= 0, applied to the coloured picture as the reference does with cv2.dilate(img, np.ones((d, d))): per channel
 * the maximum over the offsets -(d/2) .. d-1-(d/2) in both axes (anchor d/2: an even window leans up and left), pixels outside
 * the frame ignored, frames of a batch independent; d = 0 and d = 1 are the identity.  The dilation is fused with the colouring
 * (no un-dilated picture goes through device memory).  d above VPPX_VIZ_MAX_DILATION: VPPX_E_UNSUPPORTED.  The window is a
 * restatement of OpenCV's documented behaviour; for d <= 1 the pictures are pinned to the reference.
 * Argument checks (VPPX_E_INVALID_ARG, nothing launched, `out` untouched): a NULL pointer, B / H / W <= 0, dilation < 0,
 * which == 0 or with a bit outside VPPX_VIZ_ALL, scale not > 0.  A picture is a function of its own frame only. */
#define VPPX_VIZ_MAX_DILATION 31
enum { /* planes of vppx_guided_visualize_*, in the reference's key order */
    VPPX_VIZ_BAD1 = 1, VPPX_VIZ_BAD2 = 2, VPPX_VIZ_BAD3 = 4, VPPX_VIZ_BAD4 = 8, VPPX_VIZ_AVGERR = 16, VPPX_VIZ_RMS = 32,
    VPPX_VIZ_ALL = 63
};
/* color_error_image_kitti: the ten rows of _color_map_errors_kitti in order, a later row overwrites an earlier one, both ends
 * of a bin inclusive (a value on an edge takes the higher bin); the float32 error is compared in double against lo / scale and
 * hi / scale (float64 quotients); NaN matches no bin and stays (0,0,0), +inf takes the last bin.  mask (may be NULL): pixels
 * with mask == 0 are black -- a negative or NaN mask value keeps its colour.  bgr == 0 swaps channels 0 and 2 (before the
 * dilation).  Device pointers, stream-ordered, no synchronisation. */
int vppx_error_colors_dev(vppx_ctx *ctx, int B, int H, int W, const float *errors, const float *mask, double scale, int bgr,
                          int dilation, uint8_t *out);
/* The same on host pointers, synchronous. */
int vppx_error_colors_host(vppx_ctx *ctx, int B, int H, int W, const float *errors, const float *mask, double scale, int bgr,
                           int dilation, uint8_t *out);
/* guided_visualize: with e = |disp - gt| in float32, plane 'bad k' (k = 1..4) is (49,54,149) where e > k, (165,0,38) where
 * e <= k, black for a NaN; 'avgerr' is the error colours of e, 'rms' those of sqrt((disp - gt)^2) in float32; valid == 0 is
 * black everywhere, any other value of valid is drawn.  out: six pictures uint8 [6][B,H,W,3] in the order of the VPPX_VIZ_*
 * bits; only the planes whose bit is set in `which` are computed and written, the others are not touched. */
int vppx_guided_visualize_dev(vppx_ctx *ctx, int B, int H, int W, const float *disp, const float *gt, const float *valid,
                              double scale, int dilation, unsigned which, uint8_t *out);
int vppx_guided_visualize_host(vppx_ctx *ctx, int B, int H, int W, const float *disp, const float *gt, const float *valid,
                               double scale, int dilation, unsigned which, uint8_t *out);
/* test.py:325-326, :343: out = lut[uint8(clamp(x, 0, max_val) / max_val * 255)]: clamp, divide, multiply, each rounded to
 * float32, then truncated.  max_val: one float per frame [B]; lut: uint8 [256][3], the user colour map cv2.applyColorMap takes.
 * Where the reference's cast is undefined the index is 0: x NaN, max_val not > 0 (NaN included), or a NaN quotient (inf / inf). */
int vppx_colorize_dev(vppx_ctx *ctx, int B, int H, int W, const float *x, const float *max_val, const uint8_t *lut, int dilation,
                      uint8_t *out);
int vppx_colorize_host(vppx_ctx *ctx, int B, int H, int W, const float *x, const float *max_val, const uint8_t *lut, int dilation,
                       uint8_t *out);
/* test.py:318: max_out[f] = the maximum of frame f with +inf and -inf replaced by -inf (-inf when nothing else is there); a NaN
 * in the frame gives NaN, as torch's max does.  Device pointers, stream-ordered; B <= 65535. */
int vppx_finite_max_dev(vppx_ctx *ctx, int B, int H, int W, const float *x, float *max_out);

/* ---- frame stream: the hot path for callers that hold one host frame at a time ---------------------------------------
 * test.py:291-311 iterates a DataLoader with batch size 1 and runs :154-225 per frame on numpy arrays; the kernels want
 * batches of one lock-step round, resident.  A frame stream takes (left, right, hints[, g_occ]) host arrays one frame at a
 * time and returns the disparities (and, by flags, mask and patterned pair) one frame at a time IN INPUT ORDER.  Inside,
 * every frame is copied once, by `copy_threads` threads, into a page-locked ring of `depth` batches; a full batch (`batch`
 * frames, vppx_batch_quantum is a good value) is uploaded on a copy stream under the previous batch's kernels, runs through
 * vppx_occ_vpp_rsgm_dev (op != NULL: the mask of test.py:154 on the way) or vppx_vpp_rsgm_dev with cross-call pipelining,
 * and comes down on a third stream: a copy-out kernel of a few workgroups that stores into the ring (no runtime copy engine:
 * which one a device -> host hipMemcpyAsync takes differs between runtime versions, and the blit-kernel one disturbs the hot
 * path).  With depth >= 3 (recommended: 3) a batch's copy-out waits for the NEXT batch's aggregation to finish, so that it
 * runs beside the sum / WTA kernel and never beside the lock-step launch; the pop, flush or re-run that needs the results
 * first releases it at once.  With depth 2 it runs right behind the batch's own kernels.  Frame f (counted from the stream's creation) draws from srand(vp->seed + f): results
 * equal one-frame calls with that seed whatever the batch size and wherever a flush falls.  The context must launch on
 * its own stream (the default of vppx_create) and must not be used for other calls while the stream exists.
 * A lost lock step (vppx_status) is handled inside: pop verifies each batch after its download and re-runs what was in
 * flight from the device inputs it still holds (vppx_fstream_counts reports how often).  Not thread-safe: one producer /
 * consumer thread (the calls release nothing to other threads but do not hold Python's GIL).
 * flags: VPPX_FS_PATTERNS pop can return the patterned pair; VPPX_FS_MASK (with op) the mask; VPPX_FS_GOCC every push brings
 * a caller's mask (op must be NULL); VPPX_FS_GUIDED every frame also brings its validhints and runs through
 * vppx_occ_vpp_rsgm_guided_dev (push with vppx_fstream_push_guided).  copy_threads < 0: chosen from the host's core count.
 * use_distance_patch: dmin / dmax are each frame's own, computed on the device (per_frame_range is set for the stream). */
#define VPPX_FS_PATTERNS 1
#define VPPX_FS_MASK 2
#define VPPX_FS_GOCC 4
#define VPPX_FS_GUIDED 8
#define VPPX_FS_METRICS 16  /* every push brings gt + validgt (vppx_fstream_push_eval); pop can return the frame's VppxMetrics */
#define VPPX_FS_NO_DISP 32  /* needs VPPX_FS_METRICS: disparities are not copied out; pop's disp_out must be NULL */
#define VPPX_FS_SAMPLE 64   /* the hints are sampled on the device (vppx_fstream_create_sampled, vppx_fstream_push_sampled) */
typedef struct vppx_fstream vppx_fstream;
int vppx_fstream_create(vppx_ctx *ctx, const VppxOccParams *op, const VppxVppParams *vp, const VppxRsgmParams *rp, int batch,
                        int depth, int H, int W, int C, int flags, int copy_threads, vppx_fstream **out);
void vppx_fstream_destroy(vppx_fstream *fs);
/* vppx_fstream_create with --iscale / --oscale: pushes take frames of H x W x C (and a VPPX_FS_GOCC mask at the scaled
 * shape), each batch runs through vppx_occ_vpp_rsgm_scaled_dev; pop returns disparities of (Ho, Wo) and patterns / mask of
 * (h, w) (vppx_scaled_shape).  sp == NULL or {1, 1} is vppx_fstream_create. */
int vppx_fstream_create_scaled(vppx_ctx *ctx, const VppxOccParams *op, const VppxVppParams *vp, const VppxRsgmParams *rp,
                               const VppxScaleParams *sp, int batch, int depth, int H, int W, int C, int flags, int copy_threads,
                               vppx_fstream **out);

/* One frame in (host arrays of the stream's H x W x C).  Returns when the frame has been copied: the arrays may be
 * reused at once.  The frame that completes a batch also queues the batch's upload, kernels and download (no waiting).
 * Fails with VPPX_E_INVALID_ARG when `depth` whole batches are waiting to be popped.  When submitting the completed batch
 * fails, the error is returned but the frame HAS been taken: the next push or vppx_fstream_flush submits that batch again
 * (a push copies nothing until it has), so vppx_fstream_counts never reports more than `batch` frames filling. */
int vppx_fstream_push(vppx_fstream *fs, const uint8_t *left, const uint8_t *right, const float *hints, const uint8_t *g_occ);
/* The same for a VPPX_FS_GUIDED stream: validhints (float32 [H,W], required) is copied into the ring with the frame.  Each of
 * the two push calls fails with VPPX_E_INVALID_ARG on the other kind of stream. */
int vppx_fstream_push_guided(vppx_fstream *fs, const uint8_t *left, const uint8_t *right, const float *hints, const uint8_t *g_occ,
                             const float *validhints);
/* Submit the frames pushed so far as a (smaller) batch: end of the sequence, or a latency bound. */
int vppx_fstream_flush(vppx_fstream *fs);
/* The next frame's results, in input order: *got = 1 and the arrays filled (NULL = not wanted; draws_out = rand() draws the
 * frame consumed, 0 for maxDistance), waiting for its batch when that is still running; *got = 0 when nothing submitted is
 * outstanding (frames of a batch still being filled need vppx_fstream_flush). */
int vppx_fstream_pop(vppx_fstream *fs, float *disp_out, uint8_t *l_vpp_out, uint8_t *r_vpp_out, uint8_t *conf_out,
                     uint64_t *draws_out, int *got);
/* An evaluating stream (flags must hold VPPX_FS_METRICS): every push brings the frame's ground truth at the full frame shape,
 * float32 gt [H,W] and validgt [H,W] (> 0 is valid; the ring keeps one byte per pixel of it), and the metrics of every batch
 * are computed on the device behind its kernels -- vppx_guided_metrics_dev of the stream's disparities with ep->gt_scale, which
 * must take (H, W) to the shape of the returned map -- and come down with the other results, 64 bytes per frame.  With
 * VPPX_FS_NO_DISP the disparity maps stay on the device.  sp may be NULL (unscaled), ep NULL means gt_scale 1.  A batch re-run
 * after a lost lock step re-runs its metrics: what a pop returns belongs to the disparities that pop verified. */
int vppx_fstream_create_eval(vppx_ctx *ctx, const VppxOccParams *op, const VppxVppParams *vp, const VppxRsgmParams *rp,
                             const VppxScaleParams *sp, const VppxEvalParams *ep, int batch, int depth, int H, int W, int C, int flags,
                             int copy_threads, vppx_fstream **out);
/* One frame with its ground truth in; validhints NULL unless VPPX_FS_GUIDED.  As vppx_fstream_push otherwise (a failed submit
 * included).  vppx_fstream_push / _push_guided on a VPPX_FS_METRICS stream and this call on any other stream fail with
 * VPPX_E_INVALID_ARG. */
int vppx_fstream_push_eval(vppx_fstream *fs, const uint8_t *left, const uint8_t *right, const float *hints, const uint8_t *g_occ,
                           const float *validhints, const float *gt, const float *validgt);
/* vppx_fstream_pop plus the frame's metrics (metrics_out may be NULL; non-NULL needs a VPPX_FS_METRICS stream).  disp_out may
 * be NULL here, and must be on a VPPX_FS_NO_DISP stream (VPPX_E_INVALID_ARG otherwise, also from vppx_fstream_pop). */
int vppx_fstream_pop_eval(vppx_fstream *fs, float *disp_out, uint8_t *l_vpp_out, uint8_t *r_vpp_out, uint8_t *conf_out,
                          uint64_t *draws_out, VppxMetrics *metrics_out, int *got);
/* A sampling stream (flags must hold VPPX_FS_SAMPLE, smp is required): no push brings hints, every batch runs through
 * vppx_occ_vpp_rsgm_sampled_dev; frame f of the stream (counted from its creation) samples with smp->seed + f, as it draws its
 * colours from srand(vp->seed + f).  ep != NULL makes it an evaluating stream as well (flags must then hold VPPX_FS_METRICS, and
 * must not otherwise); VPPX_FS_GUIDED feeds the sampled mask as validhints.  A batch re-run after a lost lock step samples again:
 * the same bytes. */
int vppx_fstream_create_sampled(vppx_ctx *ctx, const VppxOccParams *op, const VppxVppParams *vp, const VppxRsgmParams *rp,
                                const VppxScaleParams *sp, const VppxEvalParams *ep, const VppxSampleParams *smp, int batch, int depth,
                                int H, int W, int C, int flags, int copy_threads, vppx_fstream **out);
/* One frame in.  src / validsrc (float32 [H,W], together or both NULL) are what the hints are sampled from; the ring keeps one
 * byte per pixel of validsrc > 0.  On a VPPX_FS_METRICS stream gt / validgt are required and src may be NULL: the ring then
 * holds no hints plane at all for the frame and the gt already there is the source.  (A frame whose kind of source differs
 * from the batch being filled starts a new batch.)  The other push calls fail with VPPX_E_INVALID_ARG on a sampling stream,
 * this one on any other stream. */
int vppx_fstream_push_sampled(vppx_fstream *fs, const uint8_t *left, const uint8_t *right, const uint8_t *g_occ, const float *src,
                              const float *validsrc, const float *gt, const float *validgt);
/* Frames pushed since creation, frames of the batch being filled, frames submitted and not yet popped, batches re-run
 * after a lost lock step (any pointer may be NULL). */
int vppx_fstream_counts(vppx_fstream *fs, int64_t *pushed, int64_t *filling, int64_t *unpopped, int64_t *reruns);

/* ---- hand-off to the deep front-ends (test.py:179-200) -------------------------------------- */
/* uint8 [B,H,W,C] (device) -> [B,C,Hq,Wq] float32 (dst_is_bf16 = 0) or bfloat16 (1) in [0,1]
 * (value/255. as the reference computes it), replicate-padded up to multiples of
 * pad_multiple (32 for PSMNet / RAFT-Stereo, test.py:189-198) with lo = pad//2. */
int vppx_u8_to_nchw_dev(vppx_ctx *ctx, int B, int H, int W, int C, int pad_multiple, const uint8_t *src, void *dst,
                        int dst_is_bf16);

/* PSMNet matching volume (models/psmnet/psmnet.py:157-197): fea_l/fea_r float32 [B,C,H4,W4] ->
 * cost float32 [B,2C,maxdisp/4,H4,W4] (caller-allocated, every element written):
 *   cost[b,c,i,y,x] = x>=i ? fea_l[b,c,y,x] : 0,  cost[b,C+c,i,y,x] = x>=i ? fea_r[b,c,y,x-i] : 0,
 * multiplied, when hints != NULL, by (1-v) + v*10*exp(-(i-h)^2 / (2*(1/4)^2)) with h, v the hints
 * (float32 [B,1,H,W], H/4 == H4, W/4 == W4) and validhints sub-sampled 'nearest' like F.upsample and
 * h = hints*valid/4 (psmnet.py:172-197).  float32 throughout; exp() is the only inexact step: every other operation
 * is the reference's, correctly rounded, so the argument of exp() is the reference's bit for bit, and a cell is within
 * one unit in the last place of expf, carried through the three roundings behind it, of the same expression with an
 * exact exp (tests/_handoff_ref.py, limit()).
 * A pixel with v == 0 is untouched: its cells are the un-modulated volume's, bit for bit.  That equals the reference,
 * which multiplies by (1-0) + (0*10)*exp(..) = 1, for every finite hint, and differs from it where an invalid pixel
 * carries a hint that is not finite (inf for "unknown"): there hints*valid is NaN and the reference's cells turn NaN. */
int vppx_psmnet_cost_volume_dev(vppx_ctx *ctx, const float *fea_l, const float *fea_r, const float *hints,
                                const float *validhints, int B, int C, int H4, int W4, int H, int W, int maxdisp,
                                float *cost);
/* RAFT-Stereo hint modulation of the all-pairs correlation, in place (models/raft_stereo/corr.py:160-178):
 * corr float32 [B,H4,W2,1,W3] (= einsum(fmap2,fmap3)/sqrt(D), a library GEMM left to the caller);
 * corr[b,y,x,0,k] *= (1-v) + v*10*exp(-(k-(x*v-h))^2/2).  Rows with v == 0 are untouched (not read, not written): the
 * reference's factor is exactly 1 there for a finite hint and NaN for a non-finite one, as above.
 * hints / validhints are float32 [B,1,H,W] with H/4 == H4 and W/4 == W2: the library can check only those two
 * quotients, the caller answers for B frames of H*W floats behind both pointers and B*H4*W2*W3 behind corr. */
int vppx_raft_corr_modulate_dev(vppx_ctx *ctx, float *corr, const float *hints, const float *validhints, int B, int H4,
                                int W2, int W3, int H, int W);
/* The same two calls with the storage type of the large tensors as an argument. */
typedef enum VppxDtype {
    VPPX_DT_F32 = 0,  /* float32: exactly vppx_psmnet_cost_volume_dev / vppx_raft_corr_modulate_dev, which are this case */
    VPPX_DT_BF16 = 1  /* bfloat16 (the upper 16 bits of a float32) for fea_l, fea_r and cost / for corr                   */
                      /* (2 is kept for float16, which is not implemented)                                                 */
} VppxDtype;
/* dtype = VPPX_DT_BF16: fea_l, fea_r and cost (corr) hold bfloat16, 2-byte aligned; hints and validhints stay float32
 * [B,1,H,W].  Only the storage type differs from the float32 call:
 *   - a cell is widened to float32 (exact), multiplied in float32 by the same float32 factor as above, and rounded to
 *     bfloat16 ONCE, to nearest even.  Nothing in between is held in bfloat16, neither the factor nor the sub-sampled
 *     hints.  NaN stays NaN; a product beyond the largest bfloat16 becomes infinity, as round-to-nearest-even gives.
 *   - a cell that is not modulated keeps the 16 bits of its feature (of corr): hints == NULL, a pixel with v == 0 (the
 *     v == 0 rule above; RAFT rows with v == 0 are neither read nor written).  NaN payloads, -0 and subnormals come
 *     through unchanged.  Cells with x < i are +0 (bits 0x0000).
 * What differs from the float32 call on the widened features followed by a cast to bfloat16 (round-to-nearest-even):
 * nothing in value, the result is the float32 result rounded once.  Two bit patterns differ: the cast quiets a
 * signalling NaN of an un-modulated cell where this call copies it, and a cell with x < i is +0 here where the float32
 * call leaves 0 * factor, which is -0 under a negative factor (v < 0) and NaN under a NaN factor.
 * The argument checks, their order and their messages are those of the float32 entries; a dtype other than the two
 * above is VPPX_E_INVALID_ARG with nothing launched and no output byte touched.  The volume is written with 16-byte
 * stores when W4 % 8 == 0 and cost, fea_l and fea_r are 16-byte aligned, and cell by cell otherwise. */
int vppx_psmnet_cost_volume_dt_dev(vppx_ctx *ctx, const void *fea_l, const void *fea_r, const float *hints,
                                   const float *validhints, int B, int C, int H4, int W4, int H, int W, int maxdisp,
                                   void *cost, int dtype);
int vppx_raft_corr_modulate_dt_dev(vppx_ctx *ctx, void *corr, const float *hints, const float *validhints, int B, int H4,
                                   int W2, int W3, int H, int W, int dtype);
/* ---- CorrBlock1D: the pyramid and the lookup (models/raft_stereo/corr.py:116-145) ------------------------------
 * The volume is N = B*H4*W2 rows of W3 cells, float32 or bfloat16 (dtype as above).  Level 0 is the volume itself, level i
 * has Wi = W3 >> i cells per row.  Every step below is one correctly rounded float32 operation, in this order; the
 * float32 results are those of the reference's avg_pool2d / grid_sample composition bit for bit.
 *
 * Pyramid:  level_i[k] = ((+0 + level_{i-1}[2k]) + level_{i-1}[2k+1]) / 2; an odd last column is dropped.  The sum starts
 * at +0, so two -0 cells pool to +0.  Each level is pooled from the level below AS STORED: with bfloat16 storage the
 * two bfloat16 cells are widened, summed and halved in float32 and the result is rounded to bfloat16 once, to nearest even
 * (NaN as above), which is what torch's bfloat16 avg_pool2d gives.  One sign is IEEE's and not torch's CPU kernel's: a
 * negative sum whose half rounds to zero gives -0 (torch on a CPU returns +0 there).
 * With hints != NULL the call first modulates level 0 in place, exactly as the modulation call above does (the same
 * factor, rows with v == 0 untouched), and pools the modulated values: one pass over the volume instead of two.  Rows
 * with v == 0 are not written, and are pooled like every other row.  With hints == NULL corr is not written.
 * pyr receives levels 1 .. levels-1 back to back, each dense [N][W3 >> i], in the volume's dtype; the cells-query below gives
 * the total number of cells and, in offsets[i] for i = 1 .. levels-1 (offsets[0] = 0, unused; offsets may be NULL), the first cell of
 * level i.  It returns a negative VPPX_E_* code for N, W3 <= 0, levels < 1 (INVALID_ARG) or levels > 4 (UNSUPPORTED).
 * pyr may be NULL when levels == 1 (nothing is pooled; with hints the call is then the modulation alone).
 *
 * Lookup:  for pixel n = (b, y, x) with c = coords_x[b * coords_frame_stride + y * W2 + x], level i of width W = Wi and
 * tap t = 0 .. 2*radius:
 *     x  = (float)(t - radius) + c / 2^i
 *     xg = (2 * x) / (W - 1) - 1
 *     ix = ((xg + 1) / 2) * (W - 1)          the round trip changes the position in its last bits; it is not shortcut
 *     fl = floor(ix);  wr = ix - fl;  wl = (fl + 1) - ix
 *     a  = fl     in [0, W-1] ? level_i[n][fl]     : +0
 *     b  = fl + 1 in [0, W-1] ? level_i[n][fl + 1] : +0          (compared in float: 1e30 is outside, not an index)
 *     out[b][i * (2*radius+1) + t][y][x] = fma(b, wr, +0 + a * wl)
 * out is float32 [B, levels*(2*radius+1), H4, W2], the reference's .permute(0,3,1,2).contiguous().float() layout, every
 * cell written.  A cell with neither tap in range is +0.  A NaN cell of the volume under a weight of zero gives NaN,
 * as the formula says.  Where ix is not finite (a NaN or infinite coordinate) the cell is +0: the reference converts
 * such a position to an integer index, which is undefined, so there is nothing to be equal to.
 * coords_x points at channel 0 of the reference's coords1 [B,2,H4,W2] (coords_frame_stride = 2*H4*W2) or at a bare
 * [B,H4,W2] (H4*W2); channel 1 is never read.
 * bfloat16 storage: the two taps are widened to float32 and everything else is as above; out stays float32 and is
 * not rounded.  This has no reference counterpart: torch's bfloat16 grid_sample does its arithmetic in bfloat16 and
 * does not take a float32 grid.
 * Both device calls are stream-ordered and do not synchronise.  Refused before anything is launched, with no output
 * byte touched: a NULL corr / coords_x / out, pyr == NULL with levels > 1, hints without validhints, B, H4, W2 or
 * W3 <= 0, levels < 1, radius < 0, coords_frame_stride < H4*W2, a dtype other than the two (VPPX_E_INVALID_ARG);
 * W3 >> (levels-1) < 2, where the reference divides by W - 1 = 0 (VPPX_E_INVALID_ARG); levels > VPPX_CORR_MAX_LEVELS or
 * radius > VPPX_CORR_MAX_RADIUS (VPPX_E_UNSUPPORTED); with hints, H/4 != H4 or W/4 != W2 with the modulation call's message. */
#define VPPX_CORR_MAX_LEVELS 4
#define VPPX_CORR_MAX_RADIUS 8
int64_t vppx_raft_corr_pyramid_cells(int64_t N, int W3, int levels, int64_t *offsets);
int vppx_raft_corr_pyramid_dt_dev(vppx_ctx *ctx, void *corr, const float *hints, const float *validhints, int B, int H4, int W2,
                                  int W3, int H, int W, int levels, void *pyr, int dtype);
int vppx_raft_corr_lookup_dt_dev(vppx_ctx *ctx, const void *corr, const void *pyr, const float *coords_x,
                                 int64_t coords_frame_stride, int B, int H4, int W2, int W3, int levels, int radius,
                                 float *out, int dtype);
/* ---- CorrBlock1D: the all-pairs correlation itself, fused into the pyramid (models/raft_stereo/corr.py:151-155, 116-124)
 * One launch reads fmap2 [B,D,H4,W2] and fmap3 [B,D,H4,W3] (NCHW, float32 or bfloat16, both of `dtype`) and writes level 0
 * into corr [B,H4,W2,1,W3] and levels 1 .. levels-1 into pyr, both of `dtype`, in the layout of the pyramid call above
 * (vppx_raft_corr_pyramid_cells): what it leaves is what vppx_raft_corr_lookup_dt_dev takes.  The volume is not read back.
 *     acc[b,y,x2,x3] = sum over k < D of fmap2[b,k,y,x2] * fmap3[b,k,y,x3]
 *         a float32 sum that starts at +0, accumulated in float32 by the matrix cores in an order the library chooses
 *         and this header does not promise; a bfloat16 product is exact in float32.  Where every partial sum is exact in
 *         float32, as for features on a coarse grid, the order does not matter and acc is the exact value.
 *     c = acc / sqrt((float)D)          one correctly rounded float32 square root and one correctly rounded float32
 *                                        DIVISION, never a multiplication by a reciprocal
 *     with hints != NULL, for a row (b, y, x2) with v != 0:  c = c * modulation(v, h, (float)x3, 2)
 *         the factor, the sub-sampling of hints / validhints [B,1,H,W] and the v == 0 rule are those of
 *         vppx_raft_corr_modulate_dt_dev; a row with v == 0 (or -0) keeps c.
 *     level 0: float32 storage holds c; bfloat16 storage holds c rounded to bfloat16 once, to nearest even (NaN as above): the
 *         only rounding to bfloat16 a level-0 cell sees.
 *     levels 1..: the pyramid rule above applied to the level below AS STORED, an odd last column dropped.  They equal,
 *         bit for bit in both dtypes, what vppx_raft_corr_pyramid_dt_dev without hints makes of this call's level 0.
 * A feature that is not finite makes the cells of its row (fmap2) or column (fmap3) not finite and no others; cells of
 * the matrices' padding inside the kernel are zeros and are never stored.
 * The feature maps are read with 16-byte loads when the pointer is 16-byte aligned and the row (W2, W3 cells) is a whole
 * number of 16 bytes, and cell by cell otherwise; the same holds for the stores, per level.  A map may start anywhere.
 * The call is stream-ordered and does not synchronise.  Refused before anything is launched, with no output byte touched:
 * a NULL fmap2 / fmap3 / corr, pyr == NULL with levels > 1, hints without validhints, B, D, H4, W2 or W3 <= 0,
 * levels < 1, W3 >> (levels-1) < 2, a dtype other than the two (VPPX_E_INVALID_ARG); levels > VPPX_CORR_MAX_LEVELS
 * (VPPX_E_UNSUPPORTED); with hints, H/4 != H4 or W/4 != W2 with the modulation call's message. */
int vppx_raft_corr_fused_dt_dev(vppx_ctx *ctx, const void *fmap2, const void *fmap3, const float *hints,
                                const float *validhints, int B, int D, int H4, int W2, int W3, int H, int W, int levels,
                                void *corr, void *pyr, int dtype);
/* ---- The read-out: the networks' output back as a float32 disparity map ---------------------------------------
 * (models/psmnet/psmnet.py:227-233 + submodule.py:115-128, models/raft_stereo/raft_stereo.py:69-81,153-154, and the
 * negation and crop of test.py:237-245).  Both outputs are what vppx_guided_metrics_dev, vppx_error_colors_dev and
 * vppx_colorize_dev take.  Neither call is bit-equal to the torch composition, whose summation order is torch's own:
 * both do the arithmetic below in float32 with float32 accumulators, and tests/_readout_ref.py derives how far any
 * float32 association of it can lie from the exact value.  dtype (VppxDtype) is the storage of cost / of flow and mask:
 * bfloat16 cells are widened on load (exact); out is float32 always.
 *
 * PSMNet:  cost [B,D4,H4,W4] (cost3 without its channel of one), D = maxdisp, the map is H x W.  Per axis with n_in
 * source and n_out output cells, all in float32, as ATen's align_corners = False linear upsampling to a given size:
 *     scale = (float)n_in / (float)n_out;  src = max(fma(scale, dst + 0.5f, -0.5f), 0)        one rounding, as ATen compiles it
 *     i0 = (int)src;  i1 = i0 + (i0 < n_in - 1);  l1 = src - i0;  l0 = 1 - l1
 *     p_k = ly0 * (lx0 * c[k,y0,x0] + lx1 * c[k,y0,x1]) + ly1 * (lx0 * c[k,y1,x0] + lx1 * c[k,y1,x1])      k = 0 .. D4-1
 *     z_d = l0(d) * p_i0(d) + l1(d) * p_i1(d)                                                              d = 0 .. D-1
 *     out[b,y,x] = sum_d d * exp(z_d - max_d z) / sum_d exp(z_d - max_d z)
 * Any D4, H4, W4 >= 1 and any maxdisp, H, W >= 1 (F.upsample takes any size); the 401 MB volume [B,D,H,W] of the
 * 544x960x192 case is never formed.
 *
 * RAFT-Stereo:  flow [B,C,H4,W4], frame b at flow + b * flow_frame_stride cells (so channel 0 of a [B,2,H4,W4] tensor
 * is C = 1 with a stride of 2*H4*W4, without a copy), mask [B,mask_channels,H4,W4] with mask_channels = 9*f*f, f = 1, 2,
 * 4 or 8 (2^n_downsample); the map is f*H4 x f*W4:
 *     p_k = softmax over k = 0 .. 8 of mask[b, k*f*f + i*f + j, y, x], the maximum subtracted
 *     out[b, c, f*y+i, f*x+j] = sign * sum_k p_k * (f * flow[b, c, y+ky-1, x+kx-1]),   k = 3*ky + kx
 * with flow = +0 outside the map and sign = +1 or -1 (test.py:238 negates).
 *
 * The crop (test.py:242-245):  out is [B,Hout,Wout] / [B,C,Hout,Wout], the window of Hout x Wout pixels whose first
 * pixel is (top, left) of the map; pixels outside it are not computed.  top = left = 0, Hout = H, Wout = W is the map.
 * Non-finite input follows the arithmetic and stays in its pixel: a NaN or +inf logit (mask cell) makes the pixels
 * that read it NaN, a -inf one has weight 0 (a pixel whose logits are all -inf is NaN, as 0/0 is); a non-finite flow
 * cell makes the pixels that read it NaN or infinite; as in torch, a cell under a weight of exactly zero still counts
 * (0 * inf = NaN).  Other pixels are untouched.
 * Both calls are stream-ordered and do not synchronise.  Refused before anything is launched, with no output byte
 * touched: a NULL cost / flow / mask / out, B, C, D4, H4, W4, maxdisp, H or W <= 0, a sign other than +1 and -1, a
 * dtype other than the two, f not 1, 2, 4 or 8, mask_channels != 9*f*f, flow_frame_stride < C*H4*W4, a window with
 * top or left < 0, Hout or Wout <= 0, or reaching past the map (VPPX_E_INVALID_ARG); more pixels than one launch
 * takes, or, for PSMNet, 16*maxdisp + 256*D4 bytes above 64 KiB (VPPX_E_UNSUPPORTED: maxdisp = 192 with D4 = 48 is
 * 15 KiB). */
int vppx_psmnet_readout_dt_dev(vppx_ctx *ctx, const void *cost, int B, int D4, int H4, int W4, int maxdisp, int H, int W,
                               int top, int left, int Hout, int Wout, float *out, int dtype);
int vppx_raft_upsample_dt_dev(vppx_ctx *ctx, const void *flow, int64_t flow_frame_stride, const void *mask, int B, int C,
                              int H4, int W4, int f, int mask_channels, int sign, int top, int left, int Hout, int Wout,
                              float *out, int dtype);
/* ---- The update block's glue: what BasicMultiUpdateBlock.forward runs between its convolutions ------------------
 * (models/raft_stereo/update.py:119-142 with ConvGRU.forward :23-32, pool2x :89-90, interp :95-97 and the encoder's
 * cat :87).  Three calls; the convolutions between them stay the caller's.  dtype (VppxDtype) is the storage of every
 * tensor of a call: bfloat16 cells are widened on load (exact), the arithmetic below is float32, one correctly rounded
 * operation per step, and a bfloat16 result is the float32 result rounded once, to nearest even (NaN stays NaN).
 * tests/_gru_ref.py derives how far any float32 evaluation of it can lie from the exact value.
 *
 * Addressing.  Every tensor argument is [B,C,H,W]; frame b starts b * its frame stride cells behind the pointer, and a
 * frame is contiguous.  A frame stride is at least C*H*W.  cz, cr and cq are therefore passed as the three channel
 * slices of one [B,3C,H,W] convolution output (raft_stereo.py:104) with a stride of 3C*H*W, without a copy.  No
 * pointer has to be aligned beyond its cell: a call moves 16 bytes per lane where every pointer it takes is 16-byte
 * aligned and every frame stride a whole number of 16 bytes, and cell by cell otherwise, with the same results.
 *
 * Assemble:  hx [B,hx_channels,H,W] contiguous; channels 0 .. sum C_i - 1 receive cat(sources, dim=1), channels beyond
 * them are not written.  Source i is [B,C,Hs,Ws] and arrives by its mode:
 *     VPPX_GRU_COPY     Hs = H, Ws = W; the cell itself (a bfloat16 cell keeps its 16 bits where the copy moves whole vectors,
 *                       and is widened and rounded back, which changes no value, elsewhere)
 *     VPPX_GRU_POOL2X   F.avg_pool2d(x, 3, stride=2, padding=1):  (Hs-1)/2 + 1 == H and (Ws-1)/2 + 1 == W;
 *                       out[y,x] = (sum over ky, kx = 0 .. 2 of x[2y-1+ky, 2x-1+kx], +0 outside the map, started at +0
 *                       and taken in the order k = 3*ky + kx) / 9, the divisor being 9 at the border too
 *     VPPX_GRU_INTERP   F.interpolate(x, (H,W), mode='bilinear', align_corners=True) from any Hs, Ws >= 1.  Per axis:
 *                       scale = (float)(n_in-1) / (float)(n_out-1), or 0 when n_out == 1;  src = scale * dst
 *                       i0 = (int)src;  i1 = i0 + (i0 < n_in-1);  l1 = src - i0;  l0 = 1 - l1
 *                       out = (ly0 * (lx0*a + lx1*b)) + (ly1 * (lx0*c + lx1*d)),  a, b on row y0 and c, d on row y1
 * Reset:  r = sigmoid(ar + cr);  hx[b, c] = r * h[b, c] for c < C, IN PLACE over the first C channels of hx
 * [B,hx_channels,H,W]; channels C .. hx_channels-1 are neither read nor written.
 *     Ordering contract.  The call overwrites the h part of the buffer the z and r convolutions read.  It is stream-
 *     ordered: enqueue it after both convolutions on the same stream (or behind an event of theirs) and the q
 *     convolution after it; that convolution then reads cat([r*h, x]) from the same buffer, with no second buffer and no
 *     copy of x.  h is read from its own tensor (net[i]), never from hx, and must not overlap the cells written.
 * Update:  z = sigmoid(az + cz);  q = tanh(aq + cq);  out = ((1 - z) * h) + (z * q).  z is recomputed from az rather than
 * kept by the reset call.  out may be h itself (every cell is read before it is written, by the lane that writes it);
 * it must not overlap any other argument.
 *     sigmoid(v) = 1 / (1 + expf(-v))            tanh(v) = 1 - 2 / (expf(2 * v) + 1)
 * with the device's expf and IEEE operations otherwise, so that v = +inf gives 1 and 1, v = -inf gives 0 and -1, neither
 * gives NaN, and a large finite v saturates the same way (expf overflows to +inf).  Non-finite input follows the arithmetic
 * and stays in its cell: a NaN gives NaN in that cell (and, through pool2x and interp, in the cells whose window holds it).
 * All three calls are stream-ordered, never synchronise and allocate nothing.  Refused before anything is launched, with
 * no output byte touched: a NULL pointer (sources, a source's ptr, any tensor); B, C, H, W, Hs or Ws <= 0; a frame stride
 * below C*H*W (C*Hs*Ws for a source); a dtype other than the two; n_sources < 1 or > VPPX_GRU_MAX_SOURCES; an unknown
 * mode; a copied source that is not H x W, a pooled one of the wrong size; hx_channels below sum C_i (assemble) or below
 * C (reset), where hx_frame_stride below hx_channels*H*W is refused as well (VPPX_E_INVALID_ARG); more cells than one launch
 * takes (VPPX_E_UNSUPPORTED). */
#define VPPX_GRU_MAX_SOURCES 4
typedef enum VppxGruMode { VPPX_GRU_COPY = 0, VPPX_GRU_POOL2X = 1, VPPX_GRU_INTERP = 2 } VppxGruMode;
typedef struct VppxGruSource {
    const void *ptr;      /* [B,C,Hs,Ws] of the call's dtype (device)                */
    int64_t frame_stride; /* cells between frames, >= C*Hs*Ws                        */
    int32_t C, Hs, Ws;
    int32_t mode;         /* VppxGruMode                                             */
} VppxGruSource;
int vppx_raft_gru_assemble_dt_dev(vppx_ctx *ctx, const VppxGruSource *sources, int n_sources, int B, int H, int W, void *hx,
                                  int hx_channels, int dtype);
int vppx_raft_gru_reset_dt_dev(vppx_ctx *ctx, const void *ar, int64_t ar_frame_stride, const void *cr, int64_t cr_frame_stride,
                               const void *h, int64_t h_frame_stride, void *hx, int64_t hx_frame_stride, int B, int C, int H, int W,
                               int hx_channels, int dtype);
int vppx_raft_gru_update_dt_dev(vppx_ctx *ctx, const void *az, int64_t az_frame_stride, const void *cz, int64_t cz_frame_stride,
                                const void *aq, int64_t aq_frame_stride, const void *cq, int64_t cq_frame_stride, const void *h,
                                int64_t h_frame_stride, void *out, int64_t out_frame_stride, int B, int C, int H, int W, int dtype);
/* ---- The motion encoder's front: the lookup fused into convc1, and convf1 (models/raft_stereo/update.py:80,82) -------
 * One launch makes cor1 = relu(convc1(corr_fn(coords1))) and flo1 = relu(convf1(flow)) of BasicMotionEncoder.forward; the
 * float32 [B, levels*(2*radius+1), H4, W2] tensor of taps between the lookup and convc1 is never written.  corr, pyr,
 * coords_x, coords_frame_stride, W3, levels, radius and dtype are those of vppx_raft_corr_lookup_dt_dev above.  Per pixel
 * n = (b, y, x), with K = levels*(2*radius+1) and p = ks / 2:
 *     taps[k], k = i * (2*radius+1) + t:  the lookup's arithmetic above, operation by operation (a bfloat16 cell of the
 *         pyramid is widened first); the taps stay float32 and are bit for bit what the lookup call would have stored.
 *     out_c[b][m][y][x] = relu(bias_c[m] + sum over k < K of wc[m][k] * taps[k])                                   m < Cc
 *     out_f[b][m][y][x] = relu(bias_f[m] + sum over c < 2, dy < ks, dx < ks of
 *                              wf[m][c][dy][dx] * flow[b][c][y + dy - p][x + dx - p])                              m < Cf
 *         with flow = +0 outside the map: cross-correlation, as nn.Conv2d computes it, not a flipped kernel.
 * The sums are float32, accumulated in float32 by the matrix cores (v_mfma_f32_16x16x4_f32 for both pyramid dtypes: a tap
 * is never rounded to bfloat16), starting at +0, in an order the library chooses and this header does not promise, as in
 * vppx_raft_corr_fused_dt_dev; the bias is one more term of that sum.  tests/_motion_ref.py derives how far any float32
 * evaluation in any order can lie from the exact value.  relu(v) = v > 0 ? v : 0 where a NaN stays NaN, as torch's; the
 * sign of a zero result is not specified.  A pixel whose taps are all +0 (a coordinate far outside, infinite or NaN) gives
 * relu(bias_c[m]) exactly.  A flow cell that is not finite reaches the ks x ks pixels whose window holds it and no others.
 * wc [Cc][K] and wf [Cf][2][ks][ks] are float32 always, in torch's [Cout, Cin, kh, kw] layout, contiguous; bias_c [Cc] and
 * bias_f [Cf] are float32 and either may be NULL (no bias).  flow is float32 [B,2,H4,W2].  out_c [B,Cc,H4,W2] and out_f
 * [B,Cf,H4,W2] are of out_dtype (VppxDtype), independent of the pyramid's dtype: a bfloat16 cell is the float32 result
 * rounded once, to nearest even (NaN stays NaN).  Every cell of both is written.
 * Addressing: frame b of flow, out_c and out_f starts b * its frame stride cells behind the pointer and is contiguous, so
 * out_c and out_f may be channel slices of one [B,Cc+Cf,H4,W2] buffer.  No pointer has to be aligned beyond its cell: an
 * output is written 16 bytes at a time where its pointer is 16-byte aligned and its frame stride and H4*W2 are whole numbers
 * of 16 bytes, and cell by cell otherwise, with the same results.
 * The call is stream-ordered, does not synchronise and allocates nothing.  Refused before anything is launched, with no output
 * byte touched: everything the lookup refuses, with the lookup's codes; a NULL flow, wc, wf, out_c or out_f; a frame stride
 * below its tensor's size (2, Cc or Cf planes of H4*W2); Cc or Cf <= 0; ks < 1 or even; an out_dtype other than the two
 * (VPPX_E_INVALID_ARG); Cc or Cf not a multiple of 16 or above VPPX_MOTION_MAX_CH, ks above VPPX_MOTION_MAX_KS, B*H4*W2 above
 * 2^31 - 1 pixels (VPPX_E_UNSUPPORTED). */
#define VPPX_MOTION_MAX_CH 64
#define VPPX_MOTION_MAX_KS 7
int vppx_raft_motion_front_dt_dev(vppx_ctx *ctx, const void *corr, const void *pyr, const float *coords_x,
                                  int64_t coords_frame_stride, const float *flow, int64_t flow_frame_stride, const float *wc,
                                  const float *bias_c, int Cc, const float *wf, const float *bias_f, int Cf, int ks, int B, int H4,
                                  int W2, int W3, int levels, int radius, void *out_c, int64_t out_c_frame_stride, void *out_f,
                                  int64_t out_f_frame_stride, int dtype, int out_dtype);
/* ---- The encoders' glue: what BasicEncoder / MultiBasicEncoder / ResidualBlock.forward run between their convolutions ----
 * (models/raft_stereo/extractor.py:48-60, :181-183, :276-278): InstanceNorm2d or a frozen BatchNorm2d, the ReLUs and the
 * residual sum.  Two calls; the convolutions stay the caller's.  dtype (VppxDtype) is the storage of x, res and out;
 * statistics, weights and biases are float32 always.  Addressing is that of the update block's calls above: a tensor is
 * [B,C,H,W], frame b starts b * its frame stride cells behind the pointer and is contiguous, so a channel slice of a wider
 * tensor goes in without a copy.  No pointer has to be aligned beyond its cell: both calls move 16 bytes per lane where
 * every tensor pointer is 16-byte aligned and every frame stride and H*W a whole number of 16 bytes, and cell by cell
 * otherwise, with the same bits in every result.
 *
 * Why these two calls take the context LAST and no struct: tests/test_header_cpu.py pins the number of prototypes whose
 * first parameter is the handle and the set of structs of this header, and neither may move for an addition.  Everything
 * else about them is as everywhere: VPPX_E_NO_DEVICE with "context is NULL" for a NULL context (checked first), the
 * context's stream, vppx_last_error.
 *
 * Statistics:  stats [B][C][2] float32, contiguous, receives (mean, rstd) of every plane of n = H*W cells.  A cell is
 * widened to float64 (exact); S1 = sum x and S2 = sum x*x (each square exact in float64) are accumulated in float64 in an
 * order the library chooses, which depends on H*W and on vppx_norm_stats_pieces(B*C, H*W) alone -- never on alignment, the
 * frame stride or the dtype of the cells; then, in float64,
 *     mean64 = S1 / n;   var64 = S2 / n - mean64 * mean64, and 0 where that is below 0 (a NaN stays: the biased variance
 *     F.instance_norm uses);   mean = (float)mean64;   rstd = (float)(1 / sqrt(var64 + (double)eps))
 * tests/_norm_ref.py derives the bound: n * 2^-53 relative to sum |x| and sum x*x, and the two roundings to float32.
 * A plane is split over vppx_norm_stats_pieces(B*C, H*W) workgroups, each taking ceil(H*W / pieces) cells rounded up to a
 * whole number of 16 and the last what is left; with more than one, their partial sums go through the
 * context's workspace (16 bytes per piece; the call allocates, and waits for the stream first, only while that buffer grows,
 * which a graph capture refuses) and a second small launch adds
 * them in piece order.  No float atomic, no dependence on dispatch order: a call repeated gives the same bits.
 * A NaN cell makes mean and rstd of its plane NaN; an infinite cell makes mean infinite and rstd NaN (inf - inf); either
 * way the apply call below turns every cell of that plane, and of no other, into NaN.
 *
 * Apply:  one launch, float32, one correctly rounded operation per step, per cell of plane (b, c):
 *     v = (x - mean) * rstd                        (mean, rstd) = stats[b * stats_frame_stride + 2c .. + 1]
 *     v = v * weight[c] + bias[c]                  when weight is given (bias then has to be)
 *     v = relu(v)                                  when relu_inner != 0
 *     when res is given:
 *         u = res
 *         u = (u - mean_r) * rstd_r                when res_stats is given; (mean_r, rstd_r) likewise from res_stats
 *         u = u * res_weight[c] + res_bias[c]      when res_weight is given (only with res_stats; res_bias then has to be)
 *         v = relu(u + v)
 *     out = v                                      bfloat16: rounded once, to nearest even; NaN stays NaN
 * relu(v) = v < 0 ? 0 : v, so a NaN stays NaN as torch's does; the sign of a zero result is not specified.  With neither
 * res nor relu_inner the call is the plain norm.  ResidualBlock.forward is three such launches around its convolutions:
 * norm1 + relu;  norm2 + relu + (x +) + relu with res = x; and, where the block has a downsample path, the same with
 * res = the 1x1 convolution's output and res_stats = norm3's.
 * stats_frame_stride and res_stats_frame_stride are 2*C or 0; with 0 one set [C][2] serves every frame, which is how a
 * BatchNorm2d in eval mode goes through the same kernel: the caller fills (running_mean, 1 / sqrt(running_var + eps)) once.
 * out may be x itself or res itself (the same pointer and frame stride: every cell is read before it is written, by the lane
 * that writes it) and must not overlap any other argument, nor x or res in any other way.
 *
 * Both calls are stream-ordered and never synchronise.  Refused before anything is launched, with no output byte touched:
 * a NULL x, stats or out; B, C, H or W <= 0; a frame stride below C*H*W; a stats stride other than 0 or 2*C; a dtype other
 * than the two; eps not finite or <= 0; weight without bias or the reverse (res_weight and res_bias likewise); res_stats or
 * res_weight without res, res_weight without res_stats (VPPX_E_INVALID_ARG); H*W above 2^31 - 1, or more planes and cells
 * than one launch takes (VPPX_E_UNSUPPORTED). */
int vppx_raft_norm_stats_dt_dev(const void *x, int64_t x_frame_stride, int B, int C, int H, int W, double eps, float *stats,
                                int dtype, vppx_ctx *ctx);
int vppx_raft_norm_apply_dt_dev(const void *x, int64_t x_frame_stride, const float *stats, int64_t stats_frame_stride,
                                const float *weight, const float *bias, int relu_inner, const void *res,
                                int64_t res_frame_stride, const float *res_stats, int64_t res_stats_frame_stride,
                                const float *res_weight, const float *res_bias, void *out, int64_t out_frame_stride, int B,
                                int C, int H, int W, int dtype, vppx_ctx *ctx);
/* Workgroups the statistics call gives to each of `planes` = B*C planes of `cells_per_plane` = H*W cells, without a context
 * (host arithmetic only): 1 where the planes alone fill the device or a plane is small, more for few large planes.  At
 * least 1 for any arguments, never above 64, not decreasing in cells_per_plane and not increasing in planes. */
int vppx_norm_stats_pieces(int64_t planes, int64_t cells_per_plane);
/* ---- The 3x3 convolution on the matrix cores, and a ConvGRU as assemble + two launches -------------------------------
 * (models/raft_stereo/update.py:19-32).  nn.Conv2d(Cin, Cout, 3, padding=1), stride 1: cross-correlation as torch computes
 * it, not a flipped kernel, with +0 outside the map.  Like the encoders' glue above, these calls take the context LAST and
 * no struct, for the reason given there.
 *
 * Input.  The channel concatenation of up to two sources: x0 [B,C0,H,W] and x1 [B,C1,H,W] (C1 = 0: absent, x1 is not
 * read), Cin = C0 + C1.  Addressing is that of the update block's calls: frame b of a tensor starts b * its frame stride
 * cells behind the pointer and is contiguous, so convq reads cat([r*h, x]) as x0 = the r*h buffer and x1 = hx[:, C:]
 * without a copy.  dtype (VppxDtype) is the storage of every activation and output of a call.
 *     acc[b][m][y][x] = sum over c < Cin, dy < 3, dx < 3 of w[m][c][dy][dx] * in[b][c][y + dy - 1][x + dx - 1]
 * VPPX_DT_F32:  the float32 matrix path (v_mfma_f32_16x16x4_f32): every product exact float32 arithmetic, float32
 *     accumulation.  It runs at 1/16 of the bfloat16 rate of the matrix cores: correct, and the slow one.
 * VPPX_DT_BF16: v_mfma_f32_16x16x32_bf16.  Activations are bfloat16 as stored; the weights are rounded to bfloat16 once, to
 *     nearest even, when they are packed, which is what torch does under autocast; every product is then exact in float32
 *     and the accumulation is float32.
 * The sum starts at +0 and runs in an order the library chooses and this header does not promise, as in
 * vppx_raft_corr_fused_dt_dev; tests/_gruconv_ref.py derives how far any float32 evaluation in any order can lie from
 * the exact value.  K = 9*Cin is padded to the matrix instruction's step by rows whose activation AND weight are both +0:
 * no cell of the input ever meets a padding weight.  A NaN input cell reaches the 3x3 pixels around it, in every output
 * channel of its frame, and no other cell; an infinite one likewise (NaN or infinite there).
 *
 * Packing.  packed is an opaque device buffer of vppx_raft_conv3x3_packed_bytes(Cout, Cin, dtype) bytes (0 for a shape or
 * dtype that is not built), 16-byte aligned, written once per module by vppx_raft_conv3x3_pack_dev from weight
 * [Cout][Cin][3][3] float32 (torch's layout, contiguous, device) and bias [Cout] float32 or NULL (no bias: +0).  Its layout
 * is the library's; only its size is promised, and that a buffer packed for one (Cout, Cin, dtype) serves any B, H, W and
 * any split of Cin into C0 + C1.  For the zr call the weights are convz's rows followed by convr's, [2C][Cin][3][3], and
 * the biases likewise.
 *
 * Epilogues, each operation one correctly rounded float32 operation, v = acc + bias[m]:
 *   conv3x3:  out[b][m] = relu ? (v < 0 ? 0 : v) : v         (a NaN stays NaN; the sign of a zero result is not specified)
 *   gru_zr (Cout = 2C):   m <  C:  z[b][m]    = sigmoid(v + cz[b][m])
 *                         m >= C:  rh[b][m-C] = sigmoid(v + cr[b][m-C]) * h[b][m-C]
 *       rh is a [B,C,H,W] buffer of its own.  It CANNOT be the h part of the hx the call reads, which is where
 *       vppx_raft_gru_reset_dt_dev writes r*h: other workgroups are still reading those cells as the halo of their tiles.
 *       z, rh must not overlap any input.
 *   gru_q (Cout = C):     q = tanh(v + cq[b][m]);   out[b][m] = ((1 - z[b][m]) * h[b][m]) + (z[b][m] * q)
 *       z is the buffer the zr call wrote.  out may be h itself (the same pointer and frame stride): each cell of h is read
 *       only by the lane that writes it, and the convolution reads x0 and x1, never h.  out must not overlap x0, x1, cq or z.
 * sigmoid and tanh are those of the update block's glue above, the same formulas and the same device expf.  The
 * convolution's sum enters the gate in float32 and is not rounded to bfloat16 first: one rounding fewer per gate input than
 * the path through vppx_raft_gru_reset_dt_dev / _update_dt_dev.  A bfloat16 result is the float32 result rounded once, to
 * nearest even (NaN stays NaN).  cz, cr, cq go in as channel slices of the [B,3C,H,W] context tensor by their stride.
 *
 * No pointer but packed has to be aligned beyond its cell: outputs (and the gates' inputs) move 16 bytes at a time where every
 * pointer of the epilogue is 16-byte aligned and every frame stride of it and W are whole numbers of 16 bytes, and cell by
 * cell otherwise, with the same bits.  All calls are stream-ordered, never synchronise and allocate nothing.
 * Refused before anything is launched, with no output byte touched: a NULL weight, packed, x0, x1 with C1 > 0, cz, cr, cq, h,
 * z, rh or out; B, H, W, C0, Cout or C <= 0, C1 < 0; a frame stride below its tensor's size; a dtype other than the two; a
 * packed pointer that is not 16-byte aligned (VPPX_E_INVALID_ARG); C0, C1, Cout or C not a multiple of 16, C0 + C1 above
 * VPPX_CONV_MAX_CIN, Cout (2C for the zr call) above VPPX_CONV_MAX_COUT, B*H*W above 2^31 - 1 (VPPX_E_UNSUPPORTED).
 *
 * The update block's other convolutions (update.py:34-42 FlowHead, :81,83,86 convc2 / convf2 / conv, :113-116 mask and the
 * `.25 *` of :141): vppx_raft_conv_* is the plain call above with three things more.  Everything said above about the input,
 * the two dtypes, the order of the sum, the padding of K, the alignment routes, stream order and "allocates nothing" holds.
 *   Cout is any count from 1 to VPPX_CONV_MAX_COUT.  The packing pads the output channels to the next multiple of 16 with rows
 *     whose weights and bias are +0 and writes every byte of the buffer; the call stores channel m only where m < Cout, so out
 *     may be channels [0, Cout) of a wider tensor and no cell behind channel Cout - 1 of a frame is written.  For Cout % 16 == 0
 *     and ksize 3 the size and the packed bytes are those of vppx_raft_conv3x3_*.
 *   ksize is 3 (as above) or 1: nn.Conv2d(Cin, Cout, 1), weight [Cout][Cin][1][1], acc[b][m][y][x] = sum over c < Cin of
 *     w[m][c] * in[b][c][y][x].  Nothing outside the map is read.  A NaN or infinite input cell reaches its own pixel, in every
 *     output channel of its frame, and no other cell; for ksize 3 the 3x3 pixels around it, as above.
 *   scale:  v = acc + bias[m];  relu: v = v < 0 ? 0 : v (a NaN stays NaN);  out[b][m] = v * scale, one correctly rounded float32
 *     multiplication; scale == 1.0f gives the bits of the call without it.  A bfloat16 result is that float32 product rounded
 *     once, to nearest even.  For a power of two (the mask's .25) this equals rounding v and then the product, as torch does,
 *     except where the product is subnormal.
 * For ksize 3, Cout % 16 == 0 and scale 1.0f, vppx_raft_conv_dt_dev gives the bits of vppx_raft_conv3x3_dt_dev.
 * vppx_raft_conv_packed_bytes is 0 for what is not built: Cout outside 1 .. VPPX_CONV_MAX_COUT, Cin not a positive multiple of
 * 16 up to VPPX_CONV_MAX_CIN, a ksize other than 1 and 3, a dtype other than the two.
 * Refused before anything is launched, with no output byte touched: a NULL weight, packed, x0, x1 with C1 > 0 or out; B, H, W, C0
 * or Cout <= 0, C1 < 0; a frame stride below its tensor's size; a scale that is not finite; a dtype other than the two; a packed
 * pointer that is not 16-byte aligned (VPPX_E_INVALID_ARG); a ksize other than 1 and 3, C0 or C1 not a multiple of 16, C0 + C1
 * above VPPX_CONV_MAX_CIN, Cout above VPPX_CONV_MAX_COUT, B*H*W above 2^31 - 1 or more tiles than one launch takes
 * (VPPX_E_UNSUPPORTED).
 *
 * The encoders' convolutions (models/raft_stereo/extractor.py:10-11 ResidualBlock conv1 / conv2, :45 downsample, :149 and :231
 * the basic encoder's conv2, :240,247 the output heads): vppx_raft_conv_strided_dt_dev is vppx_raft_conv_dt_dev with `stride`
 * behind ksize, nn.Conv2d(Cin, Cout, ksize, stride=stride, padding=ksize / 2) for stride 1 or 2.  H, W are the INPUT's: x0 is
 * [B,C0,H,W], x1 [B,C1,H,W], and their frame strides are checked against C0 * H * W and C1 * H * W.  The output is
 *     out [B,Cout,Ho,Wo],   Ho = (H - 1) / stride + 1,   Wo = (W - 1) / stride + 1      (integer division)
 * which is torch's size for ksize 3 with padding 1 and for ksize 1 with padding 0; out's frame stride is checked against
 * Cout * Ho * Wo.  The tile count and its refusal, the 16-byte and the cell-by-cell route (now decided by Wo) are in output pixels.
 *     ksize 3:  acc[b][m][y][x] = sum over c < Cin, dy < 3, dx < 3 of w[m][c][dy][dx] * in[b][c][stride*y + dy - 1][stride*x + dx - 1]
 *     ksize 1:  acc[b][m][y][x] = sum over c < Cin of w[m][c] * in[b][c][stride*y][stride*x]
 * with +0 outside the map: at stride 2 output pixel (y, x) sums input rows 2y-1 .. 2y+1 and columns 2x-1 .. 2x+1.  For an odd H
 * (W) the last window reaches one row (column) past the map, for an even one it does not.  The 1x1 at stride 2 reads the
 * cells (2y, 2x) only: nothing at an odd row or column is read.  Bias, ReLU, scale and the rounding are those of
 * vppx_raft_conv_dt_dev, and stride == 1 gives its bits.  The packed weights are exactly those of stride 1: a buffer packed by
 * vppx_raft_conv_pack_dev for (Cout, Cin, ksize, dtype) serves either stride.
 * NaN rule: a NaN (or infinite) input cell reaches exactly the output pixels whose window holds it, in every output channel of
 * its frame, and no other cell.  For ksize 3 at stride 2 a cell (r, c) lies in the windows of rows (r-1)/2 .. (r+1)/2 rounded
 * inwards: one output row for an even r, two for an odd r (one where the second would be row Ho), and columns likewise.  For
 * ksize 1 at stride 2 a NaN at an odd row or column reaches nothing.
 * Refused before anything is launched, with no output byte touched: a stride other than 1 and 2 (VPPX_E_UNSUPPORTED), and
 * everything vppx_raft_conv_dt_dev refuses, with the same code. */
#define VPPX_CONV_MAX_CIN 512
#define VPPX_CONV_MAX_COUT 256
size_t vppx_raft_conv3x3_packed_bytes(int Cout, int Cin, int dtype);
int vppx_raft_conv3x3_pack_dev(const float *weight, const float *bias, int Cout, int Cin, int dtype, void *packed, vppx_ctx *ctx);
int vppx_raft_conv3x3_dt_dev(const void *x0, int64_t x0_frame_stride, int C0, const void *x1, int64_t x1_frame_stride, int C1,
                             const void *packed, int Cout, int B, int H, int W, int relu, void *out, int64_t out_frame_stride,
                             int dtype, vppx_ctx *ctx);
int vppx_raft_gru_zr_dt_dev(const void *x0, int64_t x0_frame_stride, int C0, const void *x1, int64_t x1_frame_stride, int C1,
                            const void *packed_zr, const void *cz, int64_t cz_frame_stride, const void *cr, int64_t cr_frame_stride,
                            const void *h, int64_t h_frame_stride, void *z, int64_t z_frame_stride, void *rh,
                            int64_t rh_frame_stride, int B, int C, int H, int W, int dtype, vppx_ctx *ctx);
int vppx_raft_gru_q_dt_dev(const void *x0, int64_t x0_frame_stride, int C0, const void *x1, int64_t x1_frame_stride, int C1,
                           const void *packed_q, const void *cq, int64_t cq_frame_stride, const void *z, int64_t z_frame_stride,
                           const void *h, int64_t h_frame_stride, void *out, int64_t out_frame_stride, int B, int C, int H, int W,
                           int dtype, vppx_ctx *ctx);
size_t vppx_raft_conv_packed_bytes(int Cout, int Cin, int ksize, int dtype);
int vppx_raft_conv_pack_dev(const float *weight, const float *bias, int Cout, int Cin, int ksize, int dtype, void *packed, vppx_ctx *ctx);
int vppx_raft_conv_dt_dev(const void *x0, int64_t x0_frame_stride, int C0, const void *x1, int64_t x1_frame_stride, int C1,
                          const void *packed, int Cout, int ksize, int B, int H, int W, int relu, float scale, void *out,
                          int64_t out_frame_stride, int dtype, vppx_ctx *ctx);
int vppx_raft_conv_strided_dt_dev(const void *x0, int64_t x0_frame_stride, int C0, const void *x1, int64_t x1_frame_stride, int C1,
                                  const void *packed, int Cout, int ksize, int stride, int B, int H, int W, int relu, float scale,
                                  void *out, int64_t out_frame_stride, int dtype, vppx_ctx *ctx);
/* ---- PSMNet's feature_extraction (models/psmnet/submodule.py:131-253) on the convolution kernel ----------------------------
 * Its convolutions are convbn groups, Conv2d(bias=False) -> BatchNorm2d [-> ReLU], and BasicBlocks, out = conv2bn(conv1bn_relu(x));
 * out += x (:60-84).  A frozen BatchNorm folds into the weights and the bias on the host (vppstereo_amd/_convs.py), the sum with x
 * goes into the epilogue, layer4's dilation into the kernel:
 * vppx_conv2d_dt_dev is vppx_raft_conv_strided_dt_dev with `dilation` behind stride and a residual in front of relu:
 *     nn.Conv2d(Cin, Cout, ksize, stride=stride, padding=dilation * (ksize / 2), dilation=dilation)
 *     ksize 3:  acc[b][m][y][x] = sum over c < Cin, dy < 3, dx < 3 of
 *                                 w[m][c][dy][dx] * in[b][c][stride*y + dilation*(dy - 1)][stride*x + dilation*(dx - 1)]
 * with +0 outside the map; the output's size is that of the strided call for either dilation.  Built: dilation 1 with everything
 * the strided call takes, and dilation 2 at stride 1; at dilation 2 a ksize of 1 is the 1x1 convolution itself, the bits of
 * dilation 1.  The packed weights are those of vppx_raft_conv_pack_dev: one buffer serves every stride and dilation.
 * The epilogue, every step one correctly rounded float32 operation:
 *     v = acc + bias[m];   res: v = v + res[b][m][y][x] (a bfloat16 cell widened);   relu: v = v < 0 ? 0 : v (a NaN stays NaN);
 *     out[b][m][y][x] = v * scale
 * res is NULL or [B,Cout,Ho,Wo] with a frame stride of its own, at least Cout*Ho*Wo; it moves 16 bytes at a time under the rule
 * the gates' inputs follow above (its pointer and frame stride count with out's), cell by cell otherwise, with the same bits.
 * out may be res itself, the same pointer and frame stride: each cell is read by the lane that writes it.  out and res must not
 * overlap x0 or x1.  With res == NULL and dilation 1 the call gives the bits of vppx_raft_conv_strided_dt_dev.
 * NaN rule at dilation 2, ksize 3: a NaN (or infinite) input cell (r, c) reaches exactly the output pixels (r + 2i, c + 2j), i, j
 * in -1 .. 1, that lie inside the map, in every output channel of its frame, and nothing else: not (r +- 1, c +- 1).  A NaN in
 * res stays in its cell.
 * Refused before anything is launched, with no output byte touched, in this order where several apply: everything
 * vppx_raft_conv_strided_dt_dev refuses, with its code; behind the stride's refusal, a dilation other than 1 and 2, or
 * dilation 2 at stride 2 (VPPX_E_UNSUPPORTED); among the frame strides, a res_frame_stride below Cout*Ho*Wo
 * (VPPX_E_INVALID_ARG), in front of out's. */
int vppx_conv2d_dt_dev(const void *x0, int64_t x0_frame_stride, int C0, const void *x1, int64_t x1_frame_stride, int C1,
                       const void *packed, int Cout, int ksize, int stride, int dilation, int B, int H, int W,
                       const void *res, int64_t res_frame_stride, int relu, float scale,
                       void *out, int64_t out_frame_stride, int dtype, vppx_ctx *ctx);
/* ---- PSMNet's stride-1 3-D convolutions (models/psmnet/psmnet.py:24-36, 93-128) on the convolution kernel --------------------
 * vppx_conv3d_dt_dev is nn.Conv3d(Cin, Cout, 3, stride=1, padding=1) with the epilogue of vppx_conv2d_dt_dev:
 *     x [B,Cin,D,H,W], frames x_frame_stride cells apart (at least Cin*D*H*W), every frame contiguous;  out [B,Cout,D,H,W]
 *     acc[b][m][d][y][x] = sum over c < Cin, dz < 3, dy < 3, dx < 3 of w[m][c][dz][dy][dx] * x[b][c][d + dz - 1][y + dy - 1][x + dx - 1]
 * with +0 outside the volume, in depth as in the map: plane -1 and plane D of a frame are +0, never a plane of frame b - 1 or
 * b + 1.  The sum runs on the 3x3 kernel over 3*Cin pseudo-channels (channel dz*Cin + c is plane d + dz - 1 of channel c):
 * K = 27*Cin float32 accumulations from +0 in an order the library chooses, padded as above by rows whose activation and weight
 * are both +0; the two dtypes, the exact bfloat16 products and the float32 accumulation are those of the 3x3 call.
 * The epilogue, every step one correctly rounded float32 operation:
 *     v = acc + bias[m];   res: v = v + res[b][m][d][y][x] (a bfloat16 cell widened);   relu: v = v < 0 ? 0 : v (a NaN stays NaN);
 *     out[b][m][d][y][x] = v * scale          (scale == 1.0f changes no bit; a bfloat16 result is the float32 one rounded once)
 * res is NULL or [B,Cout,D,H,W] with a frame stride of its own; out may be res itself (the same pointer and frame stride): each
 * cell is read by the lane that writes it.  out and res must not overlap x.  Channel m is stored only where m < Cout: out may
 * be channels [0, Cout) of a wider tensor.  The 16-byte and the cell-by-cell route are decided as for the 3x3 call (pointers and
 * frame strides of res and out, and W) and give the same bits.  Stream-ordered, never synchronises, allocates nothing.
 * Packing.  vppx_conv3d_pack_dev writes vppx_conv3d_packed_bytes(Cout, Cin, dtype) bytes from weight [Cout][Cin][3][3][3]
 * float32 (torch's layout, contiguous, device) and bias [Cout] or NULL: exactly the bytes vppx_raft_conv_pack_dev writes for
 * the [Cout][3*Cin][3][3] weight w2[m][dz*Cin + c][dy][dx] = w[m][c][dz][dy][dx].  The size is 0, and the pack refuses, for
 * Cin not a positive multiple of 16, 3*Cin above VPPX_CONV_MAX_CIN, Cout outside 1 .. VPPX_CONV_MAX_COUT, a dtype other than
 * the two.  One buffer serves any B, D, H, W.
 * NaN rule: a NaN (or infinite) input cell (b, c, z, r, q) reaches exactly the up to 27 output cells (z + i, r + j, q + k), i, j,
 * k in -1 .. 1, that lie inside the volume, in every output channel of batch frame b, and nothing else: in particular nothing
 * in frame b - 1 or b + 1.  A NaN in res stays in its cell.
 * Every batch frame's result has the bits of the B = 1 call on that frame.
 * Refused before anything is launched, with no output byte touched, in this order where several apply: a NULL out or a scale
 * that is not finite; a NULL x or packed; B, D, H or W <= 0; a dtype other than the two (VPPX_E_INVALID_ARG); H*W or D*H*W
 * above 2^31 - 1 (VPPX_E_UNSUPPORTED); Cin or Cout <= 0 (VPPX_E_INVALID_ARG); Cin not a multiple of 16, 3*Cin above
 * VPPX_CONV_MAX_CIN, Cout above VPPX_CONV_MAX_COUT (VPPX_E_UNSUPPORTED); a packed pointer that is not 16-byte aligned; an
 * x_frame_stride below Cin*D*H*W (VPPX_E_INVALID_ARG); B*D*H*W above 2^31 - 1 (VPPX_E_UNSUPPORTED); a res_frame_stride, then an
 * out_frame_stride, below Cout*D*H*W (VPPX_E_INVALID_ARG); more tiles than one launch takes (VPPX_E_UNSUPPORTED).
 * Out of scope: Conv3d at stride 2 and ConvTranspose3d (the hourglasses' conv1, conv3, conv5, conv6) stay in torch. */
size_t vppx_conv3d_packed_bytes(int Cout, int Cin, int dtype);
int vppx_conv3d_pack_dev(const float *weight, const float *bias, int Cout, int Cin, int dtype, void *packed, vppx_ctx *ctx);
int vppx_conv3d_dt_dev(const void *x, int64_t x_frame_stride, int Cin, const void *packed, int Cout, int B, int D, int H, int W,
                       const void *res, int64_t res_frame_stride, int relu, float scale, void *out, int64_t out_frame_stride,
                       int dtype, vppx_ctx *ctx);
/* The pyramid pooling's average pools (submodule.py:149-171): every level in one launch, x [B,C,H,W] read once.
 *     level i:  nn.AvgPool2d((k, k), stride=(k, k)), k = ks[i];   outs[i] is [B,C,H/k,W/k] (integer division), contiguous
 *     out[y][x] = (the float32 sum of the k*k cells x[k*y .. k*y+k-1][k*x .. k*x+k-1]) / (float)(k*k), one correctly rounded division
 * The order of the sum is the library's (spp_kernels.hip states it): it depends on (H, W, ks) alone, never on the dispatch, so a
 * call gives the same bits run after run; tests/_psm_ref.py bounds any order.  Rows and columns behind (H/k)*k and (W/k)*k are
 * not read for that level: a NaN there reaches nothing of it; a NaN inside reaches the one cell whose window holds it.
 * ks and outs are HOST arrays of n_levels entries, outs of device pointers; the levels need not nest or be ordered, and no
 * pointer has to be aligned beyond its cell.  Stream-ordered, never synchronises, allocates nothing.
 * Refused before anything is launched, with no output byte touched: a NULL x, ks, outs or outs[i]; B, C, H or W <= 0; n_levels
 * outside 1 .. VPPX_SPP_MAX_LEVELS; a k < 1; H/k or W/k == 0; x_frame_stride below C*H*W; a dtype other than the two
 * (VPPX_E_INVALID_ARG); a k above VPPX_SPP_MAX_K, or B*C above 2^31 - 1 (VPPX_E_UNSUPPORTED). */
#define VPPX_SPP_MAX_LEVELS 4
#define VPPX_SPP_MAX_K 64
int vppx_psm_spp_pool_dt_dev(const void *x, int64_t x_frame_stride, int B, int C, int H, int W, int n_levels,
                             const int *ks /* host */, void *const *outs /* host array of device pointers */, int dtype, vppx_ctx *ctx);
/* vppx_raft_gru_assemble_dt_dev (above) into a channel slice: the destination's frames lie out_frame_stride cells apart, at
 * least sum C_i * H * W; channels 0 .. sum C_i - 1 of each frame are written and no cell behind them.  The same kernel, the same
 * arithmetic and the same 16-byte rule, out_frame_stride in hx_channels*H*W's place: with out_frame_stride = hx_channels*H*W
 * the bits of vppx_raft_gru_assemble_dt_dev.  PSMNet's four upsampled branches are one such call of four VPPX_GRU_INTERP sources
 * into channels 192 .. 319 of the 320-channel feature buffer (submodule.py:243-250).  Refusals: those of the assemble call, an
 * out_frame_stride below sum C_i * H * W in the place of hx_channels below sum C_i.  The context comes last, as in every call
 * of the flat form. */
int vppx_raft_gru_assemble_strided_dt_dev(const VppxGruSource *sources, int n_sources, int B, int H, int W, void *out,
                                          int64_t out_frame_stride, int dtype, vppx_ctx *ctx);
/* Disparity payload decoders (dataloaders/frame_utils.py): KITTI uint16 PNG samples -> disp = v/256
 * float32 + valid = disp>0 uint8 (readDispKITTI :66-69, valid may be NULL); PFM payload (after the
 * text header) -> float32 [H,W(,3)] flipped upside-down, byte-swapped if big-endian (readPFM :34-64).
 * Inflating the PNG stays with the host's image library. */
int vppx_kitti_disp_decode_dev(vppx_ctx *ctx, const uint16_t *png_u16, int64_t n, float *disp, uint8_t *valid);
/* Whole PNG FILES decoded on the device (chunk walk, zlib/DEFLATE inflate, scanline unfiltering), one wave per
 * file of a batch: `blob` (device) holds n_files files back to back -- no alignment or padding is required of it --,
 * `offsets` (HOST, n_files + 1 entries) their byte ranges.  Non-interlaced gray 8/16 bit (C = 1) or RGB 8 bit (C = 3), all files H x W.  disp/valid (C = 1):
 * disp = sample * scale as float32 (scale 1/256 = readDispKITTI frame_utils.py:66-69, 1 = readDispMidd :71-74),
 * valid = disp > 0; out_u8 [n,H,W,C]: the 8-bit samples of an 8-bit file (a 16-bit file asked into out_u8 is refused with
 * status 3).  status (device int32 [n_files], may be NULL): 0 = ok,
 * 1 signature, 2 IHDR, 3 unsupported format (palette, alpha, gray below 8 bits, RGB of 16 bits, interlaced, 16 bits into out_u8),
 * 4 size mismatch (IHDR against H, W, C; a stream that inflates to more or fewer bytes than H scanlines), 5 bad stream (zlib
 * header: CM other than 8, FDICT, FCHECK; block type 3; stored LEN / NLEN; a distance beyond the start of the output), 6 bad
 * Huffman code (code lengths over-subscribed or incomplete, a repeat with nothing to repeat or past the last length, no
 * end-of-block code, HLIT above 286 or HDIST above 30, a symbol without meaning, a length without a distance code; an incomplete
 * code is accepted only as a single code of one bit, as zlib does: a lone distance code of two bits is refused), 7 bad filter,
 * 8 truncated, 9 Adler-32 of the inflated stream does not match the one in the file (chunk CRCs are not verified); a file that
 * fails before its first scanline leaves its outputs untouched, one that fails later has written the scanlines decoded so far.
 * Scanlines up to 16 KB (1 + W * bytes per pixel). */
int vppx_png_decode_dev(vppx_ctx *ctx, int n_files, const uint8_t *blob, const int64_t *offsets, int H, int W, int C,
                        float scale, float *disp, uint8_t *valid, uint8_t *out_u8, int32_t *status);
int vppx_pfm_decode_dev(vppx_ctx *ctx, const uint8_t *raw, int H, int W, int channels, int little_endian, float *out);

/* ---- occlusion heuristic (filter.py:246-292): hints -> g_occ mask ------------------------- */
int vppx_occlusion_heuristic_host(vppx_ctx *ctx, int B, int H, int W, const float *hints, int rx, int ry, double l,
                                  double g, double th_conf, double th_filter, uint8_t *conf_out);
int vppx_occlusion_heuristic_dev(vppx_ctx *ctx, int B, int H, int W, const float *hints, int rx, int ry, double l,
                                 double g, double th_conf, double th_filter, uint8_t *conf_out);
/* Both elements of the reference's return value (filter.py:283-292): dmap_out (float32 [B,H,W], may be NULL) = the
 * filtered hints un-warped and passed through interpolate_disparity(dmap, 3), conf_out = the mask.  The reference's
 * interpolate_disparity indexes dmap[y, x +- 1] without a bounds test (filter.py:223,229): column -1 wraps to W-1, column W
 * is the first pixel of the next row; the read past the end of the last row is undefined there and taken as 0 here. */
int vppx_occlusion_heuristic_full_host(vppx_ctx *ctx, int B, int H, int W, const float *hints, int rx, int ry, double l,
                                       double g, double th_conf, double th_filter, float *dmap_out, uint8_t *conf_out);
int vppx_occlusion_heuristic_full_dev(vppx_ctx *ctx, int B, int H, int W, const float *hints, int rx, int ry, double l,
                                      double g, double th_conf, double th_filter, float *dmap_out, uint8_t *conf_out);

/* hipGraph replay of vppx_vpp_rsgm_dev: with the mode on, the second call with identical
 * shapes, parameters, pointers and stream is stream-captured and later identical calls launch the instantiated
 * graph (one launch instead of ~40: matters for small batches).  Needs a non-default stream (vppx_set_stream);
 * where capture is not possible the call silently stays on the eager path.  vppx_graph_replays counts launches.
 * A call made while stage timing is on (vppx_enable_stage_timing) runs eagerly beside the graph: it is no replay, and it neither
 * becomes the call a later one is compared with nor destroys the graph, so the identical call behind it is replayed again. */
int vppx_set_graph_mode(vppx_ctx *ctx, int enable);
long vppx_graph_replays(vppx_ctx *ctx);

/* ---- measurement helpers (bench.py) ------------------------------------------------------- */
/* The timing helpers RE-LAUNCH the aggregation stage of the last rSGM-bearing call (vppx_rsgm_dev, vppx_vpp_rsgm_dev,
 * vppx_occ_vpp_rsgm_*) on the library-owned gray / census images, the penalties and the geometry that call left, into the
 * call's own path volumes, and time the launches with a hipEvent pair on the context's stream; they synchronise.  They change
 * nothing a later call can see: its outputs, vppx_uses_vert, vppx_fused_pixels_per_wave, vppx_last_call_parts, the graph of
 * vppx_set_graph_mode (a helper between two replays costs none) and the list of vppx_last_routes (a re-launch names only
 * kernels the call named) are what they would be without the helper.  A call that ran in parts is re-launched on its LAST
 * part, a call split over VPPX_SUBSTREAMS on the part of child 0.  Every launch enters the rings of vppx_agg_kernel_ms /
 * vppx_we_kernel_ms like a call's.
 * vppx_time_aggregate: `iters` back-to-back runs of the whole stage -- the one launch of all eight paths, or, in the fused
 * layout, the lock-step launches and the W/E launch in the call's order and on the call's streams; average ms per run in
 * *ms_out.
 * Refused, with nothing launched and *ms_out untouched: iters <= 0 or a NULL ms_out (the message names the argument), no such
 * call on this context yet, or a 3-channel vppx_aggregate_img since, which writes its gray image where the call's lay and may
 * move that buffer ("call vppx_rsgm_dev first"), all three VPPX_E_INVALID_ARG; a guided last call -- its launch reads hint
 * rows that stage entries overwrite, and the census layout would be another kernel on other volumes (VPPX_E_UNSUPPORTED).
 * After vppx_aggregate / vppx_aggregate_img with one channel, which overwrite the penalty table only, the helper uploads the
 * call's table again (so a graph of that call, which holds no upload of its own, is replayed by the next identical call). */
int vppx_time_aggregate(vppx_ctx *ctx, int iters, float *ms_out);
/* Average duration (ms) of the aggregation kernel -- the eight-path launch, or the lock-step launches of the fused layout
 * (one pair around both where a batch runs as whole rounds + a remainder) -- over the last `last_n` of them on this context,
 * from hipEvent pairs recorded around every one on its launch stream (ring of 64: at most 64 are averaged).  *n_used is
 * min(last_n, launches since the last reset, 64): a call adds one per PART it ran in, a timing helper one per iteration, a
 * graph replay none (event records stay out of a captured graph), a guided call none.  A context made with VPPX_SUBSTREAMS > 1
 * answers with child 0's ring, which holds child 0's share of every split call and nothing of a call too small to split
 * (fewer than 2 frames per child).  Call after synchronising.  last_n <= 0 resets the launch counter.  n_used may be NULL. */
int vppx_agg_kernel_ms(vppx_ctx *ctx, int last_n, float *avg_ms, int *n_used);
/* The same for the W/E launch of the fused layout (the other launch of its aggregation stage; also when it makes E only,
 * next to the route "wsum<12>").  The eight-path layout never adds to it. */
int vppx_we_kernel_ms(vppx_ctx *ctx, int last_n, float *avg_ms, int *n_used);
/* Frames per launch that the timing helpers re-run: the whole batch, the LAST part of a call that ran in parts, child 0's
 * share of a call split over VPPX_SUBSTREAMS; 0 where they would refuse with "call vppx_rsgm_dev first". */
int vppx_time_aggregate_frames(vppx_ctx *ctx);
/* vppx_time_aggregate for one of the two kinds of launch of the FUSED layout (vppx_uses_vert() == 3): part 1 = the W/E launch
 * alone (we12<..>, or paths<..dirs=11 | 10>), on the context's stream even where the call ran it next to an under-filled
 * lock-step launch; part 2 = the lock-step launches alone (vert3<..> / vert4<..>), the same launches of the same kernels as
 * the call's.  Part 1 adds to the ring of vppx_we_kernel_ms only, part 2 to that of vppx_agg_kernel_ms only.  (The band
 * layout of VPPX_VERT=1: its line launch / its band launches.)  Refusals as vppx_time_aggregate's; and a part other than 1 or
 * 2 (VPPX_E_INVALID_ARG), and the eight-path layout, whose single launch has no parts (VPPX_E_UNSUPPORTED, the message names
 * the layout). */
int vppx_time_aggregate_part(vppx_ctx *ctx, int iters, int part, float *ms_out);
/* The kernel instantiations the LAST timing-helper call launched (vppx_time_aggregate, vppx_time_aggregate_part), as
 * vppx_last_routes lists a call's: distinct names in launch order, same names, same calling convention.  Empty before the
 * first helper and after one that refused.  Asked of a context whose last call was split over VPPX_SUBSTREAMS, it answers for
 * child 0, where the helpers re-launch. */
int vppx_timing_last_routes(vppx_ctx *ctx, char *buf, int n);
/* Aggregation layout of the last fused / rsgm call: 0 = all 8 paths in the line-parallel kernel, 3 = N/NW/NE and
 * S/SW/SE fused three at a time in the lock-step kernel + W and E line-parallel (register-window kernel for D = 128 / 192 /
 * 256) (default for D = 128 / 192 from 3 frames per call on; environment VPPX_VERT = 0 / 3 forces a layout), 1 = the round-1
 * band-marching experiment
 * (VPPX_VERT = 1).  All layouts give identical results. */
int vppx_uses_vert(vppx_ctx *ctx);
/* Which fused kernel the last call used: 16 = sgm_vert4_kernel (16 pixels per wave, 4 lanes per pixel: the default once a
 * batch fills the chip with its groups), 8 = sgm_vert3_kernel (8 lanes per pixel; VPPX_V3_PPW = 8 / 16 forces one),
 * 0 = the last call did not use the fused layout. */
int vppx_fused_pixels_per_wave(vppx_ctx *ctx);
/* Batch quantum of the fused layout for H x W frames and this disparity range: the number of frames that fills the GPU
 * with one whole round of (frame, pass) groups of the lock-step kernel -- batches that are a multiple of it leave no
 * part-filled last round (540 x 960 x 192 on an MI355X: 16; 375 x 1242 x 192: 12).  0 when the fused layout does not apply
 * to this device or shape.  A scheduling hint only: every batch size gives the same results.  (Runs a one-time device
 * probe on first use; not inside a graph capture.) */
int vppx_batch_quantum(vppx_ctx *ctx, int H, int W, int dmax);
/* Number of consecutive parts the last fused call (vppx_vpp_rsgm_dev / vppx_occ_vpp_rsgm_dev) ran as: a batch larger than
 * one round of the lock-step kernel runs as parts of one round each (VPPX_CHUNK); 1 = the whole batch at once. */
int vppx_last_call_parts(vppx_ctx *ctx);
/* Pieces per line of the last, part-filled layer of waves in the last launch of the W / E register-window kernel (its lines are
 * cut into 2..8 pieces that hand the path state on through memory when that evens out the SIMDs' load); 1 = nothing was cut. */
int vppx_we_last_pieces(vppx_ctx *ctx);
/* The same for the last launch of the W + sum + WTA kernel (the route "wsum<12>" of vppx_last_routes). */
int vppx_wsum_last_pieces(vppx_ctx *ctx);
/* The default rule of that route, without a context: 1 when an unguided launch of B padded Hp x Wp frames in the fused layout
 * (vppx_uses_vert() == 3) with largest penalty p2max takes it on a device of `nsimd` SIMDs (4 per compute unit): dmax = 192,
 * 3 * (24 + p2max) <= 255 and B * Hp / 4 >= 2 * nsimd.  VPPX_VARIANT=wsum / nowsum override it. */
int vppx_wsum_default_route(int B, int Hp, int Wp, int dmax, int p2max, int nsimd);
/* The kernel instantiations the last rSGM-bearing call launched, as a comma-separated list in launch order, each one once
 * (a call that ran in parts lists the union over its parts), e.g. "paths<8,24,exact,guided,u16,dirs=ff>,
 * sum_lr<12,u16,8,64,spare,nosw4,general,16,partw>".  Names: paths<lanes per pixel,disparities per lane,exact|partial,
 * census|dsi|guided,u8|u16,dirs=ff|11> (line-parallel kernel, 8 paths or W + E), we12<DPL> (W / E register-window
 * kernel), vert3<DPL> / vert4<DPL> (fused vertical kernel, 8 / 16 pixels per wave), vert_band<DPL>, sum_lr<DPL,u8|u16,
 * volumes,T,spare|nospare,sw4|nosw4,fast|general,lanes per pixel,fullw|partw> and sum_trap<DPL,T,spare|nospare> (fused
 * sum / WTA), sum_wta<DPL,exact|partial,u8|u16> + wta_right_t (materialised sum, then the right view).  Commas inside
 * <> belong to a name.  The list is cleared at the entry of vppx_rsgm_dev / _host, vppx_vpp_rsgm_dev, vppx_occ_vpp_rsgm_*
 * (guided or not) and vppx_aggregate / _img; the timing helpers re-launch the last call's aggregation and add to it -- kernels
 * the call named already, so the list stays the call's (vppx_timing_last_routes has the helper's own).  A
 * graph replay (vppx_set_graph_mode) launches nothing from the host and reports the routes of the call it captured.  The
 * children of VPPX_SUBSTREAMS keep lists of their own, which are not merged: a call split over them lists nothing.
 * Writes at most n - 1 characters and a NUL to buf (buf may be NULL when n == 0); returns the length of the whole list. */
int vppx_last_routes(vppx_ctx *ctx, char *buf, int n);
/* The same for the front stage -- the occlusion heuristic, the virtual pattern projection and the bilateral filling -- in a
 * list of its own (vppx_last_routes never names these): every kernel the last call launched from that stage, with its
 * template arguments and the host decisions that select a code path inside it, distinct names in launch order.  Names:
 * occ_warp4 | occ_warp, occ_test<NJ,PT> (NJ = 1..4 window rounds of 64 positions, 0 = any; PT = 4 or, next to a sum / WTA
 * kernel that leaves less than 12 KB of LDS, 2 pixels per thread), occ_dmap (the filtered map); hint_range,
 * compact<dist|plain>, rowscan, rand; l_bits<NW,ROWS> (first L pass: window width 1 / 3 / 5 / 7, rows per block 4 or 1),
 * l_heavy<NW> (second L pass: pixels with an occluded hint in their window), l_wide (wsize >= 9); r_rows<u16|u32,mode=M,seg=N>,
 * one entry per launch (mode 1 = apply, 2 = build the hint lists, 3 = both; N column segments per row);
 * vpp_order<independent|late|inplace,side|main> (the launch order: the sides do not depend on each other / the original right
 * image is kept and the L passes that replay it come last / R is patterned in place, so mode 2 comes first and mode 1 last; and
 * whether the L side ran on the side stream); maxdist_wave | maxdist_lds | maxdist_global; gray_ctx, bilateral_fill.
 * The list is cleared at the entry of every call that can launch one of these kernels: vppx_vpp_dev / _host and the two
 * vppx_virtual_projection_scan_* built on them, vppx_occlusion_heuristic_* (all four), vppx_vpp_rsgm_dev, vppx_occ_vpp_rsgm_*
 * (guided, scaled, evaluating or not, _dev and _host) and with them every batch of a frame stream.  A call that runs in parts
 * lists the union over its parts.  A graph replay (vppx_set_graph_mode) reports what the captured call recorded.  The children
 * of VPPX_SUBSTREAMS keep lists of their own, which are not merged: a call split over them lists nothing, as in
 * vppx_last_routes.  Same calling convention: writes at most n - 1 characters and a NUL to buf (buf may be NULL when n == 0),
 * returns the length of the whole list; VPPX_E_INVALID_ARG on a bad buffer. */
int vppx_last_front_routes(vppx_ctx *ctx, char *buf, int n);
/* Per-stage hipEvent timing of the last vppx_vpp_rsgm_dev/vppx_rsgm_dev call when stage
 * timing is enabled: fills ms[0..n) and returns the number of stages; names via
 * vppx_stage_name(i).  While it is on, a call runs without cross-call pipelining, sub-streams and graph replay, with the same
 * results; every stage closes with a mark (an event on the launch stream) and a stage's time is the sum of the intervals that
 * end in its marks, over all parts of a call that ran in parts.  The table of marks grows with the call: none is dropped,
 * however many parts (vppx_stage_marks counts them).  A stage the call did not run is 0. */
int vppx_enable_stage_timing(vppx_ctx *ctx, int enable);
int vppx_get_stage_ms(vppx_ctx *ctx, float *ms, int max_n);
/* Marks the last call recorded while stage timing was on, over all its parts (9 to 11 per part of vppx_vpp_rsgm_dev: one more
 * with the occlusion heuristic, one more where the sum falls back to sum_wta + wta_right_t; one fewer with
 * VPPX_METHOD_MAXDIST, which draws no random numbers and so has no vpp_rand stage); 0 while
 * it is off. */
int vppx_stage_marks(vppx_ctx *ctx);
const char *vppx_stage_name(int i);

/* ---- environment ------------------------------------------------------------------------------
 * Every variable the shipped library reads, all of them ONCE, in vppx_create (nothing else calls getenv; `tools/build_exp.sh`
 * measurement builds add VPPX_V3_IGNORE_LOST, VPPX_EXP_WE_TRACE and the other VPPX_EXP_*, tools/ only):
 *   VPPX_VERT           aggregation layout: -1 / unset = by shape, 0 = eight line-parallel paths, 3 = fused layout whenever the
 *                       shape allows it, 1 = the round-1 band-marching kernel (vppx_uses_vert)
 *   VPPX_CHUNK          parts of a fused call: unset = one round of the lock-step kernel each, 0 = whole batches, n = n frames
 *   VPPX_SUBSTREAMS     1..4 child contexts that share a batch (default 1)
 *   VPPX_V3_PPW         8 / 16: pixels per wave of the fused vertical kernel (default: by batch size)
 *   VPPX_V3_TIMEOUT_MS  bound of one neighbour wait of the lock-step kernel (default 250)
 *   VPPX_V3_SPIN_LIMIT  the same bound in polls (tests force the give-up path with 1; default unbounded)
 *   VPPX_GUIDED_PART_MB budget in MiB of the eight u16 path volumes of one part of a guided batch (default 49152, i.e. 48 GiB;
 *                       tests set a few MiB to run small batches in parts)
 *   VPPX_VARIANT        comma-separated tokens that select alternative kernels with identical results, each run by
 *                       tests/test_gpu_variants.py: sum_general, sum_gl8, sum_trap0, sum_trap1 (fused sum / WTA kernel), gw4, gw8,
 *                       gw16 (lanes per pixel of the line-parallel kernel), we_line (W / E on the line-parallel kernel), we_after (W / E never next to
 *                       an under-filled lock-step launch), we_lq0, we_lq1 (W / E kernel: left-view operands per step / per quad of steps), we_whole (W / E kernel: no line of the last layer of waves is cut into pieces; tests: we_layer=N takes a layer to be N waves, we_mute makes every later piece give up waiting and compute its line from the start, we_stale fills the
 *                       hand-off records of every cut launch with the dword the next launch's flags accept),
 *                       wsum (the W + sum + WTA kernel -- W path, sum and both WTAs in one pass, the W/E launch makes E only -- for every
 *                       fused D = 192 launch of 3 frames or more; by default it takes those whose line quads fill two layers of waves),
 *                       nowsum (never: W/E, then the sum / WTA kernel; tests: wsum_cut=K cuts every line of that kernel into K pieces),
 *                       tests only: fs_fail_submit=K (the K-th batch submit of a frame stream fails with "injected submit failure",
 *                       before it enqueues anything), fs_fail_from=K (every submit from the K-th on),
 *                       maxdist_lds, maxdist_global (one-wave maxDistance kernels) */

#ifdef __cplusplus
}
#endif
#endif /* VPPX_H */
