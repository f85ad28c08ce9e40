// vppx_internal.h -- shared declarations of libvppx.so (gfx950 only; not installed).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string>
#include <vector>

#include "../../include/vppx.h"

typedef uint8_t u8;
typedef uint16_t u16;
typedef uint32_t u32;
typedef uint64_t u64;

// ---------------------------------------------------------------------------------------
// error plumbing
// ---------------------------------------------------------------------------------------
void vppx_set_error(const char *fmt, ...);

#define VPPX_HIP(call)                                                                              \
    do {                                                                                            \
        hipError_t e_ = (call);                                                                     \
        if (e_ != hipSuccess) {                                                                     \
            vppx_set_error("%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__); \
            return VPPX_E_HIP;                                                                      \
        }                                                                                           \
    } while (0)

#define VPPX_CHECK_LAUNCH() VPPX_HIP(hipGetLastError())

// Every entry point runs with the context's device current and puts the caller's device back on return
// (a torch process may hold contexts on several GPUs; the library must not change its current device).
struct DevGuard {
    int prev = -1;
    bool changed = false;
    explicit DevGuard(int dev)
    {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != dev) changed = (hipSetDevice(dev) == hipSuccess);
    }
    ~DevGuard()
    {
        if (changed && prev >= 0) (void)hipSetDevice(prev);
    }
};

#define VPPX_ENTER(ctx)                                                                                              \
    if (!(ctx)) { vppx_set_error("context is NULL (vppx_create failed? there is no CPU fallback)"); return VPPX_E_NO_DEVICE; } \
    DevGuard dev_guard_((ctx)->device);                                                                                  \
    /* cross-call pipelining: any entry point but the two pipelined ones may queue work that touches the front stage's   \
       buffers, so the next front stage must wait for the whole launch stream again (PIPE_KEEP restores the flag) */      \
    const bool pipe_had_agg_done_ = (ctx)->have_agg_done;                                                                 \
    (ctx)->have_agg_done = false;                                                                                         \
    (void)pipe_had_agg_done_
#define VPPX_PIPE_KEEP(ctx) (ctx)->have_agg_done = pipe_had_agg_done_

// ---------------------------------------------------------------------------------------
// workspace arena: named, grow-only device buffers owned by the context.  Everything the
// pipeline needs between kernels lives in HBM for the lifetime of the context (288 GB:
// batches are sized so that whole cost-path volumes stay resident).
// ---------------------------------------------------------------------------------------
struct DevBuf {
    void *p = nullptr;
    size_t cap = 0;
};

enum WsSlot {
    WS_HINT_X = 0,   // compacted hint rows
    WS_HINT_REC,
    WS_HINT_DENSE,
    WS_HINT_BITS,    // per row: which scan positions hold a hint (u64 words)
    WS_RCNT,
    WS_FILLED_G,
    WS_GRAY_CTX,
    WS_RLIST,
    WS_LWORK,        // L pixels whose window holds an occluded hint (second pass of the sparse L mapping)
    WS_LWORK_CNT,
    WS_ROW_COUNT,
    WS_ROW_DRAWS,
    WS_ROW_BASE,
    WS_FRAME_TOT,
    WS_HINT_RANGE,   // [B] {dmin, dmax} of every frame's own hints (use_distance_patch with per_frame_range)
    WS_RAND,
    WS_SEEDS,
    WS_VPP_L,        // scratch copies of the pair (fused path)
    WS_VPP_R,
    WS_VPP_LSRC,
    WS_OCC_ZERO,
    WS_GRAY_L,       // padded gray images
    WS_GRAY_LV,
    WS_GRAY_RV,
    WS_CENSUS_L,
    WS_CENSUS_R,
    WS_GRAY_L2,      // second set of the images the aggregation reads (pipelined calls alternate: front_end)
    WS_CENSUS_L2,
    WS_CENSUS_R2,
    WS_PATHS,        // 8 per-path L volumes
    WS_S,            // aggregated volume (u16)
    WS_SV,           // per-pass sums of the vertical/diagonal paths (band-marching kernel)
    WS_VSTATE,
    WS_VMIN,
    WS_V3ERR,        // device-side copy of the fused kernel's error word (void_if_lost_kernel)
    WS_WE_TRACE,     // experiment builds: per-block wall-clock trace of the W/E kernel
    WS_WE_HAND,      // W/E kernel: path states handed from piece to piece of the split tail lines + a flag per line (We12Args)
    WS_WSUM_HAND,    // W + sum + WTA kernel: a fixed flag region, then the records handed from piece to piece of its tail lines (WsumArgs)
    WS_DSI,          // materialised cost volume (stage API), or the hint pixels' cost rows of a guided call
    WS_GUIDED_MAP,   // guided call: row index of every padded pixel (+ the row counter behind it)
    WS_DISP_L0,
    WS_DISP_L1,
    WS_DISP_R0,
    WS_DISP_R1,
    WS_FD8,
    WS_SPK_ROOTS,    // per tile of the speckle filter: its tile-local roots
    WS_SPK_NROOTS,
    WS_ROW_ANY,      // per row of the result: does it hold a valid disparity (column pass of _interpolate_background)
    WS_LABEL,
    WS_LCOUNT,
    WS_P2LUT,
    WS_STAGE_A,      // host-API staging (device copies of host arrays)
    WS_STAGE_B,
    WS_STAGE_C,
    WS_STAGE_D,
    WS_STAGE_E,
    WS_STAGE_F,
    WS_OCC_OMAP,
    WS_OCC_OUT,       // the mask of the fused occlusion + VPP + rSGM call (library-owned: the front stage never writes caller memory)
    WS_OCC_TMP,       // unwarp scratch of the occlusion heuristic (its own slot: with vppx_set_pipeline it runs next to the previous call's speckle filter, which owns WS_LABEL)
    WS_NHINTS,
    WS_HANDOFF_H,    // hints / valid at feature resolution (hand-off kernels)
    WS_HANDOFF_V,
    WS_PNG_RAW,      // concatenated IDAT payloads of a batch of PNG files (the zlib streams)
    WS_PNG_OFFS,
    WS_PNG_STATUS,
    WS_SCALE_L0,     // --iscale: the scaled pair, hints and validhints of a scaled call (two sets: pipelined calls alternate)
    WS_SCALE_R0,
    WS_SCALE_G0,
    WS_SCALE_V0,
    WS_SCALE_L1,
    WS_SCALE_R1,
    WS_SCALE_G1,
    WS_SCALE_V1,
    WS_SCALE_DSMALL, // the disparities at the scaled shape, when the caller does not want them (the restore kernel reads them)
    WS_SCALE_TAB,    // index / weight tables of the resize and the restore (scale_tables)
    WS_SCALE_HOST_D, // vppx_occ_vpp_rsgm_scaled_host: device copy of disp_small
    WS_METRICS_PART, // guided_metrics: one partial record per (frame, block) (metrics_kernels.hip)
    WS_METRICS_OUT,  // vppx_guided_metrics_host: device copy of the result records
    WS_VIZ_PART,     // vppx_finite_max_dev: one partial maximum per (frame, block) (viz_kernels.hip)
    WS_VIZ_OUT,      // the _host renderers: device copy of the pictures
    WS_VIZ_AUX,      // vppx_colorize_host: device copies of max_val and the colour table
    WS_SAMPLE_G0,    // sampled hints and mask of a sampling call (sample_kernels.hip; two sets: pipelined calls alternate)
    WS_SAMPLE_V0,
    WS_SAMPLE_G1,
    WS_SAMPLE_V1,
    WS_NORM_PART,    // vppx_raft_norm_stats: two float64 sums per (plane, piece) of a split plane (norm_kernels.hip)
    WS_NUM
};

#define VPPX_MAX_DEVICES 64 // power of two: per-device one-time initialisations are indexed by device id

struct vppx_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    bool legacy_stream = false;    // launches go to the legacy default (null) stream: vppx_set_stream_legacy
    hipStream_t stream2 = nullptr; // side stream: horizontal paths overlap the vertical band launches
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    // sub-contexts: the fused batched call splits its frames over `nsub` child contexts (own stream
    // and arena) so that latency-bound stages of one part overlap bandwidth-bound stages of another
    int nsub = 1;   // VPPX_SUBSTREAMS=2 overlaps two half batches (+3 %; off by default so that profiles and
                    // the in-process kernel timing see the same, un-overlapped launches)
    vppx_ctx *sub[4] = {nullptr, nullptr, nullptr, nullptr};
    hipEvent_t sub_done[4] = {nullptr, nullptr, nullptr, nullptr};
    bool is_child = false;
    // Environment, read ONCE in vppx_create (include/vppx.h lists every variable the shipped library reads): VPPX_CHUNK and
    // the VPPX_VARIANT tokens, which select kernels that give identical results (tests/test_gpu_variants.py runs each)
    struct Knobs {
        int chunk = -1;       // VPPX_CHUNK: -1 parts of one lock-step round (default), 0 whole batches, n parts of n frames
        int sum_general = 0;  // "sum_general": the general WTA decision code of the fused sum / WTA kernel (round 1)
        int gw = 0;           // "gw4" / "gw8" / "gw16": lanes per pixel of the line-parallel aggregation kernel
        int maxdist = 0;      // "maxdist_lds" (1): one wave per chain, rows in LDS; "maxdist_global" (2): in place in global memory
        int we_line = 0;      // "we_line": W / E of the fused layout on the line-parallel kernel instead of sgm_we12_kernel
        int sum_gl8 = 0;      // "sum_gl8": 8 lanes per pixel in the fused sum / WTA kernel (D = 128 / 192)
        int sum_trap = 2;     // D = 256, fused layout: trapezoid ring with spare slots; "sum_trap1": without them; "sum_trap0": uniform ring, 32-pixel rounds
        int we_next = 1;      // W/E next to an under-filled lock-step launch (rsgm_vert3_plan); "we_after": always behind it
        int we_split = 1;     // W/E kernel: the lines of the last, part-filled layer of waves are cut into pieces; "we_whole": every line whole
        int we_layer = 0;     // "we_layer=N" (tests): the W/E launcher takes a layer of waves to be N instead of the device's SIMD count
        int we_mute = 0;      // "we_mute" (tests): pieces do not publish their state: every later piece takes the give-up path
        int we_stale = 0;     // "we_stale" (tests): behind every cut W/E launch its record area is filled with the dword the NEXT launch's flags accept
        int fs_fail_submit = 0; // "fs_fail_submit=K" (tests): the K-th batch submit of a frame stream fails before it enqueues anything
        int fs_fail_from = 0;   // "fs_fail_from=K" (tests): ... and every submit from the K-th on
        int we_lq = -1;       // "we_lq0" / "we_lq1": the W/E kernel's left-view operand loads (per step / per quad of steps); default by launch
        int wsum = -1;        // "wsum": the W + sum + WTA kernel for every fused D = 192 launch of 3 frames or more; "nowsum": never; default by shape
        int wsum_cut = 0;     // "wsum_cut=K" (tests): that kernel cuts EVERY line into K pieces
        int sum_blocks = 0;   // (experiment builds) "sum_blocks=N": forced number of blocks of the sum / WTA kernel
        unsigned long long guided_part_bytes = 48ull << 30; // VPPX_GUIDED_PART_MB: volume budget of one part of a guided batch
    } knobs;
    // kernel instantiations the last rSGM-bearing call launched, distinct, in launch order (vppx_last_routes): cleared at the
    // entry of every such call, appended to by the launchers where the template arguments are known
    std::vector<std::string> routes;
    std::vector<std::string> graph_routes; // those of the captured call: a replay launches nothing from the host and restores them
    // the names the LAST timing helper launched (vppx_timing_last_routes): its launches are noted here as well as in `routes`
    std::vector<std::string> timing_routes;
    bool timing_run = false;       // a timing helper is re-launching the aggregation (route_note)
    // the same for the front stage (occlusion heuristic, VPP, bilateral filling: vppx_last_front_routes), a list of its own so
    // that vppx_last_routes keeps its content: cleared at the entry of every call that can launch a front-stage kernel
    std::vector<std::string> front_routes;
    std::vector<std::string> graph_front_routes;
    bool front_routes_keep = false; // one-shot: the host wrapper has queued the heuristic already, vpp_rsgm_entry adds to the list
    int use_vert = -1;             // VPPX_VERT: -1 pick by shape (default), 0 eight line-parallel paths, 1 band marching, 3 fused vertical kernel
    int last_vert = 0;             // what the last aggregation used (vppx_uses_vert)
    int last_parts = 1;            // parts the last fused call ran as (vppx_last_call_parts)
#ifdef VPPX_EXPERIMENT
    std::string exp_we_trace;      // VPPX_EXP_WE_TRACE: file the W/E kernel's per-block trace of the last launch goes to (tools/we_trace.py)
#endif
    unsigned we_serial = 0;        // launch serial of the W/E kernel's hand-off flags
    void *we_hand_seen = nullptr;  // the hand-off buffer as it was last cleared (launch_we12)
    size_t we_hand_cap = 0;
    int we_hand_geom[3] = {0, 0, 0}; // (ntail, pieces, DPL) of the last cut W/E launch: where its flags lie (We12Args)
    int we_last_pieces = 1;        // pieces per tail line of the last W/E launch (vppx_we_last_pieces)
    void *wsum_hand_seen = nullptr; // the W + sum + WTA kernel's hand-off buffer as its flag region was last cleared (rsgm_launch_wsum)
    size_t wsum_hand_cap = 0;
    int wsum_last_pieces = 1;      // pieces per tail line of its last launch
    bool wsum_route = false;       // the running call's aggregation leaves W to that kernel (run_aggregation)
    bool we_beside_vert = false;   // the W/E launch being queued runs next to a lock-step launch (run_aggregation)
    unsigned long long *draws_dst = nullptr; // device [B]: where the fused call leaves every frame's draw count (set per call by a frame stream)
    int last_sum_nvol = 0;         // volumes the last fused sum / WTA launch added (4: fused layout, 8: eight paths) and its
    int last_sum_D = 0, last_sum_B = 0; // shape: what a pipelined front stage has to fit next to (vpp_rsgm_one)
    // cross-call pipelining (vppx_set_pipeline): the front stage of a fused call (occlusion heuristic, VPP, pad + gray,
    // census) runs on stream_front, after the PREVIOUS call's aggregation, i.e. under that call's sum / WTA and post kernels
    bool pipeline = false;
    bool front_active = false;     // ctx->stream currently is stream_front
    bool pipe_call = false;        // the running vpp_rsgm call is pipelined (record ev_agg_done after its aggregation)
    bool have_agg_done = false;
    bool pipe_early = false;       // this pipelined call lets the next front stage start next to its aggregation (few frames per call)
    int pipe_parity = 0;           // which set of gray / census images the next pipelined call writes
    bool pipe_mid = false;         // the next front stage starts behind the fused vertical kernel, next to W/E (VPPX_VARIANT=pipe_mid of an experiment build)
    bool agg_done_recorded = false; // ... and this call's aggregation has recorded ev_agg_done already
    const u8 *last_gl = nullptr;   // the images the last call aggregated from (timing helpers)
    const u32 *last_cl = nullptr, *last_cr = nullptr;
    hipStream_t stream_front = nullptr, main_saved = nullptr;
    hipEvent_t ev_agg_done = nullptr, ev_front_done = nullptr, ev_inputs_auto = nullptr;
    void *inputs_ev = nullptr;     // caller's "inputs of the next call are ready" event (vppx_inputs_ready_event), one-shot
    // front-stage results the caller asked for (mask, patterned pair): computed into library-owned buffers on the front
    // stream, copied to the caller's memory on the LAUNCH stream once it has waited for the front stage
    struct PipeCopy { void *dst; const void *src; size_t bytes; bool early; } pipe_copy[3]; // early: ready at ev_occ_done already
    int n_pipe_copy = 0;
    hipEvent_t ev_occ_done = nullptr;   // front stream: the occlusion mask of the call is complete
    bool occ_done_recorded = false;
    // LDS a front-stage kernel can count on per CU next to the sum / WTA kernel of the previous part or call, which holds
    // one block per CU: 160 KB minus that kernel's tile ring (36 KB at D <= 192, 7 KB at D = 256).  Kernels pick block
    // shapes that fit; set by the pipelined fused entry, "everything" otherwise.
    size_t front_lds_budget = 64 * 1024;
    void *xbuf_last = nullptr;          // exchange records of the last lock-step launch ...
    size_t xbuf_last_bytes = 0;
    bool xbuf_cleared = false;          // ... and whether a clear of them is already queued on the launch stream behind it
    unsigned *vert3_err = nullptr; // pinned host word the fused vertical kernel sets (to its launch serial) when a wave gave up waiting
    bool vert3_broken = false;     // the XCD / residency probe failed on this device: the context never uses the fused layout
    int vert3_rest = 0;            // aggregations left on the line-parallel layout after a lost lock step, before the fused layout is tried again
    int vert3_backoff = 64;        // ... doubling with every loss (64, 128, ... 4096)
    bool vert3_probed = false;     // rsgm_vert3_probe has run on this context's device
    long lockstep_failures = 0;    // fused launches that reported a lost lock step (vppx_lockstep_failures)
    unsigned lockstep_last_serial = 0; // serial of the launch the last report was about
    struct V3Caps {                // what rsgm_vert3_probe found out about the device and this build of the kernels
        bool ok = false;
        int nxcd = 0, cus_per_xcd = 0;
        int blocks_per_cu[4] = {0, 0, 0, 0}; // D = 64, 128, 192, 256 (8 pixels per wave)
        int blocks_per_cu16[4] = {0, 0, 0, 0}; // the same for 16 pixels per wave (sgm_vert4_kernel)
        int ppw = 0;               // VPPX_V3_PPW: pixels per wave of the fused kernel at D = 192 (0 = by batch size, 8, 16)
        int wall_khz = 100000;     // rate of s_memrealtime
        int timeout_ms = 250;      // bound of one wait for a neighbour (VPPX_V3_TIMEOUT_MS)
        unsigned spin_limit = 0;   // polls per wait, 0 = unbounded (VPPX_V3_SPIN_LIMIT: tests force the give-up path with 1)
        unsigned serial = 0;       // serial of the last fused launch
        int last_ppw = 0;          // pixels per wave of the last fused launch (8: sgm_vert3_kernel, 16: sgm_vert4_kernel)
        bool ignore_lost = false;  // VPPX_V3_IGNORE_LOST (experiment builds only): measurement runs with forced give-ups (results void) carry on
    } v3;
    DevBuf ws[WS_NUM];
    std::string devname;
    // libc-like stream state of the single-frame scans
    uint32_t rnd_seed = 1;
    uint64_t rnd_consumed = 0;
    // last rsgm geometry (for vppx_time_aggregate)
    int last_B = 0, last_Hp = 0, last_Wp = 0, last_D = 0;
    VppxRsgmParams last_rp;
    bool have_last = false;
    bool last_guided = false;      // ... and it was a guided aggregation (rows and row map in WS_DSI / WS_GUIDED_MAP): the helpers refuse
    // hipEvent pairs around the aggregation kernel of the most recent pipeline calls (ring), recorded
    // on the launch stream: vppx_agg_kernel_ms averages them after the caller's synchronize
    static const int AGG_RING = 64;
    hipEvent_t agg_ev[2][AGG_RING];
    bool agg_ev_created = false;
    long agg_calls = 0;
    // the same around the W/E launch of the fused layout (vppx_we_kernel_ms): its in-step duration differs from what a
    // back-to-back re-launch measures, so both are on record
    hipEvent_t we_ev[2][AGG_RING];
    long we_calls = 0;
    // P2 look-up table: host copy kept alive for the asynchronous upload, re-sent only when the penalties change
    u16 lut_host[256];
    bool lut_valid = false;
    int lut_p2min = 0, lut_gamma = 0, lut_maxp2 = 0;
    float lut_alpha = 0.f;
    // hipGraph replay of the fused call (vppx_set_graph_mode): the second identical call
    // (same shapes, parameters and pointers) is stream-captured, later ones launch the instantiated graph
    struct GraphKey {
        int B, H, W, C;
        VppxVppParams vp;
        VppxRsgmParams rp;
        const void *ptr[9];
        const void *eval_ptr[4]; // gt, validgt, metrics_out, errormap of an evaluating call
        int eval_scale[4];       // gt_scale, Hg, Wg, validgt is bytes
        VppxOccParams op;
        int has_op;
        void *stream;
        unsigned long ws_gen;
    };
    bool graph_mode = false, capturing = false;
    bool have_gkey = false, have_lastkey = false;
    GraphKey gkey, lastkey;
    hipGraphExec_t gexec = nullptr;
    unsigned long ws_gen = 0;      // bumped whenever a workspace buffer is (re)allocated
    long graph_replays = 0, graph_captures = 0;
    // stage timing
    bool stage_timing = false;
    bool stage_append = false;     // the running call is a later part of a split batch: its marks follow the earlier parts'
    int n_stages = 0;              // marks of the last call (vppx_stage_marks); ev holds n_stages + 1 events or more
    std::vector<hipEvent_t> ev;    // grows with the marks: a call in many parts loses none (stage_mark)
    std::vector<int> stage_id;
    size_t total_bytes = 0;
    std::vector<long long> png_offs_host; // kept alive for the asynchronous upload
    // --iscale / --oscale (vppx_occ_vpp_rsgm_scaled_*): shape the tables in WS_SCALE_TAB were computed for, and which set of
    // scaled buffers the next pipelined scaled call writes
    int scale_key[6] = {0, 0, 0, 0, 0, 0};
    const void *scale_tab_at = nullptr;
    int last_scale_set = -1, last_sample_set = -1; // the set of scaled / sampled maps the last such call wrote: vppx_last_front_sets
    long scale_tab_builds = 0;     // times the tables were (re)built: vppx_scale_table_builds
    int scale_parity = 0;
    hipEvent_t ev_scaled = nullptr;
    // hint sampling in front of a fused call (vppx_occ_vpp_rsgm_sampled_dev): which set of sampled maps the next pipelined call writes
    int sample_parity = 0;
    hipEvent_t ev_sampled = nullptr;
};

// ---------------------------------------------------------------------------------------
// One fused hot-path call (VPP -> rSGM; scaled, evaluated, sampled on request) as every layer between an entry point and the
// kernels takes it.  The entry points and a frame stream fill one and hand it down; no layer spells the bundle out again.
// ---------------------------------------------------------------------------------------
struct HotCall {
    enum Layer { PLAIN, SCALED, EVAL, SAMPLED };
    Layer layer = PLAIN;                   // where the call enters: that layer's checks and messages come first
    // parameter blocks
    const VppxOccParams *op = nullptr;     // NULL: no occlusion heuristic on the way; g_occ (may be NULL) is the caller's mask
    VppxVppParams vp = {};                 // (by value: frames() moves the seed)
    bool vp_null = false;                  // the caller passed none: refused together with the layer's other NULL arguments
    const VppxRsgmParams *rp = nullptr;
    const VppxScaleParams *sp = nullptr;   // NULL: unscaled.  Below the scaled layer always NULL: the call at the shape it runs at
    const VppxEvalParams *ep = nullptr;    // NULL: gt_scale 1
    const VppxSampleParams *smp = nullptr;
    int B = 0, H = 0, W = 0, C = 0;
    // inputs
    const u8 *left = nullptr, *right = nullptr;
    const float *g = nullptr;              // the hints (a sampled call: NULL, they are sampled on the way)
    const u8 *g_occ = nullptr;
    const float *validhints = nullptr;     // not NULL: --guided
    // outputs
    u8 *conf_out = nullptr, *l_vpp = nullptr, *r_vpp = nullptr;
    float *disp_out = nullptr, *disp_small = nullptr;
    // evaluation request (metrics_out != NULL below the evaluating layer: guided_metrics of the result, queued behind it)
    const float *gt = nullptr;
    const void *validgt = nullptr;         // float32, or one byte per pixel (valid_is_u8: an evaluating frame stream's ring)
    int valid_is_u8 = 0;
    VppxMetrics *metrics_out = nullptr;
    float *errormap = nullptr;
    int gt_scale = 1, Hg = 0, Wg = 0;      // (resolved by the evaluating layer: ep's scale and the shape of gt / validgt)
    // sampling request
    const float *src = nullptr;            // NULL: gt / validgt are the source
    const void *validsrc = nullptr;        // float32, or one byte per pixel (vsrc_is_u8: a sampling frame stream's ring)
    int vsrc_is_u8 = 0, guided = 0;
    float *hints_out = nullptr, *validhints_out = nullptr;

    // Frames lo .. lo + nb of a call at its run shape (sp == NULL: every plane but gt / validgt has the frame shape H x W): the one
    // place that knows which planes are per frame and what their strides are.  NULL stays NULL; frame f keeps srand(seed + f).
    HotCall frames(int lo, int nb) const
    {
        HotCall p = *this;
        const size_t px = (size_t)lo * H * W, gpx = (size_t)lo * Hg * Wg;
        auto at = [](auto *ptr, size_t n) { return ptr ? ptr + n : nullptr; };
        p.B = nb;
        p.vp.seed = vp.seed + (uint32_t)lo;
        p.left = at(left, px * C);
        p.right = at(right, px * C);
        p.g = at(g, px);
        p.g_occ = at(g_occ, px);
        p.validhints = at(validhints, px);
        p.conf_out = at(conf_out, px);
        p.l_vpp = at(l_vpp, px * C);
        p.r_vpp = at(r_vpp, px * C);
        p.disp_out = at(disp_out, px);
        p.disp_small = at(disp_small, px);
        p.gt = at(gt, gpx);
        p.validgt = at((const u8 *)validgt, gpx * (valid_is_u8 ? 1 : sizeof(float)));
        p.metrics_out = at(metrics_out, (size_t)lo);
        p.errormap = at(errormap, px);
        p.src = at(src, px);
        p.validsrc = at((const u8 *)validsrc, px * (vsrc_is_u8 ? 1 : sizeof(float)));
        p.hints_out = at(hints_out, px);
        p.validhints_out = at(validhints_out, px);
        return p;
    }
};
// vppx_api.hip, for vppx_fstream.hip: the call (every entry point's route is one of these layers), an earlier call's lost lock
// step, and the argument checks of the fused entry points for a stream to make when it is CREATED
int vppx_hot_call_internal(vppx_ctx *ctx, const HotCall &c);
int vppx_lockstep_check_internal(vppx_ctx *ctx);
int vppx_check_hot_path_args_internal(const VppxVppParams *vp, const VppxRsgmParams *rp, int B, int H, int W, int C);

int ws_reserve(vppx_ctx *ctx, WsSlot s, size_t bytes, void **out);
template <typename T>
static inline int ws_get(vppx_ctx *ctx, WsSlot s, size_t count, T **out)
{
    void *p = nullptr;
    int rc = ws_reserve(ctx, s, count * sizeof(T), &p);
    *out = (T *)p;
    return rc;
}

// vppx_last_routes: the launcher of a kernel instantiation records it (printf-style name, e.g. "we12<12>"); duplicates are dropped
void route_note(vppx_ctx *ctx, const char *fmt, ...) __attribute__((format(printf, 2, 3)));
static inline void routes_reset(vppx_ctx *ctx) { ctx->routes.clear(); }
// vppx_last_front_routes: the launchers of vpp_kernels.hip record every kernel they launch and the host decisions that select a
// code path inside one (e.g. "r_rows<u16,mode=3,seg=2>"); duplicates are dropped
void front_route_note(vppx_ctx *ctx, const char *fmt, ...) __attribute__((format(printf, 2, 3)));
static inline void front_routes_reset(vppx_ctx *ctx) { ctx->front_routes.clear(); }

// stage ids (vppx_stage_name)
enum {
    ST_VPP_COMPACT = 0,
    ST_VPP_RAND,
    ST_VPP_APPLY,
    ST_PAD_GRAY,
    ST_CENSUS,
    ST_AGGREGATE,
    ST_SUM_WTA,
    ST_WTA_RIGHT,
    ST_MEDIAN_INTERP,
    ST_POST,
    ST_OCC,
    ST_COUNT
};
void stage_begin(vppx_ctx *ctx);
void stage_mark(vppx_ctx *ctx, int stage);

// ---------------------------------------------------------------------------------------
// kernel launchers (defined in the .hip files)
// ---------------------------------------------------------------------------------------
struct RsgmGeom {
    int B, H, W, C;      // input frames
    int Hp, Wp;          // padded to multiples of 16 (rsgm.py:254-256)
    int pad_l, pad_r, pad_t, pad_b;
    int D;
};

// rsgm_kernels.hip
int rsgm_launch_pad_gray(vppx_ctx *ctx, const RsgmGeom &g, const u8 *img, u8 *gray);
int rsgm_launch_pad_gray_n(vppx_ctx *ctx, const RsgmGeom &g, int n, const u8 *const *img, u8 *const *gray); // n <= 3, one launch
int rsgm_launch_to_nchw(vppx_ctx *ctx, int B, int H, int W, int C, int mult, const u8 *src, void *dst, int bf16);
int rsgm_launch_census(vppx_ctx *ctx, int B, int Hp, int Wp, const u8 *gray, u32 *census);
int rsgm_launch_pad_gray_census(vppx_ctx *ctx, const RsgmGeom &g, const u8 *left, const u8 *left_vpp, const u8 *right_vpp, u8 *gray_left,
                                u32 *census_l, u32 *census_r); // the three of the fused pipeline in one launch
int rsgm_launch_census_n(vppx_ctx *ctx, int B, int Hp, int Wp, int n, const u8 *const *gray, u32 *const *census); // n <= 2
int rsgm_launch_cost(vppx_ctx *ctx, int B, int Hp, int Wp, int D, const u32 *cl, const u32 *cr, u16 *dsi);
// --guided: the hint pixels' re-weighted cost rows (u16 [n][D], n <= B*H*W, never read back by the host) and the row index
// of every padded pixel (int [B][Hp][Wp], -1 = not a hint pixel); *count is the row counter (cleared by the launch)
int rsgm_launch_guided_rows(vppx_ctx *ctx, const RsgmGeom &g, const u32 *cl, const u32 *cr, const float *hints,
                            const float *valid, int *gmap, u16 *rows, u32 *count);
// 8-path aggregation.  Cost source: census pair (dsi == nullptr), a materialised u16 DSI, or (gmap != nullptr) the census
// pair with the guided rows `dsi` of rsgm_launch_guided_rows at the pixels gmap names.
// Writes the 8 per-path volumes into `paths` (element size elem_bytes = 1 or 2).
int rsgm_launch_paths(vppx_ctx *ctx, int B, int Hp, int Wp, int D, const u8 *gray, const u32 *cl, const u32 *cr,
                      const u16 *dsi, const u16 *p2lut, int p1, void *paths, int elem_bytes, int dir_mask,
                      const int *gmap = nullptr);
// band-marching vertical/diagonal paths (3 summed paths per pass, one byte per cell)
int rsgm_vert3_probe(vppx_ctx *ctx, u32 *scratch_dev, bool *ok);
bool rsgm_vert3_supported(int B, int Hp, int Wp, int D, int maxp2);
bool rsgm_vert3_fits(const vppx_ctx *ctx, int B, int Wp, int D);
int rsgm_vert3_frames_per_round(const vppx_ctx *ctx, int Wp, int D);
bool rsgm_vert3_wide(const vppx_ctx *ctx, int B, int Wp, int D);
size_t rsgm_vert3_xbuf_bytes(int B, int Wp, int D);
void rsgm_vert3_plan(const vppx_ctx *ctx, int B, int Wp, int D, int *whole_frames, bool *rest_underfilled);
int rsgm_launch_vert3_range(vppx_ctx *ctx, hipStream_t stream, int B_total, int f0, int nB, int Hp, int Wp, int D, const u8 *gray,
                            const u32 *cl, const u32 *cr, const u16 *p2lut, int p1, u8 *sv, u32 *xbuf, unsigned *err, unsigned *err_dev,
                            bool next_to_we);
int rsgm_launch_vert3(vppx_ctx *ctx, hipStream_t stream, int B, int Hp, int Wp, int D, const u8 *gray, const u32 *cl,
                      const u32 *cr, const u16 *p2lut, int p1, u8 *sv, u32 *xbuf, unsigned *err, unsigned *err_dev);
int rsgm_launch_void_if_lost(vppx_ctx *ctx, float *out, size_t n, const unsigned *err_dev, unsigned serial);
bool rsgm_vert_supported(int D, int maxp2);
size_t rsgm_vert_state_bytes(int B, int Wp, int D);
size_t rsgm_vert_min_elems(int B, int Wp);
int rsgm_launch_vert(vppx_ctx *ctx, hipStream_t stream, int B, int Hp, int Wp, int D, const u8 *gray, const u32 *cl,
                     const u32 *cr, const u16 *p2lut, int p1, u8 *sv, u8 *gst, u16 *gmin);
// S = sum of the 8 path volumes (+ left WTA, sub-pixel) ; disp_l may be null (stage API: S only)
int rsgm_launch_sum_wta(vppx_ctx *ctx, int B, int Hp, int Wp, int D, const void *paths, int elem_bytes, u16 *S,
                        u16 *ST, float *disp_l, u32 factor_uniq, int do_subpixel);
int rsgm_launch_wta_right_t(vppx_ctx *ctx, int B, int Hp, int Wp, int D, const u16 *ST, float *disp, u32 factor_uniq);
int rsgm_paths_elem_bytes(int D, int maxp2);
// fused sum + left/right WTA; returns 1 (not an error) when the shape is not covered
// max_path_value: upper bound of one path value (Cmax + P2max); 0 = unknown
size_t rsgm_sum_lds_bytes(const vppx_ctx *ctx, int D, int nvol);
bool rsgm_wsum_default(int B, int Hp, int Wp, int D, int maxp2, int nsimd);
bool rsgm_wsum_eligible(const vppx_ctx *ctx, int B, int Hp, int Wp, int D, int maxp2, int nsimd);
int rsgm_device_simds(vppx_ctx *ctx);
int rsgm_launch_wsum(vppx_ctx *ctx, int B, int Hp, int Wp, int D, const u8 *gray, const u32 *cl, const u32 *cr, const u16 *p2lut, int p1,
                     const void *vol_e, const void *vol_n3, const void *vol_s3, float *disp_l, float *disp_r, u32 fu);
int rsgm_launch_sum_wta_lr(vppx_ctx *ctx, int B, int Hp, int Wp, int D, const void *const *vols, int nvol, int elem_bytes,
                           float *disp_l, float *disp_r, u32 factor_uniq, int do_subpixel, int max_path_value);
int rsgm_launch_wta_left(vppx_ctx *ctx, int B, int Hp, int Wp, int D, const u16 *S, float *disp, u32 factor_uniq);
int rsgm_launch_subpixel(vppx_ctx *ctx, int B, int Hp, int Wp, int D, const u16 *S, float *disp);
int rsgm_launch_wta_right(vppx_ctx *ctx, int B, int Hp, int Wp, int D, const u16 *S, float *disp, u32 factor_uniq);
int rsgm_launch_median(vppx_ctx *ctx, int B, int Hp, int Wp, const float *src, float *dst);
// median3x3 + _linear_interpolate + clip of both views in one launch (fused pipeline)
int rsgm_launch_median_interp_clip(vppx_ctx *ctx, int B, int Hp, int Wp, const float *src_l, float *dst_l, const float *src_r,
                                   float *dst_r);
int rsgm_launch_post(vppx_ctx *ctx, const RsgmGeom &g, const float *dl_pad, const float *dr_pad, int subpixel, float *out);

// vpp_kernels.hip
struct VppGeom {
    int B, H, W, C;
};
int vpp_launch(vppx_ctx *ctx, const VppxVppParams &p, const VppGeom &g, u8 *l, u8 *r, const float *gmap,
               const u8 *occ, const float *filled_g, int64_t *n_hints_dev, const u32 *seeds_dev, const u8 *r_orig = nullptr);
// r_orig: the un-patterned right image when r is a copy of it (lets the L and R sides run side by side with a mask)
// _bilateral_filling (vpp_standalone.py:372-394) of the hints g guided by BGR2GRAY(left)
int vpp_launch_bilateral_fill(vppx_ctx *ctx, const VppxVppParams &p, const VppGeom &g, const u8 *left, const float *gmap,
                              float *filled_out);
int vpp_launch_rand_stream(vppx_ctx *ctx, u32 seed, u64 offset, int64_t n, int32_t *out_dev);
u64 vpp_draws_upper_bound(const VppxVppParams &p, const VppGeom &g);

// handoff_kernels.hip
int handoff_psmnet_cost_volume(vppx_ctx *ctx, const void *fl, const void *fr, const float *hints, const float *valid, int B, int C,
                               int H4, int W4, int H, int W, int maxdisp, void *cost, int dtype);
int handoff_raft_corr_modulate(vppx_ctx *ctx, void *corr, const float *hints, const float *valid, int B, int H4, int W2, int W3, int H,
                               int W, int dtype);
int handoff_kitti_decode(vppx_ctx *ctx, const uint16_t *png, size_t n, float *disp, u8 *valid);
int handoff_pfm_decode(vppx_ctx *ctx, const u8 *raw, int H, int W, int channels, int little, float *out);
// hints / valid -> feature resolution in WS_HANDOFF_H / _V (raft: h = x * v - hints * v / 4); refuses H / 4 != H4 or W / 4 != W4
int handoff_subsample_hints(vppx_ctx *ctx, const float *hints, const float *valid, int B, int H, int W, int H4, int W4, float **hs,
                            float **vs, int raft);
// corr_kernels.hip: CorrBlock1D's pyramid and lookup (models/raft_stereo/corr.py:116-145)
int corr_pyramid(vppx_ctx *ctx, void *corr, const float *hints, const float *valid, int B, int H4, int W2, int W3, int H, int W,
                 int levels, void *pyr, int dtype);
int corr_lookup(vppx_ctx *ctx, const void *corr, const void *pyr, const float *coords_x, int64_t coords_frame_stride, int B, int H4,
                int W2, int W3, int levels, int radius, float *out, int dtype);
// corr_gemm_kernels.hip: the all-pairs correlation itself (corr.py:151-155) on the matrix cores, fused with / sqrt(D), the hint
// modulation and the pyramid
int corr_fused(vppx_ctx *ctx, const void *fmap2, const void *fmap3, const float *hints, const float *valid, int B, int D, int H4,
               int W2, int W3, int H, int W, int levels, void *corr, void *pyr, int dtype);
// levels 1 .. levels-1 back to back, each dense [N][W3 >> i]: off[i] = first cell of level i (off[0] = 0, unused) -> cells in all
static inline int64_t corr_pyramid_offsets(int64_t N, int W3, int levels, int64_t *off)
{
    int64_t cells = 0;
    if (off) off[0] = 0;
    for (int i = 1; i < levels; i++) {
        if (off) off[i] = cells;
        cells += N * (int64_t)(W3 >> i);
    }
    return cells;
}

// readout_kernels.hip: the networks' output back as a float32 disparity map (psmnet.py:227-233, raft_stereo.py:69-81, test.py:237-245)
int readout_psm(vppx_ctx *ctx, const void *cost, int B, int D4, int H4, int W4, int D, int H, int W, int top, int left, int Hout,
                int Wout, float *out, int dtype);
int readout_raft_upsample(vppx_ctx *ctx, const void *flow, int64_t flow_frame_stride, const void *mask, int B, int C, int H4, int W4, int f,
                          int sign, int top, int left, int Hout, int Wout, float *out, int dtype);

// gru_kernels.hip: the update block's glue (models/raft_stereo/update.py:23-32, 87-97, 119-142)
int gru_assemble(vppx_ctx *ctx, const VppxGruSource *src, int n_src, int B, int H, int W, void *hx, int64_t hx_frame_stride, int dtype);
int gru_reset(vppx_ctx *ctx, const void *ar, int64_t sar, const void *cr, int64_t scr, const void *h, int64_t sh, void *hx, int64_t shx,
              int B, int C, int H, int W, int dtype);
int gru_update(vppx_ctx *ctx, const void *az, int64_t saz, const void *cz, int64_t scz, const void *aq, int64_t saq, const void *cq,
               int64_t scq, const void *h, int64_t sh, void *out, int64_t so, int B, int C, int H, int W, int dtype);

// motion_kernels.hip: the lookup fused into BasicMotionEncoder's convc1, and convf1 (models/raft_stereo/update.py:80,82)
int motion_front(vppx_ctx *ctx, const void *corr, const void *pyr, const float *coords_x, int64_t coords_frame_stride, const float *flow,
                 int64_t flow_frame_stride, const float *wc, const float *bias_c, int Cc, const float *wf, const float *bias_f, int Cf,
                 int ks, int B, int H4, int W2, int W3, int levels, int radius, void *out_c, int64_t out_c_frame_stride, void *out_f,
                 int64_t out_f_frame_stride, int dtype, int out_dtype);

// conv_kernels.hip: the 3x3 convolution on the matrix cores and ConvGRU's gates as its epilogues (update.py:19-32).
// The plain epilogue takes any Cout >= 1 (padded to 16 in the packing, masked in the store), ksize 1, stride 2, dilation 2 (at
// stride 1), a residual and a scale;
// the gates take ksize 3, stride 1, Cout % 16 == 0 and ignore the scale.
enum ConvEpi { CV_PLAIN = 0, CV_ZR = 1, CV_Q = 2 };

// a tensor the epilogue reads or writes, under the name its entry point gives it in a refusal; name NULL: the call has none
struct ConvTensor {
    const char *name = NULL;
    const void *p = NULL; // (an output's is written: its entry point took it as void *)
    int64_t stride = 0;   // cells between frames
};

// One call of the convolution kernel; what is left out is the 3x3 call at stride 1.
struct ConvCall {
    ConvEpi epi = CV_PLAIN;
    int ksize = 3, stride = 1, dilation = 1, dtype = VPPX_DT_F32;
    const void *x0 = NULL, *x1 = NULL; // the input is cat([x0, x1], dim=1); x1 is not read where C1 == 0
    int64_t s0 = 0, s1 = 0;            // cells between frames
    int C0 = 0, C1 = 0;
    const void *packed = NULL;         // conv_pack's buffer for (Cout, C0 + C1, ksize, dtype)
    int Cout = 0;                      // output channels of the packed weights (zr packs convz and convr: 2 C)
    ConvTensor in[3];                  // zr: cz, cr, h;  q: cq, z, h;  plain: the residual [B,Cout,Ho,Wo], or none
    ConvTensor out[2];                 // plain: out;  zr: z, rh;  q: out
    int B = 0, C = 0, H = 0, W = 0;    // C: the hidden size of the gates.  H, W: the input's; the output is (H - 1) / stride + 1 high
    int relu = 0;                      // plain: out = relu(v [+ res]) * scale
    float scale = 1.0f;
    bool vol = false;                  // a volume: x0 is [B,C0,D,H,W], the kernel 3x3x3 at stride 1, packed conv_pack(vol)'s for (Cout, C0);
    int D = 1;                         //   the residual and out are [B,Cout,D,H,W].  Plain epilogue, C1 == 0
};

size_t conv_packed_bytes(int Cout, int Cin, int ksize, int dtype);
int conv_pack(vppx_ctx *ctx, const float *weight, const float *bias, int Cout, int Cin, int ksize, int dtype, void *packed, bool vol = false);
int conv_run(vppx_ctx *ctx, const char *who, const ConvCall &c); // every field has been checked by vppx_net_api.hip

// spp_kernels.hip: PSMNet's pyramid pooling (models/psmnet/submodule.py:149-171), every level in one launch
int spp_pool(vppx_ctx *ctx, const void *x, int64_t sx, int B, int C, int H, int W, int n_levels, const int *ks, void *const *outs, int dtype);

// norm_kernels.hip: the encoders' glue (models/raft_stereo/extractor.py:48-60, :181-183, :276-278)
int norm_stats_pieces(int64_t planes, int64_t cells); // host arithmetic: workgroups per plane
int norm_stats(vppx_ctx *ctx, const void *x, int64_t sx, int B, int C, int H, int W, double eps, float *stats, int dtype);
int norm_apply(vppx_ctx *ctx, const void *x, int64_t sx, const float *stats, int64_t sst, const float *weight, const float *bias,
               int relu_inner, const void *res, int64_t sres, const float *res_stats, int64_t srst, const float *res_weight,
               const float *res_bias, void *out, int64_t so, int B, int C, int H, int W, int dtype);

// png_kernels.hip
int handoff_png_decode(vppx_ctx *ctx, int n_files, const u8 *blob_dev, const long long *offs_dev, int H, int W, int C, u8 *zcat,
                       const long long *zoffs_dev, float scale, float *disp, u8 *valid, u8 *out_u8, int *status_dev);

// scale_kernels.hip (--iscale / --oscale, DESIGN section 5 rule 1)
struct ScaleFrontArgs {
    const u8 *l, *r;        // [B, H, W, C]
    const float *g, *vh;    // [B, H, W]; vh may be null
    u8 *ls, *rs;            // [B, h, w, C]
    float *gs, *vhs;        // [B, h, w]
    const int4 *ytab;       // [h]: {first row, second row (clamped), b0, b1}
    const int4 *xtab;       // [w]: {first column, second column (clamped), a0, a1}
    int B, H, W, C, h, w, s;
    float fs;               // (float)s
    long long n_img_threads; // (set by the launcher)
};
int scale_launch_front(vppx_ctx *ctx, const ScaleFrontArgs &a);
int scale_launch_restore(vppx_ctx *ctx, int B, int h, int w, int Ho, int Wo, const float *src, float *out, const int *ry,
                         const int *rx, int iscale, int oscale);

// metrics_kernels.hip (losses.guided_metrics, losses.py:13-24)
#define METRICS_PARTIAL_BYTES 64
#define METRICS_MAX_BLOCKS 64
int metrics_blocks_per_frame(size_t npx); // a function of the frame's shape only: results do not depend on the batch
// gt / valid: [B, Hg, Wg] read at every gt_scale-th row and column, gt divided by gt_scale; valid: float32, or one byte per pixel
// (valid_is_u8); partials: B * metrics_blocks_per_frame(Ho * Wo) records of METRICS_PARTIAL_BYTES; errormap may be null
int metrics_launch(vppx_ctx *ctx, int B, int Ho, int Wo, const float *disp, int Hg, int Wg, int gt_scale, const float *gt,
                   const void *valid, int valid_is_u8, void *partials, VppxMetrics *out, float *errormap);

// sample_kernels.hip (losses.sample_hints, losses.py:5-10, on torch's CPU random stream)
// src / hints: float32 [B][npx]; vsrc: float32, or one byte per pixel (vsrc_is_u8); vhints may be null.  Frame f samples with
// seeds_dev[f], or with seed + f when seeds_dev is null; T = sample_threshold(probability)
int sample_launch(vppx_ctx *ctx, int B, size_t npx, const float *src, const void *vsrc, int vsrc_is_u8, float *hints, float *vhints,
                  const u32 *seeds_dev, u32 seed, u32 T);
u32 sample_threshold(double p);

// viz_kernels.hip (utils.py:17-79, test.py:318-343): pictures uint8 [B,H,W,3], dilation fused (0 and 1: none)
#define VIZ_MAX_DILATION VPPX_VIZ_MAX_DILATION
#define VIZ_FMAX_MAX_BLOCKS 64
int viz_launch_error_colors(vppx_ctx *ctx, int B, int H, int W, const float *errors, const float *mask, double scale, int bgr,
                            int dilation, u8 *out); // mask may be null
// out: six planes [6][B,H,W,3] in the reference's key order; only the planes whose bit is set in `which` are written
int viz_launch_guided(vppx_ctx *ctx, int B, int H, int W, const float *disp, const float *gt, const float *valid, double scale,
                      int dilation, unsigned which, u8 *out);
int viz_launch_colorize(vppx_ctx *ctx, int B, int H, int W, const float *x, const float *max_val, const u8 *lut, int dilation, u8 *out);
int viz_finite_max_blocks(size_t npx); // a function of the frame's shape only
int viz_launch_finite_max(vppx_ctx *ctx, int B, int H, int W, const float *x, float *part, float *out); // part: B * viz_finite_max_blocks

// occ_kernels (in vpp_kernels.hip)
int occ_launch(vppx_ctx *ctx, int B, int H, int W, const float *hints, int rx, int ry, double l, double g,
               double th_conf, double th_filter, float *omap, u8 *conf_out, float *dmap_out = nullptr);
