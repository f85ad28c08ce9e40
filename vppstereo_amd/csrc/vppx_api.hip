// vppx_api.hip -- C-ABI entry points of libvppx.so (declared in include/vppx.h).
// Host-side orchestration only: context, workspace arena, H2D/D2H staging for the
// host-pointer entry points, kernel sequencing.  No compute happens on the CPU and there is
// no CPU fallback: without a HIP device every entry point fails with VPPX_E_NO_DEVICE.
#include "vppx_internal.h"

#include <limits.h>
#include <math.h>
#include <stdarg.h>
#include <stdlib.h>
#include <string.h>

// ---------------------------------------------------------------------------------------
// errors
// ---------------------------------------------------------------------------------------
static thread_local char g_err[1024] = "";

void vppx_set_error(const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

extern "C" const char *vppx_last_error(void) { return g_err; }

// ---------------------------------------------------------------------------------------
// routes: the kernel instantiations the last rSGM-bearing call launched (vppx_last_routes)
// ---------------------------------------------------------------------------------------
static void note_once(std::vector<std::string> &list, const char *name)
{
    for (const std::string &r : list)
        if (r == name) return;
    list.emplace_back(name);
}

void route_note(vppx_ctx *ctx, const char *fmt, ...)
{
    char buf[128];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    note_once(ctx->routes, buf);
    if (ctx->timing_run) note_once(ctx->timing_routes, buf);
}

void front_route_note(vppx_ctx *ctx, const char *fmt, ...)
{
    char buf[128];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    note_once(ctx->front_routes, buf);
}

static int routes_to_buf(const char *who, vppx_ctx *ctx, const std::vector<std::string> vppx_ctx::*list, char *buf, int n)
{
    if (!ctx) { vppx_set_error("context is NULL (vppx_create failed? there is no CPU fallback)"); return VPPX_E_NO_DEVICE; }
    if (n < 0 || (n > 0 && !buf)) { vppx_set_error("%s: bad buffer", who); return VPPX_E_INVALID_ARG; }
    std::string all;
    for (const std::string &r : ctx->*list) {
        if (!all.empty()) all += ',';
        all += r;
    }
    if (n > 0) {
        const size_t k = all.size() < (size_t)n - 1 ? all.size() : (size_t)n - 1;
        memcpy(buf, all.data(), k);
        buf[k] = '\0';
    }
    return (int)all.size();
}

extern "C" int vppx_last_routes(vppx_ctx *ctx, char *buf, int n) { return routes_to_buf("vppx_last_routes", ctx, &vppx_ctx::routes, buf, n); }
extern "C" int vppx_timing_last_routes(vppx_ctx *ctx, char *buf, int n)
{
    if (ctx && !ctx->have_last && ctx->sub[0] && ctx->sub[0]->have_last) ctx = ctx->sub[0]; // the context the helpers re-launch on
    return routes_to_buf("vppx_timing_last_routes", ctx, &vppx_ctx::timing_routes, buf, n);
}
extern "C" int vppx_last_front_routes(vppx_ctx *ctx, char *buf, int n)
{
    return routes_to_buf("vppx_last_front_routes", ctx, &vppx_ctx::front_routes, buf, n);
}

extern "C" int vppx_version(void) { return VPPX_VERSION; }

extern "C" void vppx_vpp_params_default(VppxVppParams *p)
{
    memset(p, 0, sizeof(*p));
    p->method = VPPX_METHOD_RND;
    p->wsize = 3;
    p->wsize_agg_x = 64;
    p->wsize_agg_y = 3;
    p->direction = 1;
    p->uniform_color = 0;
    p->discard_occluded = 0;
    p->interpolate = 1;
    p->c = 0.4f;
    p->c_occ = 0.0f;
    p->distance_gamma = 0.3;
    p->seed = 1;
    p->bilateral_o_xy = 2.0;
    p->bilateral_o_i = 1.0;
    p->bilateral_th = 0.001;
}

extern "C" void vppx_occ_params_default(VppxOccParams *p) // filter.py:246
{
    memset(p, 0, sizeof(*p));
    p->rx = 9;
    p->ry = 7;
    p->l = 2.0;
    p->g = 0.4375;
    p->th_conf = 1.0;
    p->th_filter = 0.1;
}

extern "C" void vppx_rsgm_params_default(VppxRsgmParams *p)
{
    memset(p, 0, sizeof(*p));
    p->dmax = 192;
    p->p1 = 11;
    p->p2min = 17;
    p->alpha = 0.5f;
    p->gamma = 35;
    p->uniqueness = 0.95f;
    p->subpixel = 1;
}

// ---------------------------------------------------------------------------------------
// context / workspace
// ---------------------------------------------------------------------------------------
int ws_reserve(vppx_ctx *ctx, WsSlot s, size_t bytes, void **out)
{
    DevBuf &b = ctx->ws[s];
    if (bytes == 0) bytes = 16;
    if (b.cap < bytes) {
        if (ctx->capturing) { vppx_set_error("workspace growth during graph capture"); return VPPX_E_HIP; }
        ctx->ws_gen++;
        if (b.p) {
            // the old buffer may still be referenced by enqueued kernels
            VPPX_HIP(hipStreamSynchronize(ctx->stream));
            VPPX_HIP(hipFree(b.p));
            ctx->total_bytes -= b.cap;
            b.p = nullptr;
            b.cap = 0;
        }
        const size_t cap = (bytes + 255) & ~(size_t)255;
        hipError_t e = hipMalloc(&b.p, cap);
        if (e != hipSuccess) {
            b.p = nullptr;
            vppx_set_error("workspace allocation of %zu bytes failed: %s", cap, hipGetErrorString(e));
            return VPPX_E_OOM;
        }
        b.cap = cap;
        ctx->total_bytes += cap;
    }
    *out = b.p;
    return 0;
}

extern "C" int vppx_create(vppx_ctx **out, int device)
{
    if (!out) { vppx_set_error("vppx_create: out is NULL"); return VPPX_E_INVALID_ARG; }
    *out = nullptr;
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0) {
        vppx_set_error("no HIP device available (%s); libvppx has no CPU fallback",
                       e != hipSuccess ? hipGetErrorString(e) : "device count is 0");
        return VPPX_E_NO_DEVICE;
    }
    if (device < 0) {
        if (hipGetDevice(&device) != hipSuccess) device = 0;
    }
    if (device >= ndev) { vppx_set_error("device %d out of range (%d devices)", device, ndev); return VPPX_E_INVALID_ARG; }
    DevGuard dev_guard_(device); // the caller's current device is restored on return
    vppx_ctx *ctx = new vppx_ctx();
    ctx->device = device;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) == hipSuccess) {
        ctx->devname = prop.name[0] ? prop.name : prop.gcnArchName;
        if (strstr(prop.gcnArchName, "gfx950") == nullptr) {
            vppx_set_error("device %d is %s; libvppx is built for gfx950 only", device, prop.gcnArchName);
            delete ctx;
            return VPPX_E_NO_DEVICE;
        }
    }
    e = hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking);
    if (e != hipSuccess) {
        vppx_set_error("hipStreamCreate failed: %s", hipGetErrorString(e));
        delete ctx;
        return VPPX_E_HIP;
    }
    ctx->own_stream = true;
    if (hipStreamCreateWithFlags(&ctx->stream2, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreateWithFlags(&ctx->ev_fork, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&ctx->ev_join, hipEventDisableTiming) != hipSuccess) {
        vppx_set_error("side stream / event creation failed");
        delete ctx;
        return VPPX_E_HIP;
    }
    {
        const char *e = getenv("VPPX_VERT");
        ctx->use_vert = e ? atoi(e) : -1;
        e = getenv("VPPX_CHUNK");
        if (e) ctx->knobs.chunk = atoi(e);
        e = getenv("VPPX_VARIANT"); // comma-separated tokens: alternative kernels with identical results (vppx_internal.h, Knobs)
        if (e) {
            std::string v(e);
            auto has = [&](const char *tok) { return ("," + v + ",").find(std::string(",") + tok + ",") != std::string::npos; };
            if (has("sum_general")) ctx->knobs.sum_general = 1;
            if (has("gw4")) ctx->knobs.gw = 4;
            if (has("gw8")) ctx->knobs.gw = 8;
            if (has("gw16")) ctx->knobs.gw = 16;
            if (has("maxdist_lds")) ctx->knobs.maxdist = 1;
            if (has("maxdist_global")) ctx->knobs.maxdist = 2;
            if (has("we_line")) ctx->knobs.we_line = 1;
            if (has("sum_gl8")) ctx->knobs.sum_gl8 = 1;
            if (has("sum_trap0")) ctx->knobs.sum_trap = 0;
            if (has("sum_trap1")) ctx->knobs.sum_trap = 1;
            if (has("we_after")) ctx->knobs.we_next = 0;
            if (has("we_whole")) ctx->knobs.we_split = 0;
            if (has("we_mute")) ctx->knobs.we_mute = 1;
            if (has("we_stale")) ctx->knobs.we_stale = 1;
            {
                const size_t fk = v.find("fs_fail_submit="), ff = v.find("fs_fail_from=");
                if (fk != std::string::npos) ctx->knobs.fs_fail_submit = atoi(v.c_str() + fk + 15);
                if (ff != std::string::npos) ctx->knobs.fs_fail_from = atoi(v.c_str() + ff + 13);
            }
            {
                const size_t wl = v.find("we_layer=");
                if (wl != std::string::npos) ctx->knobs.we_layer = atoi(v.c_str() + wl + 9);
            }
            if (has("wsum")) ctx->knobs.wsum = 1;
            if (has("nowsum")) ctx->knobs.wsum = 0;
            {
                const size_t wc = v.find("wsum_cut=");
                if (wc != std::string::npos) ctx->knobs.wsum_cut = atoi(v.c_str() + wc + 9);
            }
            if (has("we_lq0")) ctx->knobs.we_lq = 0;
            if (has("we_lq1")) ctx->knobs.we_lq = 1;
#ifdef VPPX_EXPERIMENT
            if (has("pipe_mid")) ctx->pipe_mid = true; // the next front stage starts behind the vertical kernel, next to W/E (measured: 9.16 -> 9.6 ms per step)
            const size_t sb = v.find("sum_blocks=");
            if (sb != std::string::npos) ctx->knobs.sum_blocks = atoi(v.c_str() + sb + 11);
#endif
        }
        e = getenv("VPPX_SUBSTREAMS");
        if (e) ctx->nsub = atoi(e) < 1 ? 1 : (atoi(e) > 4 ? 4 : atoi(e));
        // bounds of one neighbour wait in the fused aggregation kernel: milliseconds of wall clock (the bound that counts)
        // and, for tests that must see the give-up path, a number of polls (1 = give up at the first record not there yet)
        e = getenv("VPPX_V3_TIMEOUT_MS");
        if (e && atoi(e) > 0) ctx->v3.timeout_ms = atoi(e);
        e = getenv("VPPX_V3_PPW");
        if (e && (atoi(e) == 8 || atoi(e) == 16)) ctx->v3.ppw = atoi(e);
#ifdef VPPX_EXPERIMENT // measurement builds only (tools/build_exp.sh): the shipped library cannot be told to ignore a lost lock step
        e = getenv("VPPX_V3_IGNORE_LOST");
        if (e && atoi(e) > 0) ctx->v3.ignore_lost = true;
        e = getenv("VPPX_EXP_WE_TRACE");
        if (e && *e) ctx->exp_we_trace = e;
#endif
        e = getenv("VPPX_V3_SPIN_LIMIT");
        if (e && atoi(e) > 0) ctx->v3.spin_limit = (unsigned)atoi(e);
        e = getenv("VPPX_GUIDED_PART_MB");
        if (e && atoll(e) > 0) ctx->knobs.guided_part_bytes = (unsigned long long)atoll(e) << 20;
    }
    *out = ctx;
    return 0;
}

extern "C" void vppx_destroy(vppx_ctx *ctx)
{
    if (!ctx) return;
    DevGuard dev_guard_(ctx->device);
    (void)hipDeviceSynchronize();
    for (int i = 0; i < 4; i++) {
        if (ctx->sub[i]) vppx_destroy(ctx->sub[i]);
        if (ctx->sub_done[i]) (void)hipEventDestroy(ctx->sub_done[i]);
    }
    for (int i = 0; i < WS_NUM; i++)
        if (ctx->ws[i].p) (void)hipFree(ctx->ws[i].p);
    for (hipEvent_t e : ctx->ev) (void)hipEventDestroy(e);
    if (ctx->gexec) (void)hipGraphExecDestroy(ctx->gexec);
    if (ctx->agg_ev_created)
        for (int j = 0; j < 2; j++)
            for (int i = 0; i < vppx_ctx::AGG_RING; i++) {
                (void)hipEventDestroy(ctx->agg_ev[j][i]);
                (void)hipEventDestroy(ctx->we_ev[j][i]);
            }
    if (ctx->own_stream && ctx->stream) (void)hipStreamDestroy(ctx->stream);
    if (ctx->vert3_err) (void)hipHostFree(ctx->vert3_err);
    if (ctx->stream_front) (void)hipStreamDestroy(ctx->stream_front);
    if (ctx->ev_agg_done) (void)hipEventDestroy(ctx->ev_agg_done);
    if (ctx->ev_front_done) (void)hipEventDestroy(ctx->ev_front_done);
    if (ctx->ev_occ_done) (void)hipEventDestroy(ctx->ev_occ_done);
    if (ctx->ev_inputs_auto) (void)hipEventDestroy(ctx->ev_inputs_auto);
    if (ctx->ev_scaled) (void)hipEventDestroy(ctx->ev_scaled);
    if (ctx->ev_sampled) (void)hipEventDestroy(ctx->ev_sampled);
    if (ctx->stream2) (void)hipStreamDestroy(ctx->stream2);
    if (ctx->ev_fork) (void)hipEventDestroy(ctx->ev_fork);
    if (ctx->ev_join) (void)hipEventDestroy(ctx->ev_join);
    delete ctx;
}

extern "C" int vppx_set_graph_mode(vppx_ctx *ctx, int enable)
{
    if (!ctx) return VPPX_E_INVALID_ARG;
    ctx->graph_mode = enable != 0;
    if (!enable && ctx->gexec) { (void)hipGraphExecDestroy(ctx->gexec); ctx->gexec = nullptr; ctx->have_gkey = false; }
    ctx->have_lastkey = false;
    return 0;
}

extern "C" long vppx_graph_replays(vppx_ctx *ctx) { return ctx ? ctx->graph_replays : 0; }
extern "C" long vppx_scale_table_builds(vppx_ctx *ctx) { return ctx ? ctx->scale_tab_builds : 0; }
extern "C" int vppx_last_front_sets(vppx_ctx *ctx, int *scale_set, int *sample_set)
{
    if (!ctx) { vppx_set_error("vppx_last_front_sets: ctx is NULL"); return VPPX_E_INVALID_ARG; }
    if (scale_set) *scale_set = ctx->last_scale_set;
    if (sample_set) *sample_set = ctx->last_sample_set;
    return 0;
}

// Drop the context's own stream (after draining it) before it is pointed at a caller's stream.
static int release_own_stream(vppx_ctx *ctx)
{
    if (ctx->own_stream && ctx->stream) {
        VPPX_HIP(hipStreamSynchronize(ctx->stream));
        (void)hipStreamDestroy(ctx->stream);
    }
    ctx->own_stream = false;
    ctx->stream = nullptr;
    return 0;
}

extern "C" int vppx_set_stream(vppx_ctx *ctx, void *hip_stream)
{
    VPPX_ENTER(ctx);
    if (hip_stream != nullptr) {
        if (ctx->stream == (hipStream_t)hip_stream && !ctx->own_stream && !ctx->legacy_stream) { // already bound
            VPPX_PIPE_KEEP(ctx);
            return 0;
        }
        int rc = release_own_stream(ctx);
        if (rc) return rc;
        ctx->stream = (hipStream_t)hip_stream;
        ctx->legacy_stream = false;
    } else if (!ctx->own_stream) {
        VPPX_HIP(hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking));
        ctx->own_stream = true;
        ctx->legacy_stream = false;
    }
    return 0;
}

// Launch on the legacy default ("null") stream itself: what torch's default stream is.  Work is then ordered
// with everything else the process enqueues there, exactly like kernels torch launches on its default stream.
extern "C" int vppx_set_stream_legacy(vppx_ctx *ctx)
{
    VPPX_ENTER(ctx);
    if (ctx->legacy_stream) {
        VPPX_PIPE_KEEP(ctx);
        return 0;
    }
    int rc = release_own_stream(ctx);
    if (rc) return rc;
    ctx->stream = nullptr; // hipStream_t 0 = the legacy default stream
    ctx->legacy_stream = true;
    return 0;
}

// The fused aggregation kernel (sgm_vert3_kernel) reports a lost lock step -- a wave that waited longer than the bound
// for its neighbour's record -- through a pinned host word.  Whoever looks at it first reports it: vppx_status,
// vppx_synchronize, the host-pointer entry points after their own synchronisation, and the next call of the hot path.
// The context then rests on the line-parallel kernel (vert3_rest aggregation launches, doubling with every loss) and a captured
// graph holding the launch is dropped.
static int lockstep_check(vppx_ctx *ctx)
{
    if (!ctx->vert3_err || !ctx->vert3_err[0]) return 0;
    const unsigned serial = ctx->vert3_err[0];
    ctx->vert3_err[0] = 0;
    ctx->lockstep_failures++;
    ctx->lockstep_last_serial = serial;
    if (ctx->v3.ignore_lost) return 0; // measurement only (tools/agg_probe.py: the fused kernel's time without any neighbour wait)
    // Contention is usually temporary (another process or stream held block slots of an XCD): the context rests on the
    // line-parallel layout for a while, then tries the fused layout again; the rest doubles with every loss.
    ctx->vert3_rest = ctx->vert3_backoff;
    ctx->vert3_backoff = ctx->vert3_backoff < 4096 ? ctx->vert3_backoff * 2 : 4096;
    if (ctx->gexec) {
        (void)hipGraphExecDestroy(ctx->gexec);
        ctx->gexec = nullptr;
        ctx->have_gkey = false;
    }
    ctx->have_lastkey = false;
    vppx_set_error("fused aggregation launch #%u lost its lock step (a wave waited longer than %d ms%s for its neighbour): the "
                   "disparities of that call are void, and so are those of fused calls queued behind it (last launch: #%u); "
                   "the context uses the line-parallel aggregation kernel for its next %d aggregation launches, then tries the fused layout again",
                   serial, ctx->v3.timeout_ms, ctx->v3.spin_limit ? " / VPPX_V3_SPIN_LIMIT polls" : "", ctx->v3.serial, ctx->vert3_rest);
    return VPPX_E_HIP;
}

int vppx_lockstep_check_internal(vppx_ctx *ctx) { return lockstep_check(ctx); } // (vppx_fstream.hip)
static int check_frames(int B, int H, int W, int C);
static int check_vpp_params(const VppxVppParams &p);
static int check_rsgm_params(const VppxRsgmParams &p);
// the argument checks of the fused entry points, for a frame stream to make when it is CREATED (not at its first full batch)
int vppx_check_hot_path_args_internal(const VppxVppParams *vp, const VppxRsgmParams *rp, int B, int H, int W, int C)
{
    int rc;
    if ((rc = check_frames(B, H, W, C))) return rc;
    if ((rc = check_vpp_params(*vp))) return rc;
    return check_rsgm_params(*rp);
}

extern "C" int vppx_synchronize(vppx_ctx *ctx)
{
    VPPX_ENTER(ctx);
    VPPX_HIP(hipStreamSynchronize(ctx->stream));
    return lockstep_check(ctx);
}

// Non-blocking: has any fused aggregation launch that has finished so far lost its lock step?  (After a synchronisation
// of the launch stream -- by whatever means, e.g. torch.cuda.synchronize -- the answer covers every call made so far.)
extern "C" int vppx_status(vppx_ctx *ctx)
{
    VPPX_ENTER(ctx);
    VPPX_PIPE_KEEP(ctx);
    return lockstep_check(ctx);
}

extern "C" long vppx_lockstep_failures(vppx_ctx *ctx) { return ctx ? ctx->lockstep_failures : 0; }
extern "C" int vppx_fused_pixels_per_wave(vppx_ctx *ctx) { return (ctx && ctx->last_vert == 3) ? ctx->v3.last_ppw : 0; }

static void make_geom(int B, int H, int W, int C, int D, RsgmGeom &g);
static int v3_probe_once(vppx_ctx *ctx);
extern "C" int vppx_batch_quantum(vppx_ctx *ctx, int H, int W, int dmax)
{
    if (!ctx || H < 1 || W < 1 || ctx->capturing) return 0;
    DevGuard dev_guard_(ctx->device);
    if (ctx->vert3_broken || v3_probe_once(ctx) != 0 || ctx->vert3_broken) return 0;
    RsgmGeom g;
    make_geom(1, H, W, 3, dmax, g);
    return rsgm_vert3_frames_per_round(ctx, g.Wp, g.D);
}

extern "C" size_t vppx_workspace_bytes(const vppx_ctx *ctx)
{
    if (!ctx) return 0;
    size_t t = ctx->total_bytes;
    for (int i = 0; i < 4; i++)
        if (ctx->sub[i]) t += ctx->sub[i]->total_bytes;
    return t;
}
extern "C" const char *vppx_device_name(const vppx_ctx *ctx) { return ctx ? ctx->devname.c_str() : ""; }

// ---------------------------------------------------------------------------------------
// stage timing
// ---------------------------------------------------------------------------------------
static const char *k_stage_names[ST_COUNT] = {"vpp_compact", "vpp_rand", "vpp_apply", "pad_gray", "census",
                                              "aggregate_8paths", "sum_wta_left", "wta_right", "median_interp", "post",
                                              "occlusion_heuristic"};

extern "C" const char *vppx_stage_name(int i) { return (i >= 0 && i < ST_COUNT) ? k_stage_names[i] : ""; }

// the table of marks grows with the call: events for marks 0..n exist after this (a call in parts makes 10 or 11 marks per part)
static int stage_events(vppx_ctx *ctx, size_t n)
{
    if (ctx->ev.size() > n) return 0; // (the usual mark: nothing to create, no device switch)
    DevGuard dev_guard_(ctx->device);
    while (ctx->ev.size() <= n) {
        hipEvent_t e;
        VPPX_HIP(hipEventCreate(&e));
        ctx->ev.push_back(e);
    }
    return 0;
}

extern "C" int vppx_enable_stage_timing(vppx_ctx *ctx, int enable)
{
    int rc;
    if (!ctx) return VPPX_E_INVALID_ARG;
    if (enable && (rc = stage_events(ctx, 32))) return rc;
    ctx->stage_timing = enable != 0;
    ctx->n_stages = 0;
    return 0;
}

extern "C" int vppx_stage_marks(vppx_ctx *ctx) { return (ctx && ctx->stage_timing) ? ctx->n_stages : 0; }

void stage_begin(vppx_ctx *ctx)
{
    if (!ctx->stage_timing || ctx->capturing) return;
    if (ctx->stage_append && ctx->n_stages > 0) return; // later part of a split batch: the times add up per stage
    ctx->n_stages = 0;
    (void)hipEventRecord(ctx->ev[0], ctx->stream);
}

void stage_mark(vppx_ctx *ctx, int stage)
{
    if (!ctx->stage_timing || ctx->capturing) return;
    if (stage_events(ctx, (size_t)ctx->n_stages + 1)) return; // (no event, no mark: vppx_last_error has the reason)
    ctx->stage_id.resize((size_t)ctx->n_stages + 1);
    ctx->stage_id[ctx->n_stages] = stage;
    ctx->n_stages++;
    (void)hipEventRecord(ctx->ev[ctx->n_stages], ctx->stream);
}

extern "C" int vppx_get_stage_ms(vppx_ctx *ctx, float *ms, int max_n)
{
    if (!ctx || !ms) return VPPX_E_INVALID_ARG;
    for (int i = 0; i < ST_COUNT && i < max_n; i++) ms[i] = 0.f;
    if (!ctx->stage_timing || ctx->n_stages == 0) return 0;
    VPPX_HIP(hipEventSynchronize(ctx->ev[ctx->n_stages]));
    for (int i = 0; i < ctx->n_stages; i++) {
        float t = 0.f;
        VPPX_HIP(hipEventElapsedTime(&t, ctx->ev[i], ctx->ev[i + 1]));
        if (ctx->stage_id[i] < max_n) ms[ctx->stage_id[i]] += t;
    }
    return ST_COUNT < max_n ? ST_COUNT : max_n;
}

// ---------------------------------------------------------------------------------------
// helpers
// ---------------------------------------------------------------------------------------
// Host <-> device copies of the host-pointer entry points: straight from / to the caller's (pageable) arrays.  (Round 5 measured
// a pinned staging arena owned by the context -- memcpy into it, asynchronous DMA from it, results copied out after the
// synchronisation: occlusion_heuristic + vpp + compute_rsgm of one 540x960x192 frame 1.49 -> 1.89 ms, the fused host entry
// 1.03 -> 1.13 ms: the runtime's own staging of pageable copies is faster than an extra pass over the data on one core.)
static int upload(vppx_ctx *ctx, WsSlot s, const void *host, size_t bytes, void **dev)
{
    int rc = ws_reserve(ctx, s, bytes, dev);
    if (rc) return rc;
    VPPX_HIP(hipMemcpyAsync(*dev, host, bytes, hipMemcpyHostToDevice, ctx->stream));
    return 0;
}

static int download(vppx_ctx *ctx, void *host, const void *dev, size_t bytes)
{
    VPPX_HIP(hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, ctx->stream));
    return 0;
}

// first fused launch of a context (or the first question about it): block placement and residency of this device
static int v3_probe_once(vppx_ctx *ctx)
{
    if (ctx->vert3_probed) return 0;
    int rc;
    u32 *probe;
    bool ok = false;
    if ((rc = ws_get(ctx, WS_VMIN, (size_t)512, (u16 **)&probe))) return rc;
    if ((rc = rsgm_vert3_probe(ctx, probe, &ok))) return rc;
    ctx->vert3_probed = true;
    if (!ok) ctx->vert3_broken = true;
    return 0;
}

static void make_geom(int B, int H, int W, int C, int D, RsgmGeom &g)
{
    g.B = B; g.H = H; g.W = W; g.C = C; g.D = D;
    const int pad_ht = (((H / 16) + 1) * 16 - H) % 16; // rsgm.py:254
    const int pad_wd = (((W / 16) + 1) * 16 - W) % 16; // rsgm.py:255
    g.pad_l = pad_wd / 2; g.pad_r = pad_wd - pad_wd / 2;
    g.pad_t = pad_ht / 2; g.pad_b = pad_ht - pad_ht / 2;
    g.Hp = H + pad_ht; g.Wp = W + pad_wd;
}

// P2(|dI|) = max(P2min, (int)(-alpha*|dI| + gamma)), float32 without contraction
static int p2_lut_host(const VppxRsgmParams &p, u16 *lut, int *maxp2)
{
    int mx = 0;
    for (int i = 0; i < 256; i++) {
        volatile float t = (-p.alpha) * (float)i;
        volatile float u = t + (float)p.gamma;
        float uu = u;
        long long v = (uu != uu) ? 0 : (uu > 2147483000.f ? 2147483647LL : (uu < -2147483000.f ? -2147483647LL : (long long)(int32_t)uu));
        if (v < p.p2min) v = p.p2min;
        if (v < 0) v = 0;
        if (v > 65535) v = 65535;
        lut[i] = (u16)v;
        if ((int)v > mx) mx = (int)v;
    }
    *maxp2 = mx;
    return 0;
}

static u32 uniq_factor(float uniqueness)
{
    volatile float f = 1024.0f * uniqueness;
    return (u32)f;
}

static int check_rsgm_params(const VppxRsgmParams &p)
{
    // same order and messages as rsgm.py:31-35,166-167
    if (p.dmax % 8 != 0) { vppx_set_error("Invalid dmax (%d): dmax %% 8 != 0", p.dmax); return VPPX_E_DMAX_MOD8; }
    if (p.dmax > 256) { vppx_set_error("Invalid dmax (%d): dmax > 256", p.dmax); return VPPX_E_DMAX_GT256; }
    if (p.dmax <= 0) { vppx_set_error("Invalid dmax (%d)", p.dmax); return VPPX_E_INVALID_ARG; }
    if (p.uniqueness > 1.0f || p.uniqueness <= 0.0f) {
        vppx_set_error("Invalid uniqueness (%g): uniqueness in ]0,1]", (double)p.uniqueness);
        return VPPX_E_UNIQUENESS;
    }
    return 0;
}

// ---------------------------------------------------------------------------------------
// 8-path aggregation stage.  which: 0 = everything, 1 = horizontal paths only, 2 = vertical bands
// only (timing helpers).  Fills vols[] with the volumes the sum/WTA kernel has to add.
// ---------------------------------------------------------------------------------------
// Would a call of this geometry take the fused layout (W/E line-parallel + the lock-step vertical kernel)?  use_vert: -1
// (default) = pick by shape, 0 = eight line-parallel paths, 3 = fused whenever the shape allows it.  Probes the device on
// the first question (block placement, residency).
// frames per launch from which the fused layout wins (540x960x192, ms per call 8-path / fused; round 5, with W/E next to the
// under-filled lock-step launch: 2 frames 0.99 / 1.12, 3 frames 1.41 / 1.24, 4 frames 1.77 / 1.37, 5 frames 2.12 / 1.72; one
// pair 0.56 / 1.03.  Round 4, W/E behind it: 4 frames 0.44 / 0.46 per frame, 6 frames 0.43 / 0.39: the threshold was 6)
#define VPPX_FUSED_MIN_FRAMES 3
static int fused_layout_wanted(vppx_ctx *ctx, const RsgmGeom &g, int maxp2, bool *out)
{
    int rc;
    *out = false;
    const int elem_bytes = rsgm_paths_elem_bytes(g.D, maxp2);
    bool v3_ok = !ctx->vert3_broken && ctx->vert3_rest <= 0 && elem_bytes == 1 && rsgm_vert3_supported(g.B, g.Hp, g.Wp, g.D, maxp2);
    if (v3_ok && !ctx->vert3_probed && !ctx->capturing && (ctx->use_vert == 3 || (ctx->use_vert < 0 && g.B >= VPPX_FUSED_MIN_FRAMES))) {
        // first fused launch of this context: does this device place consecutive block ids the way the kernel assumes
        // (8 XCDs, round-robin), and how many blocks of this build of the kernel does one XCD hold?
        if ((rc = v3_probe_once(ctx))) return rc;
    }
    if (!ctx->vert3_probed) v3_ok = false; // (e.g. a first call inside a graph capture takes the 8-path layout)
    v3_ok = v3_ok && !ctx->vert3_broken && rsgm_vert3_fits(ctx, g.B, g.Wp, g.D); // a whole group + early arrivals resident per XCD
    // (measured at B=32, 8-path / fused ms per step: D=64 7.5 / 7.5, D=128 10.6 / 9.2, D=192 13.3 / 11.7; 1536x2048x256 at
    // B=8 28.1 / 28.9: the default takes the fused layout for D = 128 and 192)
    // Default: the fused layout from 8 frames per launch on for D = 128 / 192, and for every D once the batch fills the chip
    // with groups of the 16-pixels-per-wave kernel (round 3, ms per step 8-path / fused 8 px per wave / fused 16 px per wave:
    // 540x960 B=32 D=64 7.4 / 7.5 / 6.8, D=128 10.6 / 9.3 / 9.0; 375x1242x192 B=32 12.1 / 10.4 / 10.2; 1536x2048x256 B=8
    // 28.7 / 32.0 / 23.1, B=16 56.4 / 64.4 / 46.1)
    *out = v3_ok && (ctx->use_vert == 3 || (ctx->use_vert < 0 && g.B >= VPPX_FUSED_MIN_FRAMES && (g.D == 128 || g.D == 192 || rsgm_vert3_wide(ctx, g.B, g.Wp, g.D))));
    return 0;
}

#ifdef VPPX_EXPERIMENT
// Experiment hooks (never in the shipped build; tools/build_exp.sh): what runs right before the W/E launch of a step.
//   VPPX_EXP_PRE=1  read every census / gray byte the launch will read (warms L2 / MALL / TLB of those)
//   VPPX_EXP_PRE=2  read one dword per 4 KB of the two volumes the launch writes (TLB of the store stream)
//   VPPX_EXP_PRE=3  ~0.3 ms of dense VALU work on every CU (clock / power state)
//   VPPX_EXP_PRE=6  write one dword per 4 KB of the two volumes
//   VPPX_EXP_ORDER=1 W/E first, fused vertical kernel second (the order of rounds 2-3);  VPPX_EXP_TWICE=1 W/E launched twice (the second is timed)
__global__ void __launch_bounds__(256) exp_read_kernel(const uint4 *p, size_t n, size_t stride, u32 *sink)
{
    u32 acc = 0;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        const uint4 v = p[i * stride];
        acc += v.x ^ v.y ^ v.z ^ v.w;
    }
    if (acc == 0x12345678u) sink[0] = acc;
}
__global__ void __launch_bounds__(256) exp_write_kernel(u32 *p, size_t n, size_t stride_words)
{
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) p[i * stride_words + 1023] = 0;
}
__global__ void __launch_bounds__(256) exp_spin_kernel(u32 *sink, int iters)
{
    u32 a = threadIdx.x, b = blockIdx.x;
    for (int i = 0; i < iters; i++) {
        a = a * 1664525u + b;
        b = b * 22695477u + a;
    }
    if ((a ^ b) == 0x12345678u) sink[0] = a;
}
// One wave that samples (shader-clock counter, 100 MHz wall counter) pairs at a fixed wall period while other launches run:
// the chip's clock over time across a step (tools/clock_trace.py).
__global__ void __launch_bounds__(64) exp_clock_trace_kernel(unsigned long long *out, int n, int period_ticks)
{
    if (threadIdx.x != 0) return;
    unsigned long long next = __builtin_amdgcn_s_memrealtime();
    for (int i = 0; i < n; i++) {
        unsigned long long w;
        do {
            __builtin_amdgcn_s_sleep(8);
            w = __builtin_amdgcn_s_memrealtime();
        } while (w < next);
        out[2 * i] = __builtin_amdgcn_s_memtime();
        out[2 * i + 1] = w;
        next = w + (unsigned long long)period_ticks;
    }
}
static hipStream_t g_exp_trace_stream = nullptr;
static unsigned long long *g_exp_trace_buf = nullptr;
static int g_exp_trace_n = 0;
extern "C" int vppx_exp_clock_trace_start(vppx_ctx *ctx, int n, int period_us)
{
    VPPX_ENTER(ctx);
    VPPX_PIPE_KEEP(ctx);
    if (!g_exp_trace_stream) VPPX_HIP(hipStreamCreateWithFlags(&g_exp_trace_stream, hipStreamNonBlocking));
    if (g_exp_trace_buf) (void)hipFree(g_exp_trace_buf);
    VPPX_HIP(hipMalloc((void **)&g_exp_trace_buf, (size_t)n * 16));
    g_exp_trace_n = n;
    exp_clock_trace_kernel<<<1, 64, 0, g_exp_trace_stream>>>(g_exp_trace_buf, n, period_us * 100);
    VPPX_CHECK_LAUNCH();
    return 0;
}
extern "C" int vppx_exp_clock_trace_read(vppx_ctx *ctx, unsigned long long *host)
{
    VPPX_ENTER(ctx);
    VPPX_PIPE_KEEP(ctx);
    VPPX_HIP(hipStreamSynchronize(g_exp_trace_stream));
    VPPX_HIP(hipMemcpy(host, g_exp_trace_buf, (size_t)g_exp_trace_n * 16, hipMemcpyDeviceToHost));
    return 0;
}
static int exp_env(const char *name)
{
    const char *e = getenv(name);
    return e ? atoi(e) : 0;
}
static int exp_pre_we(vppx_ctx *ctx, const RsgmGeom &g, const u8 *gl, const u32 *cl, const u32 *cr, void *paths, size_t ncell)
{
    const int mode = exp_env("VPPX_EXP_PRE");
    u32 *sink = (u32 *)ctx->ws[WS_P2LUT].p + 200; // never written (the condition cannot hold)
    const size_t npp = (size_t)g.B * g.Hp * g.Wp;
    if (mode == 1) {
        exp_read_kernel<<<2048, 256, 0, ctx->stream>>>((const uint4 *)cl, npp / 4, 1, sink);
        exp_read_kernel<<<2048, 256, 0, ctx->stream>>>((const uint4 *)cr, npp / 4, 1, sink);
        exp_read_kernel<<<2048, 256, 0, ctx->stream>>>((const uint4 *)gl, npp / 16, 1, sink);
    } else if (mode == 2) {
        exp_read_kernel<<<2048, 256, 0, ctx->stream>>>((const uint4 *)paths, ncell * 2 / 4096, 256, sink);
    } else if (mode == 3) {
        exp_spin_kernel<<<4096, 256, 0, ctx->stream>>>(sink, 20000);
    } else if (mode == 6) {
        exp_write_kernel<<<2048, 256, 0, ctx->stream>>>((u32 *)paths, ncell * 2 / 4096, 1024);
    }
    VPPX_CHECK_LAUNCH();
    return 0;
}
#endif

static int agg_events_create(vppx_ctx *ctx)
{
    if (ctx->agg_ev_created) return 0;
    for (int j = 0; j < 2; j++)
        for (int i = 0; i < vppx_ctx::AGG_RING; i++) {
            VPPX_HIP(hipEventCreate(&ctx->agg_ev[j][i]));
            VPPX_HIP(hipEventCreate(&ctx->we_ev[j][i]));
        }
    ctx->agg_ev_created = true;
    return 0;
}

static int run_aggregation(vppx_ctx *ctx, const VppxRsgmParams &p, const RsgmGeom &g, const u8 *gl, const u32 *cl,
                           const u32 *cr, const u16 *lut_d, int maxp2, const void **vols, int *nvol_out,
                           int *elem_bytes_out, int which, const float *hints = nullptr, const float *validhints = nullptr)
{
    int rc;
    const size_t npp = (size_t)g.B * g.Hp * g.Wp;
    const size_t ncell = npp * g.D;
    int nvol;
    ctx->wsum_route = false;
    if ((rc = lockstep_check(ctx))) return rc; // an earlier fused launch lost its lock step: say so before queueing more
    if (hints && validhints) {
        // --guided (rsgm.py:265-268): the hint pixels' re-weighted cost rows are written out compactly, every other
        // pixel's costs come from the census pair inside the aggregation (guided costs reach 240: u16 path volumes)
        u16 *rows;
        int *gmap;
        void *gp;
        if ((rc = ws_get(ctx, WS_DSI, (size_t)g.B * g.H * g.W * g.D, &rows))) return rc; // (at most every pixel has one)
        if ((rc = ws_get(ctx, WS_GUIDED_MAP, npp + 1, &gmap))) return rc;
        if ((rc = ws_reserve(ctx, WS_PATHS, ncell * 8 * 2, &gp))) return rc;
        if ((rc = rsgm_launch_guided_rows(ctx, g, cl, cr, hints, validhints, gmap, rows, (u32 *)(gmap + npp)))) return rc;
        if ((rc = rsgm_launch_paths(ctx, g.B, g.Hp, g.Wp, g.D, gl, cl, cr, rows, lut_d, p.p1, gp, 2, 0xFF, gmap))) return rc;
        for (int k = 0; k < 8; k++) vols[k] = (const u8 *)gp + (size_t)k * ncell * 2;
        *nvol_out = 8;
        *elem_bytes_out = 2;
        return 0;
    }
    const int elem_bytes = rsgm_paths_elem_bytes(g.D, maxp2);
    // Aggregation layout.  use_vert: -1 (default) = pick by shape, 0 = eight line-parallel paths, 1 = band marching
    // (round-1 experiment), 3 = fused vertical kernel whenever the shape allows it.  The fused kernel wins from 8 frames
    // per launch on (540x960x192, ms per step 8-path / fused: B=4 2.20 / 2.26, B=8 3.74 / 3.27, B=16 6.94 / 5.90,
    // B=32 13.3 / 11.7); a context whose fused launch once lost its lock step never uses it again.
    bool vert3;
    if ((rc = fused_layout_wanted(ctx, g, maxp2, &vert3))) return rc;
    if (!vert3 && ctx->vert3_rest > 0 && which == 0) ctx->vert3_rest--; // resting after a lost lock step
    const bool vert = vert3 || (ctx->use_vert == 1 && elem_bytes == 1 && rsgm_vert_supported(g.D, maxp2) && g.D <= 192);
    ctx->last_vert = vert3 ? 3 : (vert ? 1 : 0);
    void *paths;
    if (vert) {
        // W/E by the line-parallel scan; N/NW/NE and S/SW/SE fused three at a time: register-resident lock-step kernel
        // (sgm_vert3_kernel) or the older band-marching kernel on a side stream (use_vert 1)
        u8 *sv, *gst;
        u16 *gmin;
        if ((rc = ws_reserve(ctx, WS_PATHS, ncell * 2, &paths))) return rc;
        if ((rc = ws_get(ctx, WS_SV, ncell * 2, &sv))) return rc;
        if ((rc = ws_get(ctx, WS_VSTATE, vert3 ? rsgm_vert3_xbuf_bytes(g.B, g.Wp, g.D) : rsgm_vert_state_bytes(g.B, g.Wp, g.D), &gst))) return rc;
        if ((rc = ws_get(ctx, WS_VMIN, vert3 ? 8 : rsgm_vert_min_elems(g.B, g.Wp), &gmin))) return rc;
        // W and E stay on the line-parallel kernel.  (Round 3 built the fused kernels' lane layouts turned by 90 degrees for
        // them -- 16 or 8 rows per wave, the right-image census window kept in registers and shifted by one word per step:
        // 19 instead of 26 instructions per pixel, bit-exact -- and measured 1.88-2.10 ms (16 rows, 168 VGPRs: 2-3 waves per
        // SIMD cannot cover the walk's dependent chain) and 2.6 ms (8 rows: 96 VGPRs only with spills) against 1.94-2.00.)
        // W folded into the sum / WTA pass (sgm_wsum12_kernel): this launch then makes the E lines only
        ctx->wsum_route = vert3 && elem_bytes == 1 && rsgm_wsum_eligible(ctx, g.B, g.Hp, g.Wp, g.D, maxp2, rsgm_device_simds(ctx));
        const int we_dirs = ctx->wsum_route ? 0x10 : 0x11;
        bool we_launched = false; // (launch_vert has run W/E next to its under-filled launch)
        auto launch_we = [&]() -> int {
            // event pairs around this launch too: inside a step it follows a run of small kernels (or the previous step's
            // post stage) and has been seen to take longer than when it is re-launched back to back
            const bool timed = !ctx->capturing;
            if (timed && (rc = agg_events_create(ctx))) return rc;
            const int slot = (int)(ctx->we_calls % vppx_ctx::AGG_RING);
#ifdef VPPX_EXPERIMENT
            if ((rc = exp_pre_we(ctx, g, gl, cl, cr, paths, ncell))) return rc;
            if (exp_env("VPPX_EXP_TWICE") && (rc = rsgm_launch_paths(ctx, g.B, g.Hp, g.Wp, g.D, gl, cl, cr, nullptr, lut_d, p.p1, paths, 1, 0x11))) return rc;
#endif
            if (timed) VPPX_HIP(hipEventRecord(ctx->we_ev[0][slot], ctx->stream));
            const int r = rsgm_launch_paths(ctx, g.B, g.Hp, g.Wp, g.D, gl, cl, cr, nullptr, lut_d, p.p1, paths, 1, we_dirs);
            if (timed) {
                VPPX_HIP(hipEventRecord(ctx->we_ev[1][slot], ctx->stream));
                ctx->we_calls++;
            }
            return r;
        };
        auto launch_vert = [&](hipStream_t st) -> int {
            if (!vert3) return rsgm_launch_vert(ctx, st, g.B, g.Hp, g.Wp, g.D, gl, cl, cr, lut_d, p.p1, sv, gst, gmin);
            if (!ctx->vert3_err) { // the word a wave that gives up reports through: no fused launch without it
                if (hipHostMalloc((void **)&ctx->vert3_err, 64, hipHostMallocMapped) != hipSuccess) {
                    ctx->vert3_err = nullptr;
                    (void)hipGetLastError();
                    vppx_set_error("could not allocate the pinned status word of the fused aggregation kernel");
                    return VPPX_E_HIP;
                }
                ctx->vert3_err[0] = 0;
            }
            // event pairs around the fused launch: what bench.py prices as the dominant kernel
            const bool timed = !ctx->capturing && st == ctx->stream;
            if (timed && (rc = agg_events_create(ctx))) return rc;
            const int slot = (int)(ctx->agg_calls % vppx_ctx::AGG_RING);
            if (timed) VPPX_HIP(hipEventRecord(ctx->agg_ev[0][slot], st));
            unsigned *err_dev;
            {
                const bool fresh = ctx->ws[WS_V3ERR].p == nullptr;
                if ((rc = ws_get(ctx, WS_V3ERR, (size_t)4, &err_dev))) return rc;
                if (fresh) VPPX_HIP(hipMemsetAsync(err_dev, 0, 16, st));
            }
            // A batch of whole rounds + a remainder runs as two launches, and W/E runs NEXT to a launch that leaves most of an
            // XCD's SIMDs idle (rsgm_vert3_plan): the remainder, or a batch well below one round.  W/E needs nothing of the
            // vertical kernel (other volumes, the same read-only images), so the order is free; next to a FULL round it costs
            // more than it hides (NOTEBOOK: 6.1 -> 7.1 ms), next to 78 waves on 128 SIMDs it has the idle ones.
            int whole = 0;
            bool rest_under = false;
            // (which == 2, the timing helper's "lock-step launches only": the same plan, hence the same kernels, without W/E)
            if (which != 1 && ctx->knobs.we_next && st == ctx->stream && !we_launched) rsgm_vert3_plan(ctx, g.B, g.Wp, g.D, &whole, &rest_under);
            int r;
            if (!rest_under) {
                r = rsgm_launch_vert3(ctx, st, g.B, g.Hp, g.Wp, g.D, gl, cl, cr, lut_d, p.p1, sv, (u32 *)gst, ctx->vert3_err, err_dev);
            } else {
                if (whole > 0 &&
                    (r = rsgm_launch_vert3_range(ctx, st, g.B, 0, whole, g.Hp, g.Wp, g.D, gl, cl, cr, lut_d, p.p1, sv, (u32 *)gst, ctx->vert3_err, err_dev, false))) return r;
                if (which == 0) {
                    VPPX_HIP(hipEventRecord(ctx->ev_fork, st));
                    VPPX_HIP(hipStreamWaitEvent(ctx->stream2, ctx->ev_fork, 0));
                    ctx->stream = ctx->stream2;
                    ctx->we_beside_vert = true;
                    r = launch_we();
                    ctx->we_beside_vert = false;
                    ctx->stream = st;
                    if (r) return r;
                    VPPX_HIP(hipEventRecord(ctx->ev_join, ctx->stream2));
                }
                r = rsgm_launch_vert3_range(ctx, st, g.B, whole, g.B - whole, g.Hp, g.Wp, g.D, gl, cl, cr, lut_d, p.p1, sv, (u32 *)gst, ctx->vert3_err, err_dev, true);
                // the pair closes behind the last lock-step launch, BEFORE the join: it must not contain W/E's tail
                if (timed) {
                    VPPX_HIP(hipEventRecord(ctx->agg_ev[1][slot], st));
                    ctx->agg_calls++;
                }
                if (which == 0) {
                    VPPX_HIP(hipStreamWaitEvent(st, ctx->ev_join, 0));
                    we_launched = true;
                }
                return r;
            }
            if (timed) {
                VPPX_HIP(hipEventRecord(ctx->agg_ev[1][slot], st));
                ctx->agg_calls++;
            }
            return r;
        };
        if (which == 0 && vert3) {
            // One after the other: both launches fill the chip, two streams only interleave them (measured: no gain).
            // Whichever launch follows the front stage finds the gray / census images cold (written by another launch; the
            // first reader fetches them from HBM, later ones hit the memory-side cache) and its chains wait at every new
            // line.  The W/E launch pays 0.5-0.65 ms for going first (2.4-2.6 ms instead of 1.95 back to back;
            // tools/we_probe.py), the fused vertical kernel 0.2-0.3 ms: it goes first (round 4: bench step 9.66 -> 9.45 ms
            // on the same box).  Reading the images once in a launch of its own has the same effect (VPPX_EXP_PRE=1 of an
            // experiment build).  (Also tried in round 4, bit-exact, not kept: the vertical kernel adding W's and E's bytes to
            // its two sums -- 3 whole-line loads per lane and row, prefetched a row ahead -- so that the sum kernel reads
            // two volumes: sum / WTA 2.46 -> 2.09 ms, but the lock-step kernel 3.5 -> 4.55 ms whatever the loads'
            // distance, cache policy or target (in place or not): HBM-latency loads in its CUs' miss queues hold up the
            // L2-hit operand loads every row depends on.)
#ifdef VPPX_EXPERIMENT
            const bool we_first = exp_env("VPPX_EXP_ORDER") != 0; // the order of rounds 2-3
#else
            const bool we_first = false;
#endif
            if (we_first) {
                if ((rc = launch_we())) return rc;
                we_launched = true;
                if ((rc = launch_vert(ctx->stream))) return rc;
            } else {
                if ((rc = launch_vert(ctx->stream))) return rc;
                // VPPX_VARIANT=pipe_mid (experiment builds; measured slower at D = 192 and at D = 256): the NEXT call's front stage starts here, next to the W/E launch and the sum / WTA
                // kernel (it used to start after the whole aggregation).  The lock-step kernel is the one that suffers from
                // neighbours and it is done; the images W/E still reads belong to this call's set of the two alternating
                // sets (rsgm_core), which the next front stage does not touch.
                if (ctx->pipe_call && !ctx->pipe_early && ctx->pipe_mid) {
                    VPPX_HIP(hipEventRecord(ctx->ev_agg_done, ctx->stream));
                    ctx->have_agg_done = true;
                    ctx->agg_done_recorded = true;
                }
                if (!we_launched && (rc = launch_we())) return rc;
            }
        } else if (which == 0) {
            VPPX_HIP(hipEventRecord(ctx->ev_fork, ctx->stream));
            VPPX_HIP(hipStreamWaitEvent(ctx->stream2, ctx->ev_fork, 0));
            hipStream_t main_stream = ctx->stream;
            ctx->stream = ctx->stream2;
            rc = rsgm_launch_paths(ctx, g.B, g.Hp, g.Wp, g.D, gl, cl, cr, nullptr, lut_d, p.p1, paths, 1, 0x11);
            ctx->stream = main_stream;
            if (rc) return rc;
            VPPX_HIP(hipEventRecord(ctx->ev_join, ctx->stream2));
            if ((rc = launch_vert(ctx->stream))) return rc;
            VPPX_HIP(hipStreamWaitEvent(ctx->stream, ctx->ev_join, 0));
        } else if (which == 1) {
            if ((rc = launch_we())) return rc;
        } else {
            if ((rc = launch_vert(ctx->stream))) return rc;
        }
        vols[0] = paths;
        vols[1] = (const u8 *)paths + ncell;
        vols[2] = sv;
        vols[3] = sv + ncell;
        nvol = 4;
    } else {
        if ((rc = ws_reserve(ctx, WS_PATHS, ncell * 8 * elem_bytes, &paths))) return rc;
        if ((rc = agg_events_create(ctx))) return rc;
        if (ctx->capturing) { // event records stay out of a captured graph
            if ((rc = rsgm_launch_paths(ctx, g.B, g.Hp, g.Wp, g.D, gl, cl, cr, nullptr, lut_d, p.p1, paths, elem_bytes, 0xFF))) return rc;
        } else {
            const int slot = (int)(ctx->agg_calls % vppx_ctx::AGG_RING);
            VPPX_HIP(hipEventRecord(ctx->agg_ev[0][slot], ctx->stream));
            if ((rc = rsgm_launch_paths(ctx, g.B, g.Hp, g.Wp, g.D, gl, cl, cr, nullptr, lut_d, p.p1, paths, elem_bytes, 0xFF))) return rc;
            VPPX_HIP(hipEventRecord(ctx->agg_ev[1][slot], ctx->stream));
            ctx->agg_calls++;
        }
        for (int k = 0; k < 8; k++) vols[k] = (const u8 *)paths + (size_t)k * ncell * elem_bytes;
        nvol = 8;
    }
    *nvol_out = nvol;
    *elem_bytes_out = elem_bytes;
    return 0;
}

// ---------------------------------------------------------------------------------------
// rSGM on device buffers (core of compute_rsgm, rsgm.py:250-294)
// ---------------------------------------------------------------------------------------
// ---- cross-call pipelining of the front stage (vppx_set_pipeline) ----
static bool pipeline_applies(const vppx_ctx *ctx)
{
    return ctx->pipeline && !ctx->capturing && !ctx->stage_timing && !ctx->is_child && !ctx->graph_mode && ctx->nsub <= 1;
}
// From here on ctx->stream is the front stream.  It waits for (1) the previous pipelined call's aggregation, the last
// reader of the census / gray / pattern buffers the front stage rewrites (the first pipelined call waits for everything
// queued on the launch stream so far), and (2) the inputs: the caller's inputs-ready event when one was given for this
// call, else an event recorded on the launch stream right now, i.e. everything the caller queued before the call.
static int front_begin(vppx_ctx *ctx)
{
    if (!ctx->stream_front) {
        VPPX_HIP(hipStreamCreateWithFlags(&ctx->stream_front, hipStreamNonBlocking));
        VPPX_HIP(hipEventCreateWithFlags(&ctx->ev_agg_done, hipEventDisableTiming));
        VPPX_HIP(hipEventCreateWithFlags(&ctx->ev_front_done, hipEventDisableTiming));
        VPPX_HIP(hipEventCreateWithFlags(&ctx->ev_inputs_auto, hipEventDisableTiming));
    }
    if (!ctx->have_agg_done) {
        VPPX_HIP(hipEventRecord(ctx->ev_agg_done, ctx->stream));
        ctx->have_agg_done = true;
        VPPX_HIP(hipStreamWaitEvent(ctx->stream_front, ctx->ev_agg_done, 0)); // covers the inputs as well
        if (ctx->inputs_ev) VPPX_HIP(hipStreamWaitEvent(ctx->stream_front, (hipEvent_t)ctx->inputs_ev, 0));
    } else {
        VPPX_HIP(hipStreamWaitEvent(ctx->stream_front, ctx->ev_agg_done, 0));
        if (ctx->inputs_ev) {
            VPPX_HIP(hipStreamWaitEvent(ctx->stream_front, (hipEvent_t)ctx->inputs_ev, 0));
        } else {
            VPPX_HIP(hipEventRecord(ctx->ev_inputs_auto, ctx->stream));
            VPPX_HIP(hipStreamWaitEvent(ctx->stream_front, ctx->ev_inputs_auto, 0));
        }
    }
    ctx->inputs_ev = nullptr;
    ctx->main_saved = ctx->stream;
    ctx->stream = ctx->stream_front;
    ctx->front_active = true;
    return 0;
}
// Back to the launch stream, which from now on waits for the front stage: whatever is queued on it later (this call's
// aggregation, the caller's own work) sees the front stage's results.
static int front_end(vppx_ctx *ctx)
{
    if (!ctx->front_active) return 0;
    hipStream_t front = ctx->stream;
    ctx->stream = ctx->main_saved;
    ctx->front_active = false;
    VPPX_HIP(hipEventRecord(ctx->ev_front_done, front));
    // While the launch stream would only wait for the tail of the front stage, it does what does not need that tail: the
    // exchange records of the next lock-step launch are cleared (behind the last one, which is queued on this stream), and
    // the occlusion mask goes to the caller as soon as the occlusion stage is through.
    if (ctx->xbuf_last && !ctx->xbuf_cleared && ctx->xbuf_last == ctx->ws[WS_VSTATE].p) { // (still the live workspace buffer)
        VPPX_HIP(hipMemsetAsync(ctx->xbuf_last, 0, ctx->xbuf_last_bytes, ctx->stream));
        ctx->xbuf_cleared = true;
    }
    // what the caller wanted of the front stage's results, delivered in launch-stream order (and before this call's
    // aggregation, whose completion releases the library-owned buffers to the next front stage)
    if (ctx->occ_done_recorded) {
        bool any = false;
        for (int i = 0; i < ctx->n_pipe_copy; i++) any = any || ctx->pipe_copy[i].early;
        if (any) VPPX_HIP(hipStreamWaitEvent(ctx->stream, ctx->ev_occ_done, 0));
        for (int i = 0; i < ctx->n_pipe_copy; i++)
            if (ctx->pipe_copy[i].early)
                VPPX_HIP(hipMemcpyAsync(ctx->pipe_copy[i].dst, ctx->pipe_copy[i].src, ctx->pipe_copy[i].bytes, hipMemcpyDeviceToDevice, ctx->stream));
    }
    VPPX_HIP(hipStreamWaitEvent(ctx->stream, ctx->ev_front_done, 0));
    for (int i = 0; i < ctx->n_pipe_copy; i++)
        if (!(ctx->occ_done_recorded && ctx->pipe_copy[i].early))
            VPPX_HIP(hipMemcpyAsync(ctx->pipe_copy[i].dst, ctx->pipe_copy[i].src, ctx->pipe_copy[i].bytes, hipMemcpyDeviceToDevice, ctx->stream));
    ctx->n_pipe_copy = 0;
    ctx->occ_done_recorded = false;
    if (ctx->pipe_call && ctx->pipe_early) {
        // Few frames per call: the aggregation is a handful of long dependent chains that leave most of the GPU idle, so
        // the NEXT call's front stage may start right now, next to it.  From here on nothing of this call reads what a front
        // stage writes except the gray / census images its aggregation takes, and those alternate between two sets by call
        // parity; the set this call uses is rewritten by the front stage of call k+2, which waits for THIS event of call
        // k+1 -- recorded on the in-order launch stream behind call k's aggregation.
        VPPX_HIP(hipEventRecord(ctx->ev_agg_done, ctx->stream));
        ctx->have_agg_done = true;
    }
    return 0;
}
struct FrontGuard { // error paths: never leave the context on the front stream
    vppx_ctx *ctx;
    ~FrontGuard()
    {
        if (ctx->front_active) {
            ctx->stream = ctx->main_saved;
            ctx->front_active = false;
        }
        ctx->pipe_call = false;
        ctx->n_pipe_copy = 0;
        ctx->occ_done_recorded = false;
    }
};

static int rsgm_core(vppx_ctx *ctx, const VppxRsgmParams &p, const RsgmGeom &g, const u8 *left, const u8 *left_vpp,
                     const u8 *right_vpp, float *disp_out, const float *hints = nullptr, const float *validhints = nullptr)
{
    int rc;
    const size_t npp = (size_t)g.B * g.Hp * g.Wp;
    const size_t ncell = npp * g.D;
    u8 *gl;
    u32 *cl, *cr_raw;
    // pipelined calls alternate between two sets of the images the aggregation reads (see front_end); with fewer than 8
    // frames per call (8-path layout, a GPU mostly idle during the aggregation) the next front stage starts early
    const bool alt = ctx->pipe_call && (ctx->pipe_parity & 1);
    if (ctx->pipe_call) ctx->pipe_parity ^= 1;
    {
        // (the next call's front stage starts next to this call's aggregation only when that is the line-parallel kernel: the
        // lock-step kernel suffers from neighbours)
        bool fused = false;
        if (ctx->pipe_call && g.B < 8) {
            u16 lut_tmp[256];
            int mp2 = 0;
            p2_lut_host(p, lut_tmp, &mp2);
            if ((rc = fused_layout_wanted(ctx, g, mp2, &fused))) return rc;
        }
        ctx->pipe_early = ctx->pipe_call && g.B < 8 && !fused;
    }
    if ((rc = ws_get(ctx, alt ? WS_GRAY_L2 : WS_GRAY_L, npp, &gl))) return rc;
    if ((rc = ws_get(ctx, alt ? WS_CENSUS_L2 : WS_CENSUS_L, npp, &cl))) return rc;
    if ((rc = ws_get(ctx, alt ? WS_CENSUS_R2 : WS_CENSUS_R, npp + 512, &cr_raw))) return rc; // 512-word guard in front (x-d < 0 reads)
    u32 *cr = cr_raw + 512;
    ctx->last_gl = gl; ctx->last_cl = cl; ctx->last_cr = cr;
    // pad + gray of the three images and the census of the patterned pair: one launch, the pair's gray images stay in LDS
    if ((rc = rsgm_launch_pad_gray_census(ctx, g, left, left_vpp, right_vpp, gl, cl, cr))) return rc;
    stage_mark(ctx, ST_PAD_GRAY);
    stage_mark(ctx, ST_CENSUS);
    if ((rc = front_end(ctx))) return rc; // pipelined call: the front stage ends here

    u16 *lut_d;
    if ((rc = ws_get(ctx, WS_P2LUT, 256, &lut_d))) return rc;
    if (!ctx->lut_valid || ctx->lut_p2min != p.p2min || ctx->lut_gamma != p.gamma || ctx->lut_alpha != p.alpha) {
        if (ctx->capturing) { vppx_set_error("penalty table changed during graph capture"); return VPPX_E_HIP; }
        p2_lut_host(p, ctx->lut_host, &ctx->lut_maxp2);
        VPPX_HIP(hipMemcpyAsync(lut_d, ctx->lut_host, sizeof(ctx->lut_host), hipMemcpyHostToDevice, ctx->stream));
        ctx->lut_p2min = p.p2min; ctx->lut_gamma = p.gamma; ctx->lut_alpha = p.alpha;
        ctx->lut_valid = true;
    }
    const int maxp2 = ctx->lut_maxp2;
    // per-path values are bounded by Cmax + P2max (L_r - min L_r <= P2): bytes suffice when that is < 256
    const void *vols[8];
    int nvol = 0, elem_bytes = 1;
    ctx->agg_done_recorded = false;
    if ((rc = run_aggregation(ctx, p, g, gl, cl, cr, lut_d, maxp2, vols, &nvol, &elem_bytes, 0, hints, validhints))) return rc;
    if (ctx->pipe_call && !ctx->pipe_early && !ctx->agg_done_recorded) { // the next pipelined call's front stage may start now
        VPPX_HIP(hipEventRecord(ctx->ev_agg_done, ctx->stream));
        ctx->have_agg_done = true;
    }
    stage_mark(ctx, ST_AGGREGATE);
    ctx->last_B = g.B; ctx->last_Hp = g.Hp; ctx->last_Wp = g.Wp; ctx->last_D = g.D; ctx->last_rp = p; ctx->have_last = true;
    ctx->last_guided = hints && validhints;

    float *dl0, *dl1, *dr0, *dr1;
    if ((rc = ws_get(ctx, WS_DISP_L0, npp, &dl0))) return rc;
    if ((rc = ws_get(ctx, WS_DISP_L1, npp, &dl1))) return rc;
    if ((rc = ws_get(ctx, WS_DISP_R0, npp, &dr0))) return rc;
    if ((rc = ws_get(ctx, WS_DISP_R1, npp, &dr1))) return rc;
    const u32 fu = uniq_factor(p.uniqueness);
    // rsgm.py:141-142: matchWTA_SSE + subPixelRefine(.., 0) are always applied to the left map
    if (ctx->wsum_route) // W is made, summed and decided in one pass; vols[0] (W) holds nothing of this call
        rc = rsgm_launch_wsum(ctx, g.B, g.Hp, g.Wp, g.D, gl, cl, cr, lut_d, p.p1, vols[1], vols[2], vols[3], dl0, dr0, fu);
    else
        rc = rsgm_launch_sum_wta_lr(ctx, g.B, g.Hp, g.Wp, g.D, vols, nvol, elem_bytes, dl0, dr0, fu, 1,
                                    (hints && validhints) ? 0 : 24 + maxp2);
    if (rc < 0) return rc;
    if (rc == 0) {
        stage_mark(ctx, ST_SUM_WTA);
        ctx->last_sum_nvol = nvol; ctx->last_sum_D = g.D; ctx->last_sum_B = g.B;
    } else {
        ctx->last_sum_nvol = 0;
        u16 *S;
        if ((rc = ws_get(ctx, WS_S, ncell, &S))) return rc;
        if ((rc = rsgm_launch_sum_wta(ctx, g.B, g.Hp, g.Wp, g.D, vols[0], elem_bytes, nullptr, S, dl0, fu, 1))) return rc;
        stage_mark(ctx, ST_SUM_WTA);
        if ((rc = rsgm_launch_wta_right_t(ctx, g.B, g.Hp, g.Wp, g.D, S, dr0, fu))) return rc;
        stage_mark(ctx, ST_WTA_RIGHT);
    }
    if ((rc = rsgm_launch_median_interp_clip(ctx, g.B, g.Hp, g.Wp, dl0, dl1, dr0, dr1))) return rc;
    stage_mark(ctx, ST_MEDIAN_INTERP);
    { float *t = dl0; dl0 = dl1; dl1 = t; t = dr0; dr0 = dr1; dr1 = t; } // results are in the *1 buffers

    const size_t np = (size_t)g.B * g.H * g.W;
    if ((rc = rsgm_launch_post(ctx, g, dl0, dr0, p.subpixel, disp_out))) return rc;
    // fused layout: should this call's lock-step launch have given up, its output becomes NaN before anything queued
    // behind the call can read it (the host learns of it through vppx_status / vppx_synchronize / the next call)
    if (ctx->last_vert == 3 && ctx->ws[WS_V3ERR].p &&
        (rc = rsgm_launch_void_if_lost(ctx, disp_out, np, (const unsigned *)ctx->ws[WS_V3ERR].p, ctx->v3.serial))) return rc;
    stage_mark(ctx, ST_POST);
    return 0;
}

static int check_frames(int B, int H, int W, int C)
{
    if (B <= 0 || H <= 0 || W <= 0) { vppx_set_error("bad shape B=%d H=%d W=%d", B, H, W); return VPPX_E_INVALID_ARG; }
    if (C != 1 && C != 3) { vppx_set_error("channels must be 1 or 3 (got %d)", C); return VPPX_E_INVALID_ARG; }
    if (H < 5 || W < 5) { vppx_set_error("frame too small (%dx%d)", H, W); return VPPX_E_INVALID_ARG; }
    return 0;
}

// A guided batch keeps 8 u16 path volumes (16 bytes per cell): one whose volumes would exceed the budget (48 GiB;
// VPPX_GUIDED_PART_MB sets another) runs in parts of as many frames as fit (at least one).  (8 frames of 1536x2048x256
// would need 103 GB.)
static int guided_frames_per_part(const vppx_ctx *ctx, int H, int W, int C, int dmax)
{
    RsgmGeom g1;
    make_geom(1, H, W, C, dmax, g1);
    const unsigned long long per = (unsigned long long)g1.Hp * g1.Wp * g1.D * 16ull;
    const unsigned long long n = ctx->knobs.guided_part_bytes / per;
    return n < 1 ? 1 : (n > (unsigned long long)INT_MAX ? INT_MAX : (int)n);
}

extern "C" int vppx_rsgm_dev(vppx_ctx *ctx, const VppxRsgmParams *p, int B, int H, int W, int C, const uint8_t *left,
                             const uint8_t *left_vpp, const uint8_t *right_vpp, const float *hints,
                             const float *validhints, float *disp_out)
{
    int rc;
    VPPX_ENTER(ctx);
    routes_reset(ctx);
    if ((rc = lockstep_check(ctx))) return rc;
    if (!p || !left || !left_vpp || !right_vpp || !disp_out) { vppx_set_error("vppx_rsgm: NULL argument"); return VPPX_E_INVALID_ARG; }
    if ((rc = check_frames(B, H, W, C))) return rc;
    if ((rc = check_rsgm_params(*p))) return rc;
    if ((hints == nullptr) != (validhints == nullptr)) { hints = nullptr; validhints = nullptr; } // rsgm.py:265 needs both
    RsgmGeom g;
    stage_begin(ctx);
    const int q = hints ? guided_frames_per_part(ctx, H, W, C, p->dmax) : B;
    if (q >= B) {
        make_geom(B, H, W, C, p->dmax, g);
        return rsgm_core(ctx, *p, g, left, left_vpp, right_vpp, disp_out, hints, validhints);
    }
    const size_t fpx = (size_t)H * W;
    for (int lo = 0; lo < B; lo += q) {
        const int nb = B - lo < q ? B - lo : q;
        make_geom(nb, H, W, C, p->dmax, g);
        ctx->stage_append = lo > 0;
        rc = rsgm_core(ctx, *p, g, left + (size_t)lo * fpx * C, left_vpp + (size_t)lo * fpx * C, right_vpp + (size_t)lo * fpx * C,
                       disp_out + (size_t)lo * fpx, hints + (size_t)lo * fpx, validhints + (size_t)lo * fpx);
        ctx->stage_append = false;
        if (rc) return rc;
    }
    return 0;
}

extern "C" int vppx_rsgm_post_dev(vppx_ctx *ctx, int B, int H, int W, const float *disp_l_pad, const float *disp_r_pad,
                                  int subpixel, float *disp_out)
{
    int rc;
    VPPX_ENTER(ctx);
    if (!disp_l_pad || !disp_r_pad || !disp_out) { vppx_set_error("vppx_rsgm_post: NULL argument"); return VPPX_E_INVALID_ARG; }
    if ((rc = check_frames(B, H, W, 1))) return rc;
    RsgmGeom g;
    make_geom(B, H, W, 1, 64, g);
    return rsgm_launch_post(ctx, g, disp_l_pad, disp_r_pad, subpixel, disp_out);
}

// Stage entries of the three fused kernels that have no pyrSGM-style stage of their own.  Each one queues the launcher
// rsgm_core / run_aggregation call, on the caller's buffers; like vppx_rsgm_post_dev they keep no record of the call (no
// route names, no last_gl / last_cl / last_cr) and leave the workspace alone.
extern "C" int vppx_rsgm_front_dev(vppx_ctx *ctx, int B, int H, int W, int C, const uint8_t *left, const uint8_t *left_vpp,
                                   const uint8_t *right_vpp, uint8_t *gray_left, uint32_t *census_l, uint32_t *census_r)
{
    int rc;
    VPPX_ENTER(ctx);
    if (!left || !left_vpp || !right_vpp || !gray_left || !census_l || !census_r) {
        vppx_set_error("vppx_rsgm_front: NULL argument");
        return VPPX_E_INVALID_ARG;
    }
    if ((rc = check_frames(B, H, W, C))) return rc;
    RsgmGeom g;
    make_geom(B, H, W, C, 64, g);
    return rsgm_launch_pad_gray_census(ctx, g, left, left_vpp, right_vpp, gray_left, census_l, census_r);
}

extern "C" int vppx_rsgm_guided_rows_dev(vppx_ctx *ctx, int B, int H, int W, int dmax, const uint32_t *census_l,
                                         const uint32_t *census_r, const float *hints, const float *validhints, int32_t *gmap,
                                         uint16_t *rows, uint32_t *count)
{
    int rc;
    VPPX_ENTER(ctx);
    if (!census_l || !census_r || !hints || !validhints || !gmap || !rows || !count) {
        vppx_set_error("vppx_rsgm_guided_rows: NULL argument");
        return VPPX_E_INVALID_ARG;
    }
    if ((rc = check_frames(B, H, W, 1))) return rc;
    VppxRsgmParams p;
    vppx_rsgm_params_default(&p);
    p.dmax = dmax;
    if ((rc = check_rsgm_params(p))) return rc;
    RsgmGeom g;
    make_geom(B, H, W, 1, dmax, g);
    return rsgm_launch_guided_rows(ctx, g, census_l, census_r, hints, validhints, gmap, rows, count);
}

extern "C" int vppx_rsgm_mid_dev(vppx_ctx *ctx, int B, int Hp, int Wp, const float *disp_l, const float *disp_r, float *out_l,
                                 float *out_r)
{
    VPPX_ENTER(ctx);
    if (!disp_l || !disp_r || !out_l || !out_r) { vppx_set_error("vppx_rsgm_mid: NULL argument"); return VPPX_E_INVALID_ARG; }
    if (B <= 0 || Hp < 16 || Wp < 16 || Hp % 16 != 0 || Wp % 16 != 0) {
        vppx_set_error("vppx_rsgm_mid: padded maps are [B][Hp][Wp] with Hp, Wp multiples of 16 (got B=%d Hp=%d Wp=%d)", B, Hp, Wp);
        return VPPX_E_INVALID_ARG;
    }
    return rsgm_launch_median_interp_clip(ctx, B, Hp, Wp, disp_l, out_l, disp_r, out_r);
}

extern "C" int vppx_rsgm_host(vppx_ctx *ctx, const VppxRsgmParams *p, int B, int H, int W, int C, const uint8_t *left,
                              const uint8_t *left_vpp, const uint8_t *right_vpp, const float *hints,
                              const float *validhints, float *disp_out)
{
    int rc;
    VPPX_ENTER(ctx);
    if (!p || !left || !left_vpp || !right_vpp || !disp_out) { vppx_set_error("vppx_rsgm: NULL argument"); return VPPX_E_INVALID_ARG; }
    if ((rc = check_frames(B, H, W, C))) return rc;
    const size_t nb = (size_t)B * H * W * C;
    void *dl, *dlv, *drv, *dout;
    if ((rc = upload(ctx, WS_STAGE_A, left, nb, &dl))) return rc;
    if ((rc = upload(ctx, WS_STAGE_B, left_vpp, nb, &dlv))) return rc;
    if ((rc = upload(ctx, WS_STAGE_C, right_vpp, nb, &drv))) return rc;
    if ((rc = ws_reserve(ctx, WS_STAGE_D, (size_t)B * H * W * sizeof(float), &dout))) return rc;
    void *dh = nullptr, *dv = nullptr;
    if (hints && validhints) {
        if ((rc = upload(ctx, WS_STAGE_E, hints, (size_t)B * H * W * sizeof(float), &dh))) return rc;
        if ((rc = upload(ctx, WS_STAGE_F, validhints, (size_t)B * H * W * sizeof(float), &dv))) return rc;
    }
    for (int attempt = 0;; attempt++) {
        const unsigned serial_before = ctx->v3.serial; // fused launches up to here belong to earlier (asynchronous) calls
        if ((rc = vppx_rsgm_dev(ctx, p, B, H, W, C, (const u8 *)dl, (const u8 *)dlv, (const u8 *)drv, (const float *)dh, (const float *)dv, (float *)dout))) return rc;
        if ((rc = download(ctx, disp_out, dout, (size_t)B * H * W * sizeof(float)))) return rc;
        VPPX_HIP(hipStreamSynchronize(ctx->stream));
        // A synchronous entry point knows whether ITS aggregation lost the lock step: it runs again on the line-parallel
        // kernel (the context has just moved there) instead of returning void disparities.  A mark left by an EARLIER
        // asynchronous fused call is not this call's to swallow: it is reported (once, VPPX_E_HIP), as the header says.
        if ((rc = lockstep_check(ctx)) == 0) break;
        const unsigned s = ctx->lockstep_last_serial;
        const bool mine = (unsigned)(s - serial_before - 1u) < (unsigned)(ctx->v3.serial - serial_before); // serial_before < s <= now (mod 2^32)
        if (!mine || attempt > 0) return rc;
    }
    return 0;
}

// ---------------------------------------------------------------------------------------
// VPP
// ---------------------------------------------------------------------------------------
static int check_vpp_params(const VppxVppParams &p)
{
    if (p.method != VPPX_METHOD_RND && p.method != VPPX_METHOD_MAXDIST) {
        vppx_set_error("method must be \"rnd\" or \"maxDistance\"");
        return VPPX_E_METHOD;
    }
    return 0;
}

extern "C" int vppx_vpp_dev(vppx_ctx *ctx, const VppxVppParams *p, int B, int H, int W, int C, uint8_t *l, uint8_t *r,
                            const float *g, const uint8_t *g_occ, const float *filled_g, int64_t *n_hints_dev)
{
    int rc;
    VPPX_ENTER(ctx);
    if (!p || !l || !r || !g) { vppx_set_error("vppx_vpp: NULL argument"); return VPPX_E_INVALID_ARG; }
    if (B <= 0 || H <= 0 || W <= 0) { vppx_set_error("bad shape B=%d H=%d W=%d", B, H, W); return VPPX_E_INVALID_ARG; }
    if ((rc = check_vpp_params(*p))) return rc;
    front_routes_reset(ctx);
    VppGeom vg = {B, H, W, C};
    stage_begin(ctx);
    if (p->use_bilateral_patch && !filled_g) {
        float *fg;
        if ((rc = ws_get(ctx, WS_FILLED_G, (size_t)B * H * W, &fg))) return rc;
        if ((rc = vpp_launch_bilateral_fill(ctx, *p, vg, l, g, fg))) return rc; // l is still un-patterned here
        filled_g = fg;
    }
    ctx->front_lds_budget = 64 * 1024; // (no sum / WTA kernel of a previous part next to this)
    return vpp_launch(ctx, *p, vg, l, r, g, g_occ, filled_g, n_hints_dev, nullptr);
}

extern "C" int vppx_vpp_host(vppx_ctx *ctx, const VppxVppParams *p, int B, int H, int W, int C, uint8_t *l, uint8_t *r,
                             const float *g, const uint8_t *g_occ, const float *filled_g, int64_t *n_hints)
{
    int rc;
    VPPX_ENTER(ctx);
    if (!p || !l || !r || !g) { vppx_set_error("vppx_vpp: NULL argument"); return VPPX_E_INVALID_ARG; }
    if (B <= 0 || H <= 0 || W <= 0) { vppx_set_error("bad shape B=%d H=%d W=%d", B, H, W); return VPPX_E_INVALID_ARG; }
    const size_t nb = (size_t)B * H * W * C, np = (size_t)B * H * W;
    void *dl, *dr, *dg, *docc = nullptr, *dfg = nullptr, *dn;
    if ((rc = upload(ctx, WS_STAGE_A, l, nb, &dl))) return rc;
    if ((rc = upload(ctx, WS_STAGE_B, r, nb, &dr))) return rc;
    if ((rc = upload(ctx, WS_STAGE_C, g, np * sizeof(float), &dg))) return rc;
    if (g_occ && (rc = upload(ctx, WS_STAGE_D, g_occ, np, &docc))) return rc;
    if (filled_g && (rc = upload(ctx, WS_STAGE_E, filled_g, np * sizeof(float), &dfg))) return rc;
    if ((rc = ws_reserve(ctx, WS_NHINTS, (size_t)B * sizeof(int64_t), &dn))) return rc;
    if ((rc = vppx_vpp_dev(ctx, p, B, H, W, C, (u8 *)dl, (u8 *)dr, (const float *)dg, (const u8 *)docc, (const float *)dfg, (int64_t *)dn))) return rc;
    if ((rc = download(ctx, l, dl, nb))) return rc;
    if ((rc = download(ctx, r, dr, nb))) return rc;
    std::vector<int64_t> nh(B);
    if ((rc = download(ctx, nh.data(), dn, (size_t)B * sizeof(int64_t)))) return rc;
    VPPX_HIP(hipStreamSynchronize(ctx->stream));
    if (n_hints) memcpy(n_hints, nh.data(), (size_t)B * sizeof(int64_t));
    return 0;
}

extern "C" int vppx_vpp_last_draws(vppx_ctx *ctx, int B, uint64_t *draws)
{
    int rc;
    VPPX_ENTER(ctx);
    if (!draws || B <= 0 || !ctx->ws[WS_FRAME_TOT].p || ctx->ws[WS_FRAME_TOT].cap < (size_t)B * 16) {
        vppx_set_error("vppx_vpp_last_draws: no VPP call with B >= %d has run", B);
        return VPPX_E_INVALID_ARG;
    }
    std::vector<unsigned long long> tot((size_t)B * 2);
    VPPX_HIP(hipMemcpyAsync(tot.data(), ctx->ws[WS_FRAME_TOT].p, tot.size() * 8, hipMemcpyDeviceToHost, ctx->stream));
    VPPX_HIP(hipStreamSynchronize(ctx->stream));
    for (int f = 0; f < B; f++) draws[f] = tot[2 * f];
    return 0;
}

extern "C" int vppx_srand(vppx_ctx *ctx, uint32_t seed)
{
    if (!ctx) { vppx_set_error("context is NULL"); return VPPX_E_NO_DEVICE; }
    ctx->rnd_seed = seed;
    ctx->rnd_consumed = 0;
    return 0;
}

// the context's libc-like stream position (what libc keeps in its global rand() state)
extern "C" int vppx_rand_state(vppx_ctx *ctx, uint32_t *seed, uint64_t *consumed)
{
    if (!ctx) { vppx_set_error("context is NULL"); return VPPX_E_NO_DEVICE; }
    if (seed) *seed = ctx->rnd_seed;
    if (consumed) *consumed = ctx->rnd_consumed;
    return 0;
}

extern "C" int vppx_rand_advance(vppx_ctx *ctx, uint64_t draws)
{
    if (!ctx) { vppx_set_error("context is NULL"); return VPPX_E_NO_DEVICE; }
    ctx->rnd_consumed += draws;
    return 0;
}

// number of rand() draws a scan consumed = what the device prefix sums computed
static int scan_common(vppx_ctx *ctx, VppxVppParams &p, uint8_t *l, uint8_t *r, const float *g, int width, int height,
                       int channels, const uint8_t *g_occ)
{
    int rc;
    VPPX_ENTER(ctx);
    p.seed = ctx->rnd_seed;
    p.rand_offset = ctx->rnd_consumed;
    int64_t nh = 0;
    if ((rc = vppx_vpp_host(ctx, &p, 1, height, width, channels, l, r, g, g_occ, nullptr, &nh))) return rc;
    // advance the libc-like stream by the draws this scan consumed
    if (p.method == VPPX_METHOD_RND) { // maxDistance draws nothing from rand()
        uint64_t draws = 0;
        if ((rc = vppx_vpp_last_draws(ctx, 1, &draws))) return rc;
        ctx->rnd_consumed += draws;
    }
    return (int)nh;
}

extern "C" int vppx_virtual_projection_scan_rnd(vppx_ctx *ctx, uint8_t *l, uint8_t *r, const float *g, int width,
                                                int height, int channels, int uniform_color, int wsize, int direction,
                                                float c, float c_occ, const uint8_t *g_occ, int discard_occluded,
                                                int interpolate)
{
    VppxVppParams p;
    vppx_vpp_params_default(&p);
    p.method = VPPX_METHOD_RND;
    p.uniform_color = uniform_color; p.wsize = wsize; p.direction = direction; p.c = c; p.c_occ = c_occ;
    p.discard_occluded = discard_occluded; p.interpolate = interpolate;
    return scan_common(ctx, p, l, r, g, width, height, channels, g_occ);
}

extern "C" int vppx_virtual_projection_scan_max_dist(vppx_ctx *ctx, uint8_t *l, uint8_t *r, const float *g, int width,
                                                     int height, int channels, int uniform_color, int wsize,
                                                     int wsize_agg_x, int wsize_agg_y, int direction, float c, float c_occ,
                                                     const uint8_t *g_occ, int discard_occluded, int interpolate)
{
    VppxVppParams p;
    vppx_vpp_params_default(&p);
    p.method = VPPX_METHOD_MAXDIST;
    p.uniform_color = uniform_color; p.wsize = wsize; p.wsize_agg_x = wsize_agg_x; p.wsize_agg_y = wsize_agg_y;
    p.direction = direction; p.c = c; p.c_occ = c_occ;
    p.discard_occluded = discard_occluded; p.interpolate = interpolate;
    return scan_common(ctx, p, l, r, g, width, height, channels, g_occ);
}

extern "C" int vppx_rand_stream(vppx_ctx *ctx, uint32_t seed, uint64_t offset, int64_t n, int32_t *out)
{
    int rc;
    VPPX_ENTER(ctx);
    if (n < 0 || (n > 0 && !out)) { vppx_set_error("vppx_rand_stream: bad arguments"); return VPPX_E_INVALID_ARG; }
    if (n == 0) return 0;
    void *d;
    if ((rc = ws_reserve(ctx, WS_STAGE_A, (size_t)n * sizeof(int32_t), &d))) return rc;
    if ((rc = vpp_launch_rand_stream(ctx, seed, offset, n, (int32_t *)d))) return rc;
    if ((rc = download(ctx, out, d, (size_t)n * sizeof(int32_t)))) return rc;
    VPPX_HIP(hipStreamSynchronize(ctx->stream));
    return 0;
}

// ---------------------------------------------------------------------------------------
// fused hot path (test.py:158-225): VPP -> rSGM, batched, device resident
// ---------------------------------------------------------------------------------------
static int vpp_rsgm_one(vppx_ctx *ctx, const HotCall &c)
{
    int rc;
    const VppxOccParams *const op = c.op;
    const VppxVppParams *const vp = &c.vp;
    const VppxRsgmParams *const rp = c.rp;
    const int B = c.B, H = c.H, W = c.W, C = c.C;
    const u8 *const left = c.left, *const right = c.right, *g_occ = c.g_occ;
    const float *const g = c.g;
    u8 *l_vpp = c.l_vpp, *r_vpp = c.r_vpp, *const conf_out = c.conf_out;
    const size_t nb = (size_t)B * H * W * C, np = (size_t)B * H * W;
    const bool piped = pipeline_applies(ctx);
    // A pipelined front stage writes library-owned buffers only; the caller's copies are made on the launch stream
    // (front_end).  One buffer each is enough: every reader of call k's front-stage results -- its own front stage, the
    // copies, its aggregation -- is ordered before the event that lets the front stage of call k+1 start.
    u8 *l_user = l_vpp, *r_user = r_vpp, *conf_user = conf_out;
    if ((piped || !l_vpp) && (rc = ws_get(ctx, WS_VPP_L, nb, &l_vpp))) return rc;
    if ((piped || !r_vpp) && (rc = ws_get(ctx, WS_VPP_R, nb, &r_vpp))) return rc;
    float *omap = nullptr;
    u8 *conf = conf_out;
    if (op) {
        if ((rc = ws_get(ctx, WS_OCC_OMAP, np, &omap))) return rc;
        if ((piped || !conf_out) && (rc = ws_get(ctx, WS_OCC_OUT, np, &conf))) return rc;
    }
    FrontGuard guard{ctx};
    ctx->n_pipe_copy = 0;
    if (piped) {
        ctx->pipe_call = true;
        if ((rc = front_begin(ctx))) return rc;
        ctx->occ_done_recorded = false;
        if (op && conf_user) ctx->pipe_copy[ctx->n_pipe_copy++] = {conf_user, conf, np, true};
        if (l_user) ctx->pipe_copy[ctx->n_pipe_copy++] = {l_user, l_vpp, nb, false};
        if (r_user) ctx->pipe_copy[ctx->n_pipe_copy++] = {r_user, r_vpp, nb, false};
    }
    {   // what the front-stage kernels may use of a CU's LDS: next to the previous part's sum / WTA kernel when pipelined
        // (the previous part has this part's shape: its real layout when it ran with this D and batch, else the threshold's guess)
        const int nvol_prev = (ctx->last_sum_nvol && ctx->last_sum_D == rp->dmax && ctx->last_sum_B == B) ? ctx->last_sum_nvol
                                                                                                          : (B >= VPPX_FUSED_MIN_FRAMES ? 4 : 8);
        const size_t sum_lds = rsgm_sum_lds_bytes(ctx, rp->dmax, nvol_prev), cu_lds = 160 * 1024;
        const size_t left_over = cu_lds > sum_lds + 512 ? cu_lds - sum_lds - 512 : 2048;
        // Less than 6 KB left (D = 200 .. 248): nothing of the front stage fits.  D = 256 on the trapezoid ring with spare slots
        // leaves 8736 bytes, but its 4 x 125 VGPRs per SIMD leave no registers: nothing of the front stage can run NEXT to that
        // kernel either.  In both cases its kernels keep their efficient shapes and run in the sum kernel's tail.
        const bool sum_fills_cu = rp->dmax == 256 && nvol_prev == 4 && ctx->knobs.sum_trap == 2 && !ctx->knobs.sum_general;
        ctx->front_lds_budget = (piped && !sum_fills_cu && left_over < 64 * 1024 && left_over >= 6 * 1024) ? left_over : 64 * 1024;
    }
    stage_begin(ctx);
    if (op) { // test.py:154: g_occ = occlusion_heuristic(hints)[1]
        if ((rc = occ_launch(ctx, B, H, W, g, op->rx, op->ry, op->l, op->g, op->th_conf, op->th_filter, omap, conf))) return rc;
        stage_mark(ctx, ST_OCC);
        g_occ = conf;
        if (piped && conf_user) { // (front_end: the mask's copy to the caller waits for this, not for the whole front stage)
            if (!ctx->ev_occ_done) VPPX_HIP(hipEventCreateWithFlags(&ctx->ev_occ_done, hipEventDisableTiming));
            VPPX_HIP(hipEventRecord(ctx->ev_occ_done, ctx->stream));
            ctx->occ_done_recorded = true;
        }
    }
    // vpp() works on copies (np.copy, vpp_standalone.py:397)
    VPPX_HIP(hipMemcpyAsync(l_vpp, left, nb, hipMemcpyDeviceToDevice, ctx->stream));
    VPPX_HIP(hipMemcpyAsync(r_vpp, right, nb, hipMemcpyDeviceToDevice, ctx->stream));
    VppGeom vg = {B, H, W, C};
    const float *filled_g = nullptr;
    if (vp->use_bilateral_patch) {
        float *fg;
        if ((rc = ws_get(ctx, WS_FILLED_G, (size_t)B * H * W, &fg))) return rc;
        if ((rc = vpp_launch_bilateral_fill(ctx, *vp, vg, left, g, fg))) return rc;
        filled_g = fg;
    }
    if ((rc = vpp_launch(ctx, *vp, vg, l_vpp, r_vpp, g, g_occ, filled_g, nullptr, nullptr, right))) return rc;
    if (ctx->draws_dst && vp->method == VPPX_METHOD_RND) // a frame stream keeps every frame's draw count (library-owned destination)
        VPPX_HIP(hipMemcpy2DAsync(ctx->draws_dst, 8, ctx->ws[WS_FRAME_TOT].p, 16, 8, (size_t)B, hipMemcpyDeviceToDevice, ctx->stream));
    RsgmGeom rg;
    make_geom(B, H, W, C, rp->dmax, rg);
    // --guided: the VPP hints re-weight the costs too (test.py:207 passes data['hints'] to both)
    return rsgm_core(ctx, *rp, rg, left, l_vpp, r_vpp, c.disp_out, c.validhints ? g : nullptr, c.validhints);
}

static int vpp_rsgm_entry(vppx_ctx *ctx, const HotCall &c);
static int scaled_call(vppx_ctx *ctx, const HotCall &c);
static int eval_call(vppx_ctx *ctx, const HotCall &c);
static int sampled_call(vppx_ctx *ctx, const HotCall &c);

// The common part of every entry point's descriptor
static HotCall hot_call(HotCall::Layer layer, const VppxOccParams *op, const VppxVppParams *vp, const VppxRsgmParams *rp, int B, int H, int W,
                        int C, const uint8_t *left, const uint8_t *right)
{
    HotCall c;
    c.layer = layer;
    c.op = op;
    if (vp) c.vp = *vp;
    c.vp_null = !vp;
    c.rp = rp;
    c.B = B; c.H = H; c.W = W; c.C = C;
    c.left = left; c.right = right;
    return c;
}

// The call, entered at its layer; the caller's inputs-ready event is one-shot, whatever happened
int vppx_hot_call_internal(vppx_ctx *ctx, const HotCall &c)
{
    const int rc = c.layer == HotCall::SAMPLED ? sampled_call(ctx, c)
                 : c.layer == HotCall::EVAL    ? eval_call(ctx, c)
                 : c.layer == HotCall::SCALED  ? scaled_call(ctx, c)
                                               : vpp_rsgm_entry(ctx, c);
    ctx->inputs_ev = nullptr;
    return rc;
}

extern "C" int vppx_inputs_ready_event(vppx_ctx *ctx, void *hip_event)
{
    VPPX_ENTER(ctx);
    VPPX_PIPE_KEEP(ctx);
    ctx->inputs_ev = hip_event;
    return 0;
}

extern "C" int vppx_vpp_rsgm_dev(vppx_ctx *ctx, const VppxVppParams *vp, const VppxRsgmParams *rp, int B, int H, int W,
                                 int C, const uint8_t *left, const uint8_t *right, const float *g, const uint8_t *g_occ,
                                 uint8_t *l_vpp, uint8_t *r_vpp, float *disp_out)
{
    VPPX_ENTER(ctx);
    VPPX_PIPE_KEEP(ctx);
    HotCall c = hot_call(HotCall::PLAIN, nullptr, vp, rp, B, H, W, C, left, right);
    c.g = g; c.g_occ = g_occ;
    c.l_vpp = l_vpp; c.r_vpp = r_vpp; c.disp_out = disp_out;
    return vppx_hot_call_internal(ctx, c);
}

extern "C" int vppx_occ_vpp_rsgm_dev(vppx_ctx *ctx, const VppxOccParams *op, const VppxVppParams *vp, const VppxRsgmParams *rp,
                                     int B, int H, int W, int C, const uint8_t *left, const uint8_t *right, const float *g,
                                     uint8_t *conf_out, uint8_t *l_vpp, uint8_t *r_vpp, float *disp_out)
{
    VPPX_ENTER(ctx);
    VPPX_PIPE_KEEP(ctx);
    if (!op) { vppx_set_error("vppx_occ_vpp_rsgm: NULL argument"); return VPPX_E_INVALID_ARG; }
    HotCall c = hot_call(HotCall::PLAIN, op, vp, rp, B, H, W, C, left, right);
    c.g = g;
    c.conf_out = conf_out; c.l_vpp = l_vpp; c.r_vpp = r_vpp; c.disp_out = disp_out;
    return vppx_hot_call_internal(ctx, c);
}

// test.py:207-223 (--guided --stereomodel rsgm): the VPP hints g re-weight the matching costs as well (_guided_dsi).
// op != NULL computes the mask on the way, else g_occ (may be NULL) is the caller's.
extern "C" int vppx_occ_vpp_rsgm_guided_dev(vppx_ctx *ctx, const VppxOccParams *op, const VppxVppParams *vp, const VppxRsgmParams *rp,
                                            int B, int H, int W, int C, const uint8_t *left, const uint8_t *right, const float *g,
                                            const uint8_t *g_occ, const float *validhints, uint8_t *conf_out, uint8_t *l_vpp,
                                            uint8_t *r_vpp, float *disp_out)
{
    VPPX_ENTER(ctx);
    VPPX_PIPE_KEEP(ctx);
    if (!validhints) { vppx_set_error("vppx_occ_vpp_rsgm_guided: validhints is NULL"); ctx->inputs_ev = nullptr; return VPPX_E_INVALID_ARG; }
    HotCall c = hot_call(HotCall::PLAIN, op, vp, rp, B, H, W, C, left, right);
    c.g = g; c.g_occ = op ? nullptr : g_occ; c.validhints = validhints;
    c.conf_out = conf_out; c.l_vpp = l_vpp; c.r_vpp = r_vpp; c.disp_out = disp_out;
    return vppx_hot_call_internal(ctx, c);
}

// The tail of a host call: `call` queues the hot path on the staged inputs; its results come down (entries without a device
// buffer are skipped), with them the rand() draws each frame consumed (draws_out, may be NULL), and the stream is waited for.
// Like vppx_rsgm_host: a lost lock step of THIS call is repeated once, on the line-parallel kernel, an earlier call's is reported.
struct HostCopy { void *host; const void *dev; size_t bytes; };
template <typename Call>
static int host_call_tail(vppx_ctx *ctx, const VppxVppParams *vp, int B, Call call, std::initializer_list<HostCopy> copies, uint64_t *draws_out)
{
    int rc;
    for (int attempt = 0;; attempt++) {
        const unsigned serial_before = ctx->v3.serial;
        rc = call();
        ctx->inputs_ev = nullptr;
        if (rc) return rc;
        for (const HostCopy &k : copies)
            if (k.dev && (rc = download(ctx, k.host, k.dev, k.bytes))) return rc;
        std::vector<unsigned long long> tot;
        // the totals of THIS context's single part only: parts overwrite each other's, sub-stream children keep their own
        if (draws_out && vp->method == VPPX_METHOD_RND && ctx->ws[WS_FRAME_TOT].p && ctx->last_parts == 1 &&
            ctx->ws[WS_FRAME_TOT].cap >= (size_t)B * 16) {
            tot.resize((size_t)B * 2);
            VPPX_HIP(hipMemcpyAsync(tot.data(), ctx->ws[WS_FRAME_TOT].p, tot.size() * 8, hipMemcpyDeviceToHost, ctx->stream));
        }
        VPPX_HIP(hipStreamSynchronize(ctx->stream));
        if (draws_out)
            for (int f = 0; f < B; f++) draws_out[f] = tot.empty() ? 0 : tot[2 * f];
        if ((rc = lockstep_check(ctx)) == 0) break;
        const unsigned s = ctx->lockstep_last_serial;
        const bool mine = (unsigned)(s - serial_before - 1u) < (unsigned)(ctx->v3.serial - serial_before);
        if (!mine || attempt > 0) return rc;
    }
    return 0;
}

// test.py:154-225 for host arrays in ONE call: the pair, the hints (and a caller's mask) go up once, the disparities (and, on
// request, the mask and the patterned pair) come down once; nothing is uploaded three times as with filter.occlusion_heuristic
// + vpp_standalone.vpp + rsgm.compute_rsgm called one after the other.  op != NULL computes the mask on the way (--maskocc),
// else g_occ (may be NULL) is the caller's.  draws_out (may be NULL, [B]): rand() draws each frame consumed, so that a
// single-frame caller can advance the libc-like stream exactly like vpp() does.
static int occ_vpp_rsgm_host(vppx_ctx *ctx, const VppxOccParams *op, const VppxVppParams *vp, const VppxRsgmParams *rp, int B, int H,
                             int W, int C, const uint8_t *left, const uint8_t *right, const float *g, const uint8_t *g_occ,
                             const float *validhints, uint8_t *conf_out, uint8_t *l_vpp_out, uint8_t *r_vpp_out, float *disp_out,
                             uint64_t *draws_out)
{
    int rc;
    if (!vp || !rp || !left || !right || !g || !disp_out) { vppx_set_error("vppx_occ_vpp_rsgm_host: NULL argument"); return VPPX_E_INVALID_ARG; }
    if ((rc = check_frames(B, H, W, C))) return rc;
    const size_t nb = (size_t)B * H * W * C, np = (size_t)B * H * W;
    void *dl, *dr, *dg, *docc = nullptr, *dconf = nullptr, *dlv = nullptr, *drv = nullptr, *dout, *dvh = nullptr;
    // the hints go up first and the occlusion heuristic is queued at once: its kernels run while the host is busy with the
    // (pageable, i.e. host-blocking) uploads of the pair
    if ((rc = upload(ctx, WS_STAGE_C, g, np * sizeof(float), &dg))) return rc;
    if (op) {
        float *omap;
        if ((rc = ws_get(ctx, WS_OCC_OMAP, np, &omap))) return rc;
        if ((rc = ws_reserve(ctx, WS_STAGE_D, np, &dconf))) return rc;
        ctx->front_lds_budget = 64 * 1024;
        front_routes_reset(ctx);
        if ((rc = occ_launch(ctx, B, H, W, (const float *)dg, op->rx, op->ry, op->l, op->g, op->th_conf, op->th_filter, omap, (u8 *)dconf))) return rc;
        docc = dconf; // from here on a given mask
        if (!conf_out) dconf = nullptr;
    } else if (g_occ && (rc = upload(ctx, WS_STAGE_D, g_occ, np, &docc))) return rc;
    if (validhints && (rc = upload(ctx, WS_HANDOFF_V, validhints, np * sizeof(float), &dvh))) return rc;
    if ((rc = upload(ctx, WS_STAGE_A, left, nb, &dl))) return rc;
    if ((rc = upload(ctx, WS_STAGE_B, right, nb, &dr))) return rc;
    if (l_vpp_out && (rc = ws_reserve(ctx, WS_STAGE_E, nb, &dlv))) return rc;
    if (r_vpp_out && (rc = ws_reserve(ctx, WS_STAGE_F, nb, &drv))) return rc;
    if ((rc = ws_reserve(ctx, WS_HANDOFF_H, np * sizeof(float), &dout))) return rc;
    HotCall c = hot_call(HotCall::PLAIN, nullptr, vp, rp, B, H, W, C, (const u8 *)dl, (const u8 *)dr);
    c.g = (const float *)dg; c.g_occ = (const u8 *)docc; c.validhints = (const float *)dvh;
    c.l_vpp = (u8 *)dlv; c.r_vpp = (u8 *)drv; c.disp_out = (float *)dout;
    auto call = [&]() {
        ctx->front_routes_keep = op != nullptr; // (vppx_last_front_routes: the heuristic above belongs to this call)
        return vpp_rsgm_entry(ctx, c);
    };
    return host_call_tail(ctx, vp, B, call,
                          {{disp_out, dout, np * sizeof(float)}, {conf_out, dconf, np}, {l_vpp_out, dlv, nb}, {r_vpp_out, drv, nb}}, draws_out);
}

extern "C" int vppx_occ_vpp_rsgm_host(vppx_ctx *ctx, const VppxOccParams *op, const VppxVppParams *vp, const VppxRsgmParams *rp, int B, int H,
                                      int W, int C, const uint8_t *left, const uint8_t *right, const float *g, const uint8_t *g_occ,
                                      uint8_t *conf_out, uint8_t *l_vpp_out, uint8_t *r_vpp_out, float *disp_out, uint64_t *draws_out)
{
    VPPX_ENTER(ctx);
    return occ_vpp_rsgm_host(ctx, op, vp, rp, B, H, W, C, left, right, g, g_occ, nullptr, conf_out, l_vpp_out, r_vpp_out, disp_out, draws_out);
}

extern "C" int vppx_occ_vpp_rsgm_guided_host(vppx_ctx *ctx, const VppxOccParams *op, const VppxVppParams *vp, const VppxRsgmParams *rp,
                                             int B, int H, int W, int C, const uint8_t *left, const uint8_t *right, const float *g,
                                             const uint8_t *g_occ, const float *validhints, uint8_t *conf_out, uint8_t *l_vpp_out,
                                             uint8_t *r_vpp_out, float *disp_out, uint64_t *draws_out)
{
    VPPX_ENTER(ctx);
    if (!validhints) { vppx_set_error("vppx_occ_vpp_rsgm_guided_host: validhints is NULL"); return VPPX_E_INVALID_ARG; }
    return occ_vpp_rsgm_host(ctx, op, vp, rp, B, H, W, C, left, right, g, op ? nullptr : g_occ, validhints, conf_out, l_vpp_out, r_vpp_out,
                             disp_out, draws_out);
}

// ---------------------------------------------------------------------------------------
// --iscale / --oscale (test.py:136-148, :247-248): resize on the way in, restore on the way out
// ---------------------------------------------------------------------------------------
extern "C" void vppx_scale_params_default(VppxScaleParams *p)
{
    if (!p) return;
    p->iscale = 1;
    p->oscale = 1;
}

// test.py:247: `if args.iscale != 1 and args.iscale/args.oscale != 1`
static bool scale_restores(const VppxScaleParams &sp) { return sp.iscale != 1 && sp.iscale != sp.oscale; }

extern "C" int vppx_scaled_shape(int H, int W, const VppxScaleParams *sp, int *h, int *w, int *Ho, int *Wo)
{
    if (!sp) { vppx_set_error("vppx_scaled_shape: sp is NULL"); return VPPX_E_INVALID_ARG; }
    if (sp->iscale < 1 || sp->oscale < 1) {
        vppx_set_error("iscale and oscale must be positive integers (got iscale %d, oscale %d)", sp->iscale, sp->oscale);
        return VPPX_E_INVALID_ARG;
    }
    if (H < 1 || W < 1) { vppx_set_error("vppx_scaled_shape: bad shape %dx%d", H, W); return VPPX_E_INVALID_ARG; }
    const int hs = H / sp->iscale, ws = W / sp->iscale; // cv2.resize(img, (w // iscale, h // iscale))
    if (hs < 1 || ws < 1) {
        vppx_set_error("iscale %d leaves nothing of %dx%d frames", sp->iscale, H, W);
        return VPPX_E_INVALID_ARG;
    }
    int ho = hs, wo = ws;
    if (scale_restores(*sp)) { // F.interpolate(scale_factor=iscale/oscale): floor(size * factor) in double
        const double f = (double)sp->iscale / (double)sp->oscale;
        ho = (int)floor((double)hs * f);
        wo = (int)floor((double)ws * f);
        if (ho < 1 || wo < 1) {
            vppx_set_error("iscale %d / oscale %d restores %dx%d to an empty map", sp->iscale, sp->oscale, hs, ws);
            return VPPX_E_INVALID_ARG;
        }
    }
    if (h) *h = hs;
    if (w) *w = ws;
    if (Ho) *Ho = ho;
    if (Wo) *Wo = wo;
    return 0;
}

// DESIGN section 5, rule 1: the tables OpenCV's resize (INTER_LINEAR, 8U) builds for one axis, n_in -> n_out; per output
// {first source index, second (clamped), weight of the first, weight of the second} (weights: cvRound(x * 2048), half-even)
static void resize_axis_table(int n_in, int n_out, int *tab)
{
    const double inv = (double)n_out / n_in, scale = 1.0 / inv;
    for (int d = 0; d < n_out; d++) {
        float f = (float)((d + 0.5) * scale - 0.5);
        int s0 = (int)floorf(f);
        f -= (float)s0;
        if (s0 < 0) { s0 = 0; f = 0.f; }
        if (s0 >= n_in - 1) { s0 = n_in - 1; f = 0.f; }
        tab[4 * d] = s0;
        tab[4 * d + 1] = s0 + 1 < n_in ? s0 + 1 : n_in - 1;
        tab[4 * d + 2] = (int)(short)lrintf((1.f - f) * 2048.f);
        tab[4 * d + 3] = (int)(short)lrintf(f * 2048.f);
    }
}

// torch's nearest_idx (ATen UpSample.h) for scale_factor = factor, n_in -> n_out
static void restore_axis_table(int n_in, int n_out, double factor, int *idx)
{
    const float sc = (float)(1.0 / factor);
    for (int i = 0; i < n_out; i++) {
        long long v;
        if (n_out == n_in) v = i;
        else if (n_out == 2 * n_in) v = i >> 1;
        else v = (long long)floorf((float)i * sc);
        idx[i] = (int)(v < n_in - 1 ? v : n_in - 1);
    }
}

// Tables of one shape in WS_SCALE_TAB: ytab [h] int4, xtab [w] int4, ry [Ho], rx [Wo].  Kept per context and rebuilt when the
// shape changes -- after both streams are idle, since a call in flight may still read the old ones.
static int scale_tables(vppx_ctx *ctx, int H, int W, const VppxScaleParams &sp, int h, int w, int Ho, int Wo, const int **tab)
{
    const int key[6] = {H, W, sp.iscale, sp.oscale, Ho, Wo};
    if (ctx->scale_tab_at && ctx->scale_tab_at == ctx->ws[WS_SCALE_TAB].p && memcmp(key, ctx->scale_key, sizeof(key)) == 0) {
        *tab = (const int *)ctx->scale_tab_at;
        return 0;
    }
    std::vector<int> host((size_t)4 * h + (size_t)4 * w + Ho + Wo);
    resize_axis_table(H, h, host.data());
    resize_axis_table(W, w, host.data() + 4 * h);
    const double f = (double)sp.iscale / (double)sp.oscale;
    restore_axis_table(h, Ho, f, host.data() + 4 * h + 4 * w);
    restore_axis_table(w, Wo, f, host.data() + 4 * h + 4 * w + Ho);
    VPPX_HIP(hipStreamSynchronize(ctx->stream));
    if (ctx->stream_front) VPPX_HIP(hipStreamSynchronize(ctx->stream_front));
    void *d = nullptr;
    int rc;
    if ((rc = ws_reserve(ctx, WS_SCALE_TAB, host.size() * sizeof(int), &d))) return rc;
    VPPX_HIP(hipMemcpy(d, host.data(), host.size() * sizeof(int), hipMemcpyHostToDevice));
    memcpy(ctx->scale_key, key, sizeof(key));
    ctx->scale_tab_at = d;
    ctx->scale_tab_builds++;
    *tab = (const int *)d;
    return 0;
}

// guided_metrics of a finished map on the launch stream (the evaluation request of c: vppx_occ_vpp_rsgm_eval_dev).  The partial
// records have their own workspace slot: a pipelined next call's front stage runs next to this and shares nothing with it.
static int eval_launch(vppx_ctx *ctx, const HotCall &c, int Ho, int Wo, const float *disp)
{
    void *part = nullptr;
    int rc = ws_reserve(ctx, WS_METRICS_PART, (size_t)c.B * metrics_blocks_per_frame((size_t)Ho * Wo) * METRICS_PARTIAL_BYTES, &part);
    if (rc) return rc;
    return metrics_launch(ctx, c.B, Ho, Wo, disp, c.Hg, c.Wg, c.gt_scale, c.gt, c.validgt, c.valid_is_u8, part, c.metrics_out, c.errormap);
}

// One kernel in front of the front stage (the resize of a scaled call, the sampling of a sampled one).  With vppx_set_pipeline
// it is the first kernel of the front stage: it waits for what every front stage waits for (the previous
// call's aggregation event and this call's inputs) and writes the set of buffers the previous call did NOT use -- the caller
// picks it by *parity, flipped here; the front stage proper then starts on the kernel's event.  Otherwise the kernel goes on the
// launch stream, behind the caller's inputs event.  The context is back on the launch stream before any return.
template <typename Launch>
static int pre_front(vppx_ctx *ctx, hipEvent_t *ev, int *parity, Launch launch)
{
    int rc;
    if (!pipeline_applies(ctx)) {
        if (ctx->inputs_ev) {
            VPPX_HIP(hipStreamWaitEvent(ctx->stream, (hipEvent_t)ctx->inputs_ev, 0));
            ctx->inputs_ev = nullptr;
        }
        return launch();
    }
    if (!*ev) VPPX_HIP(hipEventCreateWithFlags(ev, hipEventDisableTiming));
    if ((rc = front_begin(ctx))) return rc;
    rc = launch();
    const hipError_t e = rc ? hipSuccess : hipEventRecord(*ev, ctx->stream);
    ctx->stream = ctx->main_saved;
    ctx->front_active = false;
    if (rc) return rc;
    if (e != hipSuccess) { vppx_set_error("hipEventRecord failed: %s", hipGetErrorString(e)); return VPPX_E_HIP; }
    *parity ^= 1;
    ctx->inputs_ev = (void *)*ev;
    return 0;
}

// The scaled call on device pointers: resize + decimation (scale_front_kernel), the unchanged hot path at (h, w) on the
// library-owned scaled buffers, then the restore (scale_restore_kernel) on the launch stream.
static int scaled_call(vppx_ctx *ctx, const HotCall &c)
{
    int rc;
    const VppxScaleParams *const sp = c.sp;
    const int B = c.B, H = c.H, W = c.W, C = c.C;
    if (c.vp_null || !c.rp || !sp || !c.left || !c.right || !c.g || !c.disp_out) { vppx_set_error("vppx_occ_vpp_rsgm_scaled: NULL argument"); return VPPX_E_INVALID_ARG; }
    int h, w, Ho, Wo;
    if ((rc = vppx_scaled_shape(H, W, sp, &h, &w, &Ho, &Wo))) return rc;
    if ((rc = check_frames(B, H, W, C))) return rc;
    if ((rc = check_frames(B, h, w, C))) {
        char msg[512];
        snprintf(msg, sizeof(msg), "%s", vppx_last_error());
        vppx_set_error("vppx_occ_vpp_rsgm_scaled: iscale %d turns %dx%d frames into %dx%d: %s", sp->iscale, H, W, h, w, msg);
        return rc;
    }
    if ((rc = check_vpp_params(c.vp))) return rc;
    if ((rc = check_rsgm_params(*c.rp))) return rc;
    HotCall run = c; // the call at the shape it runs at
    run.sp = nullptr;
    run.g_occ = c.op ? nullptr : c.g_occ;
    run.conf_out = c.op ? c.conf_out : nullptr;
    run.disp_small = nullptr;
    if (sp->iscale == 1) { // nothing to resize, nothing to restore: the unscaled call
        rc = vpp_rsgm_entry(ctx, run);
        if (rc == 0 && c.disp_small)
            VPPX_HIP(hipMemcpyAsync(c.disp_small, c.disp_out, (size_t)B * H * W * sizeof(float), hipMemcpyDeviceToDevice, ctx->stream));
        return rc;
    }
    if ((rc = lockstep_check(ctx))) return rc; // (before anything is queued, as the hot path itself does)
    const int *tab = nullptr;
    if ((rc = scale_tables(ctx, H, W, *sp, h, w, Ho, Wo, &tab))) return rc;
    const int set = pipeline_applies(ctx) ? ctx->scale_parity : 0;
    ctx->last_scale_set = set;
    const size_t np = (size_t)B * h * w, nb = np * C;
    u8 *ls, *rs;
    float *gs, *vhs = nullptr;
    if ((rc = ws_get(ctx, set ? WS_SCALE_L1 : WS_SCALE_L0, nb, &ls))) return rc;
    if ((rc = ws_get(ctx, set ? WS_SCALE_R1 : WS_SCALE_R0, nb, &rs))) return rc;
    if ((rc = ws_get(ctx, set ? WS_SCALE_G1 : WS_SCALE_G0, np, &gs))) return rc;
    if (c.validhints && (rc = ws_get(ctx, set ? WS_SCALE_V1 : WS_SCALE_V0, np, &vhs))) return rc;
    const bool restore = scale_restores(*sp);
    float *dsmall = restore ? c.disp_small : c.disp_out;
    if (restore && !dsmall && (rc = ws_get(ctx, WS_SCALE_DSMALL, np, &dsmall))) return rc;
    ScaleFrontArgs a;
    a.l = c.left; a.r = c.right; a.g = c.g; a.vh = c.validhints;
    a.ls = ls; a.rs = rs; a.gs = gs; a.vhs = vhs;
    a.ytab = (const int4 *)tab;
    a.xtab = (const int4 *)(tab + 4 * h);
    a.B = B; a.H = H; a.W = W; a.C = C; a.h = h; a.w = w; a.s = sp->iscale;
    a.fs = (float)sp->iscale;
    a.n_img_threads = 0;
    if ((rc = pre_front(ctx, &ctx->ev_scaled, &ctx->scale_parity, [&]() { return scale_launch_front(ctx, a); }))) return rc;
    run.H = h; run.W = w;
    run.left = ls; run.right = rs; run.g = gs; run.validhints = vhs;
    run.disp_out = dsmall;
    // the metrics read the restored map: with a restore they are queued below, behind it, and the hot path has no request
    if (restore) run.metrics_out = nullptr;
    if ((rc = vpp_rsgm_entry(ctx, run))) return rc;
    {   // vppx_last_routes: the resize first, the restore last
        char buf[32];
        snprintf(buf, sizeof(buf), "scale_front<%d>", C);
        ctx->routes.insert(ctx->routes.begin(), std::string(buf));
    }
    if (restore) {
        const int *ry = tab + 4 * h + 4 * w, *rx = ry + Ho;
        if ((rc = scale_launch_restore(ctx, B, h, w, Ho, Wo, dsmall, c.disp_out, ry, rx, sp->iscale, sp->oscale))) return rc;
        route_note(ctx, "scale_restore");
        if (c.metrics_out && (rc = eval_launch(ctx, c, Ho, Wo, c.disp_out))) return rc;
    } else if (c.disp_small) {
        VPPX_HIP(hipMemcpyAsync(c.disp_small, c.disp_out, np * sizeof(float), hipMemcpyDeviceToDevice, ctx->stream));
    }
    return 0;
}

extern "C" int vppx_occ_vpp_rsgm_scaled_dev(vppx_ctx *ctx, const VppxOccParams *op, const VppxVppParams *vp, const VppxRsgmParams *rp,
                                            const VppxScaleParams *sp, int B, int H, int W, int C, const uint8_t *left, const uint8_t *right,
                                            const float *g, const uint8_t *g_occ, const float *validhints, uint8_t *conf_out, uint8_t *l_vpp,
                                            uint8_t *r_vpp, float *disp_out, float *disp_small)
{
    VPPX_ENTER(ctx);
    VPPX_PIPE_KEEP(ctx);
    HotCall c = hot_call(HotCall::SCALED, op, vp, rp, B, H, W, C, left, right);
    c.sp = sp;
    c.g = g; c.g_occ = g_occ; c.validhints = validhints;
    c.conf_out = conf_out; c.l_vpp = l_vpp; c.r_vpp = r_vpp; c.disp_out = disp_out; c.disp_small = disp_small;
    return vppx_hot_call_internal(ctx, c);
}

extern "C" int vppx_occ_vpp_rsgm_scaled_host(vppx_ctx *ctx, const VppxOccParams *op, const VppxVppParams *vp, const VppxRsgmParams *rp,
                                             const VppxScaleParams *sp, int B, int H, int W, int C, const uint8_t *left, const uint8_t *right,
                                             const float *g, const uint8_t *g_occ, const float *validhints, uint8_t *conf_out,
                                             uint8_t *l_vpp_out, uint8_t *r_vpp_out, float *disp_out, float *disp_small, uint64_t *draws_out)
{
    VPPX_ENTER(ctx);
    int rc;
    if (!vp || !rp || !sp || !left || !right || !g || !disp_out) { vppx_set_error("vppx_occ_vpp_rsgm_scaled_host: NULL argument"); return VPPX_E_INVALID_ARG; }
    int h, w, Ho, Wo;
    if ((rc = vppx_scaled_shape(H, W, sp, &h, &w, &Ho, &Wo))) return rc;
    if ((rc = check_frames(B, H, W, C))) return rc;
    if ((rc = check_frames(B, h, w, C))) {
        char msg[512];
        snprintf(msg, sizeof(msg), "%s", vppx_last_error());
        vppx_set_error("vppx_occ_vpp_rsgm_scaled_host: iscale %d turns %dx%d frames into %dx%d: %s", sp->iscale, H, W, h, w, msg);
        return rc;
    }
    const size_t nb = (size_t)B * H * W * C, np = (size_t)B * H * W;
    const size_t nbs = (size_t)B * h * w * C, nps = (size_t)B * h * w, npo = (size_t)B * Ho * Wo;
    void *dl, *dr, *dg, *docc = nullptr, *dconf = nullptr, *dlv = nullptr, *drv = nullptr, *dout, *dvh = nullptr, *dsm = nullptr;
    if ((rc = upload(ctx, WS_STAGE_C, g, np * sizeof(float), &dg))) return rc;
    if (validhints && (rc = upload(ctx, WS_HANDOFF_V, validhints, np * sizeof(float), &dvh))) return rc;
    if (!op && g_occ && (rc = upload(ctx, WS_STAGE_D, g_occ, nps, &docc))) return rc;
    if (op && conf_out && (rc = ws_reserve(ctx, WS_STAGE_D, nps, &dconf))) return rc;
    if ((rc = upload(ctx, WS_STAGE_A, left, nb, &dl))) return rc;
    if ((rc = upload(ctx, WS_STAGE_B, right, nb, &dr))) return rc;
    if (l_vpp_out && (rc = ws_reserve(ctx, WS_STAGE_E, nbs, &dlv))) return rc;
    if (r_vpp_out && (rc = ws_reserve(ctx, WS_STAGE_F, nbs, &drv))) return rc;
    if ((rc = ws_reserve(ctx, WS_HANDOFF_H, npo * sizeof(float), &dout))) return rc;
    if (disp_small && (rc = ws_reserve(ctx, WS_SCALE_HOST_D, nps * sizeof(float), &dsm))) return rc;
    HotCall c = hot_call(HotCall::SCALED, op, vp, rp, B, H, W, C, (const u8 *)dl, (const u8 *)dr);
    c.sp = sp;
    c.g = (const float *)dg; c.g_occ = (const u8 *)docc; c.validhints = (const float *)dvh;
    c.conf_out = (u8 *)dconf; c.l_vpp = (u8 *)dlv; c.r_vpp = (u8 *)drv; c.disp_out = (float *)dout; c.disp_small = (float *)dsm;
    return host_call_tail(ctx, vp, B, [&]() { return scaled_call(ctx, c); },
                          {{disp_out, dout, npo * sizeof(float)}, {disp_small, dsm, nps * sizeof(float)}, {conf_out, dconf, nps},
                           {l_vpp_out, dlv, nbs}, {r_vpp_out, drv, nbs}},
                          draws_out);
}

// ---------------------------------------------------------------------------------------
// evaluation metrics (losses.py:13-24; test.py:150-152, :251-252)
// ---------------------------------------------------------------------------------------
extern "C" void vppx_eval_params_default(VppxEvalParams *p)
{
    if (!p) return;
    p->gt_scale = 1;
    p->reserved0 = 0;
}

static int check_metrics_args(const char *name, const VppxEvalParams *ep, int B, int Ho, int Wo, int Hg, int Wg, int *gt_scale)
{
    const int s = ep ? ep->gt_scale : 1;
    if (s < 1) { vppx_set_error("%s: gt_scale %d (>= 1)", name, s); return VPPX_E_INVALID_ARG; }
    if (B < 1 || B > 65535 || Ho < 1 || Wo < 1 || Hg < 1 || Wg < 1 || (size_t)Hg * Wg > ((size_t)1 << 31)) {
        vppx_set_error("%s: bad shape (B %d, map %d x %d, gt %d x %d)", name, B, Ho, Wo, Hg, Wg);
        return VPPX_E_INVALID_ARG;
    }
    if (Hg / s != Ho || Wg / s != Wo) {
        vppx_set_error("%s: gt of %d x %d at gt_scale %d is %d x %d, the disparity map is %d x %d", name, Hg, Wg, s, Hg / s, Wg / s, Ho, Wo);
        return VPPX_E_INVALID_ARG;
    }
    *gt_scale = s;
    return 0;
}

static int guided_metrics_dev(vppx_ctx *ctx, const char *name, const VppxEvalParams *ep, int B, int Ho, int Wo, const float *disp, int Hg,
                              int Wg, const float *gt, const void *valid, int valid_is_u8, VppxMetrics *metrics_out, float *errormap)
{
    int rc, s = 1;
    if (!disp || !gt || !valid || !metrics_out) { vppx_set_error("%s: NULL argument", name); return VPPX_E_INVALID_ARG; }
    if ((rc = check_metrics_args(name, ep, B, Ho, Wo, Hg, Wg, &s))) return rc;
    void *part = nullptr;
    if ((rc = ws_reserve(ctx, WS_METRICS_PART, (size_t)B * metrics_blocks_per_frame((size_t)Ho * Wo) * METRICS_PARTIAL_BYTES, &part))) return rc;
    return metrics_launch(ctx, B, Ho, Wo, disp, Hg, Wg, s, gt, valid, valid_is_u8, part, metrics_out, errormap);
}

extern "C" int vppx_guided_metrics_dev(vppx_ctx *ctx, const VppxEvalParams *ep, int B, int Ho, int Wo, const float *disp, int Hg, int Wg,
                                       const float *gt, const float *validgt, VppxMetrics *metrics_out, float *errormap)
{
    VPPX_ENTER(ctx);
    VPPX_PIPE_KEEP(ctx); // (its only scratch is a slot no front stage touches)
    return guided_metrics_dev(ctx, "vppx_guided_metrics_dev", ep, B, Ho, Wo, disp, Hg, Wg, gt, validgt, 0, metrics_out, errormap);
}

extern "C" int vppx_guided_metrics_host(vppx_ctx *ctx, const VppxEvalParams *ep, int B, int Ho, int Wo, const float *disp, int Hg, int Wg,
                                        const float *gt, const float *validgt, VppxMetrics *metrics_out, float *errormap)
{
    VPPX_ENTER(ctx);
    int rc, s = 1;
    if (!disp || !gt || !validgt || !metrics_out) { vppx_set_error("vppx_guided_metrics_host: NULL argument"); return VPPX_E_INVALID_ARG; }
    if ((rc = check_metrics_args("vppx_guided_metrics_host", ep, B, Ho, Wo, Hg, Wg, &s))) return rc;
    const size_t npo = (size_t)B * Ho * Wo, npg = (size_t)B * Hg * Wg;
    void *dd, *dg, *dv, *dm, *de = nullptr;
    if ((rc = upload(ctx, WS_STAGE_A, disp, npo * sizeof(float), &dd))) return rc;
    if ((rc = upload(ctx, WS_STAGE_B, gt, npg * sizeof(float), &dg))) return rc;
    if ((rc = upload(ctx, WS_STAGE_C, validgt, npg * sizeof(float), &dv))) return rc;
    if ((rc = ws_reserve(ctx, WS_METRICS_OUT, (size_t)B * sizeof(VppxMetrics), &dm))) return rc;
    if (errormap && (rc = ws_reserve(ctx, WS_STAGE_E, npo * sizeof(float), &de))) return rc;
    if ((rc = guided_metrics_dev(ctx, "vppx_guided_metrics_host", ep, B, Ho, Wo, (const float *)dd, Hg, Wg, (const float *)dg, dv, 0,
                                 (VppxMetrics *)dm, (float *)de)))
        return rc;
    if ((rc = download(ctx, metrics_out, dm, (size_t)B * sizeof(VppxMetrics)))) return rc;
    if (de && (rc = download(ctx, errormap, de, npo * sizeof(float)))) return rc;
    VPPX_HIP(hipStreamSynchronize(ctx->stream));
    return 0;
}

// The evaluating call: the scaled call with the evaluation request resolved; the hot path (or scaled_call, behind a restore)
// queues the metrics.  validgt: float32, or one byte per pixel (an evaluating frame stream's ring).
static int eval_call(vppx_ctx *ctx, const HotCall &c)
{
    int rc, s = 1;
    if (!c.gt || !c.validgt || !c.metrics_out || !c.disp_out) { vppx_set_error("vppx_occ_vpp_rsgm_eval: NULL argument"); return VPPX_E_INVALID_ARG; }
    const VppxScaleParams one = {1, 1};
    HotCall e = c;
    if (!e.sp) e.sp = &one;
    int h, w, Ho, Wo;
    if ((rc = vppx_scaled_shape(c.H, c.W, e.sp, &h, &w, &Ho, &Wo))) return rc;
    if ((rc = check_metrics_args("vppx_occ_vpp_rsgm_eval", c.ep, c.B, Ho, Wo, c.H, c.W, &s))) return rc;
    {   // the records' slot is sized before anything is queued (and before a capture could begin)
        void *part = nullptr;
        if ((rc = ws_reserve(ctx, WS_METRICS_PART, (size_t)c.B * metrics_blocks_per_frame((size_t)Ho * Wo) * METRICS_PARTIAL_BYTES, &part))) return rc;
    }
    e.gt_scale = s; e.Hg = c.H; e.Wg = c.W;
    return scaled_call(ctx, e);
}

extern "C" int vppx_occ_vpp_rsgm_eval_dev(vppx_ctx *ctx, const VppxOccParams *op, const VppxVppParams *vp, const VppxRsgmParams *rp,
                                          const VppxScaleParams *sp, const VppxEvalParams *ep, int B, int H, int W, int C, const uint8_t *left,
                                          const uint8_t *right, const float *g, const uint8_t *g_occ, const float *validhints, const float *gt,
                                          const float *validgt, uint8_t *conf_out, uint8_t *l_vpp, uint8_t *r_vpp, float *disp_out,
                                          float *disp_small, VppxMetrics *metrics_out, float *errormap)
{
    VPPX_ENTER(ctx);
    VPPX_PIPE_KEEP(ctx);
    HotCall c = hot_call(HotCall::EVAL, op, vp, rp, B, H, W, C, left, right);
    c.sp = sp; c.ep = ep;
    c.g = g; c.g_occ = g_occ; c.validhints = validhints;
    c.conf_out = conf_out; c.l_vpp = l_vpp; c.r_vpp = r_vpp; c.disp_out = disp_out; c.disp_small = disp_small;
    c.gt = gt; c.validgt = validgt; c.metrics_out = metrics_out; c.errormap = errormap;
    return vppx_hot_call_internal(ctx, c);
}

// ---------------------------------------------------------------------------------------
// hint sampling (losses.py:5-10 sample_hints; test.py:125-129) on torch's CPU random stream
// ---------------------------------------------------------------------------------------
extern "C" void vppx_sample_params_default(VppxSampleParams *p)
{
    if (!p) return;
    memset(p, 0, sizeof(*p));
    p->probability = 0.05;
    p->seed = 1;
}

extern "C" uint32_t vppx_sample_threshold(double probability) { return sample_threshold(probability); }

static int check_sample_args(const char *name, const VppxSampleParams *smp, int B, int H, int W)
{
    if (!smp) { vppx_set_error("%s: NULL argument", name); return VPPX_E_INVALID_ARG; }
    if (B < 1 || H < 1 || W < 1 || (size_t)H * W > ((size_t)1 << 31)) {
        vppx_set_error("%s: bad shape (B %d, %d x %d)", name, B, H, W);
        return VPPX_E_INVALID_ARG;
    }
    return 0;
}

extern "C" int vppx_sample_hints_dev(vppx_ctx *ctx, const VppxSampleParams *smp, int B, int H, int W, const float *src, const float *validsrc,
                                     float *hints_out, float *validhints_out)
{
    VPPX_ENTER(ctx);
    VPPX_PIPE_KEEP(ctx); // (no workspace)
    int rc;
    if (!smp || !src || !validsrc || !hints_out) { vppx_set_error("vppx_sample_hints_dev: NULL argument"); return VPPX_E_INVALID_ARG; }
    if ((rc = check_sample_args("vppx_sample_hints_dev", smp, B, H, W))) return rc;
    return sample_launch(ctx, B, (size_t)H * W, src, validsrc, 0, hints_out, validhints_out, nullptr, smp->seed, sample_threshold(smp->probability));
}

extern "C" int vppx_sample_hints_host(vppx_ctx *ctx, const VppxSampleParams *smp, int B, int H, int W, const float *src, const float *validsrc,
                                      float *hints_out, float *validhints_out)
{
    VPPX_ENTER(ctx);
    int rc;
    if (!smp || !src || !validsrc || !hints_out) { vppx_set_error("vppx_sample_hints_host: NULL argument"); return VPPX_E_INVALID_ARG; }
    if ((rc = check_sample_args("vppx_sample_hints_host", smp, B, H, W))) return rc;
    const size_t bytes = (size_t)B * H * W * sizeof(float);
    void *ds, *dv, *dh, *dvh = nullptr;
    if ((rc = upload(ctx, WS_STAGE_A, src, bytes, &ds))) return rc;
    if ((rc = upload(ctx, WS_STAGE_B, validsrc, bytes, &dv))) return rc;
    if ((rc = ws_reserve(ctx, WS_STAGE_C, bytes, &dh))) return rc;
    if (validhints_out && (rc = ws_reserve(ctx, WS_STAGE_E, bytes, &dvh))) return rc;
    if ((rc = sample_launch(ctx, B, (size_t)H * W, (const float *)ds, dv, 0, (float *)dh, (float *)dvh, nullptr, smp->seed,
                            sample_threshold(smp->probability))))
        return rc;
    if ((rc = download(ctx, hints_out, dh, bytes))) return rc;
    if (dvh && (rc = download(ctx, validhints_out, dvh, bytes))) return rc;
    VPPX_HIP(hipStreamSynchronize(ctx->stream));
    return 0;
}

// The sampled call: the hints (and, guided, their mask) of the batch are sampled into the workspace in front of the scaled /
// evaluating call, which then takes them exactly where a caller's maps would enter.  With vppx_set_pipeline the sampling is the
// first kernel of the front stage, as the resize of a scaled call is: it waits for what every front stage waits for and writes
// the set of maps the previous call did not use.  src == NULL: gt / validgt are the source.  validsrc / validgt: float32, or one
// byte per pixel (a frame stream's ring).
static int sampled_call(vppx_ctx *ctx, const HotCall &c)
{
    int rc;
    const char *const name = "vppx_occ_vpp_rsgm_sampled";
    const VppxSampleParams *const smp = c.smp;
    const int B = c.B, H = c.H, W = c.W;
    if (c.vp_null || !c.rp || !smp || !c.left || !c.right || !c.disp_out) { vppx_set_error("%s: NULL argument", name); return VPPX_E_INVALID_ARG; }
    const bool eval = c.gt || c.validgt || c.metrics_out;
    if (eval && (!c.gt || !c.validgt || !c.metrics_out)) { vppx_set_error("%s: gt, validgt and metrics_out go together", name); return VPPX_E_INVALID_ARG; }
    if (!eval && (c.ep || c.errormap)) { vppx_set_error("%s: ep / errormap without gt, validgt and metrics_out", name); return VPPX_E_INVALID_ARG; }
    if ((c.src != nullptr) != (c.validsrc != nullptr)) { vppx_set_error("%s: src and validsrc go together", name); return VPPX_E_INVALID_ARG; }
    const float *src = c.src;
    const void *validsrc = c.validsrc;
    int vsrc_is_u8 = c.vsrc_is_u8;
    if (!src) {
        if (!c.gt) { vppx_set_error("%s: src is NULL and there is no gt to sample from", name); return VPPX_E_INVALID_ARG; }
        src = c.gt;
        validsrc = c.validgt;
        vsrc_is_u8 = c.valid_is_u8;
    }
    if ((rc = check_sample_args(name, smp, B, H, W))) return rc;
    const VppxScaleParams one = {1, 1};
    HotCall run = c; // the scaled / evaluating call behind the sampling
    if (!run.sp) run.sp = &one;
    {   // everything the call itself would refuse is refused before the sampling is queued
        int h, w, Ho, Wo, s = 1;
        if ((rc = vppx_scaled_shape(H, W, run.sp, &h, &w, &Ho, &Wo))) return rc;
        if ((rc = check_frames(B, H, W, c.C))) return rc;
        if ((rc = check_frames(B, h, w, c.C))) return rc;
        if ((rc = check_vpp_params(c.vp))) return rc;
        if ((rc = check_rsgm_params(*c.rp))) return rc;
        if (eval && (rc = check_metrics_args(name, c.ep, B, Ho, Wo, H, W, &s))) return rc;
    }
    if ((rc = lockstep_check(ctx))) return rc;
    const int set = pipeline_applies(ctx) ? ctx->sample_parity : 0;
    ctx->last_sample_set = set;
    const size_t np = (size_t)B * H * W;
    float *gs, *vs = nullptr;
    if ((rc = ws_get(ctx, set ? WS_SAMPLE_G1 : WS_SAMPLE_G0, np, &gs))) return rc;
    if ((c.guided || c.validhints_out) && (rc = ws_get(ctx, set ? WS_SAMPLE_V1 : WS_SAMPLE_V0, np, &vs))) return rc;
    const u32 T = sample_threshold(smp->probability);
    if ((rc = pre_front(ctx, &ctx->ev_sampled, &ctx->sample_parity,
                        [&]() { return sample_launch(ctx, B, (size_t)H * W, src, validsrc, vsrc_is_u8, gs, vs, nullptr, smp->seed, T); })))
        return rc;
    run.g = gs;
    run.validhints = c.guided ? vs : nullptr;
    if ((rc = eval ? eval_call(ctx, run) : scaled_call(ctx, run))) return rc;
    // the caller's copies of the maps, in launch-stream order (the launch stream has waited for the front stage by now)
    if (c.hints_out) VPPX_HIP(hipMemcpyAsync(c.hints_out, gs, np * sizeof(float), hipMemcpyDeviceToDevice, ctx->stream));
    if (c.validhints_out) VPPX_HIP(hipMemcpyAsync(c.validhints_out, vs, np * sizeof(float), hipMemcpyDeviceToDevice, ctx->stream));
    return 0;
}

extern "C" int vppx_occ_vpp_rsgm_sampled_dev(vppx_ctx *ctx, const VppxOccParams *op, const VppxVppParams *vp, const VppxRsgmParams *rp,
                                             const VppxScaleParams *sp, const VppxEvalParams *ep, const VppxSampleParams *smp, int B, int H, int W,
                                             int C, const uint8_t *left, const uint8_t *right, const float *src, const float *validsrc, int guided,
                                             const uint8_t *g_occ, const float *gt, const float *validgt, uint8_t *conf_out, uint8_t *l_vpp,
                                             uint8_t *r_vpp, float *disp_out, float *disp_small, VppxMetrics *metrics_out, float *errormap,
                                             float *hints_out, float *validhints_out)
{
    VPPX_ENTER(ctx);
    VPPX_PIPE_KEEP(ctx);
    HotCall c = hot_call(HotCall::SAMPLED, op, vp, rp, B, H, W, C, left, right);
    c.sp = sp; c.ep = ep; c.smp = smp;
    c.g_occ = g_occ;
    c.conf_out = conf_out; c.l_vpp = l_vpp; c.r_vpp = r_vpp; c.disp_out = disp_out; c.disp_small = disp_small;
    c.gt = gt; c.validgt = validgt; c.metrics_out = metrics_out; c.errormap = errormap;
    c.src = src; c.validsrc = validsrc; c.guided = guided; c.hints_out = hints_out; c.validhints_out = validhints_out;
    return vppx_hot_call_internal(ctx, c);
}

// Batches larger than one round of the lock-step kernel are run as consecutive parts of one round each ("batch quantum":
// 16 frames at 540x960x192, 12 at 375x1242x192).  Frames are independent and frame f draws from srand(seed + f) whatever
// the split, so results do not change; what changes is the length of the bursts: 32 frames per launch keep the chip's
// hottest kernel running for 3.5 ms, and it clocks down under its power limit (tools/clock_trace.py: 2.25 -> 2.05 GHz
// inside a step; the kernel takes 3.55 ms inside a step against 3.30 re-launched alone), while 16-frame parts alternate
// 1.65 ms of it with the cooler W/E, sum and post launches (bench at 540x960x192, ms per frame: 16 per call 0.285, 32 per
// call 0.294, 48: 0.290, 24: 0.317 -- 1.5 rounds).  The part in front takes the remainder (or, below 8 frames, rides on
// the first full part) so that the last part -- the one the timing helpers re-launch -- is a whole round.  With
// vppx_set_pipeline the front stage of a part runs under the previous part's sum / WTA and post kernels, as between calls.
// VPPX_CHUNK=0 keeps whole batches, VPPX_CHUNK=n forces parts of n frames.
static int vpp_rsgm_parts(vppx_ctx *ctx, const HotCall &c)
{
    int rc;
    const VppxRsgmParams *const rp = c.rp;
    const int B = c.B, H = c.H, W = c.W, C = c.C;
    const bool validhints = c.validhints != nullptr;
    const int chunk_env = ctx->knobs.chunk;
    int q = 0;
    if (chunk_env > 0) {
        q = chunk_env;
    } else if (chunk_env < 0 && !ctx->is_child && B >= 16 && !validhints) { // (guided calls never take the lock-step kernel)
        RsgmGeom g1;
        make_geom(1, H, W, C, rp->dmax, g1);
        u16 lut[256];
        int maxp2 = 0;
        p2_lut_host(*rp, lut, &maxp2);
        if (!ctx->vert3_broken && ctx->vert3_rest <= 0 && (ctx->vert3_probed || !ctx->capturing) && v3_probe_once(ctx) == 0 && !ctx->vert3_broken) {
            const int fpr = rsgm_vert3_frames_per_round(ctx, g1.Wp, g1.D);
            bool fused = false;
            if (fpr >= 8 && fpr < B) {
                g1.B = fpr;
                if ((rc = fused_layout_wanted(ctx, g1, maxp2, &fused))) return rc;
            }
            if (fused) q = fpr;
        }
    }
    // guided: parts of at most the memory budget; a remainder is a part of its own, never merged into a full one (a forced part
    // of as many frames as the budget holds, plus the remainder, would be past it)
    if (validhints) {
        const int fb = guided_frames_per_part(ctx, H, W, C, rp->dmax);
        if (fb < B && (q <= 0 || q > fb)) q = fb;
    }
    ctx->last_parts = 1;
    if (q <= 0 || q >= B) return vpp_rsgm_one(ctx, c);
    ctx->last_parts = 0;
    void *const inputs_ev = ctx->inputs_ev; // one-shot per CALL: every part's front stage may start on it
    // The plan.  Forced part sizes (VPPX_CHUNK=n): the remainder first, riding on the first full part below 8 frames (unguided).  Default
    // (q = one round of the lock-step kernel): whole rounds; a remainder is spread over them when that adds at most a third
    // of a round to each -- such a part runs its whole round, then the extra frames as an under-filled lock-step launch next
    // to its W/E launch (rsgm_vert3_plan), which costs less than a part of its own with its exposed front / post tail
    // (375x1242x192, 32 frames, q = 12: 16 + 16 instead of 8 + 12 + 12: 8.80 -> 8.49 ms) -- else it is a part of its own, first.
    std::vector<int> plan;
    {
        const int k = B / q, r = B % q;
        if (chunk_env < 0 && !validhints && r > 0 && k >= 1 && 3 * ((r + k - 1) / k) <= q) {
            for (int i = 0; i < k; i++) plan.push_back(q + r / k + (i < r % k ? 1 : 0));
        } else {
            int left_over = B;
            while (left_over > 0) {
                int nb = left_over % q;
                if (nb == 0) nb = q;
                else if (nb < 8 && left_over > q && !validhints) nb += q; // a few frames do not make a launch of their own
                plan.push_back(nb);
                left_over -= nb;
            }
        }
    }
    int lo = 0;
    unsigned long long *const draws_base = ctx->draws_dst;
    struct DrawsRestore { vppx_ctx *c; unsigned long long *p; ~DrawsRestore() { c->draws_dst = p; } } draws_restore{ctx, draws_base};
    for (size_t pi = 0; pi < plan.size(); pi++) {
        const int nb = plan[pi];
        ctx->inputs_ev = inputs_ev;
        ctx->stage_append = lo > 0;
        ctx->draws_dst = draws_base ? draws_base + lo : nullptr;
        rc = vpp_rsgm_one(ctx, c.frames(lo, nb));
        ctx->stage_append = false;
        if (rc) return rc;
        ctx->last_parts++;
        lo += nb;
    }
    return 0;
}

extern "C" int vppx_last_call_parts(vppx_ctx *ctx) { return ctx ? ctx->last_parts : 0; }
extern "C" int vppx_we_last_pieces(vppx_ctx *ctx) { return ctx ? ctx->we_last_pieces : 0; }
extern "C" int vppx_wsum_last_pieces(vppx_ctx *ctx) { return ctx ? ctx->wsum_last_pieces : 0; }
extern "C" int vppx_wsum_default_route(int B, int Hp, int Wp, int dmax, int p2max, int nsimd)
{
    return rsgm_wsum_default(B, Hp, Wp, dmax, p2max, nsimd) ? 1 : 0;
}

// The parts of a call and, for an evaluating call whose map is complete with them, its metrics: once, over the whole batch,
// behind the last part -- and inside the capture when the call is being captured.
static int vpp_rsgm_parts_eval(vppx_ctx *ctx, const HotCall &c)
{
    const int rc = vpp_rsgm_parts(ctx, c);
    if (rc || !c.metrics_out) return rc;
    return eval_launch(ctx, c, c.H, c.W, c.disp_out);
}

static int vpp_rsgm_entry(vppx_ctx *ctx, const HotCall &c)
{
    int rc;
    routes_reset(ctx); // (sub-stream children record into their own lists: not merged here)
    if (!ctx->front_routes_keep) front_routes_reset(ctx);
    ctx->front_routes_keep = false;
    const size_t front_base = ctx->front_routes.size(); // (what a host wrapper queued before this: not part of a captured graph)
    if ((rc = lockstep_check(ctx))) return rc;
    if (c.vp_null || !c.rp || !c.left || !c.right || !c.g || !c.disp_out) { vppx_set_error("vppx_vpp_rsgm: NULL argument"); return VPPX_E_INVALID_ARG; }
    const VppxRsgmParams *const rp = c.rp;
    const int B = c.B;
    if ((rc = check_frames(B, c.H, c.W, c.C))) return rc;
    if ((rc = check_vpp_params(c.vp))) return rc;
    if ((rc = check_rsgm_params(*rp))) return rc;
    if (ctx->inputs_ev && !pipeline_applies(ctx)) { // not pipelined: the inputs event is simply waited for on the launch stream
        VPPX_HIP(hipStreamWaitEvent(ctx->stream, (hipEvent_t)ctx->inputs_ev, 0));
        ctx->inputs_ev = nullptr;
    }
    const int nsub = (ctx->stage_timing || ctx->is_child) ? 1 : (B >= 2 * ctx->nsub ? ctx->nsub : 1);
    if (nsub <= 1 && ctx->graph_mode && !ctx->stage_timing) {
        // hipGraph replay: launch-bound small batches pay ~40 kernel launches per call otherwise
        vppx_ctx::GraphKey key;
        memset(&key, 0, sizeof(key));
        key.B = B; key.H = c.H; key.W = c.W; key.C = c.C; key.vp = c.vp; key.rp = *rp;
        key.ptr[0] = c.left; key.ptr[1] = c.right; key.ptr[2] = c.g; key.ptr[3] = c.g_occ; key.ptr[4] = c.l_vpp; key.ptr[5] = c.r_vpp;
        key.ptr[6] = c.disp_out; key.ptr[7] = c.conf_out; key.ptr[8] = c.validhints;
        key.has_op = c.op ? 1 : 0;
        if (c.op) key.op = *c.op;
        key.stream = (void *)ctx->stream;
        if (c.metrics_out) { // (the metrics this call queues itself: they are part of the captured graph)
            key.eval_ptr[0] = c.gt; key.eval_ptr[1] = c.validgt; key.eval_ptr[2] = c.metrics_out; key.eval_ptr[3] = c.errormap;
            key.eval_scale[0] = c.gt_scale; key.eval_scale[1] = c.Hg; key.eval_scale[2] = c.Wg; key.eval_scale[3] = c.valid_is_u8;
        }
        key.ws_gen = ctx->ws_gen;
        // the graph does not contain the penalty-table upload: it must still be the table of these parameters
        const bool lut_ok = ctx->lut_valid && ctx->lut_p2min == rp->p2min && ctx->lut_gamma == rp->gamma && ctx->lut_alpha == rp->alpha;
        if (lut_ok && ctx->gexec && ctx->have_gkey && memcmp(&key, &ctx->gkey, sizeof(key)) == 0) {
            VPPX_HIP(hipGraphLaunch(ctx->gexec, ctx->stream));
            ctx->graph_replays++;
            ctx->routes = ctx->graph_routes; // what the captured call launched
            for (const std::string &r : ctx->graph_front_routes) front_route_note(ctx, "%s", r.c_str());
            return 0;
        }
        if (lut_ok && ctx->have_lastkey && memcmp(&key, &ctx->lastkey, sizeof(key)) == 0) {
            // second identical call (the first one sized the workspace and warmed every lazy init): capture it
            if (ctx->gexec) { (void)hipGraphExecDestroy(ctx->gexec); ctx->gexec = nullptr; ctx->have_gkey = false; }
            hipError_t e = hipStreamBeginCapture(ctx->stream, hipStreamCaptureModeThreadLocal);
            if (e == hipSuccess) {
                ctx->capturing = true;
                rc = vpp_rsgm_parts_eval(ctx, c);
                ctx->capturing = false;
                hipGraph_t graph = nullptr;
                e = hipStreamEndCapture(ctx->stream, &graph);
                if (rc != 0) { // the call itself failed (its message stands): that is not "capture impossible"
                    if (graph) (void)hipGraphDestroy(graph);
                    (void)hipGetLastError();
                    ctx->have_lastkey = false;
                    return rc;
                }
                if (e == hipSuccess && graph) {
                    e = hipGraphInstantiate(&ctx->gexec, graph, nullptr, nullptr, 0);
                    (void)hipGraphDestroy(graph);
                    if (e == hipSuccess) {
                        ctx->gkey = key;
                        ctx->have_gkey = true;
                        ctx->graph_routes = ctx->routes;
                        ctx->graph_front_routes.assign(ctx->front_routes.begin() + front_base, ctx->front_routes.end());
                        ctx->graph_captures++;
                        VPPX_HIP(hipGraphLaunch(ctx->gexec, ctx->stream));
                        ctx->graph_replays++;
                        return 0;
                    }
                    ctx->gexec = nullptr;
                } else if (graph) {
                    (void)hipGraphDestroy(graph);
                }
            }
            // capture is not possible here (e.g. the legacy default stream): stay on the eager path
            (void)hipGetLastError();
            ctx->graph_mode = false;
            return vpp_rsgm_parts_eval(ctx, c);
        }
        rc = vpp_rsgm_parts_eval(ctx, c);
        key.ws_gen = ctx->ws_gen; // the workspace as this call left it
        ctx->lastkey = key;
        ctx->have_lastkey = (rc == 0);
        return rc;
    }
    if (nsub <= 1) return vpp_rsgm_parts_eval(ctx, c);
    // Frames are independent: split the batch over child contexts (own stream + arena).  The
    // latency-bound stages of one part (VPP replay, post-processing) then overlap the
    // bandwidth-bound stages of another (aggregation stores, sum/WTA loads).
    for (int i = 0; i < nsub; i++) {
        if (!ctx->sub[i]) {
            if ((rc = vppx_create(&ctx->sub[i], ctx->device))) return rc;
            ctx->sub[i]->is_child = true;
            // the fused vertical kernel needs all blocks of a (frame, pass) group resident together; two such launches
            // racing for the same slots on concurrent streams can starve each other (bounded polls would notice, but
            // why try): sub-stream parts stay on the line-parallel kernel
            ctx->sub[i]->use_vert = (ctx->use_vert == 1) ? 1 : 0;
            VPPX_HIP(hipEventCreateWithFlags(&ctx->sub_done[i], hipEventDisableTiming));
        }
    }
    VPPX_HIP(hipEventRecord(ctx->ev_fork, ctx->stream));
    int lo = 0;
    for (int i = 0; i < nsub; i++) {
        const int nb = B / nsub + (i < B % nsub ? 1 : 0);
        vppx_ctx *sub = ctx->sub[i];
        VPPX_HIP(hipStreamWaitEvent(sub->stream, ctx->ev_fork, 0));
        // (a guided part goes through the parts of its own context: the memory budget holds for it as well)
        const HotCall part = c.frames(lo, nb);
        if ((rc = c.validhints ? vpp_rsgm_parts(sub, part) : vpp_rsgm_one(sub, part))) return rc;
        VPPX_HIP(hipEventRecord(ctx->sub_done[i], sub->stream));
        VPPX_HIP(hipStreamWaitEvent(ctx->stream, ctx->sub_done[i], 0));
        lo += nb;
    }
    if (c.metrics_out && (rc = eval_launch(ctx, c, c.H, c.W, c.disp_out))) return rc;
    // timing helpers look at the last geometry of the first child
    ctx->have_last = false;
    ctx->last_parts = 0; // the children's arenas hold the per-frame draw totals, not this context's (vppx_occ_vpp_rsgm_host reports 0)
    return 0;
}

// ---------------------------------------------------------------------------------------
// occlusion heuristic
// ---------------------------------------------------------------------------------------
extern "C" int vppx_occlusion_heuristic_dev(vppx_ctx *ctx, int B, int H, int W, const float *hints, int rx, int ry,
                                            double l, double g, double th_conf, double th_filter, uint8_t *conf_out)
{
    return vppx_occlusion_heuristic_full_dev(ctx, B, H, W, hints, rx, ry, l, g, th_conf, th_filter, nullptr, conf_out);
}

extern "C" int vppx_occlusion_heuristic_full_dev(vppx_ctx *ctx, int B, int H, int W, const float *hints, int rx, int ry,
                                                 double l, double g, double th_conf, double th_filter, float *dmap_out,
                                                 uint8_t *conf_out)
{
    int rc;
    VPPX_ENTER(ctx); // (like every entry point but the two pipelined ones: the next front stage waits for the launch stream)
    if ((rc = lockstep_check(ctx))) return rc;
    if (!hints || !conf_out || B <= 0 || H <= 0 || W <= 0) { vppx_set_error("vppx_occlusion_heuristic: bad arguments"); return VPPX_E_INVALID_ARG; }
    const size_t n = (size_t)B * H * W;
    float *omap;
    if ((rc = ws_get(ctx, WS_OCC_OMAP, n, &omap))) return rc;
    ctx->front_lds_budget = 64 * 1024;
    front_routes_reset(ctx);
    return occ_launch(ctx, B, H, W, hints, rx, ry, l, g, th_conf, th_filter, omap, conf_out, dmap_out);
}

// Cross-call pipelining of vppx_occ_vpp_rsgm_dev / vppx_vpp_rsgm_dev (contract: include/vppx.h).  Off by default.
extern "C" int vppx_set_pipeline(vppx_ctx *ctx, int on)
{
    int rc;
    VPPX_ENTER(ctx);
    (void)rc;
    ctx->pipeline = on != 0;
    ctx->have_agg_done = false;
    return 0;
}

extern "C" int vppx_occlusion_heuristic_host(vppx_ctx *ctx, int B, int H, int W, const float *hints, int rx, int ry,
                                             double l, double g, double th_conf, double th_filter, uint8_t *conf_out)
{
    return vppx_occlusion_heuristic_full_host(ctx, B, H, W, hints, rx, ry, l, g, th_conf, th_filter, nullptr, conf_out);
}

extern "C" int vppx_occlusion_heuristic_full_host(vppx_ctx *ctx, int B, int H, int W, const float *hints, int rx, int ry,
                                                  double l, double g, double th_conf, double th_filter, float *dmap_out,
                                                  uint8_t *conf_out)
{
    int rc;
    VPPX_ENTER(ctx);
    if (!hints || !conf_out || B <= 0 || H <= 0 || W <= 0) { vppx_set_error("vppx_occlusion_heuristic: bad arguments"); return VPPX_E_INVALID_ARG; }
    const size_t n = (size_t)B * H * W;
    void *dh, *dc, *dd = nullptr;
    if ((rc = upload(ctx, WS_STAGE_A, hints, n * sizeof(float), &dh))) return rc;
    if ((rc = ws_reserve(ctx, WS_STAGE_B, n, &dc))) return rc;
    if (dmap_out && (rc = ws_reserve(ctx, WS_STAGE_C, n * sizeof(float), &dd))) return rc;
    if ((rc = vppx_occlusion_heuristic_full_dev(ctx, B, H, W, (const float *)dh, rx, ry, l, g, th_conf, th_filter, (float *)dd, (u8 *)dc))) return rc;
    if ((rc = download(ctx, conf_out, dc, n))) return rc;
    if (dmap_out && (rc = download(ctx, dmap_out, dd, n * sizeof(float)))) return rc;
    VPPX_HIP(hipStreamSynchronize(ctx->stream));
    return 0;
}

// ---------------------------------------------------------------------------------------
// pyrSGM-compatible stage entry points (host pointers, one frame)
// ---------------------------------------------------------------------------------------
static int check_w16(int w)
{
    if (w % 16 != 0) { vppx_set_error("Invalid width (%d): width %% 16 != 0", w); return VPPX_E_WIDTH_MOD16; }
    return 0;
}
static int check_dmax(int dmax)
{
    if (dmax % 8 != 0) { vppx_set_error("Invalid dmax (%d): dmax %% 8 != 0", dmax); return VPPX_E_DMAX_MOD8; }
    if (dmax > 256) { vppx_set_error("Invalid dmax (%d): dmax > 256", dmax); return VPPX_E_DMAX_GT256; }
    if (dmax <= 0) { vppx_set_error("Invalid dmax (%d)", dmax); return VPPX_E_INVALID_ARG; }
    return 0;
}

extern "C" int vppx_census5x5(vppx_ctx *ctx, const uint8_t *img, uint32_t *out, int w, int h)
{
    int rc;
    VPPX_ENTER(ctx);
    if (!img || !out || w <= 0 || h <= 0) { vppx_set_error("vppx_census5x5: bad arguments"); return VPPX_E_INVALID_ARG; }
    if ((rc = check_w16(w))) return rc;
    const size_t n = (size_t)w * h;
    void *di, *dout;
    if ((rc = upload(ctx, WS_STAGE_A, img, n, &di))) return rc;
    if ((rc = ws_reserve(ctx, WS_STAGE_B, n * sizeof(u32), &dout))) return rc;
    if ((rc = rsgm_launch_census(ctx, 1, h, w, (const u8 *)di, (u32 *)dout))) return rc;
    if ((rc = download(ctx, out, dout, n * sizeof(u32)))) return rc;
    VPPX_HIP(hipStreamSynchronize(ctx->stream));
    return 0;
}

extern "C" int vppx_cost_census5x5_xyd(vppx_ctx *ctx, const uint32_t *cl, const uint32_t *cr, uint16_t *dsi, int w, int h,
                                       int dmax, int n_threads_ignored)
{
    (void)n_threads_ignored;
    int rc;
    VPPX_ENTER(ctx);
    if (!cl || !cr || !dsi || w <= 0 || h <= 0) { vppx_set_error("vppx_cost: bad arguments"); return VPPX_E_INVALID_ARG; }
    if ((rc = check_dmax(dmax))) return rc;
    if ((rc = check_w16(w))) return rc;
    const size_t n = (size_t)w * h;
    void *dcl, *dcr, *dd;
    if ((rc = upload(ctx, WS_STAGE_A, cl, n * sizeof(u32), &dcl))) return rc;
    if ((rc = upload(ctx, WS_STAGE_B, cr, n * sizeof(u32), &dcr))) return rc;
    if ((rc = ws_reserve(ctx, WS_DSI, n * dmax * sizeof(u16), &dd))) return rc;
    if ((rc = rsgm_launch_cost(ctx, 1, h, w, dmax, (const u32 *)dcl, (const u32 *)dcr, (u16 *)dd))) return rc;
    if ((rc = download(ctx, dsi, dd, n * dmax * sizeof(u16)))) return rc;
    VPPX_HIP(hipStreamSynchronize(ctx->stream));
    return 0;
}

extern "C" int vppx_aggregate(vppx_ctx *ctx, const uint8_t *img, const uint16_t *dsi, uint16_t *dsi_agg, int w, int h,
                              int dmax, int p1, int p2min, float alpha, int gamma)
{
    return vppx_aggregate_img(ctx, img, 1, dsi, dsi_agg, w, h, dmax, p1, p2min, alpha, gamma);
}

// rsgm.py:270 hands aggregate_SSE the padded H x W x 3 COLOUR image although the native reads one byte per pixel.
// What upstream does with it is unknown (parity unpinned); this build defines the P2 image of every route as
// gray(left), so a 3-channel image is converted on the device exactly like the fused compute_rsgm does.
extern "C" int vppx_aggregate_img(vppx_ctx *ctx, const uint8_t *img, int channels, const uint16_t *dsi, uint16_t *dsi_agg,
                                  int w, int h, int dmax, int p1, int p2min, float alpha, int gamma)
{
    int rc;
    VPPX_ENTER(ctx);
    routes_reset(ctx);
    if (!img || !dsi || !dsi_agg || w <= 0 || h <= 0) { vppx_set_error("vppx_aggregate: bad arguments"); return VPPX_E_INVALID_ARG; }
    if (channels != 1 && channels != 3) { vppx_set_error("vppx_aggregate: image must have 1 or 3 channels (got %d)", channels); return VPPX_E_INVALID_ARG; }
    if ((rc = check_w16(w))) return rc; // rsgm.py:51-58 order
    if ((rc = check_dmax(dmax))) return rc;
    const size_t n = (size_t)w * h, nc = n * dmax;
    VppxRsgmParams p;
    vppx_rsgm_params_default(&p);
    p.dmax = dmax; p.p1 = p1; p.p2min = p2min; p.alpha = alpha; p.gamma = gamma;
    u16 lut_h[256];
    int maxp2;
    p2_lut_host(p, lut_h, &maxp2);
    void *dimg, *ddsi, *paths;
    u16 *lut_d, *S;
    if ((rc = upload(ctx, WS_STAGE_A, img, n * channels, &dimg))) return rc;
    if (channels == 3) {
        u8 *gray;
        // the gray image goes where the last call's may lie (and a larger one moves the buffer): the timing helpers have nothing
        // to re-launch on until the next rSGM call
        ctx->have_last = false;
        if ((rc = ws_get(ctx, WS_GRAY_L, n, &gray))) return rc;
        RsgmGeom g1;
        g1.B = 1; g1.H = g1.Hp = h; g1.W = g1.Wp = w; g1.C = 3; g1.D = dmax;
        g1.pad_l = g1.pad_r = g1.pad_t = g1.pad_b = 0;
        if ((rc = rsgm_launch_pad_gray(ctx, g1, (const u8 *)dimg, gray))) return rc;
        dimg = gray;
    }
    if ((rc = upload(ctx, WS_DSI, dsi, nc * sizeof(u16), &ddsi))) return rc;
    if ((rc = ws_get(ctx, WS_P2LUT, 256, &lut_d))) return rc;
    VPPX_HIP(hipMemcpyAsync(lut_d, lut_h, sizeof(lut_h), hipMemcpyHostToDevice, ctx->stream));
    ctx->lut_valid = false; // the fused path's cached table was overwritten
    if ((rc = ws_reserve(ctx, WS_PATHS, nc * 8 * 2, &paths))) return rc;
    if ((rc = ws_get(ctx, WS_S, nc, &S))) return rc;
    if ((rc = rsgm_launch_paths(ctx, 1, h, w, dmax, (const u8 *)dimg, nullptr, nullptr, (const u16 *)ddsi, lut_d, p1, paths, 2, 0xFF))) return rc;
    if ((rc = rsgm_launch_sum_wta(ctx, 1, h, w, dmax, paths, 2, S, nullptr, nullptr, 0, 0))) return rc;
    if ((rc = download(ctx, dsi_agg, S, nc * sizeof(u16)))) return rc;
    VPPX_HIP(hipStreamSynchronize(ctx->stream));
    return 0;
}

static int wta_common(vppx_ctx *ctx, const uint16_t *dsi, float *disp, int w, int h, int dmax, float uniqueness, int which)
{
    int rc;
    VPPX_ENTER(ctx);
    if (!dsi || !disp || w <= 0 || h <= 0) { vppx_set_error("vppx_match_wta: bad arguments"); return VPPX_E_INVALID_ARG; }
    if ((rc = check_w16(w))) return rc;
    if ((rc = check_dmax(dmax))) return rc;
    if (which != 2 && (uniqueness > 1.0f || uniqueness <= 0.0f)) {
        vppx_set_error("Invalid uniqueness (%g): uniqueness in ]0,1]", (double)uniqueness);
        return VPPX_E_UNIQUENESS;
    }
    const size_t n = (size_t)w * h, nc = n * dmax;
    void *dS, *dd;
    if ((rc = upload(ctx, WS_S, dsi, nc * sizeof(u16), &dS))) return rc;
    if (which == 2) {
        if ((rc = upload(ctx, WS_DISP_L0, disp, n * sizeof(float), &dd))) return rc;
        if ((rc = rsgm_launch_subpixel(ctx, 1, h, w, dmax, (const u16 *)dS, (float *)dd))) return rc;
    } else {
        if ((rc = ws_reserve(ctx, WS_DISP_L0, n * sizeof(float), &dd))) return rc;
        const u32 fu = uniq_factor(uniqueness);
        if (which == 0) rc = rsgm_launch_wta_left(ctx, 1, h, w, dmax, (const u16 *)dS, (float *)dd, fu);
        else rc = rsgm_launch_wta_right(ctx, 1, h, w, dmax, (const u16 *)dS, (float *)dd, fu);
        if (rc) return rc;
    }
    if ((rc = download(ctx, disp, dd, n * sizeof(float)))) return rc;
    VPPX_HIP(hipStreamSynchronize(ctx->stream));
    return 0;
}

extern "C" int vppx_match_wta(vppx_ctx *ctx, const uint16_t *dsi, float *disp, int w, int h, int dmax, float uniqueness)
{
    return wta_common(ctx, dsi, disp, w, h, dmax, uniqueness, 0);
}
extern "C" int vppx_match_wta_right(vppx_ctx *ctx, const uint16_t *dsi, float *disp, int w, int h, int dmax, float uniqueness)
{
    return wta_common(ctx, dsi, disp, w, h, dmax, uniqueness, 1);
}
extern "C" int vppx_subpixel_refine(vppx_ctx *ctx, const uint16_t *dsi, float *disp, int w, int h, int dmax, int method)
{
    if (method != 0) return 0; // only the equiangular method is used by the reference (rsgm.py:142)
    return wta_common(ctx, dsi, disp, w, h, dmax, 1.0f, 2);
}

extern "C" int vppx_median3x3(vppx_ctx *ctx, const float *src, float *dst, int w, int h)
{
    int rc;
    VPPX_ENTER(ctx);
    if (!src || !dst || w <= 0 || h <= 0) { vppx_set_error("vppx_median3x3: bad arguments"); return VPPX_E_INVALID_ARG; }
    const size_t n = (size_t)w * h;
    void *ds, *dd;
    if ((rc = upload(ctx, WS_DISP_L0, src, n * sizeof(float), &ds))) return rc;
    if ((rc = ws_reserve(ctx, WS_DISP_L1, n * sizeof(float), &dd))) return rc;
    if ((rc = rsgm_launch_median(ctx, 1, h, w, (const float *)ds, (float *)dd))) return rc;
    if ((rc = download(ctx, dst, dd, n * sizeof(float)))) return rc;
    VPPX_HIP(hipStreamSynchronize(ctx->stream));
    return 0;
}

// ---------------------------------------------------------------------------------------
// measurement helper: time the dominant kernel alone with hipEvents on the launch stream
// ---------------------------------------------------------------------------------------
// The event pair around `iters` re-launches.  The events it creates are the caller's to destroy, whatever this returns.
static int timed_relaunches(vppx_ctx *ctx, const RsgmGeom &g, const u16 *lut_d, int maxp2, int iters, int which, hipEvent_t *e0,
                            hipEvent_t *e1, float *ms_out)
{
    VPPX_HIP(hipEventCreate(e0));
    VPPX_HIP(hipEventCreate(e1));
    const void *vols[8];
    int nvol, eb, rc = 0;
    // what the call decided stays the call's: a re-launch counts as no call of a context that rests after a lost lock step,
    // and leaves the W route flag, which rsgm_core reads behind its own run_aggregation, as it found it
    const int rest = ctx->vert3_rest;
    const bool wsum = ctx->wsum_route;
    VPPX_HIP(hipEventRecord(*e0, ctx->stream));
    ctx->timing_run = true;
    for (int i = 0; i < iters && rc == 0; i++)
        rc = run_aggregation(ctx, ctx->last_rp, g, ctx->last_gl, ctx->last_cl, ctx->last_cr, lut_d, maxp2, vols, &nvol, &eb, which);
    ctx->timing_run = false;
    ctx->vert3_rest = rest;
    ctx->wsum_route = wsum;
    if (rc) return rc;
    float ms = 0.f;
    VPPX_HIP(hipEventRecord(*e1, ctx->stream));
    VPPX_HIP(hipEventSynchronize(*e1));
    VPPX_HIP(hipEventElapsedTime(&ms, *e0, *e1));
    *ms_out = ms / (float)iters;
    return 0;
}

// which: 0 = the whole aggregation stage of the last call, 1 = its W/E launch alone, 2 = its lock-step launches alone (fused
// layout only).  Re-launches on the images, the penalties and the geometry the last call left (last_gl / last_cl / last_cr,
// last_rp); everything that could make that another launch than the call's, or a launch on memory that is no longer the
// call's, is refused BEFORE anything is queued, with *ms_out untouched.
static int time_aggregation(vppx_ctx *ctx, int iters, int which, float *ms_out)
{
    int rc;
    VPPX_ENTER(ctx);
    if (!ctx->have_last && ctx->sub[0] && ctx->sub[0]->have_last) ctx = ctx->sub[0]; // batch was split: time one part
    ctx->timing_routes.clear();
    if (iters <= 0) { vppx_set_error("vppx_time_aggregate: iters must be positive (got %d)", iters); return VPPX_E_INVALID_ARG; }
    if (!ms_out) { vppx_set_error("vppx_time_aggregate: ms_out is NULL"); return VPPX_E_INVALID_ARG; }
    if (!ctx->have_last) { vppx_set_error("vppx_time_aggregate: call vppx_rsgm_dev first"); return VPPX_E_INVALID_ARG; }
    if (ctx->last_guided) {
        // the guided launch reads the hint rows from WS_DSI / WS_GUIDED_MAP, which the stage entries overwrite, and the census
        // layout is another kernel on other volumes: nothing here would be the call's aggregation
        vppx_set_error("vppx_time_aggregate: the last call was guided (eight u16 path volumes from the hint rows): its aggregation is not re-launched");
        return VPPX_E_UNSUPPORTED;
    }
    if (which != 0 && ctx->last_vert == 0) {
        vppx_set_error("vppx_time_aggregate_part: the last call ran the eight-path layout (one launch of all eight paths): it has no part %d", which);
        return VPPX_E_UNSUPPORTED;
    }
    const VppxRsgmParams &p = ctx->last_rp;
    // the penalty table of the last call: vppx_aggregate / vppx_aggregate_img upload their own (the hot path's rule, rsgm_core)
    u16 *lut_d;
    if ((rc = ws_get(ctx, WS_P2LUT, 256, &lut_d))) return rc;
    if (!ctx->lut_valid || ctx->lut_p2min != p.p2min || ctx->lut_gamma != p.gamma || ctx->lut_alpha != p.alpha) {
        p2_lut_host(p, ctx->lut_host, &ctx->lut_maxp2);
        VPPX_HIP(hipMemcpyAsync(lut_d, ctx->lut_host, sizeof(ctx->lut_host), hipMemcpyHostToDevice, ctx->stream));
        ctx->lut_p2min = p.p2min; ctx->lut_gamma = p.gamma; ctx->lut_alpha = p.alpha;
        ctx->lut_valid = true;
    }
    const int maxp2 = ctx->lut_maxp2;
    RsgmGeom g;
    g.B = ctx->last_B; g.Hp = ctx->last_Hp; g.Wp = ctx->last_Wp; g.D = ctx->last_D;
    g.H = g.Hp; g.W = g.Wp; g.C = 1; g.pad_l = g.pad_r = g.pad_t = g.pad_b = 0;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    rc = timed_relaunches(ctx, g, lut_d, maxp2, iters, which, &e0, &e1, ms_out);
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    return rc;
}

#ifdef VPPX_EXPERIMENT
// Experiment (tools/overlap_probe.py): the sum / WTA kernel of the last fused call and a W/E launch of the same size started
// TOGETHER on two streams, `iters` times; ms[0] = wall time per pair, ms[1] / ms[2] = each kernel's own duration inside the pair.
// mode 1 = sum only, 2 = W/E only, 3 = both.  The W/E launch writes a scratch volume (the sum keeps reading valid data).
// lds_pad > 0: the W/E blocks ask for that much extra dynamic LDS (caps how many of them fit next to a sum block).
extern "C" int vppx_exp_overlap(vppx_ctx *ctx, int mode, int iters, float *ms)
{
    int rc;
    VPPX_ENTER(ctx);
    if (!ctx->have_last || ctx->last_vert != 3 || iters <= 0 || !ms) { vppx_set_error("vppx_exp_overlap: call the fused path first"); return VPPX_E_INVALID_ARG; }
    const VppxRsgmParams &p = ctx->last_rp;
    u16 lut_h[256];
    int maxp2;
    p2_lut_host(p, lut_h, &maxp2);
    const int B = ctx->last_B, Hp = ctx->last_Hp, Wp = ctx->last_Wp, D = ctx->last_D;
    const size_t ncell = (size_t)B * Hp * Wp * D;
    void *scratch;
    if ((rc = ws_reserve(ctx, WS_DSI, ncell * 2, &scratch))) return rc;
    const void *vols[8] = {ctx->ws[WS_PATHS].p, (const u8 *)ctx->ws[WS_PATHS].p + ncell, ctx->ws[WS_SV].p, (const u8 *)ctx->ws[WS_SV].p + ncell};
    hipStream_t sa = ctx->stream, sb = ctx->stream2;
    hipEvent_t e0, e1, a0, a1, b0, b1, ej;
    for (hipEvent_t *e : {&e0, &e1, &a0, &a1, &b0, &b1, &ej}) VPPX_HIP(hipEventCreate(e));
    VPPX_HIP(hipStreamSynchronize(sa));
    VPPX_HIP(hipStreamSynchronize(sb));
    float tot[3] = {0, 0, 0};
    for (int i = 0; i < iters; i++) {
        VPPX_HIP(hipEventRecord(e0, sa));
        VPPX_HIP(hipStreamWaitEvent(sb, e0, 0));
        if (mode & 2) {
            hipStream_t keep = ctx->stream;
            ctx->stream = sb;
            VPPX_HIP(hipEventRecord(b0, sb));
            rc = rsgm_launch_paths(ctx, B, Hp, Wp, D, ctx->last_gl, ctx->last_cl, ctx->last_cr, nullptr, (const u16 *)ctx->ws[WS_P2LUT].p, p.p1, scratch, 1, 0x11);
            VPPX_HIP(hipEventRecord(b1, sb));
            ctx->stream = keep;
            if (rc) return rc;
        }
        if (mode & 1) {
            VPPX_HIP(hipEventRecord(a0, sa));
            rc = rsgm_launch_sum_wta_lr(ctx, B, Hp, Wp, D, vols, 4, 1, (float *)ctx->ws[WS_DISP_L0].p, (float *)ctx->ws[WS_DISP_R0].p, uniq_factor(p.uniqueness), 1, 24 + maxp2);
            VPPX_HIP(hipEventRecord(a1, sa));
            if (rc) return rc;
        }
        VPPX_HIP(hipEventRecord(ej, sb));
        VPPX_HIP(hipStreamWaitEvent(sa, ej, 0));
        VPPX_HIP(hipEventRecord(e1, sa));
        VPPX_HIP(hipEventSynchronize(e1));
        float t = 0.f;
        VPPX_HIP(hipEventElapsedTime(&t, e0, e1)); tot[0] += t;
        if (mode & 1) { VPPX_HIP(hipEventElapsedTime(&t, a0, a1)); tot[1] += t; }
        if (mode & 2) { VPPX_HIP(hipEventElapsedTime(&t, b0, b1)); tot[2] += t; }
    }
    for (int k = 0; k < 3; k++) ms[k] = tot[k] / (float)iters;
    for (hipEvent_t e : {e0, e1, a0, a1, b0, b1, ej}) (void)hipEventDestroy(e);
    return 0;
}
#endif

// whole aggregation stage (all launches of the 8 paths) per batch
extern "C" int vppx_time_aggregate(vppx_ctx *ctx, int iters, float *ms_out) { return time_aggregation(ctx, iters, 0, ms_out); }
// part: 1 = horizontal line kernel only, 2 = vertical band launches only
extern "C" int vppx_time_aggregate_part(vppx_ctx *ctx, int iters, int part, float *ms_out)
{
    if (part != 1 && part != 2) {
        if (ctx) ((!ctx->have_last && ctx->sub[0] && ctx->sub[0]->have_last) ? ctx->sub[0] : ctx)->timing_routes.clear(); // (nothing launched)
        vppx_set_error("part must be 1 or 2");
        return VPPX_E_INVALID_ARG;
    }
    return time_aggregation(ctx, iters, part, ms_out);
}
// Average duration of the aggregation kernel over the last `last_n` launches made by the pipeline
// (or by vppx_time_aggregate) on this context, from the hipEvent pairs recorded around each launch
// on its own stream.  The caller must have synchronised.  last_n <= 0 resets the launch counter.
extern "C" int vppx_agg_kernel_ms(vppx_ctx *ctx, int last_n, float *avg_ms, int *n_used)
{
    int rc;
    VPPX_ENTER(ctx);
    if (ctx->nsub > 1 && ctx->sub[0]) ctx = ctx->sub[0]; // split batch: one part's launches
    if (last_n <= 0) { ctx->agg_calls = 0; if (n_used) *n_used = 0; if (avg_ms) *avg_ms = 0.f; return 0; }
    if (!avg_ms) return VPPX_E_INVALID_ARG;
    long n = ctx->agg_calls < last_n ? ctx->agg_calls : last_n;
    if (n > vppx_ctx::AGG_RING) n = vppx_ctx::AGG_RING;
    double tot = 0.0;
    for (long i = 0; i < n; i++) {
        const int slot = (int)((ctx->agg_calls - 1 - i) % vppx_ctx::AGG_RING);
        float t = 0.f;
        VPPX_HIP(hipEventSynchronize(ctx->agg_ev[1][slot]));
        VPPX_HIP(hipEventElapsedTime(&t, ctx->agg_ev[0][slot], ctx->agg_ev[1][slot]));
        tot += t;
    }
    *avg_ms = n > 0 ? (float)(tot / (double)n) : 0.f;
    if (n_used) *n_used = (int)n;
    return 0;
}
// The same for the W/E launch of the fused layout (0 launches in the 8-path layout, whose one launch is the one above).
extern "C" int vppx_we_kernel_ms(vppx_ctx *ctx, int last_n, float *avg_ms, int *n_used)
{
    int rc;
    VPPX_ENTER(ctx);
    VPPX_PIPE_KEEP(ctx);
    if (ctx->nsub > 1 && ctx->sub[0]) ctx = ctx->sub[0];
    if (last_n <= 0) { ctx->we_calls = 0; if (n_used) *n_used = 0; if (avg_ms) *avg_ms = 0.f; return 0; }
    if (!avg_ms) return VPPX_E_INVALID_ARG;
    long n = ctx->we_calls < last_n ? ctx->we_calls : last_n;
    if (n > vppx_ctx::AGG_RING) n = vppx_ctx::AGG_RING;
    double tot = 0.0;
    for (long i = 0; i < n; i++) {
        const int slot = (int)((ctx->we_calls - 1 - i) % vppx_ctx::AGG_RING);
        float t = 0.f;
        VPPX_HIP(hipEventSynchronize(ctx->we_ev[1][slot]));
        VPPX_HIP(hipEventElapsedTime(&t, ctx->we_ev[0][slot], ctx->we_ev[1][slot]));
        tot += t;
    }
    *avg_ms = n > 0 ? (float)(tot / (double)n) : 0.f;
    if (n_used) *n_used = (int)n;
    (void)rc;
    return 0;
}
// frames per launch that vppx_time_aggregate re-runs (a split batch is timed on one part)
extern "C" int vppx_time_aggregate_frames(vppx_ctx *ctx)
{
    if (ctx && !ctx->have_last && ctx->sub[0] && ctx->sub[0]->have_last) ctx = ctx->sub[0];
    return (ctx && ctx->have_last) ? ctx->last_B : 0;
}
// how the aggregation stage of the last call was executed: 0 = eight line-parallel paths, 1 = band marching,
// 3 = W/E line-parallel + the fused vertical kernel
extern "C" int vppx_uses_vert(vppx_ctx *ctx)
{
    if (ctx && !ctx->have_last && ctx->sub[0] && ctx->sub[0]->have_last) ctx = ctx->sub[0];
    if (!ctx || !ctx->have_last) return 0;
    return ctx->last_vert;
}

// ---------------------------------------------------------------------------------------
// pictures (utils.py:17-79; test.py:318-343): viz_kernels.hip
// ---------------------------------------------------------------------------------------
static int check_viz_args(const char *name, int B, int H, int W, int dilation, bool all_pointers)
{
    if (!all_pointers) { vppx_set_error("%s: NULL argument", name); return VPPX_E_INVALID_ARG; }
    if (B < 1 || H < 1 || W < 1) { vppx_set_error("%s: bad shape (B %d, %d x %d)", name, B, H, W); return VPPX_E_INVALID_ARG; }
    if (dilation < 0) { vppx_set_error("%s: dilation %d (>= 0)", name, dilation); return VPPX_E_INVALID_ARG; }
    if (dilation > VIZ_MAX_DILATION) {
        vppx_set_error("%s: dilation %d is above this build's limit of %d", name, dilation, VIZ_MAX_DILATION);
        return VPPX_E_UNSUPPORTED;
    }
    return 0;
}

static int check_viz_scale(const char *name, double scale)
{
    if (!(scale > 0.0)) { vppx_set_error("%s: scale %g (> 0)", name, scale); return VPPX_E_INVALID_ARG; }
    return 0;
}

static int check_viz_which(const char *name, unsigned which)
{
    if (which == 0 || (which & ~(unsigned)VPPX_VIZ_ALL)) {
        vppx_set_error("%s: which 0x%x (one or more of the VPPX_VIZ_* bits)", name, which);
        return VPPX_E_INVALID_ARG;
    }
    return 0;
}

extern "C" int vppx_error_colors_dev(vppx_ctx *ctx, int B, int H, int W, const float *errors, const float *mask, double scale, int bgr,
                                     int dilation, uint8_t *out)
{
    VPPX_ENTER(ctx);
    VPPX_PIPE_KEEP(ctx); // (no scratch)
    int rc;
    if ((rc = check_viz_args("vppx_error_colors_dev", B, H, W, dilation, errors && out))) return rc;
    if ((rc = check_viz_scale("vppx_error_colors_dev", scale))) return rc;
    return viz_launch_error_colors(ctx, B, H, W, errors, mask, scale, bgr, dilation, out);
}

extern "C" int vppx_error_colors_host(vppx_ctx *ctx, int B, int H, int W, const float *errors, const float *mask, double scale, int bgr,
                                      int dilation, uint8_t *out)
{
    VPPX_ENTER(ctx);
    int rc;
    if ((rc = check_viz_args("vppx_error_colors_host", B, H, W, dilation, errors && out))) return rc;
    if ((rc = check_viz_scale("vppx_error_colors_host", scale))) return rc;
    const size_t npx = (size_t)B * H * W;
    void *de, *dm = nullptr, *dout;
    if ((rc = upload(ctx, WS_STAGE_A, errors, npx * sizeof(float), &de))) return rc;
    if (mask && (rc = upload(ctx, WS_STAGE_B, mask, npx * sizeof(float), &dm))) return rc;
    if ((rc = ws_reserve(ctx, WS_VIZ_OUT, npx * 3, &dout))) return rc;
    if ((rc = viz_launch_error_colors(ctx, B, H, W, (const float *)de, (const float *)dm, scale, bgr, dilation, (u8 *)dout))) return rc;
    if ((rc = download(ctx, out, dout, npx * 3))) return rc;
    VPPX_HIP(hipStreamSynchronize(ctx->stream));
    return 0;
}

extern "C" int vppx_guided_visualize_dev(vppx_ctx *ctx, int B, int H, int W, const float *disp, const float *gt, const float *valid,
                                         double scale, int dilation, unsigned which, uint8_t *out)
{
    VPPX_ENTER(ctx);
    VPPX_PIPE_KEEP(ctx); // (no scratch)
    int rc;
    if ((rc = check_viz_args("vppx_guided_visualize_dev", B, H, W, dilation, disp && gt && valid && out))) return rc;
    if ((rc = check_viz_which("vppx_guided_visualize_dev", which))) return rc;
    if ((rc = check_viz_scale("vppx_guided_visualize_dev", scale))) return rc;
    return viz_launch_guided(ctx, B, H, W, disp, gt, valid, scale, dilation, which, out);
}

extern "C" int vppx_guided_visualize_host(vppx_ctx *ctx, int B, int H, int W, const float *disp, const float *gt, const float *valid,
                                          double scale, int dilation, unsigned which, uint8_t *out)
{
    VPPX_ENTER(ctx);
    int rc;
    if ((rc = check_viz_args("vppx_guided_visualize_host", B, H, W, dilation, disp && gt && valid && out))) return rc;
    if ((rc = check_viz_which("vppx_guided_visualize_host", which))) return rc;
    if ((rc = check_viz_scale("vppx_guided_visualize_host", scale))) return rc;
    const size_t npx = (size_t)B * H * W;
    void *dd, *dg, *dv, *dout;
    if ((rc = upload(ctx, WS_STAGE_A, disp, npx * sizeof(float), &dd))) return rc;
    if ((rc = upload(ctx, WS_STAGE_B, gt, npx * sizeof(float), &dg))) return rc;
    if ((rc = upload(ctx, WS_STAGE_C, valid, npx * sizeof(float), &dv))) return rc;
    if ((rc = ws_reserve(ctx, WS_VIZ_OUT, 6 * npx * 3, &dout))) return rc;
    if ((rc = viz_launch_guided(ctx, B, H, W, (const float *)dd, (const float *)dg, (const float *)dv, scale, dilation, which, (u8 *)dout)))
        return rc;
    for (int k = 0; k < 6; k++) // the planes that were not asked for stay as the caller left them
        if ((which >> k & 1) && (rc = download(ctx, out + k * npx * 3, (const u8 *)dout + k * npx * 3, npx * 3))) return rc;
    VPPX_HIP(hipStreamSynchronize(ctx->stream));
    return 0;
}

extern "C" int vppx_colorize_dev(vppx_ctx *ctx, int B, int H, int W, const float *x, const float *max_val, const uint8_t *lut,
                                 int dilation, uint8_t *out)
{
    VPPX_ENTER(ctx);
    VPPX_PIPE_KEEP(ctx); // (no scratch)
    int rc;
    if ((rc = check_viz_args("vppx_colorize_dev", B, H, W, dilation, x && max_val && lut && out))) return rc;
    return viz_launch_colorize(ctx, B, H, W, x, max_val, lut, dilation, out);
}

extern "C" int vppx_colorize_host(vppx_ctx *ctx, int B, int H, int W, const float *x, const float *max_val, const uint8_t *lut,
                                  int dilation, uint8_t *out)
{
    VPPX_ENTER(ctx);
    int rc;
    if ((rc = check_viz_args("vppx_colorize_host", B, H, W, dilation, x && max_val && lut && out))) return rc;
    const size_t npx = (size_t)B * H * W;
    const size_t mv_bytes = ((size_t)B * sizeof(float) + 15) & ~(size_t)15;
    void *dx, *daux, *dout;
    if ((rc = upload(ctx, WS_STAGE_A, x, npx * sizeof(float), &dx))) return rc;
    if ((rc = ws_reserve(ctx, WS_VIZ_AUX, mv_bytes + 768, &daux))) return rc;
    VPPX_HIP(hipMemcpyAsync(daux, max_val, (size_t)B * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
    VPPX_HIP(hipMemcpyAsync((u8 *)daux + mv_bytes, lut, 768, hipMemcpyHostToDevice, ctx->stream));
    if ((rc = ws_reserve(ctx, WS_VIZ_OUT, npx * 3, &dout))) return rc;
    if ((rc = viz_launch_colorize(ctx, B, H, W, (const float *)dx, (const float *)daux, (const u8 *)daux + mv_bytes, dilation, (u8 *)dout)))
        return rc;
    if ((rc = download(ctx, out, dout, npx * 3))) return rc;
    VPPX_HIP(hipStreamSynchronize(ctx->stream));
    return 0;
}

extern "C" int vppx_finite_max_dev(vppx_ctx *ctx, int B, int H, int W, const float *x, float *max_out)
{
    VPPX_ENTER(ctx);
    VPPX_PIPE_KEEP(ctx); // (its only scratch is a slot no front stage touches)
    int rc;
    if ((rc = check_viz_args("vppx_finite_max_dev", B, H, W, 0, x && max_out))) return rc;
    if (B > 65535) { vppx_set_error("vppx_finite_max_dev: %d frames, above the limit of 65535 per call", B); return VPPX_E_UNSUPPORTED; }
    float *part = nullptr;
    if ((rc = ws_get(ctx, WS_VIZ_PART, (size_t)B * viz_finite_max_blocks((size_t)H * W), &part))) return rc;
    return viz_launch_finite_max(ctx, B, H, W, x, part, max_out);
}
