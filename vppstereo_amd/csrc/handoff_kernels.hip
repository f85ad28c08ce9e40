// handoff_kernels.hip -- gfx950 kernels for the rows either side of the hot path:
//   * PSMNet concat volume + hint modulation          models/psmnet/psmnet.py:157-197
//   * RAFT-Stereo all-pairs correlation modulation    models/raft_stereo/corr.py:160-178
//   * disparity file payload decoders                 dataloaders/frame_utils.py:34-69
// All of them are HBM streaming kernels (write-bound volume fill; sparse in-place row scaling).
#include "corr_shared.h"

#include <math.h>

// ---------------------------------------------------------------------------------------
// nearest sub-sampling of the hint pair to feature resolution (F.upsample(size=[H//4, W//4],
// mode='nearest'): src = min((int)floorf(dst * (float)in / out), in - 1)), then
//   psmnet: h = hints * valid / 4                     (psmnet.py:186)
//   raft  : h = x * valid - hints * valid / 4         (corr.py:168-169)
// ---------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) subsample_hints_kernel(const float *__restrict__ hints, const float *__restrict__ valid,
                                                              int H, int W, int H4, int W4, float sy, float sx,
                                                              float *__restrict__ hs, float *__restrict__ vs, int raft)
{
    const int x = blockIdx.x * blockDim.x + threadIdx.x;
    const int y = blockIdx.y, b = blockIdx.z;
    if (x >= W4) return;
    int yy = (int)floorf(__fmul_rn((float)y, sy));
    int xx = (int)floorf(__fmul_rn((float)x, sx));
    yy = yy < H - 1 ? yy : H - 1;
    xx = xx < W - 1 ? xx : W - 1;
    const size_t si = ((size_t)b * H + yy) * W + xx;
    const float v = valid[si];
    float h = __fdiv_rn(__fmul_rn(hints[si], v), 4.0f);
    if (raft) h = __fsub_rn(__fmul_rn((float)x, v), h);
    const size_t di = ((size_t)b * H4 + y) * W4 + x;
    hs[di] = h;
    vs[di] = v;
}

// modulation(): (1 - v) + (v * height) * exp(-(d - h)^2 / two_w2), shared with corr_kernels.hip (vppx_internal.h)

// cost[b, c, i, y, x]     = x >= i ? fea_l[b, c, y, x]     : 0
// cost[b, C + c, i, y, x] = x >= i ? fea_r[b, c, y, x - i] : 0      (psmnet.py:157-166), times the
// modulation of (b, i, y, x) when hints are given.  The modulation does not depend on the channel:
// one thread owns VEC consecutive x of one (b, i, y), evaluates it once and streams the 2C channels.
template <int VEC>
__global__ void __launch_bounds__(256) psm_volume_kernel(const float *__restrict__ fl, const float *__restrict__ fr,
                                                         const float *__restrict__ hs, const float *__restrict__ vs,
                                                         int C, int D4, int H4, int W4, float *__restrict__ cost)
{
    const int wv = (W4 + VEC - 1) / VEC;                  // vectors per row (VEC divides W4 when VEC > 1)
    const int pv = blockIdx.x * blockDim.x + threadIdx.x; // flat vector index in the (y, x) plane
    if (pv >= wv * H4) return;
    const int y = pv / wv, x0 = (pv % wv) * VEC;
    const int i = blockIdx.y, b = blockIdx.z;
    float mod[VEC];
    bool any = false;
#pragma unroll
    for (int j = 0; j < VEC; j++) {
        mod[j] = 1.0f;
        if (hs && x0 + j < W4) {
            const size_t pi = ((size_t)b * H4 + y) * W4 + x0 + j;
            const float v = vs[pi];
            if (v != 0.0f) { // v == 0 (or -0): untouched.  The reference's (1 - 0) + 0 * 10 * e is 1 exactly for a finite
                             // hint only; under a non-finite one it is NaN, and this library keeps the cell (vppx.h)
                mod[j] = modulation(v, hs[pi], (float)i, 0.125f); // 2 * (1/4)^2  (psmnet.py:187)
                any = true;
            }
        }
    }
    const size_t plane = (size_t)H4 * W4;
    const float *sl = fl + (size_t)b * C * plane + (size_t)y * W4;
    const float *sr = fr + (size_t)b * C * plane + (size_t)y * W4;
    float *dst = cost + (((size_t)b * 2 * C * D4 + i) * H4 + y) * W4 + x0;
    for (int ch = 0; ch < 2 * C; ch++) {
        const bool right = ch >= C;
        const float *src = right ? sr + (size_t)(ch - C) * plane : sl + (size_t)ch * plane;
        float out[VEC];
#pragma unroll
        for (int j = 0; j < VEC; j++) {
            const int x = x0 + j;
            float val = 0.f;
            if (x < W4 && x >= i) val = src[right ? x - i : x];
            out[j] = any ? __fmul_rn(val, mod[j]) : val;
        }
        float *d = dst + (size_t)ch * D4 * plane;
        if (VEC == 4) {
            typedef float f4 __attribute__((ext_vector_type(4)));
            f4 v4 = {out[0], out[1], out[2], out[3]};
            __builtin_nontemporal_store(v4, (f4 *)d); // written once, read by the next layer much later
        } else {
#pragma unroll
            for (int j = 0; j < VEC; j++)
                if (x0 + j < W4) d[j] = out[j];
        }
    }
}

// corr[b, y, x2, 0, k] *= modulation(b, y, x2; k); rows with valid == 0 are untouched, which is the
// reference's "times exactly 1" for every finite hint (vppx.h has the non-finite case): one 64-lane
// wave per (b, y, x2) row, skipping those.
__global__ void __launch_bounds__(256) raft_modulate_kernel(float *__restrict__ corr, const float *__restrict__ hs,
                                                            const float *__restrict__ vs, size_t nrows, int W3)
{
    const size_t row = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= nrows) return;
    const float v = vs[row];
    if (v == 0.0f) return;
    const float h = hs[row];
    float *p = corr + row * (size_t)W3;
    for (int k = threadIdx.x & 63; k < W3; k += 64) p[k] = __fmul_rn(p[k], modulation(v, h, (float)k, 2.0f));
}

// ---------------------------------------------------------------------------------------
// bfloat16 storage (VPPX_DT_BF16): the same two kernels on 16-bit cells.  Only the storage type differs: a cell is
// widened to float32 (exact), multiplied by the float32 factor above (__fmul_rn) and rounded to bf16 once, to nearest
// even; hs / vs and the factor are never held in bf16.  A cell that is not modulated (no hints, v == 0) keeps its 16
// bits: it does not pass through a float, so NaN payloads, -0 and subnormals survive.
// ---------------------------------------------------------------------------------------
// bf16_widen / bf16_rne / bf16_scale: vppx_internal.h

// the factors of `N` consecutive x of one (b, i, y): mod[j] is valid where bit j of the result is set
template <int N>
__device__ __forceinline__ u32 psm_factors(const float *__restrict__ hs, const float *__restrict__ vs, size_t pi, int x0, int W4,
                                           int i, float *mod)
{
    u32 on = 0;
#pragma unroll
    for (int j = 0; j < N; j++) {
        mod[j] = 1.0f;
        if (hs && x0 + j < W4) {
            const float v = vs[pi + j];
            if (v != 0.0f) { // the float32 kernel's rule: v == 0 (or -0) is untouched
                mod[j] = modulation(v, hs[pi + j], (float)i, 0.125f);
                on |= 1u << j;
            }
        }
    }
    return on;
}

// elements cut .. cut + 7 of the 16 bf16 held in a (0..7) and b (8..15), cut in 0..7 and the same for the whole wave:
// the word part of the shift is two rounds of selects, the odd element one funnel shift per word
__device__ __forceinline__ uint4 bf16_window(const uint4 a, const uint4 b, int cut)
{
    const u32 w[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
    u32 t[6], u[5];
#pragma unroll
    for (int k = 0; k < 6; k++) t[k] = (cut & 4) ? w[k + 2] : w[k];
#pragma unroll
    for (int k = 0; k < 5; k++) u[k] = (cut & 2) ? t[k + 1] : t[k];
    const u32 sh = (cut & 1) * 16;
    return make_uint4(__funnelshift_r(u[0], u[1], sh), __funnelshift_r(u[1], u[2], sh), __funnelshift_r(u[2], u[3], sh),
                      __funnelshift_r(u[3], u[4], sh));
}

// Wide route: W4 % 8 == 0, cost and both feature pointers 16-byte aligned.  One thread owns 8 consecutive x of one
// (b, i, y): one 16-byte nontemporal store per lane and channel.  The left feature is one aligned 16-byte load; the
// right one starts at x0 - i, which is not aligned: it is cut out of the two aligned vectors around it.  The cut
// (x0 - i) & 7 is the same for the whole block (x0 is a multiple of 8, i is the block's).  A vector that lies left of
// the row, or right of it, is loaded from the nearest one inside the row instead: every cell it would feed has x < i
// and is masked to 0 (left), or is not part of the window (right, cut == 0), so both loads are unconditional.
__global__ void __launch_bounds__(256) psm_volume_bf16x8_kernel(const u16 *__restrict__ fl, const u16 *__restrict__ fr,
                                                                const float *__restrict__ hs, const float *__restrict__ vs,
                                                                int C, int D4, int H4, int W4, u16 *__restrict__ cost)
{
    const int wv = W4 / 8;
    const int pv = blockIdx.x * blockDim.x + threadIdx.x;
    if (pv >= wv * H4) return;
    const int y = pv / wv, x0 = (pv % wv) * 8;
    const int i = blockIdx.y, b = blockIdx.z;
    float mod[8];
    u32 on = psm_factors<8>(hs, vs, ((size_t)b * H4 + y) * W4 + x0, x0, W4, i, mod);
    u32 live[4]; // cells with x >= i, as masks over the four packed words
#pragma unroll
    for (int k = 0; k < 4; k++) live[k] = (x0 + 2 * k >= i ? 0x0000FFFFu : 0u) | (x0 + 2 * k + 1 >= i ? 0xFFFF0000u : 0u);
    if (i > x0) on &= i - x0 < 8 ? 0xFFu << (i - x0) : 0u; // a cell with x < i is +0 under any factor, a negative or NaN one included
    const int r0 = x0 - i, cut = r0 & 7, a0 = r0 - cut; // a0: the aligned vector that holds x0 - i (may lie left of the row)
    const int xa = min(max(a0, 0), W4 - 8), xb = min(max(a0 + 8, 0), W4 - 8);
    const size_t plane = (size_t)H4 * W4;
    const u16 *sl = fl + (size_t)b * C * plane + (size_t)y * W4 + x0;
    const u16 *sr = fr + (size_t)b * C * plane + (size_t)y * W4;
    u16 *dst = cost + (((size_t)b * 2 * C * D4 + i) * H4 + y) * W4 + x0;
    for (int ch = 0; ch < 2 * C; ch++) {
        uint4 q;
        if (ch < C) {
            q = *(const uint4 *)(sl + (size_t)ch * plane);
        } else {
            const u16 *s = sr + (size_t)(ch - C) * plane;
            q = bf16_window(*(const uint4 *)(s + xa), *(const uint4 *)(s + xb), cut);
        }
        u32 w[4] = {q.x & live[0], q.y & live[1], q.z & live[2], q.w & live[3]};
        if (on) {
#pragma unroll
            for (int k = 0; k < 4; k++) {
                u32 lo = w[k] & 0xFFFFu, hi = w[k] >> 16;
                if (on & (1u << (2 * k))) lo = bf16_scale(lo, mod[2 * k]);
                if (on & (2u << (2 * k))) hi = bf16_scale(hi, mod[2 * k + 1]);
                w[k] = lo | (hi << 16);
            }
        }
        typedef u32 u4 __attribute__((ext_vector_type(4)));
        const u4 v4 = {w[0], w[1], w[2], w[3]};
        __builtin_nontemporal_store(v4, (u4 *)(dst + (size_t)ch * D4 * plane)); // written once, read by the next layer much later
    }
}

// Narrow route: any W4, any 2-byte-aligned pointer; one cell per thread and channel.
__global__ void __launch_bounds__(256) psm_volume_bf16_kernel(const u16 *__restrict__ fl, const u16 *__restrict__ fr,
                                                              const float *__restrict__ hs, const float *__restrict__ vs, int C,
                                                              int D4, int H4, int W4, u16 *__restrict__ cost)
{
    const int pv = blockIdx.x * blockDim.x + threadIdx.x;
    if (pv >= W4 * H4) return;
    const int y = pv / W4, x = pv % W4;
    const int i = blockIdx.y, b = blockIdx.z;
    float mod;
    const u32 on = psm_factors<1>(hs, vs, ((size_t)b * H4 + y) * W4 + x, x, W4, i, &mod);
    const size_t plane = (size_t)H4 * W4;
    const u16 *sl = fl + (size_t)b * C * plane + (size_t)y * W4;
    const u16 *sr = fr + (size_t)b * C * plane + (size_t)y * W4;
    u16 *dst = cost + (((size_t)b * 2 * C * D4 + i) * H4 + y) * W4 + x;
    for (int ch = 0; ch < 2 * C; ch++) {
        u32 bits = 0;
        if (x >= i) bits = ch < C ? sl[(size_t)ch * plane + x] : sr[(size_t)(ch - C) * plane + x - i];
        if (on && x >= i) bits = bf16_scale(bits, mod); // a cell with x < i is +0 under any factor
        dst[(size_t)ch * D4 * plane] = (u16)bits;
    }
}

// One 64-lane wave per (b, y, x2) row of bf16 cells, rows with v == 0 neither read nor written.  A lane takes two
// cells as one 32-bit word.  A row of an odd W3 may start on an odd element, so the pairs are laid from the row's
// first 4-byte boundary: the cell in front of it, and a last cell without a partner, go as single 16-bit accesses.
// Every access stays inside the row, which belongs to this wave alone.
__global__ void __launch_bounds__(256) raft_modulate_bf16_kernel(u16 *__restrict__ corr, const float *__restrict__ hs,
                                                                 const float *__restrict__ vs, size_t nrows, int W3)
{
    const size_t row = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= nrows) return;
    const float v = vs[row];
    if (v == 0.0f) return;
    const float h = hs[row];
    u16 *p = corr + row * (size_t)W3;
    const int lane = threadIdx.x & 63;
    const int head = (int)(((uintptr_t)p >> 1) & 1); // cells in front of the first 4-byte boundary
    if (head && lane == 0) p[0] = (u16)bf16_scale(p[0], modulation(v, h, 0.0f, 2.0f));
    for (int k = head + 2 * lane; k < W3; k += 128) {
        if (k + 1 < W3) {
            u32 *q = (u32 *)(p + k);
            const u32 w = *q;
            const u32 lo = bf16_scale(w & 0xFFFFu, modulation(v, h, (float)k, 2.0f));
            const u32 hi = bf16_scale(w >> 16, modulation(v, h, (float)(k + 1), 2.0f));
            *q = lo | (hi << 16);
        } else {
            p[k] = (u16)bf16_scale(p[k], modulation(v, h, (float)k, 2.0f));
        }
    }
}

__global__ void __launch_bounds__(256) kitti_decode_kernel(const uint16_t *__restrict__ png, size_t n, float *__restrict__ disp,
                                                           u8 *__restrict__ valid)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float d = __fdiv_rn((float)png[i], 256.0f); // exact for every u16 (frame_utils.py:67)
    disp[i] = d;
    if (valid) valid[i] = d > 0.0f ? 1 : 0;
}

__global__ void __launch_bounds__(256) pfm_decode_kernel(const u32 *__restrict__ raw, int H, int rowwords, int little,
                                                         u32 *__restrict__ out)
{
    const int x = blockIdx.x * blockDim.x + threadIdx.x;
    const int y = blockIdx.y;
    if (x >= rowwords) return;
    u32 w = raw[(size_t)(H - 1 - y) * rowwords + x]; // np.flipud (frame_utils.py:63)
    if (!little) w = __builtin_bswap32(w);
    out[(size_t)y * rowwords + x] = w;
}

// ---------------------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------------------
int handoff_subsample_hints(vppx_ctx *ctx, const float *hints, const float *valid, int B, int H, int W, int H4, int W4, float **hs,
                            float **vs, int raft)
{
    int rc;
    if (H / 4 != H4 || W / 4 != W4) {
        vppx_set_error("hints are %dx%d: sub-sampled by 4 that is %dx%d, but the features are %dx%d", H, W, H / 4, W / 4, H4, W4);
        return VPPX_E_INVALID_ARG;
    }
    if ((rc = ws_get(ctx, WS_HANDOFF_H, (size_t)B * H4 * W4, hs))) return rc;
    if ((rc = ws_get(ctx, WS_HANDOFF_V, (size_t)B * H4 * W4, vs))) return rc;
    volatile float fy = (float)H / (float)H4, fx = (float)W / (float)W4; // float32 scale like ATen
    subsample_hints_kernel<<<dim3((W4 + 255) / 256, H4, B), 256, 0, ctx->stream>>>(hints, valid, H, W, H4, W4, fy, fx, *hs, *vs,
                                                                                   raft);
    VPPX_CHECK_LAUNCH();
    return 0;
}

int handoff_psmnet_cost_volume(vppx_ctx *ctx, const void *fl, const void *fr, const float *hints, const float *valid, int B, int C,
                               int H4, int W4, int H, int W, int maxdisp, void *cost, int dtype)
{
    int rc;
    const int D4 = maxdisp / 4;
    float *hs = nullptr, *vs = nullptr;
    if (hints && (rc = handoff_subsample_hints(ctx, hints, valid, B, H, W, H4, W4, &hs, &vs, 0))) return rc;
    if (D4 > 65535 || B > 65535) {
        vppx_set_error("psmnet cost volume: maxdisp/4 and B must be <= 65535");
        return VPPX_E_UNSUPPORTED;
    }
    if (dtype == VPPX_DT_BF16) {
        const u16 *l = (const u16 *)fl, *r = (const u16 *)fr;
        if (W4 % 8 == 0 && (((uintptr_t)cost | (uintptr_t)fl | (uintptr_t)fr) & 15) == 0) {
            psm_volume_bf16x8_kernel<<<dim3((W4 / 8 * H4 + 255) / 256, D4, B), 256, 0, ctx->stream>>>(l, r, hs, vs, C, D4, H4, W4,
                                                                                                     (u16 *)cost);
        } else {
            psm_volume_bf16_kernel<<<dim3((W4 * H4 + 255) / 256, D4, B), 256, 0, ctx->stream>>>(l, r, hs, vs, C, D4, H4, W4, (u16 *)cost);
        }
    } else if (W4 % 4 == 0 && ((uintptr_t)cost & 15) == 0) {
        psm_volume_kernel<4><<<dim3((W4 / 4 * H4 + 255) / 256, D4, B), 256, 0, ctx->stream>>>((const float *)fl, (const float *)fr, hs, vs,
                                                                                              C, D4, H4, W4, (float *)cost);
    } else {
        psm_volume_kernel<1><<<dim3((W4 * H4 + 255) / 256, D4, B), 256, 0, ctx->stream>>>((const float *)fl, (const float *)fr, hs, vs, C,
                                                                                          D4, H4, W4, (float *)cost);
    }
    VPPX_CHECK_LAUNCH();
    return 0;
}

int handoff_raft_corr_modulate(vppx_ctx *ctx, void *corr, const float *hints, const float *valid, int B, int H4, int W2, int W3, int H,
                               int W, int dtype)
{
    int rc;
    float *hs, *vs;
    if ((rc = handoff_subsample_hints(ctx, hints, valid, B, H, W, H4, W2, &hs, &vs, 1))) return rc;
    const size_t nrows = (size_t)B * H4 * W2;
    const dim3 grid((unsigned)((nrows + 3) / 4));
    if (dtype == VPPX_DT_BF16)
        raft_modulate_bf16_kernel<<<grid, 256, 0, ctx->stream>>>((u16 *)corr, hs, vs, nrows, W3);
    else
        raft_modulate_kernel<<<grid, 256, 0, ctx->stream>>>((float *)corr, hs, vs, nrows, W3);
    VPPX_CHECK_LAUNCH();
    return 0;
}

int handoff_kitti_decode(vppx_ctx *ctx, const uint16_t *png, size_t n, float *disp, u8 *valid)
{
    kitti_decode_kernel<<<dim3((unsigned)((n + 255) / 256)), 256, 0, ctx->stream>>>(png, n, disp, valid);
    VPPX_CHECK_LAUNCH();
    return 0;
}

int handoff_pfm_decode(vppx_ctx *ctx, const u8 *raw, int H, int W, int channels, int little, float *out)
{
    const int rowwords = W * channels;
    pfm_decode_kernel<<<dim3((rowwords + 255) / 256, H), 256, 0, ctx->stream>>>((const u32 *)raw, H, rowwords, little, (u32 *)out);
    VPPX_CHECK_LAUNCH();
    return 0;
}
