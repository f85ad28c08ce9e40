// scale_kernels.hip -- gfx950 kernels of --iscale / --oscale around the rSGM hot path (test.py:136-148, :247-248):
//   * scale_front_kernel: cv2.resize(INTER_LINEAR) of the u8 pair to (H // s, W // s) and the nearest decimation of the
//     hints (divided by s) and of validhints, the whole batch in one launch (rule 1; INTEGRATION row 17)
//   * scale_restore_kernel: F.interpolate(d, scale_factor=iscale/oscale, mode='nearest') * iscale / oscale
// Both are gathers through index / weight tables the host computed with the reference's own double / float expressions
// (vppx_api.hip, scale_tables): the kernels only do integer arithmetic and correctly rounded float multiplies / divides.
// Memory-bound: every thread owns 16 output bytes of the pair (one 16-byte store per image) or 4 output floats.
#include "vppx_internal.h"

// Image part: flat byte index i of the output plane [B, h, w, C] -> 16 consecutive bytes per thread.  Hint part: flat
// index of [B, h, w] -> 4 consecutive floats per thread.  Both output planes start 256-byte aligned (workspace arena).
template <int C>
__global__ void __launch_bounds__(256) scale_front_kernel(ScaleFrontArgs a)
{
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    const size_t plane = (size_t)a.h * a.w;
    if (t < a.n_img_threads) {
        const size_t total = (size_t)a.B * plane * C;
        const size_t i0 = (size_t)t * 16;
        // decode the first byte, then walk (channel, column, row) with carries
        size_t pix = i0 / C;
        int c = (int)(i0 - pix * C);
        size_t row = pix / a.w; // b * h + y
        int x = (int)(pix - row * a.w);
        union { uint4 v; u8 b[16]; } ol, orr;
        const int n = total - i0 < 16 ? (int)(total - i0) : 16;
        int4 xt = a.xtab[x];
        size_t b = row / a.h;
        int y = (int)(row - b * a.h);
        int4 yt = a.ytab[y];
        const u8 *fl = a.l + b * (size_t)a.H * a.W * C, *fr = a.r + b * (size_t)a.H * a.W * C;
#pragma unroll
        for (int k = 0; k < 16; k++) {
            if (k < n) {
                const size_t r0 = (size_t)yt.x * a.W * C, r1 = (size_t)yt.y * a.W * C;
                const int c0 = xt.x * C + c, c1 = xt.y * C + c;
                const int tl0 = (int)fl[r0 + c0] * xt.z + (int)fl[r0 + c1] * xt.w;
                const int tl1 = (int)fl[r1 + c0] * xt.z + (int)fl[r1 + c1] * xt.w;
                const int tr0 = (int)fr[r0 + c0] * xt.z + (int)fr[r0 + c1] * xt.w;
                const int tr1 = (int)fr[r1 + c0] * xt.z + (int)fr[r1 + c1] * xt.w;
                ol.b[k] = (u8)((((yt.z * (tl0 >> 4)) >> 16) + ((yt.w * (tl1 >> 4)) >> 16) + 2) >> 2);
                orr.b[k] = (u8)((((yt.z * (tr0 >> 4)) >> 16) + ((yt.w * (tr1 >> 4)) >> 16) + 2) >> 2);
                if (++c == C) {
                    c = 0;
                    if (++x == a.w) {
                        x = 0;
                        if (++y == a.h) {
                            y = 0;
                            b++;
                            fl += (size_t)a.H * a.W * C;
                            fr += (size_t)a.H * a.W * C;
                        }
                        yt = a.ytab[y];
                    }
                    xt = a.xtab[x];
                }
            }
        }
        if (n == 16) {
            *(uint4 *)(a.ls + i0) = ol.v;
            *(uint4 *)(a.rs + i0) = orr.v;
        } else {
            for (int k = 0; k < n; k++) {
                a.ls[i0 + k] = ol.b[k];
                a.rs[i0 + k] = orr.b[k];
            }
        }
        return;
    }
    const long long th = t - a.n_img_threads;
    const size_t total = (size_t)a.B * plane;
    const size_t i0 = (size_t)th * 4;
    if (i0 >= total) return;
    const int n = total - i0 < 4 ? (int)(total - i0) : 4;
    size_t row = i0 / a.w;
    int x = (int)(i0 - row * a.w);
    size_t b = row / a.h;
    int y = (int)(row - b * a.h);
    float og[4], ov[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        if (k < n) {
            const size_t si = (b * a.H + (size_t)y * a.s) * a.W + (size_t)x * a.s;
            og[k] = __fdiv_rn(a.g[si], a.fs); // true division, as the reference's `/ args.iscale`
            if (a.vh) ov[k] = a.vh[si];
            if (++x == a.w) {
                x = 0;
                if (++y == a.h) {
                    y = 0;
                    b++;
                }
            }
        }
    }
    if (n == 4) {
        *(float4 *)(a.gs + i0) = make_float4(og[0], og[1], og[2], og[3]);
        if (a.vh) *(float4 *)(a.vhs + i0) = make_float4(ov[0], ov[1], ov[2], ov[3]);
    } else {
        for (int k = 0; k < n; k++) {
            a.gs[i0 + k] = og[k];
            if (a.vh) a.vhs[i0 + k] = ov[k];
        }
    }
}

int scale_launch_front(vppx_ctx *ctx, const ScaleFrontArgs &a0)
{
    ScaleFrontArgs a = a0;
    const size_t img_bytes = (size_t)a.B * a.h * a.w * a.C;
    const size_t px = (size_t)a.B * a.h * a.w;
    a.n_img_threads = (long long)((img_bytes + 15) / 16);
    const long long n_hint_threads = (long long)((px + 3) / 4);
    const long long threads = a.n_img_threads + n_hint_threads;
    const unsigned blocks = (unsigned)((threads + 255) / 256);
    if (a.C == 3) scale_front_kernel<3><<<blocks, 256, 0, ctx->stream>>>(a);
    else scale_front_kernel<1><<<blocks, 256, 0, ctx->stream>>>(a);
    VPPX_CHECK_LAUNCH();
    return 0;
}

// out[b, Y, X] = (src[b, ry[Y], rx[X]] * (float)iscale) / (float)oscale, 4 consecutive outputs per thread (one 16-byte
// store when the caller's map is 16-byte aligned)
__global__ void __launch_bounds__(256) scale_restore_kernel(const float *__restrict__ src, float *__restrict__ out, const int *__restrict__ ry,
                                                            const int *__restrict__ rx, int B, int h, int w, int Ho, int Wo, float fi,
                                                            float fo, int aligned)
{
    const size_t total = (size_t)B * Ho * Wo;
    const size_t i0 = ((size_t)blockIdx.x * 256 + threadIdx.x) * 4;
    if (i0 >= total) return;
    const int n = total - i0 < 4 ? (int)(total - i0) : 4;
    size_t row = i0 / Wo;
    int X = (int)(i0 - row * Wo);
    size_t b = row / Ho;
    int Y = (int)(row - b * Ho);
    float o[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        if (k < n) {
            const float v = src[(b * h + ry[Y]) * w + rx[X]];
            o[k] = __fdiv_rn(__fmul_rn(v, fi), fo);
            if (++X == Wo) {
                X = 0;
                if (++Y == Ho) {
                    Y = 0;
                    b++;
                }
            }
        }
    }
    if (n == 4 && aligned) {
        *(float4 *)(out + i0) = make_float4(o[0], o[1], o[2], o[3]);
    } else {
        for (int k = 0; k < n; k++) out[i0 + k] = o[k];
    }
}

int scale_launch_restore(vppx_ctx *ctx, int B, int h, int w, int Ho, int Wo, const float *src, float *out, const int *ry,
                         const int *rx, int iscale, int oscale)
{
    const size_t total = (size_t)B * Ho * Wo;
    const unsigned blocks = (unsigned)((total + 1023) / 1024);
    const int aligned = ((uintptr_t)out & 15) == 0;
    scale_restore_kernel<<<blocks, 256, 0, ctx->stream>>>(src, out, ry, rx, B, h, w, Ho, Wo, (float)iscale, (float)oscale, aligned);
    VPPX_CHECK_LAUNCH();
    return 0;
}
