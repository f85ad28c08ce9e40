// readout_kernels.hip -- gfx950 kernels that take the deep front-ends' output back as a float32 disparity map:
//   * psm_readout:   trilinear upsample of cost3 + softmax over D + disparity regression + crop, one pass
//                    (models/psmnet/psmnet.py:227-233, submodule.py:115-128, test.py:242-245)
//   * raft_upsample: convex upsampling (softmax over 9, 3x3 unfold of f * flow with zero padding, sum, the
//                    permute + reshape copy), channel slice, negation and crop, one launch
//                    (models/raft_stereo/raft_stereo.py:69-81,153-154, test.py:237-245)
// Neither is bit-equal to the torch composition: both are held to the float64 referee of tests/_readout_ref.py, whose
// limit() is what any float32 association of the same arithmetic can reach.  include/vppx.h has the arithmetic.
#include "cells.h"

#include <math.h>

// ATen's source index of align_corners = False linear upsampling to a given output size, all in float32
// (area_pixel_compute_source_index with scale = n_in / n_out): -> i0, the weight l1 of i0 + (i0 < n_in - 1).  The fused
// multiply-add is ATen's: its kernels, vectorised CPU and device alike, are compiled with contraction on, and the CPU
// tests pin these weights against torch bit for bit.
__device__ __forceinline__ void lin_src(float scale, int dst, int n_in, int &i0, int &i1, float &l0, float &l1)
{
    const float src = fmaxf(__fmaf_rn(scale, __fadd_rn((float)dst, 0.5f), -0.5f), 0.0f);
    i0 = min((int)src, n_in - 1); // src < n_in - 0.5 by the formula; the clamp keeps a rounding at the last cell inside
    i1 = i0 + (i0 < n_in - 1 ? 1 : 0);
    l1 = __fsub_rn(src, (float)i0);
    l0 = __fsub_rn(1.0f, l1);
}

struct PsmTap { // one output disparity: the two source planes (as offsets into the lane's column of LDS) and their weights
    int o0, o1;
    float l0, l1;
};

// A workgroup is T/64 waves; a wave is 64 consecutive output pixels of one row of the crop window, so the stores of a
// wave are 256 contiguous bytes.  Three phases:
//   0  the D entries of PsmTap, which every pixel shares, into LDS;
//   1  each lane interpolates the D4 source planes in y and x at its pixel (4 taps per plane: D4 * 4 loads instead of
//      D * 8, neighbouring lanes share cells, four lanes per cell at x4, so a wave reads about 17 cells of two rows per
//      plane) and keeps them in its own column of LDS, plane-major: lane l's plane k is at p[k * T + l], conflict-free;
//   2  the logits z_d = l0 * p[i0] + l1 * p[i1] twice, first for their maximum, then for sum exp(z - max) and
//      sum d * exp(z - max): the same expression both times, so the maximum is the maximum of what is exponentiated.
// A NaN logit is skipped by fmaxf and turns the sums NaN; a +inf logit gives inf - inf; a -inf one exp(-inf) = 0.
template <bool BF16>
__global__ void __launch_bounds__(256) psm_readout_kernel(const void *__restrict__ cost, int D4, int H4, int W4, int D, int H, int W,
                                                          int top, int left, int Hout, int Wout, int xtiles, int ytiles,
                                                          float *__restrict__ out)
{
    extern __shared__ __align__(16) unsigned char lds[];
    PsmTap *tab = (PsmTap *)lds;
    float *p = (float *)(lds + (size_t)D * sizeof(PsmTap));
    const int T = blockDim.x, rows = T >> 6;
    {
        const float sd = __fdiv_rn((float)D4, (float)D);
        for (int d = threadIdx.x; d < D; d += T) {
            PsmTap t;
            lin_src(sd, d, D4, t.o0, t.o1, t.l0, t.l1);
            t.o0 *= T, t.o1 *= T;
            tab[d] = t;
        }
    }
    size_t blk = blockIdx.x;
    const int xt = (int)(blk % xtiles);
    blk /= xtiles;
    const int yt = (int)(blk % ytiles);
    const size_t b = blk / ytiles;
    const int xo = xt * 64 + (threadIdx.x & 63), yo = yt * rows + (threadIdx.x >> 6);
    const bool live = xo < Wout && yo < Hout;
    if (live) {
        int y0, y1, x0, x1;
        float ly0, ly1, lx0, lx1;
        lin_src(__fdiv_rn((float)H4, (float)H), yo + top, H4, y0, y1, ly0, ly1);
        lin_src(__fdiv_rn((float)W4, (float)W), xo + left, W4, x0, x1, lx0, lx1);
        const size_t plane = (size_t)H4 * W4, base = b * (size_t)D4 * plane;
        const size_t a00 = base + (size_t)y0 * W4 + x0, a01 = base + (size_t)y0 * W4 + x1;
        const size_t a10 = base + (size_t)y1 * W4 + x0, a11 = base + (size_t)y1 * W4 + x1;
        float *mine = p + threadIdx.x;
        for (int k = 0; k < D4; k++) {
            const size_t o = (size_t)k * plane;
            const float r0 = __fmaf_rn(lx1, load_cell<BF16>(cost, a01 + o), __fmul_rn(lx0, load_cell<BF16>(cost, a00 + o)));
            const float r1 = __fmaf_rn(lx1, load_cell<BF16>(cost, a11 + o), __fmul_rn(lx0, load_cell<BF16>(cost, a10 + o)));
            mine[(size_t)k * T] = __fmaf_rn(ly1, r1, __fmul_rn(ly0, r0));
        }
    }
    __syncthreads(); // the table; a lane reads its own column only
    if (!live) return;
    const float *mine = p + threadIdx.x;
    float m = -INFINITY;
#pragma unroll 4
    for (int d = 0; d < D; d++) {
        const PsmTap t = tab[d];
        m = fmaxf(m, __fmaf_rn(t.l1, mine[t.o1], __fmul_rn(t.l0, mine[t.o0])));
    }
    float den = 0.0f, num = 0.0f;
#pragma unroll 4
    for (int d = 0; d < D; d++) {
        const PsmTap t = tab[d];
        const float z = __fmaf_rn(t.l1, mine[t.o1], __fmul_rn(t.l0, mine[t.o0]));
        const float e = expf(__fsub_rn(z, m));
        den = __fadd_rn(den, e);
        num = __fmaf_rn((float)d, e, num);
    }
    out[(b * Hout + yo) * (size_t)Wout + xo] = __fdiv_rn(num, den);
}

// One thread per (b, output row Y of the window, source column x): it owns the F output pixels F*x .. F*x + F-1 of
// that row.  Lanes are consecutive x, so every one of the 9 * F mask loads of a wave is 64 consecutive cells of one
// channel's row, and a wave's stores cover 64 * F consecutive floats of the output row: as F-float (at most 4-float)
// vectors when `vec` says that every group is aligned and lies wholly inside or outside the window, else float by float.
// The softmax weights are made once and serve every channel of the flow.
template <int F, bool BF16>
__global__ void __launch_bounds__(256) raft_upsample_kernel(const void *__restrict__ flow, long long fstride, const void *__restrict__ mask,
                                                            int C, int H4, int W4, float sign, int top, int left, int Hout, int Wout,
                                                            int x_lo, int nx, size_t n, bool vec, float *__restrict__ out)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int x = x_lo + (int)(i % nx);
    const size_t by = i / nx;
    const int Yo = (int)(by % Hout);
    const size_t b = by / Hout;
    const int Y = Yo + top, y = Y / F, sub = Y % F;
    const size_t plane = (size_t)H4 * W4, at = (size_t)y * W4 + x;
    const size_t mbase = b * (size_t)(9 * F * F) * plane + (size_t)(sub * F) * plane + at;
    float e[F][9], den[F];
#pragma unroll
    for (int j = 0; j < F; j++) {
        float z[9], m = -INFINITY;
#pragma unroll
        for (int k = 0; k < 9; k++) {
            z[k] = load_cell<BF16>(mask, mbase + (size_t)(k * F * F + j) * plane);
            m = fmaxf(m, z[k]);
        }
        den[j] = 0.0f;
#pragma unroll
        for (int k = 0; k < 9; k++) {
            e[j][k] = expf(__fsub_rn(z[k], m));
            den[j] = __fadd_rn(den[j], e[j][k]);
        }
    }
    const int X0 = F * x - left; // the group's first pixel, in window coordinates
    for (int c = 0; c < C; c++) {
        const size_t fbase = b * (size_t)fstride + (size_t)c * plane;
        float fl[9];
#pragma unroll
        for (int k = 0; k < 9; k++) {
            const int yy = y + k / 3 - 1, xx = x + k % 3 - 1;
            const bool in = yy >= 0 && yy < H4 && xx >= 0 && xx < W4;
            fl[k] = in ? __fmul_rn((float)F, load_cell<BF16>(flow, fbase + (size_t)yy * W4 + xx)) : 0.0f;
        }
        float r[F];
#pragma unroll
        for (int j = 0; j < F; j++) {
            float acc = 0.0f;
#pragma unroll
            for (int k = 0; k < 9; k++) acc = __fmaf_rn(__fdiv_rn(e[j][k], den[j]), fl[k], acc);
            r[j] = __fmul_rn(sign, acc);
        }
        float *orow = out + ((b * C + c) * (size_t)Hout + Yo) * (size_t)Wout;
        if (vec && F == 2) {
            if (X0 >= 0 && X0 < Wout) *(float2 *)(orow + X0) = make_float2(r[0], r[1]);
        } else if (vec && F >= 4) {
#pragma unroll
            for (int j = 0; j + 3 < F; j += 4) // a group of 8 may have one half in the window
                if (X0 + j >= 0 && X0 + j < Wout) *(float4 *)(orow + X0 + j) = make_float4(r[j], r[j + 1], r[j + 2], r[j + 3]);
        } else {
#pragma unroll
            for (int j = 0; j < F; j++)
                if (X0 + j >= 0 && X0 + j < Wout) orow[X0 + j] = r[j];
        }
    }
}

// ---------------------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------------------
#define READOUT_LDS_BYTES 65536 // what a launch may ask for without raising the function's limit

int readout_psm(vppx_ctx *ctx, const void *cost, int B, int D4, int H4, int W4, int D, int H, int W, int top, int left, int Hout,
                int Wout, float *out, int dtype)
{
    // the lane's column of planes: 256, 128 or 64 lanes per workgroup, whichever is the most that fits
    int T = 256;
    const size_t tab = (size_t)D * sizeof(PsmTap);
    while (T >= 64 && tab + (size_t)D4 * T * sizeof(float) > READOUT_LDS_BYTES) T >>= 1;
    if (T < 64) {
        vppx_set_error("psmnet readout: %d planes and %d disparities need %zu bytes of LDS per wave, %d is the limit", D4, D,
                       tab + (size_t)D4 * 64 * sizeof(float), READOUT_LDS_BYTES);
        return VPPX_E_UNSUPPORTED;
    }
    const int rows = T / 64;
    const size_t xtiles = ((size_t)Wout + 63) / 64, ytiles = ((size_t)Hout + rows - 1) / rows;
    const size_t blocks = (size_t)B * ytiles * xtiles;
    if (blocks > 0x7FFFFFFFull) {
        vppx_set_error("psmnet readout: %d frames of %dx%d pixels are %zu workgroups, more than one launch takes", B, Hout, Wout, blocks);
        return VPPX_E_UNSUPPORTED;
    }
    const size_t lds = tab + (size_t)D4 * T * sizeof(float);
    if (dtype == VPPX_DT_BF16)
        psm_readout_kernel<true><<<dim3((unsigned)blocks), T, lds, ctx->stream>>>(cost, D4, H4, W4, D, H, W, top, left, Hout, Wout,
                                                                                  (int)xtiles, (int)ytiles, out);
    else
        psm_readout_kernel<false><<<dim3((unsigned)blocks), T, lds, ctx->stream>>>(cost, D4, H4, W4, D, H, W, top, left, Hout, Wout,
                                                                                   (int)xtiles, (int)ytiles, out);
    VPPX_CHECK_LAUNCH();
    return 0;
}

template <int F>
static void raft_upsample_launch(vppx_ctx *ctx, unsigned blocks, bool bf16, const void *flow, long long fstride, const void *mask, int C,
                                 int H4, int W4, float sign, int top, int left, int Hout, int Wout, int x_lo, int nx, size_t n, bool vec,
                                 float *out)
{
    if (bf16)
        raft_upsample_kernel<F, true><<<dim3(blocks), 256, 0, ctx->stream>>>(flow, fstride, mask, C, H4, W4, sign, top, left, Hout, Wout,
                                                                             x_lo, nx, n, vec, out);
    else
        raft_upsample_kernel<F, false><<<dim3(blocks), 256, 0, ctx->stream>>>(flow, fstride, mask, C, H4, W4, sign, top, left, Hout, Wout,
                                                                              x_lo, nx, n, vec, out);
}

int readout_raft_upsample(vppx_ctx *ctx, const void *flow, int64_t flow_frame_stride, const void *mask, int B, int C, int H4, int W4, int f,
                          int sign, int top, int left, int Hout, int Wout, float *out, int dtype)
{
    // the source columns whose F pixels touch the window
    const int x_lo = left / f, x_hi = (left + Wout - 1) / f, nx = x_hi - x_lo + 1;
    const size_t n = (size_t)B * Hout * nx;
    if ((n + 255) / 256 > 0x7FFFFFFFull) {
        vppx_set_error("raft upsample: %d frames of %dx%d pixels are %zu threads, more than one launch takes", B, Hout, Wout, n);
        return VPPX_E_UNSUPPORTED;
    }
    // a group of V = min(f, 4) floats as one store: out aligned to it, and every group whole or absent in the window
    const int V = f < 4 ? f : 4;
    const bool vec = V > 1 && (uintptr_t)out % (V * sizeof(float)) == 0 && Wout % V == 0 && left % V == 0;
    const unsigned blocks = (unsigned)((n + 255) / 256);
    const bool bf16 = dtype == VPPX_DT_BF16;
    const float s = sign < 0 ? -1.0f : 1.0f;
    const long long fs = (long long)flow_frame_stride;
    switch (f) {
    case 1: raft_upsample_launch<1>(ctx, blocks, bf16, flow, fs, mask, C, H4, W4, s, top, left, Hout, Wout, x_lo, nx, n, vec, out); break;
    case 2: raft_upsample_launch<2>(ctx, blocks, bf16, flow, fs, mask, C, H4, W4, s, top, left, Hout, Wout, x_lo, nx, n, vec, out); break;
    case 4: raft_upsample_launch<4>(ctx, blocks, bf16, flow, fs, mask, C, H4, W4, s, top, left, Hout, Wout, x_lo, nx, n, vec, out); break;
    default: raft_upsample_launch<8>(ctx, blocks, bf16, flow, fs, mask, C, H4, W4, s, top, left, Hout, Wout, x_lo, nx, n, vec, out); break;
    }
    VPPX_CHECK_LAUNCH();
    return 0;
}
