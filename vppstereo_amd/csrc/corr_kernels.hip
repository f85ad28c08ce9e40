// corr_kernels.hip -- gfx950 kernels for what CorrBlock1D does with the all-pairs volume (models/raft_stereo/corr.py:116-145):
//   * the pyramid: levels 1.. of avg_pool2d([1,2]) in one pass over level 0, fused with the hint modulation   corr.py:117-124
//   * the lookup:  2r+1 bilinear taps per level around coords / 2^i, all levels in one launch                  corr.py:126-145
// Every arithmetic step is one correctly rounded float32 operation in the order include/vppx.h writes down: the results
// are the reference's bit for bit, so nothing here may be reassociated or contracted.
#include "corr_shared.h"

#include <math.h>

// CorrLevels, store_cells, corr_pool_levels and corr_levels are shared with corr_gemm_kernels.hip, corr_tap (one tap of the
// lookup) with motion_kernels.hip: corr_shared.h

// One 64-lane wave per (b, y, x2) row, four rows per workgroup; a lane owns 8 consecutive cells of level 0 per trip of
// 512, which are 4, 2 and 1 cells of levels 1, 2 and 3: every pooled cell is made in the lane's registers from the
// level below it, no level is read back and no lane needs another's.  Level 0 is read once; with hints a row with
// v != 0 is multiplied by raft_modulate_kernel's factor and written back once, and the pooled levels are those of the
// written values.  A row with v == 0 is not written, but it is pooled like any other.
// float32: c[] are the cells.  bfloat16: a level is pooled from the level below AS STORED, i.e. from its bf16 values
// widened, summed and halved in float32 and rounded once (bf16_rne); cells that are not modulated keep their bits.
template <bool BF16>
__global__ void __launch_bounds__(256) raft_pyramid_kernel(void *__restrict__ corr_, const float *__restrict__ hs,
                                                           const float *__restrict__ vs, size_t nrows, int W3, int levels,
                                                           void *__restrict__ pyr_, CorrLevels lv)
{
    const size_t row = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= nrows) return;
    const float v = hs ? vs[row] : 0.0f;
    const bool mod = v != 0.0f; // raft_modulate_kernel's rule: v == 0 (or -0) is untouched
    const float h = mod ? hs[row] : 0.0f;
    const bool vec0 = lv.vec & 1u;
    for (int k0 = (threadIdx.x & 63) * 8; k0 < W3; k0 += 512) {
        const int valid = W3 - k0; // cells of this group inside the row (may exceed 8)
        float c[8];
        if (BF16) {
            u16 *p = (u16 *)corr_ + row * (size_t)W3 + k0;
            u32 b[8];
            if (vec0) { // W3 % 8 == 0: the group is whole
                const uint4 q = *(const uint4 *)p;
                const u32 w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
                for (int j = 0; j < 4; j++) b[2 * j] = w[j] & 0xFFFFu, b[2 * j + 1] = w[j] >> 16;
            } else {
#pragma unroll
                for (int j = 0; j < 8; j++) b[j] = j < valid ? p[j] : 0u;
            }
            if (mod) {
#pragma unroll
                for (int j = 0; j < 8; j++) b[j] = bf16_scale(b[j], modulation(v, h, (float)(k0 + j), 2.0f));
                store_cells<8>(p, b, valid, vec0);
            }
#pragma unroll
            for (int j = 0; j < 8; j++) c[j] = bf16_widen(b[j]);
        } else {
            float *p = (float *)corr_ + row * (size_t)W3 + k0;
            if (vec0) { // W3 % 4 == 0: each half is whole or absent
                const float4 q0 = *(const float4 *)p;
                const float4 q1 = valid > 4 ? *(const float4 *)(p + 4) : make_float4(0.f, 0.f, 0.f, 0.f);
                c[0] = q0.x, c[1] = q0.y, c[2] = q0.z, c[3] = q0.w, c[4] = q1.x, c[5] = q1.y, c[6] = q1.z, c[7] = q1.w;
            } else {
#pragma unroll
                for (int j = 0; j < 8; j++) c[j] = j < valid ? p[j] : 0.0f;
            }
            if (mod) {
#pragma unroll
                for (int j = 0; j < 8; j++) c[j] = __fmul_rn(c[j], modulation(v, h, (float)(k0 + j), 2.0f));
                store_cells<4>(p, c, valid, vec0);
                store_cells<4>(p + 4, c + 4, valid - 4, vec0);
            }
        }
        corr_pool_levels<BF16>(c, row, k0, W3, levels, pyr_, lv);
    }
}

// One thread per pixel n = (b, y, x), lanes are consecutive pixels of an image row (of the frame's plane, where a row
// ends inside a wave): the levels * (2r+1) stores of a wave are 256 contiguous bytes each.  Per level a thread reads
// 2r+2 consecutive cells of its own row n; both taps are loaded per position, since floor(ix) of neighbouring
// positions need not differ by one after the round trip through the normalised coordinate.
// x  = (t - r) + c / 2^i;  xg = 2x / (W-1) - 1;  ix = ((xg + 1) / 2) * (W-1)          (corr.py:134-140, utils.py:63,
// grid_sample with align_corners = True); the taps outside [0, W-1] are +0, compared in float so that 1e30 is outside
// and not an index; a position that is not finite gives +0.
template <bool BF16>
__global__ void __launch_bounds__(256) raft_lookup_kernel(const void *__restrict__ corr_, const void *__restrict__ pyr_, CorrLevels lv,
                                                          const float *__restrict__ coords_x, long long cstride, size_t plane,
                                                          size_t n_pix, int W3, int levels, int radius, float *__restrict__ out)
{
    const size_t n = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (n >= n_pix) return;
    const size_t b = n / plane, p = n - b * plane;
    const float c = coords_x[(size_t)b * (size_t)cstride + p];
    const int taps = 2 * radius + 1;
    float *o = out + b * (size_t)(levels * taps) * plane + p;
    for (int i = 0; i < levels; i++) {
        const int W = W3 >> i;
        const float wm1 = (float)(W - 1);
        const float xc = __fdiv_rn(c, (float)(1 << i));
        const size_t base = (i ? (size_t)lv.off[i] : 0) + n * (size_t)W;
        const float *rf = (const float *)(i ? pyr_ : corr_) + base;
        const u16 *rb = (const u16 *)(i ? pyr_ : corr_) + base;
        for (int t = 0; t < taps; t++) {
            const float val = corr_tap<BF16>(rf, rb, wm1, xc, t, radius);
            o[(size_t)(i * taps + t) * plane] = val;
        }
    }
}

// ---------------------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------------------
int corr_pyramid(vppx_ctx *ctx, void *corr, const float *hints, const float *valid, int B, int H4, int W2, int W3, int H, int W,
                 int levels, void *pyr, int dtype)
{
    int rc;
    const size_t nrows = (size_t)B * H4 * W2;
    if ((nrows + 3) / 4 > 0x7FFFFFFFull) {
        vppx_set_error("raft corr pyramid: B*H4*W2 = %zu rows are more than one launch takes", nrows);
        return VPPX_E_UNSUPPORTED;
    }
    float *hs = nullptr, *vs = nullptr;
    if (hints && (rc = handoff_subsample_hints(ctx, hints, valid, B, H, W, H4, W2, &hs, &vs, 1))) return rc;
    const CorrLevels lv = corr_levels(pyr, nrows, W3, levels, dtype, corr);
    const dim3 grid((unsigned)((nrows + 3) / 4));
    if (dtype == VPPX_DT_BF16)
        raft_pyramid_kernel<true><<<grid, 256, 0, ctx->stream>>>(corr, hs, vs, nrows, W3, levels, pyr, lv);
    else
        raft_pyramid_kernel<false><<<grid, 256, 0, ctx->stream>>>(corr, hs, vs, nrows, W3, levels, pyr, lv);
    VPPX_CHECK_LAUNCH();
    return 0;
}

int corr_lookup(vppx_ctx *ctx, const void *corr, const void *pyr, const float *coords_x, int64_t coords_frame_stride, int B, int H4,
                int W2, int W3, int levels, int radius, float *out, int dtype)
{
    const size_t plane = (size_t)H4 * W2, n_pix = plane * B;
    if ((n_pix + 255) / 256 > 0x7FFFFFFFull) {
        vppx_set_error("raft corr lookup: B*H4*W2 = %zu pixels are more than one launch takes", n_pix);
        return VPPX_E_UNSUPPORTED;
    }
    const CorrLevels lv = corr_levels(pyr, n_pix, W3, levels, dtype, corr);
    const dim3 grid((unsigned)((n_pix + 255) / 256));
    if (dtype == VPPX_DT_BF16)
        raft_lookup_kernel<true><<<grid, 256, 0, ctx->stream>>>(corr, pyr, lv, coords_x, (long long)coords_frame_stride, plane, n_pix, W3,
                                                                 levels, radius, out);
    else
        raft_lookup_kernel<false><<<grid, 256, 0, ctx->stream>>>(corr, pyr, lv, coords_x, (long long)coords_frame_stride, plane, n_pix, W3,
                                                                  levels, radius, out);
    VPPX_CHECK_LAUNCH();
    return 0;
}
