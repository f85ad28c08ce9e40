// corr_shared.h -- device code that handoff_kernels.hip, corr_kernels.hip, corr_gemm_kernels.hip and motion_kernels.hip
// share: the hint modulation, where the pyramid's levels lie, how a level is pooled and stored, and one tap of the lookup.
#pragma once
#include "cells.h"

// (1 - v) + (v * height) * exp(-(d - h)^2 / two_w2)     (psmnet.py:197, corr.py:178)
__device__ __forceinline__ float modulation(float v, float h, float d, float two_w2)
{
    const float diff = __fsub_rn(d, h);
    const float e = expf(__fdiv_rn(-__fmul_rn(diff, diff), two_w2));
    return __fadd_rn(__fsub_rn(1.0f, v), __fmul_rn(__fmul_rn(v, 10.0f), e));
}

struct CorrLevels {
    long long off[VPPX_CORR_MAX_LEVELS]; // first cell of level i inside pyr (off[0] unused: level 0 is corr)
    unsigned vec;                        // bit i: a lane's group of 8 >> i cells of level i may go as one aligned store
};

// ((+0 + a) + b) / 2: the sum starts at +0 as avg_pool2d's accumulator does, so two -0 cells pool to +0
__device__ __forceinline__ float pool2(float a, float b) { return __fdiv_rn(__fadd_rn(__fadd_rn(0.0f, a), b), 2.0f); }

// N consecutive cells of one level, the first `valid` of them inside the row; `vec`: p is aligned to the N cells
template <int N>
__device__ __forceinline__ void store_cells(float *p, const float *c, int valid, bool vec)
{
    if (N == 4 && vec && valid >= 4) {
        *(float4 *)p = make_float4(c[0], c[1], c[2], c[3]);
    } else if (N == 2 && vec && valid >= 2) {
        *(float2 *)p = make_float2(c[0], c[1]);
    } else {
#pragma unroll
        for (int j = 0; j < N; j++)
            if (j < valid) p[j] = c[j];
    }
}

template <int N>
__device__ __forceinline__ void store_cells(u16 *p, const u32 *c, int valid, bool vec)
{
    if (N == 8 && vec && valid >= 8) {
        *(uint4 *)p = make_uint4(c[0] | (c[1] << 16), c[2] | (c[3] << 16), c[4] | (c[5] << 16), c[6] | (c[7] << 16));
    } else if (N == 4 && vec && valid >= 4) {
        *(uint2 *)p = make_uint2(c[0] | (c[1] << 16), c[2] | (c[3] << 16));
    } else if (N == 2 && vec && valid >= 2) {
        *(u32 *)p = c[0] | (c[1] << 16);
    } else {
#pragma unroll
        for (int j = 0; j < N; j++)
            if (j < valid) p[j] = (u16)c[j];
    }
}

// Levels 1 .. levels-1 of a lane's eight consecutive level-0 cells c[] from cell k0 of `row` on: 4, 2 and 1 cells, each pooled
// in the lane's registers from the level below it and stored.  float32: c[] are the cells.  bfloat16: c[] are level 0 AS
// STORED, widened, and each level is summed and halved in float32, rounded once (bf16_rne) and pooled on from the rounded
// values.  A pooled cell past the end of its level is made from cells that are not the row's and is never stored.
// raft_pyramid_kernel and raft_corr_fused_kernel both pool here, so the two calls agree bit for bit.
template <bool BF16>
__device__ __forceinline__ void corr_pool_levels(const float *c, size_t row, int k0, int W3, int levels, void *__restrict__ pyr_,
                                                 const CorrLevels &lv)
{
    float l1[4], l2[2], l3[1];
#pragma unroll
    for (int j = 0; j < 4; j++) l1[j] = pool2(c[2 * j], c[2 * j + 1]);
    if (levels > 1) {
        const int W = W3 >> 1, k = k0 >> 1;
        if (BF16) {
            u32 b[4];
#pragma unroll
            for (int j = 0; j < 4; j++) b[j] = bf16_rne(l1[j]), l1[j] = bf16_widen(b[j]);
            store_cells<4>((u16 *)pyr_ + lv.off[1] + row * (size_t)W + k, b, W - k, lv.vec & 2u);
        } else {
            store_cells<4>((float *)pyr_ + lv.off[1] + row * (size_t)W + k, l1, W - k, lv.vec & 2u);
        }
    }
#pragma unroll
    for (int j = 0; j < 2; j++) l2[j] = pool2(l1[2 * j], l1[2 * j + 1]);
    if (levels > 2) {
        const int W = W3 >> 2, k = k0 >> 2;
        if (BF16) {
            u32 b[2];
#pragma unroll
            for (int j = 0; j < 2; j++) b[j] = bf16_rne(l2[j]), l2[j] = bf16_widen(b[j]);
            store_cells<2>((u16 *)pyr_ + lv.off[2] + row * (size_t)W + k, b, W - k, lv.vec & 4u);
        } else {
            store_cells<2>((float *)pyr_ + lv.off[2] + row * (size_t)W + k, l2, W - k, lv.vec & 4u);
        }
    }
    l3[0] = pool2(l2[0], l2[1]);
    if (levels > 3) {
        const int W = W3 >> 3, k = k0 >> 3;
        if (BF16) {
            u32 b[1] = {bf16_rne(l3[0])};
            store_cells<1>((u16 *)pyr_ + lv.off[3] + row * (size_t)W + k, b, W - k, false);
        } else {
            store_cells<1>((float *)pyr_ + lv.off[3] + row * (size_t)W + k, l3, W - k, false);
        }
    }
}

// One tap of the lookup (include/vppx.h has the arithmetic): rf / rb point at row n of the level (float32 / bfloat16), wm1 is
// (float)(W - 1) of the level, xc = c / 2^i.  Both cells are loaded per position, since floor(ix) of neighbouring positions
// need not differ by one after the round trip through the normalised coordinate; a cell outside [0, W-1] is +0, compared
// in float so that 1e30 is outside and not an index; a position that is not finite gives +0.
template <bool BF16>
__device__ __forceinline__ float corr_tap(const float *rf, const u16 *rb, float wm1, float xc, int t, int radius)
{
    const float x = __fadd_rn((float)(t - radius), xc);
    const float xg = __fsub_rn(__fdiv_rn(__fmul_rn(2.0f, x), wm1), 1.0f);
    const float ix = __fmul_rn(__fdiv_rn(__fadd_rn(xg, 1.0f), 2.0f), wm1);
    const float fl = floorf(ix), fl1 = __fadd_rn(fl, 1.0f);
    const bool in_a = fl >= 0.0f && fl <= wm1, in_b = fl1 >= 0.0f && fl1 <= wm1; // false for NaN
    float val = 0.0f;
    if ((in_a || in_b) && isfinite(ix)) {
        const float wr = __fsub_rn(ix, fl), wl = __fsub_rn(fl1, ix);
        float a = 0.0f, bb = 0.0f;
        if (in_a) a = BF16 ? bf16_widen(rb[(int)fl]) : rf[(int)fl];
        if (in_b) bb = BF16 ? bf16_widen(rb[(int)fl1]) : rf[(int)fl1];
        val = __fmaf_rn(bb, wr, __fadd_rn(0.0f, __fmul_rn(a, wl)));
    }
    return val;
}

static inline CorrLevels corr_levels(const void *pyr, size_t nrows, int W3, int levels, int dtype, const void *corr)
{
    CorrLevels lv = {};
    int64_t off[VPPX_CORR_MAX_LEVELS];
    corr_pyramid_offsets((int64_t)nrows, W3, levels, off);
    const size_t cell = dtype == VPPX_DT_BF16 ? 2 : 4;
    for (int i = 0; i < levels; i++) {
        lv.off[i] = off[i];
        // level 0 goes as 16-byte vectors (4 float32 cells, 8 bf16 cells); level i >= 1 as the lane's whole group of 8 >> i cells
        const size_t width = i ? (8 >> i) * cell : 16;
        const uintptr_t first = i ? (uintptr_t)pyr + (size_t)off[i] * cell : (uintptr_t)corr;
        if (width > cell && first % width == 0 && ((size_t)(W3 >> i) * cell) % width == 0) lv.vec |= 1u << i;
    }
    return lv;
}
