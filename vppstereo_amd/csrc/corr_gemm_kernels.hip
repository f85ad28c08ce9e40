// corr_gemm_kernels.hip -- gfx950 kernel for CorrBlock1D's all-pairs correlation (models/raft_stereo/corr.py:151-155), fused
// with the division by sqrt(D), the hint modulation and the pyramid: the two feature maps are read, level 0 and the pooled
// levels are written, and the volume never comes back from memory.
//
// Per (b, y) the work is the GEMM [W3 x D] . [D x W2] on the matrix cores.  fmap3 is the A operand (M = x3) and fmap2 the B
// operand (N = x2): the 16x16 C/D map then puts x2 on the lane (lane & 15) and four consecutive x3 in a lane's registers.
// The rows of two M tiles are interleaved (row r of tile t is x3 = 8 * (r >> 2) + 4 * t + (r & 3) of their 32 columns), so a
// lane's eight accumulator registers of a tile pair are EIGHT consecutive x3 of one output row: 32 contiguous bytes in
// float32, and every cell of levels 1, 2 and 3 is pooled in the lane's own registers exactly as raft_pyramid_kernel does.
// The interleave costs nothing: it is only which LDS column a lane reads its A fragment from.
//
// A workgroup of four waves makes a tile of 128 x3 by 64 x2 of one (b, y): wave (wm, wn) owns 64 x3 by 32 x2, i.e. two tile
// pairs by two N tiles, 32 accumulator registers.  Both operands lie k-major in memory (contiguous along x), so a slab of
// 32 k (float32) or 64 k (bfloat16) is copied to LDS as it lies, [k][x], with 16-byte loads where pointer and row length
// allow and cell by cell otherwise; cells outside the matrices (k >= D, x >= W) are staged as zeros.  The next slab's
// loads are issued into registers before the current slab is multiplied, so their latency lies under the matrix work.
//   float32:  v_mfma_f32_16x16x4_f32 takes A[l & 15][k = l >> 4], one 4-byte LDS read per fragment, no transpose.
//   bfloat16: v_mfma_f32_16x16x32_bf16 takes 8 consecutive k of one x per lane: eight 2-byte LDS reads down a column.
// The accumulators start at +0 and are float32; the order of the sum is the matrix cores'.
#include "corr_shared.h"

#include <math.h>
#include <type_traits>

#define CG_TM 128 // x3 per workgroup
#define CG_TN 64  // x2 per workgroup
#define CG_KS_F32 32  // k per slab
#define CG_KS_BF16 64
// LDS row lengths in cells: whole 16-byte groups, and the four k rows (float32) or the four groups of eight k rows
// (bfloat16) that one fragment read touches start in different banks
#define CG_SA (CG_TM + 16)
#define CG_SB (CG_TN + 16)
#define CG_SAH (CG_TM + 8)
#define CG_SBH (CG_TN + 8)

typedef float cg_f32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 cg_bf16x8 __attribute__((ext_vector_type(8)));

__device__ __forceinline__ uint4 cg_load_cells(const float *p, int valid)
{
    float t[4];
#pragma unroll
    for (int j = 0; j < 4; j++) t[j] = j < valid ? p[j] : 0.0f;
    return make_uint4(__float_as_uint(t[0]), __float_as_uint(t[1]), __float_as_uint(t[2]), __float_as_uint(t[3]));
}

__device__ __forceinline__ uint4 cg_load_cells(const u16 *p, int valid)
{
    u32 t[8];
#pragma unroll
    for (int j = 0; j < 8; j++) t[j] = j < valid ? (u32)p[j] : 0u;
    return make_uint4(t[0] | (t[1] << 16), t[2] | (t[3] << 16), t[4] | (t[5] << 16), t[6] | (t[7] << 16));
}

// KS rows of COLS cells from k0, x0 on, a 16-byte group per thread and trip: cg_fetch loads them into q[], cg_put writes
// q[] to s[KS][STRIDE].  g points at cell (k = 0, x = 0) of the row (b, y) and kstride is the distance between two k.
// vec: g is 16-byte aligned and W is a whole number of 16-byte groups, so a group lies wholly inside the row or wholly
// outside.
template <typename T, int COLS, int KS>
__device__ __forceinline__ void cg_fetch(uint4 (&q)[KS * COLS * (int)sizeof(T) / 16 / 256], const T *g, size_t kstride, int k0, int D,
                                         int x0, int W, bool vec)
{
    constexpr int V = 16 / (int)sizeof(T), GROUPS = COLS / V, TRIPS = KS * GROUPS / 256;
#pragma unroll
    for (int t = 0; t < TRIPS; t++) {
        const int i = threadIdx.x + 256 * t;
        const int k = k0 + i / GROUPS, x = x0 + (i % GROUPS) * V;
        q[t] = make_uint4(0u, 0u, 0u, 0u);
        if (k < D && x < W) {
            const T *p = g + (size_t)k * kstride + x;
            q[t] = vec ? *(const uint4 *)p : cg_load_cells(p, W - x);
        }
    }
}

template <typename T, int COLS, int KS, int STRIDE>
__device__ __forceinline__ void cg_put(T *s, const uint4 (&q)[KS * COLS * (int)sizeof(T) / 16 / 256])
{
    constexpr int V = 16 / (int)sizeof(T), GROUPS = COLS / V, TRIPS = KS * GROUPS / 256;
#pragma unroll
    for (int t = 0; t < TRIPS; t++) {
        const int i = threadIdx.x + 256 * t;
        *(uint4 *)(s + (i / GROUPS) * STRIDE + (i % GROUPS) * V) = q[t];
    }
}

// The lane's eight consecutive cells c[] of level 0 from cell k0 of `row` on, already divided: the modulation, the store
// and the pooled levels, which are raft_pyramid_kernel's own code (corr_pool_levels).
template <bool BF16>
__device__ __forceinline__ void cg_emit(float *c, size_t row, int k0, int W3, int levels, bool mod, float v, float h,
                                        void *__restrict__ corr_, void *__restrict__ pyr_, const CorrLevels &lv)
{
    const int valid = W3 - k0;
    const bool vec0 = lv.vec & 1u;
    if (mod) {
#pragma unroll
        for (int j = 0; j < 8; j++) c[j] = __fmul_rn(c[j], modulation(v, h, (float)(k0 + j), 2.0f));
    }
    if (BF16) {
        u32 b[8];
#pragma unroll
        for (int j = 0; j < 8; j++) b[j] = bf16_rne(c[j]), c[j] = bf16_widen(b[j]);
        store_cells<8>((u16 *)corr_ + row * (size_t)W3 + k0, b, valid, vec0);
    } else {
        float *p = (float *)corr_ + row * (size_t)W3 + k0;
        store_cells<4>(p, c, valid, vec0);
        store_cells<4>(p + 4, c + 4, valid - 4, vec0);
    }
    corr_pool_levels<BF16>(c, row, k0, W3, levels, pyr_, lv);
}

// grid: (x3 chunks * x2 chunks, H4, B).  invec bit 0 / 1: fmap2 / fmap3 may be read with 16-byte loads.
template <bool BF16>
__global__ void __launch_bounds__(256) raft_corr_fused_kernel(const void *__restrict__ f2_, const void *__restrict__ f3_,
                                                              const float *__restrict__ hs, const float *__restrict__ vs, int D,
                                                              int H4, int W2, int W3, float sqrt_d, int levels,
                                                              void *__restrict__ corr_, void *__restrict__ pyr_, CorrLevels lv,
                                                              unsigned invec)
{
    typedef typename std::conditional<BF16, u16, float>::type T;
    constexpr int SA = BF16 ? CG_SAH : CG_SA, SB = BF16 ? CG_SBH : CG_SB, KS = BF16 ? CG_KS_BF16 : CG_KS_F32;
    __shared__ __attribute__((aligned(16))) T sA[KS * SA];
    __shared__ __attribute__((aligned(16))) T sB[KS * SB];

    const int mchunks = (W3 + CG_TM - 1) / CG_TM;
    const int x3c = (blockIdx.x % mchunks) * CG_TM, x2c = (blockIdx.x / mchunks) * CG_TN;
    const int y = blockIdx.y, b = blockIdx.z;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, g = lane >> 4, i = lane & 15;
    const int wm = wave & 1, wn = wave >> 1;
    // a wave whose tile lies wholly outside the matrices stages with the others and computes nothing
    const bool live = x3c + wm * 64 < W3 && x2c + wn * 32 < W2;

    const T *g2 = (const T *)f2_ + ((size_t)b * D * H4 + y) * W2;
    const T *g3 = (const T *)f3_ + ((size_t)b * D * H4 + y) * W3;
    const size_t ks2 = (size_t)H4 * W2, ks3 = (size_t)H4 * W3;

    int colA[4], colB[2]; // the LDS column of this lane's fragment: tile (pair, t) of A, tile n of B
#pragma unroll
    for (int m = 0; m < 4; m++) colA[m] = wm * 64 + 32 * (m >> 1) + 8 * (i >> 2) + 4 * (m & 1) + (i & 3);
#pragma unroll
    for (int n = 0; n < 2; n++) colB[n] = wn * 32 + 16 * n + i;

    cg_f32x4 acc[4][2];
#pragma unroll
    for (int m = 0; m < 4; m++)
#pragma unroll
        for (int n = 0; n < 2; n++) acc[m][n] = (cg_f32x4){0.0f, 0.0f, 0.0f, 0.0f};

    uint4 qa[KS * CG_TM * (int)sizeof(T) / 16 / 256], qb[KS * CG_TN * (int)sizeof(T) / 16 / 256];
    cg_fetch<T, CG_TM, KS>(qa, g3, ks3, 0, D, x3c, W3, invec & 2u);
    cg_fetch<T, CG_TN, KS>(qb, g2, ks2, 0, D, x2c, W2, invec & 1u);
    for (int k0 = 0; k0 < D; k0 += KS) {
        cg_put<T, CG_TM, KS, SA>(sA, qa);
        cg_put<T, CG_TN, KS, SB>(sB, qb);
        __syncthreads();
        if (k0 + KS < D) {
            cg_fetch<T, CG_TM, KS>(qa, g3, ks3, k0 + KS, D, x3c, W3, invec & 2u);
            cg_fetch<T, CG_TN, KS>(qb, g2, ks2, k0 + KS, D, x2c, W2, invec & 1u);
        }
        if (live) {
            if (BF16) {
#pragma unroll 1
                for (int kk = 0; kk < KS && k0 + kk < D; kk += 32) { // rows from D on are zeros: whole steps of them are skipped
                    const u16 *pa = (const u16 *)sA + (kk + 8 * g) * SA, *pb = (const u16 *)sB + (kk + 8 * g) * SB;
                    cg_bf16x8 fa[4], fb[2];
#pragma unroll
                    for (int m = 0; m < 4; m++) {
                        u32 w[4];
#pragma unroll
                        for (int j = 0; j < 4; j++)
                            w[j] = (u32)pa[(2 * j) * SA + colA[m]] | ((u32)pa[(2 * j + 1) * SA + colA[m]] << 16);
                        fa[m] = __builtin_bit_cast(cg_bf16x8, make_uint4(w[0], w[1], w[2], w[3]));
                    }
#pragma unroll
                    for (int n = 0; n < 2; n++) {
                        u32 w[4];
#pragma unroll
                        for (int j = 0; j < 4; j++)
                            w[j] = (u32)pb[(2 * j) * SB + colB[n]] | ((u32)pb[(2 * j + 1) * SB + colB[n]] << 16);
                        fb[n] = __builtin_bit_cast(cg_bf16x8, make_uint4(w[0], w[1], w[2], w[3]));
                    }
#pragma unroll
                    for (int m = 0; m < 4; m++)
#pragma unroll
                        for (int n = 0; n < 2; n++)
                            acc[m][n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[m], fb[n], acc[m][n], 0, 0, 0);
                }
            } else {
                const float *pa = (const float *)sA + g * SA, *pb = (const float *)sB + g * SB;
                const int kend = min(KS, D - k0); // rows from D on are zeros: whole steps of them are skipped
                for (int kk = 0; kk < kend; kk += 4) {
                    float fa[4], fb[2];
#pragma unroll
                    for (int m = 0; m < 4; m++) fa[m] = pa[kk * SA + colA[m]];
#pragma unroll
                    for (int n = 0; n < 2; n++) fb[n] = pb[kk * SB + colB[n]];
#pragma unroll
                    for (int m = 0; m < 4; m++)
#pragma unroll
                        for (int n = 0; n < 2; n++) acc[m][n] = __builtin_amdgcn_mfma_f32_16x16x4f32(fa[m], fb[n], acc[m][n], 0, 0, 0);
                }
            }
        }
        __syncthreads();
    }
    if (!live) return;

#pragma unroll
    for (int n = 0; n < 2; n++) {
        const int x2 = x2c + colB[n];
        if (x2 >= W2) continue;
        const size_t row = ((size_t)b * H4 + y) * W2 + x2;
        const float v = hs ? vs[row] : 0.0f;
        const bool mod = v != 0.0f; // raft_modulate_kernel's rule: v == 0 (or -0) is untouched
        const float h = mod ? hs[row] : 0.0f;
#pragma unroll
        for (int pair = 0; pair < 2; pair++) {
            const int k0 = x3c + wm * 64 + 32 * pair + 8 * g;
            if (k0 >= W3) continue;
            float c[8];
#pragma unroll
            for (int j = 0; j < 8; j++) c[j] = __fdiv_rn(acc[2 * pair + (j >> 2)][n][j & 3], sqrt_d);
            cg_emit<BF16>(c, row, k0, W3, levels, mod, v, h, corr_, pyr_, lv);
        }
    }
}

// ---------------------------------------------------------------------------------------
// launcher
// ---------------------------------------------------------------------------------------
int corr_fused(vppx_ctx *ctx, const void *fmap2, const void *fmap3, const float *hints, const float *valid, int B, int D, int H4,
               int W2, int W3, int H, int W, int levels, void *corr, void *pyr, int dtype)
{
    int rc;
    const size_t nrows = (size_t)B * H4 * W2;
    const size_t chunks = (size_t)((W3 + CG_TM - 1) / CG_TM) * (size_t)((W2 + CG_TN - 1) / CG_TN);
    if (chunks > 0x7FFFFFFFull || H4 > 65535 || B > 65535) {
        vppx_set_error("raft corr fused: %zu tiles per row, %d rows and %d frames are more than one launch takes", chunks, H4, B);
        return VPPX_E_UNSUPPORTED;
    }
    float *hs = nullptr, *vs = nullptr;
    if (hints && (rc = handoff_subsample_hints(ctx, hints, valid, B, H, W, H4, W2, &hs, &vs, 1))) return rc;
    const CorrLevels lv = corr_levels(pyr, nrows, W3, levels, dtype, corr);
    const size_t cell = dtype == VPPX_DT_BF16 ? 2 : 4;
    unsigned invec = 0;
    if ((uintptr_t)fmap2 % 16 == 0 && ((size_t)W2 * cell) % 16 == 0) invec |= 1u;
    if ((uintptr_t)fmap3 % 16 == 0 && ((size_t)W3 * cell) % 16 == 0) invec |= 2u;
    const float sqrt_d = sqrtf((float)D); // correctly rounded: __fsqrt_rn((float)D)
    const dim3 grid((unsigned)chunks, (unsigned)H4, (unsigned)B);
    if (dtype == VPPX_DT_BF16)
        raft_corr_fused_kernel<true><<<grid, 256, 0, ctx->stream>>>(fmap2, fmap3, hs, vs, D, H4, W2, W3, sqrt_d, levels, corr, pyr, lv, invec);
    else
        raft_corr_fused_kernel<false><<<grid, 256, 0, ctx->stream>>>(fmap2, fmap3, hs, vs, D, H4, W2, W3, sqrt_d, levels, corr, pyr, lv, invec);
    VPPX_CHECK_LAUNCH();
    return 0;
}
