// metrics_kernels.hip -- gfx950 kernels of losses.guided_metrics (losses.py:13-24, test.py:150-152, :251-252) for a batch:
// per frame, over the pixels with valid > 0,
//   e = fabsf(disp - gt), d2 = (disp - gt) * (disp - gt)            (float32, no FMA contraction: oracle/rsgm_oracle.c does the same)
//   n_valid, n(e > 1), n(e > 2), n(e > 3), n(e > 4)                 (exact integers)
//   sum(e), sum(d2)                                                 (float64 accumulators of the float32 terms)
// and optionally errormap = e * (valid > 0), the seventh entry of the reference's dict.
//
// Deterministic and independent of the batch: no floating-point atomics.  metrics_partial_kernel writes one record per
// (frame, block); the number of blocks per frame and the pixels each thread owns depend on the frame's shape only -- never on
// the batch size, on pointer alignment or on which load path a launch takes.  Inside a block: every thread adds its own pixels
// in index order, waves fold by __shfl_xor (a butterfly: every lane ends with the same sum), wave sums go through LDS and are
// added in wave order.  metrics_finish_kernel (one wave per frame) adds a frame's records in block order and writes its VppxMetrics.
// Memory-bound and small (12 bytes per pixel): 16-byte loads where the planes allow them, the same pixels per thread where not.
#include "vppx_internal.h"

#define MT_THREADS 256
#define MT_PX 4 // consecutive pixels per thread and trip (one 16-byte load per float plane)

struct MtPartial {
    unsigned long long n, b1, b2, b3, b4;
    double se, sq;
    unsigned long long pad;
};
static_assert(sizeof(MtPartial) == METRICS_PARTIAL_BYTES, "partial record size");

int metrics_blocks_per_frame(size_t npx)
{
    // a block's trip covers 1024 pixels; four trips per block, at most METRICS_MAX_BLOCKS blocks per frame
    const size_t per_block = (size_t)MT_THREADS * MT_PX * 4;
    size_t n = (npx + per_block - 1) / per_block;
    if (n < 1) n = 1;
    if (n > METRICS_MAX_BLOCKS) n = METRICS_MAX_BLOCKS;
    return (int)n;
}

template <typename VT> struct MtValid;
template <> struct MtValid<float> {
    static __device__ __forceinline__ void load4(const float *p, float *v)
    {
        const float4 q = *(const float4 *)p;
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    }
    // losses.py:14-15, :24: error[valid == 0] = 0, then error * (valid > 0)
    static __device__ __forceinline__ float emap(float e, float v) { return __fmul_rn(v == 0.f ? 0.f : e, v > 0.f ? 1.f : 0.f); }
};
template <> struct MtValid<u8> {
    static __device__ __forceinline__ void load4(const u8 *p, u8 *v)
    {
        const uchar4 q = *(const uchar4 *)p;
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    }
    static __device__ __forceinline__ float emap(float e, u8 v) { return v ? e : 0.f; }
};

// grid (blocks per frame, B).  VEC: gt_scale == 1 and every frame's planes start 16-byte aligned with a pixel count that is a
// multiple of 4 (so do the chunks: chunk is a multiple of 4).
template <typename VT, bool VEC>
__global__ void __launch_bounds__(MT_THREADS) metrics_partial_kernel(const float *__restrict__ disp, const float *__restrict__ gt,
                                                                     const VT *__restrict__ valid, float *__restrict__ emap,
                                                                     MtPartial *__restrict__ part, int Ho, int Wo, int Hg, int Wg, int s,
                                                                     float fs, unsigned chunk)
{
    const size_t npx = (size_t)Ho * Wo, ngt = (size_t)Hg * Wg;
    const int f = blockIdx.y;
    disp += (size_t)f * npx;
    gt += (size_t)f * ngt;
    valid += (size_t)f * ngt;
    if (emap) emap += (size_t)f * npx;
    const size_t lo = (size_t)blockIdx.x * chunk;
    const size_t hi = lo + chunk < npx ? lo + chunk : npx;
    unsigned n = 0, b1 = 0, b2 = 0, b3 = 0, b4 = 0;
    double se = 0.0, sq = 0.0;
    for (size_t i0 = lo + (size_t)threadIdx.x * MT_PX; i0 < hi; i0 += (size_t)MT_THREADS * MT_PX) {
        const int m = hi - i0 < MT_PX ? (int)(hi - i0) : MT_PX;
        float d[MT_PX], g[MT_PX], em[MT_PX];
        VT v[MT_PX];
        if (VEC && m == MT_PX) {
            const float4 qd = *(const float4 *)(disp + i0), qg = *(const float4 *)(gt + i0);
            d[0] = qd.x; d[1] = qd.y; d[2] = qd.z; d[3] = qd.w;
            g[0] = qg.x; g[1] = qg.y; g[2] = qg.z; g[3] = qg.w;
            MtValid<VT>::load4(valid + i0, v);
        } else {
            size_t y = 0;
            int x = 0;
            if (s != 1) {
                y = i0 / Wo;
                x = (int)(i0 - y * Wo);
            }
#pragma unroll
            for (int k = 0; k < MT_PX; k++) {
                if (k < m) {
                    // test.py:150-152: every s-th row and column of gt / validgt (F.interpolate nearest), gt / s in float32
                    const size_t gi = s == 1 ? i0 + k : (y * s) * Wg + (size_t)x * s;
                    d[k] = disp[i0 + k];
                    g[k] = s == 1 ? gt[gi] : __fdiv_rn(gt[gi], fs);
                    v[k] = valid[gi];
                    if (s != 1 && ++x == Wo) {
                        x = 0;
                        y++;
                    }
                }
            }
        }
#pragma unroll
        for (int k = 0; k < MT_PX; k++) {
            if (k < m) {
                const float diff = __fsub_rn(d[k], g[k]);
                const float e = fabsf(diff);
                em[k] = MtValid<VT>::emap(e, v[k]);
                if (v[k] > 0) {
                    n++;
                    b1 += e > 1.f;
                    b2 += e > 2.f;
                    b3 += e > 3.f;
                    b4 += e > 4.f;
                    se += (double)e;
                    sq += (double)__fmul_rn(diff, diff);
                }
            }
        }
        if (emap) {
            if (VEC && m == MT_PX) *(float4 *)(emap + i0) = make_float4(em[0], em[1], em[2], em[3]);
            else
                for (int k = 0; k < m; k++) emap[i0 + k] = em[k];
        }
    }
    // wave fold: xor butterfly in a fixed order of distances
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        n += __shfl_xor(n, off);
        b1 += __shfl_xor(b1, off);
        b2 += __shfl_xor(b2, off);
        b3 += __shfl_xor(b3, off);
        b4 += __shfl_xor(b4, off);
        se += __shfl_xor(se, off);
        sq += __shfl_xor(sq, off);
    }
    __shared__ unsigned s_cnt[MT_THREADS / 64][5];
    __shared__ double s_sum[MT_THREADS / 64][2];
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        s_cnt[wave][0] = n; s_cnt[wave][1] = b1; s_cnt[wave][2] = b2; s_cnt[wave][3] = b3; s_cnt[wave][4] = b4;
        s_sum[wave][0] = se; s_sum[wave][1] = sq;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        MtPartial r;
        unsigned long long c[5] = {0, 0, 0, 0, 0};
        double a = 0.0, b = 0.0;
        for (int w = 0; w < MT_THREADS / 64; w++) { // wave order
            for (int k = 0; k < 5; k++) c[k] += s_cnt[w][k];
            a += s_sum[w][0];
            b += s_sum[w][1];
        }
        r.n = c[0]; r.b1 = c[1]; r.b2 = c[2]; r.b3 = c[3]; r.b4 = c[4];
        r.se = a; r.sq = b;
        r.pad = 0;
        part[(size_t)f * gridDim.x + blockIdx.x] = r;
    }
}

// One wave per frame: the lanes fetch the frame's records side by side, lane 0 adds them in block order, then losses.py:17-23
// in float64.
__global__ void __launch_bounds__(64) metrics_finish_kernel(const MtPartial *__restrict__ part, int nblk, VppxMetrics *__restrict__ out)
{
    __shared__ MtPartial s_rec[METRICS_MAX_BLOCKS];
    const int f = blockIdx.x;
    for (int k = threadIdx.x; k < nblk; k += 64) s_rec[k] = part[(size_t)f * nblk + k];
    __syncthreads();
    if (threadIdx.x != 0) return;
    unsigned long long n = 0, b1 = 0, b2 = 0, b3 = 0, b4 = 0;
    double se = 0.0, sq = 0.0;
    for (int k = 0; k < nblk; k++) {
        const MtPartial &r = s_rec[k];
        n += r.n; b1 += r.b1; b2 += r.b2; b3 += r.b3; b4 += r.b4;
        se += r.se;
        sq += r.sq;
    }
    VppxMetrics m;
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    const double dn = (double)n;
    m.bad1 = n ? (double)b1 / dn : nan;
    m.bad2 = n ? (double)b2 / dn : nan;
    m.bad3 = n ? (double)b3 / dn : nan;
    m.bad4 = n ? (double)b4 / dn : nan;
    m.avgerr = n ? se / dn : nan;
    m.rms = n ? sqrt(sq / dn) : nan;
    m.n_valid = dn;
    m.reserved = 0.0;
    out[f] = m;
}

template <typename VT>
static int launch_t(vppx_ctx *ctx, int B, int Ho, int Wo, const float *disp, int Hg, int Wg, int s, const float *gt, const VT *valid,
                    void *partials, VppxMetrics *out, float *errormap)
{
    const size_t npx = (size_t)Ho * Wo;
    const int nblk = metrics_blocks_per_frame(npx);
    // pixels per block: a multiple of 4, the same for every launch on this shape
    size_t chunk = (npx + nblk - 1) / nblk;
    chunk = (chunk + MT_PX - 1) / MT_PX * MT_PX;
    const bool vec = s == 1 && npx % 4 == 0 && ((uintptr_t)disp & 15) == 0 && ((uintptr_t)gt & 15) == 0 &&
                     ((uintptr_t)valid & (4 * sizeof(VT) - 1)) == 0 && (!errormap || ((uintptr_t)errormap & 15) == 0);
    const dim3 grid((unsigned)nblk, (unsigned)B);
    if (vec)
        metrics_partial_kernel<VT, true><<<grid, MT_THREADS, 0, ctx->stream>>>(disp, gt, valid, errormap, (MtPartial *)partials, Ho, Wo, Hg, Wg,
                                                                                 s, (float)s, (unsigned)chunk);
    else
        metrics_partial_kernel<VT, false><<<grid, MT_THREADS, 0, ctx->stream>>>(disp, gt, valid, errormap, (MtPartial *)partials, Ho, Wo, Hg, Wg,
                                                                                  s, (float)s, (unsigned)chunk);
    VPPX_CHECK_LAUNCH();
    metrics_finish_kernel<<<B, 64, 0, ctx->stream>>>((const MtPartial *)partials, nblk, out);
    VPPX_CHECK_LAUNCH();
    return 0;
}

int metrics_launch(vppx_ctx *ctx, int B, int Ho, int Wo, const float *disp, int Hg, int Wg, int gt_scale, const float *gt,
                   const void *valid, int valid_is_u8, void *partials, VppxMetrics *out, float *errormap)
{
    if (valid_is_u8) return launch_t<u8>(ctx, B, Ho, Wo, disp, Hg, Wg, gt_scale, gt, (const u8 *)valid, partials, out, errormap);
    return launch_t<float>(ctx, B, Ho, Wo, disp, Hg, Wg, gt_scale, gt, (const float *)valid, partials, out, errormap);
}
