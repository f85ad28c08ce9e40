// norm_kernels.hip -- gfx950 kernels for what the RAFT-Stereo encoders run between their convolutions
// (models/raft_stereo/extractor.py: ResidualBlock.forward :48-60, BasicEncoder.forward :181-183, MultiBasicEncoder.forward
// :276-278): InstanceNorm2d or a frozen BatchNorm2d, the ReLUs and the residual sum.
//   * norm_stats:  (mean, rstd) of every [H,W] plane, from float64 sums of x and x*x
//   * norm_apply:  out = relu?(norm(x)) or relu(norm?(res) + relu?(norm(x))) in one launch, float32 arithmetic
// Storage is float32 or bfloat16 (widened on load, rounded once on store); include/vppx.h has the arithmetic,
// tests/_norm_ref.py the float64 referee and its bound.  Both are bound by their passes over the tensor: the statistics
// read x once, the apply reads x (and res) once and writes once.
#include "cells.h"

#include <math.h>

#define NS_THREADS 256
#define NS_TRIP 16              // consecutive cells a lane takes per trip: 64 bytes of float32, 32 of bfloat16
#define NS_TARGET_BLOCKS 2048   // workgroups that fill the device (256 compute units, 8 per unit)
#define NS_MIN_PIECE 16384      // a piece is worth a workgroup from 4 trips per lane on
#define NS_MAX_PIECES 64

int norm_stats_pieces(int64_t planes, int64_t cells)
{
    if (planes < 1 || cells < 1) return 1;
    const int64_t by_fill = (NS_TARGET_BLOCKS + planes - 1) / planes;
    const int64_t by_size = (cells + NS_MIN_PIECE - 1) / NS_MIN_PIECE;
    int64_t p = by_fill < by_size ? by_fill : by_size;
    if (p < 1) p = 1;
    if (p > NS_MAX_PIECES) p = NS_MAX_PIECES;
    return (int)p;
}

// cells of a piece: the plane's cells over the pieces, rounded up to whole trips; a function of (cells, pieces) alone
static long long norm_stats_chunk(long long cells, int pieces)
{
    const long long c = (cells + pieces - 1) / pieces;
    return (c + NS_TRIP - 1) / NS_TRIP * NS_TRIP;
}

// (mean, rstd) from the sums of a plane of n cells, in float64 (include/vppx.h)
__device__ __forceinline__ void norm_finish(double s1, double s2, double n, double eps, float *out)
{
    const double mean = s1 / n;
    double var = s2 / n - mean * mean;
    if (var < 0.0) var = 0.0; // a NaN stays
    out[0] = (float)mean;
    out[1] = (float)(1.0 / sqrt(var + eps));
}

// ---------------------------------------------------------------------------------------
// statistics.  Workgroup (plane, piece) adds the cells [piece * chunk, min(+ chunk, hw)) of its plane: lane t takes trips
// t, t + 256, ... of 16 consecutive cells, each added in cell order to the lane's two float64 sums; waves fold by an xor
// butterfly, wave sums are added in wave order.  Which lane adds which cell in which order depends on (hw, pieces) alone, so
// the 16-byte route (VEC) and the cell-by-cell route give the same bits.  With one piece the workgroup writes (mean, rstd)
// itself; otherwise it writes its two sums to part[plane][piece] and norm_stats_finish_kernel adds them in piece order.
// ---------------------------------------------------------------------------------------
template <bool BF16, bool VEC>
__global__ void __launch_bounds__(NS_THREADS) norm_stats_kernel(const void *x, long long sx, int C, long long hw, long long chunk, int pieces,
                                                                double *part, float *stats, double eps)
{
    const unsigned plane = blockIdx.x / (unsigned)pieces, piece = blockIdx.x - plane * (unsigned)pieces;
    const unsigned b = plane / (unsigned)C, c = plane - b * (unsigned)C;
    const size_t base = (size_t)b * (size_t)sx + (size_t)c * (size_t)hw;
    const long long lo = (long long)piece * chunk;
    const long long hi = lo + chunk < hw ? lo + chunk : hw;
    double s1 = 0.0, s2 = 0.0;
    for (long long i0 = lo + (long long)threadIdx.x * NS_TRIP; i0 < hi; i0 += (long long)NS_THREADS * NS_TRIP) {
        float v[NS_TRIP];
        if (i0 + NS_TRIP <= hi) {
            load_cells<BF16, VEC, NS_TRIP>(x, base + (size_t)i0, v);
#pragma unroll
            for (int k = 0; k < NS_TRIP; k++) {
                const double d = (double)v[k];
                s1 += d;
                s2 += d * d;
            }
        } else {
            for (long long k = i0; k < hi; k++) {
                const double d = (double)load_cell<BF16>(x, base + (size_t)k);
                s1 += d;
                s2 += d * d;
            }
        }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        s1 += __shfl_xor(s1, off);
        s2 += __shfl_xor(s2, off);
    }
    __shared__ double s_sum[NS_THREADS / 64][2];
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) s_sum[wave][0] = s1, s_sum[wave][1] = s2;
    __syncthreads();
    if (threadIdx.x != 0) return;
    double a = 0.0, q = 0.0;
    for (int w = 0; w < NS_THREADS / 64; w++) a += s_sum[w][0], q += s_sum[w][1];
    if (pieces == 1) {
        norm_finish(a, q, (double)hw, eps, stats + 2 * (size_t)plane);
    } else {
        part[2 * (size_t)blockIdx.x] = a;
        part[2 * (size_t)blockIdx.x + 1] = q;
    }
}

__global__ void __launch_bounds__(NS_THREADS) norm_stats_finish_kernel(const double *part, int pieces, long long planes, long long hw,
                                                                       double eps, float *stats)
{
    const long long plane = (long long)blockIdx.x * NS_THREADS + threadIdx.x;
    if (plane >= planes) return;
    double a = 0.0, q = 0.0;
    for (int k = 0; k < pieces; k++) {
        a += part[2 * ((size_t)plane * pieces + k)];
        q += part[2 * ((size_t)plane * pieces + k) + 1];
    }
    norm_finish(a, q, (double)hw, eps, stats + 2 * (size_t)plane);
}

// ---------------------------------------------------------------------------------------
// apply.  A workgroup owns NA_TRIPS * 256 groups of V consecutive cells of ONE plane, so the plane's statistics, weight and
// bias are uniform over it.  A lane loads all its cells of x and res, then computes and stores them: out may be x or res.
// ---------------------------------------------------------------------------------------
#define NA_TRIPS 4

struct NormApply {
    const void *x, *res;
    void *out;
    const float *stats, *weight, *bias, *res_stats, *res_weight, *res_bias;
    long long sx, sres, so, sst, srst, hw;
    int C, relu_inner;
    unsigned bpp; // workgroups per plane
};

struct NormPlane {
    float mean, rstd, w, b, mean_r, rstd_r, rw, rb;
    bool has_w, relu_inner, has_res, has_rs, has_rw;
};

__device__ __forceinline__ float norm_cell(const NormPlane &p, float x, float r)
{
    float v = __fmul_rn(__fsub_rn(x, p.mean), p.rstd);
    if (p.has_w) v = __fadd_rn(__fmul_rn(v, p.w), p.b);
    if (p.relu_inner) v = relu_nan(v);
    if (p.has_res) {
        float u = r;
        if (p.has_rs) u = __fmul_rn(__fsub_rn(u, p.mean_r), p.rstd_r);
        if (p.has_rw) u = __fadd_rn(__fmul_rn(u, p.rw), p.rb);
        v = relu_nan(__fadd_rn(u, v));
    }
    return v;
}

template <bool BF16, int V>
__global__ void __launch_bounds__(256) norm_apply_kernel(NormApply a)
{
    const unsigned plane = blockIdx.x / a.bpp, blk = blockIdx.x - plane * a.bpp;
    const unsigned b = plane / (unsigned)a.C, c = plane - b * (unsigned)a.C;
    NormPlane p;
    p.has_w = a.weight != nullptr, p.relu_inner = a.relu_inner != 0, p.has_res = a.res != nullptr;
    p.has_rs = a.res_stats != nullptr, p.has_rw = a.res_weight != nullptr;
    p.mean = a.stats[(size_t)b * a.sst + 2 * c], p.rstd = a.stats[(size_t)b * a.sst + 2 * c + 1];
    p.w = p.has_w ? a.weight[c] : 1.0f, p.b = p.has_w ? a.bias[c] : 0.0f;
    p.mean_r = p.has_rs ? a.res_stats[(size_t)b * a.srst + 2 * c] : 0.0f;
    p.rstd_r = p.has_rs ? a.res_stats[(size_t)b * a.srst + 2 * c + 1] : 1.0f;
    p.rw = p.has_rw ? a.res_weight[c] : 1.0f, p.rb = p.has_rw ? a.res_bias[c] : 0.0f;
    const size_t in_plane = (size_t)c * (size_t)a.hw;
    const size_t bx = (size_t)b * a.sx + in_plane, br = (size_t)b * a.sres + in_plane, bo = (size_t)b * a.so + in_plane;
    const long long first = ((long long)blk * (NA_TRIPS * 256) + threadIdx.x) * V;
    float xv[NA_TRIPS][V], rv[NA_TRIPS][V];
#pragma unroll
    for (int t = 0; t < NA_TRIPS; t++) {
        const long long at = first + (long long)t * 256 * V;
        if (at + V <= a.hw) {
            load_cells<BF16, (V > 1), V>(a.x, bx + (size_t)at, xv[t]);
            if (p.has_res) load_cells<BF16, (V > 1), V>(a.res, br + (size_t)at, rv[t]);
        } else {
#pragma unroll
            for (int j = 0; j < V; j++) {
                if (at + j < a.hw) {
                    xv[t][j] = load_cell<BF16>(a.x, bx + (size_t)(at + j));
                    if (p.has_res) rv[t][j] = load_cell<BF16>(a.res, br + (size_t)(at + j));
                }
            }
        }
    }
#pragma unroll
    for (int t = 0; t < NA_TRIPS; t++) {
        const long long at = first + (long long)t * 256 * V;
        float o[V];
        if (at + V <= a.hw) {
#pragma unroll
            for (int j = 0; j < V; j++) o[j] = norm_cell(p, xv[t][j], p.has_res ? rv[t][j] : 0.0f);
            store_group<BF16, V>(a.out, bo + (size_t)at, o);
        } else {
#pragma unroll
            for (int j = 0; j < V; j++) {
                if (at + j < a.hw) {
                    o[0] = norm_cell(p, xv[t][j], p.has_res ? rv[t][j] : 0.0f);
                    store_group<BF16, 1>(a.out, bo + (size_t)(at + j), o);
                }
            }
        }
    }
}

// ---------------------------------------------------------------------------------------
// launchers (every argument has been checked by vppx_net_api.hip)
// ---------------------------------------------------------------------------------------
int norm_stats(vppx_ctx *ctx, const void *x, int64_t sx, int B, int C, int H, int W, double eps, float *stats, int dtype)
{
    const bool bf16 = dtype == VPPX_DT_BF16;
    const int VF = bf16 ? 8 : 4;
    const long long hw = (long long)H * W, planes = (long long)B * C;
    const int pieces = norm_stats_pieces(planes, hw);
    if (planes * pieces > 0x7FFFFFFFll) {
        vppx_set_error("vppx_raft_norm_stats: %lld planes in %d pieces each are more workgroups than one launch takes", planes, pieces);
        return VPPX_E_UNSUPPORTED;
    }
    const long long chunk = norm_stats_chunk(hw, pieces);
    double *part = nullptr;
    int rc;
    if (pieces > 1 && (rc = ws_get(ctx, WS_NORM_PART, (size_t)planes * pieces * 2, &part))) return rc;
    // every plane and every piece starts on a 16-byte boundary: chunk is a whole number of trips
    const bool vec = aligned16(x) && sx % VF == 0 && hw % VF == 0;
    const unsigned blocks = (unsigned)(planes * pieces);
#define NORM_STATS_LAUNCH(BF, VV) \
    norm_stats_kernel<BF, (VV > 1)><<<dim3(blocks), NS_THREADS, 0, ctx->stream>>>(x, (long long)sx, C, hw, chunk, pieces, part, stats, eps)
    CELLS_LAUNCH(bf16, vec, NORM_STATS_LAUNCH);
#undef NORM_STATS_LAUNCH
    VPPX_CHECK_LAUNCH();
    if (pieces > 1) {
        norm_stats_finish_kernel<<<dim3((unsigned)((planes + NS_THREADS - 1) / NS_THREADS)), NS_THREADS, 0, ctx->stream>>>(part, pieces, planes, hw,
                                                                                                                     eps, stats);
        VPPX_CHECK_LAUNCH();
    }
    return 0;
}

int norm_apply(vppx_ctx *ctx, const void *x, int64_t sx, const float *stats, int64_t sst, const float *weight, const float *bias,
               int relu_inner, const void *res, int64_t sres, const float *res_stats, int64_t srst, const float *res_weight,
               const float *res_bias, void *out, int64_t so, int B, int C, int H, int W, int dtype)
{
    const bool bf16 = dtype == VPPX_DT_BF16;
    const int VF = bf16 ? 8 : 4;
    NormApply a;
    a.x = x, a.res = res, a.out = out;
    a.stats = stats, a.weight = weight, a.bias = bias, a.res_stats = res_stats, a.res_weight = res_weight, a.res_bias = res_bias;
    a.sx = sx, a.sres = res ? sres : 0, a.so = so, a.sst = sst, a.srst = srst, a.hw = (long long)H * W;
    a.C = C, a.relu_inner = relu_inner;
    const bool vec = aligned16(x) && aligned16(out) && (!res || (aligned16(res) && sres % VF == 0)) && sx % VF == 0 && so % VF == 0 &&
                     a.hw % VF == 0;
    const int V = vec ? VF : 1;
    const long long groups = (a.hw + V - 1) / V, per_block = (long long)NA_TRIPS * 256;
    const long long bpp = (groups + per_block - 1) / per_block, nb = bpp * (long long)B * C;
    if (nb > 0x7FFFFFFFll) {
        vppx_set_error("vppx_raft_norm_apply: %lld planes of %lld cells are %lld workgroups, more than one launch takes", (long long)B * C,
                       a.hw, nb);
        return VPPX_E_UNSUPPORTED;
    }
    a.bpp = (unsigned)bpp;
    const dim3 grid((unsigned)nb);
#define NORM_APPLY_LAUNCH(BF, VV) norm_apply_kernel<BF, VV><<<grid, 256, 0, ctx->stream>>>(a)
    CELLS_LAUNCH(bf16, vec, NORM_APPLY_LAUNCH);
#undef NORM_APPLY_LAUNCH
    VPPX_CHECK_LAUNCH();
    return 0;
}
