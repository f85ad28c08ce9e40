// gru_kernels.hip -- gfx950 kernels for what BasicMultiUpdateBlock.forward runs between its convolutions
// (models/raft_stereo/update.py:119-142, ConvGRU.forward :23-32):
//   * gru_assemble: hx = cat(sources, dim=1) in one launch, a source being copied, pooled (pool2x, :89-90) or
//                   interpolated (interp, :95-97) on its way
//   * gru_reset:    r = sigmoid(ar + cr), r * h over the first C channels of hx, in place
//   * gru_update:   z = sigmoid(az + cz), q = tanh(aq + cq), h' = (1 - z) * h + z * q
// Storage is float32 or bfloat16 (widened on load, rounded once on store), the arithmetic float32; include/vppx.h has it,
// tests/_gru_ref.py the float64 referee with the bound any float32 evaluation of it keeps.
// Every tensor is [B,C,H,W] with a frame stride of its own: a lane owns V consecutive cells of one frame (16 bytes: 4 float32,
// 8 bfloat16) and moves them as one vector where the launcher found every base 16-byte aligned and every frame stride a
// multiple of V; otherwise the same kernels run with V = 1.
#include "cells.h"
#include "gru_math.h"

#include <math.h>
#include <string.h>

// ---------------------------------------------------------------------------------------
// the gates.  n = C*H*W cells per frame, G = ceil(n / V) groups per frame, one lane per (frame, group); a last group that
// is not whole goes cell by cell.
// ---------------------------------------------------------------------------------------
template <bool BF16, int V>
__global__ void __launch_bounds__(256) gru_reset_kernel(const void *ar, long long sar, const void *cr, long long scr, const void *h,
                                                        long long sh, void *hx, long long shx, long long n, long long G, size_t total)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const size_t b = i / (size_t)G;
    const long long at = (long long)(i - b * (size_t)G) * V;
    float a[V], c[V], hh[V], o[V];
    if (at + V <= n) {
        load_cells<BF16, (V > 1), V>(ar, b * sar + at, a);
        load_cells<BF16, (V > 1), V>(cr, b * scr + at, c);
        load_cells<BF16, (V > 1), V>(h, b * sh + at, hh);
#pragma unroll
        for (int j = 0; j < V; j++) o[j] = __fmul_rn(gru_sigmoid(__fadd_rn(a[j], c[j])), hh[j]);
        store_group<BF16, V>(hx, b * shx + at, o);
    } else {
        for (long long k = at; k < n; k++) {
            const float r = gru_sigmoid(__fadd_rn(load_cell<BF16>(ar, b * sar + k), load_cell<BF16>(cr, b * scr + k)));
            store_cell<BF16>(hx, b * shx + k, __fmul_rn(r, load_cell<BF16>(h, b * sh + k)));
        }
    }
}

__device__ __forceinline__ float gru_blend(float az, float cz, float aq, float cq, float h)
{
    const float z = gru_sigmoid(__fadd_rn(az, cz));
    const float q = gru_tanh(__fadd_rn(aq, cq));
    return gru_mix(z, q, h);
}

// out may be h: a lane reads its cells of h before it writes the same cells of out, and no other lane touches them
template <bool BF16, int V>
__global__ void __launch_bounds__(256) gru_update_kernel(const void *az, long long saz, const void *cz, long long scz, const void *aq,
                                                         long long saq, const void *cq, long long scq, const void *h, long long sh,
                                                         void *out, long long so, long long n, long long G, size_t total)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const size_t b = i / (size_t)G;
    const long long at = (long long)(i - b * (size_t)G) * V;
    float vaz[V], vcz[V], vaq[V], vcq[V], hh[V], o[V];
    if (at + V <= n) {
        load_cells<BF16, (V > 1), V>(az, b * saz + at, vaz);
        load_cells<BF16, (V > 1), V>(cz, b * scz + at, vcz);
        load_cells<BF16, (V > 1), V>(aq, b * saq + at, vaq);
        load_cells<BF16, (V > 1), V>(cq, b * scq + at, vcq);
        load_cells<BF16, (V > 1), V>(h, b * sh + at, hh);
#pragma unroll
        for (int j = 0; j < V; j++) o[j] = gru_blend(vaz[j], vcz[j], vaq[j], vcq[j], hh[j]);
        store_group<BF16, V>(out, b * so + at, o);
    } else {
        for (long long k = at; k < n; k++)
            store_cell<BF16>(out, b * so + k,
                             gru_blend(load_cell<BF16>(az, b * saz + k), load_cell<BF16>(cz, b * scz + k), load_cell<BF16>(aq, b * saq + k),
                                       load_cell<BF16>(cq, b * scq + k), load_cell<BF16>(h, b * sh + k)));
    }
}

// ---------------------------------------------------------------------------------------
// the assembly of hx
// ---------------------------------------------------------------------------------------
struct GruSrc {
    const void *p;
    long long stride;  // cells between frames
    long long first;   // the source's first cell inside a frame of hx
    int Hs, Ws, mode;
    float sy, sx;      // interp: (n_in - 1) / (n_out - 1), or 0 for one output cell
    int vec;           // copy: p is 16-byte aligned, stride and first are multiples of V
};
struct GruAsm {
    GruSrc s[VPPX_GRU_MAX_SOURCES];
    int n;
};

// ATen's align_corners = True source index, in float32: -> i0, i1 = i0 + (i0 < n_in - 1), the weights l0 = 1 - l1 and l1
__device__ __forceinline__ void lin_src_ac(float scale, int dst, int n_in, int &i0, int &i1, float &l0, float &l1)
{
    const float src = __fmul_rn(scale, (float)dst);
    i0 = min((int)src, n_in - 1); // src <= n_in - 1 up to its rounding; the clamp keeps the last cell inside
    i1 = i0 + (i0 < n_in - 1 ? 1 : 0);
    l1 = __fsub_rn(src, (float)i0);
    l0 = __fsub_rn(1.0f, l1);
}

// cell (c, y, x) of the source's part of hx; MODE is the source's mode where the caller has branched on it, -1 otherwise
template <bool BF16, int MODE = -1>
__device__ __forceinline__ float gru_source_cell(const GruSrc &s, size_t b, long long c, int y, int x)
{
    const size_t base = b * (size_t)s.stride + (size_t)c * s.Hs * s.Ws;
    const int mode = MODE < 0 ? s.mode : MODE;
    if (mode == VPPX_GRU_COPY) return load_cell<BF16>(s.p, base + (size_t)y * s.Ws + x);
    if (mode == VPPX_GRU_POOL2X) {
        // avg_pool2d(3, stride 2, padding 1, count_include_pad): rows 2y-1 .. 2y+1, +0 outside the map, / 9 always
        float acc = 0.0f;
#pragma unroll
        for (int ky = 0; ky < 3; ky++) {
            const int yy = 2 * y - 1 + ky;
#pragma unroll
            for (int kx = 0; kx < 3; kx++) {
                const int xx = 2 * x - 1 + kx;
                const bool in = yy >= 0 && yy < s.Hs && xx >= 0 && xx < s.Ws;
                acc = __fadd_rn(acc, in ? load_cell<BF16>(s.p, base + (size_t)yy * s.Ws + xx) : 0.0f);
            }
        }
        return __fdiv_rn(acc, 9.0f);
    }
    int y0, y1, x0, x1;
    float ly0, ly1, lx0, lx1;
    lin_src_ac(s.sy, y, s.Hs, y0, y1, ly0, ly1);
    lin_src_ac(s.sx, x, s.Ws, x0, x1, lx0, lx1);
    const float a = load_cell<BF16>(s.p, base + (size_t)y0 * s.Ws + x0), bb = load_cell<BF16>(s.p, base + (size_t)y0 * s.Ws + x1);
    const float cc = load_cell<BF16>(s.p, base + (size_t)y1 * s.Ws + x0), d = load_cell<BF16>(s.p, base + (size_t)y1 * s.Ws + x1);
    const float r0 = __fadd_rn(__fmul_rn(lx0, a), __fmul_rn(lx1, bb));
    const float r1 = __fadd_rn(__fmul_rn(lx0, cc), __fmul_rn(lx1, d));
    return __fadd_rn(__fmul_rn(ly0, r0), __fmul_rn(ly1, r1));
}

// V cells of one source from (ch, y, x) on, unrolled, so that the loads of all of them are in flight together
template <bool BF16, int V, int MODE>
__device__ __forceinline__ void gru_source_cells(const GruSrc &s, size_t b, long long ch, int y, int x, int H, int W, float *c)
{
#pragma unroll
    for (int j = 0; j < V; j++) {
        c[j] = gru_source_cell<BF16, MODE>(s, b, ch, y, x);
        if (++x == W) {
            x = 0;
            if (++y == H) y = 0, ch++;
        }
    }
}

// n cells per frame of hx are written (the sources' channels), G = ceil(n / V) groups; shx cells between frames of hx.
// A group that lies inside one copied source whose cells are aligned with hx's moves as one vector; a group inside one
// source of any other kind is made by that kind's unrolled loop; a group that straddles two sources, or the last one of a
// frame when it is not whole, goes cell by cell.  A whole group leaves as one store.
template <bool BF16, int V>
__global__ void __launch_bounds__(256) gru_assemble_kernel(GruAsm a, int H, int W, void *hx, long long shx, long long n, long long G, size_t total)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const size_t b = i / (size_t)G;
    const long long at = (long long)(i - b * (size_t)G) * V;
    int k = 0;
#pragma unroll
    for (int j = 1; j < VPPX_GRU_MAX_SOURCES; j++)
        if (j < a.n && at >= a.s[j].first) k = j;
    const long long end = k + 1 < a.n ? a.s[k + 1].first : n;
    float c[V];
    if (V > 1 && at + V <= end && a.s[k].mode == VPPX_GRU_COPY && a.s[k].vec) {
        load_cells<BF16, (V > 1), V>(a.s[k].p, b * (size_t)a.s[k].stride + (size_t)(at - a.s[k].first), c);
        store_group<BF16, V>(hx, b * shx + at, c);
        return;
    }
    const int m = (int)((n - at) < V ? (n - at) : V);
    const long long plane = (long long)H * W, local = at - a.s[k].first;
    long long ch = local / plane, lim = end;
    int y = (int)(local - ch * plane) / W, x = (int)(local - ch * plane) - y * W;
    if (V > 1 && at + V <= end) {
        if (a.s[k].mode == VPPX_GRU_INTERP)
            gru_source_cells<BF16, V, VPPX_GRU_INTERP>(a.s[k], b, ch, y, x, H, W, c);
        else if (a.s[k].mode == VPPX_GRU_POOL2X)
            gru_source_cells<BF16, V, VPPX_GRU_POOL2X>(a.s[k], b, ch, y, x, H, W, c);
        else
            gru_source_cells<BF16, V, VPPX_GRU_COPY>(a.s[k], b, ch, y, x, H, W, c);
        store_group<BF16, V>(hx, b * shx + at, c);
        return;
    }
    for (int j = 0; j < m; j++) {
        if (at + j >= lim) { // the next source's first cell; every source has at least one
            k++, lim = k + 1 < a.n ? a.s[k + 1].first : n;
            ch = 0, y = 0, x = 0;
        }
        c[j] = gru_source_cell<BF16>(a.s[k], b, ch, y, x);
        if (++x == W) {
            x = 0;
            if (++y == H) y = 0, ch++;
        }
    }
    if (m == V) {
        store_group<BF16, V>(hx, b * shx + at, c);
    } else {
        for (int j = 0; j < m; j++) store_cell<BF16>(hx, b * shx + at + j, c[j]);
    }
}

// ---------------------------------------------------------------------------------------
// launchers (every argument has been checked by vppx_net_api.hip)
// ---------------------------------------------------------------------------------------
static int gru_grid(const char *who, int B, long long n, int V, long long *G, size_t *total, unsigned *blocks)
{
    *G = (n + V - 1) / V;
    *total = (size_t)B * (size_t)*G;
    const size_t nb = (*total + 255) / 256;
    if (nb > 0x7FFFFFFFull) {
        vppx_set_error("%s: %d frames of %lld cells are %zu workgroups, more than one launch takes", who, B, n, nb);
        return VPPX_E_UNSUPPORTED;
    }
    *blocks = (unsigned)nb;
    return 0;
}

// shx: cells between the frames of hx, at least the sources' channels; the cells of a frame behind them are not written
int gru_assemble(vppx_ctx *ctx, const VppxGruSource *src, int n_src, int B, int H, int W, void *hx, int64_t hx_frame_stride, int dtype)
{
    const bool bf16 = dtype == VPPX_DT_BF16;
    const int VF = bf16 ? 8 : 4;
    const long long plane = (long long)H * W, shx = (long long)hx_frame_stride;
    GruAsm a;
    memset(&a, 0, sizeof(a));
    a.n = n_src;
    long long n = 0;
    for (int k = 0; k < n_src; k++) {
        GruSrc &s = a.s[k];
        s.p = src[k].ptr, s.stride = (long long)src[k].frame_stride, s.first = n;
        s.Hs = src[k].Hs, s.Ws = src[k].Ws, s.mode = src[k].mode;
        s.sy = H > 1 ? (float)(s.Hs - 1) / (float)(H - 1) : 0.0f;
        s.sx = W > 1 ? (float)(s.Ws - 1) / (float)(W - 1) : 0.0f;
        s.vec = aligned16(s.p) && s.stride % VF == 0 && s.first % VF == 0;
        n += (long long)src[k].C * plane;
    }
    const int V = aligned16(hx) && shx % VF == 0 ? VF : 1;
    long long G;
    size_t total;
    unsigned blocks;
    int rc;
    if ((rc = gru_grid("vppx_raft_gru_assemble", B, n, V, &G, &total, &blocks))) return rc;
#define GRU_ASSEMBLE_LAUNCH(BF, VV) gru_assemble_kernel<BF, VV><<<dim3(blocks), 256, 0, ctx->stream>>>(a, H, W, hx, shx, n, G, total)
    CELLS_LAUNCH(bf16, V > 1, GRU_ASSEMBLE_LAUNCH);
#undef GRU_ASSEMBLE_LAUNCH
    VPPX_CHECK_LAUNCH();
    return 0;
}

int gru_reset(vppx_ctx *ctx, const void *ar, int64_t sar, const void *cr, int64_t scr, const void *h, int64_t sh, void *hx, int64_t shx,
              int B, int C, int H, int W, int dtype)
{
    const bool bf16 = dtype == VPPX_DT_BF16;
    const int VF = bf16 ? 8 : 4;
    const long long n = (long long)C * H * W;
    const bool vec = aligned16(ar) && aligned16(cr) && aligned16(h) && aligned16(hx) && sar % VF == 0 && scr % VF == 0 && sh % VF == 0 &&
                     shx % VF == 0;
    const int V = vec ? VF : 1;
    long long G;
    size_t total;
    unsigned blocks;
    int rc;
    if ((rc = gru_grid("vppx_raft_gru_reset", B, n, V, &G, &total, &blocks))) return rc;
#define GRU_RESET_LAUNCH(BF, VV) \
    gru_reset_kernel<BF, VV><<<dim3(blocks), 256, 0, ctx->stream>>>(ar, (long long)sar, cr, (long long)scr, h, (long long)sh, hx, (long long)shx, n, G, total)
    CELLS_LAUNCH(bf16, vec, GRU_RESET_LAUNCH);
#undef GRU_RESET_LAUNCH
    VPPX_CHECK_LAUNCH();
    return 0;
}

int gru_update(vppx_ctx *ctx, const void *az, int64_t saz, const void *cz, int64_t scz, const void *aq, int64_t saq, const void *cq,
               int64_t scq, const void *h, int64_t sh, void *out, int64_t so, int B, int C, int H, int W, int dtype)
{
    const bool bf16 = dtype == VPPX_DT_BF16;
    const int VF = bf16 ? 8 : 4;
    const long long n = (long long)C * H * W;
    const bool vec = aligned16(az) && aligned16(cz) && aligned16(aq) && aligned16(cq) && aligned16(h) && aligned16(out) && saz % VF == 0 &&
                     scz % VF == 0 && saq % VF == 0 && scq % VF == 0 && sh % VF == 0 && so % VF == 0;
    const int V = vec ? VF : 1;
    long long G;
    size_t total;
    unsigned blocks;
    int rc;
    if ((rc = gru_grid("vppx_raft_gru_update", B, n, V, &G, &total, &blocks))) return rc;
#define GRU_UPDATE_LAUNCH(BF, VV)                                                                                                        \
    gru_update_kernel<BF, VV><<<dim3(blocks), 256, 0, ctx->stream>>>(az, (long long)saz, cz, (long long)scz, aq, (long long)saq, cq,      \
                                                                     (long long)scq, h, (long long)sh, out, (long long)so, n, G, total)
    CELLS_LAUNCH(bf16, vec, GRU_UPDATE_LAUNCH);
#undef GRU_UPDATE_LAUNCH
    VPPX_CHECK_LAUNCH();
    return 0;
}
