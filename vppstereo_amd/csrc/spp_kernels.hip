// spp_kernels.hip -- gfx950 kernel for the average pools of PSMNet's pyramid pooling (models/psmnet/submodule.py:149-171
// branch1 .. branch4: nn.AvgPool2d((k, k), stride=(k, k)) for k = 64, 32, 16, 8 over one [B,128,H4,W4] tensor): every level in
// one launch, a workgroup per plane.  include/vppx.h has the arithmetic, tests/_psm_ref.py the float64 referee.
//
// Level i is out_i[y][x] = (the float32 sum of the k_i x k_i cells of its window) / (float)(k_i * k_i), rows and columns behind
// (H / k_i) * k_i and (W / k_i) * k_i not being read for that level.  The sum's order:
//   shared route (g = gcd of the k_i, and the grid of (H / g) x (W / g) sums fits SPP_GRID cells of LDS): a thread adds the g x g
//     cells of one grid cell in row order to +0; a level then adds its (k_i / g) x (k_i / g) grid cells in row order to +0.  x is
//     read once for all levels.  Grid row r belongs to level i only where r < (H / k_i) * (k_i / g) <= H / g: a level's windows
//     never reach a grid cell that holds a row or column behind its own floor boundary.
//   direct route (the grid does not fit: small k over a large map): a thread adds the k_i x k_i cells of its window in row order
//     to +0, level by level.
// Which route a call takes and which thread adds what depend on (H, W, ks) alone, never on the dispatch: no atomics, the same
// bits run after run.  Storage is float32 or bfloat16 (widened on load, rounded once on store), cell by cell: no alignment
// is asked of any pointer.
#include "cells.h"

#define SPP_THREADS 256
#define SPP_GRID 8192 // float32 cells of LDS for the shared sums: 32 KB

struct SppArgs {
    void *out[VPPX_SPP_MAX_LEVELS];
    int k[VPPX_SPP_MAX_LEVELS];
    int n;      // levels
    int g;      // shared route: the edge of a grid cell;  0: the direct route
    int Hg, Wg; // shared route: the grid's size, H / g by W / g
};

template <bool BF16>
__global__ void __launch_bounds__(SPP_THREADS) spp_pool_kernel(const void *x, long long sx, int C, int H, int W, SppArgs a)
{
    __shared__ float grid[SPP_GRID];
    const size_t plane = blockIdx.x, b = plane / (unsigned)C, c = plane - b * (unsigned)C;
    const size_t base = b * (size_t)sx + c * (size_t)H * W;
    const int g = a.g, Wg = a.Wg;
    if (g) {
        const int cells = a.Hg * Wg; // <= SPP_GRID: the launcher chose the route
        for (int cell = threadIdx.x; cell < cells; cell += SPP_THREADS) {
            const int yy = cell / Wg, xx = cell - yy * Wg;
            const size_t at = base + (size_t)(yy * g) * W + (size_t)(xx * g);
            float acc = 0.0f;
            for (int r = 0; r < g; r++)
                for (int q = 0; q < g; q++) acc = __fadd_rn(acc, load_cell<BF16>(x, at + (size_t)r * W + q));
            grid[cell] = acc;
        }
        __syncthreads();
    }
    for (int i = 0; i < a.n; i++) {
        const int k = a.k[i], Ho = H / k, Wo = W / k, m = g ? k / g : 0;
        const float div = (float)(k * k);
        for (int o = threadIdx.x; o < Ho * Wo; o += SPP_THREADS) {
            const int oy = o / Wo, ox = o - oy * Wo;
            float acc = 0.0f;
            if (g) {
                for (int r = 0; r < m; r++)
                    for (int q = 0; q < m; q++) acc = __fadd_rn(acc, grid[(oy * m + r) * Wg + ox * m + q]);
            } else {
                const size_t at = base + (size_t)(oy * k) * W + (size_t)(ox * k);
                for (int r = 0; r < k; r++)
                    for (int q = 0; q < k; q++) acc = __fadd_rn(acc, load_cell<BF16>(x, at + (size_t)r * W + q));
            }
            store_cell<BF16>(a.out[i], plane * (size_t)(Ho * Wo) + o, __fdiv_rn(acc, div));
        }
    }
}

static int spp_gcd(int p, int q)
{
    while (q) {
        const int t = p % q;
        p = q, q = t;
    }
    return p;
}

// every argument has been checked by vppx_net_api.hip: 1 <= k <= VPPX_SPP_MAX_K, H / k and W / k >= 1, B * C planes fit a launch
int spp_pool(vppx_ctx *ctx, const void *x, int64_t sx, int B, int C, int H, int W, int n_levels, const int *ks, void *const *outs, int dtype)
{
    SppArgs a = {};
    a.n = n_levels;
    int g = 0;
    for (int i = 0; i < n_levels; i++) {
        a.out[i] = outs[i], a.k[i] = ks[i];
        g = spp_gcd(g, ks[i]);
    }
    a.Hg = H / g, a.Wg = W / g;
    a.g = (long long)a.Hg * a.Wg <= SPP_GRID ? g : 0;
    const unsigned blocks = (unsigned)B * (unsigned)C;
    if (dtype == VPPX_DT_BF16)
        spp_pool_kernel<true><<<dim3(blocks), SPP_THREADS, 0, ctx->stream>>>(x, (long long)sx, C, H, W, a);
    else
        spp_pool_kernel<false><<<dim3(blocks), SPP_THREADS, 0, ctx->stream>>>(x, (long long)sx, C, H, W, a);
    VPPX_CHECK_LAUNCH();
    return 0;
}
