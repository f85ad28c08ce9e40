// viz_kernels.hip -- gfx950 kernels of the pictures test.py saves per frame (utils.py:17-79, test.py:318-343) for a batch:
//   error colours      utils.color_error_image_kitti: the ten rows of _color_map_errors_kitti in order, a later row overwrites
//                      an earlier one, both ends of a bin inclusive, float32 error compared in double against lo / scale, hi / scale
//   guided_visualize   six maps from e = fabsf(disp - gt) (float32, no FMA contraction, as metrics_kernels.hip): 'bad k' for
//                      k = 1..4, 'avgerr' = error colours of e, 'rms' = error colours of sqrtf((disp - gt)^2); valid == 0 is black
//   colour-mapped map  lut[uint8(clamp(x, 0, max_val) / max_val * 255)], every step rounded to float32, then truncated
// each followed by cv2.dilate(img, ones((d, d))): per channel the maximum over the offsets -(d/2) .. d-1-(d/2) in both axes
// (anchor d/2: an even window leans up and left), pixels outside the frame ignored.
//
// One kernel, viz_kernel<MODE>.  A block owns a VZ_TW x VZ_TH tile of one frame.  The colour is a function of the pixel, so the
// block classifies tile + halo into LDS (one packed dword per pixel; what lies outside the frame is black, the identity of a
// maximum of bytes), takes the row maximum (one thread per pixel: consecutive lanes on consecutive banks), then the column
// maximum (one thread per four pixels, 16-byte LDS reads) and stores twelve bytes per thread: no un-dilated image goes through
// HBM, and a tile never reads another frame.  guided_visualize keeps disp - gt and the valid flag of tile + halo in LDS and
// runs the classify / maximum / store passes once per selected plane.  Every output byte is a function of its own frame's
// pixels only: deterministic and independent of the batch.
#include "vppx_internal.h"

#define VZ_TW 64
#define VZ_TH 16
#define VZ_THREADS 256
static_assert(VZ_THREADS == (VZ_TW / 4) * VZ_TH, "one thread per four pixels of the tile");

enum { VZ_ERR = 0, VZ_GUIDED = 1, VZ_CMAP = 2 };

// utils.py:4-15; colours packed channel 0 in the low byte
static const double kBinLo[10] = {0, 0.1875, 0.375, 0.75, 1.5, 3, 6, 12, 24, 48};
static const u8 kBinCol[10][3] = {{149, 54, 49}, {180, 117, 69}, {209, 173, 116}, {233, 217, 171}, {248, 243, 224},
                                  {144, 224, 254}, {97, 174, 253}, {67, 109, 244}, {39, 48, 215}, {38, 0, 165}};
#define VZ_BAD_ABOVE (49u | 54u << 8 | 149u << 16) // utils.py:46
#define VZ_BAD_BELOW (165u | 0u << 8 | 38u << 16)  // utils.py:47

struct VizArgs {
    const float *a, *b, *c; // VZ_ERR: errors, mask (may be null), -; VZ_GUIDED: disp, gt, valid; VZ_CMAP: x, max_val [B], -
    const u8 *lut;          // VZ_CMAP: [256][3]
    u8 *out;
    int B, H, W, d;         // d >= 1 (the launcher turns 0 into 1: both are the identity)
    int tiles_x, tiles_y;
    unsigned which;         // VZ_GUIDED: planes to write
    double lo[10], hi[10];  // bin edges divided by scale, in double (utils.py:22)
    u32 col[10];
};

static __device__ __forceinline__ u32 err_color(const VizArgs &a, float e)
{
    const double de = (double)e;
    u32 c = 0; // NaN matches no bin
#pragma unroll
    for (int k = 0; k < 10; k++)
        if (de >= a.lo[k] && de <= a.hi[k]) c = a.col[k];
    return c;
}

static __device__ __forceinline__ u32 bad_color(float e, float t) { return e > t ? VZ_BAD_ABOVE : e <= t ? VZ_BAD_BELOW : 0u; }

// test.py:325: torch.clamp, true division, times 255, astype(uint8).  The cast is undefined in the reference for a NaN; the
// index is 0 there: NaN input, max_val not > 0 (NaN included), NaN quotient (inf / inf)
static __device__ __forceinline__ int cmap_index(float x, float mv)
{
    if (!(mv > 0.f) || x != x) return 0;
    const float cl = fminf(fmaxf(x, 0.f), mv);
    const float q = __fmul_rn(__fdiv_rn(cl, mv), 255.f);
    return q != q ? 0 : (int)q;
}

template <int MODE>
__global__ void __launch_bounds__(VZ_THREADS) viz_kernel(const VizArgs a)
{
    extern __shared__ __align__(16) unsigned char smem[];
    __shared__ u32 s_lut[MODE == VZ_CMAP ? 256 : 1];
    const int d = a.d, anchor = d >> 1;
    const int HW = VZ_TW + d - 1, HH = VZ_TH + d - 1, NH = HH * HW;
    u32 *s_h = (u32 *)smem;                // [HH][VZ_TW] row maxima
    u32 *s_c = s_h + HH * VZ_TW;           // [HH][HW] colours of tile + halo
    float *s_diff = (float *)(s_c + NH);   // VZ_GUIDED: disp - gt
    u8 *s_valid = (u8 *)(s_diff + NH);     // VZ_GUIDED: inside the frame and valid != 0
    const int tid = threadIdx.x;
    unsigned blk = blockIdx.x;
    const int bx = blk % a.tiles_x;
    blk /= a.tiles_x;
    const int by = blk % a.tiles_y;
    const int f = blk / a.tiles_y;
    const int x0 = bx * VZ_TW, y0 = by * VZ_TH;
    const size_t npx = (size_t)a.H * a.W, fbase = (size_t)f * npx;

    if (MODE == VZ_CMAP) {
        s_lut[tid] = (u32)a.lut[3 * tid] | (u32)a.lut[3 * tid + 1] << 8 | (u32)a.lut[3 * tid + 2] << 16;
        __syncthreads();
    }
    if (MODE == VZ_GUIDED) {
        for (int i = tid; i < NH; i += VZ_THREADS) {
            const int hy = i / HW, hx = i - hy * HW;
            const int sy = y0 - anchor + hy, sx = x0 - anchor + hx;
            float df = 0.f;
            u8 v = 0;
            if (sy >= 0 && sy < a.H && sx >= 0 && sx < a.W) {
                const size_t p = fbase + (size_t)sy * a.W + sx;
                df = __fsub_rn(a.a[p], a.b[p]);
                v = !(a.c[p] == 0.f); // utils.py:48: valid == 0 is black, any other value (negative, NaN) is drawn
            }
            s_diff[i] = df;
            s_valid[i] = v;
        }
        __syncthreads();
    }
    const float mv = MODE == VZ_CMAP ? a.b[f] : 0.f;
    const int nplanes = MODE == VZ_GUIDED ? 6 : 1;
    const size_t plane_bytes = (size_t)a.B * npx * 3;
    const int ty = tid >> 4, tx4 = (tid & 15) << 2;
    for (int pl = 0; pl < nplanes; pl++) {
        if (MODE == VZ_GUIDED && !(a.which >> pl & 1)) continue; // (block-uniform)
        // colours of tile + halo
        for (int i = tid; i < NH; i += VZ_THREADS) {
            u32 c = 0;
            if (MODE == VZ_GUIDED) {
                if (s_valid[i]) {
                    const float df = s_diff[i];
                    if (pl < 4) c = bad_color(fabsf(df), (float)(pl + 1));
                    else if (pl == 4) c = err_color(a, fabsf(df));
                    else c = err_color(a, __fsqrt_rn(__fmul_rn(df, df))); // utils.py:74-75
                }
            } else {
                const int hy = i / HW, hx = i - hy * HW;
                const int sy = y0 - anchor + hy, sx = x0 - anchor + hx;
                if (sy >= 0 && sy < a.H && sx >= 0 && sx < a.W) {
                    const size_t p = fbase + (size_t)sy * a.W + sx;
                    if (MODE == VZ_ERR) {
                        c = err_color(a, a.a[p]);
                        if (a.b && a.b[p] == 0.f) c = 0; // utils.py:26: mask == 0, not mask > 0
                    } else {
                        c = s_lut[cmap_index(a.a[p], mv)];
                    }
                }
            }
            s_c[i] = c;
        }
        __syncthreads();
        const u32 *src = s_c; // d == 1: HW == VZ_TW, the colours are the result
        if (d > 1) {
            for (int i = tid; i < HH * VZ_TW; i += VZ_THREADS) {
                const int hy = i / VZ_TW, x = i - hy * VZ_TW;
                const u32 *row = s_c + hy * HW + x;
                u32 m0 = 0, m1 = 0, m2 = 0;
                for (int k = 0; k < d; k++) {
                    const u32 v = row[k];
                    m0 = max(m0, v & 0xffu);
                    m1 = max(m1, v & 0xff00u);
                    m2 = max(m2, v & 0xff0000u);
                }
                s_h[i] = m0 | m1 | m2;
            }
            __syncthreads();
            src = s_h;
        }
        // column maximum of four pixels, twelve bytes out
        const int y = y0 + ty, x = x0 + tx4;
        if (y < a.H && x < a.W) {
            u32 m[4][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
            for (int k = 0; k < d; k++) {
                const uint4 q = *(const uint4 *)(src + (ty + k) * VZ_TW + tx4);
                const u32 v[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    m[j][0] = max(m[j][0], v[j] & 0xffu);
                    m[j][1] = max(m[j][1], v[j] & 0xff00u);
                    m[j][2] = max(m[j][2], v[j] & 0xff0000u);
                }
            }
            u32 p[4];
#pragma unroll
            for (int j = 0; j < 4; j++) p[j] = m[j][0] | m[j][1] | m[j][2];
            u8 *o = a.out + (MODE == VZ_GUIDED ? pl * plane_bytes : 0) + (fbase + (size_t)y * a.W + x) * 3;
            const int n = a.W - x < 4 ? a.W - x : 4;
            if (n == 4 && ((uintptr_t)o & 3) == 0) {
                struct W3 { u32 w0, w1, w2; };
                W3 w;
                w.w0 = p[0] | p[1] << 24;
                w.w1 = p[1] >> 8 | p[2] << 16;
                w.w2 = p[2] >> 16 | p[3] << 8;
                *(W3 *)o = w;
            } else {
                for (int j = 0; j < n; j++) {
                    o[3 * j] = (u8)p[j];
                    o[3 * j + 1] = (u8)(p[j] >> 8);
                    o[3 * j + 2] = (u8)(p[j] >> 16);
                }
            }
        }
        // the next plane's colours overwrite s_c, which nobody reads after the barrier above; its row maxima overwrite s_h
        // behind the next barrier, which every thread reaches with this plane's column pass done
        if (MODE == VZ_GUIDED && d == 1) __syncthreads(); // d == 1 reads s_c in the column pass
    }
}

static size_t viz_lds_bytes(int mode, int d)
{
    const size_t HW = VZ_TW + d - 1, HH = VZ_TH + d - 1;
    size_t n = HH * VZ_TW * 4 + HH * HW * 4;
    if (mode == VZ_GUIDED) n += HH * HW * 4 + HH * HW;
    return (n + 15) & ~(size_t)15;
}

static int viz_launch(vppx_ctx *ctx, int mode, VizArgs &a, const char *name)
{
    if (a.d > VIZ_MAX_DILATION) {
        vppx_set_error("%s: dilation %d is above this build's limit of %d", name, a.d, VIZ_MAX_DILATION);
        return VPPX_E_UNSUPPORTED;
    }
    if (a.d < 1) a.d = 1;
    a.tiles_x = (a.W + VZ_TW - 1) / VZ_TW;
    a.tiles_y = (a.H + VZ_TH - 1) / VZ_TH;
    const unsigned long long nblk = (unsigned long long)a.tiles_x * a.tiles_y * a.B;
    if (nblk > 0x7fffffffull) {
        vppx_set_error("%s: %d frames of %d x %d are %llu tiles, above the limit of 2^31 - 1 per call", name, a.B, a.H, a.W, nblk);
        return VPPX_E_UNSUPPORTED;
    }
    const size_t lds = viz_lds_bytes(mode, a.d);
    if (mode == VZ_ERR) viz_kernel<VZ_ERR><<<(unsigned)nblk, VZ_THREADS, lds, ctx->stream>>>(a);
    else if (mode == VZ_GUIDED) viz_kernel<VZ_GUIDED><<<(unsigned)nblk, VZ_THREADS, lds, ctx->stream>>>(a);
    else viz_kernel<VZ_CMAP><<<(unsigned)nblk, VZ_THREADS, lds, ctx->stream>>>(a);
    VPPX_CHECK_LAUNCH();
    return 0;
}

static void viz_bins(VizArgs &a, double scale, bool bgr)
{
    for (int k = 0; k < 10; k++) {
        a.lo[k] = kBinLo[k] / scale;
        a.hi[k] = (k < 9 ? kBinLo[k + 1] : (double)INFINITY) / scale;
        const u8 *c = kBinCol[k];
        a.col[k] = bgr ? (u32)c[0] | (u32)c[1] << 8 | (u32)c[2] << 16 : (u32)c[2] | (u32)c[1] << 8 | (u32)c[0] << 16; // utils.py:28-29
    }
}

int viz_launch_error_colors(vppx_ctx *ctx, int B, int H, int W, const float *errors, const float *mask, double scale, int bgr,
                            int dilation, u8 *out)
{
    VizArgs a = {};
    a.a = errors; a.b = mask; a.out = out;
    a.B = B; a.H = H; a.W = W; a.d = dilation;
    viz_bins(a, scale, bgr != 0);
    return viz_launch(ctx, VZ_ERR, a, "vppx_error_colors");
}

int viz_launch_guided(vppx_ctx *ctx, int B, int H, int W, const float *disp, const float *gt, const float *valid, double scale,
                      int dilation, unsigned which, u8 *out)
{
    VizArgs a = {};
    a.a = disp; a.b = gt; a.c = valid; a.out = out;
    a.B = B; a.H = H; a.W = W; a.d = dilation;
    a.which = which;
    viz_bins(a, scale, true);
    return viz_launch(ctx, VZ_GUIDED, a, "vppx_guided_visualize");
}

int viz_launch_colorize(vppx_ctx *ctx, int B, int H, int W, const float *x, const float *max_val, const u8 *lut, int dilation, u8 *out)
{
    VizArgs a = {};
    a.a = x; a.b = max_val; a.lut = lut; a.out = out;
    a.B = B; a.H = H; a.W = W; a.d = dilation;
    return viz_launch(ctx, VZ_CMAP, a, "vppx_colorize");
}

// ---------------------------------------------------------------------------------------
// test.py:318: max of a frame with +-inf replaced by -inf.  torch's max propagates NaN: so does this.  Two stages, the blocks
// per frame a function of the frame's shape only; a maximum does not depend on the order it is taken in.
// ---------------------------------------------------------------------------------------
#define FM_THREADS 256

int viz_finite_max_blocks(size_t npx)
{
    size_t n = (npx + 4095) / 4096;
    if (n < 1) n = 1;
    if (n > VIZ_FMAX_MAX_BLOCKS) n = VIZ_FMAX_MAX_BLOCKS;
    return (int)n;
}

static __device__ __forceinline__ void fm_take(float v, float &m, int &nan)
{
    if (v != v) nan = 1;
    else if (fabsf(v) != INFINITY) m = fmaxf(m, v);
}

// folds a block's (m, nan) and returns the result in thread 0
static __device__ __forceinline__ float fm_fold(float m, int nan)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        m = fmaxf(m, __shfl_xor(m, off));
        nan |= __shfl_xor(nan, off);
    }
    __shared__ float s_m[FM_THREADS / 64];
    __shared__ int s_n[FM_THREADS / 64];
    if ((threadIdx.x & 63) == 0) {
        s_m[threadIdx.x >> 6] = m;
        s_n[threadIdx.x >> 6] = nan;
    }
    __syncthreads();
    for (int w = 0; w < (int)blockDim.x / 64; w++) {
        m = fmaxf(m, s_m[w]);
        nan |= s_n[w];
    }
    return nan ? __int_as_float(0x7fc00000) : m;
}

// grid (blocks per frame, B): part[f][block] = that block's maximum (NaN when it saw one)
__global__ void __launch_bounds__(FM_THREADS) finite_max_partial_kernel(const float *__restrict__ x, float *__restrict__ part, size_t npx,
                                                                        size_t chunk)
{
    x += (size_t)blockIdx.y * npx;
    const size_t lo = (size_t)blockIdx.x * chunk;
    const size_t hi = lo + chunk < npx ? lo + chunk : npx;
    float m = -INFINITY;
    int nan = 0;
    for (size_t i = lo + threadIdx.x; i < hi; i += FM_THREADS) fm_take(x[i], m, nan);
    const float r = fm_fold(m, nan);
    if (threadIdx.x == 0) part[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = r;
}

__global__ void __launch_bounds__(64) finite_max_finish_kernel(const float *__restrict__ part, int nblk, float *__restrict__ out)
{
    float m = -INFINITY;
    int nan = 0;
    for (int k = threadIdx.x; k < nblk; k += 64) {
        const float v = part[(size_t)blockIdx.x * nblk + k];
        if (v != v) nan = 1;
        else m = fmaxf(m, v); // (a partial is never +inf)
    }
    const float r = fm_fold(m, nan);
    if (threadIdx.x == 0) out[blockIdx.x] = r;
}

int viz_launch_finite_max(vppx_ctx *ctx, int B, int H, int W, const float *x, float *part, float *out)
{
    const size_t npx = (size_t)H * W;
    const int nblk = viz_finite_max_blocks(npx);
    const size_t chunk = (npx + nblk - 1) / nblk;
    finite_max_partial_kernel<<<dim3((unsigned)nblk, (unsigned)B), FM_THREADS, 0, ctx->stream>>>(x, part, npx, chunk);
    VPPX_CHECK_LAUNCH();
    finite_max_finish_kernel<<<B, 64, 0, ctx->stream>>>(part, nblk, out);
    VPPX_CHECK_LAUNCH();
    return 0;
}
