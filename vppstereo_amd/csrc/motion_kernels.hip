// motion_kernels.hip -- gfx950 kernel for the front of BasicMotionEncoder.forward (models/raft_stereo/update.py:80,82):
//   cor1 = relu(convc1(corr_fn(coords)))   the lookup (corr.py:126-145) fused into the 1x1 convolution that reads it
//   flo1 = relu(convf1(flow))              the ks x ks convolution over the two flow channels
// in one launch.  The [B, levels*(2r+1), H4, W2] tensor of taps is never written: include/vppx.h has the arithmetic.
//
// Both convolutions are GEMMs on the f32 matrix path (v_mfma_f32_16x16x4_f32) with the pixels on M and the output channels
// on N: A[pixel = lane & 15][k = lane >> 4] is one tap (convc1) or one flow cell of the pixel's window (convf1), B[k][channel]
// one weight.  A lane computes exactly the operand it feeds, straight into its A register: the K = levels*(2r+1) taps of 16
// pixels are K/4 steps, no tap is computed twice and none passes through LDS.  The taps are corr_tap's, the lookup kernel's
// own code, so they are bit for bit what vppx_raft_corr_lookup_dt_dev would have stored.
//
// A wave owns 32 consecutive pixels n = (b, y, x) of the flat [B*H4*W2] index as two M tiles whose rows are interleaved as
// corr_gemm_kernels.hip interleaves its own (row r of tile t is pixel 8 * (r >> 2) + 4 * t + (r & 3)): with the 16x16 C/D map
// (column = lane & 15, row = 4 * (lane >> 4) + register) a lane's registers of a tile pair are EIGHT consecutive pixels of one
// output channel, 32 contiguous bytes in float32 and 16 in bfloat16.  A workgroup of four waves takes chunks of 128 pixels.
// The weights lie in LDS, transposed to [k][channel] with K padded to a multiple of 4 by zero rows, and stay there for every
// chunk of the workgroup; rows are MF_SW cells apart so that the four k rows of one fragment read start in different banks.
// What a step's k means (level and tap, or channel, dy and dx) is looked up in a table made once per workgroup.
// The flow window is read from memory as it is (two channels of a frame are 0.26 MB at 544x960 and stay in the caches).
#include "corr_shared.h"

#include <math.h>

#define MF_PIX 128 // pixels per chunk: four waves of 32
#define MF_SW (VPPX_MOTION_MAX_CH + 16)

typedef float mf_f32x4 __attribute__((ext_vector_type(4)));

struct MotionArgs {
    const void *corr, *pyr;
    CorrLevels lv;
    const float *coords_x, *flow, *wc, *bias_c, *wf, *bias_f;
    void *out_c, *out_f;
    long long cstride, fstride, ocstride, ofstride; // cells between frames
    unsigned n_pix, plane, nchunks;
    int H4, W2, W3, levels, radius, Cc, Cf, ks, Kc, Kf, KcP, KfP; // K*: levels*(2r+1) and 2*ks*ks; K*P: padded to 4
    unsigned vec; // bit 0 / 1: out_c / out_f may be written with 16-byte stores
};

// The eight cells c[] of channel m from flat pixel n0 on.  vec: the base and the frame stride are whole 16-byte groups and
// so is a plane, so a group of 4 float32 (8 bfloat16) cells lies inside one frame, wholly inside the tensor or wholly outside.
template <bool OBF16>
__device__ __forceinline__ void mf_store8(void *out, long long stride, unsigned plane, unsigned n0, unsigned n_pix, int m, const float *c,
                                          bool vec)
{
    if (n0 >= n_pix) return;
    unsigned b = n0 / plane, p = n0 - b * plane;
    if (vec) {
        if (OBF16) {
            u32 h[8];
#pragma unroll
            for (int j = 0; j < 8; j++) h[j] = bf16_rne(c[j]);
            *(uint4 *)((u16 *)out + (size_t)b * (size_t)stride + (size_t)m * plane + p) =
                make_uint4(h[0] | (h[1] << 16), h[2] | (h[3] << 16), h[4] | (h[5] << 16), h[6] | (h[7] << 16));
        } else {
            *(float4 *)((float *)out + (size_t)b * (size_t)stride + (size_t)m * plane + p) = make_float4(c[0], c[1], c[2], c[3]);
            const unsigned n1 = n0 + 4;
            if (n1 < n_pix) {
                b = n1 / plane, p = n1 - b * plane;
                *(float4 *)((float *)out + (size_t)b * (size_t)stride + (size_t)m * plane + p) = make_float4(c[4], c[5], c[6], c[7]);
            }
        }
        return;
    }
#pragma unroll
    for (int j = 0; j < 8; j++) {
        if (n0 + j < n_pix) {
            const size_t at = (size_t)b * (size_t)stride + (size_t)m * plane + p;
            if (OBF16)
                ((u16 *)out)[at] = (u16)bf16_rne(c[j]);
            else
                ((float *)out)[at] = c[j];
        }
        if (++p == plane) p = 0, b++;
    }
}

// relu(acc + bias) of the wave's tile pair, N tile by N tile
template <bool OBF16>
__device__ __forceinline__ void mf_emit(const mf_f32x4 (&acc)[2][4], int ntiles, const float *sBias, void *out, long long stride,
                                        unsigned plane, unsigned n0, unsigned n_pix, int i, bool vec)
{
#pragma unroll
    for (int n = 0; n < 4; n++) {
        if (n >= ntiles) break;
        const int m = 16 * n + i;
        const float bias = sBias[m];
        float c[8];
#pragma unroll
        for (int j = 0; j < 8; j++) c[j] = relu_nan(__fadd_rn(acc[j >> 2][n][j & 3], bias));
        mf_store8<OBF16>(out, stride, plane, n0, n_pix, m, c, vec);
    }
}

template <bool BF16, bool OBF16>
__global__ void __launch_bounds__(256) raft_motion_front_kernel(MotionArgs a)
{
    extern __shared__ __attribute__((aligned(16))) float mf_lds[];
    float *sWc = mf_lds;                // [KcP][MF_SW]
    float *sWf = sWc + a.KcP * MF_SW;   // [KfP][MF_SW]
    float *sBias = sWf + a.KfP * MF_SW; // bias_c at 0, bias_f at VPPX_MOTION_MAX_CH
    int *sTc = (int *)(sBias + 2 * VPPX_MOTION_MAX_CH); // [KcP]: level << 8 | tap, -1 for a padding row
    int *sTf = sTc + a.KcP;                             // [KfP]: channel << 16 | dy << 8 | dx, -1 for a padding row

    const int tid = threadIdx.x;
    for (int k = tid; k < (a.KcP + a.KfP) * MF_SW; k += 256) mf_lds[k] = 0.0f;
    for (int k = tid; k < 2 * VPPX_MOTION_MAX_CH; k += 256) {
        const int m = k & (VPPX_MOTION_MAX_CH - 1);
        const float *bias = k < VPPX_MOTION_MAX_CH ? a.bias_c : a.bias_f;
        sBias[k] = bias && m < (k < VPPX_MOTION_MAX_CH ? a.Cc : a.Cf) ? bias[m] : 0.0f;
    }
    const int taps = 2 * a.radius + 1, ks2 = a.ks * a.ks;
    for (int k = tid; k < a.KcP; k += 256) sTc[k] = k < a.Kc ? ((k / taps) << 8) | (k % taps) : -1;
    for (int k = tid; k < a.KfP; k += 256) sTf[k] = k < a.Kf ? ((k / ks2) << 16) | (((k % ks2) / a.ks) << 8) | ((k % ks2) % a.ks) : -1;
    __syncthreads();
    for (int k = tid; k < a.Cc * a.Kc; k += 256) sWc[(k % a.Kc) * MF_SW + k / a.Kc] = a.wc[k];
    for (int k = tid; k < a.Cf * a.Kf; k += 256) sWf[(k % a.Kf) * MF_SW + k / a.Kf] = a.wf[k];
    __syncthreads();

    const int wave = tid >> 6, lane = tid & 63, g = lane >> 4, i = lane & 15;
    const int pad = a.ks / 2, nc = a.Cc >> 4, nf = a.Cf >> 4;
    const unsigned plane = a.plane, n_pix = a.n_pix;

    for (unsigned chunk = blockIdx.x; chunk < a.nchunks; chunk += gridDim.x) { // no barrier inside: a wave may leave early
        const unsigned nw = chunk * MF_PIX + wave * 32;
        if (nw >= n_pix) continue;
        // the two pixels whose operands this lane makes: row i of tiles 0 and 1
        unsigned np[2], bp[2];
        int yp[2], xp[2];
        bool ok[2];
        float cx[2];
#pragma unroll
        for (int t = 0; t < 2; t++) {
            np[t] = nw + 8 * (i >> 2) + 4 * t + (i & 3);
            ok[t] = np[t] < n_pix;
            const unsigned n = ok[t] ? np[t] : 0;
            bp[t] = n / plane;
            const unsigned p = n - bp[t] * plane;
            yp[t] = (int)(p / (unsigned)a.W2), xp[t] = (int)(p - (unsigned)yp[t] * a.W2);
            cx[t] = ok[t] ? a.coords_x[(size_t)bp[t] * (size_t)a.cstride + p] : 0.0f;
        }
        const unsigned n0 = nw + 8 * g; // the first of the eight pixels whose results this lane holds

        mf_f32x4 acc[2][4];
#pragma unroll
        for (int t = 0; t < 2; t++)
#pragma unroll
            for (int n = 0; n < 4; n++) acc[t][n] = (mf_f32x4){0.0f, 0.0f, 0.0f, 0.0f};
        for (int k = g; k < a.KcP; k += 4) {
            const int tab = sTc[k];
            float fa[2] = {0.0f, 0.0f};
            if (tab >= 0) {
                const int lvl = tab >> 8, t = tab & 255, W = a.W3 >> lvl;
                const float wm1 = (float)(W - 1), scale = (float)(1 << lvl);
                const void *level = lvl ? a.pyr : a.corr;
#pragma unroll
                for (int tt = 0; tt < 2; tt++) {
                    if (!ok[tt]) continue;
                    const size_t base = (lvl ? (size_t)a.lv.off[lvl] : 0) + (size_t)np[tt] * (size_t)W;
                    fa[tt] = corr_tap<BF16>((const float *)level + base, (const u16 *)level + base, wm1, __fdiv_rn(cx[tt], scale), t, a.radius);
                }
            }
            const float *pb = sWc + k * MF_SW + i;
#pragma unroll
            for (int n = 0; n < 4; n++) {
                if (n >= nc) break;
                const float fb = pb[16 * n];
                acc[0][n] = __builtin_amdgcn_mfma_f32_16x16x4f32(fa[0], fb, acc[0][n], 0, 0, 0);
                acc[1][n] = __builtin_amdgcn_mfma_f32_16x16x4f32(fa[1], fb, acc[1][n], 0, 0, 0);
            }
        }
        mf_emit<OBF16>(acc, nc, sBias, a.out_c, a.ocstride, plane, n0, n_pix, i, a.vec & 1u);

#pragma unroll
        for (int t = 0; t < 2; t++)
#pragma unroll
            for (int n = 0; n < 4; n++) acc[t][n] = (mf_f32x4){0.0f, 0.0f, 0.0f, 0.0f};
        for (int k = g; k < a.KfP; k += 4) {
            const int tab = sTf[k];
            float fa[2] = {0.0f, 0.0f};
            if (tab >= 0) {
                const int c = tab >> 16, dy = (tab >> 8) & 255, dx = tab & 255;
#pragma unroll
                for (int tt = 0; tt < 2; tt++) {
                    const int yy = yp[tt] + dy - pad, xx = xp[tt] + dx - pad;
                    if (ok[tt] && yy >= 0 && yy < a.H4 && xx >= 0 && xx < a.W2)
                        fa[tt] = a.flow[(size_t)bp[tt] * (size_t)a.fstride + (size_t)c * plane + (size_t)yy * a.W2 + xx];
                }
            }
            const float *pb = sWf + k * MF_SW + i;
#pragma unroll
            for (int n = 0; n < 4; n++) {
                if (n >= nf) break;
                const float fb = pb[16 * n];
                acc[0][n] = __builtin_amdgcn_mfma_f32_16x16x4f32(fa[0], fb, acc[0][n], 0, 0, 0);
                acc[1][n] = __builtin_amdgcn_mfma_f32_16x16x4f32(fa[1], fb, acc[1][n], 0, 0, 0);
            }
        }
        mf_emit<OBF16>(acc, nf, sBias + VPPX_MOTION_MAX_CH, a.out_f, a.ofstride, plane, n0, n_pix, i, a.vec & 2u);
    }
}

// ---------------------------------------------------------------------------------------
// launcher (every argument has been checked by vppx_net_api.hip)
// ---------------------------------------------------------------------------------------
int motion_front(vppx_ctx *ctx, const void *corr, const void *pyr, const float *coords_x, int64_t coords_frame_stride, const float *flow,
                 int64_t flow_frame_stride, const float *wc, const float *bias_c, int Cc, const float *wf, const float *bias_f, int Cf,
                 int ks, int B, int H4, int W2, int W3, int levels, int radius, void *out_c, int64_t out_c_frame_stride, void *out_f,
                 int64_t out_f_frame_stride, int dtype, int out_dtype)
{
    const size_t plane = (size_t)H4 * W2, n_pix = plane * B;
    if (n_pix > 0x7FFFFFFFull) {
        vppx_set_error("vppx_raft_motion_front: B*H4*W2 = %zu pixels are more than one launch takes", n_pix);
        return VPPX_E_UNSUPPORTED;
    }
    MotionArgs a = {};
    a.corr = corr, a.pyr = pyr, a.lv = corr_levels(pyr, n_pix, W3, levels, dtype, corr);
    a.coords_x = coords_x, a.flow = flow, a.wc = wc, a.bias_c = bias_c, a.wf = wf, a.bias_f = bias_f;
    a.out_c = out_c, a.out_f = out_f;
    a.cstride = (long long)coords_frame_stride, a.fstride = (long long)flow_frame_stride;
    a.ocstride = (long long)out_c_frame_stride, a.ofstride = (long long)out_f_frame_stride;
    a.n_pix = (unsigned)n_pix, a.plane = (unsigned)plane, a.nchunks = (unsigned)((n_pix + MF_PIX - 1) / MF_PIX);
    a.H4 = H4, a.W2 = W2, a.W3 = W3, a.levels = levels, a.radius = radius, a.Cc = Cc, a.Cf = Cf, a.ks = ks;
    a.Kc = levels * (2 * radius + 1), a.Kf = 2 * ks * ks;
    a.KcP = (a.Kc + 3) & ~3, a.KfP = (a.Kf + 3) & ~3;
    const bool obf16 = out_dtype == VPPX_DT_BF16;
    const size_t group = obf16 ? 8 : 4; // cells of 16 bytes
    if ((uintptr_t)out_c % 16 == 0 && (size_t)out_c_frame_stride % group == 0 && plane % group == 0) a.vec |= 1u;
    if ((uintptr_t)out_f % 16 == 0 && (size_t)out_f_frame_stride % group == 0 && plane % group == 0) a.vec |= 2u;
    // the weights are read into LDS once per workgroup: beyond a few workgroups per compute unit a workgroup takes several chunks
    const unsigned grid = a.nchunks < 1024u ? a.nchunks : 1024u;
    const size_t lds = ((size_t)(a.KcP + a.KfP) * MF_SW + 2 * VPPX_MOTION_MAX_CH) * sizeof(float) + (size_t)(a.KcP + a.KfP) * sizeof(int);
    const bool bf16 = dtype == VPPX_DT_BF16;
    if (bf16 && obf16)
        raft_motion_front_kernel<true, true><<<dim3(grid), 256, lds, ctx->stream>>>(a);
    else if (bf16)
        raft_motion_front_kernel<true, false><<<dim3(grid), 256, lds, ctx->stream>>>(a);
    else if (obf16)
        raft_motion_front_kernel<false, true><<<dim3(grid), 256, lds, ctx->stream>>>(a);
    else
        raft_motion_front_kernel<false, false><<<dim3(grid), 256, lds, ctx->stream>>>(a);
    VPPX_CHECK_LAUNCH();
    return 0;
}
