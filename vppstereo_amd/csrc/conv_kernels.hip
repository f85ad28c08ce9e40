// conv_kernels.hip -- gfx950 implicit-GEMM kernel for nn.Conv2d(Cin, Cout, 3, padding=1), stride 1 (2: below), on the matrix cores, with
// the gates of ConvGRU.forward (models/raft_stereo/update.py:23-32) as epilogues: include/vppx.h has the arithmetic.
//   M = pixels, N = output channels, K = 9 * Cin.  bfloat16 storage: v_mfma_f32_16x16x32_bf16; float32 storage:
//   v_mfma_f32_16x16x4_f32 (exact float32 products, 1/16 of the bfloat16 rate).  Accumulation is float32 either way.
//
// Tile.  A workgroup of four waves owns CV_TH x CV_TW = 8 x 32 pixels of one frame and CV_NB = 64 output channels
// (blockIdx.y counts the channel blocks).  A wave owns two rows of the tile: per row two M tiles of 16 pixels whose rows are
// interleaved as motion_kernels.hip interleaves its own (row r of tile t is pixel 8 * (r >> 2) + 4 * t + (r & 3) of the 32), so
// that with the 16x16 C/D map (column = lane & 15 = channel, row = 4 * (lane >> 4) + register) a lane's registers of a tile
// pair are EIGHT consecutive pixels of one output channel: 16 bytes of bfloat16, two 16-byte groups of float32.  4 M tiles x
// 4 N tiles = 16 accumulators of 4 registers per lane.
//
// K runs in chunks of CK input channels (32 bfloat16, 16 float32: 64 bytes per pixel either way) and, inside a chunk, over the
// nine taps.  A chunk's activations -- the tile and its one-pixel halo, 10 x 34 pixels, +0 outside the map and for channels
// beyond Cin -- are staged into LDS TRANSPOSED to [pixel][channel], rows CV_ROWB = 80 bytes apart, so that a lane's A
// fragment of any tap (8 bfloat16 channels, or 4 float32 channels = the four k-steps of a chunk) is one 16-byte LDS read at the
// shifted pixel.  A thread reads its 22 four-byte units of the NEXT chunk into registers before the matrix instructions of
// the current one and writes them to LDS behind the barrier that ends it, so the loads' latency lies under the arithmetic
// (one LDS image, two barriers per chunk).  The weights come from the packed buffer in fragment order, [chunk][tap][N tile][lane] 16 bytes: a wave's B
// fragment is 1 KiB of contiguous memory, the same for the four waves of a workgroup, read one step ahead of its use.
// A packed weight of a channel beyond Cin is +0 and meets only the +0 the staging wrote, never a cell of the input.
//
// The plain epilogue also serves the update block's other convolutions (vppx_raft_conv_*): any Cout >= 1 (the packing pads the
// output channels to 16 with +0 rows and +0 bias slots, the store skips channel m >= Cout), a 1x1 kernel (TAPS = 1) and a scale.
//
// Stride 2 (STRIDE = 2, plain epilogue only; the encoders' layerN[0].conv1 and downsample[0]).  Tiles, the epilogue and the tile
// count are in OUTPUT pixels, Ho = (H - 1) / 2 + 1 and Wo likewise; the packed weights are those of stride 1.
//   1x1: output pixel (y, x) is input cell (2y, 2x).  The staged image is the TAPS = 1 image of stride 1, fetched at doubled
//     source offsets: no cell of an odd row or column is read.
//   3x3: output pixel (y, x) sums input rows 2y-1 .. 2y+1 and columns 2x-1 .. 2x+1.  A tile is CV_TH2 x CV_TW = 4 x 32 output
//     pixels, one row and two M tiles per wave: its footprint of 9 x 65 input pixels is 46.8 KB of LDS, so that two workgroups
//     still share a CU (8 x 32 would need 17 x 65 pixels = 88 KB, more than a static array holds).  A staged row is split by
//     COLUMN PARITY: first the 33 odd columns 2 (x0 + q) - 1, q = 0 .. 32, then the 32 even columns 2 (x0 + q).  Tap dx = 0 of
//     output pixel x0 + xl is then slot xl, dx = 1 slot 33 + xl and dx = 2 slot xl + 1: the pixels of an M tile lie CV_ROWB
//     bytes apart as at stride 1, with the bank pattern of stride 1 (at 160 bytes, pixels 8 apart start on the same bank, and
//     an M tile's rows are pixels 0-3, 8-11, 16-19, 24-27: the lanes of a read group would collide at least two ways), and the
//     A fragment stays one 16-byte read per lane and tap.
//
// Dilation 2 (DIL = 2: nine taps, stride 1, plain epilogue only; PSMNet's layer4).  Tap (dy, dx) of output pixel (y, x) is input
// cell (y + 2 (dy - 1), x + 2 (dx - 1)).  The staged image is the tile and a TWO-pixel halo, 12 x 36 = 432 pixels = 34.6 KB, so two
// workgroups still share a CU, and tap (dy, dx) is the staged pixel 2 dy rows and 2 dx columns behind the lane's own at tap (0, 0).
// The lanes of a read are the pixels of one M tile in one staged row, CV_ROWB bytes apart exactly as at dilation 1; a tap moves
// all of them by the same 2 dx * 80 + 2 dy * 36 * 80 bytes, and a shift common to every lane of a read changes which bank each
// lane starts on but not which lanes share one (160 bytes = 40 banks; at dilation 1 a tap step is 20 banks): the bank pattern of
// a read is that of stride 1, one 16-byte read per lane and tap.  Staging: thread tid stages pixel tid whole, and the 176 pixels
// beyond the first 256 are 2816 = 11 * 256 units, unit e = 256 j + tid being unit e / 176 of pixel 256 + e % 176 (neighbouring
// threads read neighbouring pixels of one channel): 27 units per thread, every thread the same, read one chunk ahead.
//
// Volume (VOL: nine taps, stride 1, dilation 1, plain epilogue only; PSMNet's stride-1 Conv3d(k=3, padding=1)).  A 3x3x3
// convolution of x [B,C,D,H,W] is, for output plane (b, d), the 3x3 convolution over 3 C pseudo-channels: pseudo-channel
// q = dz * C + c is plane d + dz - 1 of channel c, +0 (no load) where that plane is outside 0 .. D-1, and its weights are
// w2[m][q][dy][dx] = w[m][c][dz][dy][dx], which is what the packing writes.  A frame of the launch is a plane: frame index
// t -> (b = t / D, d = t % D).  Only `unit` (the source address: channels D*H*W apart, the plane's offset on top) and the
// epilogue's addresses (m * D*H*W + d * H*W) know; tile, LDS image, tap loop and both store routes are those of stride 1.  With
// C % 16 == 0 a float32 chunk lies in one plane and the two channels of a bfloat16 unit do; a bfloat16 chunk may hold the last 16
// channels of one plane and the first 16 of the next (C = 16, 48): `unit` decides per unit.
//
// A residual (plain epilogue): v = acc + bias, then v + res[b][m][y][x] before the ReLU and the scale, res being read by the lane
// that writes the cell, so that out may be res itself.
#include "cells.h"
#include "gru_math.h"

#define CV_TH 8
#define CV_TW 32
#define CV_HW (CV_TW + 2)
#define CV_HALO ((CV_TH + 2) * CV_HW)
#define CV_TH2 4                 // rows of a tile of the 3x3 at stride 2
#define CV_ODD2 (CV_TW + 1)      // odd columns of a staged row there, in front of the CV_TW even ones
#define CV_HW2 (2 * CV_TW + 1)
#define CV_HALO2 ((2 * CV_TH2 + 1) * CV_HW2)
#define CV_HWD (CV_TW + 4)       // dilation 2: a staged row with its two-pixel halo
#define CV_HALOD ((CV_TH + 4) * CV_HWD)
#define CV_ROWB 80
#define CV_NB 64

typedef float cv_f32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 cv_bf16x8 __attribute__((ext_vector_type(8)));

struct ConvArgs {
    const void *x0, *x1;     // the two sources of the input; x1 is unused where C1 == 0
    long long s0, s1;        // cells between frames
    const uint4 *packed;     // [chunk][tap][N tile][lane] fragments
    const float *bias;       // [Cout], behind the fragments
    const void *e0, *e1, *e2; // epilogue inputs: zr: cz, cr, h;  q: cq, z, h;  plain: e0 = the residual where res != 0
    long long se0, se1, se2;
    void *o0, *o1;           // plain: out;  zr: z, rh;  q: out
    long long so0, so1;
    int C0, Cin, NT, nchunks; // NT = ceil(Cout / 16): the packing pads the output channels with rows of +0
    int H, W, tilesX, tilesY; // H, W: the OUTPUT's size (the input's too at stride 1)
    int C, relu, vec;        // C: the hidden size of the gates;  vec: 16-byte groups in the epilogue
    int Cout;                // plain: channel m is stored where m < Cout (the gates' Cout is NT * 16)
    float scale;             // plain: out = relu(v) * scale
    int Hi, Wi;              // STRIDE == 2: the input's size
    int res;                 // plain: v += e0[b][m][y][x] in front of the ReLU
    int D;                   // VOL: planes of a frame; C0 is then the volume's channels and Cin = 3 * C0 the pseudo-channels
};

// Eight cells of a [B,C,H,W] tensor from cell `at` on, the first `nv` of them inside the row.  vec: every base, stride, plane
// and row of the call is a whole number of 16-byte groups, so a group of 4 float32 (8 bfloat16) cells is wholly inside or outside.
template <bool BF16>
__device__ __forceinline__ void cv_load8(const void *p, size_t at, int nv, bool vec, float *c)
{
    if (vec) {
        if (BF16) {
            load_cells<true, true, 8>(p, at, c);
        } else {
            load_cells<false, true, 4>(p, at, c);
            if (nv > 4)
                load_cells<false, true, 4>(p, at + 4, c + 4);
            else
                c[4] = c[5] = c[6] = c[7] = 0.0f;
        }
        return;
    }
#pragma unroll
    for (int j = 0; j < 8; j++) c[j] = j < nv ? load_cell<BF16>(p, at + j) : 0.0f;
}

template <bool BF16>
__device__ __forceinline__ void cv_store8(void *p, size_t at, int nv, bool vec, const float *c)
{
    if (vec) {
        if (BF16) {
            store_group<true, 8>(p, at, c);
        } else {
            store_group<false, 4>(p, at, c);
            if (nv > 4) store_group<false, 4>(p, at + 4, c + 4);
        }
        return;
    }
#pragma unroll
    for (int j = 0; j < 8; j++)
        if (j < nv) store_cell<BF16>(p, at + j, c[j]);
}

// TAPS = 9: the 3x3 convolution.  TAPS = 1: a 1x1 convolution as the centre tap of the same staged image; its halo slots are
// written as +0 without a read, so that nothing but the tile's own pixels is fetched.
// STRIDE = 2: see the head of the file.  S2 marks the 3x3 at stride 2, the one instance with a tile and a staged image of its own.
// DIL = 2, VOL: see the head of the file.
template <bool BF16, int EPI, int TAPS, int STRIDE = 1, int DIL = 1, bool VOL = false>
__global__ void __launch_bounds__(256, 2) raft_conv3x3_kernel(ConvArgs a)
{
    static_assert(TAPS == 9 || TAPS == 1, "3x3 or 1x1");
    static_assert(STRIDE == 1 || (STRIDE == 2 && EPI == CV_PLAIN), "stride 2 goes with the plain epilogue");
    static_assert(DIL == 1 || (DIL == 2 && TAPS == 9 && STRIDE == 1 && EPI == CV_PLAIN), "dilation 2 goes with nine taps, stride 1 and the plain epilogue");
    static_assert(!VOL || (TAPS == 9 && STRIDE == 1 && DIL == 1 && EPI == CV_PLAIN), "a volume goes with nine taps, stride 1, dilation 1 and the plain epilogue");
    constexpr int CK = BF16 ? 32 : 16;
    constexpr bool S2 = STRIDE == 2 && TAPS == 9, D2 = DIL == 2;
    constexpr int TH = S2 ? CV_TH2 : CV_TH, RPW = TH / 4, MT = 2 * RPW; // rows and M tiles of a wave
    constexpr int HW = S2 ? CV_HW2 : D2 ? CV_HWD : CV_HW, NPIX = S2 ? CV_HALO2 : D2 ? CV_HALOD : CV_HALO;
    constexpr int NFULL = NPIX / 256, REM = NPIX - 256 * NFULL;        // pixels a thread stages whole, and those shared out
    static_assert(D2 || (3 * REM <= 256 && REM > 0), "the pixels beyond the whole rounds are spread three units apart");
    constexpr int NB = D2 ? 16 * REM / 256 : 6;                        // units of the shared-out pixels a thread holds
    static_assert(!D2 || (16 * REM == 256 * NB && 16 * NFULL + NB == 27), "dilation 2: every thread stages the same 27 units");
    __shared__ __attribute__((aligned(16))) unsigned char sA[NPIX * CV_ROWB];

    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, g = lane >> 4, i = lane & 15;
    unsigned t = blockIdx.x;
    const int tx = (int)(t % (unsigned)a.tilesX);
    t /= (unsigned)a.tilesX;
    const int ty = (int)(t % (unsigned)a.tilesY);
    const size_t fr = t / (unsigned)a.tilesY;                          // the frame of the launch; VOL: plane d of batch frame b
    const int d = VOL ? (int)(fr % (unsigned)a.D) : 0;
    const size_t b = VOL ? fr / (unsigned)a.D : fr;
    const int x0 = tx * CV_TW, y0 = ty * TH, H = a.H, W = a.W;
    const int Hi = STRIDE == 1 ? H : a.Hi, Wi = STRIDE == 1 ? W : a.Wi;
    const size_t plane = (size_t)H * W, planeIn = STRIDE == 1 ? plane : (size_t)Hi * Wi;
    const size_t chan = VOL ? plane * (size_t)a.D : plane;             // cells between the channels of an epilogue tensor
    const int nb = blockIdx.y, ntl = min(4, a.NT - 4 * nb);

    // The staging.  A pixel's row of a chunk is 16 units of 4 bytes: one float32 channel, or two bfloat16 channels (an even
    // channel and the next lie in the same source, both below Cin or both not, because C0 and Cin are multiples of 16).
    // Thread tid stages all 16 units of pixel tid of the 340, and unit tid / 84 + 3 j of pixel 256 + tid % 84 (tid < 252), so
    // that the 84 pixels beyond the first 256 are spread over the workgroup: 22 units per thread, read into registers one
    // chunk ahead, while the matrix cores work on the chunk before.  (The 3x3 at stride 2: pixels tid and 256 + tid of the 585
    // whole, and the last 73 spread likewise: 38 units.)
    const int pB = 256 * NFULL + tid % REM, uB = tid / REM;
    // y * Wi + x of the input cell behind staged pixel p, -1 outside the map and for a slot that is written as +0 unread
    auto source = [&](int p) -> int {
        int gy, gx;
        bool in = true;
        if (S2) {
            const int r = p / HW, q = p - r * HW;
            gy = 2 * y0 - 1 + r, gx = q < CV_ODD2 ? 2 * (x0 + q) - 1 : 2 * (x0 + q - CV_ODD2);
        } else {
            const int ry = p / HW, rx = p - ry * HW;
            in = TAPS == 9 || (ry >= 1 && ry <= CV_TH && rx >= 1 && rx <= CV_TW);
            gy = STRIDE * (y0 + ry - DIL), gx = STRIDE * (x0 + rx - DIL);
        }
        return in && gy >= 0 && gy < Hi && gx >= 0 && gx < Wi ? gy * Wi + gx : -1;
    };
    int offA[NFULL], offB, offD[D2 ? NB : 1];
#pragma unroll
    for (int f = 0; f < NFULL; f++) offA[f] = source(tid + 256 * f);
    offB = !D2 && uB < 3 ? source(pB) : -1;
    if (D2) {
#pragma unroll
        for (int j = 0; j < NB; j++) offD[j] = source(256 * NFULL + (tid + 256 * j) % REM);
    }
    auto unit = [&](int chunk, int u, int off) -> u32 {
        const int c = chunk * CK + (BF16 ? 2 * u : u);
        if (off < 0 || c >= a.Cin) return 0u; // +0 outside the map and for the channels that pad K
        if (VOL) { // pseudo-channel c = dz * C0 + cc: plane d + dz - 1 of channel cc, +0 outside the volume and never of another frame
            const int dz = (c >= a.C0) + (c >= 2 * a.C0), z = d + dz - 1;
            if (z < 0 || z >= a.D) return 0u;
            const size_t at = b * (size_t)a.s0 + (size_t)(c - dz * a.C0) * chan + (size_t)z * plane + (size_t)off;
            if (BF16) {
                const u16 *p = (const u16 *)a.x0 + at;
                return (u32)p[0] | ((u32)p[chan] << 16);
            }
            return ((const u32 *)a.x0)[at];
        }
        const bool first = c < a.C0;
        const size_t at = (first ? b * (size_t)a.s0 + (size_t)c * planeIn : b * (size_t)a.s1 + (size_t)(c - a.C0) * planeIn) + (size_t)off;
        const void *src = first ? a.x0 : a.x1;
        if (BF16) {
            const u16 *p = (const u16 *)src + at;
            return (u32)p[0] | ((u32)p[planeIn] << 16);
        }
        return ((const u32 *)src)[at];
    };
    u32 stA[NFULL][16], stB[NB];
    auto fetch = [&](int chunk) {
#pragma unroll
        for (int f = 0; f < NFULL; f++)
#pragma unroll
            for (int u = 0; u < 16; u++) stA[f][u] = unit(chunk, u, offA[f]);
        if (D2) {
#pragma unroll
            for (int j = 0; j < NB; j++) stB[j] = unit(chunk, (tid + 256 * j) / REM, offD[D2 ? j : 0]);
        } else {
#pragma unroll
            for (int j = 0; j < NB; j++) stB[j] = uB + 3 * j < 16 ? unit(chunk, uB + 3 * j, offB) : 0u;
        }
    };
    fetch(0);

    cv_f32x4 acc[MT][4];
#pragma unroll
    for (int m = 0; m < MT; m++)
#pragma unroll
        for (int n = 0; n < 4; n++) acc[m][n] = (cv_f32x4){0.0f, 0.0f, 0.0f, 0.0f};

    // byte offset of this lane's A fragment of M tile m = 2 * p + t at tap (0, 0); S2: output row `wave` is staged row 2 * wave
    int la[MT];
#pragma unroll
    for (int m = 0; m < MT; m++)
        la[m] = ((S2 ? 2 * wave : 2 * wave + (m >> 1)) * HW + 8 * (i >> 2) + 4 * (m & 1) + (i & 3)) * CV_ROWB + 16 * g;

    const uint4 *pk = a.packed + (size_t)(4 * nb) * 64 + lane;
    const size_t step = (size_t)a.NT * 64; // fragments of one (chunk, tap)
    const int nsteps = a.nchunks * TAPS;
    uint4 bcur[4], bnext[4];
#pragma unroll
    for (int n = 0; n < 4; n++) bcur[n] = n < ntl ? pk[64 * n] : make_uint4(0, 0, 0, 0);

    for (int chunk = 0; chunk < a.nchunks; chunk++) {
        __syncthreads(); // the last chunk's fragments have been read
#pragma unroll
        for (int f = 0; f < NFULL; f++)
#pragma unroll
            for (int k = 0; k < 4; k++)
                *(uint4 *)(sA + (tid + 256 * f) * CV_ROWB + 16 * k) = make_uint4(stA[f][4 * k], stA[f][4 * k + 1], stA[f][4 * k + 2], stA[f][4 * k + 3]);
        if (D2) {
#pragma unroll
            for (int j = 0; j < NB; j++)
                *(u32 *)(sA + (256 * NFULL + (tid + 256 * j) % REM) * CV_ROWB + 4 * ((tid + 256 * j) / REM)) = stB[j];
        } else if (uB < 3) {
#pragma unroll
            for (int j = 0; j < NB; j++)
                if (uB + 3 * j < 16) *(u32 *)(sA + pB * CV_ROWB + 4 * (uB + 3 * j)) = stB[j];
        }
        __syncthreads();
        if (chunk + 1 < a.nchunks) fetch(chunk + 1); // in flight during this chunk's matrix instructions
#pragma unroll
        for (int tap = 0; tap < TAPS; tap++) {
            const int s = chunk * TAPS + tap;
            if (s + 1 < nsteps) {
#pragma unroll
                for (int n = 0; n < 4; n++)
                    if (n < ntl) bnext[n] = pk[(size_t)(s + 1) * step + 64 * n];
            }
            // S2: columns 2x - 1 and 2x + 1 are slots x and x + 1 of the odd part, column 2x slot x of the even part behind it
            const int toff = (S2 ? (tap / 3) * HW + (tap % 3 == 1 ? CV_ODD2 : tap % 3 / 2) : TAPS == 9 ? DIL * ((tap / 3) * HW + tap % 3) : CV_HW + 1) * CV_ROWB;
            uint4 fa[MT];
#pragma unroll
            for (int m = 0; m < MT; m++) fa[m] = *(const uint4 *)(sA + la[m] + toff);
            if (BF16) {
#pragma unroll
                for (int n = 0; n < 4; n++) {
                    if (n >= ntl) break;
#pragma unroll
                    for (int m = 0; m < MT; m++)
                        acc[m][n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(cv_bf16x8, fa[m]),
                                                                            __builtin_bit_cast(cv_bf16x8, bcur[n]), acc[m][n], 0, 0, 0);
                }
            } else {
                // the k-step outermost: consecutive instructions then work on different accumulators
#pragma unroll
                for (int k = 0; k < 4; k++) {
#pragma unroll
                    for (int n = 0; n < 4; n++) {
                        if (n >= ntl) break;
#pragma unroll
                        for (int m = 0; m < MT; m++)
                            acc[m][n] = __builtin_amdgcn_mfma_f32_16x16x4f32(__builtin_bit_cast(cv_f32x4, fa[m])[k],
                                                                             __builtin_bit_cast(cv_f32x4, bcur[n])[k], acc[m][n], 0, 0, 0);
                    }
                }
            }
#pragma unroll
            for (int n = 0; n < 4; n++) bcur[n] = bnext[n];
        }
    }

    // the epilogue: per row of the wave and N tile, eight consecutive pixels of one channel
    const bool vec = a.vec != 0;
    const int x = x0 + 8 * g, nv = min(8, W - x);
    if (nv <= 0) return;
#pragma unroll
    for (int p = 0; p < RPW; p++) {
        const int y = y0 + RPW * wave + p;
        if (y >= H) break;
        const size_t pix = (VOL ? (size_t)d * plane : 0) + (size_t)y * W + x;
#pragma unroll
        for (int n = 0; n < 4; n++) {
            if (n >= ntl) break;
            const int m = 64 * nb + 16 * n + i;
            const float bias = a.bias[m]; // m < 16 * NT: a padding channel reads the +0 the packing wrote
            if (EPI == CV_PLAIN && m >= a.Cout) continue; // per lane: neither the 16-byte route nor the cell route stores it
            float v[8], o[8];
#pragma unroll
            for (int j = 0; j < 8; j++) v[j] = __fadd_rn(acc[2 * p + (j >> 2)][n][j & 3], bias);
            if (EPI == CV_PLAIN) {
                if (a.res) { // uniform over the launch; out may be the residual: read before the store
                    float r[8];
                    cv_load8<BF16>(a.e0, b * (size_t)a.se0 + (size_t)m * chan + pix, nv, vec, r);
#pragma unroll
                    for (int j = 0; j < 8; j++) v[j] = __fadd_rn(v[j], r[j]);
                }
#pragma unroll
                for (int j = 0; j < 8; j++) o[j] = __fmul_rn(a.relu ? relu_nan(v[j]) : v[j], a.scale);
                cv_store8<BF16>(a.o0, b * (size_t)a.so0 + (size_t)m * chan + pix, nv, vec, o);
            } else if (EPI == CV_ZR) {
                float c[8];
                if (m < a.C) { // uniform over the N tile: C is a multiple of 16
                    cv_load8<BF16>(a.e0, b * (size_t)a.se0 + (size_t)m * chan + pix, nv, vec, c);
#pragma unroll
                    for (int j = 0; j < 8; j++) o[j] = gru_sigmoid(__fadd_rn(v[j], c[j]));
                    cv_store8<BF16>(a.o0, b * (size_t)a.so0 + (size_t)m * chan + pix, nv, vec, o);
                } else {
                    const size_t mm = (size_t)(m - a.C);
                    float hh[8];
                    cv_load8<BF16>(a.e1, b * (size_t)a.se1 + mm * chan + pix, nv, vec, c);
                    cv_load8<BF16>(a.e2, b * (size_t)a.se2 + mm * chan + pix, nv, vec, hh);
#pragma unroll
                    for (int j = 0; j < 8; j++) o[j] = __fmul_rn(gru_sigmoid(__fadd_rn(v[j], c[j])), hh[j]);
                    cv_store8<BF16>(a.o1, b * (size_t)a.so1 + mm * chan + pix, nv, vec, o);
                }
            } else {
                float c[8], z[8], hh[8];
                cv_load8<BF16>(a.e0, b * (size_t)a.se0 + (size_t)m * chan + pix, nv, vec, c);
                cv_load8<BF16>(a.e1, b * (size_t)a.se1 + (size_t)m * chan + pix, nv, vec, z);
                cv_load8<BF16>(a.e2, b * (size_t)a.se2 + (size_t)m * chan + pix, nv, vec, hh); // out may be h: read before the store
#pragma unroll
                for (int j = 0; j < 8; j++) o[j] = gru_mix(z[j], gru_tanh(__fadd_rn(v[j], c[j])), hh[j]);
                cv_store8<BF16>(a.o0, b * (size_t)a.so0 + (size_t)m * chan + pix, nv, vec, o);
            }
        }
    }
}

// ---------------------------------------------------------------------------------------
// the packing: torch's [Cout][Cin][k][k] float32 (taps = k * k) -> fragment order, input channels beyond Cin and output
// channels beyond Cout as +0, the bias behind: NT * 16 slots, +0 beyond Cout.  Every fragment and slot is written.
// ---------------------------------------------------------------------------------------
// fragment f = ((chunk * taps + tap) * NT + N tile) * 64 + lane holds, for lane = 16 g + i, output channel 16 * tile + i and
//   bfloat16: element j = input channel 32 * chunk + 8 g + j          (the 16x16x32 B map: k = 8 (lane >> 4) + j)
//   float32:  element j = input channel 16 * chunk + 4 g + j          (k-step j of the chunk, 16x16x4 B map: k = lane >> 4)
// VOL: w is [Cout][Cin / 3][3][3][3] and channel c of the packed layout is pseudo-channel dz * (Cin / 3) + cc (the head of the file).
template <bool BF16, bool VOL = false>
__global__ void __launch_bounds__(256) raft_conv3x3_pack_kernel(const float *w, const float *bias, int Cout, int Cin, int nchunks, int taps, void *packed)
{
    constexpr int E = BF16 ? 8 : 4, CK = BF16 ? 32 : 16;
    const int NT = (Cout + 15) / 16;
    const size_t nfrag = (size_t)nchunks * taps * NT * 64;
    const size_t f = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (f < (size_t)NT * 16) ((float *)((uint4 *)packed + nfrag))[f] = bias && f < (size_t)Cout ? bias[f] : 0.0f; // nfrag >= 64 NT
    if (f >= nfrag) return;
    const int lane = (int)(f & 63), g = lane >> 4, i = lane & 15;
    size_t r = f >> 6;
    const int tile = (int)(r % NT);
    r /= NT;
    const int tap = (int)(r % taps), chunk = (int)(r / taps);
    const int m = 16 * tile + i;
    float v[E];
#pragma unroll
    for (int j = 0; j < E; j++) {
        const int c = CK * chunk + E * g + j;
        if (VOL) {
            const int C3 = Cin / 3, dz = c / C3, cc = c - dz * C3;
            v[j] = c < Cin && m < Cout ? w[(((size_t)m * C3 + cc) * 3 + dz) * taps + tap] : 0.0f;
        } else {
            v[j] = c < Cin && m < Cout ? w[((size_t)m * Cin + c) * taps + tap] : 0.0f;
        }
    }
    if (BF16) {
        u32 h[8];
#pragma unroll
        for (int j = 0; j < E; j++) h[j] = bf16_rne(v[j]);
        ((uint4 *)packed)[f] = make_uint4(h[0] | (h[1] << 16), h[2] | (h[3] << 16), h[4 % E] | (h[5 % E] << 16), h[6 % E] | (h[7 % E] << 16));
    } else {
        ((float4 *)packed)[f] = make_float4(v[0], v[1], v[2], v[3]);
    }
}

// ---------------------------------------------------------------------------------------
// launchers (every argument has been checked by vppx_net_api.hip)
// ---------------------------------------------------------------------------------------
static int conv_chunks(int Cin, int dtype) { return dtype == VPPX_DT_BF16 ? (Cin + 31) / 32 : (Cin + 15) / 16; }

static int conv_ntiles(int Cout) { return (Cout + 15) / 16; }

static size_t conv_weight_bytes(int Cout, int Cin, int ksize, int dtype)
{
    return (size_t)conv_chunks(Cin, dtype) * (ksize * ksize) * conv_ntiles(Cout) * 64 * 16;
}

// the fragments and one bias slot per PADDED output channel: for Cout % 16 == 0 what it has always been
size_t conv_packed_bytes(int Cout, int Cin, int ksize, int dtype)
{
    return conv_weight_bytes(Cout, Cin, ksize, dtype) + (size_t)conv_ntiles(Cout) * 16 * sizeof(float);
}

// vol: weight is [Cout][Cin][3][3][3], packed as the [Cout][3 Cin][3][3] weight of the pseudo-channels
int conv_pack(vppx_ctx *ctx, const float *weight, const float *bias, int Cout, int Cin, int ksize, int dtype, void *packed, bool vol)
{
    if (vol) Cin *= 3;
    const int nchunks = conv_chunks(Cin, dtype), taps = ksize * ksize;
    const size_t nfrag = (size_t)nchunks * taps * conv_ntiles(Cout) * 64;
    const unsigned blocks = (unsigned)((nfrag + 255) / 256);
    if (vol && dtype == VPPX_DT_BF16)
        raft_conv3x3_pack_kernel<true, true><<<dim3(blocks), 256, 0, ctx->stream>>>(weight, bias, Cout, Cin, nchunks, taps, packed);
    else if (vol)
        raft_conv3x3_pack_kernel<false, true><<<dim3(blocks), 256, 0, ctx->stream>>>(weight, bias, Cout, Cin, nchunks, taps, packed);
    else if (dtype == VPPX_DT_BF16)
        raft_conv3x3_pack_kernel<true><<<dim3(blocks), 256, 0, ctx->stream>>>(weight, bias, Cout, Cin, nchunks, taps, packed);
    else
        raft_conv3x3_pack_kernel<false><<<dim3(blocks), 256, 0, ctx->stream>>>(weight, bias, Cout, Cin, nchunks, taps, packed);
    VPPX_CHECK_LAUNCH();
    return 0;
}

// one launch per (epilogue, taps, stride, dilation) that is built: ksize 1, stride 2, dilation 2 and a Cout that is no multiple
// of 16 go with the plain epilogue only, dilation 2 with stride 1; a 1x1 at dilation 2 is the 1x1 itself (vppx_net_api.hip sees to it);
// a volume is 3x3x3 at stride 1, dilation 1
template <bool BF16>
static void conv_launch(vppx_ctx *ctx, const ConvCall &c, const ConvArgs &a, dim3 grid)
{
    if (c.vol) raft_conv3x3_kernel<BF16, CV_PLAIN, 9, 1, 1, true><<<grid, 256, 0, ctx->stream>>>(a);
    else if (c.epi == CV_PLAIN && c.stride == 2 && c.ksize == 1) raft_conv3x3_kernel<BF16, CV_PLAIN, 1, 2><<<grid, 256, 0, ctx->stream>>>(a);
    else if (c.epi == CV_PLAIN && c.stride == 2) raft_conv3x3_kernel<BF16, CV_PLAIN, 9, 2><<<grid, 256, 0, ctx->stream>>>(a);
    else if (c.epi == CV_PLAIN && c.ksize == 3 && c.dilation == 2) raft_conv3x3_kernel<BF16, CV_PLAIN, 9, 1, 2><<<grid, 256, 0, ctx->stream>>>(a);
    else if (c.epi == CV_PLAIN && c.ksize == 1) raft_conv3x3_kernel<BF16, CV_PLAIN, 1><<<grid, 256, 0, ctx->stream>>>(a);
    else if (c.epi == CV_PLAIN) raft_conv3x3_kernel<BF16, CV_PLAIN, 9><<<grid, 256, 0, ctx->stream>>>(a);
    else if (c.epi == CV_ZR) raft_conv3x3_kernel<BF16, CV_ZR, 9><<<grid, 256, 0, ctx->stream>>>(a);
    else raft_conv3x3_kernel<BF16, CV_Q, 9><<<grid, 256, 0, ctx->stream>>>(a);
}

int conv_run(vppx_ctx *ctx, const char *who, const ConvCall &c)
{
    const bool bf16 = c.dtype == VPPX_DT_BF16;
    ConvArgs a = {};
    a.x0 = c.x0, a.x1 = c.C1 ? c.x1 : c.x0, a.s0 = (long long)c.s0, a.s1 = c.C1 ? (long long)c.s1 : 0;
    a.C0 = c.C0, a.Cin = c.vol ? 3 * c.C0 : c.C0 + c.C1, a.D = c.vol ? c.D : 1, a.NT = conv_ntiles(c.Cout), a.nchunks = conv_chunks(a.Cin, c.dtype);
    a.Cout = c.Cout, a.scale = c.scale;
    a.packed = (const uint4 *)c.packed;
    a.bias = (const float *)((const unsigned char *)c.packed + conv_weight_bytes(c.Cout, a.Cin, c.ksize, c.dtype));
    a.e0 = c.in[0].p, a.e1 = c.in[1].p, a.e2 = c.in[2].p;
    a.se0 = (long long)c.in[0].stride, a.se1 = (long long)c.in[1].stride, a.se2 = (long long)c.in[2].stride;
    a.o0 = (void *)c.out[0].p, a.o1 = (void *)c.out[1].p, a.so0 = (long long)c.out[0].stride, a.so1 = (long long)c.out[1].stride;
    const int Ho = (c.H - 1) / c.stride + 1, Wo = (c.W - 1) / c.stride + 1, th = c.stride == 2 && c.ksize == 3 ? CV_TH2 : CV_TH;
    a.H = Ho, a.W = Wo, a.Hi = c.H, a.Wi = c.W, a.tilesX = (Wo + CV_TW - 1) / CV_TW, a.tilesY = (Ho + th - 1) / th;
    a.C = c.C, a.relu = c.relu, a.res = c.epi == CV_PLAIN && c.in[0].p != NULL;
    const size_t tiles = (size_t)c.B * a.D * a.tilesX * a.tilesY;
    if (tiles > 0x7FFFFFFFull) {
        vppx_set_error("%s: %lld frames of %dx%d are %zu workgroups, more than one launch takes", who, (long long)c.B * a.D, Ho, Wo, tiles);
        return VPPX_E_UNSUPPORTED;
    }
    const int64_t V = bf16 ? 8 : 4;
    bool vec = Wo % V == 0; // then Ho * Wo is a whole number of groups as well
    for (const ConvTensor &t : c.in)
        if (t.p) vec = vec && aligned16(t.p) && t.stride % V == 0;
    for (const ConvTensor &t : c.out)
        if (t.p) vec = vec && aligned16(t.p) && t.stride % V == 0;
    a.vec = vec;
    const dim3 grid((unsigned)tiles, (unsigned)((a.NT + 3) / 4));
    if (bf16) conv_launch<true>(ctx, c, a, grid);
    else conv_launch<false>(ctx, c, a, grid);
    VPPX_CHECK_LAUNCH();
    return 0;
}
