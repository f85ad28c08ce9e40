// cells.h -- how the network-glue kernels keep a cell: float32, or bfloat16 widened on load and rounded once on store, the
// arithmetic in between float32.  Device code; only the kernel files that move such cells include it.
#pragma once
#include "vppx_internal.h"

typedef u16 u16x8 __attribute__((ext_vector_type(8)));

__device__ __forceinline__ float bf16_widen(u32 bits) { return __uint_as_float(bits << 16); }

// round-to-nearest-even; NaN stays NaN (quieted, sign and upper payload kept), beyond the largest bf16 -> infinity
__device__ __forceinline__ u32 bf16_rne(float f)
{
    const u32 u = __float_as_uint(f);
    if ((u & 0x7FFFFFFFu) > 0x7F800000u) return (u >> 16) | 0x0040u;
    return (u + 0x7FFFu + ((u >> 16) & 1u)) >> 16;
}

__device__ __forceinline__ u32 bf16_scale(u32 bits, float mod) { return bf16_rne(__fmul_rn(bf16_widen(bits), mod)); }

// relu as torch's: a NaN stays NaN
__device__ __forceinline__ float relu_nan(float v) { return v < 0.0f ? 0.0f : v; }

// N cells from cell `at` of p on, widened; VEC: as 16-byte loads of 4 float32 or 8 bfloat16 cells (the caller has checked
// the alignment, and N is a whole number of them)
template <bool BF16, bool VEC, int N>
__device__ __forceinline__ void load_cells(const void *p, size_t at, float *c)
{
    if (BF16) {
        const u16 *q = (const u16 *)p + at;
        if (VEC) {
#pragma unroll
            for (int g = 0; g < N / 8; g++) {
                const u16x8 v = *(const u16x8 *)(q + 8 * g);
#pragma unroll
                for (int j = 0; j < 8; j++) c[8 * g + j] = bf16_widen(v[j]);
            }
        } else {
#pragma unroll
            for (int j = 0; j < N; j++) c[j] = bf16_widen(q[j]);
        }
    } else {
        const float *q = (const float *)p + at;
        if (VEC) {
#pragma unroll
            for (int g = 0; g < N / 4; g++) {
                const float4 v = *(const float4 *)(q + 4 * g);
                c[4 * g] = v.x, c[4 * g + 1] = v.y, c[4 * g + 2] = v.z, c[4 * g + 3] = v.w;
            }
        } else {
#pragma unroll
            for (int j = 0; j < N; j++) c[j] = q[j];
        }
    }
}

// V cells to cell `at` of p on, rounded; one 16-byte store where V is a whole vector (8 bfloat16, 4 float32)
template <bool BF16, int V>
__device__ __forceinline__ void store_group(void *p, size_t at, const float *c)
{
    if (BF16) {
        u16 *q = (u16 *)p + at;
        if (V == 8) {
            u16x8 v;
#pragma unroll
            for (int j = 0; j < 8; j++) v[j] = (u16)bf16_rne(c[j]);
            *(u16x8 *)q = v;
        } else {
#pragma unroll
            for (int j = 0; j < V; j++) q[j] = (u16)bf16_rne(c[j]);
        }
    } else {
        float *q = (float *)p + at;
        if (V == 4) {
            *(float4 *)q = make_float4(c[0], c[1], c[2], c[3]);
        } else {
#pragma unroll
            for (int j = 0; j < V; j++) q[j] = c[j];
        }
    }
}

template <bool BF16>
__device__ __forceinline__ float load_cell(const void *p, size_t i)
{
    return BF16 ? bf16_widen(((const u16 *)p)[i]) : ((const float *)p)[i];
}

template <bool BF16>
__device__ __forceinline__ void store_cell(void *p, size_t i, float v)
{
    if (BF16)
        ((u16 *)p)[i] = (u16)bf16_rne(v);
    else
        ((float *)p)[i] = v;
}

// ---------------------------------------------------------------------------------------
// host side: which of the four instances a launcher starts
// ---------------------------------------------------------------------------------------
static inline bool aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }

// LAUNCH(BF16, V) is the launch with its two template arguments open: V is 8 (bfloat16) or 4 (float32) cells per lane where
// `vec` says that every base is 16-byte aligned and every stride a multiple of V, else 1
#define CELLS_LAUNCH(bf16, vec, LAUNCH) \
    do {                                \
        if ((bf16) && (vec))            \
            LAUNCH(true, 8);            \
        else if (bf16)                  \
            LAUNCH(true, 1);            \
        else if (vec)                   \
            LAUNCH(false, 4);           \
        else                            \
            LAUNCH(false, 1);           \
    } while (0)
