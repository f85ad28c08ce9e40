// sample_kernels.hip -- gfx950 kernel of losses.sample_hints (losses.py:5-10, test.py:125-129) for a batch, bit-exact with
// torch's CPU generator: frame f equals torch.manual_seed(seed + f); sample_hints(src, validsrc > 0, p).
//
// torch.rand_like(float32) on the CPU draws one tempered MT19937 word y per element in row-major order and keeps
// k = y & 0xFFFFFF; rand < p is k < T with T = clamp(ceil(double(float(p)) * 2^24), 0, 2^24) (computed on the host).  So
//   sel_j = validsrc_j > 0 && k_j < T;   hints_j = sel_j ? src_j : +0.0f;   validhints_j = sel_j ? 1.0f : 0.0f.
//
// The generator is the serial part: x[n] = x[n-227] ^ twist(x[n-624], x[n-623]), so at most 227 new words exist per dependent
// step.  One block per frame: wave 0 walks the recurrence in steps of SM_STEP = 224 words, 56 lanes with four consecutive
// words each, into a ring of raw words in LDS.  Word n - 227 is word 4 * lane - 3 of the step before: three words of the lane
// below and the lane's own, so the chain runs through registers (a DPP wavefront shift, one three-way XOR); the old words x[n-624 ..
// n-620] come from the ring, loaded two steps ahead, and the store into the ring is for later steps and the other waves only.
// No wait sits in the loop: the LDS serves one wave's operations in order.  The other SM_CONSUMERS waves temper, threshold and
// apply the PREVIOUS chunk of SM_CHUNK words meanwhile: 16 bytes per lane of src and validsrc in (fetched one chunk ahead),
// 16 bytes per lane of hints and validhints out.  One __syncthreads() per chunk hands a chunk over.  No atomics, no waiting
// on another block, no polling: every loop has a trip count fixed by the frame's shape.
#include "vppx_internal.h"

#define SM_THREADS 1024
#define SM_CONSUMERS (SM_THREADS / 64 - 1)
#define SM_STEP 224               // words per dependent step: a multiple of 4, at most 227
#define SM_STEPS_PER_CHUNK 16      // even: the walk makes two steps per trip
#define SM_CHUNK (SM_STEP * SM_STEPS_PER_CHUNK) // 3584 words: at most one quad per consumer lane (15 * 64 * 4 = 3840)
#define SM_RING 8192              // words; >= 2 * SM_CHUNK, a power of two
#define SM_N 624
#define SM_M 397
static_assert(SM_CHUNK <= SM_CONSUMERS * 64 * 4, "one quad per consumer lane");
static_assert(2 * SM_CHUNK + 32 <= SM_RING && SM_CHUNK >= SM_N, "the ring holds the chunk being written, the one being read and the state");
static_assert(SM_STEP % 4 == 0 && SM_STEP <= SM_N - SM_M, "step");

// what one wave wrote to LDS is visible to its other lanes: LDS operations of a wave complete in order, the fences keep the
// compiler from moving accesses across
static __device__ __forceinline__ void sm_wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// a compiler-only barrier for the walking wave's own LDS traffic (no wait: the LDS serves a wave's operations in order)
static __device__ __forceinline__ void sm_order() { asm volatile("" ::: "memory"); }

// lane L gets lane L - 1's `cur` (a DPP wavefront shift: no LDS, a few cycles); lane 0 gets lane 55's `before`
static __device__ __forceinline__ u32 sm_from_lane_below(u32 cur, u32 before)
{
    const u32 edge = (u32)__builtin_amdgcn_readlane((int)before, SM_STEP / 4 - 1);
    return (u32)__builtin_amdgcn_update_dpp((int)edge, (int)cur, 0x138 /* wave_shr:1 */, 0xf, 0xf, false);
}

// The walk is bound by the one wave's instruction count, so its step is spelled in the instructions it should be: the compiler
// expands the bit-field insert and the three-way XOR into five and two operations, and the signed extract into three.
static __device__ __forceinline__ u32 sm_bfi(u32 mask, u32 x, u32 y) // (mask & x) | (~mask & y)
{
    u32 r;
    asm("v_bfi_b32 %0, %1, %2, %3" : "=v"(r) : "v"(mask), "v"(x), "v"(y));
    return r;
}
static __device__ __forceinline__ u32 sm_xor3(u32 x, u32 y, u32 z)
{
    u32 r;
    asm("v_bitop3_b32 %0, %1, %2, %3 bitop3:0x96" : "=v"(r) : "v"(x), "v"(y), "v"(z));
    return r;
}
static __device__ __forceinline__ u32 sm_bit0_mask(u32 x) // x & 1 ? 0xffffffff : 0
{
    u32 r;
    asm("v_bfe_i32 %0, %1, 0, 1" : "=v"(r) : "v"(x));
    return r;
}

// y = (a & 0x80000000) | (b & 0x7fffffff); m ^ (y >> 1) ^ (y & 1 ? 0x9908b0df : 0).  a1, b1: a >> 1, b >> 1 (a quad shares them)
static __device__ __forceinline__ u32 sm_twist(u32 a1, u32 b1, u32 b, u32 m)
{
    return sm_xor3(m, sm_bfi(0x3fffffffu, b1, a1), sm_bit0_mask(b) & 0x9908b0dfu);
}

static __device__ __forceinline__ u32 sm_temper24(u32 y)
{
    y ^= y >> 11;
    y ^= (y << 7) & 0x9d2c5680u;
    y ^= (y << 15) & 0xefc60000u;
    y ^= y >> 18;
    return y & 0xFFFFFFu;
}

// One step of the walk at word n = step start + 4 * lane.  (a, a4): x[n-624 .. n-620], loaded two steps ago; prev: this lane's
// quad of the last step, before: of the step before it, which receives this step's quad.
static __device__ __forceinline__ void sm_step(u32 *ring, unsigned n, uint4 &a, u32 &a4, const uint4 &prev, uint4 &before)
{
    // x[n - 227 + i] = word 4 * lane - 3 + i of the last step: three words of the lane below (of lane 55 two steps back, for
    // lane 0) and this lane's own first.  They come through registers: this is the dependency chain.
    uint4 o;
    const u32 s0 = a.x >> 1, s1 = a.y >> 1, s2 = a.z >> 1, s3 = a.w >> 1, s4 = a4 >> 1;
    o.x = sm_twist(s0, s1, a.y, sm_from_lane_below(prev.y, before.y));
    o.y = sm_twist(s1, s2, a.z, sm_from_lane_below(prev.z, before.z));
    o.z = sm_twist(s2, s3, a.w, sm_from_lane_below(prev.w, before.w));
    o.w = sm_twist(s3, s4, a4, prev.x);
    // All 64 lanes store (no branch in the walk): lanes 56 .. 63 put 32 meaningless words where the NEXT step's first words go,
    // which that step's own store -- later in the same in-order queue -- replaces before anything reads them.  (Behind a chunk's
    // last step they fall on the first words of the chunk after it, which the walk writes next; SM_RING - 2 * SM_CHUNK >= 32
    // keeps them off the chunk the other waves are reading.)
    *(uint4 *)&ring[n & (SM_RING - 1)] = o;
    before = o;
    sm_order(); // the loads below stay behind this store
    // The old words of the step after the next (624 .. 620 back from it: the youngest is word 51 of THIS step, stored just now,
    // and the LDS serves one wave's operations in order): two steps ahead, their latency is off the chain.
    const unsigned nn = n + 2 * SM_STEP;
    a = *(const uint4 *)&ring[4 * (((nn - SM_N) >> 2) & (SM_RING / 4 - 1))];
    a4 = ring[(nn - SM_N + 4) & (SM_RING - 1)];
    sm_order();
}

// grid (B); word n of the ring is output n of the stream (pixel n), at ring[n & (SM_RING - 1)]; the seeded state is words
// -624 .. -1.  VEC: a frame's pixel count is a multiple of 4 and all planes start 16-byte aligned.
template <typename VT> struct SmValid;
template <> struct SmValid<float> {
    static __device__ __forceinline__ void load4(const float *p, bool *v)
    {
        const float4 q = *(const float4 *)p;
        v[0] = q.x > 0.f; v[1] = q.y > 0.f; v[2] = q.z > 0.f; v[3] = q.w > 0.f;
    }
};
template <> struct SmValid<u8> {
    static __device__ __forceinline__ void load4(const u8 *p, bool *v)
    {
        const uchar4 q = *(const uchar4 *)p;
        v[0] = q.x > 0; v[1] = q.y > 0; v[2] = q.z > 0; v[3] = q.w > 0;
    }
};

template <typename VT, bool VEC>
__global__ void __launch_bounds__(SM_THREADS) sample_hints_kernel(const float *__restrict__ src, const VT *__restrict__ vsrc,
                                                                  float *__restrict__ hints, float *__restrict__ vhints,
                                                                  const u32 *__restrict__ seeds_dev, u32 seed, u32 T, unsigned npx)
{
    __shared__ __attribute__((aligned(16))) u32 ring[SM_RING];
    const int f = blockIdx.x;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const size_t base = (size_t)f * npx;
    src += base;
    vsrc += base;
    hints += base;
    if (vhints) vhints += base;
    const unsigned nchunks = (npx + SM_CHUNK - 1) / SM_CHUNK;

    if (wave == 0) { // init_genrand(seed): mt[i] = 1812433253 * (mt[i-1] ^ (mt[i-1] >> 30)) + i
        if (lane == 0) {
            u32 x = seeds_dev ? seeds_dev[f] : seed + (u32)f;
            ring[SM_RING - SM_N] = x;
            for (u32 i = 1; i < SM_N; i++) {
                x = 1812433253u * (x ^ (x >> 30)) + i;
                ring[SM_RING - SM_N + i] = x;
            }
        }
        sm_wave_sync();
    }
    // the walk's registers (wave 0): the quads this lane made in the last two steps, and the old state words of the step to come
    uint4 p1 = make_uint4(0, 0, 0, 0), p0 = p1, a = p1, b = p1;
    u32 a4 = 0, b4 = 0;
    if (wave == 0) {
        p1 = *(const uint4 *)&ring[(SM_RING - SM_STEP + 4 * lane) & (SM_RING - 1)];      // the step "before" step 0: x[-224 ..]
        p0 = *(const uint4 *)&ring[(SM_RING - 2 * SM_STEP + 4 * lane) & (SM_RING - 1)];  // and the one before that
        a = *(const uint4 *)&ring[4 * (((4u * lane - SM_N) >> 2) & (SM_RING / 4 - 1))];
        a4 = ring[(4u * lane - SM_N + 4) & (SM_RING - 1)];
        b = *(const uint4 *)&ring[4 * (((4u * lane + SM_STEP - SM_N) >> 2) & (SM_RING / 4 - 1))];
        b4 = ring[(4u * lane + SM_STEP - SM_N + 4) & (SM_RING - 1)];
    }
    // the consumers' registers: src and validsrc of the chunk they apply next, fetched one chunk ahead
    float4 sv = make_float4(0.f, 0.f, 0.f, 0.f);
    bool v[4] = {false, false, false, false};
    const unsigned q = (unsigned)(wave - 1) * 64 + lane;
    for (unsigned c = 0; c <= nchunks; c++) {
        if (wave == 0) {
            if (c < nchunks) { // the walk: chunk c
                const unsigned n_lo = c * SM_CHUNK;
                const unsigned left = npx - n_lo;
                const unsigned steps = left >= SM_CHUNK ? SM_STEPS_PER_CHUNK : (left + SM_STEP - 1) / SM_STEP;
                // Two steps per trip, so that the registers alternate without copies: the even step takes its old words from (a, a4)
                // and leaves its quad in p0, the odd one from (b, b4) into p1.  (An odd count of steps makes one step more than
                // needed: words of this chunk's own part of the ring that nobody reads.)
                // A whole chunk is straight-line code: the compiler then waits for exactly the loads a step consumes (issued two steps
                // earlier) and for nothing younger; around a loop's back edge it drains the LDS queue.
                if (left >= SM_CHUNK) {
#pragma unroll
                    for (unsigned s = 0; s < SM_STEPS_PER_CHUNK; s += 2) {
                        const unsigned n = n_lo + s * SM_STEP + 4 * lane; // a multiple of 4: the quads never wrap inside
                        sm_step(ring, n, a, a4, p1, p0);
                        sm_step(ring, n + SM_STEP, b, b4, p0, p1);
                    }
                } else {
#pragma unroll 1
                    for (unsigned s = 0; s < steps; s += 2) {
                        const unsigned n = n_lo + s * SM_STEP + 4 * lane;
                        sm_step(ring, n, a, a4, p1, p0);
                        sm_step(ring, n + SM_STEP, b, b4, p0, p1);
                    }
                }
            }
        } else {
            if (c >= 1) { // everything else, wide: chunk c - 1
                const unsigned n = (c - 1) * SM_CHUNK + 4 * q;
                if (4 * q < SM_CHUNK && n < npx) {
                    const uint4 raw = *(const uint4 *)&ring[n & (SM_RING - 1)];
                    const u32 k[4] = {sm_temper24(raw.x), sm_temper24(raw.y), sm_temper24(raw.z), sm_temper24(raw.w)};
                    if (VEC) { // (npx % 4 == 0: the quad is whole)
                        const bool s0 = v[0] && k[0] < T, s1 = v[1] && k[1] < T, s2 = v[2] && k[2] < T, s3 = v[3] && k[3] < T;
                        *(float4 *)(hints + n) = make_float4(s0 ? sv.x : 0.f, s1 ? sv.y : 0.f, s2 ? sv.z : 0.f, s3 ? sv.w : 0.f);
                        if (vhints) *(float4 *)(vhints + n) = make_float4(s0 ? 1.f : 0.f, s1 ? 1.f : 0.f, s2 ? 1.f : 0.f, s3 ? 1.f : 0.f);
                    } else {
                        const unsigned m = npx - n < 4 ? npx - n : 4;
#pragma unroll
                        for (unsigned i = 0; i < 4; i++) {
                            if (i < m) {
                                const bool s = vsrc[n + i] > 0 && k[i] < T;
                                hints[n + i] = s ? src[n + i] : 0.f;
                                if (vhints) vhints[n + i] = s ? 1.f : 0.f;
                            }
                        }
                    }
                }
            }
            if (VEC && c < nchunks) { // the inputs of chunk c, which the next trip applies: their latency lies under the walk of chunk c
                const unsigned n = c * SM_CHUNK + 4 * q;
                if (4 * q < SM_CHUNK && n < npx) {
                    sv = *(const float4 *)(src + n);
                    SmValid<VT>::load4(vsrc + n, v);
                }
            }
        }
        __syncthreads();
    }
}

template <typename VT>
static int launch_t(vppx_ctx *ctx, int B, size_t npx, const float *src, const VT *vsrc, float *hints, float *vhints, const u32 *seeds_dev,
                    u32 seed, u32 T)
{
    const bool vec = npx % 4 == 0 && ((uintptr_t)src & 15) == 0 && ((uintptr_t)vsrc & (4 * sizeof(VT) - 1)) == 0 &&
                     ((uintptr_t)hints & 15) == 0 && (!vhints || ((uintptr_t)vhints & 15) == 0);
    if (vec) sample_hints_kernel<VT, true><<<B, SM_THREADS, 0, ctx->stream>>>(src, vsrc, hints, vhints, seeds_dev, seed, T, (unsigned)npx);
    else sample_hints_kernel<VT, false><<<B, SM_THREADS, 0, ctx->stream>>>(src, vsrc, hints, vhints, seeds_dev, seed, T, (unsigned)npx);
    VPPX_CHECK_LAUNCH();
    return 0;
}

// Frame f of the launch samples with seeds_dev[f], or with seed + f when seeds_dev is null (the way vpp_launch takes its seeds).
int sample_launch(vppx_ctx *ctx, int B, size_t npx, const float *src, const void *vsrc, int vsrc_is_u8, float *hints, float *vhints,
                  const u32 *seeds_dev, u32 seed, u32 T)
{
    if (vsrc_is_u8) return launch_t<u8>(ctx, B, npx, src, (const u8 *)vsrc, hints, vhints, seeds_dev, seed, T);
    return launch_t<float>(ctx, B, npx, src, (const float *)vsrc, hints, vhints, seeds_dev, seed, T);
}

// torch: rand < p with a Python float p compares float32(rand) with float32(p); rand = k * 2^-24, so it is k < ceil(float(p) * 2^24)
u32 sample_threshold(double p)
{
    const float pf = (float)p;
    if (!(pf > 0.f)) return 0; // NaN selects nothing
    const double t = ceil((double)pf * 16777216.0);
    return t >= 16777216.0 ? 16777216u : (u32)t;
}
