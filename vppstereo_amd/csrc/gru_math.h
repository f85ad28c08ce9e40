// gru_math.h -- the gate formulas of ConvGRU.forward (models/raft_stereo/update.py:27-31) as include/vppx.h states them: one
// correctly rounded float32 operation per step around the device's expf.  gru_kernels.hip (the glue between torch's
// convolutions) and conv_kernels.hip (the same gates as epilogues of the convolutions) share them.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

// 1 / (1 + exp(-v)): +inf -> 1 / (1 + 0) = 1, -inf -> 1 / inf = 0
__device__ __forceinline__ float gru_sigmoid(float v) { return __fdiv_rn(1.0f, __fadd_rn(1.0f, expf(-v))); }
// 1 - 2 / (exp(2v) + 1): +inf -> 1 - 2 / inf = 1, -inf -> 1 - 2 / 1 = -1
__device__ __forceinline__ float gru_tanh(float v) { return __fsub_rn(1.0f, __fdiv_rn(2.0f, __fadd_rn(expf(__fmul_rn(2.0f, v)), 1.0f))); }

// ((1 - z) * h) + (z * q)
__device__ __forceinline__ float gru_mix(float z, float q, float h) { return __fadd_rn(__fmul_rn(__fsub_rn(1.0f, z), h), __fmul_rn(z, q)); }
