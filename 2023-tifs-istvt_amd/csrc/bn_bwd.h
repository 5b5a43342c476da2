// The BatchNorm-backward apply expression, shared by bn_bwd_apply_kernel (stem.hip) and the fused 1x1-convolution
// backward (pw_bwd.hip): both must produce the same bf16 du from the same operands, bit for bit.
//
//   du = gamma * rstd * (dz - s1/M - xhat * s2/M),   xhat = (u - mean) * rstd
//
// k1 = (float)s1 / M and k2 = (float)s2 / M in train mode, 0 in eval mode (running statistics are constants).
#pragma once
#include "common.h"

// per-channel constants of one 8-channel chunk c0 .. c0+7
struct BnBwdChunk {
    float mu[8], rs[8], g[8], k1[8], k2[8];
};

__device__ __forceinline__ void bn_bwd_chunk_load(BnBwdChunk& k, const float* __restrict__ bnp,
                                                  const float* __restrict__ gamma, const double* s1, const double* s2,
                                                  int C, int c0, float invM) {
    load8(bnp + c0, k.mu);          // pack row 0: mean
    load8(bnp + C + c0, k.rs);      // pack row 1: rstd
    load8(gamma + c0, k.g);
#pragma unroll
    for (int j = 0; j < 8; ++j) { k.k1[j] = (float)s1[c0 + j] * invM; k.k2[j] = (float)s2[c0 + j] * invM; }
}

__device__ __forceinline__ float bn_bwd_du(float dz, float u, const BnBwdChunk& k, int j) {
    const float x = (u - k.mu[j]) * k.rs[j];
    return k.g[j] * k.rs[j] * (dz - k.k1[j] - x * k.k2[j]);
}
