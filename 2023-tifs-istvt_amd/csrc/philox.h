// Philox4x32-10 (Salmon, Moraes, Dror and Shaw, "Parallel random numbers: as easy as 1, 2, 3", SC'11): a four-word counter
// and a two-word key -> four 32-bit words.  Ten rounds of two 32 x 32 -> 64-bit products; the key words grow by the Weyl
// constants between rounds.  Known answers (counter and key all zero -> 6627e8d5 e169c58d bc57ac4c 9b00dbd8) are held by
// clips.philox4x32_10, the host restatement the kernels' bytes are compared with.  A host program compiles it too
// (csrc/batch_draw.h, tools/batch_draw_check.cpp): plain integer arithmetic, the same words on either side.
#pragma once
#if defined(__HIPCC__)
#include "common.h"
#define PHILOX_HD __host__ __device__ __forceinline__
#else
#define PHILOX_HD inline
#endif

PHILOX_HD void philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1,
                             unsigned (&r)[4]) {
#pragma unroll
    for (int i = 0; i < 10; ++i) {
        const unsigned long long p0 = (unsigned long long)0xD2511F53u * c0, p1 = (unsigned long long)0xCD9E8D57u * c2;
        const unsigned n0 = (unsigned)(p1 >> 32) ^ c1 ^ k0, n1 = (unsigned)p1;
        const unsigned n2 = (unsigned)(p0 >> 32) ^ c3 ^ k1, n3 = (unsigned)p0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    r[0] = c0; r[1] = c1; r[2] = c2; r[3] = c3;
}
