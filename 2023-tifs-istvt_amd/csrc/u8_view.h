// Reading decoded frames, uint8 [frames][Hs][Ws][3], as conv1's input: the normalisation every byte kernel applies and the
// staging of a VIEW of a source frame (a crop window and an optional horizontal flip) in LDS.
//
//   view[f] = (y0, x0, flip): output pixel (y, x) of frame f is source pixel (y0 + y, x0 + (flip ? S - 1 - x : x)); the
//   channel order inside a pixel is never reversed.  A null table is (0, 0, 0) for every frame.
//
// The bytes of a view row are ONE contiguous range of the source (S * 3 bytes at ((f * Hs + y0 + y) * Ws + x0) * 3), but
// successive rows are Ws * 3 bytes apart: rows are staged one by one, each from its enclosing 16-byte-aligned range with
// 16-byte loads, so row r of a work item lies at sb + r * pitch + lead(r), lead(r) = the row's address & 15.  A 16-byte
// piece that sticks out of [x, x + total) is read byte by byte: any slice of a batch is accepted, unaligned base
// pointers included, and nothing outside the tensor is touched.  The flip is applied where a pixel is looked up
// (u8_view_px), not in the staged bytes.
#pragma once
#include "common.h"

// v = (float(u) / 255 - mean) / std as torchvision's ToTensor + Normalize compute it on the host: each operation rounded
// on its own (the explicitly rounded intrinsics: nothing for -ffp-contract=fast to fuse or reassociate)
__device__ __forceinline__ float u8_normalise(int u, float mean, float stdv) {
    return __fdiv_rn(__fsub_rn(__fdiv_rn((float)u, 255.0f), mean), stdv);
}

// A byte has 256 values: the three channels' normalised values as a 3 x 256 float table in LDS, lut[c * 256 + u]
__device__ __forceinline__ void u8_fill_lut(float* lut, const float* __restrict__ mean, const float* __restrict__ stdv,
                                            int tid, int nthreads) {
    for (int i = tid; i < 3 * 256; i += nthreads) {
        const int c = i >> 8;
        lut[i] = u8_normalise(i & 255, mean[c], stdv[c]);
    }
}

struct U8View {
    int y0, x0, flip;
};

// The view of frame f, forced into the source (a table that was not validated can then still read nothing it must not)
__device__ __forceinline__ U8View u8_view_of(const int* __restrict__ view, long f, int Hs, int Ws, int S) {
    U8View v{0, 0, 0};
    if (view) {
        v.y0 = min(max(view[f * 3 + 0], 0), Hs - S);
        v.x0 = min(max(view[f * 3 + 1], 0), Ws - S);
        v.flip = view[f * 3 + 2] != 0;
    }
    return v;
}

// 16 bytes at offset o from x (x + o is 16-byte aligned); the part outside [0, total) reads as zero and is never used
__device__ __forceinline__ uint4 u8_load16(const uint8_t* __restrict__ x, long o, long total) {
    if (o >= 0 && o + 16 <= total) return *reinterpret_cast<const uint4*>(x + o);
    unsigned char b[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) b[j] = (o + j >= 0 && o + j < total) ? x[o + j] : (unsigned char)0;
    return *reinterpret_cast<const uint4*>(b);
}

// pitch of a staged row of S pixels: lead (<= 15) + S * 3 bytes, in whole 16-byte pieces
__host__ __device__ __forceinline__ int u8_row_pitch(int S) { return ((S * 3 + 30) >> 4) << 4; }

// Stage rows [0, nrows) of a work item, `len` bytes each: row r is the bytes at g0 + r * rstride (offsets from x), laid down
// at sb + r * pitch + lead(r); pitch >= 15 + len in whole 16-byte pieces.  Returns lead(0); lead(r) = (lead(0) + r *
// rstride) & 15 (u8_row_lead).  The caller synchronises.
__device__ __forceinline__ int u8_stage_byte_rows(const uint8_t* __restrict__ x, long total, long g0, int rstride, int nrows,
                                                  int len, unsigned char* sb, int pitch, int tid, int nthreads) {
    const int lead0 = (int)((reinterpret_cast<uintptr_t>(x) + (uintptr_t)g0) & 15);
    const int cpr = pitch >> 4;
    for (int i = tid; i < nrows * cpr; i += nthreads) {
        const int rr = i / cpr, c = i - rr * cpr;
        const int lead = (lead0 + rr * rstride) & 15;
        if (16 * c >= lead + len) continue;
        const long o = g0 + (long)rr * rstride - lead + 16L * c;
        *reinterpret_cast<uint4*>(sb + rr * pitch + 16 * c) = u8_load16(x, o, total);
    }
    return lead0;
}

// The same for rows of S packed RGB pixels (S * 3 bytes, pitch = u8_row_pitch(S))
__device__ __forceinline__ int u8_stage_rows(const uint8_t* __restrict__ x, long total, long g0, int rstride, int nrows,
                                             int S, unsigned char* sb, int pitch, int tid, int nthreads) {
    return u8_stage_byte_rows(x, total, g0, rstride, nrows, S * 3, sb, pitch, tid, nthreads);
}

__device__ __forceinline__ int u8_row_lead(int lead0, int r, int rstride) { return (lead0 + r * rstride) & 15; }

// first byte (channel 0) of view pixel px of a staged row
__device__ __forceinline__ int u8_view_px(int px, int S, int flip) { return (flip ? S - 1 - px : px) * 3; }
