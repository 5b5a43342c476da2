// The unfilter of one band that stands alone, by one wave (DESIGN.md "PNG bands that stand alone"): what the two kernels of
// csrc/png_alone.hip share.  Every wave of a file settles the file's status for itself, from the band statuses and one pass
// over the H filter bytes, before it writes a pixel; so every wave of a failed file zeroes its own rows of the canvas and no
// wave needs another.  The decisions are csrc/png_alone.h's.
#pragma once
#include "png_alone.h"
#include "png_unfilter.h"

namespace {

// Rows [r0, r1) of a file whose bands stand alone, 64 rows at a time with png_unfilter_file's diagonal scheme: lane l holds
// row r0 + 64 g + l and reconstructs pixel x = t - l at step t.  b = c = 0 on row r0; the last row of a group of 64 is written
// back over its filtered bytes, and lane 0 of the next group reads it there.  Only bytes of rows [r0, r1) are read or written,
// and never a row's filter byte.
__device__ __forceinline__ void png_unfilter_rows(int r0, int r1, int W, int bpp, uint8_t* raw, long stride, uint8_t* canvas, int Wc,
                                                  int lane) {
    for (int g = 0; r0 + g * 64 < r1; ++g) {
        const int r = r0 + g * 64 + lane;
        const bool active = r < r1;
        const uint8_t* row = raw + (active ? r : r0) * stride;
        const int ft = active ? row[0] : 0;
        const uint8_t* above = row - stride + 1;                 // read by lane 0 of the groups after the first
        const bool keep = lane == 63 && r + 1 < r1;
        uint32_t last = 0, c = 0;
        for (int t = 0; t < W + 63; ++t) {
            const int x = t - lane;
            uint32_t b = __shfl_up(last, 1);
            if (!active || x < 0 || x >= W) continue;
            const uint8_t* src = row + 1 + (long)x * bpp;
            if (lane == 0) {
                b = 0;
                if (g > 0)
                    for (int k = 0; k < bpp; ++k) b |= (uint32_t)above[(long)x * bpp + k] << (8 * k);
            }
            const uint32_t a = x > 0 ? last : 0;
            if (x == 0) c = 0;
            uint32_t px = 0;
            for (int k = 0; k < bpp; ++k) {
                const int v = src[k], ak = (a >> (8 * k)) & 255, bk = (b >> (8 * k)) & 255, ck = (c >> (8 * k)) & 255;
                const int pred = ft == 0 ? 0 : ft == 1 ? ak : ft == 2 ? bk : ft == 3 ? (ak + bk) >> 1 : png_paeth(ak, bk, ck);
                px |= (uint32_t)((v + pred) & 255) << (8 * k);
            }
            last = px;
            c = b;
            uint8_t* dst = canvas + ((long)r * Wc + x) * 3;
            if (bpp == 1) {
                dst[0] = dst[1] = dst[2] = (uint8_t)px;
            } else {
                dst[0] = (uint8_t)px;
                dst[1] = (uint8_t)(px >> 8);
                dst[2] = (uint8_t)(px >> 16);
            }
            if (keep)
                for (int k = 0; k < bpp; ++k) raw[r * stride + 1 + (long)x * bpp + k] = (uint8_t)(px >> (8 * k));
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();                                         // lane 63's row has landed before lane 0 reads it
    }
}

// Wave k of file f, whose count >= 1 bands of R rows stand alone and whose band rows csrc/png_alone.h has passed, k < count:
// the file's status (the first band status that is not 0 in band order, then the filter bytes), then rows [k R, min(H, (k + 1)
// R)) of the canvas, reconstructed or zeroed, with the margin right of them.  The wave of band 0 writes status and sizes and
// zeroes the margin below the image.  raw: the file's filtered rows, canvas: its place in `out`.
__device__ __forceinline__ void png_unfilter_alone(int H, int W, int bpp, int R, int k, const int* __restrict__ first_status, int count,
                                                   uint8_t* raw, uint8_t* canvas, int Hc, int Wc, int* __restrict__ sizes, int* status,
                                                   int f, int lane) {
    const long stride = 1 + (long)W * bpp;
    int band = 0;
    for (int k0 = 0; k0 < count && band == 0; k0 += 64) {
        const int mine = k0 + lane < count ? first_status[k0 + lane] : 0;
        const unsigned long long failed = __ballot(mine != 0);
        if (failed) band = __shfl(mine, __ffsll((long long)failed) - 1);
    }
    int marks = 0;
    if (band == 0) {
        const int mine = pa_marks(raw, stride, H, R, lane, 64);
        marks = (__any(mine & 1) ? 1 : 0) | (__any(mine & 2) ? 2 : 0);
    }
    const int st = pa_status(band, marks);
    int r0, r1;
    pa_band_span(H, R, k, &r0, &r1);
    if (k == 0) {
        if (lane == 0) {
            status[f] = st;
            sizes[2 * f] = pa_sized(st) ? H : 0;
            sizes[2 * f + 1] = pa_sized(st) ? W : 0;
        }
        png_zero(canvas + (long)H * Wc * 3, (long)(Hc - H) * Wc * 3, lane);
    }
    if (st != 0) {
        png_zero(canvas + (long)r0 * Wc * 3, (long)(r1 - r0) * Wc * 3, lane);
        return;
    }
    const int right = (Wc - W) * 3;
    if (right > 0)
        for (int y = r0; y < r1; ++y) png_zero(canvas + ((long)y * Wc + W) * 3, right, lane);
    png_unfilter_rows(r0, r1, W, bpp, raw, stride, canvas, Wc, lane);
}

}  // namespace
