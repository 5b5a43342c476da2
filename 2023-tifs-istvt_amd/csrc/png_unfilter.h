// What the PNG decoders (csrc/png.hip, csrc/png_bands.hip, csrc/png_bank.hip) share behind the inflate: the unfilter of one file
// by one wave; and for the two batch decoders the rows of the image table and the checks of the host tables that both entries
// make before any launch.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "common.h"
#include "istvt_hip.h"

namespace {

constexpr int PG_H = 0, PG_W = 1, PG_TYPE = 2, PG_BPP = 3, PG_BEGIN = 4, PG_END = 5;
constexpr int PG_FIRST_BAND = 6, PG_BANDS = 7;                  // of a batch with bands: the file's rows of the band table
constexpr int PG_FILTER = 6;               // the status of a filter byte above 4

__device__ __forceinline__ int png_paeth(int a, int b, int c) {
    const int pa = abs(b - c), pb = abs(a - c), pc = abs(a + b - 2 * c);
    return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}

// n zero bytes at p, by the wave: single bytes up to the first multiple of 4 and behind the last, dwords between
__device__ __forceinline__ void png_zero(uint8_t* p, long n, int lane) {
    long head = (long)((4 - (reinterpret_cast<uintptr_t>(p) & 3)) & 3);
    if (head > n) head = n;
    const long words = (n - head) >> 2, tail = head + 4 * words;
    if (lane < head) p[lane] = 0;
    uint32_t* q = reinterpret_cast<uint32_t*>(p + head);
    for (long i = lane; i < words; i += 64) q[i] = 0u;
    if (tail + lane < n) p[tail + lane] = 0;
}

// Lane l of band k holds row 64 k + l and reconstructs pixel x = t - l at step t: its `b` is what lane l - 1 made one step
// earlier (one cross-lane move), its `c` the `b` of its last step, its `a` its own last pixel; a pixel is one dword, bpp <= 4.
// The last row of a band is written back over its filtered bytes, all bpp channels, and lane 0 of the next band reads it there.
// BANDS: the inflate's status of the file is that of its first band that failed, in band order (band_status, read with BANDS
// only); else it is status[f]
// The form with the file's fields apart from the tables: H, W and bpp of the file, first_status its first band status word and
// count its bands (read with BANDS only), place its row of the scratch, of `out`, of sizes and of status.  csrc/png_bank.hip
// takes the fields from the bank's row of the drawn file and the place from the wave.
template <bool BANDS>
__device__ __forceinline__ void png_unfilter_file(int H, int W, int bpp, const int* __restrict__ first_status, int count, uint8_t* scratch,
                                                  long raw_stride, uint8_t* __restrict__ out, int Hc, int Wc, int* __restrict__ sizes,
                                                  int* status, int f, int lane) {
    const long stride = 1 + (long)W * bpp;
    uint8_t* raw = scratch + (long)f * raw_stride;
    uint8_t* canvas = out + (long)f * Hc * Wc * 3;
    int st;
    if constexpr (BANDS) {
        st = 0;
        for (int k0 = 0; k0 < count && st == 0; k0 += 64) {
            const int mine = k0 + lane < count ? first_status[k0 + lane] : 0;
            const unsigned long long failed = __ballot(mine != 0);
            if (failed) st = __shfl(mine, __ffsll((long long)failed) - 1);
        }
    } else {
        st = status[f];
    }
    if (st == 0) {
        int bad = 0;
        for (int r = lane; r < H; r += 64) bad |= raw[r * stride] > 4;
        if (__any(bad)) st = PG_FILTER;
    }
    if (lane == 0) {
        status[f] = st;
        sizes[2 * f] = H;
        sizes[2 * f + 1] = W;
    }
    if (st != 0) {
        png_zero(canvas, (long)Hc * Wc * 3, lane);
        return;
    }
    const int right = (Wc - W) * 3;                              // the margin beside the image, row by row; then the rows below
    if (right > 0)
        for (int y = 0; y < H; ++y) png_zero(canvas + ((long)y * Wc + W) * 3, right, lane);
    png_zero(canvas + (long)H * Wc * 3, (long)(Hc - H) * Wc * 3, lane);
    for (int band = 0; band * 64 < H; ++band) {
        const int r = band * 64 + lane;
        const bool active = r < H;
        const uint8_t* row = raw + (active ? r : 0) * stride;
        const int ft = active ? row[0] : 0;
        const uint8_t* above = row - stride + 1;                 // read by lane 0 of the bands after the first
        const bool keep = lane == 63 && r + 1 < H;
        uint32_t last = 0, c = 0;
        for (int t = 0; t < W + 63; ++t) {
            const int x = t - lane;
            uint32_t b = __shfl_up(last, 1);
            if (!active || x < 0 || x >= W) continue;
            const uint8_t* src = row + 1 + (long)x * bpp;
            if (lane == 0) {
                b = 0;
                if (band > 0)
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

// The form of the two batch decoders: file f's fields are row f of `images`, its band statuses start at its first band row
template <bool BANDS>
__device__ __forceinline__ void png_unfilter_file(const int* __restrict__ images, const int* __restrict__ band_status, uint8_t* scratch,
                                                  long raw_stride, uint8_t* __restrict__ out, int Hc, int Wc, int* __restrict__ sizes,
                                                  int* status, int f, int lane) {
    const int* im = images + (long)f * ISTVT_PNG_IMAGE_INTS;
    if constexpr (BANDS)
        png_unfilter_file<true>(im[PG_H], im[PG_W], im[PG_BPP], band_status + im[PG_FIRST_BAND], im[PG_BANDS], scratch, raw_stride, out, Hc,
                                Wc, sizes, status, f, lane);
    else
        png_unfilter_file<false>(im[PG_H], im[PG_W], im[PG_BPP], nullptr, 0, scratch, raw_stride, out, Hc, Wc, sizes, status, f, lane);
}

// one row of the host copy of the image table against the byte range: sides, a colour type with its bpp, a stream at a
// multiple of 16 inside the bytes
bool png_image_row_ok(const int* im, long nbytes) {
    const int H = im[PG_H], W = im[PG_W], ct = im[PG_TYPE], bpp = im[PG_BPP];
    if (H < 1 || W < 1 || H > 16384 || W > 16384) return false;
    if (!((ct == 0 && bpp == 1) || (ct == 2 && bpp == 3) || (ct == 6 && bpp == 4))) return false;
    return !(im[PG_BEGIN] < 0 || (im[PG_BEGIN] & 15) || im[PG_BEGIN] > im[PG_END] || im[PG_END] > nbytes);
}

// The block without its canvas and its scratch row: the pointers, the counts, the alignment and every image row.  What any
// decoder of a batch asks, whatever it decodes into (csrc/png_window.hip brings a canvas and a scratch of its own).
bool png_decode_block_ok(const istvt_jpeg_decode_args* a) {
    if (!a || a->n <= 0 || a->nbytes < 0 || a->nbytes > ISTVT_PNG_MAX_BYTES) return false;
    if (!a->bytes || !a->images || !a->images_host || !a->scratch || !a->out || !a->sizes || !a->status) return false;
    if ((reinterpret_cast<uintptr_t>(a->scratch) & 15) || (reinterpret_cast<uintptr_t>(a->bytes) & 15)) return false;
    for (int i = 0; i < a->n; ++i)
        if (!png_image_row_ok(a->images_host + (long)i * ISTVT_PNG_IMAGE_INTS, a->nbytes)) return false;
    return true;
}

// the host copy of the image table against the canvas and the scratch
bool png_decode_check(const istvt_jpeg_decode_args* a, long raw_stride) {
    for (int i = 0; i < a->n; ++i) {
        const int* im = a->images_host + (long)i * ISTVT_PNG_IMAGE_INTS;
        if (im[PG_H] > a->Hc || im[PG_W] > a->Wc) return false;
        if ((long)im[PG_H] * (1 + (long)im[PG_W] * im[PG_BPP]) > raw_stride) return false;
    }
    return true;
}

// what both entries refuse before they look at the scratch
bool png_decode_args_ok(const istvt_jpeg_decode_args* a, int raw_stride) {
    if (!png_decode_block_ok(a) || raw_stride < 16 || (raw_stride & 15)) return false;
    if (a->Hc < 1 || a->Wc < 1 || a->Hc > 16384 || a->Wc > 16384) return false;
    if (!png_decode_check(a, raw_stride)) return false;
    const uint8_t* src = (const uint8_t*)a->bytes;
    const uint8_t* out = (const uint8_t*)a->out;
    const long nout = (long)a->n * a->Hc * a->Wc * 3;
    return !(out < src + a->nbytes && src < out + nout);
}

}  // namespace
