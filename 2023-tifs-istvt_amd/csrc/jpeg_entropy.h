// The entropy decoder of a baseline JPEG restart interval (DESIGN.md "JPEG files"): one __host__ __device__ function that
// the device kernel (jpeg.hip) and a host program (tools/jpeg_entropy_check.cpp, built with sanitizers) both compile.
// clips._JpegBits / _jpeg_block are the same steps on the host and the definition of every status.
//
// The rules that bound it on any input:
//   - a byte is read only behind pos < end (je_need); past the end zeros are fed, and consuming one of them is status 1
//   - a Huffman step looks at 16 bits and takes at most 16 (je_huffman); a prefix no code matches is status 2
//   - the coefficient index of a block only grows, by at least 1 per symbol, and a run past 63 is status 3
//   - a segment decodes exactly mcu_count MCUs: at most 64 symbols per block whatever the bits say
//   - no address is made from a decoded value: table look-ups are masked to the table's 256 values, coefficients land at
//     zigzag[k] with k in 1..63, blocks at places counted from the MCU index
#ifndef ISTVT_JPEG_ENTROPY_H
#define ISTVT_JPEG_ENTROPY_H

#include <stdint.h>

#include "istvt_hip.h"
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define JE_HD __host__ __device__ __forceinline__
#else
#define JE_HD inline
#endif

// a Huffman table in decode form (clips.jpeg_huffman_table): limit[16], offset[16], values[256]
constexpr int JE_HUFF_INTS = ISTVT_JPEG_HUFF_INTS;

struct JeBits {
    const uint8_t* data;
    long pos, end;
    uint32_t buf;      // the last n bits are waiting; n <= 23
    int n, fake;       // fake: how many of the waiting bits are zeros fed past the end
    int status;
};

// at least k <= 16 bits waiting: FF 00 is the byte FF
JE_HD void je_need(JeBits& s, int k) {
    while (s.n < k) {
        uint32_t b = 0;
        if (s.pos < s.end) {
            b = s.data[s.pos++];
            if (b == 0xFF && s.pos < s.end && s.data[s.pos] == 0) ++s.pos;
        } else {
            s.fake += 8;
        }
        s.buf = (s.buf << 8) | b;
        s.n += 8;
    }
}

JE_HD void je_skip(JeBits& s, int k) {
    s.n -= k;
    if (s.n < s.fake) {
        if (s.status < 1) s.status = 1;
        s.fake = s.n;
    }
}

// the next symbol of table t, or -1 where the next 16 bits start no code
JE_HD int je_huffman(JeBits& s, const int* t) {
    je_need(s, 16);
    const int c = (int)((s.buf >> (s.n - 16)) & 0xFFFF);
    for (int l = 1; l <= 16; ++l) {
        if (c < t[l - 1]) {
            je_skip(s, l);
            return t[32 + ((t[16 + l - 1] + (c >> (16 - l))) & 255)] & 255;
        }
    }
    return -1;
}

// size <= 15 bits as a signed value (T.81 F.2.2.1)
JE_HD int je_receive(JeBits& s, int size) {
    je_need(s, size);
    const int r = (int)((s.buf >> (s.n - size)) & ((1u << size) - 1));
    je_skip(s, size);
    return r >= (1 << (size - 1)) ? r : r - (1 << size) + 1;
}

JE_HD int je_zigzag(int k) {
    static constexpr unsigned char ZZ[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                             41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                             30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
    return ZZ[k & 63];
}

// One block: its coefficients go to w.put(block, natural index, value); the block is zero on entry.  -> 0, or status 2 / 3
template <class Writer> JE_HD int je_block(JeBits& s, const int* dc, const int* ac, int& pred, Writer& w, long block) {
    int size = je_huffman(s, dc);
    if (size < 0 || size > 11) return 2;
    if (size) pred = (int16_t)(pred + je_receive(s, size));        // the prediction lives in the int16 a coefficient has
    w.put(block, 0, pred);
    int k = 1;
    while (k < 64) {
        const int rs = je_huffman(s, ac);
        if (rs < 0) return 2;
        const int r = rs >> 4;
        size = rs & 15;
        if (size == 0) {
            if (r != 15) break;
            k += 16;
            if (k > 64) return 3;
            continue;
        }
        k += r;
        if (k > 63) return 3;
        w.put(block, je_zigzag(k), je_receive(s, size));
        ++k;
    }
    return 0;
}

// How an image's blocks lie in its MCUs: v rows of h luma blocks, then nc chroma blocks (Cb, Cr: 2, or 0 for greyscale).
// The MCU is 8 h x 8 v pixels and a chroma plane has one block per MCU.
struct JeLayout {
    int h, v, nc;
};

// the layout of an images row from its layout code (ISTVT_JPEG_LAYOUT_*) and its chroma step; a code nobody defined reads as 0
JE_HD JeLayout je_layout(int code, int sub) {
    const int s = sub == 2 ? 2 : 1;
    const JeLayout l = {code == ISTVT_JPEG_LAYOUT_GREY ? 1 : code == ISTVT_JPEG_LAYOUT_422 ? 2 : s,
                        code == ISTVT_JPEG_LAYOUT_GREY || code == ISTVT_JPEG_LAYOUT_422 ? 1 : s,
                        code == ISTVT_JPEG_LAYOUT_GREY ? 0 : 2};
    return l;
}

// One restart interval: bytes [begin, end) of data, MCUs [first_mcu, first_mcu + mcu_count) of an image whose rows hold
// mcu_cols MCUs of layout lay (4:2:0: four Y blocks per MCU, 4:2:2: two side by side, 4:4:4 and greyscale: one).  huff: the DC
// and AC tables of Y, Cb, Cr; those of a component the layout does not have are never read, nor is its prediction touched.
// The writer names a block by component, block row and block column (w.block), clears it (w.clear) and takes its non-zero
// coefficients (w.put).  Every block of the interval is cleared; after status 2 or 3 the rest stay zero.  -> the status
template <class Writer>
JE_HD int je_decode_segment(const uint8_t* data, long begin, long end, const int* const* huff, const JeLayout& lay, int mcu_cols,
                            int first_mcu, int mcu_count, Writer& w) {
    JeBits s = {data, begin, end, 0u, 0, 0, 0};
    int pred[3] = {0, 0, 0};
    int dead = 0;
    for (int m = 0; m < mcu_count; ++m) {
        const int mcu = first_mcu + m;
        const int my = mcu / mcu_cols, mx = mcu - my * mcu_cols;
        for (int c = 0; c <= lay.nc; ++c) {
            const int nv = c == 0 ? lay.v : 1, nh = c == 0 ? lay.h : 1;
            for (int v = 0; v < nv; ++v) {
                for (int h = 0; h < nh; ++h) {
                    const long block = w.block(c, my * nv + v, mx * nh + h);
                    w.clear(block);
                    if (!dead) dead = je_block(s, huff[2 * c], huff[2 * c + 1], pred[c], w, block);
                }
            }
        }
    }
    return dead > s.status ? dead : s.status;
}

#endif
