// The entropy coder of a baseline JPEG restart interval (DESIGN.md "JPEG files out"): one __host__ __device__ function that
// the device kernels (jpeg.hip: once to count, once to store) and a host program (tools/jpeg_entropy_enc_check.cpp, built
// with sanitizers) both compile.  clips.jpeg_encode_host is the same steps on the host and the definition of every byte.
//
// The rules that bound it on any int16 input:
//   - a byte leaves only through the sink (sink.byte), which counts it and, where it stores, stores it only inside
//     [begin, begin + counted length) of its segment
//   - the count pass and the store pass are this one function on the same coefficients, so their lengths agree
//   - a table index is masked to the table's size (16 DC categories, 256 AC symbols); a coefficient outside baseline's
//     categories is coded clamped (DC difference to +-2047, AC to +-1023) and reported as status 3
//   - no address is made from a coefficient's value: a block's place is counted from the MCU index
//   - a block costs at most 1 + 63 symbols and 3 ZRLs per run, so a segment is bounded by its MCU count
#ifndef ISTVT_JPEG_ENTROPY_ENC_H
#define ISTVT_JPEG_ENTROPY_ENC_H

#include <stdint.h>

#include "jpeg_entropy.h"
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define JEE_HD __host__ __device__ __forceinline__
#else
#define JEE_HD inline
#endif

// ITU-T T.81 Annex K.3: the four typical Huffman tables as (codes of length 1..16, values in code order); [class][id] with
// class 0 = DC, 1 = AC and id 0 = luminance, 1 = chrominance (clips.JPEG_STD_HUFFMAN)
struct JeStdHuffman {
    uint8_t counts[2][2][16];
    uint8_t values[2][2][256];
    int total[2][2];
};

constexpr JeStdHuffman je_std_huffman() {
    JeStdHuffman t{};
    constexpr uint8_t counts[2][2][16] = {{{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}},
                                          {{0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d},
                                           {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77}}};
    // the head of each AC value list; after it run r carries the sizes lo[r]..10
    constexpr uint8_t head0[39] = {0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13,
                                   0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1, 0x08, 0x23, 0x42,
                                   0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a};
    constexpr uint8_t head1[47] = {0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71,
                                   0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0,
                                   0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a};
    constexpr uint8_t lo0[16] = {0, 6, 5, 4, 3, 3, 3, 3, 3, 2, 2, 2, 2, 2, 1, 1};       // run 0 is all in the head
    constexpr uint8_t lo1[16] = {0, 0, 6, 5, 3, 3, 3, 3, 2, 2, 2, 2, 2, 2, 2, 2};       // runs 0 and 1 likewise
    for (int c = 0; c < 2; ++c)
        for (int id = 0; id < 2; ++id)
            for (int l = 0; l < 16; ++l) t.counts[c][id][l] = counts[c][id][l];
    for (int id = 0; id < 2; ++id) {
        for (int v = 0; v < 12; ++v) t.values[0][id][v] = (uint8_t)v;
        t.total[0][id] = 12;
    }
    int at = 0;
    for (int i = 0; i < 39; ++i) t.values[1][0][at++] = head0[i];
    for (int r = 1; r < 16; ++r)
        for (int s = lo0[r]; s < 11; ++s) t.values[1][0][at++] = (uint8_t)((r << 4) | s);
    t.total[1][0] = at;
    at = 0;
    for (int i = 0; i < 47; ++i) t.values[1][1][at++] = head1[i];
    for (int r = 2; r < 16; ++r)
        for (int s = lo1[r]; s < 11; ++s) t.values[1][1][at++] = (uint8_t)((r << 4) | s);
    t.total[1][1] = at;
    return t;
}

// The same tables in coding form: (code << 8) | length per symbol, 0 for a symbol the table does not hold.
// dc[id][category & 15], ac[id][(run << 4 | size) & 255]; as one array of JE_CODE_WORDS words: dc[0] | dc[1] | ac[0] | ac[1]
constexpr int JE_CODE_WORDS = 2 * 16 + 2 * 256;
constexpr int JE_CODE_DC = 0, JE_CODE_AC = 32;      // first word of dc[0] and of ac[0]

struct JeCodeTables {
    uint32_t w[JE_CODE_WORDS];
};

constexpr JeCodeTables je_make_code_tables() {
    JeCodeTables t{};
    const JeStdHuffman h = je_std_huffman();
    for (int c = 0; c < 2; ++c)
        for (int id = 0; id < 2; ++id) {
            uint32_t code = 0;
            int at = 0;
            for (int l = 1; l <= 16; ++l) {
                for (int k = 0; k < h.counts[c][id][l - 1]; ++k) {
                    const int sym = h.values[c][id][at++];
                    t.w[c == 0 ? JE_CODE_DC + id * 16 + (sym & 15) : JE_CODE_AC + id * 256 + sym] = (code << 8) | (uint32_t)l;
                    ++code;
                }
                code <<= 1;
            }
        }
    return t;
}

// the coding tables, built at compile time; a kernel copies them into LDS once per workgroup
JEE_HD uint32_t je_code_word(int i) {
    static constexpr JeCodeTables T = je_make_code_tables();
    return T.w[i];
}

// 16 bytes of a block: coefficients 8 i .. 8 i + 7 in zig-zag order, coefficient j in bits 16 j .. of lo (j < 4) or hi
struct alignas(16) JeQuad {
    uint64_t lo, hi;
};

// a sink that only counts (the first pass)
struct JeCount {
    long n;
    JEE_HD void byte(uint32_t) { ++n; }
};

// a sink that stores: byte k of the segment goes to data[begin + k] where k < len, the length the first pass counted
struct JeStore {
    uint8_t* data;
    long begin, len, n;
    JEE_HD void byte(uint32_t b) {
        if (n < len) data[begin + n] = (uint8_t)b;
        ++n;
    }
};

struct JeEnc {
    uint64_t acc;      // the last n bits are waiting; n < 32 between two puts
    int n, status;
};

template <class Sink> JEE_HD void je_stuffed(Sink& s, uint32_t b) {
    s.byte(b);
    if (b == 0xFF) s.byte(0);
}

// len <= 32 bits of code behind the waiting ones; whole bytes leave four at a time, from the register
template <class Sink> JEE_HD void je_put(JeEnc& e, Sink& s, uint32_t code, int len) {
    e.acc = (e.acc << len) | code;
    e.n += len;
    if (e.n >= 32) {
        e.n -= 32;
        const uint32_t w = (uint32_t)(e.acc >> e.n);
        je_stuffed(s, w >> 24);
        je_stuffed(s, (w >> 16) & 255);
        je_stuffed(s, (w >> 8) & 255);
        je_stuffed(s, w & 255);
    }
}

// the category of v (T.81 F.1.2.1): the bits of |v|; |v| < 2^15
JEE_HD int je_size(int v) {
    const uint32_t a = (uint32_t)(v < 0 ? -v : v);
    return a ? 32 - __builtin_clz(a) : 0;
}

// a Huffman code word t and the `size` low bits of v (v - 1 for a negative v) behind it
template <class Sink> JEE_HD void je_symbol(JeEnc& e, Sink& s, uint32_t t, int v, int size) {
    const uint32_t bits = (uint32_t)(v < 0 ? v - 1 : v) & ((1u << size) - 1);
    je_put(e, s, ((t >> 8) << size) | bits, (int)(t & 255) + size);
}

// `count` <= 4 AC coefficients from the low end of w
template <class Sink> JEE_HD void je_ac(JeEnc& e, Sink& s, uint64_t w, int count, int& run, const uint32_t* ac) {
    for (int j = 0; j < count; ++j) {
        if (w == 0) {
            run += count - j;
            return;
        }
        int v = (int16_t)(w & 0xFFFF);
        w >>= 16;
        if (v == 0) {
            ++run;
            continue;
        }
        while (run > 15) {
            const uint32_t zrl = ac[0xF0];
            je_put(e, s, zrl >> 8, (int)(zrl & 255));
            run -= 16;
        }
        if (v > 1023 || v < -1023) {
            v = v > 0 ? 1023 : -1023;
            e.status = 3;
        }
        const int size = je_size(v);
        je_symbol(e, s, ac[((run << 4) | size) & 255], v, size);
        run = 0;
    }
}

// One block: 64 int16 in zig-zag order, read as eight 16-byte loads.  pred: the DC of the previous block of the component
template <class Sink> JEE_HD void je_encode_block(JeEnc& e, Sink& s, const JeQuad* blk, int& pred, const uint32_t* dc, const uint32_t* ac) {
    JeQuad q[8];
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int i = 0; i < 8; ++i) q[i] = blk[i];
    const int v0 = (int16_t)(q[0].lo & 0xFFFF);
    int diff = v0 - pred;
    pred = v0;
    if (diff > 2047 || diff < -2047) {
        diff = diff > 0 ? 2047 : -2047;
        e.status = 3;
    }
    const int size = je_size(diff);
    je_symbol(e, s, dc[size & 15], diff, size);
    int run = 0;
    je_ac(e, s, q[0].lo >> 16, 3, run, ac);
    je_ac(e, s, q[0].hi, 4, run, ac);
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int i = 1; i < 8; ++i) {
        if ((q[i].lo | q[i].hi) == 0) {
            run += 8;
            continue;
        }
        je_ac(e, s, q[i].lo, 4, run, ac);
        je_ac(e, s, q[i].hi, 4, run, ac);
    }
    if (run) {                                                   // zeros to the end of the block: EOB
        const uint32_t eob = ac[0];
        je_put(e, s, eob >> 8, (int)(eob & 255));
    }
}

// One restart interval: MCUs [first_mcu, first_mcu + mcu_count) of an image of mcu_rows x mcu_cols MCUs of layout lay
// (JeLayout of jpeg_entropy.h; 4:2:0: four Y blocks per MCU, 4:2:2: two side by side, 4:4:4 and greyscale: one; greyscale has
// no Cb or Cr and codes with table id 0 only).  coef: the image's blocks, int16 [block][64] in zig-zag order, 16-byte
// aligned: those of Y row by row of the plane padded to whole MCUs, then Cb's, then Cr's.  codes: je_code_word's words
// (JE_CODE_WORDS of them).  The DC prediction starts at 0 and is the DC of the previous block of the component, read from
// coef.  After the last MCU the bits are padded with ones to a whole byte and FF `marker` follows (RSTm, or EOI after the
// last interval).
// -> the bytes handed to the sink, stuffed bytes, pad and marker included; status: 0, or 3 where a coefficient was clamped
template <class Sink>
JEE_HD long je_encode_segment(const int16_t* coef, const JeLayout& lay, int mcu_cols, int mcu_rows, int first_mcu, int mcu_count,
                              const uint32_t* codes, int marker, Sink& sink, int& status) {
    JeEnc e = {0u, 0, 0};
    int pred[3] = {0, 0, 0};
    const JeQuad* blocks = reinterpret_cast<const JeQuad*>(coef);
    const long ybw = (long)mcu_cols * lay.h, ny = ybw * mcu_rows * lay.v, nc = (long)mcu_cols * mcu_rows;
    const long mcus = nc;
    for (int m = 0; m < mcu_count; ++m) {
        const long mcu = (long)first_mcu + m;
        if (mcu < 0 || mcu >= mcus) break;
        const int my = (int)(mcu / mcu_cols), mx = (int)(mcu - (long)my * mcu_cols);
        for (int c = 0; c <= lay.nc && c < 3; ++c) {
            const int nv = c == 0 ? lay.v : 1, nh = c == 0 ? lay.h : 1;
            const uint32_t* dc = codes + JE_CODE_DC + (c ? 16 : 0);
            const uint32_t* ac = codes + JE_CODE_AC + (c ? 256 : 0);
            for (int v = 0; v < nv; ++v) {
                for (int h = 0; h < nh; ++h) {
                    const long b = c == 0 ? ((long)my * lay.v + v) * ybw + (long)mx * lay.h + h : ny + (c - 1) * nc + mcu;
                    je_encode_block(e, sink, blocks + b * 8, pred[c], dc, ac);
                }
            }
        }
    }
    if (e.n & 7) {
        const int k = 8 - (e.n & 7);
        je_put(e, sink, (1u << k) - 1, k);
    }
    while (e.n > 0) {
        e.n -= 8;
        je_stuffed(sink, (uint32_t)(e.acc >> e.n) & 255);
    }
    sink.byte(0xFF);
    sink.byte((uint32_t)marker & 255);
    status = e.status;
    return sink.n;
}

#endif
