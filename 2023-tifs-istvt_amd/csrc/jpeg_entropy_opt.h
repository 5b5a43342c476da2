// Optimised Huffman tables for the encoder (DESIGN.md "JPEG files out, optimised tables"): symbol counts of a block, the
// table libjpeg's jpeg_gen_optimal_table makes of 256 counts, and its code words in the layout je_encode_segment reads.  One
// set of __host__ __device__ functions that jpeg_tables_kernel (jpeg.hip) and a host program
// (tools/jpeg_entropy_opt_check.cpp, built with sanitizers) both compile.  clips.jpeg_symbol_counts and
// clips.jpeg_optimal_table are the same steps on the host and the definition of every table.
//
// The rules that bound it on any 256 counts and any int16 coefficients:
//   - a symbol is counted where je_encode_block codes one, with the same clamps, so a symbol coded has a code
//   - a count leaves only through the sink (sink.dc / sink.ac) with its index masked to 16 / 256
//   - 257 symbols give at most 256 merges; the loop is bounded by that number, not by the counts
//   - a chain of `others` is followed for at most 257 steps and every link is range-checked
//   - a length is capped at 32 where it indexes; where one passed 32 the counts are halved, rounding up, and the merging
//     starts again: at most 32 times, after which every count is 1 and no length passes 9
//   - no address is made from a count: counts are only compared and added, in 64 bits
#ifndef ISTVT_JPEG_ENTROPY_OPT_H
#define ISTVT_JPEG_ENTROPY_OPT_H

#include "jpeg_entropy_enc.h"

constexpr int JO_SYMBOLS = 257;             // 256 and the reserved one, which keeps the all-ones code free
constexpr int JO_MAX_LENGTH = 32;           // the longest length the folding loop starts from (libjpeg's MAX_CLEN)

// what jo_optimal_table works in: a kernel keeps one per table in LDS
struct JoWork {
    uint64_t freq[JO_SYMBOLS];
    int16_t others[JO_SYMBOLS], live[JO_SYMBOLS];       // live[0 .. n): the symbols with a count, ascending
    uint8_t size[JO_SYMBOLS];
    int bits[JO_MAX_LENGTH + 1];
};

// One pass of merging over counts >> shift (rounded up).  -> whether every length stayed <= 32
JEE_HD bool jo_merge(const uint32_t* counts, int shift, JoWork& w, int& n_live) {
    int n = 0;
    for (int s = 0; s < JO_SYMBOLS; ++s) {
        const uint64_t c = s < 256 ? (((uint64_t)counts[s] + ((1ull << shift) - 1)) >> shift) : 1;
        w.freq[s] = c;
        w.others[s] = -1;
        w.size[s] = 0;
        if (c) w.live[n++] = (int16_t)s;
    }
    n_live = n;
    bool fits = true;
    for (int merge = 0; merge < JO_SYMBOLS - 1; ++merge) {
        int c1 = -1, c2 = -1;                                     // the smallest count, then the next; ties: the larger symbol
        uint64_t v = ~0ull;
        for (int p = 0; p < n; ++p) {
            const int s = w.live[p];
            const uint64_t f = w.freq[s];
            if (f && f <= v) v = f, c1 = s;
        }
        v = ~0ull;
        for (int p = 0; p < n; ++p) {
            const int s = w.live[p];
            const uint64_t f = w.freq[s];
            if (f && f <= v && s != c1) v = f, c2 = s;
        }
        if (c2 < 0) break;
        w.freq[c1] += w.freq[c2];
        w.freq[c2] = 0;
        for (int side = 0; side < 2; ++side) {                    // one bit more for every symbol of both chains
            int c = side ? c2 : c1;
            for (int step = 0; step < JO_SYMBOLS; ++step) {
                if (w.size[c] < 255) ++w.size[c];
                if (w.size[c] > JO_MAX_LENGTH) fits = false;
                const int next = w.others[c];
                if (next < 0 || next >= JO_SYMBOLS) break;
                c = next;
            }
            if (side == 0) w.others[c] = (int16_t)c2;             // the chain of c2 behind the chain of c1
        }
    }
    return fits;
}

// 256 counts -> the table: bits[l - 1] codes of length l, values[0 .. total) in code order; the bytes of a DHT segment
// behind its class and id.  All-zero counts -> an empty table (bits all 0, total 0), which no scan symbol refers to.
JEE_HD void jo_optimal_table(const uint32_t counts[256], uint8_t bits[16], uint8_t values[256], int* total, JoWork& w) {
    for (int l = 0; l < 16; ++l) bits[l] = 0;
    *total = 0;
    uint32_t any = 0;
    for (int s = 0; s < 256; ++s) any |= counts[s];
    if (!any) return;
    int n = 0;
    for (int shift = 0; shift <= 32; ++shift)
        if (jo_merge(counts, shift, w, n)) break;
    for (int l = 0; l <= JO_MAX_LENGTH; ++l) w.bits[l] = 0;
    for (int p = 0; p < n; ++p) {
        const int l = w.size[w.live[p]];
        ++w.bits[l < JO_MAX_LENGTH ? l : JO_MAX_LENGTH];
    }
    for (int i = JO_MAX_LENGTH; i > 16; --i) {                    // T.81 K.2: fold the lengths above 16 down
        for (int guard = 0; guard < JO_SYMBOLS && w.bits[i] > 1; ++guard) {
            int j = i - 2;
            while (j > 0 && w.bits[j] == 0) --j;
            if (j == 0) break;
            w.bits[i] -= 2;
            w.bits[i - 1] += 1;
            w.bits[j + 1] += 2;
            w.bits[j] -= 1;
        }
    }
    int i = 16;
    while (i > 0 && w.bits[i] == 0) --i;
    if (i > 0) --w.bits[i];                                       // the reserved symbol's code, the longest
    for (int l = 1; l <= 16; ++l) bits[l - 1] = (uint8_t)(w.bits[l] & 255);
    int at = 0;
    for (int l = 1; l <= JO_MAX_LENGTH; ++l)                      // by length before the folding, then by symbol
        for (int p = 0; p < n; ++p) {
            const int s = w.live[p];
            if (s < 256 && w.size[s] == l && at < 256) values[at++] = (uint8_t)s;
        }
    *total = at;
}

JEE_HD void jo_optimal_table(const uint32_t counts[256], uint8_t bits[16], uint8_t values[256], int* total) {
    JoWork w;
    jo_optimal_table(counts, bits, values, total, w);
}

// the table as code words, (code << 8) | length per symbol and 0 for a symbol it does not hold: words[sym & (n - 1)], n = 16
// for a DC table (JE_CODE_DC + 16 id) and 256 for an AC table (JE_CODE_AC + 256 id) of the JE_CODE_WORDS layout
JEE_HD void jo_code_words(const uint8_t bits[16], const uint8_t* values, int total, uint32_t* words, int n) {
    for (int i = 0; i < n; ++i) words[i] = 0;
    uint32_t code = 0;
    int at = 0;
    for (int l = 1; l <= 16; ++l) {
        for (int k = 0; k < bits[l - 1] && at < total && at < 256; ++k) {
            words[values[at++] & (n - 1)] = (code << 8) | (uint32_t)l;
            ++code;
        }
        code <<= 1;
    }
}

// a sink that counts into four histograms of 256 in the order of the file's DHT segments and of the JE_CODE_WORDS layout:
// DC of table id 0, DC of id 1, AC of id 0, AC of id 1
struct JoHistogram {
    uint32_t* counts;                      // [4][256]
    JEE_HD void dc(int id, int sym) { ++counts[(id & 1) * 256 + (sym & 255)]; }
    JEE_HD void ac(int id, int sym, uint32_t times) { counts[(2 + (id & 1)) * 256 + (sym & 255)] += times; }
};

// `count` <= 4 AC coefficients from the low end of w: je_ac's walk
template <class Sink> JEE_HD void jo_ac(Sink& s, int id, uint64_t w, int count, int& run) {
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
        if (run > 15) s.ac(id, 0xF0, (uint32_t)(run >> 4));       // a ZRL per 16 zeros
        run &= 15;
        if (v > 1023 || v < -1023) v = v > 0 ? 1023 : -1023;
        s.ac(id, ((run << 4) | je_size(v)) & 255, 1u);
        run = 0;
    }
}

// The symbols of one block as je_encode_block codes them: 64 int16 in zig-zag order; pred: the DC of the previous block of
// the component, or 0 behind a restart; id: the block's pair of tables (0 for Y, 1 for the rest)
template <class Sink> JEE_HD void jo_count_block(Sink& s, const JeQuad* blk, int pred, int id) {
    JeQuad q[8];
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int i = 0; i < 8; ++i) q[i] = blk[i];
    int diff = (int16_t)(q[0].lo & 0xFFFF) - pred;
    if (diff > 2047 || diff < -2047) diff = diff > 0 ? 2047 : -2047;
    s.dc(id, je_size(diff) & 15);
    int run = 0;
    jo_ac(s, id, q[0].lo >> 16, 3, run);
    jo_ac(s, id, q[0].hi, 4, run);
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int i = 1; i < 8; ++i) {
        if ((q[i].lo | q[i].hi) == 0) {
            run += 8;
            continue;
        }
        jo_ac(s, id, q[i].lo, 4, run);
        jo_ac(s, id, q[i].hi, 4, run);
    }
    if (run) s.ac(id, 0, 1u);                                     // zeros to the end of the block: EOB
}

// Block b of an image in the order of its coefficients (Y row by row of the padded plane, then Cb, then Cr) -> the block
// whose DC predicts it in the scan, or -1 where the prediction is 0: the first block of its component in a restart interval
// of ri >= 1 MCUs.  lay, mcu_cols, mcu_rows as je_encode_segment takes them; a greyscale image has Y blocks only
JEE_HD long jo_previous_block(long b, const JeLayout& lay, int mcu_cols, int mcu_rows, int ri, int& id) {
    const long ybw = (long)mcu_cols * lay.h, ny = ybw * mcu_rows * lay.v, nc = (long)mcu_cols * mcu_rows;
    if (b >= ny) {                                                // chroma: one block per MCU
        id = 1;
        const long mcu = (b - ny) % nc;
        return mcu % ri == 0 ? -1 : b - 1;
    }
    id = 0;
    const long row = b / ybw, col = b - row * ybw;
    const int v = (int)(row % lay.v), h = (int)(col % lay.h);
    if (h > 0) return b - 1;
    if (v > 0) return b - ybw + (lay.h - 1);                      // the last block of the MCU's row above
    const long my = row / lay.v, mx = col / lay.h, mcu = my * mcu_cols + mx;
    if (mcu % ri == 0) return -1;
    const long py = mx > 0 ? my : my - 1, px = mx > 0 ? mx - 1 : mcu_cols - 1;    // the MCU before: its last block
    return (py * lay.v + (lay.v - 1)) * ybw + px * lay.h + (lay.h - 1);
}

// The counts of one restart interval, MCUs [first_mcu, first_mcu + mcu_count), block by block through jo_previous_block:
// what je_encode_segment codes of the same arguments
template <class Sink>
JEE_HD void jo_count_segment(const int16_t* coef, const JeLayout& lay, int mcu_cols, int mcu_rows, int ri, int first_mcu,
                             int mcu_count, Sink& sink) {
    const JeQuad* blocks = reinterpret_cast<const JeQuad*>(coef);
    const long ybw = (long)mcu_cols * lay.h, ny = ybw * mcu_rows * lay.v, nc = (long)mcu_cols * mcu_rows;
    for (int m = 0; m < mcu_count; ++m) {
        const long mcu = (long)first_mcu + m;
        if (mcu < 0 || mcu >= nc) break;
        const long my = mcu / mcu_cols, mx = mcu - my * mcu_cols;
        for (int c = 0; c <= lay.nc && c < 3; ++c) {
            const int nv = c == 0 ? lay.v : 1, nh = c == 0 ? lay.h : 1;
            for (int v = 0; v < nv; ++v)
                for (int h = 0; h < nh; ++h) {
                    const long b = c == 0 ? (my * lay.v + v) * ybw + mx * lay.h + h : ny + (c - 1) * nc + mcu;
                    int id = 0;
                    const long p = jo_previous_block(b, lay, mcu_cols, mcu_rows, ri, id);
                    const int pred = p < 0 ? 0 : (int16_t)(blocks[p * 8].lo & 0xFFFF);
                    jo_count_block(sink, blocks + b * 8, pred, id);
                }
        }
    }
}

#endif
