// A restart interval decoded from several start points at once (DESIGN.md "JPEG files without restart markers"): the
// pieces that the split entropy kernel (jpeg.hip) and a host program (tools/jpeg_entropy_split_check.cpp, built with
// sanitizers) both compile.  clips.jpeg_split_host is the same steps on the host and the definition of the state table.
//
// The interval's bytes [begin, end) are cut into S chunks of `chunk` bytes; lane i owns the symbols (a Huffman code and its
// extra bits) that start in bytes [begin + i * chunk, begin + (i + 1) * chunk), the last lane everything from its boundary
// on.  The entry state of lane i is the decoder's position at the first symbol that starts at or after its boundary:
//     pos  the raw index of the byte that holds the next bit (never the stuffed 00 behind an FF; past `end` the zeros that
//          are fed count on as bytes end, end + 1, ...)
//     bit  bits of that byte already taken, 0..7
//     blk  the block within the MCU, 0..5 at 4:2:0, 0..2 at 4:4:4, 0..3 at 4:2:2 and 0 for greyscale
//     k    the coefficient index the next symbol continues at; 0: the next symbol is a DC code
// Lane 0 knows its state, (begin, 0, 0, 0); every other lane starts from js_guess and the states are relaxed: in every round
// lane i runs js_chunk from the exit state lane i - 1 had in the round before.  After round r the states of lanes 0..r are
// the sequential decoder's, so the fixed point is the sequential decode whatever the guesses were.
//
// js_chunk is lenient, so that it cannot die on the bits a wrong state shows it: a prefix no code matches takes 16 bits and
// counts as the value 0, a DC category above 11 counts as 0, a run past 63 ends the block.  Up to the first of these it is
// je_block's decode, and up to there it also keeps the strict tallies: blocks started, the DC predictions from 0, the first
// error.  js_write is je_block again from a converged state, between the lane's boundaries, with stores.
//
// The rules of jpeg_entropy.h hold: bytes are read behind pos < end only, a symbol takes 1..32 bits so a chunk is a bounded
// loop, at most 64 symbols go into a block, and no address is made from a decoded value: a block's place comes from its
// number, which is counted.
#ifndef ISTVT_JPEG_ENTROPY_SPLIT_H
#define ISTVT_JPEG_ENTROPY_SPLIT_H

#include "jpeg_entropy.h"

// A reader that knows where it is.  Three bytes wait in win (un-stuffed; zeros past the end); p0, p1, p2 are their raw
// indices and p3 the next to fetch, so the position of the next bit is (p0, bit) at any time and a reader can be opened there.
struct JsBits {
    const uint8_t* data;
    long end;
    long p0, p1, p2, p3;
    uint32_t win;      // 24 bits
    int bit;           // bits of the byte at p0 already taken, 0..7
    int status;        // 1 once a bit of a fed zero has been taken
};

struct JsState {
    long pos;
    int bit, blk, k;
};

// what a lane's strict decode of its chunk amounts to, up to its first error
struct JsTally {
    int blocks;        // blocks whose DC code starts in the chunk
    int err;           // 0, or 2 / 3 as je_block names them
    int pred[3];       // the DC predictions from 0, in the int16 a coefficient has
};

// The chunk rule (clips.jpeg_split_plan): an interval of `length` bytes is cut into chunks of max(chunk_bytes, ceil(length /
// JS_LANES)) bytes, at least one and at most JS_LANES of them; the last ends with the interval.
constexpr int JS_LANES = 256;
JE_HD long js_chunk_bytes(long length, int chunk_bytes) {
    const long even = (length + JS_LANES - 1) / JS_LANES;
    return even > chunk_bytes ? even : chunk_bytes;
}
JE_HD int js_chunks(long length, int chunk_bytes) {
    const long c = js_chunk_bytes(length, chunk_bytes), n = (length + c - 1) / c;
    return n < 1 ? 1 : (int)n;
}

// Where the S state rows of segment s, whose bytes start at `begin`, lie in the table behind the statuses -> its first
// row, or -1 where they do not fit.  Two addressings:
//   by byte offset (STRIDED = false)  row begin / chunk_bytes + s of a table of `rows` rows.  Segments lie in order in the
//       bytes and a segment has at most length / chunk_bytes + 1 chunks, so the rows of two segments never meet and the
//       table of a call over nbytes has nbytes / chunk_bytes + nseg rows: the batch call (istvt_jpeg_decode_split_u8).
//   per segment (STRIDED = true)  `rows` is the row stride R, and segment s owns rows [s * R, (s + 1) * R) of a table of
//       nseg * R rows whatever its bytes' place: the bank's calls, whose bytes are a whole set but whose segments are the few
//       drawn.  A segment of more than R chunks does not fit.
template <bool STRIDED> JE_HD long js_row0(long begin, int chunk_bytes, int s, int S, long rows) {
    if (STRIDED) return s >= 0 && S >= 1 && S <= rows ? (long)s * rows : -1;
    const long row0 = begin / chunk_bytes + s;
    return row0 >= 0 && row0 + S <= rows ? row0 : -1;
}

JE_HD bool js_same(const JsState& a, const JsState& b) { return a.pos == b.pos && a.bit == b.bit && a.blk == b.blk && a.k == b.k; }

// the byte at p (FF 00 is the byte FF, zeros past the end) and p moved behind it
JE_HD uint32_t js_fetch(const uint8_t* data, long end, long& p) {
    uint32_t b = 0;
    if (p < end) {
        b = data[p++];
        if (b == 0xFF && p < end && data[p] == 0) ++p;
    } else {
        ++p;
    }
    return b;
}

JE_HD void js_open(JsBits& s, const uint8_t* data, long end, long pos, int bit) {
    s.data = data, s.end = end, s.bit = bit & 7, s.status = 0;
    s.p0 = s.p1 = pos;
    uint32_t w = js_fetch(data, end, s.p1);
    s.p2 = s.p1;
    w = (w << 8) | js_fetch(data, end, s.p2);
    s.p3 = s.p2;
    s.win = (w << 8) | js_fetch(data, end, s.p3);
}

// 1 <= k <= 16 bits taken
JE_HD void js_skip(JsBits& s, int k) {
    long last = s.p0;                       // the byte of the last bit taken
    s.bit += k;
    while (s.bit >= 8) {
        last = s.p0;
        s.p0 = s.p1, s.p1 = s.p2, s.p2 = s.p3;
        s.win = ((s.win << 8) | js_fetch(s.data, s.end, s.p3)) & 0xFFFFFFu;
        s.bit -= 8;
    }
    if (s.bit > 0) last = s.p0;
    if (last >= s.end) s.status = 1;
}

// je_huffman: the next symbol of table t, or -1 (and nothing taken) where the next 16 bits start no code
JE_HD int js_huffman(JsBits& s, const int* t) {
    const int c = (int)((s.win >> (8 - s.bit)) & 0xFFFF);
    for (int l = 1; l <= 16; ++l) {
        if (c < t[l - 1]) {
            js_skip(s, l);
            return t[32 + ((t[16 + l - 1] + (c >> (16 - l))) & 255)] & 255;
        }
    }
    return -1;
}

// je_receive: 1 <= size <= 15 bits as a signed value
JE_HD int js_receive(JsBits& s, int size) {
    const int r = (int)((s.win >> (24 - s.bit - size)) & ((1u << size) - 1));
    js_skip(s, size);
    return r >= (1 << (size - 1)) ? r : r - (1 << size) + 1;
}

// blocks of an MCU, and the component of block blk of an MCU
JE_HD int js_mcu_blocks(const JeLayout& lay) { return lay.h * lay.v + lay.nc; }
JE_HD int js_component(const JeLayout& lay, int blk) { return blk < lay.h * lay.v ? 0 : blk - lay.h * lay.v + 1; }

// Where block number cur of an interval that starts at MCU first_mcu lies, as je_decode_segment counts the blocks: the
// writer's name for it; c: its component
template <class Writer> JE_HD long js_place(const JeLayout& lay, int mcu_cols, int first_mcu, long cur, Writer& w, int& c) {
    const int nblk = js_mcu_blocks(lay);     // 6, 3, 4 or 1 (je_layout): no division by a variable
    const long q = nblk == 6 ? cur / 6 : nblk == 4 ? cur >> 2 : nblk == 3 ? cur / 3 : cur;
    const int mcu = first_mcu + (int)q, j = (int)(cur - q * nblk);
    const int my = mcu / mcu_cols, mx = mcu - my * mcu_cols;
    c = js_component(lay, j);
    if (c != 0) return w.block(c, my, mx);
    return lay.h == 2 ? w.block(0, my * lay.v + (j >> 1), mx * 2 + (j & 1)) : w.block(0, my * lay.v + j, mx);
}

// The guess of lane i >= 1: its boundary, stepped past a stuffed 00, at the start of an MCU
JE_HD JsState js_guess(const uint8_t* data, long begin, long end, long boundary) {
    JsState g = {boundary, 0, 0, 0};
    if (boundary > begin && boundary < end && data[boundary - 1] == 0xFF && data[boundary] == 0) g.pos = boundary + 1;
    return g;
}

// The lenient transition of one lane: symbols from state `in` while they start before `limit` (<= end) -> the exit state.
// t: the strict tallies of the same symbols, frozen at the first error.
JE_HD JsState js_chunk(const uint8_t* data, long end, long limit, const int* const* huff, const JeLayout& lay,
                       const JsState& in, JsTally& t) {
    JsBits s;
    js_open(s, data, end, in.pos, in.bit);
    const int nblk = js_mcu_blocks(lay);
    int blk = in.blk < 0 || in.blk >= nblk ? 0 : in.blk, k = in.k & 63;
    t.blocks = t.err = 0;
    t.pred[0] = t.pred[1] = t.pred[2] = 0;
    while (s.p0 < limit) {
        const int c = js_component(lay, blk);
        bool done = false;                  // the block ends with this symbol
        if (k == 0) {
            int size = js_huffman(s, huff[2 * c]);
            if (size < 0) js_skip(s, 16);
            if (!t.err) ++t.blocks;
            if (size < 0 || size > 11) {
                if (!t.err) t.err = 2;
                size = 0;
            }
            if (size) {
                const int diff = js_receive(s, size);
                if (!t.err) t.pred[c] = (int16_t)(t.pred[c] + diff);
            }
            k = 1;
        } else {
            int rs = js_huffman(s, huff[2 * c + 1]);
            if (rs < 0) {
                js_skip(s, 16);
                if (!t.err) t.err = 2;
                rs = 0;
            }
            const int r = rs >> 4, size = rs & 15;
            if (size == 0) {
                if (r != 15) {
                    done = true;
                } else {
                    k += 16;
                    if (k > 64 && !t.err) t.err = 3;
                    done = k >= 64;
                }
            } else {
                k += r;
                if (k > 63) {
                    if (!t.err) t.err = 3;
                    done = true;
                } else {
                    js_skip(s, size);
                    done = ++k == 64;
                }
            }
        }
        if (done) {
            k = 0;
            blk = blk + 1 == nblk ? 0 : blk + 1;
        }
    }
    const JsState out = {s.p0, s.bit, blk, k};
    return out;
}

// The strict decode of one lane with stores: je_block's steps from the converged state `in`, on the symbols that start before
// `limit`, or with last = true until block `total` of the interval would start.  `next` is the number, within the interval,
// of the next block to start (the sum of the tallies of the lanes in front) and pred the predictions summed the same way; a
// block's place is counted from first_mcu and its number as je_decode_segment counts it.  The blocks are zero on entry.
// -> the largest of the error (2, 3) and status 1; started: the blocks this lane started
template <class Writer>
JE_HD int js_write(const uint8_t* data, long end, long limit, bool last, const int* const* huff, const JeLayout& lay,
                   int mcu_cols, int first_mcu, long total, const JsState& in, long next, const int* pred_in, Writer& w,
                   int& started) {
    JsBits s;
    js_open(s, data, end, in.pos, in.bit);
    int pred[3] = {pred_in[0], pred_in[1], pred_in[2]};
    int k = in.k & 63, c = 0;
    long block = -1;                        // where the block in progress lies; -1: nowhere, its coefficients are dropped
    started = 0;
    if (k > 0 && next >= 1 && next <= total) {
        block = js_place(lay, mcu_cols, first_mcu, next - 1, w, c);         // the block lane i - 1 left unfinished
    } else if (k > 0) {
        return 0;                           // no state of a sound walk: nothing in front that a block could continue
    }
    while (last || s.p0 < limit) {
        if (k == 0) {
            if (next >= total) break;
            block = js_place(lay, mcu_cols, first_mcu, next++, w, c);
            ++started;
            const int size = js_huffman(s, huff[2 * c]);
            if (size < 0 || size > 11) return 2;
            if (size) pred[c] = (int16_t)(pred[c] + js_receive(s, size));
            w.put(block, 0, pred[c]);
            k = 1;
            continue;
        }
        const int rs = js_huffman(s, huff[2 * c + 1]);
        if (rs < 0) return 2;
        const int r = rs >> 4, size = rs & 15;
        if (size == 0) {
            if (r != 15) {
                k = 0;
                continue;
            }
            k += 16;
            if (k > 64) return 3;
            if (k == 64) k = 0;
            continue;
        }
        k += r;
        if (k > 63) return 3;
        w.put(block, je_zigzag(k), js_receive(s, size));
        if (++k == 64) k = 0;
    }
    return s.status;
}

#endif
