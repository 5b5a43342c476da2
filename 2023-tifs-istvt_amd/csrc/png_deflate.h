// DEFLATE (RFC 1951) out, for one band of a PNG file's filtered rows (DESIGN.md "PNG files out"): literals and matches at
// distance 1, one dynamic-Huffman block and an empty stored block, so the band starts and ends on a byte.  __host__
// __device__, as png_inflate.h is: the device runs it with the 64 lanes of one wave, tools/png_deflate_check.cpp runs the
// same code with one lane under sanitizers, clips.png_encode_banded_host is its definition, byte for byte.
//
// The lanes stand across the band's bytes, 64 at a time.  Byte i of a maximal run of equal bytes that began at s has k = i - s:
// k == 0 is a literal; k > 0 and k % 258 == 0 closes a match of 258; the run's last byte closes what is left, r = k % 258: a
// match of r where r >= 3, else r literals.  Tokens closed in this order are the definition's tokens in its order (first byte,
// matches of 258, remainder), a lane needs the run's start (one max-scan, carried from group to group) and the byte behind
// its own, and it holds at most two literals or one match: at most 30 bits.  pd_count_band histograms them, pd_build makes
// both code tables, the block header's bits and the band's size from the histogram, pd_store_band codes them: a prefix sum
// of the lanes' bit counts places every lane's bits in a staging row (LDS on the device), from which whole dwords leave.
//
// What bounds it for any bytes: a count only indexes through pd_length_symbol's 29 rows and a byte; the merging loop runs at
// most n - 1 times over a list that loses a symbol each time and a chain is followed for at most n links, each range-checked; a block header is at most 17 + 57 + 287
// * 14 bits < PD_HEADER_WORDS dwords even if every length cost a code and 7 extra bits; pd_store_band writes exactly
// the bytes [0, pd_build's size) of dst, bytes where a dword would reach outside them.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define PD_HD __host__ __device__ __forceinline__
#else
#define PD_HD inline
#endif

#if defined(__HIP_DEVICE_COMPILE__)
#define PD_LANES 64
#define PD_SYNC() __syncthreads()
#define PD_ADD(p, v) atomicAdd((p), (v))            // on LDS only
#define PD_OR(p, v) atomicOr((p), (v))
#else
#define PD_LANES 1
#define PD_SYNC() ((void)0)
#define PD_ADD(p, v) (*(p) += (v))
#define PD_OR(p, v) (*(p) |= (v))
#endif

#define PD_SYMBOLS 286                     // literals, the end-of-block, 29 lengths
#define PD_SLOTS 288
#define PD_CL_SYMBOLS 19
#define PD_HEADER_WORDS 136                // 17 + 57 + 287 * 14 = 4092 bits at the very most; a real header is under 2100
#define PD_ADLER 65521u

// a band's row in the scratch, ints: the literal/length code words (bit-reversed code << 8 | length, ready for a stream that
// fills bytes from the low end), the header's bits, then PD_META
#define PD_ROW_WORDS 0
#define PD_ROW_HEADER PD_SLOTS
#define PD_ROW_META (PD_SLOTS + PD_HEADER_WORDS)
#define PD_ROW_INTS (PD_ROW_META + 8)      // 432 ints = 1728 bytes
#define PD_META_HEADER_BITS 0
#define PD_META_BYTES 1                    // the band in the stream, its empty stored block included
#define PD_META_ADLER_A 2                  // sum of the band's bytes mod 65521
#define PD_META_ADLER_B 3                  // sum of (length - i) * byte i mod 65521
#define PD_META_LENGTH 4                   // the band's filtered bytes
#define PD_META_DIST 5                     // the distance code's one word: code 0, one bit
#define PD_META_OFFSET 6                   // where the band begins in the stream (the prefix sum writes it)

struct PdWork {
    uint32_t counts[PD_SLOTS];             // literal/length counts
    uint32_t freq[PD_SLOTS];
    int16_t others[PD_SLOTS], live[PD_SLOTS];
    uint16_t size[PD_SLOTS];
    uint16_t bits[PD_SLOTS + 2];
    uint8_t lens[PD_SLOTS];                // literal/length lengths, then the sequence sent: [0, hlit) and the distance's 1
    uint32_t clcounts[PD_CL_SYMBOLS];
    uint8_t cllens[PD_CL_SYMBOLS];
    uint32_t clwords[PD_CL_SYMBOLS];
    uint32_t words[PD_SLOTS];
    uint32_t header[PD_HEADER_WORDS];
    int header_bits, band_bytes;
};

struct PdStage {
    uint32_t words[PD_SLOTS];              // the literal/length code words of the band
    uint32_t stage[68];                    // 32 bits carried + 64 lanes x 32 bits + one word of spill
};

// ---- the lanes of a wave; one lane on the host -------------------------------------------------------------------------------
PD_HD int pd_scan_max(int v, int lane) {   // inclusive
#if defined(__HIP_DEVICE_COMPILE__)
    for (int d = 1; d < 64; d <<= 1) {
        const int o = __shfl_up(v, d);
        if (lane >= d && o > v) v = o;
    }
#endif
    (void)lane;
    return v;
}

PD_HD int pd_scan_add(int v, int lane) {   // inclusive
#if defined(__HIP_DEVICE_COMPILE__)
    for (int d = 1; d < 64; d <<= 1) {
        const int o = __shfl_up(v, d);
        if (lane >= d) v += o;
    }
#endif
    (void)lane;
    return v;
}

PD_HD int pd_last(int v) {                 // the last lane's value
#if defined(__HIP_DEVICE_COMPILE__)
    return __shfl(v, 63);
#else
    return v;
#endif
}

PD_HD uint32_t pd_sum(uint32_t v) {        // over the lanes
#if defined(__HIP_DEVICE_COMPILE__)
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d);
#endif
    return v;
}

// ---- tokens --------------------------------------------------------------------------------------------------------------------
// a match length 3..258 -> its symbol 257..285, the extra bits and their count; 258 is symbol 285
PD_HD int pd_length_symbol(int L, int* extra, int* ebits) {
    const uint16_t lbase[29] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258};
    const uint8_t lext[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};
    int k = 28;
    while (k > 0 && lbase[k] > L) --k;
    *extra = L - lbase[k];
    *ebits = lext[k];
    return 257 + k;
}

PD_HD int pd_length_extra_bits(int sym) {  // of a symbol 257..285
    const int k = sym - 257;
    return (k < 8 || k >= 28) ? 0 : (k - 4) >> 2;
}

// What byte i of the band closes: `times` literals of `byte` (0, 1 or 2), or one match of `match` bytes (0: none).  start: the
// running carry, the first byte of the run that the previous group ended in (-1 at the band's start).
struct PdToken {
    int byte, times, match;
};

PD_HD PdToken pd_lane_token(const uint8_t* band, int nb, int i, int& start, int lane) {
    PdToken t;
    t.byte = 0;
    t.times = 0;
    t.match = 0;
    const bool valid = i < nb;
    int b = 0, s = -1;
    bool end = false;
    if (valid) {
        b = band[i];
        if (i == 0 || band[i - 1] != b) s = i;
        end = i == nb - 1 || band[i + 1] != b;
    }
    s = pd_scan_max(s, lane);
    if (start > s) s = start;
    start = pd_last(s);
    if (!valid) return t;
    const int k = i - s;
    t.byte = b;
    if (k == 0) {
        t.times = 1;
    } else if (k % 258 == 0) {
        t.match = 258;
    } else if (end) {
        const int r = k % 258;
        if (r >= 3)
            t.match = r;
        else
            t.times = r;
    }
    return t;
}

// The histogram of a band (counts[0 .. PD_SLOTS) zeroed by the caller, synchronised behind) and its Adler-32 parts
PD_HD void pd_count_band(const uint8_t* band, int nb, uint32_t* counts, uint32_t* adler_a, uint32_t* adler_b, int lane) {
    int start = -1;
    uint64_t sa = 0, sb = 0;                                      // 64 bits: right for one lane and a band of 2^30 bytes too
    for (int g = 0; g < nb; g += PD_LANES) {
        const int i = g + lane;
        const PdToken t = pd_lane_token(band, nb, i, start, lane);
        if (t.times) PD_ADD(&counts[t.byte & 255], (uint32_t)t.times);
        if (t.match) {
            int e, eb;
            PD_ADD(&counts[pd_length_symbol(t.match, &e, &eb)], 1u);
        }
        if (i < nb) {
            sa += (uint32_t)t.byte;
            sb += (uint64_t)((uint32_t)(nb - i) % PD_ADLER) * (uint32_t)t.byte;
        }
    }
    *adler_a = pd_sum((uint32_t)(sa % PD_ADLER)) % PD_ADLER;
    *adler_b = pd_sum((uint32_t)(sb % PD_ADLER)) % PD_ADLER;
    PD_SYNC();
}

// ---- code tables: one lane -----------------------------------------------------------------------------------------------------
// counts[0 .. n) -> lens[0 .. n), at most `limit` bits and complete where two symbols or more have a count; the rule of
// clips._png_code_lengths, step by step
PD_HD void pd_code_lengths(const uint32_t* counts, int n, int limit, uint8_t* lens, PdWork& w) {
    int live = 0;
    for (int s = 0; s < n; ++s) {
        lens[s] = 0;
        w.freq[s] = counts[s];
        w.others[s] = -1;
        w.size[s] = 0;
        if (counts[s]) w.live[live++] = (int16_t)s;
    }
    if (live < 2) {
        if (live == 1) lens[w.live[0]] = 1;
        return;
    }
    // one pass finds the best and the second best of the live list, "better" being the smaller count and, of equal counts, the
    // larger symbol: the definition's two picks.  The list shrinks by the symbol merged away, so its order does not matter.
    int listed = live;
    for (int merge = 0; merge < n - 1 && listed > 1; ++merge) {
        int c1 = -1, c2 = -1;
        uint32_t v1 = 0xffffffffu, v2 = 0xffffffffu;
        for (int p = 0; p < listed; ++p) {
            const int s = w.live[p];
            const uint32_t f = w.freq[s];
            if (f < v1 || (f == v1 && s > c1)) {
                v2 = v1, c2 = c1;
                v1 = f, c1 = s;
            } else if (f < v2 || (f == v2 && s > c2)) {
                v2 = f, c2 = s;
            }
        }
        if (c1 < 0 || c2 < 0) break;
        w.freq[c1] += w.freq[c2];                                 // the counts of a band sum to less than 2^31
        w.freq[c2] = 0;
        int tail = c1;
        for (int side = 0; side < 2; ++side) {
            int c = side ? c2 : c1;
            for (int step = 0; step < n; ++step) {
                if (w.size[c] < n) ++w.size[c];
                const int next = w.others[c];
                if (next < 0 || next >= n) break;
                c = next;
            }
            if (side == 0) tail = c;
        }
        w.others[tail] = (int16_t)c2;                             // the chain of c2 behind the chain of c1
        for (int p = 0; p < listed; ++p)                            // c2 leaves the list
            if (w.live[p] == c2) {
                w.live[p] = w.live[listed - 1];
                break;
            }
        --listed;
    }
    for (int l = 0; l < n + 2; ++l) w.bits[l] = 0;
    int longest = 0;
    for (int s = 0; s < n; ++s)
        if (counts[s]) {
            ++w.bits[w.size[s]];
            if (w.size[s] > longest) longest = w.size[s];
        }
    for (int i = n; i > limit; --i) {
        for (int guard = 0; guard < n && w.bits[i] > 1; ++guard) {
            int j = i - 2;
            while (j > 0 && w.bits[j] == 0) --j;
            if (j == 0) break;
            w.bits[i] -= 2;
            w.bits[i - 1] += 1;
            w.bits[j + 1] += 2;
            w.bits[j] -= 1;
        }
    }
    // the symbols by (length before the limit, symbol) take the lengths of bits[] in ascending order
    int l = 1, left = w.bits[1];
    const int top = limit < n ? limit : n;
    for (int size = 1; size <= longest; ++size)
        for (int s = 0; s < n; ++s) {
            if (!counts[s] || w.size[s] != size) continue;
            while (left == 0 && l < top) left = w.bits[++l];
            if (left == 0) return;
            lens[s] = (uint8_t)l;
            --left;
        }
}

PD_HD uint32_t pd_reverse(uint32_t code, int len) {
    uint32_t r = 0;
    for (int i = 0; i < len; ++i) r |= ((code >> i) & 1u) << (len - 1 - i);
    return r;
}

// RFC 1951 3.2.2 -> words[s] = bit-reversed code << 8 | length, 0 for a symbol without a code
PD_HD void pd_code_words(const uint8_t* lens, int n, uint32_t* words) {
    uint32_t count[16], next[16];
    for (int i = 0; i < 16; ++i) count[i] = 0;
    for (int s = 0; s < n; ++s) ++count[lens[s] & 15];
    count[0] = 0;
    uint32_t code = 0;
    next[0] = 0;
    for (int l = 1; l < 16; ++l) {
        code = (code + count[l - 1]) << 1;
        next[l] = code;
    }
    for (int s = 0; s < n; ++s) {
        const int l = lens[s] & 15;
        words[s] = l ? (pd_reverse(next[l]++, l) << 8) | (uint32_t)l : 0u;
    }
}

PD_HD void pd_put(uint32_t* words, int& nbits, uint32_t v, int k) {       // k <= 16 bits, words zeroed beforehand
    if (k == 0 || nbits + k > 32 * PD_HEADER_WORDS) return;
    const int at = nbits >> 5, sh = nbits & 31;
    words[at] |= v << sh;
    if (sh + k > 32) words[at + 1] |= v >> (32 - sh);
    nbits += k;
}

// the lengths seq[0 .. n) as code-length symbols, greedy from the left (clips._png_length_tokens): sink(symbol, extra, bits)
template <class Sink> PD_HD void pd_length_tokens(const uint8_t* seq, int n, Sink& sink) {
    int i = 0;
    while (i < n) {
        int j = i;
        while (j < n && seq[j] == seq[i]) ++j;
        const int v = seq[i];
        int r = j - i;
        if (v == 0) {
            while (r >= 11) {
                const int k = r < 138 ? r : 138;
                sink.put(18, k - 11, 7);
                r -= k;
            }
            if (r >= 3) {
                sink.put(17, r - 3, 3);
                r = 0;
            }
        } else {
            sink.put(v, 0, 0);
            r -= 1;
            while (r >= 3) {
                const int k = r < 6 ? r : 6;
                sink.put(16, k - 3, 2);
                r -= k;
            }
        }
        for (; r > 0; --r) sink.put(v, 0, 0);
        i = j;
    }
}

struct PdClCount {
    uint32_t* counts;
    PD_HD void put(int s, int, int) { ++counts[s]; }
};

struct PdClWrite {
    const uint32_t* clwords;
    uint32_t* header;
    int nbits;
    PD_HD void put(int s, int extra, int k) {
        pd_put(header, nbits, clwords[s] >> 8, (int)(clwords[s] & 255));
        pd_put(header, nbits, (uint32_t)extra, k);
    }
};

// counts (the end-of-block not yet among them) -> w.words, w.header / w.header_bits, w.band_bytes.  One lane.
PD_HD void pd_build(PdWork& w) {
    const uint8_t order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    for (int s = PD_SYMBOLS; s < PD_SLOTS; ++s) w.counts[s] = 0;
    w.counts[256] = 1;
    pd_code_lengths(w.counts, PD_SYMBOLS, 15, w.lens, w);
    pd_code_words(w.lens, PD_SYMBOLS, w.words);
    for (int s = PD_SYMBOLS; s < PD_SLOTS; ++s) w.words[s] = 0;
    int hlit = PD_SYMBOLS;
    while (hlit > 257 && w.lens[hlit - 1] == 0) --hlit;
    long bits = 0;                                                // the tokens: counts are the band's, lengths <= 15
    for (int s = 0; s < PD_SYMBOLS; ++s)
        bits += (long)w.counts[s] * (w.lens[s] + (s > 256 ? pd_length_extra_bits(s) + 1 : 0));
    w.lens[hlit] = 1;                                             // the distance code: symbol 0, one bit
    const int nseq = hlit + 1;
    for (int s = 0; s < PD_CL_SYMBOLS; ++s) w.clcounts[s] = 0;
    PdClCount count = {w.clcounts};
    pd_length_tokens(w.lens, nseq, count);
    pd_code_lengths(w.clcounts, PD_CL_SYMBOLS, 7, w.cllens, w);
    pd_code_words(w.cllens, PD_CL_SYMBOLS, w.clwords);
    int hclen = 19;
    while (hclen > 4 && w.cllens[order[hclen - 1]] == 0) --hclen;
    for (int i = 0; i < PD_HEADER_WORDS; ++i) w.header[i] = 0;
    PdClWrite out = {w.clwords, w.header, 0};
    pd_put(w.header, out.nbits, 0u, 1);                           // BFINAL
    pd_put(w.header, out.nbits, 2u, 2);                           // BTYPE: dynamic
    pd_put(w.header, out.nbits, (uint32_t)(hlit - 257), 5);
    pd_put(w.header, out.nbits, 0u, 5);                           // HDIST: one distance code
    pd_put(w.header, out.nbits, (uint32_t)(hclen - 4), 4);
    for (int i = 0; i < hclen; ++i) pd_put(w.header, out.nbits, w.cllens[order[i]], 3);
    pd_length_tokens(w.lens, nseq, out);
    w.header_bits = out.nbits;
    bits += out.nbits + 3;                                        // and the empty stored block's three bits
    w.band_bytes = (int)((bits + 7) >> 3) + 4;
}

// ---- the bit writer: the lanes' bits in lane order -----------------------------------------------------------------------------
struct PdOut {
    uint8_t* base;                         // dst rounded down to 4 bytes: bit positions count from here
    uint32_t* stage;
    long pos;                              // bits so far, the head's included
    long word0;                            // dwords that have left
    int head;                              // dst - base: these bytes are another band's and are never written
};

PD_HD void pd_out_begin(PdOut& o, uint8_t* dst, uint32_t* stage, int lane) {
    o.head = (int)(reinterpret_cast<uintptr_t>(dst) & 3);
    o.base = dst - o.head;
    o.stage = stage;
    o.pos = 8 * o.head;
    o.word0 = 0;
    for (int i = lane; i < 68; i += PD_LANES) stage[i] = 0;
    PD_SYNC();
}

// every lane hands `n` <= 32 bits (0: none); uniform call
PD_HD void pd_out_append(PdOut& o, uint32_t v, int n, int lane) {
    const int incl = pd_scan_add(n, lane);
    const int total = pd_last(incl);
    if (n > 0) {
        const long p = o.pos - 32 * o.word0 + (incl - n);         // < 32 + 63 * 32
        const int at = (int)(p >> 5), sh = (int)(p & 31);
        const uint64_t wide = (uint64_t)v << sh;
        PD_OR(&o.stage[at], (uint32_t)wide);
        if (wide >> 32) PD_OR(&o.stage[at + 1], (uint32_t)(wide >> 32));
    }
    o.pos += total;
    PD_SYNC();
    const int full = (int)((o.pos >> 5) - o.word0);               // <= 64 on the device, <= 1 on the host
    for (int i = lane; i < full; i += PD_LANES) {
        const uint32_t word = o.stage[i];
        uint8_t* q = o.base + 4 * (o.word0 + i);
        if (o.word0 + i == 0 && o.head) {
            for (int k = o.head; k < 4; ++k) q[k] = (uint8_t)(word >> (8 * k));
        } else {
            *reinterpret_cast<uint32_t*>(q) = word;
        }
    }
    const uint32_t carry0 = o.stage[full], carry1 = o.stage[full + 1];
    PD_SYNC();
    for (int i = lane; i < 68; i += PD_LANES) o.stage[i] = i == 0 ? carry0 : (i == 1 ? carry1 : 0u);
    o.word0 += full;
    PD_SYNC();
}

// the band ends on a byte: the bytes of the last, partial dword leave one by one
PD_HD void pd_out_end(PdOut& o, int lane) {
    const int rest = (int)((o.pos - 32 * o.word0) >> 3);
    if (lane == 0) {
        const uint32_t word = o.stage[0];
        uint8_t* q = o.base + 4 * o.word0;
        for (int k = (o.word0 == 0 ? o.head : 0); k < rest; ++k) q[k] = (uint8_t)(word >> (8 * k));
    }
}

// One band's bytes: the header's bits, the tokens, the end-of-block, the empty stored block -> dst[0 .. band_bytes).
// words: the band's code words (PdStage::words on the device); header: header_bits bits in dwords.
PD_HD void pd_store_band(const uint8_t* band, int nb, int final, const uint32_t* words, const uint32_t* header, int header_bits,
                         uint8_t* dst, uint32_t* stage, int lane) {
    PdOut o;
    pd_out_begin(o, dst, stage, lane);
    for (int g = 0; 32 * g < header_bits; g += PD_LANES) {
        const int left = header_bits - 32 * (g + lane);
        const int n = left <= 0 ? 0 : (left < 32 ? left : 32);
        pd_out_append(o, n > 0 ? header[g + lane] : 0u, n, lane);
    }
    int start = -1;
    for (int g = 0; g < nb; g += PD_LANES) {
        const PdToken t = pd_lane_token(band, nb, g + lane, start, lane);
        uint32_t v = 0;
        int n = 0;
        if (t.times) {
            const uint32_t cw = words[t.byte & 255];
            const int len = (int)(cw & 255);
            v = cw >> 8;
            n = len;
            if (t.times == 2) {
                v |= v << len;
                n = 2 * len;
            }
        } else if (t.match) {
            int e, eb;
            const uint32_t cw = words[pd_length_symbol(t.match, &e, &eb)];
            const int len = (int)(cw & 255);
            v = (cw >> 8) | ((uint32_t)e << len);                 // and the distance code: one zero bit
            n = len + eb + 1;
        }
        pd_out_append(o, v, n, lane);
    }
    // the end-of-block, BFINAL and type 00 of the stored block, zeros up to the byte; then LEN = 0 and its complement
    const uint32_t eob = words[256];
    const int len = (int)(eob & 255);
    uint32_t v = 0;
    int n = 0;
    if (lane == 0) {
        v = (eob >> 8) | ((uint32_t)(final ? 1 : 0) << len);
        n = len + 3;
        n += (int)((8 - ((o.pos + n) & 7)) & 7);
    }
    if (PD_LANES > 1) {
        if (lane == 1) v = 0xffff0000u, n = 32;
        pd_out_append(o, v, n, lane);
    } else {
        pd_out_append(o, v, n, lane);
        pd_out_append(o, 0xffff0000u, 32, lane);
    }
    pd_out_end(o, lane);
}

// ---- the container's checksums ---------------------------------------------------------------------------------------------------
// Adler-32 of a stream that grows by a block of `len` bytes with its own sums (a, b): A, B are the running pair, A from 1
PD_HD void pd_adler_append(uint32_t& A, uint32_t& B, uint32_t a, uint32_t b, uint32_t len) {
    B = (uint32_t)((B + (uint64_t)(len % PD_ADLER) * A + b) % PD_ADLER);
    A = (A + a) % PD_ADLER;
}

#define PD_CRC_POLY 0xedb88320u

PD_HD uint32_t pd_crc_entry(uint32_t i) {  // row i of the byte table
    for (int k = 0; k < 8; ++k) i = (i & 1u) ? (i >> 1) ^ PD_CRC_POLY : i >> 1;
    return i;
}

// a(x) b(x) mod P in the reflected representation (bit 31 is x^0)
PD_HD uint32_t pd_crc_multiply(uint32_t a, uint32_t b) {
    uint32_t p = 0;
    for (int i = 31; i >= 0; --i) {
        if ((a >> i) & 1u) p ^= b;
        b = (b & 1u) ? (b >> 1) ^ PD_CRC_POLY : b >> 1;
    }
    return p;
}

PD_HD uint32_t pd_crc_shift(uint64_t nbytes) {    // x^(8 nbytes) mod P
    uint32_t p = 0x80000000u, sq = 0x00800000u;  // x^0, x^8
    while (nbytes) {
        if (nbytes & 1u) p = pd_crc_multiply(sq, p);
        sq = pd_crc_multiply(sq, sq);
        nbytes >>= 1;
    }
    return p;
}

// crc(A | B) of the finished CRC-32s of A and B, B of len_b bytes, shift = pd_crc_shift(len_b): zlib's crc32_combine
PD_HD uint32_t pd_crc_combine(uint32_t crc_a, uint32_t crc_b, uint32_t shift) { return pd_crc_multiply(shift, crc_a) ^ crc_b; }
