// DEFLATE (RFC 1951) for one stream into a buffer whose exact length is known beforehand: the inflate of a PNG file's IDAT
// stream (DESIGN.md "PNG files").  Written from the RFC.  __host__ __device__: the device runs it with the 64 lanes of one
// wave, tools/png_inflate_check.cpp runs the same code with one lane under sanitizers, clips._png_inflate is its definition.
//
// Every lane of the wave holds the same decoder state (bit reader, position, tables' contents): symbol decoding is uniform,
// and the lanes differ only where bytes are stored -- literals are gathered, one per lane, and stored together; a match is
// copied by the lanes together, out[pos + i] = out[pos - D + (i mod D)], which reads only bytes in front of pos and so is
// right for D < L too.  A match may read what other lanes stored for an earlier symbol: pi_fence() orders the two at
// workgroup scope, and is only reached when the source range touches bytes stored since the last fence.
//
// Status (the first fault in stream order decides; clips.PNG_STATUS words them): 0 fine | 1 the stream ends early | 2 a
// reserved block type, or LEN != ~NLEN | 3 code lengths over-subscribed or incomplete, or a code no table holds | 4 a distance
// beyond the bytes produced | 5 more, or fewer, bytes than expected.  A stored block checks 2, then 5, then 1.
//
// The band mode (pi_inflate<true>, clips.png_decode_bands_host is its definition): [begin, end) is one band of a file whose
// index names its bands, begin any byte, out the band's first output byte and expected its rows' bytes -- so the window, the
// count and the fence bookkeeping are the band's own with no further code.  A band that is not its file's last (middle) gives
// status 7 for a block header with BFINAL set, before the block's type is looked at, and stops behind a stored block that ends
// at byte `end`; the last band stops at its BFINAL block.  Both are tests per block: the symbol loop is the sequential one.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define PI_HD __host__ __device__ __forceinline__
#else
#define PI_HD inline
#endif

#if defined(__HIP_DEVICE_COMPILE__)
#define PI_LANES 64
#define PI_SYNC() __syncthreads()
#else
#define PI_LANES 1
#define PI_SYNC() ((void)0)
#endif

#define PI_OK 0
#define PI_EARLY 1
#define PI_BLOCK 2
#define PI_CODES 3
#define PI_DISTANCE 4
#define PI_LENGTH 5
#define PI_BAND 7                          // 6 is the unfilter's

#define PI_LIT_FAST 10                     // bits of the literal/length lookup; longer codes take the limit scan
#define PI_DIST_FAST 8

// one canonical code: limit[len] is the first 15-bit left-aligned code beyond the codes of `len` bits, offset[len] the index
// in syms of the first symbol of that length minus its code; fast[bits] = symbol << 4 | length for codes of at most
// fast_bits bits, 0 for the others.  One set per wave: in LDS on the device.
struct PiTable {
    uint32_t limit[16];
    int32_t offset[16];
    int32_t err;
};

struct PiTables {
    PiTable cl, lit, dist;
    uint16_t cl_syms[19], lit_syms[288], dist_syms[32];
    uint16_t lit_fast[1 << PI_LIT_FAST], dist_fast[1 << PI_DIST_FAST];
    uint8_t lens[352];                     // [0, 19) the code-length code's, [32, 320) literal/length, [320, 352) distance
};

struct PiBits {
    const uint8_t* data;                   // the base the byte offsets count from; 4-byte aligned on the device
    int begin, p, end;                     // bytes [begin, end) may be read (a band begins at any byte); a batch holds < 2^31
    uint64_t buf;
    int cnt;
#if defined(__HIP_DEVICE_COMPILE__)
    uint32_t chunk;                        // this lane's aligned word of the 256-byte window the reader is in
    int window;
    int lane;
#endif
};

PI_HD uint32_t pi_brev15(uint32_t bits) {  // the next 15 bits of the stream, first bit on top
#if defined(__HIP_DEVICE_COMPILE__)
    return __brev(bits) >> 17;
#else
    uint32_t r = 0;
    for (int i = 0; i < 15; ++i) r |= ((bits >> i) & 1u) << (14 - i);
    return r;
#endif
}

// an aligned word that lies inside [begin, end)
PI_HD uint32_t pi_word(PiBits& r) {
#if defined(__HIP_DEVICE_COMPILE__)
    const int window = r.p & ~255;
    if (window != r.window) {              // the wave loads 256 bytes at once, a word per lane, never outside the stream
        const int at = window + 4 * r.lane;
        r.chunk = (at >= r.begin && r.end - at >= 4) ? *reinterpret_cast<const uint32_t*>(r.data + at) : 0u;
        r.window = window;
    }
    return (uint32_t)__builtin_amdgcn_readlane((int)r.chunk, __builtin_amdgcn_readfirstlane((int)((r.p >> 2) & 63)));
#else
    uint32_t w;                            // the host's base need not be aligned: a checker gives a band a block of its own
    __builtin_memcpy(&w, r.data + r.p, 4);
    return w;
#endif
}

// at least 32 bits in the buffer, or every byte of the stream: the byte range is checked on every load.  Behind a stored
// block the position is rarely a multiple of 4: at most 3 single bytes bring it back to one, then words are loaded again.
PI_HD void pi_refill(PiBits& r) {
    if (r.cnt > 32) return;
    while ((r.p & 3) && r.p < r.end) {     // cnt <= 32 + 24
        r.buf |= (uint64_t)r.data[r.p] << r.cnt;
        r.cnt += 8;
        r.p += 1;
    }
    if (r.end - r.p >= 4) {
        if (r.cnt <= 32) {
            r.buf |= (uint64_t)pi_word(r) << r.cnt;
            r.cnt += 32;
            r.p += 4;
        }
    } else {
        while (r.cnt <= 56 && r.p < r.end) {
            r.buf |= (uint64_t)r.data[r.p] << r.cnt;
            r.cnt += 8;
            r.p += 1;
        }
    }
}

PI_HD uint32_t pi_take(PiBits& r, int n) {  // n <= 16 bits the caller knows are there
    const uint32_t v = (uint32_t)r.buf & ((1u << n) - 1u);
    r.buf >>= n;
    r.cnt -= n;
    return v;
}

PI_HD void pi_fence() {
#if defined(__HIP_DEVICE_COMPILE__)
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
#endif
}

// the code of `n` symbols with lengths lens[0..n): lane 0 builds, the lanes fill the lookup together.  single_ok: the
// one-code (or empty) distance tree that DEFLATE permits.  -> 0 or PI_CODES
PI_HD int pi_build(PiTable* t, uint16_t* syms, uint16_t* fast, int fast_bits, const uint8_t* lens, int n, bool single_ok,
                   int lane) {
    if (lane == 0) {
        int count[16], next[16];
        for (int i = 0; i < 16; ++i) count[i] = 0;
        for (int i = 0; i < n; ++i) count[lens[i]]++;
        int left = 1, used = 0;
        bool over = false;
        for (int len = 1; len < 16; ++len) {
            left = 2 * left - count[len];
            if (left < 0) {
                over = true;
                break;
            }
            used += count[len];
        }
        // incomplete: only a distance code of no symbol at all, or of one symbol of one bit
        const bool fine = !over && (left == 0 || (single_ok && (used == 0 || (used == 1 && count[1] == 1))));
        t->err = fine ? 0 : PI_CODES;
        uint32_t code = 0;
        int index = 0;
        t->limit[0] = 0;
        t->offset[0] = 0;
        for (int len = 1; len < 16; ++len) {
            const int c = fine ? count[len] : 0;
            code <<= 1;
            next[len] = index;
            t->offset[len] = index - (int)code;
            code += (uint32_t)c;
            index += c;
            t->limit[len] = code << (15 - len);
        }
        if (fine)
            for (int i = 0; i < n; ++i)
                if (lens[i]) syms[next[lens[i]]++] = (uint16_t)i;
    }
    PI_SYNC();
    if (fast) {
        for (int i = lane; i < (1 << fast_bits); i += PI_LANES) {
            const uint32_t c15 = pi_brev15((uint32_t)i);
            uint16_t e = 0;
            for (int len = 1; len <= fast_bits; ++len)
                if (c15 < t->limit[len]) {
                    e = (uint16_t)(syms[t->offset[len] + (int)(c15 >> (15 - len))] << 4 | len);
                    break;
                }
            fast[i] = e;
        }
        PI_SYNC();
    }
    return t->err;
}

// the next symbol -> its value, or -PI_EARLY / -PI_CODES; the bits are taken
PI_HD int pi_symbol(PiBits& r, const PiTable* t, const uint16_t* syms, const uint16_t* fast, int fast_bits) {
    const uint32_t bits = (uint32_t)r.buf;
    int len = 0, sym = 0;
    if (fast) {
        const uint16_t e = fast[bits & ((1u << fast_bits) - 1u)];
        len = e & 15;
        sym = e >> 4;
    }
    if (len == 0) {
        const uint32_t c15 = pi_brev15(bits);
        for (int l = fast ? fast_bits + 1 : 1; l < 16; ++l)
            if (c15 < t->limit[l]) {
                len = l;
                sym = syms[t->offset[l] + (int)(c15 >> (15 - l))];
                break;
            }
        if (len == 0) return -PI_CODES;
    }
    if (len > r.cnt) return -PI_EARLY;
    r.buf >>= len;
    r.cnt -= len;
    return sym;
}

// what the lanes hold back: literal k of the pending run is lane k's
struct PiOut {
    uint8_t* out;
    int produced, expected, fenced;        // bytes [0, fenced) are known to have landed; H (1 + W bpp) < 2^31
    int run0;                              // where the pending literals go
    int pending;
    uint32_t mine;
};

PI_HD void pi_flush(PiOut& o, int lane) {
    if (lane < o.pending) o.out[o.run0 + lane] = (uint8_t)o.mine;
    o.pending = 0;
}

PI_HD void pi_literal(PiOut& o, uint32_t v, int lane) {
    if (o.pending == 0) o.run0 = o.produced;
    if (lane == o.pending) o.mine = v;
    o.pending += 1;
    o.produced += 1;
    if (o.pending == PI_LANES) pi_flush(o, lane);
}

PI_HD void pi_match(PiOut& o, int L, int D, int lane) {
    pi_flush(o, lane);
    const int src = o.produced - D;
    if (src + (L < D ? L : D) > o.fenced) {
        pi_fence();
        o.fenced = o.produced;
    }
    for (int i = lane; i < L; i += PI_LANES) o.out[o.produced + i] = o.out[src + (i < D ? i : i % D)];
    o.produced += L;
}

PI_HD int pi_fixed_lengths(uint8_t* lens) {
    for (int i = 0; i < 144; ++i) lens[i] = 8;
    for (int i = 144; i < 256; ++i) lens[i] = 9;
    for (int i = 256; i < 280; ++i) lens[i] = 7;
    for (int i = 280; i < 288; ++i) lens[i] = 8;
    for (int i = 0; i < 32; ++i) lens[288 + i] = 5;
    return 0;
}

// the lengths of a dynamic block's two codes into T->lens[0..hlit) and T->lens[288..288 + hdist) -> 0 or a status
PI_HD int pi_dynamic_lengths(PiBits& r, PiTables* T, int* hlit_out, int* hdist_out, int lane) {
    const uint8_t order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    pi_refill(r);
    if (r.cnt < 14) return PI_EARLY;
    const int hlit = (int)pi_take(r, 5) + 257, hdist = (int)pi_take(r, 5) + 1, hclen = (int)pi_take(r, 4) + 4;
    if (hlit > 286 || hdist > 30) return PI_CODES;
    PI_SYNC();                             // the last block's tables are not read any more
    if (lane == 0)
        for (int i = 0; i < 19; ++i) T->lens[i] = 0;
    PI_SYNC();
    for (int i = 0; i < hclen; ++i) {
        pi_refill(r);
        if (r.cnt < 3) return PI_EARLY;
        const uint32_t v = pi_take(r, 3);
        if (lane == 0) T->lens[order[i]] = (uint8_t)v;
    }
    PI_SYNC();
    if (pi_build(&T->cl, T->cl_syms, nullptr, 0, T->lens, 19, false, lane)) return PI_CODES;
    // the two sets are one run of hlit + hdist lengths: a repeat may cross from the first into the second
    const int total = hlit + hdist;
    int at = 0, prev = -1;
    PI_SYNC();
    while (at < total) {
        pi_refill(r);
        const int s = pi_symbol(r, &T->cl, T->cl_syms, nullptr, 0);
        if (s < 0) return -s;
        int rep = 1, val = s;
        if (s == 16) {
            if (prev < 0) return PI_CODES;
            if (r.cnt < 2) return PI_EARLY;
            rep = 3 + (int)pi_take(r, 2);
            val = prev;
        } else if (s == 17) {
            if (r.cnt < 3) return PI_EARLY;
            rep = 3 + (int)pi_take(r, 3);
            val = 0;
        } else if (s == 18) {
            if (r.cnt < 7) return PI_EARLY;
            rep = 11 + (int)pi_take(r, 7);
            val = 0;
        }
        if (at + rep > total) return PI_CODES;
        if (lane == 0)
            for (int k = 0; k < rep; ++k) {
                const int i = at + k;
                T->lens[32 + (i < hlit ? i : 288 + i - hlit)] = (uint8_t)val;   // staged behind the code-length code's own
            }
        at += rep;
        prev = val;
    }
    PI_SYNC();
    *hlit_out = hlit;
    *hdist_out = hdist;
    return 0;
}

// a length symbol s (257..287) and the distance behind it -> -1 where the match was copied, else the status
PI_HD int pi_pair(PiBits& r, PiOut& o, const PiTables* T, int s, int lane) {
    const uint16_t lbase[29] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258};
    const uint8_t lext[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};
    const uint16_t dbase[30] = {1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145,
                                8193, 12289, 16385, 24577};
    const uint8_t dext[30] = {0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13};
    if (s > 285) return PI_CODES;
    int L = lbase[s - 257];
    const int le = lext[s - 257];
    if (r.cnt < le) return PI_EARLY;
    L += (int)pi_take(r, le);
    pi_refill(r);
    const int ds = pi_symbol(r, &T->dist, T->dist_syms, T->dist_fast, PI_DIST_FAST);
    if (ds < 0) return -ds;
    if (ds > 29) return PI_CODES;
    int D = dbase[ds];
    const int de = dext[ds];
    if (r.cnt < de) return PI_EARLY;
    D += (int)pi_take(r, de);
    if (D > o.produced) return PI_DISTANCE;
    if (L > o.expected - o.produced) return PI_LENGTH;
    pi_match(o, L, D, lane);
    return -1;
}

// One stream: bytes [begin, end) of data -> out[0 .. expected), by the PI_LANES lanes of the caller together.  Nothing outside
// out[0, expected) is written and no byte outside [begin, end) is read.  -> the status.  BAND: the band mode above; middle is
// read with BAND only.  pi_inflate(...) without either is the sequential decoder.
template <bool BAND = false>
PI_HD int pi_inflate(const uint8_t* data, int begin, int end, uint8_t* out, int expected, PiTables* T, int lane, bool middle = false) {
    PiBits r;
    r.data = data;
    r.begin = begin;
    r.p = begin;
    r.end = end;
    r.buf = 0;
    r.cnt = 0;
#if defined(__HIP_DEVICE_COMPILE__)
    r.chunk = 0;
    r.window = -1;
    r.lane = lane;
#endif
    PiOut o;
    o.out = out;
    o.produced = 0;
    o.expected = expected;
    o.fenced = 0;
    o.run0 = 0;
    o.pending = 0;
    o.mine = 0;
    for (;;) {
        pi_refill(r);
        if (r.cnt < 3) return PI_EARLY;
        const int last = (int)pi_take(r, 1), type = (int)pi_take(r, 2);
        if constexpr (BAND)
            if (middle && last) return PI_BAND;
        if (type == 3) return PI_BLOCK;
        if (type == 0) {
            pi_take(r, r.cnt & 7);
            pi_refill(r);
            if (r.cnt < 32) return PI_EARLY;
            const uint32_t len = pi_take(r, 16), nlen = pi_take(r, 16);
            if ((len ^ 0xffffu) != nlen) return PI_BLOCK;
            if ((int)len > expected - o.produced) return PI_LENGTH;
            if ((int)len > (r.cnt >> 3) + (r.end - r.p)) return PI_EARLY;
            pi_flush(o, lane);
            int done = 0;
            while (done < (int)len && r.cnt > 0) {              // the bytes the bit buffer holds already: at most 8
                const uint32_t v = pi_take(r, 8);
                if (lane == 0) out[o.produced + done] = (uint8_t)v;
                done += 1;
            }
            const int rest = (int)len - done;
            for (int i = lane; i < rest; i += PI_LANES) out[o.produced + done + i] = data[r.p + i];
            r.p += rest;
            o.produced += (int)len;
            if constexpr (BAND)
                if (middle && r.p - (r.cnt >> 3) == end) break;
        } else {
            int hlit = 288, hdist = 32;
            if (type == 1) {
                PI_SYNC();
                if (lane == 0) pi_fixed_lengths(T->lens + 32);
                PI_SYNC();
            } else {
                const int rc = pi_dynamic_lengths(r, T, &hlit, &hdist, lane);
                if (rc) return rc;
                if (T->lens[32 + 256] == 0) return PI_CODES;     // no end-of-block code
            }
            if (pi_build(&T->lit, T->lit_syms, T->lit_fast, PI_LIT_FAST, T->lens + 32, hlit, false, lane)) return PI_CODES;
            if (pi_build(&T->dist, T->dist_syms, T->dist_fast, PI_DIST_FAST, T->lens + 32 + 288, hdist, true, lane)) return PI_CODES;
            // one exit: st < 0 while the block runs, 0 at its end, else the status
            int st = -1;
            do {
                pi_refill(r);
                const int s = pi_symbol(r, &T->lit, T->lit_syms, T->lit_fast, PI_LIT_FAST);
                if (s < 256) {
                    if (s < 0)
                        st = -s;
                    else if (o.produced >= expected)
                        st = PI_LENGTH;
                    else
                        pi_literal(o, (uint32_t)s, lane);
                } else if (s == 256) {
                    st = 0;
                } else {
                    st = pi_pair(r, o, T, s, lane);
                }
            } while (st < 0);
            if (st) return st;
        }
        if (last) break;
    }
    pi_flush(o, lane);
    return o.produced == expected ? PI_OK : PI_LENGTH;
}
