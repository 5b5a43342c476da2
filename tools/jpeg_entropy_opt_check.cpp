// The table builder of csrc/jpeg_entropy_opt.h on the host, under sanitizers (DESIGN.md "JPEG files out, optimised tables"):
//
//     clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//         -I include -I 2023-tifs-istvt_amd/csrc tools/jpeg_entropy_opt_check.cpp -o jpeg_entropy_opt_check
//     ./jpeg_entropy_opt_check tests/golden/J4_jpeg_optimize_vectors.txt
//
// The vectors file (tests/golden/make_jpeg_optimize_golden.py writes it) holds whitespace-separated integers: the number of
// vectors, then per vector 256 counts, the 16 length counts and the number of values clips.jpeg_optimal_table gives, and the
// values.  jo_optimal_table must give the same.  Then six families of counts from a fixed LCG -- random | all equal | one
// symbol | 256 symbols | Fibonacci-like, which force lengths past 16 and past 32 | near 2^31 (and 2^32 - 1) -- and for each
// table: every length <= 16, a Kraft sum below 1 (the all-ones code is free), a code for every counted symbol, at most 256
// values.  For each, coefficient blocks whose symbols are drawn from the counted ones are counted (jo_count_segment), coded
// with the tables of those counts (je_encode_segment into a heap buffer of exactly the counted size) and decoded by
// je_decode_segment of csrc/jpeg_entropy.h: the coefficients must come back.  Prints one line per family, `ok` at the end,
// exit status 1 on any failure.
// A hand tool for a CPU: nothing here touches a GPU.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "jpeg_entropy.h"
#include "jpeg_entropy_enc.h"
#include "jpeg_entropy_opt.h"

namespace {

uint32_t lcg_state = 20261020u;
uint32_t lcg() {
    lcg_state = lcg_state * 1664525u + 1013904223u;
    return lcg_state >> 8;
}
int between(int lo, int hi) { return lo + (int)(lcg() % (uint32_t)(hi - lo + 1)); }

int failures = 0;
void fail(const char* what, const char* family, int item) {
    printf("FAILED: %s (%s, item %d)\n", what, family, item);
    ++failures;
}

struct Table {
    uint8_t bits[16], values[256];
    int total;
};

// the properties every table must have on its counts
void check_table(const uint32_t* counts, const Table& t, const char* family, int item) {
    if (t.total < 0 || t.total > 256) return fail("total <= 256", family, item);
    uint64_t kraft = 0;                                          // in units of 2^-16
    int codes = 0;
    for (int l = 1; l <= 16; ++l) kraft += (uint64_t)t.bits[l - 1] << (16 - l), codes += t.bits[l - 1];
    if (codes != t.total) fail("as many codes as values", family, item);
    bool any = false, held[256] = {};
    for (int i = 0; i < t.total; ++i) {
        if (held[t.values[i]]) fail("a value twice", family, item);
        held[t.values[i]] = true;
    }
    for (int s = 0; s < 256; ++s) {
        any |= counts[s] != 0;
        if ((counts[s] != 0) != held[s]) fail("a code for every counted symbol and for no other", family, item);
    }
    if (any && kraft >= 65536) fail("a Kraft sum below 1", family, item);
    if (!any && (t.total != 0 || kraft != 0)) fail("an empty table for all-zero counts", family, item);
}

int decode_form(const Table& t, int* out) {                      // clips.jpeg_huffman_table
    int code = 0, at = 0;
    for (int l = 1; l <= 16; ++l) {
        out[16 + l - 1] = at - code;
        code += t.bits[l - 1];
        at += t.bits[l - 1];
        out[l - 1] = code << (16 - l);
        code <<= 1;
    }
    for (int i = 0; i < 256; ++i) out[32 + i] = i < t.total ? t.values[i] : 0;
    return at;
}

struct Writer {
    std::vector<int16_t> coef;             // natural order
    int ybw = 0, cbw = 0, ny = 0, nc = 0;
    long block(int c, int row, int col) { return c == 0 ? (long)row * ybw + col : ny + (long)(c - 1) * nc + (long)row * cbw + col; }
    void clear(long b) {
        for (int i = 0; i < 64; ++i) coef[b * 64 + i] = 0;
    }
    void put(long b, int at, int v) { coef[b * 64 + at] = (int16_t)v; }
};

// a value of category `size`
int of_size(int size) {
    if (size == 0) return 0;
    const int lo = 1 << (size - 1), hi = (1 << size) - 1, v = between(lo, hi);
    return lcg() & 1 ? v : -v;
}

// Blocks whose AC symbols are drawn from `allowed` (symbols with a count in the family's AC histogram; sizes 1..10 only) and
// whose DC differences have the categories of `dc_allowed`; then count, build, code, decode, compare.
void round_trip(const uint32_t* dc_counts, const uint32_t* ac_counts, const char* family, int item) {
    std::vector<int> ac_syms, dc_sizes;
    for (int s = 0; s < 256; ++s)
        if (ac_counts[s] && (s & 15) >= 1 && (s & 15) <= 10) ac_syms.push_back(s);
    for (int s = 0; s < 12; ++s)
        if (dc_counts[s]) dc_sizes.push_back(s);
    if (dc_sizes.empty()) dc_sizes.push_back(0);
    for (int sub = 2; sub >= 1; --sub) {
        const int mx = 3, my = 2, mcus = mx * my;
        const JeLayout lay = je_layout(0, sub);
        const long ybw = (long)mx * sub, ny = ybw * my * sub, nc = mcus, nb = ny + 2 * nc;
        std::vector<JeQuad> backing(nb * 8);                     // 16-byte aligned, exactly the image's blocks
        int16_t* coef = reinterpret_cast<int16_t*>(backing.data());
        memset(coef, 0, nb * 128);
        for (long b = 0; b < nb; ++b) {
            int k = 1;
            while (!ac_syms.empty() && lcg() % 5 != 0) {
                const int sym = ac_syms[lcg() % ac_syms.size()];
                k += sym >> 4;
                if (k > 63) break;
                coef[b * 64 + k++] = (int16_t)of_size(sym & 15);
            }
        }
        const int intervals[3] = {0, 1, mx};
        for (int ri : intervals) {
            const int per = ri ? ri : mcus, nseg = (mcus + per - 1) / per;
            // the DCs: walk the blocks in scan order so that every difference has an allowed category
            for (int mcu = 0; mcu < mcus; ++mcu)
                for (int c = 0; c < 3; ++c)
                    for (int v = 0; v < (c ? 1 : sub); ++v)
                        for (int h = 0; h < (c ? 1 : sub); ++h) {
                            const long b = c == 0 ? ((long)(mcu / mx) * sub + v) * ybw + (long)(mcu % mx) * sub + h : ny + (c - 1) * nc + mcu;
                            int id = 0;
                            const long p = jo_previous_block(b, lay, mx, my, per, id);
                            const int pred = p < 0 ? 0 : coef[p * 64];
                            int d = of_size(dc_sizes[lcg() % dc_sizes.size()]);
                            if (pred + d > 1023 || pred + d < -1023) d = -d;
                            if (pred + d > 1023 || pred + d < -1023) d = 0;
                            coef[b * 64] = (int16_t)(pred + d);
                        }
            uint32_t hist[4 * 256] = {};
            JoHistogram sink = {hist};
            for (int s = 0; s < nseg; ++s) jo_count_segment(coef, lay, mx, my, per, s * per, mcus - s * per < per ? mcus - s * per : per, sink);
            // the tables of the blocks' own counts, then (where they hold EOB and category 0, which any block may need) the
            // tables of the family's counts themselves
            for (int variant = 0; variant < 2; ++variant) {
            if (variant == 1 && !(ac_counts[0] && dc_counts[0])) continue;
            Table t[4];
            uint32_t codes[JE_CODE_WORDS];
            int huff[4][JE_HUFF_INTS];
            for (int k = 0; k < 4; ++k) {
                const uint32_t* from = variant == 0 ? hist + k * 256 : k < 2 ? dc_counts : ac_counts;
                jo_optimal_table(from, t[k].bits, t[k].values, &t[k].total);
                check_table(from, t[k], family, item);
                jo_code_words(t[k].bits, t[k].values, t[k].total, codes + (k < 2 ? JE_CODE_DC + 16 * k : JE_CODE_AC + 256 * (k - 2)), k < 2 ? 16 : 256);
                decode_form(t[k], huff[k]);
            }
            const int* tabs[6] = {huff[0], huff[2], huff[1], huff[3], huff[1], huff[3]};
            Writer w;
            w.ybw = (int)ybw, w.cbw = mx, w.ny = (int)ny, w.nc = (int)nc;
            w.coef.assign(nb * 64, 0x5a5a);
            for (int s = 0; s < nseg; ++s) {
                const int first = s * per, count = mcus - first < per ? mcus - first : per;
                const int marker = s == nseg - 1 ? 0xD9 : 0xD0 + (s & 7);
                JeCount counter = {0};
                int st0 = -1, st1 = -1;
                const long len = je_encode_segment(coef, lay, mx, my, first, count, codes, marker, counter, st0);
                if (len < 2) {
                    fail("a segment holds its marker at least", family, item);
                    continue;
                }
                std::vector<uint8_t> out((size_t)len, 0xAA);     // exactly the counted size
                JeStore store = {out.data(), 0, len, 0};
                const long wrote = je_encode_segment(coef, lay, mx, my, first, count, codes, marker, store, st1);
                if (wrote != len || st0 != 0 || st1 != 0) fail("the stored length equals the counted one, status 0", family, item);
                if (je_decode_segment(out.data(), 0L, len - 2, tabs, lay, mx, first, count, w) != 0)
                    fail("the segment decodes with status 0", family, item);
            }
            for (long b = 0; b < nb; ++b)
                for (int k = 0; k < 64; ++k)
                    if (w.coef[b * 64 + je_zigzag(k)] != coef[b * 64 + k]) {
                        fail("the decoded coefficients equal the coded ones", family, item);
                        b = nb;
                        break;
                    }
            }
        }
    }
}

int check_vectors(const char* path) {
    FILE* f = fopen(path, "r");
    if (!f) {
        printf("FAILED: cannot open %s\n", path);
        return ++failures;
    }
    long n = 0;
    if (fscanf(f, "%ld", &n) != 1 || n < 1 || n > 100000) fail("the vectors file starts with its count", "vectors", 0), n = 0;
    int limited = 0;
    for (long i = 0; i < n; ++i) {
        uint32_t counts[256];
        long v = 0, bits[16], total = 0;
        bool read = true;
        for (int s = 0; s < 256 && read; ++s) read = fscanf(f, "%ld", &v) == 1 && v >= 0 && v <= 0xFFFFFFFFL, counts[s] = (uint32_t)v;
        for (int l = 0; l < 16 && read; ++l) read = fscanf(f, "%ld", &bits[l]) == 1;
        read = read && fscanf(f, "%ld", &total) == 1 && total >= 0 && total <= 256;
        std::vector<long> values(read ? total : 0);
        for (long k = 0; k < total && read; ++k) read = fscanf(f, "%ld", &values[k]) == 1;
        if (!read) {
            fail("a whole vector", "vectors", (int)i);
            break;
        }
        Table t;
        jo_optimal_table(counts, t.bits, t.values, &t.total);
        check_table(counts, t, "vectors", (int)i);
        bool same = t.total == total;
        for (int l = 0; l < 16; ++l) same = same && t.bits[l] == bits[l];
        for (long k = 0; k < total && same; ++k) same = t.values[k] == values[k];
        if (!same) fail("the table of clips.jpeg_optimal_table", "vectors", (int)i);
        limited += t.bits[15] != 0;
    }
    fclose(f);
    printf("vectors: %ld tables equal the definition's, %d of them reach length 16\n", n, limited);
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 2) {
        printf("usage: jpeg_entropy_opt_check VECTORS\n");
        return 2;
    }
    check_vectors(argv[1]);
    const char* names[6] = {"random", "all equal", "one symbol", "256 symbols", "Fibonacci-like", "near 2^31"};
    for (int f = 0; f < 6; ++f) {
        int tables = 0, longest = 0;
        for (int item = 0; item < 40; ++item) {
            uint32_t ac[256] = {}, dc[256] = {};
            if (f == 0) {
                const int kinds = between(1, 256);
                for (int k = 0; k < kinds; ++k) ac[lcg() & 255] = lcg() % (1u << between(1, 24));
            } else if (f == 1) {
                const int kinds = between(1, 256);
                const uint32_t c = 1 + lcg() % 1000;
                for (int k = 0; k < kinds; ++k) ac[(k * 37 + item) & 255] = c;
            } else if (f == 2) {
                ac[item % 4 == 0 ? 0 : lcg() & 255] = item & 1 ? 1u : 1u + lcg();
            } else if (f == 3) {
                for (int s = 0; s < 256; ++s) ac[s] = 1 + lcg() % (item < 20 ? 4u : 1u << 20);
            } else if (f == 4) {                                  // lengths up to `depth` + 1 without the limit
                const int depth = between(12, 47), first = lcg() & 255;
                uint64_t a = 1, b = 1;
                for (int k = 0; k < depth; ++k) {
                    ac[(first + k * 5) & 255] = (uint32_t)(a > 0xFFFFFFFFull ? 0xFFFFFFFFull : a);
                    const uint64_t c = a + b;
                    a = b, b = c;
                }
            } else {
                const int kinds = between(1, 256);
                for (int k = 0; k < kinds; ++k) ac[lcg() & 255] = item % 3 == 0 ? 0xFFFFFFFFu : 0x7FFFFFFFu - lcg() % 3 + (item % 3 == 1);
            }
            if (f != 2 && (item & 1) && !ac[0]) ac[0] = 1 + lcg() % 100;       // EOB among them: the family's own tables code blocks
            for (int s = 0; s < 12; ++s) dc[s] = ac[s * 21 & 255] | (s == item % 12 || s == 0);
            Table t;
            jo_optimal_table(ac, t.bits, t.values, &t.total);
            check_table(ac, t, names[f], item);
            for (int l = 16; l >= 1; --l)
                if (t.bits[l - 1]) {
                    if (l > longest) longest = l;
                    break;
                }
            jo_optimal_table(dc, t.bits, t.values, &t.total);
            check_table(dc, t, names[f], item);
            tables += 2;
            round_trip(dc, ac, names[f], item);
        }
        printf("%s: %d tables, longest code %d\n", names[f], tables, longest);
    }
    uint32_t zero[256] = {};
    Table t;
    jo_optimal_table(zero, t.bits, t.values, &t.total);
    check_table(zero, t, "all zero", 0);
    printf("%s\n", failures ? "FAILED" : "ok");
    return failures ? 1 : 0;
}
