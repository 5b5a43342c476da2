// The entropy coder of csrc/jpeg_entropy_enc.h on the host, under sanitizers (DESIGN.md "JPEG files out"):
//
//     clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//         -I include -I 2023-tifs-istvt_amd/csrc tools/jpeg_entropy_enc_check.cpp -o jpeg_entropy_enc_check
//     ./jpeg_entropy_enc_check
//
// Coefficient arrays from a fixed LCG in four flavours -- sparse and realistic | dense, every coefficient in +-1023 | runs of
// 16 and more zeros, 62 zero AC coefficients before a non-zero last one among them | arbitrary int16 with +-32767 and -32768 -- for
// both chroma steps, images of 1 x 1, 3 x 2, 5 x 3 and 7 x 1 MCUs and restart intervals of 0, 1, 2, 5 MCUs and one MCU row.
// Every segment is counted (JeCount) and then stored (JeStore) into a heap buffer of exactly the counted size, so
// AddressSanitizer sees any store outside; the stored length must equal the counted one and the segment must end with FF
// and its marker.  The first three flavours must report status 0 and decode back, through je_decode_segment of
// csrc/jpeg_entropy.h with the tables of the same Annex K.3 lists, to the coefficients they were made from; the fourth must
// report status 3.  Prints one line per flavour, exit status 1 on any failure.
// A hand tool for a CPU: it is no test of the suite and nothing here touches a GPU.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "jpeg_entropy.h"
#include "jpeg_entropy_enc.h"

namespace {

uint32_t lcg_state = 20251019u;
uint32_t lcg() {
    lcg_state = lcg_state * 1664525u + 1013904223u;
    return lcg_state >> 8;
}
int between(int lo, int hi) { return lo + (int)(lcg() % (uint32_t)(hi - lo + 1)); }

struct Table {
    int t[JE_HUFF_INTS];
};

// clips.jpeg_huffman_table
void decode_form(const uint8_t* counts, const uint8_t* values, int total, Table& out) {
    int code = 0, at = 0;
    for (int l = 1; l <= 16; ++l) {
        out.t[16 + l - 1] = at - code;
        code += counts[l - 1];
        at += counts[l - 1];
        out.t[l - 1] = code << (16 - l);
        code <<= 1;
    }
    for (int i = 0; i < 256; ++i) out.t[32 + i] = i < total ? values[i] : 0;
}

struct Writer {
    std::vector<int16_t> coef;             // natural order, exactly the image's blocks
    long blocks = 0;
    int ybw = 0, cbw = 0, ny = 0, nc = 0;
    long block(int c, int row, int col) { return c == 0 ? (long)row * ybw + col : ny + (long)(c - 1) * nc + (long)row * cbw + col; }
    void clear(long b) {
        for (int i = 0; i < 64; ++i) coef[b * 64 + i] = 0;
    }
    void put(long b, int at, int v) { coef[b * 64 + at] = (int16_t)v; }
};

// one block of flavour f into c[0..63] (zig-zag order); dc: the running DC of the component
void make_block(int f, int16_t* c, int& dc) {
    memset(c, 0, 128);
    if (f == 0) {
        dc += between(-60, 60);
        dc = dc > 1023 ? 1023 : dc < -1023 ? -1023 : dc;
        c[0] = (int16_t)dc;
        const int last = between(0, 20);
        for (int k = 1; k <= last; ++k)
            if (lcg() % 3 == 0) c[k] = (int16_t)(between(-40, 40) / (1 + k / 4));
    } else if (f == 1) {
        for (int k = 0; k < 64; ++k) c[k] = (int16_t)between(-1023, 1023);
    } else if (f == 2) {
        c[0] = (int16_t)between(-1023, 1023);
        switch (lcg() % 6) {
            case 0: c[63] = (int16_t)(lcg() & 1 ? 1 : -1023); break;                     // 62 zeros, then the last one
            case 1: c[17] = 5, c[50] = -7; break;                                        // runs of 16 and 32
            case 2: c[1] = -1, c[63] = 1023; break;
            case 3: c[33] = (int16_t)between(1, 1023); break;                            // two ZRLs, then EOB
            case 4: c[16] = 1, c[32] = -1, c[48] = 2, c[49] = -2; break;                 // runs of exactly 15
            default: break;                                                              // DC and EOB
        }
    } else {
        for (int k = 0; k < 64; ++k) {
            const uint32_t r = lcg();
            c[k] = r % 7 == 0 ? (int16_t)(r & 0x100 ? 32767 : -32767) : r % 11 == 0 ? (int16_t)-32768 : (int16_t)(r & 0xFFFF);
        }
    }
}

int failures = 0;
void fail(const char* what, int f, int sub, int mx, int my, int ri, long seg) {
    printf("FAILED: %s (flavour %d, sub %d, %d x %d MCUs, interval %d, segment %ld)\n", what, f, sub, mx, my, ri, seg);
    ++failures;
}

}  // namespace

int main() {
    static constexpr JeStdHuffman std_tables = je_std_huffman();
    Table huff[2][2];
    for (int c = 0; c < 2; ++c)
        for (int id = 0; id < 2; ++id) decode_form(std_tables.counts[c][id], std_tables.values[c][id], std_tables.total[c][id], huff[c][id]);
    if (std_tables.total[1][0] != 162 || std_tables.total[1][1] != 162) fail("the AC value lists hold 162 symbols", -1, 0, 0, 0, 0, 0);
    const int* tabs[6] = {huff[0][0].t, huff[1][0].t, huff[0][1].t, huff[1][1].t, huff[0][1].t, huff[1][1].t};
    uint32_t codes[JE_CODE_WORDS];
    for (int i = 0; i < JE_CODE_WORDS; ++i) codes[i] = je_code_word(i);
    const int shapes[4][2] = {{1, 1}, {3, 2}, {5, 3}, {7, 1}};
    const char* names[4] = {"sparse", "dense +-1023", "long zero runs", "arbitrary int16"};
    for (int f = 0; f < 4; ++f) {
        long segments = 0, bytes = 0, stuffed = 0;
        int worst = 0;
        for (int sub = 2; sub >= 1; --sub) {
            for (const auto& shape : shapes) {
                const int mx = shape[0], my = shape[1], mcus = mx * my;
                const long nb = (long)mcus * (sub * sub + 2);
                std::vector<JeQuad> backing(nb * 8);                       // 16-byte aligned, exactly the image's blocks
                int16_t* coef = reinterpret_cast<int16_t*>(backing.data());
                const int intervals[5] = {0, 1, 2, 5, mx};
                for (int ri : intervals) {
                    const long ybw = (long)mx * sub, ny = ybw * my * sub, nc = mcus;
                    int dc[3] = {0, 0, 0};
                    for (long b = 0; b < nb; ++b) make_block(f, coef + b * 64, dc[b < ny ? 0 : b < ny + nc ? 1 : 2]);
                    if (f == 3) coef[1] = 32767, coef[64 * (nb - 1)] = -32768;
                    const int per = ri ? (ri < mcus ? ri : mcus) : mcus, nseg = (mcus + per - 1) / per;
                    Writer w;
                    w.ybw = (int)ybw, w.cbw = mx, w.ny = (int)ny, w.nc = (int)nc, w.blocks = nb;
                    w.coef.assign(nb * 64, 0x5a5a);
                    int image_status = 0;
                    for (int s = 0; s < nseg; ++s) {
                        const int first = s * per, count = mcus - first < per ? mcus - first : per;
                        const int marker = s == nseg - 1 ? 0xD9 : 0xD0 + (s & 7);
                        JeCount counter = {0};
                        int st0 = -1, st1 = -1;
                        const long len = je_encode_segment(coef, je_layout(0, sub), mx, my, first, count, codes, marker, counter, st0);
                        if (len < 2) {
                            fail("a segment holds its marker at least", f, sub, mx, my, ri, s);
                            continue;
                        }
                        std::vector<uint8_t> out((size_t)len, 0xAA);       // exactly the counted size
                        JeStore store = {out.data(), 0, len, 0};
                        const long wrote = je_encode_segment(coef, je_layout(0, sub), mx, my, first, count, codes, marker, store, st1);
                        if (wrote != len || store.n != len) fail("the stored length equals the counted one", f, sub, mx, my, ri, s);
                        if (st0 != st1 || (st0 != 0 && st0 != 3)) fail("one status, 0 or 3, from both passes", f, sub, mx, my, ri, s);
                        if (out[len - 2] != 0xFF || out[len - 1] != marker) fail("FF and the marker end the segment", f, sub, mx, my, ri, s);
                        for (long i = 0; i + 2 < len; ++i)
                            if (out[i] == 0xFF) {
                                if (out[i + 1] != 0) fail("FF inside the scan is followed by 00", f, sub, mx, my, ri, s);
                                ++stuffed;
                            }
                        if (st0 > image_status) image_status = st0;
                        ++segments, bytes += len;
                        if (f < 3) {
                            const int st = je_decode_segment(out.data(), 0L, len - 2, tabs, je_layout(0, sub), mx, first, count, w);
                            if (st != 0) fail("the segment decodes with status 0", f, sub, mx, my, ri, s);
                        }
                    }
                    if (image_status > worst) worst = image_status;
                    if (f < 3) {
                        if (image_status != 0) fail("status 0 inside baseline's categories", f, sub, mx, my, ri, -1);
                        for (long b = 0; b < nb; ++b)
                            for (int k = 0; k < 64; ++k)
                                if (w.coef[b * 64 + je_zigzag(k)] != coef[b * 64 + k]) {
                                    fail("the decoded coefficients equal the coded ones", f, sub, mx, my, ri, b);
                                    b = nb;
                                    break;
                                }
                    } else if (image_status != 3) {
                        fail("status 3 outside baseline's categories", f, sub, mx, my, ri, -1);
                    }
                }
            }
        }
        printf("%s: %ld segments, %ld bytes (%ld stuffed), status %d\n", names[f], segments, bytes, stuffed, worst);
    }
    printf("%s\n", failures ? "FAILED" : "ok");
    return failures ? 1 : 0;
}
