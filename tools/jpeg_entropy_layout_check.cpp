// The entropy coder of csrc/jpeg_entropy_enc.h and the table builder of csrc/jpeg_entropy_opt.h in the layouts 4:2:2 and
// greyscale, on the host, under sanitizers (DESIGN.md "JPEG files out, 4:2:2 and greyscale"):
//
//     clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//         -I include -I 2023-tifs-istvt_amd/csrc tools/jpeg_entropy_layout_check.cpp -o jpeg_entropy_layout_check
//     ./jpeg_entropy_layout_check tests/golden/J5_jpeg_encode_layouts_scans.txt
//
// For both layouts, images of 1 x 1, 3 x 2, 5 x 3 and 7 x 1 MCUs, restart intervals of 0, 1, 3 MCUs and one MCU row, and
// blocks drawn from a fixed LCG: every segment is counted (JeCount) and then stored (JeStore) into a heap buffer of exactly
// the counted size, so AddressSanitizer sees any store outside, once with the Annex K.3 tables and once with the tables
// jo_optimal_table makes of jo_count_segment's counts (a greyscale image leaves both id-1 tables empty), and decoded by
// je_decode_segment of csrc/jpeg_entropy.h back to the coefficients.  jo_previous_block must name, for every block, the block
// the scan coded before it in its component.  Then the scans file (tests/golden/make_jpeg_encode_layouts_golden.py writes
// it): whitespace-separated integers, the number of cases, then per case layout code, MCU columns, MCU rows, restart
// interval, optimised (0 / 1), the number of blocks, 64 coefficients per block (zig-zag) in the order of the device's scratch,
// the number of scan bytes and the scan of clips.jpeg_encode_host(layout=); coding the blocks must give those bytes.  Prints
// one line per layout, one for the scans, `ok` at the end; exit status 1 on any failure.
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
void fail(const char* what, int layout, int mx, int my, int ri) {
    printf("FAILED: %s (layout %d, %d x %d MCUs, interval %d)\n", what, layout, mx, my, ri);
    ++failures;
}

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
    int ybw = 0, cbw = 0, ny = 0, nc = 0;
    long block(int c, int row, int col) { return c == 0 ? (long)row * ybw + col : ny + (long)(c - 1) * nc + (long)row * cbw + col; }
    void clear(long b) {
        for (int i = 0; i < 64; ++i) coef[b * 64 + i] = 0;
    }
    void put(long b, int at, int v) { coef[b * 64 + at] = (int16_t)v; }
};

// the code words and decode tables of a call: Annex K.3, or the tables of the image's own counts
struct Coding {
    uint32_t codes[JE_CODE_WORDS];
    Table huff[4];                         // DC 0, DC 1, AC 0, AC 1
    int totals[4];
};

void standard_coding(Coding& c) {
    static constexpr JeStdHuffman std_tables = je_std_huffman();
    for (int i = 0; i < JE_CODE_WORDS; ++i) c.codes[i] = je_code_word(i);
    for (int k = 0; k < 4; ++k) {
        c.totals[k] = std_tables.total[k >> 1][k & 1];
        decode_form(std_tables.counts[k >> 1][k & 1], std_tables.values[k >> 1][k & 1], c.totals[k], c.huff[k]);
    }
}

void optimal_coding(const int16_t* coef, const JeLayout& lay, int mx, int my, int per, Coding& c) {
    const int mcus = mx * my, nseg = (mcus + per - 1) / per;
    uint32_t hist[4 * 256] = {};
    JoHistogram sink = {hist};
    for (int s = 0; s < nseg; ++s) jo_count_segment(coef, lay, mx, my, per, s * per, mcus - s * per < per ? mcus - s * per : per, sink);
    for (int k = 0; k < 4; ++k) {
        uint8_t bits[16], values[256];
        jo_optimal_table(hist + k * 256, bits, values, &c.totals[k]);
        jo_code_words(bits, values, c.totals[k], c.codes + (k < 2 ? JE_CODE_DC + 16 * k : JE_CODE_AC + 256 * (k - 2)), k < 2 ? 16 : 256);
        decode_form(bits, values, c.totals[k], c.huff[k]);
    }
}

// every segment of the image into a heap buffer of exactly its counted size -> the scan; `back`: decoded again
bool code_image(const int16_t* coef, const JeLayout& lay, int mx, int my, int per, const Coding& c, std::vector<uint8_t>& scan,
                Writer* back) {
    const int mcus = mx * my, nseg = (mcus + per - 1) / per;
    const int* tabs[6] = {c.huff[0].t, c.huff[2].t, c.huff[1].t, c.huff[3].t, c.huff[1].t, c.huff[3].t};
    bool good = true;
    for (int s = 0; s < nseg; ++s) {
        const int first = s * per, count = mcus - first < per ? mcus - first : per;
        const int marker = s == nseg - 1 ? 0xD9 : 0xD0 + (s & 7);
        JeCount counter = {0};
        int st0 = -1, st1 = -1;
        const long len = je_encode_segment(coef, lay, mx, my, first, count, c.codes, marker, counter, st0);
        if (len < 2) return false;
        std::vector<uint8_t> out((size_t)len, 0xAA);             // exactly the counted size
        JeStore store = {out.data(), 0, len, 0};
        const long wrote = je_encode_segment(coef, lay, mx, my, first, count, c.codes, marker, store, st1);
        good = good && wrote == len && st0 == 0 && st1 == 0 && out[len - 2] == 0xFF && out[len - 1] == marker;
        if (back) good = good && je_decode_segment(out.data(), 0L, len - 2, tabs, lay, mx, first, count, *back) == 0;
        scan.insert(scan.end(), out.begin(), out.end());
    }
    return good;
}

// one sparse block (zig-zag order); dc: the running DC of the component
void make_block(int16_t* c, int& dc) {
    memset(c, 0, 128);
    dc += between(-60, 60);
    dc = dc > 1023 ? 1023 : dc < -1023 ? -1023 : dc;
    c[0] = (int16_t)dc;
    switch (lcg() % 5) {
        case 0: break;                                                                   // DC and EOB
        case 1: c[63] = (int16_t)between(-1023, 1023); break;                            // three ZRLs
        case 2: c[17] = 5, c[50] = -7; break;                                            // runs of 16 and 32
        default:
            for (int k = 1, last = between(1, 40); k <= last; ++k)
                if (lcg() % 3 == 0) c[k] = (int16_t)(between(-200, 200) / (1 + k / 4));
    }
}

void check_layout(int code, const char* name) {
    const JeLayout lay = je_layout(code, code == ISTVT_JPEG_LAYOUT_422 ? 2 : 1);
    const int shapes[4][2] = {{1, 1}, {3, 2}, {5, 3}, {7, 1}};
    long images = 0, bytes = 0, saved = 0;
    for (const auto& shape : shapes) {
        const int mx = shape[0], my = shape[1], mcus = mx * my;
        const long ybw = (long)mx * lay.h, ny = ybw * my * lay.v, nc = mcus, nb = ny + lay.nc * nc;
        std::vector<JeQuad> backing(nb * 8);                     // 16-byte aligned, exactly the image's blocks
        int16_t* coef = reinterpret_cast<int16_t*>(backing.data());
        const int intervals[4] = {0, 1, 3, mx};
        for (int ri : intervals) {
            int dc[3] = {0, 0, 0};
            for (long b = 0; b < nb; ++b) make_block(coef + b * 64, dc[b < ny ? 0 : b < ny + nc ? 1 : 2]);
            const int per = ri ? (ri < mcus ? ri : mcus) : mcus;
            // jo_previous_block against the order of the scan
            long last[3] = {-1, -1, -1};
            for (int mcu = 0; mcu < mcus; ++mcu) {
                if (mcu % per == 0) last[0] = last[1] = last[2] = -1;
                for (int c = 0; c <= lay.nc; ++c)
                    for (int v = 0; v < (c ? 1 : lay.v); ++v)
                        for (int h = 0; h < (c ? 1 : lay.h); ++h) {
                            const long b = c == 0 ? ((long)(mcu / mx) * lay.v + v) * ybw + (long)(mcu % mx) * lay.h + h : ny + (c - 1) * nc + mcu;
                            int id = -1;
                            if (jo_previous_block(b, lay, mx, my, per, id) != last[c] || id != (c ? 1 : 0))
                                fail("jo_previous_block names the block the scan coded before", code, mx, my, ri);
                            last[c] = b;
                        }
            }
            long length[2] = {0, 0};
            for (int optimised = 0; optimised < 2; ++optimised) {
                Coding c;
                if (optimised) optimal_coding(coef, lay, mx, my, per, c);
                else standard_coding(c);
                if (optimised && lay.nc == 0 && (c.totals[1] != 0 || c.totals[3] != 0))
                    fail("a greyscale image leaves the id-1 tables empty", code, mx, my, ri);
                Writer w;
                w.ybw = (int)ybw, w.cbw = mx, w.ny = (int)ny, w.nc = (int)nc;
                w.coef.assign(nb * 64, 0x5a5a);
                std::vector<uint8_t> scan;
                if (!code_image(coef, lay, mx, my, per, c, scan, &w)) fail("count, store and decode agree with status 0", code, mx, my, ri);
                for (long b = 0; b < nb; ++b)
                    for (int k = 0; k < 64; ++k)
                        if (w.coef[b * 64 + je_zigzag(k)] != coef[b * 64 + k]) {
                            fail("the decoded coefficients equal the coded ones", code, mx, my, ri);
                            b = nb;
                            break;
                        }
                length[optimised] = (long)scan.size();
            }
            if (length[1] > length[0]) fail("the optimised scan is no longer", code, mx, my, ri);
            ++images, bytes += length[0], saved += length[0] - length[1];
        }
    }
    printf("%s: %ld images, %ld scan bytes, %ld saved by their own tables\n", name, images, bytes, saved);
}

void check_scans(const char* path) {
    FILE* f = fopen(path, "r");
    if (!f) {
        printf("FAILED: cannot open %s\n", path);
        ++failures;
        return;
    }
    long n = 0, equal = 0;
    if (fscanf(f, "%ld", &n) != 1 || n < 1 || n > 10000) fail("the scans file starts with its count", 0, 0, 0, 0), n = 0;
    for (long i = 0; i < n; ++i) {
        long code = 0, mx = 0, my = 0, ri = 0, optimised = 0, nb = 0, len = 0, v = 0;
        bool read = fscanf(f, "%ld %ld %ld %ld %ld %ld", &code, &mx, &my, &ri, &optimised, &nb) == 6;
        read = read && (code == ISTVT_JPEG_LAYOUT_422 || code == ISTVT_JPEG_LAYOUT_GREY) && mx >= 1 && my >= 1 && mx * my <= 4096 &&
               ri >= 0 && ri <= 65535;
        const JeLayout lay = je_layout((int)code, code == ISTVT_JPEG_LAYOUT_422 ? 2 : 1);
        read = read && nb == mx * my * (lay.h * lay.v + lay.nc);
        std::vector<JeQuad> backing(read ? nb * 8 : 0);
        int16_t* coef = reinterpret_cast<int16_t*>(backing.data());
        for (long k = 0; k < nb * 64 && read; ++k) read = fscanf(f, "%ld", &v) == 1 && v >= -32768 && v <= 32767, coef[k] = (int16_t)v;
        read = read && fscanf(f, "%ld", &len) == 1 && len >= 2 && len <= (1 << 24);
        std::vector<uint8_t> want(read ? len : 0);
        for (long k = 0; k < len && read; ++k) read = fscanf(f, "%ld", &v) == 1 && v >= 0 && v <= 255, want[k] = (uint8_t)v;
        if (!read) {
            fail("a whole case", (int)code, (int)mx, (int)my, (int)ri);
            break;
        }
        const int mcus = (int)(mx * my), per = ri ? (ri < mcus ? (int)ri : mcus) : mcus;
        Coding c;
        if (optimised) optimal_coding(coef, lay, (int)mx, (int)my, per, c);
        else standard_coding(c);
        std::vector<uint8_t> scan;
        if (!code_image(coef, lay, (int)mx, (int)my, per, c, scan, nullptr) || scan != want)
            fail("the scan of clips.jpeg_encode_host(layout=)", (int)code, (int)mx, (int)my, (int)ri);
        else
            ++equal;
    }
    fclose(f);
    printf("scans: %ld of %ld equal the definition's\n", equal, n);
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 2) {
        printf("usage: jpeg_entropy_layout_check SCANS\n");
        return 2;
    }
    check_layout(ISTVT_JPEG_LAYOUT_422, "4:2:2");
    check_layout(ISTVT_JPEG_LAYOUT_GREY, "greyscale");
    check_scans(argv[1]);
    printf("%s\n", failures ? "FAILED" : "ok");
    return failures ? 1 : 0;
}
