// The entropy decoder of csrc/jpeg_entropy.h on the host, under sanitizers (DESIGN.md "JPEG files"):
//
//     clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//         -I include -I 2023-tifs-istvt_amd/csrc tools/jpeg_entropy_check.cpp -o jpeg_entropy_check
//     python tests/golden/make_jpeg_files_golden.py jpg && python tests/golden/make_jpeg_layouts_golden.py jpg
//     ./jpeg_entropy_check jpg/*.jpg
//
// For every baseline file named: the markers are read and the segment table rebuilt here (the job of clips.jpeg_parse and
// clips.jpeg_batch), then je_decode_segment decodes (1) the file as it is, (2) the file cut at every byte length of its scan
// and (3) copies with bits of the scan flipped by a fixed LCG, the segment table kept.  Each run must come back with a status
// in 0..3 after clearing exactly the blocks of the image and writing inside them; the coefficient buffer has the exact
// size, so AddressSanitizer sees any write or read outside.  Prints one line per file, exit status 1 on any failure.
// The files may be 4:2:0, 4:4:4, 4:2:2 or greyscale.
// A hand tool for a CPU: it is no test of the suite and nothing here touches a GPU.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "jpeg_entropy.h"

namespace {

struct Table {
    int t[JE_HUFF_INTS];
};

struct File {
    std::vector<uint8_t> data;
    int H = 0, W = 0, nf = 0, ri = 0;
    JeLayout lay = {0, 0, 0};               // h = 0: no SOF0 yet
    int dc[3] = {0, 0, 0}, ac[3] = {0, 0, 0};
    Table huff[2][4];
    bool have[2][4] = {};
    long scan = 0, scan_end = 0;
    std::vector<long> begin, end;          // the restart intervals
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

bool parse(File& f) {
    const std::vector<uint8_t>& d = f.data;
    const long n = (long)d.size();
    if (n < 4 || d[0] != 0xFF || d[1] != 0xD8) return false;
    long pos = 2;
    for (;;) {
        if (pos + 4 > n || d[pos] != 0xFF) return false;
        while (pos < n && d[pos] == 0xFF) ++pos;
        if (pos + 3 > n) return false;
        const int m = d[pos++];
        const long len = (d[pos] << 8) | d[pos + 1];
        if (len < 2 || pos + len > n) return false;
        const uint8_t* s = d.data() + pos + 2;
        const long sl = len - 2;
        pos += len;
        if (m == 0xC0) {
            if (sl < 6 || s[0] != 8 || (s[5] != 3 && s[5] != 1) || sl != 6 + 3 * s[5]) return false;
            f.H = (s[1] << 8) | s[2], f.W = (s[3] << 8) | s[4], f.nf = s[5];
            if (f.H < 1 || f.W < 1) return false;
            if (f.nf == 1) {                // one component: one block per MCU whatever its factors say (T.81 A.2.2)
                f.lay = JeLayout{1, 1, 0};
            } else {                        // 4:2:0, 4:4:4 or 4:2:2
                if ((s[7] != 0x22 && s[7] != 0x11 && s[7] != 0x21) || s[10] != 0x11 || s[13] != 0x11) return false;
                f.lay = JeLayout{s[7] >> 4, s[7] & 15, 2};
            }
        } else if (m == 0xC4) {
            long at = 0;
            while (at + 17 <= sl) {
                const int tc = s[at] >> 4, th = s[at] & 15;
                int total = 0, space = 1;
                for (int i = 0; i < 16; ++i) {
                    total += s[at + 1 + i];
                    space = 2 * space - s[at + 1 + i];
                    if (space < 0) return false;
                }
                if (tc > 1 || th > 3 || total > 256 || at + 17 + total > sl) return false;
                decode_form(s + at + 1, s + at + 17, total, f.huff[tc][th]);
                f.have[tc][th] = true;
                at += 17 + total;
            }
        } else if (m == 0xDD) {
            if (sl != 2) return false;
            f.ri = (s[0] << 8) | s[1];
        } else if (m == 0xDA) {
            if (f.lay.h == 0 || s[0] != f.nf || sl != 4 + 2 * f.nf) return false;
            for (int c = 0; c < 3; ++c) {   // the slots of components the file does not have repeat Y's
                const int at = c < f.nf ? 2 + 2 * c : 2;
                f.dc[c] = s[at] >> 4, f.ac[c] = s[at] & 15;
                if (f.dc[c] > 3 || f.ac[c] > 3 || !f.have[0][f.dc[c]] || !f.have[1][f.ac[c]]) return false;
            }
            break;
        } else if (m == 0xC2 || m == 0xD9) {
            return false;
        }
    }
    f.scan = pos;
    long begin = pos, at = pos;
    f.scan_end = n;
    while (at < n) {
        if (d[at] != 0xFF) {
            ++at;
            continue;
        }
        long k = at + 1;
        while (k < n && d[k] == 0xFF) ++k;
        if (k >= n) break;
        if (d[k] == 0 && k == at + 1) {
            at += 2;
            continue;
        }
        if (d[k] >= 0xD0 && d[k] <= 0xD7) {
            f.begin.push_back(begin), f.end.push_back(at);
            begin = at = k + 1;
            continue;
        }
        f.scan_end = at;
        break;
    }
    f.begin.push_back(begin), f.end.push_back(f.scan_end);
    return true;
}

struct Writer {
    std::vector<int16_t> coef;             // exactly the image's blocks
    long blocks = 0, cleared = 0, puts = 0;
    int ybw = 0, cbw = 0, ny = 0, nc = 0;
    bool bad = false;
    long block(int c, int row, int col) {
        const long b = c == 0 ? (long)row * ybw + col : ny + (long)(c - 1) * nc + (long)row * cbw + col;
        if (b < 0 || b >= blocks) bad = true;
        return b;                           // handed on as it is: a wrong place is for the sanitizer to see
    }
    void clear(long b) {
        for (int i = 0; i < 64; ++i) coef[b * 64 + i] = 0;
        ++cleared;
    }
    void put(long b, int at, int v) {
        if (at < 0 || at > 63) bad = true;
        coef[b * 64 + at] = (int16_t)v;
        ++puts;
    }
};

// all segments of a file whose bytes are `bytes` (cut to `limit`) -> the file's status, or -1 on a broken promise
int decode(const File& f, const std::vector<uint8_t>& bytes, long limit) {
    const JeLayout lay = f.lay;
    const int mcux = (f.W + 8 * lay.h - 1) / (8 * lay.h), mcuy = (f.H + 8 * lay.v - 1) / (8 * lay.v);
    const long mcus = (long)mcux * mcuy;
    Writer w;
    w.ybw = mcux * lay.h, w.cbw = mcux, w.ny = mcux * lay.h * mcuy * lay.v, w.nc = mcux * mcuy;
    w.blocks = w.ny + lay.nc * w.nc;
    w.coef.assign(w.blocks * 64, 0x5a5a);
    const int* huff[6];
    for (int c = 0; c < 3; ++c) huff[2 * c] = f.huff[0][f.dc[c]].t, huff[2 * c + 1] = f.huff[1][f.ac[c]].t;
    const long ri = f.ri ? f.ri : mcus, want = (mcus + ri - 1) / ri;
    int status = 0;
    for (long i = 0; i < want; ++i) {
        long b = i < (long)f.begin.size() ? f.begin[i] : limit, e = i < (long)f.end.size() ? f.end[i] : limit;
        if (b > limit) b = limit;
        if (e > limit) e = limit;
        const long first = i * ri, count = mcus - first < ri ? mcus - first : ri;
        const int st = je_decode_segment(bytes.data(), b, e, huff, lay, mcux, (int)first, (int)count, w);
        if (st < 0 || st > 3) return -1;
        if (st > status) status = st;
    }
    // every block cleared exactly once, at most 64 coefficients put into each
    if (w.bad || w.cleared != w.blocks || w.puts > w.blocks * 64) return -1;
    return status;
}

}  // namespace

int main(int argc, char** argv) {
    int failures = 0;
    for (int a = 1; a < argc; ++a) {
        File f;
        FILE* fh = fopen(argv[a], "rb");
        if (!fh) {
            printf("%s: cannot open\n", argv[a]);
            ++failures;
            continue;
        }
        uint8_t buf[4096];
        size_t got;
        while ((got = fread(buf, 1, sizeof buf, fh)) > 0) f.data.insert(f.data.end(), buf, buf + got);
        fclose(fh);
        if (!parse(f)) {
            printf("%s: not a baseline file of a layout this tool reads\n", argv[a]);
            ++failures;
            continue;
        }
        const long n = (long)f.data.size();
        const int whole = decode(f, f.data, n);
        int hist[4] = {0, 0, 0, 0};
        long runs = 0, broken = whole < 0;
        for (long cut = f.scan; cut < f.scan_end; ++cut) {
            const std::vector<uint8_t> head(f.data.begin(), f.data.begin() + cut);     // exact size: a read past it is seen
            const int st = decode(f, head, cut);
            ++runs;
            if (st < 0) ++broken;
            else ++hist[st];
        }
        uint32_t lcg = 12345u;
        std::vector<uint8_t> copy;
        for (int trial = 0; trial < 400; ++trial) {
            copy = f.data;
            const int flips = 1 + trial % 4;
            for (int k = 0; k < flips; ++k) {
                lcg = lcg * 1664525u + 1013904223u;
                const long at = f.scan + (long)((lcg >> 8) % (uint32_t)(f.scan_end - f.scan > 0 ? f.scan_end - f.scan : 1));
                if (at < n) copy[at] ^= (uint8_t)(1u << (lcg >> 29));
            }
            const int st = decode(f, copy, n);
            ++runs;
            if (st < 0) ++broken;
            else ++hist[st];
        }
        printf("%s: %d x %d, %zu segments, status %d; %ld damaged runs: status 0/1/2/3 = %d/%d/%d/%d, broken %ld\n", argv[a], f.H,
               f.W, f.begin.size(), whole, runs, hist[0], hist[1], hist[2], hist[3], broken);
        if (broken) ++failures;
    }
    printf("%s\n", failures ? "FAILED" : "ok");
    return failures ? 1 : 0;
}
