// The DEFLATE coder of the PNG writer (2023-tifs-istvt_amd/csrc/png_deflate.h) on the host, with one lane, against the vectors
// the Python definition wrote (tests/test_png_encode_cpu.py writes them from clips.png_encode_banded_host).  Every case runs in
// heap buffers of exactly the band's and the result's length, so a read or a write one byte outside either is what
// AddressSanitizer reports:
//
//     clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//         -I 2023-tifs-istvt_amd/csrc tools/png_deflate_check.cpp -o png_deflate_check && ./png_deflate_check VECTORS
//
// A line of VECTORS is one of
//     band NAME FINAL SHIFT ROWS CODED    the filtered bytes of one band in hex and what the definition codes them to; the result
//                                         is written SHIFT bytes behind a 4-byte boundary, as a band lies in a file
//     file NAME H W BPP BAND_ROWS ROWS FILE   the filtered rows of a whole image and the definition's file: bands as above, then
//                                         the container with the header's Adler-32 combine and CRC-32 fold over 64 slices
// Exit status 0 and one line `png_deflate_check: N cases agree` where every case gives the definition's bytes.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "png_deflate.h"

static std::vector<uint8_t> unhex(const std::string& s) {
    std::vector<uint8_t> v;
    if (s == "-") return v;
    v.reserve(s.size() / 2);
    for (size_t i = 0; i + 1 < s.size(); i += 2) {
        auto nib = [](char c) { return c <= '9' ? c - '0' : (c | 32) - 'a' + 10; };
        v.push_back((uint8_t)(nib(s[i]) << 4 | nib(s[i + 1])));
    }
    return v;
}

// one band -> its bytes, coded into an exact heap block `shift` bytes behind a 4-byte boundary; the Adler parts on the way
static std::vector<uint8_t> code_band(const uint8_t* rows, int nb, int final, int shift, uint32_t* a, uint32_t* b) {
    uint8_t* band = (uint8_t*)std::malloc((size_t)nb);
    std::memcpy(band, rows, (size_t)nb);
    PdWork* w = (PdWork*)std::malloc(sizeof(PdWork));
    PdStage* s = (PdStage*)std::malloc(sizeof(PdStage));
    std::memset(w, 0xA5, sizeof(PdWork));
    std::memset(s, 0xA5, sizeof(PdStage));
    for (int i = 0; i < PD_SLOTS; ++i) w->counts[i] = 0;
    pd_count_band(band, nb, w->counts, a, b, 0);
    pd_build(*w);
    for (int i = 0; i < PD_SLOTS; ++i) s->words[i] = w->words[i];
    // malloc's blocks are 16-byte aligned: the band starts `shift` bytes behind a boundary, the block ends with the band, and
    // the bytes in front of it keep their fill
    uint8_t* block = (uint8_t*)std::malloc((size_t)(shift + w->band_bytes));
    std::memset(block, 0xEE, (size_t)shift);
    pd_store_band(band, nb, final, s->words, w->header, w->header_bits, block + shift, s->stage, 0);
    std::vector<uint8_t> out;
    for (int i = 0; i < shift; ++i)
        if (block[i] != 0xEE) out.push_back(0);                  // a byte in front of the band was written: the lengths will differ
    out.insert(out.end(), block + shift, block + shift + w->band_bytes);
    std::free(block);
    std::free(s);
    std::free(w);
    std::free(band);
    return out;
}

static void be32(std::vector<uint8_t>& v, uint32_t x) {
    for (int k = 3; k >= 0; --k) v.push_back((uint8_t)(x >> (8 * k)));
}

static uint32_t crc_slices(const uint8_t* p, long total) {       // as png_container_kernel folds it
    uint32_t table[256];
    for (uint32_t i = 0; i < 256; ++i) table[i] = pd_crc_entry(i);
    const long slice = (total + 63) / 64;
    uint32_t all = 0;
    for (int lane = 0; lane < 64; ++lane) {
        const long lo = std::min(total, lane * slice), hi = std::min(total, lo + slice);
        uint32_t crc = 0xffffffffu;
        for (long i = lo; i < hi; ++i) crc = table[(crc ^ p[i]) & 255] ^ (crc >> 8);
        crc = hi > lo ? ~crc : 0u;
        all = lane == 0 ? crc : pd_crc_combine(all, crc, pd_crc_shift((uint64_t)(hi - lo)));
    }
    return all;
}

static std::vector<uint8_t> code_file(const std::vector<uint8_t>& rows, int H, int W, int bpp, int R) {
    const long stride = 1 + (long)W * bpp;
    std::vector<uint8_t> body = {'I', 'D', 'A', 'T', 0x78, 0x01};
    uint32_t A = 1, B = 0;
    for (int r0 = 0; r0 < H; r0 += R) {
        const int r1 = std::min(H, r0 + R), nb = (int)((r1 - r0) * stride);
        uint32_t a = 0, b = 0;
        const std::vector<uint8_t> part = code_band(rows.data() + r0 * stride, nb, r1 == H, (int)(body.size() + 37) & 3, &a, &b);
        body.insert(body.end(), part.begin(), part.end());
        pd_adler_append(A, B, a, b, (uint32_t)nb);
    }
    be32(body, (B << 16) | A);
    std::vector<uint8_t> file = {0x89, 'P', 'N', 'G', '\r', '\n', 0x1a, '\n', 0, 0, 0, 13};
    std::vector<uint8_t> ihdr = {'I', 'H', 'D', 'R'};
    be32(ihdr, (uint32_t)W);
    be32(ihdr, (uint32_t)H);
    const uint8_t rest[5] = {8, (uint8_t)(bpp == 1 ? 0 : bpp == 3 ? 2 : 6), 0, 0, 0};
    ihdr.insert(ihdr.end(), rest, rest + 5);
    file.insert(file.end(), ihdr.begin(), ihdr.end());
    be32(file, crc_slices(ihdr.data(), (long)ihdr.size()));
    be32(file, (uint32_t)(body.size() - 4));
    file.insert(file.end(), body.begin(), body.end());
    be32(file, crc_slices(body.data(), (long)body.size()));
    const uint8_t iend[12] = {0, 0, 0, 0, 'I', 'E', 'N', 'D', 0xae, 0x42, 0x60, 0x82};
    file.insert(file.end(), iend, iend + 12);
    return file;
}

int main(int argc, char** argv) {
    if (argc != 2) {
        std::fprintf(stderr, "usage: png_deflate_check VECTORS\n");
        return 2;
    }
    std::ifstream in(argv[1]);
    if (!in) {
        std::fprintf(stderr, "png_deflate_check: cannot read %s\n", argv[1]);
        return 2;
    }
    std::string line;
    int cases = 0, bad = 0;
    while (std::getline(in, line)) {
        if (line.empty() || line[0] == '#') continue;
        std::istringstream ss(line);
        std::string kind, name, h1, h2;
        ss >> kind >> name;
        std::vector<uint8_t> got, want;
        if (kind == "band") {
            int final = 0, shift = 0;
            ss >> final >> shift >> h1 >> h2;
            const std::vector<uint8_t> rows = unhex(h1);
            want = unhex(h2);
            uint32_t a = 0, b = 0;
            got = code_band(rows.data(), (int)rows.size(), final, shift & 3, &a, &b);
        } else if (kind == "file") {
            int H = 0, W = 0, bpp = 0, R = 0;
            ss >> H >> W >> bpp >> R >> h1 >> h2;
            const std::vector<uint8_t> rows = unhex(h1);
            want = unhex(h2);
            if (H < 1 || W < 1 || R < 1 || (long)rows.size() != H * (1 + (long)W * bpp)) {
                std::printf("%s: a malformed vector\n", name.c_str());
                ++cases, ++bad;
                continue;
            }
            got = code_file(rows, H, W, bpp, R);
        } else {
            std::printf("%s: an unknown kind of vector\n", kind.c_str());
            ++cases, ++bad;
            continue;
        }
        ++cases;
        if (got != want) {
            size_t at = 0;
            while (at < got.size() && at < want.size() && got[at] == want[at]) ++at;
            std::printf("%s: %zu bytes, the definition has %zu; the first difference is at byte %zu\n", name.c_str(), got.size(),
                        want.size(), at);
            ++bad;
        }
    }
    if (bad || !cases) {
        std::printf("png_deflate_check: %d of %d cases disagree\n", bad, cases);
        return 1;
    }
    std::printf("png_deflate_check: %d cases agree\n", cases);
    return 0;
}
