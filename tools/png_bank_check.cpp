// The lookup of the PNG bank (2023-tifs-istvt_amd/csrc/png_bank.h) and the band inflate behind it (pi_inflate<true> of
// csrc/png_inflate.h) on the host, against vectors the Python definition wrote (tests/test_png_bank_cpu.py writes them from
// clips.png_bank and clips.png_bank_decode_host).  The functions are the ones the kernels of csrc/png_bank.hip call; here every
// wave of a call is run in order, with the tables in heap blocks of exactly their size, so a read one int outside a table is
// what AddressSanitizer reports:
//
//     clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//         -I 2023-tifs-istvt_amd/csrc tools/png_bank_check.cpp -o png_bank_check && ./png_bank_check VECTORS
//
// Two kinds of lines in VECTORS, ints separated by commas within a field:
//   L name nbytes n nseg band_max raw_stride Hc Wc m IMAGES BANDS INDEX STATUS BASES
//       one call's lookup: the image rows (n * 10 ints), the band rows (nseg * 5), the index (m), the status the definition
//       has for every place as far as the tables decide it (8, 9 or 0), and every place's 64-bit base as its row has it (-1
//       outside the bank).  No stream is there: what a wave would read and write is checked as integers against nbytes and
//       the scratch row, and the base pointer against BASES.
//   B name status k nbytes n nseg band_max raw_stride Hc Wc IMAGE BAND STREAM EXPECTED
//       band k of one file through the bank's rows: its image row (10 ints) and band row (5 ints) must pass the checks, then
//       the band is inflated in heap blocks of exactly its input's and output's length, at the file-relative offset it has.
//       STREAM and EXPECTED in hex (- for none; EXPECTED is - where the status is not 0).
// Exit status 0 and one line `png_bank_check: N lookups and M bands agree` where everything gives the definition's result.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "png_bank.h"
#include "png_inflate.h"

static std::vector<long long> ints(const std::string& s) {
    std::vector<long long> v;
    if (s == "-") return v;
    std::stringstream ss(s);
    std::string t;
    while (std::getline(ss, t, ',')) v.push_back(std::stoll(t));
    return v;
}

static std::vector<uint8_t> unhex(const std::string& s) {
    std::vector<uint8_t> v;
    if (s == "-") return v;
    for (size_t i = 0; i + 1 < s.size(); i += 2) v.push_back((uint8_t)std::stoi(s.substr(i, 2), nullptr, 16));
    return v;
}

// a heap block of exactly v.size() ints
static int* block(const std::vector<long long>& v) {
    int* p = (int*)std::malloc(v.size() ? v.size() * sizeof(int) : 1);
    for (size_t i = 0; i < v.size(); ++i) p[i] = (int)v[i];
    return p;
}

static bool lookup(std::istringstream& ss, const std::string& name) {
    PkCall c;
    int m = 0;
    std::string si, sb, sx, sst, sba;
    ss >> c.nbytes >> c.n >> c.nseg >> c.band_max >> c.raw_stride >> c.Hc >> c.Wc >> m >> si >> sb >> sx >> sst >> sba;
    const std::vector<long long> vi = ints(si), vb = ints(sb), vx = ints(sx), want = ints(sst), bases = ints(sba);
    if ((long)vi.size() != (long)c.n * PK_IMAGE_INTS || (long)vb.size() != (long)c.nseg * PK_BAND_INTS || (int)vx.size() != m ||
        (int)want.size() != m || (int)bases.size() != m) {
        std::printf("%s: a malformed line\n", name.c_str());
        return false;
    }
    const long scratch_bytes = (long)m * c.raw_stride + 4L * m * c.band_max;
    if (!pk_scalars_ok(c, m, scratch_bytes) || pk_scalars_ok(c, m, scratch_bytes - 1)) {
        std::printf("%s: the scalars of the call and the scratch size disagree\n", name.c_str());
        return false;
    }
    int* images = block(vi);
    int* bands = block(vb);
    int* index = block(vx);
    std::vector<int> band_status((size_t)m * c.band_max, -1);    // -1: never written, and never read if the lookup is right
    bool ok = true;
    const uintptr_t bytes = 0x100000;                            // the bank's data as an address; nothing is read through it
    for (long b = 0; b < (long)m * c.band_max && ok; ++b) {      // the inflate launch, wave by wave
        int j, k;
        pk_wave((int)b, c.band_max, &j, &k);
        const int* im = nullptr;
        const int* row = nullptr;
        const int plan = pk_band_plan(images, bands, c, index[j], k, &im, &row);
        if (plan == PK_SKIP) continue;
        if (plan == PK_RUN) {
            const int64_t base = pk_base(im);
            const uintptr_t data = bytes + (uintptr_t)base;
            if (base != bases[j] || data - bytes != (uintptr_t)bases[j]) {
                std::printf("%s: place %d has base %lld, the definition has %lld\n", name.c_str(), j, (long long)base, bases[j]);
                ok = false;
            }
            if (row[PKB_BEGIN] < 0 || row[PKB_BEGIN] > row[PKB_END] || base + row[PKB_END] > c.nbytes ||
                row[PKB_OUT] < 0 || row[PKB_OUT_BYTES] < 0 || (long)row[PKB_OUT] + row[PKB_OUT_BYTES] > c.raw_stride) {
                std::printf("%s: wave %ld would leave the bank's bytes or its row of the scratch\n", name.c_str(), b);
                ok = false;
            }
        }
        band_status[(size_t)j * c.band_max + k] = plan == PK_RUN ? 0 : PK_ROW;
    }
    for (int j = 0; j < m && ok; ++j) {                          // the unfilter launch
        const int* im = nullptr;
        int st = pk_place_plan(images, c, index[j], &im);
        if (st == 0)
            for (int k = 0; k < im[PK_BANDS] && st == 0; ++k) {
                st = band_status[(size_t)j * c.band_max + k];
                if (st < 0) {
                    std::printf("%s: place %d reads the status of band %d, which no wave wrote\n", name.c_str(), j, k);
                    ok = false;
                }
            }
        if (ok && st != want[j]) {
            std::printf("%s: place %d has status %d, the definition has %lld\n", name.c_str(), j, st, want[j]);
            ok = false;
        }
    }
    std::free(index);
    std::free(bands);
    std::free(images);
    return ok;
}

static bool band(std::istringstream& ss, const std::string& name) {
    PkCall c;
    int status = 0, k = 0;
    std::string si, sb, hs, ho;
    ss >> status >> k >> c.nbytes >> c.n >> c.nseg >> c.band_max >> c.raw_stride >> c.Hc >> c.Wc >> si >> sb >> hs >> ho;
    const std::vector<long long> vi = ints(si), vb = ints(sb);
    const std::vector<uint8_t> stream = unhex(hs), want = unhex(ho);
    if (vi.size() != PK_IMAGE_INTS || vb.size() != PK_BAND_INTS) {
        std::printf("%s: a malformed line\n", name.c_str());
        return false;
    }
    int* im = block(vi);
    int* row = block(vb);
    bool ok = true;
    if (!pk_image_ok(im, c) || k >= im[PK_BANDS] || !pk_band_ok(row, im, row[PKB_FILE]) ||
        (long)stream.size() != (long)row[PKB_END] - row[PKB_BEGIN]) {
        std::printf("%s: the bank's rows do not pass the checks\n", name.c_str());
        ok = false;
    } else {
        const long expected = row[PKB_OUT_BYTES];
        // exact lengths; the base lies `begin` bytes in front of the block (never read: no byte in front of `begin` is), so
        // the band starts at the offset it has in its file, which the base of a multiple of 16 keeps mod 4
        uint8_t* src = (uint8_t*)std::malloc(stream.size() ? stream.size() : 1);
        uint8_t* out = (uint8_t*)std::malloc(expected ? (size_t)expected : 1);
        PiTables* T = (PiTables*)std::malloc(sizeof(PiTables));
        if (!stream.empty()) std::memcpy(src, stream.data(), stream.size());
        std::memset(out, 0xA5, expected ? (size_t)expected : 1);
        std::memset(T, 0, sizeof(PiTables));
        const uint8_t* base = reinterpret_cast<const uint8_t*>(reinterpret_cast<uintptr_t>(src) - (uintptr_t)row[PKB_BEGIN]);
        const int got = pi_inflate<true>(base, row[PKB_BEGIN], row[PKB_END], out, (int)expected, T, 0, k != im[PK_BANDS] - 1);
        if (got != status) {
            std::printf("%s: status %d, the definition has %d\n", name.c_str(), got, status);
            ok = false;
        } else if (status == 0 && ((long)want.size() != expected || std::memcmp(out, want.data(), (size_t)expected) != 0)) {
            std::printf("%s: the bytes differ from the definition's\n", name.c_str());
            ok = false;
        }
        std::free(T);
        std::free(out);
        std::free(src);
    }
    std::free(row);
    std::free(im);
    return ok;
}

int main(int argc, char** argv) {
    if (argc != 2) {
        std::fprintf(stderr, "usage: png_bank_check VECTORS\n");
        return 2;
    }
    std::ifstream in(argv[1]);
    if (!in) {
        std::fprintf(stderr, "png_bank_check: cannot read %s\n", argv[1]);
        return 2;
    }
    std::string line;
    int lookups = 0, bands = 0, bad = 0;
    while (std::getline(in, line)) {
        if (line.empty() || line[0] == '#') continue;
        std::istringstream ss(line);
        std::string kind, name;
        ss >> kind >> name;
        if (kind == "L") {
            ++lookups;
            bad += !lookup(ss, name);
        } else {
            ++bands;
            bad += !band(ss, name);
        }
    }
    if (bad || !(lookups + bands)) {
        std::printf("png_bank_check: %d of %d lines disagree\n", bad, lookups + bands);
        return 1;
    }
    std::printf("png_bank_check: %d lookups and %d bands agree\n", lookups, bands);
    return 0;
}
