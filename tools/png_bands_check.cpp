// The band mode of the PNG path's DEFLATE decoder (pi_inflate<true> of 2023-tifs-istvt_amd/csrc/png_inflate.h) on the host, with
// one lane, against the vectors the Python definition wrote (tests/test_png_bands_cpu.py writes them from
// clips.png_inflate_bands_host: every band of every file of the GPU tests, the bands of the lying indexes and of the damaged
// files among them).  Every band runs in heap blocks of exactly its input's and its output's length, at the byte offset mod 4
// it has in its batch, so a read or a write one byte outside either is what AddressSanitizer reports:
//
//     clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//         -I 2023-tifs-istvt_amd/csrc tools/png_bands_check.cpp -o png_bands_check && ./png_bands_check VECTORS
//
// A line of VECTORS: name, status, 1 for a band that is not its file's last, begin mod 4, expected length, the band's bytes in
// hex (- for none), expected bytes in hex (- where the status is not 0).  Exit status 0 and one line `png_bands_check: N bands
// agree` where every band gives its status and, at status 0, its bytes.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "png_inflate.h"

static std::vector<uint8_t> unhex(const std::string& s) {
    std::vector<uint8_t> v;
    if (s == "-") return v;
    for (size_t i = 0; i + 1 < s.size(); i += 2) v.push_back((uint8_t)std::stoi(s.substr(i, 2), nullptr, 16));
    return v;
}

int main(int argc, char** argv) {
    if (argc != 2) {
        std::fprintf(stderr, "usage: png_bands_check VECTORS\n");
        return 2;
    }
    std::ifstream in(argv[1]);
    if (!in) {
        std::fprintf(stderr, "png_bands_check: cannot read %s\n", argv[1]);
        return 2;
    }
    std::string line;
    int cases = 0, bad = 0;
    while (std::getline(in, line)) {
        if (line.empty() || line[0] == '#') continue;
        std::istringstream ss(line);
        std::string name, hs, ho;
        int status = 0, middle = 0, phase = 0;
        long expected = 0;
        ss >> name >> status >> middle >> phase >> expected >> hs >> ho;
        const std::vector<uint8_t> band = unhex(hs), want = unhex(ho);
        // exact lengths.  The reader counts bytes from a base and takes single bytes up to a multiple of 4, then words: with the
        // base `phase` bytes in front of the block (never read: no byte in front of `begin` is) the band starts where it does
        // in its batch, phase = begin mod 4.
        uint8_t* src = (uint8_t*)std::malloc(band.size() ? band.size() : 1);
        uint8_t* out = (uint8_t*)std::malloc(expected ? (size_t)expected : 1);
        PiTables* T = (PiTables*)std::malloc(sizeof(PiTables));
        if (!band.empty()) std::memcpy(src, band.data(), band.size());
        std::memset(out, 0xA5, expected ? (size_t)expected : 1);
        std::memset(T, 0, sizeof(PiTables));
        const uint8_t* base = reinterpret_cast<const uint8_t*>(reinterpret_cast<uintptr_t>(src) - (uintptr_t)phase);
        const int got = pi_inflate<true>(base, phase, phase + (int)band.size(), out, (int)expected, T, 0, middle != 0);
        ++cases;
        if (got != status) {
            std::printf("%s: status %d, the definition has %d\n", name.c_str(), got, status);
            ++bad;
        } else if (status == 0 && ((long)want.size() != expected || std::memcmp(out, want.data(), (size_t)expected) != 0)) {
            std::printf("%s: the bytes differ from the definition's\n", name.c_str());
            ++bad;
        }
        std::free(T);
        std::free(out);
        std::free(src);
    }
    if (bad || !cases) {
        std::printf("png_bands_check: %d of %d bands disagree\n", bad, cases);
        return 1;
    }
    std::printf("png_bands_check: %d bands agree\n", cases);
    return 0;
}
