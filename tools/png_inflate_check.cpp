// The DEFLATE decoder of the PNG path (2023-tifs-istvt_amd/csrc/png_inflate.h) on the host, with one lane, against the vectors
// the Python definition wrote (tests/test_png_cpu.py writes them from clips._png_inflate: streams, expected bytes, expected
// statuses; damaged streams among them).  Every case runs in heap buffers of exactly the stream's and the output's length, so
// a read or a write one byte outside either is what AddressSanitizer reports:
//
//     clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//         -I 2023-tifs-istvt_amd/csrc tools/png_inflate_check.cpp -o png_inflate_check && ./png_inflate_check VECTORS
//
// A line of VECTORS: name, status, expected length, stream in hex (- for none), expected bytes in hex (- where the status is not
// 0).  Exit status 0 and one line `png_inflate_check: N cases agree` where every case gives its status and, at status 0, its bytes.
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
        std::fprintf(stderr, "usage: png_inflate_check VECTORS\n");
        return 2;
    }
    std::ifstream in(argv[1]);
    if (!in) {
        std::fprintf(stderr, "png_inflate_check: cannot read %s\n", argv[1]);
        return 2;
    }
    std::string line;
    int cases = 0, bad = 0;
    while (std::getline(in, line)) {
        if (line.empty() || line[0] == '#') continue;
        std::istringstream ss(line);
        std::string name, hs, ho;
        int status = 0;
        long expected = 0;
        ss >> name >> status >> expected >> hs >> ho;
        const std::vector<uint8_t> stream = unhex(hs), want = unhex(ho);
        // exact lengths: malloc gives 16-byte aligned blocks, so the word path of the reader runs as it does on the device
        uint8_t* src = (uint8_t*)std::malloc(stream.size() ? stream.size() : 1);
        uint8_t* out = (uint8_t*)std::malloc(expected ? (size_t)expected : 1);
        PiTables* T = (PiTables*)std::malloc(sizeof(PiTables));
        if (!stream.empty()) std::memcpy(src, stream.data(), stream.size());
        std::memset(out, 0xA5, expected ? (size_t)expected : 1);
        std::memset(T, 0, sizeof(PiTables));
        const int got = pi_inflate(src, 0, (int)stream.size(), out, (int)expected, T, 0);
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
        std::printf("png_inflate_check: %d of %d cases disagree\n", bad, cases);
        return 1;
    }
    std::printf("png_inflate_check: %d cases agree\n", cases);
    return 0;
}
