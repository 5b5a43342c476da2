// The arithmetic of PNG bands that stand alone (2023-tifs-istvt_amd/csrc/png_alone.h) on the host, against vectors the Python
// definition wrote (tests/test_png_alone_cpu.py writes them from clips.png_decode_alone_host and clips.png_bank_decode_host).
// The functions are the ones the kernels of csrc/png_alone.hip call; here every wave of a flagged file is walked in order, its
// 64 lanes one after another, with the tables in heap blocks of exactly their size, so a read one int or one byte outside a
// table is what AddressSanitizer reports:
//
//     clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//         -I 2023-tifs-istvt_amd/csrc tools/png_alone_check.cpp -o png_alone_check && ./png_alone_check VECTORS
//
// One kind of line in VECTORS, ints separated by commas within a field:
//   F name H W bpp count waves ROWS FILTERS STATUSES status R SPANS
//       one flagged file: its band rows as the decoder has them (count * 5 ints; doctored rows among them), the filter byte
//       of each of its H rows as the inflate left them, the status of each of its count bands, then what the definition has:
//       the file's status, R (0 where the band rows are refused: status 9) and per band k the rows r0:r1 its wave takes.  waves
//       >= count: the waves a launch runs for the file (band_max of a bank); those from count on must leave.
// Checked: the lanes' answers taken together equal the host's single pass (pa_rows_fit, pa_marks); the plan of every wave;
// the status; every wave's rows; and that the rows of all waves tile [0, H) -- no row twice, none left out -- or, for a
// refused file, that the wave of band 0 alone writes.  The filtered rows stand in a block of exactly H (1 + W bpp) bytes.
// Exit status 0 and one line `png_alone_check: N files and M waves agree` where everything gives the definition's result.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "png_alone.h"

static std::vector<long long> ints(const std::string& s) {
    std::vector<long long> v;
    if (s == "-") return v;
    std::stringstream ss(s);
    std::string t;
    while (std::getline(ss, t, ',')) v.push_back(std::stoll(t));
    return v;
}

static long waves_walked = 0;

static bool file(std::istringstream& ss, const std::string& name) {
    int H = 0, W = 0, bpp = 0, count = 0, waves = 0, want_status = 0, want_R = 0;
    std::string srows, sfilters, sstatuses, sspans;
    ss >> H >> W >> bpp >> count >> waves >> srows >> sfilters >> sstatuses >> want_status >> want_R >> sspans;
    const std::vector<long long> vrows = ints(srows), vfilters = ints(sfilters), vstatuses = ints(sstatuses);
    std::vector<std::string> spans;
    {
        std::stringstream sp(sspans);
        std::string t;
        while (sspans != "-" && std::getline(sp, t, ',')) spans.push_back(t);
    }
    if (H < 1 || W < 1 || bpp < 1 || count < 1 || waves < count || (long)vrows.size() != (long)count * PA_BAND_INTS ||
        (int)vfilters.size() != H || (int)vstatuses.size() != count || (want_R > 0 && (int)spans.size() != count)) {
        std::printf("%s: a malformed line\n", name.c_str());
        return false;
    }
    const long stride = 1 + (long)W * bpp;
    int* rows = (int*)std::malloc(vrows.size() * sizeof(int));                  // exactly count band rows
    for (size_t i = 0; i < vrows.size(); ++i) rows[i] = (int)vrows[i];
    uint8_t* raw = (uint8_t*)std::calloc((size_t)(H * stride), 1);              // exactly the file's filtered rows
    for (int r = 0; r < H; ++r) raw[r * stride] = (uint8_t)vfilters[r];
    bool ok = true;
    std::vector<int> written(H, 0);
    int refused = 0, got_status = -1;
    for (int k = 0; k < waves && ok; ++k) {                       // the unfilter launch, wave by wave
        ++waves_walked;
        const int R = pa_alone_rows(rows[PAB_OUT_BYTES], stride);
        bool fit = R > 0;
        for (int lane = 0; lane < 64 && R > 0; ++lane) fit = pa_rows_fit(rows, H, stride, R, count, lane, 64) && fit;
        if (fit != (R > 0 && pa_rows_fit(rows, H, stride, R, count, 0, 1))) {
            std::printf("%s: the lanes together and the host's pass disagree on the band rows\n", name.c_str());
            ok = false;
            break;
        }
        const int plan = pa_wave_plan(fit, k, count);
        if (plan == PA_REFUSE) {
            ++refused;
            got_status = PA_NO_ROW;
        }
        if (plan != PA_ROWS) continue;
        if (R != want_R) {
            std::printf("%s: R is %d, the definition has %d\n", name.c_str(), R, want_R);
            ok = false;
            break;
        }
        int band = 0;
        for (int b = 0; b < count && band == 0; ++b) band = (int)vstatuses[b];
        int marks = 0;
        if (band == 0) {
            for (int lane = 0; lane < 64; ++lane) marks |= pa_marks(raw, stride, H, R, lane, 64);
            if (marks != pa_marks(raw, stride, H, R, 0, 1)) {
                std::printf("%s: the lanes together and the host's pass disagree on the filter bytes\n", name.c_str());
                ok = false;
                break;
            }
        }
        const int st = pa_status(band, marks);
        if (k == 0) got_status = st;
        if (st != want_status) {
            std::printf("%s: wave %d has status %d, the definition has %d\n", name.c_str(), k, st, want_status);
            ok = false;
            break;
        }
        int r0, r1;
        pa_band_span(H, R, k, &r0, &r1);
        char text[64];
        std::snprintf(text, sizeof text, "%d:%d", r0, r1);
        if (spans[k] != text) {
            std::printf("%s: wave %d takes rows %s, the definition has %s\n", name.c_str(), k, text, spans[k].c_str());
            ok = false;
            break;
        }
        if (r0 < 0 || r1 > H || r0 >= r1) {
            std::printf("%s: wave %d takes rows %s of %d\n", name.c_str(), k, text, H);
            ok = false;
            break;
        }
        for (int r = r0; r < r1; ++r) ++written[r];
    }
    if (ok && got_status != want_status) {
        std::printf("%s: the file has status %d, the definition has %d\n", name.c_str(), got_status, want_status);
        ok = false;
    }
    if (ok && want_R == 0 && refused != 1) {
        std::printf("%s: %d waves refuse the file, one does\n", name.c_str(), refused);
        ok = false;
    }
    for (int r = 0; ok && r < H; ++r)
        if (written[r] != (want_R == 0 ? 0 : 1)) {
            std::printf("%s: row %d is written %d times\n", name.c_str(), r, written[r]);
            ok = false;
        }
    std::free(rows);
    std::free(raw);
    return ok;
}

int main(int argc, char** argv) {
    if (argc != 2) {
        std::fprintf(stderr, "usage: png_alone_check VECTORS\n");
        return 2;
    }
    std::ifstream in(argv[1]);
    if (!in) {
        std::fprintf(stderr, "png_alone_check: cannot read %s\n", argv[1]);
        return 2;
    }
    std::string line;
    long files = 0, bad = 0;
    while (std::getline(in, line)) {
        if (line.empty()) continue;
        std::istringstream ss(line);
        std::string kind, name;
        ss >> kind >> name;
        if (kind != "F") {
            std::printf("%s: an unknown kind of line\n", kind.c_str());
            ++bad;
            continue;
        }
        ++files;
        if (!file(ss, name)) ++bad;
    }
    if (bad || files == 0) {
        std::printf("png_alone_check: %ld of %ld files disagree\n", bad, files);
        return 1;
    }
    std::printf("png_alone_check: %ld files and %ld waves agree\n", files, waves_walked);
    return 0;
}
