// The arithmetic of the windowed PNG decode (2023-tifs-istvt_amd/csrc/png_window.h) on the host, against vectors the Python
// definition wrote (tests/test_png_window_cpu.py writes them from clips.png_bank_window_host).  The functions are the ones the
// kernels of csrc/png_window.hip call; here every wave of every place of a call is walked in order, first the inflate launch,
// then the unfilter launch, its 64 lanes one after another, with the tables, the box and the window's filtered rows in heap
// blocks of exactly their size, so a read one int or one byte outside them is what AddressSanitizer reports:
//
//     clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//         -I 2023-tifs-istvt_amd/csrc tools/png_window_check.cpp -o build/png_window_check && build/png_window_check VECTORS
//
// Two kinds of line in VECTORS, ints separated by commas within a field, `-` an empty field:
//   T name nbytes n nseg band_max raw_stride rows Wc win_bands win_stride bank IMAGES BANDS
//       the scalars and the tables of a call as the device has them (doctored rows among them): bank = 1 with a bank's image
//       rows of 10 ints, 0 with a batch's of 8
//   P name i BOX FILTERS STATUSES status PLAN SIZES origin MOVED
//       one place of the call above: the file it names, its box, the filter byte of each row of its window as the inflate
//       left them, the inflate's status of each touched band, then what the definition has: the place's status, kfirst, klast,
//       w0, w1 (0,-1,0,0 where the place has no window), the size, the origin and the moved box
// Checked: the lanes' answers taken together equal the host's single pass (pa_rows_fit, pw_marks); the window; every touched
// band's bytes lie inside [0, win_stride); the status by its precedence; what the wave of slot 0 writes; every wave's rows; and
// that the rows of all waves tile [0, w1 - w0) -- no row twice, none left out -- or, for a place with a status, that no wave
// takes a row.  Exit status 0 and one line `png_window_check: N places and M waves agree` where everything gives the
// definition's result.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "png_window.h"

static std::vector<long long> ints(const std::string& s) {
    std::vector<long long> v;
    if (s == "-") return v;
    std::stringstream ss(s);
    std::string t;
    while (std::getline(ss, t, ',')) v.push_back(std::stoll(t));
    return v;
}

static int* block(const std::vector<long long>& v) {              // exactly the ints of v
    int* p = (int*)std::malloc((v.empty() ? 1 : v.size()) * sizeof(int));
    for (size_t i = 0; i < v.size(); ++i) p[i] = (int)v[i];
    return p;
}

static long waves_walked = 0;
static PwCall call;
static int* images = nullptr;
static int* bands = nullptr;
static bool have_call = false;

static bool tables(std::istringstream& ss, const std::string& name) {
    long long nbytes = 0;
    std::string simages, sbands;
    ss >> nbytes >> call.k.n >> call.k.nseg >> call.k.band_max >> call.k.raw_stride >> call.k.Hc >> call.k.Wc >> call.win_bands >>
        call.win_stride >> call.bank >> simages >> sbands;
    call.k.nbytes = (long)nbytes;
    const std::vector<long long> vi = ints(simages), vb = ints(sbands);
    if (!ss || call.k.n < 1 || call.k.nseg < 1 || call.win_bands < 1 || call.win_stride < 16 ||
        (long)vi.size() != (long)call.k.n * (call.bank ? PK_IMAGE_INTS : 8) || (long)vb.size() != (long)call.k.nseg * PK_BAND_INTS) {
        std::printf("%s: a malformed T line\n", name.c_str());
        return false;
    }
    std::free(images);
    std::free(bands);
    images = block(vi);
    bands = block(vb);
    have_call = true;
    return true;
}

// what the lanes of a wave find together, as pw_settle of csrc/png_window.hip has it -> the status, or -1 where the lanes and
// the host's single pass disagree
static int settle(int i, const int* box, int* im, const int** rows, int* R, PwWindow* w) {
    const int st = pw_file(images, bands, call, i, im, rows, R);
    if (st != 0) return st;
    const long stride = 1 + (long)im[PK_W] * im[PK_BPP];
    bool fit = true;
    for (int lane = 0; lane < 64; ++lane) fit = pa_rows_fit(*rows, im[PK_H], stride, *R, im[PK_BANDS], lane, 64) && fit;
    if (fit != pa_rows_fit(*rows, im[PK_H], stride, *R, im[PK_BANDS], 0, 1)) return -1;
    return pw_place(fit, im, *R, box, call, w);
}

static bool place(std::istringstream& ss, const std::string& name) {
    int i = 0, want_status = 0, want_origin = 0;
    std::string sbox, sfilters, sstatuses, splan, ssizes, smoved;
    ss >> i >> sbox >> sfilters >> sstatuses >> want_status >> splan >> ssizes >> want_origin >> smoved;
    const std::vector<long long> vbox = ints(sbox), vfilters = ints(sfilters), vstatuses = ints(sstatuses), vplan = ints(splan),
                                 vsizes = ints(ssizes), vmoved = ints(smoved);
    if (!ss || !have_call || vbox.size() != 4 || vplan.size() != 4 || vsizes.size() != 2 || vmoved.size() != 4) {
        std::printf("%s: a malformed P line\n", name.c_str());
        return false;
    }
    int* box = block(vbox);                                       // exactly the four ints of the box
    const long want_rows = vplan[3] - vplan[2];
    uint8_t* raw = nullptr;
    bool ok = true;
    auto fail = [&](const char* text, long a = 0, long b = 0) {
        std::printf("%s: ", name.c_str());
        std::printf(text, a, b);
        std::printf("\n");
        ok = false;
    };
    std::vector<int> eff(vstatuses.begin(), vstatuses.end());     // the band statuses the inflate launch leaves
    for (int t = 0; t < call.win_bands && ok; ++t) {              // the inflate launch, wave by wave
        ++waves_walked;
        int im[PK_IMAGE_INTS], R = 0;
        const int* rows = nullptr;
        PwWindow w;
        const int st = settle(i, box, im, &rows, &R, &w);
        if (st == -1) fail("the lanes together and the host's pass disagree on the band rows");
        if (st != 0) continue;
        const int k = pw_band(w, t);
        if (k < 0) continue;
        if ((long)eff.size() != w.klast - w.kfirst + 1) {
            fail("%ld band statuses for %ld touched bands", (long)eff.size(), (long)(w.klast - w.kfirst + 1));
            break;
        }
        const int* row = rows + (long)k * PK_BAND_INTS;
        const long at = pw_band_at(row, w, 1 + (long)im[PK_W] * im[PK_BPP], call.win_stride);
        if (at < 0 || !pk_band_ok(row, im, i))
            eff[t] = PK_ROW;
        else if (at + row[PKB_OUT_BYTES] > (long)call.win_stride || at + row[PKB_OUT_BYTES] > (long)call.k.Hc * (1 + (long)im[PK_W] * im[PK_BPP]))
            fail("band %ld writes up to byte %ld of the place's scratch", (long)k, at + row[PKB_OUT_BYTES]);
    }
    std::vector<int> written(want_rows > 0 ? want_rows : 0, 0);
    int got_status = -1, writers = 0;
    for (int t = 0; t < call.win_bands && ok; ++t) {              // the unfilter launch
        ++waves_walked;
        int im[PK_IMAGE_INTS], R = 0, sizes[2] = {0, 0}, origin = 0, moved[4] = {0, 0, 1, 1};
        const int* rows = nullptr;
        PwWindow w;
        int st = settle(i, box, im, &rows, &R, &w);
        if (st == 0) {
            if (w.kfirst != vplan[0] || w.klast != vplan[1] || w.w0 != vplan[2] || w.w1 != vplan[3]) {
                fail("the window is rows %ld to %ld, the definition has another", (long)w.w0, (long)w.w1);
                break;
            }
            if ((long)vfilters.size() != want_rows) {
                fail("%ld filter bytes for a window of %ld rows", (long)vfilters.size(), want_rows);
                break;
            }
            const long stride = 1 + (long)im[PK_W] * im[PK_BPP];
            if (!raw) {
                raw = (uint8_t*)std::calloc((size_t)(want_rows * stride), 1);    // exactly the window's filtered rows
                for (long r = 0; r < want_rows; ++r) raw[r * stride] = (uint8_t)vfilters[r];
            }
            int band = 0;
            for (size_t b = 0; b < eff.size() && band == 0; ++b) band = eff[b];
            int marks = 0;
            if (band == 0) {
                for (int lane = 0; lane < 64; ++lane) marks |= pw_marks(raw, stride, w, R, lane, 64);
                if (marks != pw_marks(raw, stride, w, R, 0, 1)) {
                    fail("the lanes together and the host's pass disagree on the filter bytes");
                    break;
                }
            }
            st = pa_status(band, marks);
            if (st == 0) {
                if (t == 0) {
                    ++writers;
                    sizes[0] = im[PK_H], sizes[1] = im[PK_W], origin = w.w0;
                    moved[0] = box[0] - w.w0, moved[1] = box[1], moved[2] = box[2], moved[3] = box[3];
                }
                const int k = pw_band(w, t);
                if (k >= 0) {
                    int r0, r1;
                    pa_band_span(im[PK_H], R, k, &r0, &r1);
                    if (r0 < w.w0 || r1 > w.w1 || r0 >= r1) {
                        fail("a wave takes rows %ld to %ld outside the window", (long)r0, (long)r1);
                        break;
                    }
                    for (int r = r0; r < r1; ++r) ++written[r - w.w0];
                }
            }
        }
        if (st == -1) {
            fail("the lanes together and the host's pass disagree on the band rows");
            break;
        }
        if (st != want_status) {
            fail("a wave has status %ld, the definition has %ld", (long)st, (long)want_status);
            break;
        }
        if (t != 0) continue;
        got_status = st;
        if (st != 0) {
            ++writers;
            sizes[0] = pw_sized(st) ? im[PK_H] : 0, sizes[1] = pw_sized(st) ? im[PK_W] : 0;
        }
        if (sizes[0] != vsizes[0] || sizes[1] != vsizes[1]) fail("the size is %ld x %ld, the definition has another", sizes[0], sizes[1]);
        if (ok && origin != want_origin) fail("the origin is %ld, the definition has %ld", origin, want_origin);
        for (int q = 0; ok && q < 4; ++q)
            if (moved[q] != vmoved[q]) fail("word %ld of the moved box is %ld, the definition has another", q, moved[q]);
    }
    if (ok && got_status != want_status) fail("the place has status %ld, the definition has %ld", got_status, want_status);
    if (ok && writers != 1) fail("%ld waves write the place's status, one does", writers);
    for (long r = 0; ok && r < (long)written.size(); ++r)
        if (written[r] != (want_status == 0 ? 1 : 0)) fail("row %ld of the window is written %ld times", r, written[r]);
    std::free(box);
    std::free(raw);
    return ok;
}

int main(int argc, char** argv) {
    if (argc != 2) {
        std::fprintf(stderr, "usage: png_window_check VECTORS\n");
        return 2;
    }
    std::ifstream in(argv[1]);
    if (!in) {
        std::fprintf(stderr, "png_window_check: cannot read %s\n", argv[1]);
        return 2;
    }
    std::string line;
    long places = 0, bad = 0;
    while (std::getline(in, line)) {
        if (line.empty()) continue;
        std::istringstream ss(line);
        std::string kind, name;
        ss >> kind >> name;
        if (kind == "T") {
            if (!tables(ss, name)) ++bad;
        } else if (kind == "P") {
            ++places;
            if (!place(ss, name)) ++bad;
        } else {
            std::printf("%s: an unknown kind of line\n", kind.c_str());
            ++bad;
        }
    }
    std::free(images);
    std::free(bands);
    if (bad || places == 0) {
        std::printf("png_window_check: %ld of %ld places disagree\n", bad, places);
        return 1;
    }
    std::printf("png_window_check: %ld places and %ld waves agree\n", places, waves_walked);
    return 0;
}
