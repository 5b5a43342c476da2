// The split decode of a JPEG bank (DESIGN.md "JPEG bank, split") on the host, under sanitizers:
//
//     clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//         -I include -I 2023-tifs-istvt_amd/csrc tools/jpeg_bank_split_check.cpp -o jpeg_bank_split_check
//     ./jpeg_bank_split_check
//
// What istvt_jpeg_decode_indexed_split_u8 launches, with the arithmetic the kernels compile (csrc/jpeg_bank_scan.h,
// csrc/jpeg_entropy_split.h) and every table in a heap buffer of its exact size, so AddressSanitizer sees a store outside one.
// The bank is made here: scans of random coefficients written with a DC table of T.81 K.3 and a small AC table of this
// tool's own, laid end to end.  Its places: 4:2:0 without restart markers (long enough that the 256-lane cap raises the
// chunk size at chunk 16), 4:4:4 with a marker per MCU row, 4:2:2 without markers, greyscale with a marker per MCU row, an
// empty place, and a 4:4:4 file without markers whose one segment is longer than seg_bytes_max, the longest of the others.
// At chunk 16, 37 and 128:
//   (1) the row bound: js_chunks(L) <= chunk_rows = min(256, max(1, ceil(seg_bytes_max / chunk))) for every L <= seg_bytes_max
//   (2) the plan (jb_plan_status with the limit, jb_plan_image, jb_plan_segment) for indices inside, outside and repeated;
//       the over-long file reads as status 5, and as 0 without a limit
//   (3) every planned segment row s as jpeg_entropy_split_kernel<LANES, true> treats it, lanes in order: the kernel's
//       comparisons, the chunk rule, js_row0<true>, the guesses and rounds, the scan of the tallies, js_write, the row
//       stores.  Required: every row store inside [s * R, (s + 1) * R) and inside a table of exactly m * seg_max * R rows;
//       rows behind a segment's chunks, of padded segment rows and of places that are not decodable untouched;
//       coefficients and status those of je_decode_segment on the same planned tables; the blocks a sound segment's lanes
//       started sum to its blocks
//   (4) a row stride smaller than a segment's chunk count is refused (js_row0 -> -1)
// Prints one line per chunk size and `ok`; exit status 1 on any failure.  A hand tool for a CPU: nothing here touches a GPU.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "jpeg_bank_scan.h"
#include "jpeg_entropy_split.h"

namespace {

int failures = 0;

void fail(const char* what, long a, long b) {
    if (++failures <= 20) std::printf("FAILED %s (%ld, %ld)\n", what, a, b);
}

uint32_t lcg_state = 2463534242u;
uint32_t lcg() {
    lcg_state = lcg_state * 1664525u + 1013904223u;
    return lcg_state >> 8;
}

// a Huffman table from its counts per length and its values: the decode form (clips.jpeg_huffman_table) and the codes
struct Table {
    int t[JE_HUFF_INTS];
    int code[256], len[256];
};

void make_table(const std::vector<int>& counts, const std::vector<int>& values, Table& out) {
    int code = 0, at = 0;
    std::memset(out.len, 0, sizeof out.len);
    for (int l = 1; l <= 16; ++l) {
        out.t[16 + l - 1] = at - code;
        for (int i = 0; i < counts[(size_t)l - 1]; ++i) out.code[values[(size_t)at + i]] = code + i, out.len[values[(size_t)at + i]] = l;
        code += counts[(size_t)l - 1];
        at += counts[(size_t)l - 1];
        out.t[l - 1] = code << (16 - l);
        code <<= 1;
    }
    for (int i = 0; i < 256; ++i) out.t[32 + i] = i < (int)values.size() ? values[(size_t)i] : 0;
}

struct BitWriter {
    std::vector<uint8_t> bytes;
    uint32_t acc = 0;
    int n = 0;
    void put(int value, int bits) {
        for (int b = bits - 1; b >= 0; --b) {
            acc = (acc << 1) | ((value >> b) & 1);
            if (++n == 8) {
                bytes.push_back((uint8_t)acc);
                if ((acc & 0xFF) == 0xFF) bytes.push_back(0);
                acc = 0, n = 0;
            }
        }
    }
    void flush() {                          // pad with ones, as an encoder does
        while (n) put(1, 1);
    }
};

int category(int v) {
    int a = v < 0 ? -v : v, c = 0;
    while (a) ++c, a >>= 1;
    return c;
}

void put_value(BitWriter& w, int v, int size) { w.put(v >= 0 ? v : v + (1 << size) - 1, size); }

// one block of random coefficients: a DC difference of up to 11 bits now and then, ACs of 1..4 bits behind runs of 0..17
void put_block(BitWriter& w, const Table& dc, const Table& ac, int dense) {
    int diff = (int)(lcg() % 121) - 60;
    if (lcg() % 16 == 0) diff = (int)(lcg() % 4001) - 2000;
    const int size = category(diff);
    w.put(dc.code[size], dc.len[size]);
    if (size) put_value(w, diff, size);
    int k = 1;
    for (int i = 0; i < dense && k < 64; ++i) {
        int run = (int)(lcg() % 4);
        if (lcg() % 32 == 0) run += 16;
        if (k + run > 63) break;
        if (run >= 16) w.put(ac.code[0xF0], ac.len[0xF0]), run -= 16, k += 16;
        int v = (int)(lcg() % 15) + 1;
        if (lcg() & 1) v = -v;
        const int s = category(v), rs = run << 4 | s;
        w.put(ac.code[rs], ac.len[rs]);
        put_value(w, v, s);
        k += run + 1;
    }
    if (k < 64) w.put(ac.code[0], ac.len[0]);
}

struct Place {
    int H, W, sub, layout;
    bool rows;                              // a restart marker per MCU row
    int dense;
};

struct Bank {
    std::vector<int> images, segments, htabs;
    uint8_t* data = nullptr;               // exactly nbytes
    long nbytes = 0;
    int n = 0, nseg = 0, seg_max = 0, block_stride = 0, Hmax = 0, Wmax = 0;
    std::vector<long> longest;             // per place
};

void build_bank(const std::vector<Place>& places, const Table& dc, const Table& ac, Bank& bank) {
    std::vector<uint8_t> all;
    bank.n = (int)places.size();
    bank.images.assign((size_t)bank.n * JB_IMAGE_INTS, 0);
    for (int i = 0; i < bank.n; ++i) {
        const Place& p = places[(size_t)i];
        int* im = &bank.images[(size_t)i * JB_IMAGE_INTS];
        const JeLayout lay = je_layout(p.layout, p.sub);
        im[JB_H] = p.H, im[JB_W] = p.W, im[JB_SUB] = p.sub, im[JB_LAYOUT] = p.layout;
        im[JB_MCUX] = (p.W + 8 * lay.h - 1) / (8 * lay.h), im[JB_MCUY] = (p.H + 8 * lay.v - 1) / (8 * lay.v);
        for (int k = 0; k < 6; ++k) im[JB_HUFF + k] = k & 1;      // slot 0: DC, slot 1: AC, for every component
        im[JB_NBLOCKS] = im[JB_MCUX] * im[JB_MCUY] * js_mcu_blocks(lay);
        im[JB_SEG0] = bank.nseg;
        bank.longest.push_back(0);
        if (p.dense < 0) continue;                                // an empty place: no segments
        const int mcus = im[JB_MCUX] * im[JB_MCUY], per = p.rows ? im[JB_MCUX] : mcus;
        for (int first = 0; first < mcus; first += per) {
            BitWriter w;
            for (int b = 0; b < per * js_mcu_blocks(lay); ++b) put_block(w, dc, ac, p.dense);
            w.flush();
            const long begin = (long)all.size();
            all.insert(all.end(), w.bytes.begin(), w.bytes.end());
            const int row[5] = {i, (int)begin, (int)all.size(), first, per};
            bank.segments.insert(bank.segments.end(), row, row + 5);
            if ((long)w.bytes.size() > bank.longest.back()) bank.longest.back() = (long)w.bytes.size();
            if (first + per < mcus) all.push_back(0xFF), all.push_back((uint8_t)(0xD0 + (first / per) % 8));
            ++im[JB_NSEG], ++bank.nseg;
        }
        bank.seg_max = im[JB_NSEG] > bank.seg_max ? im[JB_NSEG] : bank.seg_max;
        bank.block_stride = im[JB_NBLOCKS] > bank.block_stride ? im[JB_NBLOCKS] : bank.block_stride;
        bank.Hmax = p.H > bank.Hmax ? p.H : bank.Hmax, bank.Wmax = p.W > bank.Wmax ? p.W : bank.Wmax;
    }
    bank.block_stride = (bank.block_stride + ISTVT_JPEG_IDCT_BLOCKS - 1) / ISTVT_JPEG_IDCT_BLOCKS * ISTVT_JPEG_IDCT_BLOCKS;
    bank.nbytes = (long)all.size();
    bank.data = (uint8_t*)std::malloc(all.size());
    std::memcpy(bank.data, all.data(), all.size());
    bank.htabs.assign(dc.t, dc.t + JE_HUFF_INTS);
    bank.htabs.insert(bank.htabs.end(), ac.t, ac.t + JE_HUFF_INTS);
}

// JdWriter of jpeg.hip on a buffer of exactly `total` blocks
struct Writer {
    int16_t* coef;
    long block0, total;
    int ybw, cbw, ny, nc;
    bool* bad;
    long block(int c, int row, int col) const {
        const long b = block0 + (c == 0 ? (long)row * ybw + col : ny + (long)(c - 1) * nc + (long)row * cbw + col);
        return b >= 0 && b < total ? b : -1;
    }
    void clear(long b) const {
        if (b >= 0) std::memset(coef + b * 64, 0, 128);
    }
    void put(long b, int at, int v) const {
        if (at < 0 || at > 63) *bad = true;
        if (b >= 0) coef[b * 64 + at] = (int16_t)v;
    }
};

constexpr int SENTINEL = 0x5a5a5a5a;

// the row table of a call: exactly m * seg_max * R rows
struct Rows {
    int* rows;
    long nrows, R;
    void store(long s, long row, const int* v) {
        if (row < s * R || row >= (s + 1) * R) fail("a row store outside its segment's rows", s, row);
        if (row < 0 || row >= nrows) fail("a row store outside the table", s, row);
        std::memcpy(rows + row * ISTVT_JPEG_STATE_INTS, v, sizeof(int) * ISTVT_JPEG_STATE_INTS);   // for the sanitizer to see
    }
};

// Planned segment row s as a workgroup of jpeg_entropy_split_kernel<LANES, true> treats it -> its status word.  *wrote: the
// rows it stored, 0 where it was refused.
int split_segment(const Bank& bank, const int* images, int m, const int* segments, int s, int lanes, int chunk_bytes,
                  int16_t* coef, long total_blocks, Rows& table, int* wrote, bool* bad) {
    *wrote = 0;
    const int* sg = segments + (long)s * JB_SEGMENT_INTS;
    const int img = sg[0], first = sg[3], count = sg[4];
    const long begin = sg[1], end = sg[2];
    bool ok = img >= 0 && img < m && begin >= 0 && begin <= end && end <= bank.nbytes && first >= 0 && count >= 0;
    const int* im = images + (long)(ok ? img : 0) * JB_IMAGE_INTS;
    const JeLayout lay = je_layout(im[JB_LAYOUT], im[JB_SUB]);
    const int mcux = im[JB_MCUX] > 1 ? im[JB_MCUX] : 1, mcuy = im[JB_MCUY] > 1 ? im[JB_MCUY] : 1;
    ok = ok && (long)first + count <= (long)mcux * mcuy;
    const int* huff[6];
    for (int k = 0; k < 6; ++k) {
        const int slot = im[JB_HUFF + k];
        ok = ok && slot >= 0 && slot < 2;
        huff[k] = bank.htabs.data() + (long)(ok ? slot : 0) * JE_HUFF_INTS;
    }
    const long chunk = ok ? js_chunk_bytes(end - begin, chunk_bytes) : chunk_bytes;
    const int S = ok ? js_chunks(end - begin, chunk_bytes) : 1;
    const long row0 = js_row0<true>(begin, chunk_bytes, s, S, table.R);
    ok = ok && S <= lanes && row0 >= 0;
    if (!ok) return 2;
    const Writer w = {coef, (long)im[JB_BLOCK0], total_blocks, mcux * lay.h, mcux, mcux * lay.h * mcuy * lay.v, mcux * mcuy, bad};
    const long total = (long)count * js_mcu_blocks(lay);
    for (long cur = 0; cur < total; ++cur) {
        int c;
        w.clear(js_place(lay, mcux, first, cur, w, c));
    }
    std::vector<JsState> in((size_t)S), out((size_t)S), seen;
    std::vector<JsTally> t((size_t)S);
    for (int i = 0; i < S; ++i) {
        in[(size_t)i] = i ? js_guess(bank.data, begin, end, begin + (long)i * chunk) : JsState{begin, 0, 0, 0};
        out[(size_t)i] = in[(size_t)i];
        t[(size_t)i] = JsTally{0, 0, {0, 0, 0}};
        if (i < S - 1) out[(size_t)i] = js_chunk(bank.data, end, begin + (long)(i + 1) * chunk, huff, lay, in[(size_t)i], t[(size_t)i]);
    }
    int rounds = 0;
    for (int r = 1; r < S; ++r) {
        seen = out;
        bool changed = false;
        for (int i = 1; i < S; ++i) {
            if (js_same(seen[(size_t)i - 1], in[(size_t)i])) continue;
            in[(size_t)i] = seen[(size_t)i - 1];
            if (i < S - 1) {
                const JsState o = js_chunk(bank.data, end, begin + (long)(i + 1) * chunk, huff, lay, in[(size_t)i], t[(size_t)i]);
                changed = changed || !js_same(o, out[(size_t)i]);
                out[(size_t)i] = o;
            }
        }
        if (!changed) break;
        ++rounds;
    }
    int dead = JS_LANES;
    for (int i = S - 2; i >= 0; --i)
        if (t[(size_t)i].err) dead = i;
    long next = 0, sum = 0;
    int pred[3] = {0, 0, 0}, status = 0;
    for (int i = 0; i < S; ++i) {
        int started = 0, st = 0;
        if (i <= dead)
            st = js_write(bank.data, end, begin + (long)(i + 1) * chunk, i == S - 1, huff, lay, mcux, first, total, in[(size_t)i],
                          next, pred, w, started);
        status = st > status ? st : status;
        sum += started;
        const int row[ISTVT_JPEG_STATE_INTS] = {(int)in[(size_t)i].pos, in[(size_t)i].bit, in[(size_t)i].blk, in[(size_t)i].k, started,
                                                (int)(next < total ? next : total), st, rounds};
        table.store(s, row0 + i, row);
        if (i < S - 1) {
            next += t[(size_t)i].blocks;
            for (int c = 0; c < 3; ++c) pred[c] = (int16_t)(pred[c] + t[(size_t)i].pred[c]);
        }
    }
    if (status == 0 && sum != total) fail("the lanes of a sound segment did not start its blocks", s, sum);
    *wrote = S;
    return status;
}

void run(const Bank& bank, int seg_bytes_max, int over, int empty, int chunk_bytes) {
    int R = (seg_bytes_max + chunk_bytes - 1) / chunk_bytes;
    R = R < 1 ? 1 : R > JS_LANES ? JS_LANES : R;
    for (long L = 0; L <= seg_bytes_max; ++L)
        if (js_chunks(L, chunk_bytes) > R) fail("chunk_rows is no bound", L, js_chunks(L, chunk_bytes));
    if (js_row0<true>(0, chunk_bytes, 3, R + 1, R) != -1 || js_row0<true>(0, chunk_bytes, 3, R, R) != 3L * R)
        fail("js_row0", R, chunk_bytes);
    const int n = bank.n, seg_max = bank.seg_max, lanes = R <= 64 ? 64 : JS_LANES;
    const std::vector<int> index = {0, over, 3, 3, -1, 2, n, empty, 1, 0, -2147483647 - 1, 2147483647, over};
    const int m = (int)index.size();
    const long nseg = (long)m * seg_max, blocks = (long)m * bank.block_stride;
    int* images = (int*)std::malloc(sizeof(int) * (size_t)m * JB_IMAGE_INTS);
    int* segments = (int*)std::malloc(sizeof(int) * (size_t)nseg * JB_SEGMENT_INTS);
    int* rows = (int*)std::malloc(sizeof(int) * (size_t)nseg * R * ISTVT_JPEG_STATE_INTS);
    int16_t* got = (int16_t*)std::malloc(sizeof(int16_t) * (size_t)blocks * 64);
    int16_t* want = (int16_t*)std::malloc(sizeof(int16_t) * (size_t)blocks * 64);
    for (long i = 0; i < nseg * R * ISTVT_JPEG_STATE_INTS; ++i) rows[i] = SENTINEL;
    for (long i = 0; i < blocks * 64; ++i) got[i] = want[i] = 0x5a5a;
    std::vector<int> place((size_t)m);
    for (int j = 0; j < m; ++j) {
        const int idx = index[(size_t)j];
        const int st = jb_plan_status(bank.images.data(), n, bank.segments.data(), bank.nseg, idx, seg_max, bank.block_stride,
                                      bank.Hmax, bank.Wmax, seg_bytes_max);
        const int expect = idx < 0 || idx >= n ? JB_STATUS_INDEX : idx == over || idx == empty ? JB_STATUS_EMPTY : 0;
        if (st != expect) fail("plan status", j, st);
        if (idx == over && jb_plan_status(bank.images.data(), n, bank.segments.data(), bank.nseg, idx, seg_max, bank.block_stride,
                                          bank.Hmax, bank.Wmax, -1) != 0)
            fail("the long file is not decodable without a limit", j, idx);
        place[(size_t)j] = st;
        jb_plan_image(bank.images.data(), idx, st, j, m, seg_max, bank.block_stride, images + (long)j * JB_IMAGE_INTS);
        for (int k = 0; k < seg_max; ++k)
            jb_plan_segment(bank.images.data(), bank.segments.data(), idx, st, j, k, segments + ((long)j * seg_max + k) * JB_SEGMENT_INTS);
    }
    Rows table = {rows, nseg * R, R};
    bool bad = false;
    long stored = 0, decoded = 0;
    for (int s = 0; s < (int)nseg; ++s) {
        const int j = s / seg_max, k = s - j * seg_max;
        const int* im = images + (long)j * JB_IMAGE_INTS;
        const bool real = place[(size_t)j] == 0 && k < im[JB_NSEG];
        int wrote = 0;
        const int st = split_segment(bank, images, m, segments, s, lanes, chunk_bytes, got, blocks, table, &wrote, &bad);
        if (!real) {
            if (st != 2 || wrote != 0) fail("a padded segment row, or one of a place without a file, was decoded", s, st);
        } else {
            const int* sg = segments + (long)s * JB_SEGMENT_INTS;
            const JeLayout lay = je_layout(im[JB_LAYOUT], im[JB_SUB]);
            const int mcux = im[JB_MCUX], mcuy = im[JB_MCUY];
            const int* huff[6];
            for (int q = 0; q < 6; ++q) huff[q] = bank.htabs.data() + (long)im[JB_HUFF + q] * JE_HUFF_INTS;
            Writer w = {want, (long)im[JB_BLOCK0], blocks, mcux * lay.h, mcux, mcux * lay.h * mcuy * lay.v, mcux * mcuy, &bad};
            const int ref = je_decode_segment(bank.data, (long)sg[1], (long)sg[2], huff, lay, mcux, sg[3], sg[4], w);
            if (st != ref || ref != 0) fail("status", s, st);     // the files made here are sound
            if (wrote != js_chunks((long)sg[2] - sg[1], chunk_bytes)) fail("rows stored", s, wrote);
            ++decoded;
        }
        for (long r = (long)s * R + wrote; r < (long)(s + 1) * R; ++r)      // behind the chunks: untouched
            for (int f = 0; f < ISTVT_JPEG_STATE_INTS; ++f)
                if (rows[r * ISTVT_JPEG_STATE_INTS + f] != SENTINEL) fail("a row behind a segment's chunks was written", s, r);
        for (long r = (long)s * R; r < (long)s * R + wrote; ++r)
            if (rows[r * ISTVT_JPEG_STATE_INTS + 7] == SENTINEL) fail("a row of a chunk was not written", s, r);
        stored += wrote;
    }
    if (bad) fail("a coefficient outside 0..63", 0, 0);
    if (std::memcmp(got, want, sizeof(int16_t) * (size_t)blocks * 64) != 0) fail("coefficients", chunk_bytes, 0);
    std::printf("chunk %d: %d rows per segment, %d lanes, %d places, %ld segments decoded, %ld rows stored of %ld\n", chunk_bytes, R,
                lanes, m, decoded, stored, nseg * R);
    std::free(images), std::free(segments), std::free(rows), std::free(got), std::free(want);
}

}  // namespace

int main() {
    Table dc, ac;
    // T.81 K.3, luminance DC: categories 0..11
    make_table({0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11}, dc);
    // AC: end of block at 2 bits, three short codes, then ZRL and every (run 0..15, size 1..4) at 8 bits: a code that leaves
    // prefixes no symbol has, which a lane that starts from a wrong state must survive
    std::vector<int> counts(16, 0), values = {0x00, 0x01, 0x02, 0x11, 0xF0};
    for (int run = 0; run < 16; ++run)
        for (int size = 1; size <= 4; ++size)
            if ((run << 4 | size) != 0x01 && (run << 4 | size) != 0x02 && (run << 4 | size) != 0x11) values.push_back(run << 4 | size);
    counts[1] = 1, counts[3] = 3, counts[7] = (int)values.size() - 4;
    make_table(counts, values, ac);
    const int empty = 4, over = 5;
    const std::vector<Place> places = {{96, 80, 2, 0, false, 30},
                                       {24, 40, 1, 0, true, 12},
                                       {16, 48, 2, ISTVT_JPEG_LAYOUT_422, false, 8},
                                       {40, 24, 1, ISTVT_JPEG_LAYOUT_GREY, true, 20},
                                       {16, 16, 2, 0, false, -1},
                                       {96, 96, 1, 0, false, 30}};
    Bank bank;
    build_bank(places, dc, ac, bank);
    long seg_bytes_max = 0;
    for (int i = 0; i < bank.n; ++i)
        if (i != over && bank.longest[(size_t)i] > seg_bytes_max) seg_bytes_max = bank.longest[(size_t)i];
    if (bank.longest[(size_t)over] <= seg_bytes_max) fail("the long file is not the longest", bank.longest[(size_t)over], seg_bytes_max);
    if (seg_bytes_max <= 16 * JS_LANES) fail("no segment long enough for the lane cap at chunk 16", seg_bytes_max, 16 * JS_LANES);
    std::printf("bank: %d places, %d segments, %ld bytes, seg_max %d, longest segment %ld, over-long %ld\n", bank.n, bank.nseg,
                bank.nbytes, bank.seg_max, seg_bytes_max, bank.longest[(size_t)over]);
    for (int chunk_bytes : {16, 37, 128}) run(bank, (int)seg_bytes_max, over, empty, chunk_bytes);
    std::free(bank.data);
    if (failures) {
        std::printf("%d failures\n", failures);
        return 1;
    }
    std::printf("ok\n");
    return 0;
}
