// The arithmetic of the JPEG bank (csrc/jpeg_bank_scan.h, DESIGN.md "JPEG bank") on the host, under sanitizers:
//
//     clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//         -I include -I 2023-tifs-istvt_amd/csrc tools/jpeg_bank_check.cpp -o jpeg_bank_check
//     ./jpeg_bank_check
//
// (1) The marker scan.  jpeg_bank_scan_kernel is emulated with its lanes in order -- tiles of 256 x 16 bytes from the scan's
// first byte, jb_markers per lane, the prefix of the counts, marker r ends interval r and starts interval r + 1 -- on
// synthetic scans, and compared with a byte-by-byte walk.  The scans: filler bytes with one FF Dn pair at every position
// 0..40 and 4080..4112 and 8176..8208 of the scan (so at every offset relative to a 16-byte lane boundary and across the
// 4096-byte tile boundaries), the same with two and three pairs, with the pairs back to back, with a stuffed FF 00 at the
// same positions (which is no marker), and scans of every length 0..40 and 4090..4100 that end in FF D9 right behind their
// last byte, with a pair as their last two bytes or an FF as their last byte.  Every scan sits in a buffer that ends with
// its EOI, at an odd distance from the buffer's start, so AddressSanitizer sees a read past `end + 1` or in front of `begin`.
// (2) The plan.  jb_plan_status, jb_plan_image and jb_plan_segment, the whole of jpeg_bank_plan_kernel's arithmetic, run
// on a small bank in all four layouts with an empty row, for indices inside, outside (-1, n, INT_MIN, INT_MAX) and
// repeated, into tables of the exact size.  Required: images of the uniform strides whose blocks fit their stride; first
// workgroups that ascend, as the IDCT kernel's binary search needs; segment rows that name their place, or are rejected by
// jpeg_entropy_kernel's own comparison; the status words an image folds are those of its real segments alone, or its one
// place word, inside the table.  Prints one line per part and `ok`; exit status 1 on any failure.  A hand tool for a CPU:
// nothing here touches a GPU.
#include <climits>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "jpeg_bank_scan.h"

namespace {

int failures = 0;

void fail(const char* what, long a, long b) {
    if (++failures <= 20) std::printf("FAILED %s (%ld, %ld)\n", what, a, b);
}

struct Interval {
    long begin, end;
};

// clips.jpeg_scan_segments_host
std::vector<Interval> walk(const uint8_t* d, long begin, long end) {
    std::vector<Interval> out;
    long first = begin, at = begin;
    while (at + 1 < end) {
        if (d[at] == 0xFF && d[at + 1] >= 0xD0 && d[at + 1] <= 0xD7) {
            out.push_back({first, at});
            first = at = at + 2;
        } else {
            ++at;
        }
    }
    out.push_back({first, end});
    return out;
}

// jpeg_bank_scan_kernel's loop for one readable file, lanes in order; rows: [seg_max] exactly.  -> markers found
int scan(const uint8_t* d, long begin, long end, std::vector<Interval>& rows) {
    const int seg_max = (int)rows.size();
    rows[0].begin = begin, rows[seg_max - 1].end = end;
    int found = 0;
    for (long tile = begin; tile < end; tile += JB_TILE_BYTES) {
        int counts[256], total = 0;
        uint32_t masks[256];
        for (int tid = 0; tid < 256; ++tid) {
            const long lo = tile + (long)tid * JB_LANE_BYTES, hi = lo + JB_LANE_BYTES < end ? lo + JB_LANE_BYTES : end;
            masks[tid] = jb_markers(d, lo, hi, end);
            counts[tid] = total;                                  // the exclusive prefix
            total += __builtin_popcount(masks[tid]);
        }
        for (int tid = 0; tid < 256; ++tid) {
            const long lo = tile + (long)tid * JB_LANE_BYTES;
            int r = found + counts[tid];
            for (uint32_t mask = masks[tid]; mask; mask &= mask - 1, ++r) {
                const long p = lo + __builtin_ctz(mask);
                if (r < seg_max - 1) rows[r].end = p, rows[r + 1].begin = p + 2;
            }
        }
        found += total;
    }
    return found;
}

long scans_run = 0;

// a scan of `body` behind `lead` bytes of header, EOI behind it, in a buffer of exactly that size
void check_scan(const std::vector<uint8_t>& body, long lead) {
    std::vector<uint8_t> buf((size_t)lead, 0xFF);                // FF D0 in front of the scan must not be found
    if (lead >= 2) buf[(size_t)lead - 1] = 0xD0;
    buf.insert(buf.end(), body.begin(), body.end());
    buf.push_back(0xFF), buf.push_back(0xD9);
    uint8_t* exact = (uint8_t*)std::malloc(buf.size());          // the vector's capacity may exceed its size
    std::memcpy(exact, buf.data(), buf.size());
    const long begin = lead, end = lead + (long)body.size();
    const std::vector<Interval> want = walk(exact, begin, end);
    for (int extra = -1; extra <= 1; ++extra) {                  // the expected count, one less, one more
        const int seg_max = (int)want.size() + extra;
        if (seg_max < 1) continue;
        std::vector<Interval> rows((size_t)seg_max, Interval{-7, -7});
        const int found = scan(exact, begin, end, rows);
        if (found != (int)want.size() - 1) fail("marker count", found, (long)want.size() - 1);
        if (extra == 0)
            for (size_t k = 0; k < want.size(); ++k)
                if (rows[k].begin != want[k].begin || rows[k].end != want[k].end) fail("interval", (long)k, rows[k].begin);
    }
    std::free(exact);
    ++scans_run;
}

void filler(std::vector<uint8_t>& body) {
    for (size_t i = 0; i < body.size(); ++i) body[i] = (uint8_t)(1 + (i * 37) % 200);   // no FF, no 00
}

void part_scan() {
    std::vector<long> places;
    for (long p = 0; p <= 40; ++p) places.push_back(p);
    for (long p = 4080; p <= 4112; ++p) places.push_back(p);
    for (long p = 8176; p <= 8208; ++p) places.push_back(p);
    const long length = 8300;
    for (long lead : {0L, 1L, 623L}) {
        for (long p : places) {
            for (int second = 0; second < 2; ++second) {
                for (int pairs = 1; pairs <= 3; ++pairs) {
                    std::vector<uint8_t> body((size_t)length);
                    filler(body);
                    for (int q = 0; q < pairs; ++q) {           // back to back, or 16 and 4096 bytes apart
                        const long at = p + (pairs == 2 ? 2 * q : q == 1 ? 16 : q == 2 ? 4096 : 0);
                        if (at + 1 < length) body[(size_t)at] = 0xFF, body[(size_t)at + 1] = second ? 0x00 : (uint8_t)(0xD0 + (q & 7));
                    }
                    check_scan(body, lead);
                }
            }
        }
        for (long n = 0; n <= 4100; n = n == 40 ? 4090 : n + 1) {
            for (int tail = 0; tail < 3; ++tail) {               // plain | a pair as the last two bytes | FF as the last byte
                std::vector<uint8_t> body((size_t)n);
                filler(body);
                if (tail == 1 && n >= 2) body[(size_t)n - 2] = 0xFF, body[(size_t)n - 1] = 0xD3;
                if (tail == 2 && n >= 1) body[(size_t)n - 1] = 0xFF;   // FF FF D9: the pair FF D9 is no RSTn, and [n, n + 1] is EOI
                check_scan(body, lead);
            }
        }
    }
    std::printf("scan: %ld scans\n", scans_run);
}

// an images row as clips.jpeg_batch packs it: geometry, slots, packed firsts
void bank_row(int* row, int H, int W, int sub, int layout, int seg0, int nseg) {
    const JeLayout lay = je_layout(layout, sub);
    std::memset(row, 0, sizeof(int) * JB_IMAGE_INTS);
    row[JB_H] = H, row[JB_W] = W, row[JB_SUB] = sub, row[JB_LAYOUT] = layout;
    row[JB_MCUX] = (W + 8 * lay.h - 1) / (8 * lay.h), row[JB_MCUY] = (H + 8 * lay.v - 1) / (8 * lay.v);
    row[JB_NBLOCKS] = row[JB_MCUX] * row[JB_MCUY] * (lay.h * lay.v + lay.nc);
    row[JB_SEG0] = seg0, row[JB_NSEG] = nseg;
}

void part_plan() {
    // 420 with a marker per MCU row, 444 without markers, 422 per MCU, grey, an empty row, a row too large for the strides
    const int n = 6;
    std::vector<int> images((size_t)n * JB_IMAGE_INTS);
    bank_row(&images[0 * JB_IMAGE_INTS], 33, 64, 2, 0, 0, 3);
    bank_row(&images[1 * JB_IMAGE_INTS], 17, 23, 1, 0, 3, 1);
    bank_row(&images[2 * JB_IMAGE_INTS], 8, 40, 2, ISTVT_JPEG_LAYOUT_422, 4, 3);
    bank_row(&images[3 * JB_IMAGE_INTS], 40, 24, 1, ISTVT_JPEG_LAYOUT_GREY, 7, 5);
    bank_row(&images[4 * JB_IMAGE_INTS], 16, 16, 2, 0, 12, 0);
    bank_row(&images[5 * JB_IMAGE_INTS], 640, 640, 1, 0, 12, 2);
    const int bank_nseg = 14, seg_max = 5;
    int most = 0;
    for (int i = 0; i < 4; ++i) most = images[(size_t)i * JB_IMAGE_INTS + JB_NBLOCKS] > most ? images[(size_t)i * JB_IMAGE_INTS + JB_NBLOCKS] : most;
    const int block_stride = (most + ISTVT_JPEG_IDCT_BLOCKS - 1) / ISTVT_JPEG_IDCT_BLOCKS * ISTVT_JPEG_IDCT_BLOCKS;
    std::vector<int> segments((size_t)bank_nseg * JB_SEGMENT_INTS);
    for (int s = 0; s < bank_nseg; ++s) {
        int* row = &segments[(size_t)s * JB_SEGMENT_INTS];
        row[0] = 99, row[1] = 100 * s, row[2] = 100 * s + 60, row[3] = s, row[4] = 1;
    }
    const std::vector<int> index = {0, 3, -1, 2, 2, n, 4, 1, INT_MIN, INT_MAX, 5, 0};
    const int m = (int)index.size(), Hc = 40, Wc = 64;
    const long words = (long)m * seg_max + m;
    int* out_images = (int*)std::malloc(sizeof(int) * (size_t)m * JB_IMAGE_INTS);
    int* out_segments = (int*)std::malloc(sizeof(int) * (size_t)m * seg_max * JB_SEGMENT_INTS);
    const int want_status[] = {0, 0, 4, 0, 0, 4, 5, 0, 4, 4, 5, 0};
    for (int j = 0; j < m; ++j) {
        const int st = jb_plan_status(images.data(), n, bank_nseg, index[(size_t)j], seg_max, block_stride, Hc, Wc);
        if (st != want_status[j]) fail("plan status", j, st);
        jb_plan_image(images.data(), index[(size_t)j], st, j, m, seg_max, block_stride, out_images + (long)j * JB_IMAGE_INTS);
        for (int k = 0; k < seg_max; ++k)
            jb_plan_segment(images.data(), segments.data(), index[(size_t)j], st, j, k,
                            out_segments + ((long)j * seg_max + k) * JB_SEGMENT_INTS);
    }
    for (int j = 0; j < m; ++j) {
        const int* im = out_images + (long)j * JB_IMAGE_INTS;
        const JeLayout lay = je_layout(im[JB_LAYOUT], im[JB_SUB]);
        const long nb = (long)im[JB_MCUX] * im[JB_MCUY] * (lay.h * lay.v + lay.nc);
        if (im[JB_BLOCK0] != j * block_stride || im[JB_GROUP0] != j * (block_stride / ISTVT_JPEG_IDCT_BLOCKS)) fail("strides", j, im[JB_BLOCK0]);
        if (nb > block_stride) fail("blocks past the stride", j, nb);
        if (j > 0 && im[JB_GROUP0] <= im[JB_GROUP0 - JB_IMAGE_INTS]) fail("first workgroups do not ascend", j, im[JB_GROUP0]);
        if (im[JB_SEG0] < 0 || (long)im[JB_SEG0] + im[JB_NSEG] > words) fail("status words outside the table", j, im[JB_SEG0]);
        if (want_status[j] == 0) {
            const int* b = &images[(size_t)index[(size_t)j] * JB_IMAGE_INTS];
            if (im[JB_SEG0] != j * seg_max || im[JB_NSEG] != b[JB_NSEG] || im[JB_H] != b[JB_H] || im[JB_W] != b[JB_W]) fail("image", j, im[JB_SEG0]);
        } else if (im[JB_SEG0] != (long)m * seg_max + j || im[JB_NSEG] != 1 || nb != 0 || im[JB_H] != 0 || im[JB_W] != 0) {
            fail("a place without a file", j, im[JB_SEG0]);
        }
        for (int k = 0; k < seg_max; ++k) {
            const int* sg = out_segments + ((long)j * seg_max + k) * JB_SEGMENT_INTS;
            const bool real = want_status[j] == 0 && k < im[JB_NSEG];
            const bool taken = sg[0] >= 0 && sg[0] < m;          // the first comparison of jpeg_entropy_kernel
            if (real != taken) fail("a padded row is decoded, or a real one is not", j, k);
            if (real) {
                const int* src = &segments[((size_t)images[(size_t)index[(size_t)j] * JB_IMAGE_INTS + JB_SEG0] + (size_t)k) * JB_SEGMENT_INTS];
                if (sg[0] != j || std::memcmp(sg + 1, src + 1, 4 * sizeof(int)) != 0) fail("segment row", j, k);
            }
        }
    }
    std::free(out_images);
    std::free(out_segments);
    std::printf("plan: %d places\n", m);
}

}  // namespace

int main() {
    part_scan();
    part_plan();
    if (failures) {
        std::printf("%d failures\n", failures);
        return 1;
    }
    std::printf("ok\n");
    return 0;
}
