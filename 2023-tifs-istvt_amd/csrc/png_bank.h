// The lookup arithmetic of the PNG bank (DESIGN.md "PNG bank"): which place and band a wave is, whether the bank's row of
// the drawn file and the band's row fit the call, and the file's 64-bit base.  __host__ __device__: the kernels of
// csrc/png_bank.hip call these functions and nothing else decides; tools/png_bank_check.cpp runs the same code on the host
// under sanitizers, in blocks of exactly the tables' size.  clips.png_bank writes the rows, clips.png_bank_decode_host reads
// them as these functions do.
//
// A row of the bank's images (PK_IMAGE_INTS ints): H, W, colour type, bpp, base low word, base high word, stream bytes, first
// band row, band count, 0.  The base is a byte offset into the bank's data, 64 bits wide and a multiple of 16; everything
// inside a file is a 32-bit offset from it.  A row of the bank's bands (PK_BAND_INTS ints, clips.png_band_table's): file,
// begin, end, first output byte, output bytes, begin and end counted from the file's base.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define PK_HD __host__ __device__ __forceinline__
#else
#define PK_HD inline
#endif

#define PK_IMAGE_INTS 10
#define PK_BAND_INTS 5
#define PK_MAX_SIDE 16384
#define PK_OUTSIDE 8                       // index[j] is outside [0, n)
#define PK_ROW 9                           // the bank's row for the place, or one of its band rows, does not fit the call

enum { PK_H = 0, PK_W = 1, PK_TYPE = 2, PK_BPP = 3, PK_BASE_LO = 4, PK_BASE_HI = 5, PK_BYTES = 6, PK_FIRST_BAND = 7, PK_BANDS = 8,
       PK_FLAGS = 9 };                      // read by csrc/png_alone.hip only: bit 0, the file's bands stand alone
enum { PKB_FILE = 0, PKB_BEGIN = 1, PKB_END = 2, PKB_OUT = 3, PKB_OUT_BYTES = 4 };

// what the checks of a call compare the rows with: the call's scalars, the same for every wave
struct PkCall {
    long nbytes;                           // of the bank's data; may exceed 2^31
    int n, nseg, band_max, raw_stride, Hc, Wc;
};

// wave b of the inflate launch is band k of place j
PK_HD void pk_wave(int b, int band_max, int* j, int* k) {
    *j = b / band_max;
    *k = b % band_max;
}

PK_HD bool pk_inside(int i, int n) { return i >= 0 && i < n; }

PK_HD int64_t pk_base(const int* im) {
    return (int64_t)(((uint64_t)(uint32_t)im[PK_BASE_HI] << 32) | (uint64_t)(uint32_t)im[PK_BASE_LO]);
}

// the filtered bytes of a file whose sides and bpp pk_image_ok has bounded: at most 16384 (1 + 4 * 16384)
PK_HD long pk_raw_bytes(const int* im) { return (long)im[PK_H] * (1 + (long)im[PK_W] * im[PK_BPP]); }

// The image row of the drawn file against the call: sides of 1..16384 inside the canvas, a colour type with its bpp, filtered
// rows that fit a row of the scratch, a band count of 1..band_max, and a stream [base, base + bytes) inside the data at a
// multiple of 16.  Reads im[0 .. PK_IMAGE_INTS) only.
PK_HD bool pk_image_ok(const int* im, const PkCall& c) {
    const int H = im[PK_H], W = im[PK_W], ct = im[PK_TYPE], bpp = im[PK_BPP];
    if (H < 1 || W < 1 || H > PK_MAX_SIDE || W > PK_MAX_SIDE || H > c.Hc || W > c.Wc) return false;
    if (!((ct == 0 && bpp == 1) || (ct == 2 && bpp == 3) || (ct == 6 && bpp == 4))) return false;
    if (pk_raw_bytes(im) > (long)c.raw_stride) return false;
    if (im[PK_BANDS] < 1 || im[PK_BANDS] > c.band_max) return false;
    const int64_t base = pk_base(im);
    if (base < 0 || (base & 15) || im[PK_BYTES] < 0) return false;
    return base <= (int64_t)c.nbytes && (int64_t)im[PK_BYTES] <= (int64_t)c.nbytes - base;
}

// Band k of file i, whose image row `im` has passed pk_image_ok: where its row of the band table is, or -1 where no such row
// is inside the table.  Nothing of the table is read.
PK_HD long pk_band_row(const int* im, int k, int nseg) {
    const long row = (long)im[PK_FIRST_BAND] + k;
    return (im[PK_FIRST_BAND] < 0 || row >= (long)nseg) ? -1 : row;
}

// The band row `row` (PK_BAND_INTS ints) of file i against its image row: it names the file, lies inside the file's stream
// and writes inside the file's filtered rows.
PK_HD bool pk_band_ok(const int* row, const int* im, int i) {
    if (row[PKB_FILE] != i) return false;
    if (row[PKB_BEGIN] < 0 || row[PKB_BEGIN] > row[PKB_END] || row[PKB_END] > im[PK_BYTES]) return false;
    if (row[PKB_OUT] < 0 || row[PKB_OUT_BYTES] < 0) return false;
    return (long)row[PKB_OUT] + row[PKB_OUT_BYTES] <= pk_raw_bytes(im);
}

// What a wave of the inflate launch does, decided from the tables alone.  PK_SKIP: it leaves and writes nothing (the index is
// outside the bank, the image row fails, or the file has no band k); PK_REFUSE: its band status is PK_ROW and it writes
// nothing else; PK_RUN: it inflates *row.
enum { PK_SKIP = 0, PK_REFUSE = 1, PK_RUN = 2 };

PK_HD int pk_band_plan(const int* images, const int* bands, const PkCall& c, int i, int k, const int** im_out, const int** row_out) {
    if (!pk_inside(i, c.n)) return PK_SKIP;
    const int* im = images + (long)i * PK_IMAGE_INTS;
    if (!pk_image_ok(im, c) || k >= im[PK_BANDS]) return PK_SKIP;
    *im_out = im;
    const long at = pk_band_row(im, k, c.nseg);
    if (at < 0) return PK_REFUSE;
    const int* row = bands + at * PK_BAND_INTS;
    if (!pk_band_ok(row, im, i)) return PK_REFUSE;
    *row_out = row;
    return PK_RUN;
}

// The status the unfilter launch starts from for place j: PK_OUTSIDE, PK_ROW, or 0 with *im_out the file's row
PK_HD int pk_place_plan(const int* images, const PkCall& c, int i, const int** im_out) {
    if (!pk_inside(i, c.n)) return PK_OUTSIDE;
    const int* im = images + (long)i * PK_IMAGE_INTS;
    if (!pk_image_ok(im, c)) return PK_ROW;
    *im_out = im;
    return 0;
}

// the scalars of a call, checked once on the host before any launch: counts, alignment, m * band_max as an int, the scratch
PK_HD bool pk_scalars_ok(const PkCall& c, int m, long scratch_bytes) {
    if (c.n < 1 || c.nseg < 1 || c.nbytes < 0 || m < 1 || c.band_max < 1) return false;
    if (c.raw_stride < 16 || (c.raw_stride & 15)) return false;
    if (c.Hc < 1 || c.Wc < 1 || c.Hc > PK_MAX_SIDE || c.Wc > PK_MAX_SIDE) return false;
    if ((long)m * c.band_max > 0x7fffffffL) return false;
    return scratch_bytes >= (long)m * c.raw_stride + 4L * m * c.band_max;
}
