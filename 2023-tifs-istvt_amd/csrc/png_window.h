// The arithmetic of the windowed PNG decode (DESIGN.md "PNG windows"): the window of rows a box needs of a file whose bands
// stand alone, the status of a place by its precedence, which band wave t of a place takes and where that band's filtered bytes
// go in the place's window of the scratch.  __host__ __device__: the kernels of csrc/png_window.hip call these functions and
// nothing else decides; tools/png_window_check.cpp runs the same code on the host under sanitizers, in blocks of exactly the
// tables' size.  clips.png_window_plan and clips._png_window_place are the same steps in Python.
#pragma once
#include <stdint.h>

#include "png_alone.h"
#include "png_bank.h"

#if defined(__HIPCC__)
#define PW_HD __host__ __device__ __forceinline__
#else
#define PW_HD inline
#endif

#define PW_WHOLE 11                        // the file's index does not say its bands stand alone: it is decoded whole, not by a box
#define PW_BOX 12                          // the box does not lie in the image, or its bands do not fit the window
#define PW_BOX_INTS 4                      // y0, x0, h, w

// the scalars of a call: the bank's (k.Hc is the window height `rows`, k.Wc the canvas width), the slots and the bytes of a
// place, and whether `images` are a bank's rows read through an index or a batch's, place j being file j
struct PwCall {
    PkCall k;
    int win_bands, win_stride, bank;
};

struct PwWindow {
    int kfirst, klast, w0, w1;             // the bands [kfirst, klast] and the rows [w0, w1) of the image
};

// wave b of either launch is slot t of place j
PW_HD void pw_wave(int b, int win_bands, int* j, int* t) {
    *j = b / win_bands;
    *t = b % win_bands;
}

// The window of box (y0, x0, h, w) in a file of H x W in `count` bands of R >= 1 rows -> 0, or PW_BOX where the box does not
// lie in the image, the window has more than `rows` rows or more than win_bands bands
PW_HD int pw_window(int H, int W, int R, int count, const int* box, int rows, int win_bands, PwWindow* w) {
    const long y0 = box[0], x0 = box[1], h = box[2], bw = box[3];
    if (h < 1 || bw < 1 || y0 < 0 || x0 < 0 || y0 + h > H || x0 + bw > W) return PW_BOX;
    const long kfirst = y0 / R, klast = (y0 + h - 1) / R;
    const long w0 = kfirst * R, w1 = (klast + 1) * R < H ? (klast + 1) * R : H;
    if (klast >= count || w1 - w0 > rows || klast - kfirst + 1 > win_bands) return PW_BOX;
    w->kfirst = (int)kfirst, w->klast = (int)klast, w->w0 = (int)w0, w->w1 = (int)w1;
    return 0;
}

// File i as a row of a bank, whichever table it stands in.  A batch's row (H, W, colour type, bpp, begin, end, first band row,
// band count) becomes the bank row of a file at base 0 whose stream is all of the call's bytes -- its band rows count from
// there -- with the flag set: the host has seen every flag of a batch.
PW_HD void pw_row(const int* images, const PwCall& c, int i, int* im) {
    if (c.bank) {
        for (int q = 0; q < PK_IMAGE_INTS; ++q) im[q] = images[(long)i * PK_IMAGE_INTS + q];
        return;
    }
    const int* row = images + (long)i * 8;
    im[PK_H] = row[0], im[PK_W] = row[1], im[PK_TYPE] = row[2], im[PK_BPP] = row[3];
    im[PK_BASE_LO] = 0, im[PK_BASE_HI] = 0, im[PK_BYTES] = (int)c.k.nbytes;
    im[PK_FIRST_BAND] = row[6], im[PK_BANDS] = row[7], im[PK_FLAGS] = 1;
}

// What the tables say of place j's file i before its box is looked at: PK_OUTSIDE, PK_ROW (the image row does not fit the
// call, min(H, rows) of its filtered rows do not fit win_stride, its band rows are not inside the table or give no R), PW_WHOLE
// (no flag), or 0 with im[PK_IMAGE_INTS] the file's row, *rows its first band row and *R its band height.  The image row is
// checked as pk_image_ok checks it, but for the height: W against the canvas width, H against 16384 alone.
PW_HD int pw_file(const int* images, const int* bands, const PwCall& c, int i, int* im, const int** rows, int* R) {
    if (!pk_inside(i, c.k.n)) return PK_OUTSIDE;
    pw_row(images, c, i, im);
    PkCall wide = c.k;
    wide.Hc = PK_MAX_SIDE;
    if (!pk_image_ok(im, wide)) return PK_ROW;
    const long stride = 1 + (long)im[PK_W] * im[PK_BPP];
    if ((long)(im[PK_H] < c.k.Hc ? im[PK_H] : c.k.Hc) * stride > (long)c.win_stride) return PK_ROW;
    if (!(im[PK_FLAGS] & 1)) return PW_WHOLE;
    const long at = pk_band_row(im, 0, c.k.nseg);
    if (at < 0 || pk_band_row(im, im[PK_BANDS] - 1, c.k.nseg) < 0) return PK_ROW;
    *rows = bands + at * PK_BAND_INTS;
    *R = pa_alone_rows((*rows)[PKB_OUT_BYTES], stride);
    return *R < 1 ? PK_ROW : 0;
}

// ... and behind pw_file's 0, with `fit` what the lanes found together (pa_rows_fit over all band rows of the file): PK_ROW,
// PW_BOX, or 0 with the window
PW_HD int pw_place(bool fit, const int* im, int R, const int* box, const PwCall& c, PwWindow* w) {
    if (!fit) return PK_ROW;
    return pw_window(im[PK_H], im[PK_W], R, im[PK_BANDS], box, c.k.Hc, c.win_bands, w);
}

// the band slot t of a place takes, or -1 where the window has no such band: the wave leaves
PW_HD int pw_band(const PwWindow& w, int t) { return t <= w.klast - w.kfirst ? w.kfirst + t : -1; }

// Where the bytes of band row `row` go in the place's win_stride bytes of scratch, or -1 where they would not lie inside them.
// With pa_rows_fit true and the band one of the window's this is (k R - w0) stride, and the band ends at most (w1 - w0) stride
// <= min(H, rows) stride <= win_stride bytes in: never -1.
PW_HD long pw_band_at(const int* row, const PwWindow& w, long stride, int win_stride) {
    const long at = (long)row[PKB_OUT] - (long)w.w0 * stride;
    return (at < 0 || row[PKB_OUT_BYTES] < 0 || at + row[PKB_OUT_BYTES] > (long)win_stride) ? -1 : at;
}

// the marks (pa_row_mark) of rows begin, begin + step, ... of the window [w0, w1), or-ed; win: the window's filtered rows, row
// w0 first.  Row w0 counts as a band's first row where w0 >= 1: it is one.
PW_HD int pw_marks(const uint8_t* win, long stride, const PwWindow& w, int R, int begin, int step) {
    int marks = 0;
    for (int r = w.w0 + begin; r < w.w1; r += step) marks |= pa_row_mark(r, win[(long)(r - w.w0) * stride], R);
    return marks;
}

// a place with this status reports its file's H x W, else 0 x 0
PW_HD bool pw_sized(int status) { return status != PK_OUTSIDE && status != PK_ROW; }

// the scratch of m places: the windows' filtered rows, a status word per slot, then from the next multiple of 16 the moved boxes
// int32 [m][4] and the origins int32 [m]
PW_HD long pw_boxes_at(long m, int win_bands, int win_stride) { return (m * win_stride + 4 * m * win_bands + 15) / 16 * 16; }
PW_HD long pw_scratch_bytes(long m, int win_bands, int win_stride) { return pw_boxes_at(m, win_bands, win_stride) + 4 * m * (PW_BOX_INTS + 1); }
