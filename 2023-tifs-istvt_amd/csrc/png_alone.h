// The arithmetic of PNG bands that stand alone (DESIGN.md "PNG bands that stand alone"): which rows a wave takes, whether the
// band rows of a file that carries the flag are the R-row bands of an index, and the status the filter bytes give.
// __host__ __device__: the kernels of csrc/png_alone.hip call these functions and nothing else decides;
// tools/png_alone_check.cpp runs the same code on the host under sanitizers, in blocks of exactly the tables' size.
// clips._png_alone_band_rows and clips._png_alone_rows are the same steps in Python.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define PA_HD __host__ __device__ __forceinline__
#else
#define PA_HD inline
#endif

#define PA_BAND_INTS 5
#define PA_FILTER 6                        // a filter byte above 4
#define PA_LIES 10                         // the index says its bands stand alone, and a band's first row reads the row above

enum { PAB_OUT = 3, PAB_OUT_BYTES = 4 };

// R of a file from its band row 0: out_bytes / stride where that is a whole number of at least 1, else 0
PA_HD int pa_alone_rows(int out_bytes0, long stride) {
    if (stride < 2 || (long)out_bytes0 < stride || (long)out_bytes0 % stride) return 0;
    return (int)((long)out_bytes0 / stride);
}

// the bands of H rows in bands of R >= 1
PA_HD int pa_band_count(int H, int R) { return (H + R - 1) / R; }

// the rows [r0, r1) of band k of a file of H rows in bands of R: empty where k is not one of its bands
PA_HD void pa_band_span(int H, int R, int k, int* r0, int* r1) {
    const long a = (long)k * R, b = a + R;
    *r0 = (int)(a < H ? a : H);
    *r1 = (int)(b < H ? b : H);
}

// Band row `row` (PA_BAND_INTS ints), the k-th of `count` of a file of H rows of `stride` bytes in bands of R >= 1: it writes
// the rows of band k and nothing else, and the file has as many bands as H and R give.  With this true for every k in
// [0, count) the spans of the waves tile [0, H): no row of the canvas is written twice or left unwritten.
PA_HD bool pa_band_row_fits(const int* row, int H, long stride, int R, int count, int k) {
    if (count != pa_band_count(H, R) || k < 0 || k >= count) return false;
    int r0, r1;
    pa_band_span(H, R, k, &r0, &r1);
    return (long)row[PAB_OUT] == (long)r0 * stride && (long)row[PAB_OUT_BYTES] == (long)(r1 - r0) * stride;
}

// ... for the band rows begin, begin + step, ... of the file, `rows` its first: a wave asks with (lane, 64) and takes the
// answers of all lanes together, a host with (0, 1)
PA_HD bool pa_rows_fit(const int* rows, int H, long stride, int R, int count, int begin, int step) {
    for (int k = begin; k < count; k += step)
        if (!pa_band_row_fits(rows + (long)k * PA_BAND_INTS, H, stride, R, count, k)) return false;
    return true;
}

// What wave k of a flagged file of a bank does, `fit` being what its lanes found together (R >= 1 and pa_rows_fit).
// PA_REFUSE: status PA_NO_ROW, size 0 x 0 and the whole canvas zeroed, by the wave of band 0 alone; PA_LEAVE: nothing is
// written; PA_ROWS: the file's status and the rows of band k.
enum { PA_LEAVE = 0, PA_REFUSE = 1, PA_ROWS = 2 };
PA_HD int pa_wave_plan(bool fit, int k, int count) { return !fit ? (k == 0 ? PA_REFUSE : PA_LEAVE) : (k >= count ? PA_LEAVE : PA_ROWS); }

// what row r with filter byte ft adds to the file's marks: bit 0 a byte above 4, bit 1 a band's first row behind row 0 that
// is filtered against the row above (types 2, 3, 4)
PA_HD int pa_row_mark(int r, int ft, int R) { return (ft > 4 ? 1 : 0) | ((r > 0 && r % R == 0 && ft >= 2 && ft <= 4) ? 2 : 0); }

// the marks of rows begin, begin + step, ... of the filtered rows `raw` (H rows of `stride` bytes), or-ed
PA_HD int pa_marks(const uint8_t* raw, long stride, int H, int R, int begin, int step) {
    int marks = 0;
    for (int r = begin; r < H; r += step) marks |= pa_row_mark(r, raw[(long)r * stride], R);
    return marks;
}

// The file's status from the first failing band status in band order (0: none failed) and the marks of all rows or-ed; the
// marks are looked at with band == 0 only, for the rows of a failed band are not all there.
PA_HD int pa_status(int band, int marks) { return band != 0 ? band : (marks & 1) ? PA_FILTER : (marks & 2) ? PA_LIES : 0; }

// the size a file with this status reports: 0 x 0 for the bank's PA_NO_ROW, as csrc/png_bank.hip has it, else H x W
#define PA_NO_ROW 9
PA_HD bool pa_sized(int status) { return status != PA_NO_ROW; }
