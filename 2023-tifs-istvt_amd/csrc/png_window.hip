// PNG windows (DESIGN.md "PNG windows"): the decode of a batch or a bank of files whose bands stand alone through one box per
// place.  Only the bands a box touches are inflated and unfiltered, into a canvas that is a window of `rows` rows, and the box
// moved into that window is handed on to the crop.  Two launches of m * win_bands workgroups of one wave: wave b is slot
// b % win_bands of place b / win_bands and takes band kfirst + slot of the place's window.  Every wave settles the place for
// itself from the tables and the box (csrc/png_window.h has the arithmetic and every check), so no wave needs another.  The
// inflate is csrc/png_inflate.h's and the rows are unfiltered by csrc/png_unfilter_alone.h's png_unfilter_rows, both as they
// are.  The bytes and statuses of clips.png_bank_window_host.  A file of its own, so that the kernels of the other decoders
// compile as they did.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "common.h"
#include "istvt_hip.h"
#include "png_inflate.h"
#include "png_launch.h"
#include "png_unfilter_alone.h"
#include "png_window.h"

static_assert(PK_IMAGE_INTS == ISTVT_PNG_BANK_IMAGE_INTS && PK_BAND_INTS == ISTVT_PNG_BAND_INTS && ISTVT_PNG_IMAGE_INTS == 8,
              "csrc/png_window.h and the header disagree");

namespace {

// What every wave of place j finds, from values that are the same in all lanes: the status the tables and the box give (0:
// none) -> and with 0 the file's number, its row, its first band row, R and the window.  All 64 lanes are here: the band rows
// of the file are checked by the lanes together.
__device__ __forceinline__ int pw_settle(const int* __restrict__ images, const int* __restrict__ bands, const int* __restrict__ index,
                                         const int* __restrict__ boxes, const PwCall& c, int j, int lane, int* i, int* im,
                                         const int** rows, int* R, PwWindow* w) {
    *i = c.bank ? index[j] : j;
    const int st = pw_file(images, bands, c, *i, im, rows, R);
    if (st != 0) return st;
    const long stride = 1 + (long)im[PK_W] * im[PK_BPP];
    const bool fit = __all(pa_rows_fit(*rows, im[PK_H], stride, *R, im[PK_BANDS], lane, 64));
    return pw_place(fit, im, *R, boxes + (long)j * PW_BOX_INTS, c, w);
}

// Slot t of place j inflates band kfirst + t into the place's window of the scratch: a wave whose place has a status, or
// whose window has no such band, leaves whole and before any barrier.  A band row that does not name the file or its stream
// (pk_band_ok), or would write outside the place's win_stride bytes, is band status PK_ROW and nothing is written.
__global__ __launch_bounds__(64) void png_window_inflate_kernel(const uint8_t* __restrict__ bytes, const int* __restrict__ images,
                                                                const int* __restrict__ bands, const int* __restrict__ index,
                                                                const int* __restrict__ boxes, PwCall c, uint8_t* __restrict__ scratch,
                                                                int* __restrict__ band_status) {
    __shared__ PiTables T;
    const int lane = threadIdx.x;
    int j, t, i, R, im[PK_IMAGE_INTS];
    const int* rows = nullptr;
    PwWindow w;
    pw_wave((int)blockIdx.x, c.win_bands, &j, &t);
    if (pw_settle(images, bands, index, boxes, c, j, lane, &i, im, &rows, &R, &w) != 0) return;
    const int k = pw_band(w, t);
    if (k < 0) return;
    const int* row = rows + (long)k * PK_BAND_INTS;
    const long at = pw_band_at(row, w, 1 + (long)im[PK_W] * im[PK_BPP], c.win_stride);
    int st = PK_ROW;
    if (at >= 0 && pk_band_ok(row, im, i))
        st = pi_inflate<true>(bytes + pk_base(im), row[PKB_BEGIN], row[PKB_END], scratch + (long)j * c.win_stride + at,
                              row[PKB_OUT_BYTES], &T, lane, k != im[PK_BANDS] - 1);
    if (lane == 0) band_status[(long)j * c.win_bands + t] = st;
}

// what the wave of slot 0 leaves of a place with status st: the status, the size (0 x 0 where the file's row was not
// accepted), origin 0, the box (0, 0, 1, 1) and a window of zeros
__device__ __forceinline__ void pw_refuse(int st, const int* im, uint8_t* window, const PwCall& c, int* __restrict__ sizes, int* status,
                                          int* __restrict__ moved, int* __restrict__ origin, int j, int lane) {
    if (lane == 0) {
        status[j] = st;
        sizes[2 * j] = pw_sized(st) ? im[PK_H] : 0;
        sizes[2 * j + 1] = pw_sized(st) ? im[PK_W] : 0;
        origin[j] = 0;
        moved[4 * j] = 0, moved[4 * j + 1] = 0, moved[4 * j + 2] = 1, moved[4 * j + 3] = 1;
    }
    png_zero(window, (long)c.k.Hc * c.k.Wc * 3, lane);
}

// Slot t of place j: the place's status -- the tables and the box as in the inflate, then the first status that is not 0 of
// the touched bands in band order, then the filter bytes of rows [w0, w1) alone -- and with status 0 the rows of band kfirst +
// t, unfiltered onto rows [r0 - w0, r1 - w0) of the window with the margin right of them.  The wave of slot 0 writes status,
// sizes, origin and the moved box, zeroes the rows below w1 - w0, and zeroes the whole window of a place with a status; the
// other waves of such a place leave.  The pointers handed to png_unfilter_rows stand w0 rows in front of the window's: it
// dereferences rows [r0, r1) only, which lie inside.
__global__ __launch_bounds__(64) void png_window_unfilter_kernel(const int* __restrict__ images, const int* __restrict__ bands,
                                                                 const int* __restrict__ index, const int* __restrict__ boxes, PwCall c,
                                                                 const int* __restrict__ band_status, uint8_t* scratch, uint8_t* out,
                                                                 int* __restrict__ sizes, int* status, int* __restrict__ moved,
                                                                 int* __restrict__ origin) {
    const int lane = threadIdx.x;
    int j, t, i, R, im[PK_IMAGE_INTS];
    const int* rows = nullptr;
    PwWindow w;
    pw_wave((int)blockIdx.x, c.win_bands, &j, &t);
    uint8_t* window = out + (long)j * c.k.Hc * c.k.Wc * 3;
    int st = pw_settle(images, bands, index, boxes, c, j, lane, &i, im, &rows, &R, &w);
    if (st == 0) {
        const int H = im[PK_H], W = im[PK_W], bpp = im[PK_BPP], touched = w.klast - w.kfirst + 1;
        const long stride = 1 + (long)W * bpp;
        uint8_t* raw = scratch + (long)j * c.win_stride;
        const int* statuses = band_status + (long)j * c.win_bands;
        int band = 0;
        for (int k0 = 0; k0 < touched && band == 0; k0 += 64) {
            const int mine = k0 + lane < touched ? statuses[k0 + lane] : 0;
            const unsigned long long failed = __ballot(mine != 0);
            if (failed) band = __shfl(mine, __ffsll((long long)failed) - 1);
        }
        int marks = 0;
        if (band == 0) {
            const int mine = pw_marks(raw, stride, w, R, lane, 64);
            marks = (__any(mine & 1) ? 1 : 0) | (__any(mine & 2) ? 2 : 0);
        }
        st = pa_status(band, marks);
        if (st == 0) {
            const int* box = boxes + (long)j * PW_BOX_INTS;
            if (t == 0) {
                if (lane == 0) {
                    status[j] = 0;
                    sizes[2 * j] = H, sizes[2 * j + 1] = W;
                    origin[j] = w.w0;
                    moved[4 * j] = box[0] - w.w0, moved[4 * j + 1] = box[1], moved[4 * j + 2] = box[2], moved[4 * j + 3] = box[3];
                }
                png_zero(window + (long)(w.w1 - w.w0) * c.k.Wc * 3, (long)(c.k.Hc - (w.w1 - w.w0)) * c.k.Wc * 3, lane);
            }
            const int k = pw_band(w, t);
            if (k < 0) return;
            int r0, r1;
            pa_band_span(H, R, k, &r0, &r1);
            const int right = (c.k.Wc - W) * 3;
            if (right > 0)
                for (int y = r0; y < r1; ++y) png_zero(window + ((long)(y - w.w0) * c.k.Wc + W) * 3, right, lane);
            png_unfilter_rows(r0, r1, W, bpp, raw - (long)w.w0 * stride, stride, window - (long)w.w0 * c.k.Wc * 3, c.k.Wc, lane);
            return;
        }
    }
    if (t == 0) pw_refuse(st, im, window, c, sizes, status, moved, origin, j, lane);
}

// what both entries ask beside the checks of the decoder they stand beside: the boxes, the slots, the bytes of a place, the
// scratch of the layout (csrc/png_window.h)
bool pw_args_ok(const istvt_jpeg_decode_args* a, int m, int win_bands, int win_stride) {
    if (!a->qtabs || a->nq != m || win_bands < 1 || win_stride < 16 || (win_stride & 15)) return false;
    if ((long)m * win_bands > 0x7fffffffL) return false;
    return a->scratch_bytes >= pw_scratch_bytes(m, win_bands, win_stride);
}

int pw_launch(const istvt_jpeg_decode_args* a, int m, const int* index, const PwCall& c) {
    uint8_t* scratch = (uint8_t*)a->scratch;
    int* band_status = reinterpret_cast<int*>(scratch + (long)m * c.win_stride);     // a multiple of 16 behind the rows
    int* moved = reinterpret_cast<int*>(scratch + pw_boxes_at(m, c.win_bands, c.win_stride));
    const dim3 grid((unsigned)(m * c.win_bands));
    hipLaunchKernelGGL(png_window_inflate_kernel, grid, dim3(64), 0, a->stream, (const uint8_t*)a->bytes, a->images, a->segments, index,
                       a->qtabs, c, scratch, band_status);
    const int rc = istvt_check_launch();
    if (rc != ISTVT_OK) return rc;
    hipLaunchKernelGGL(png_window_unfilter_kernel, grid, dim3(64), 0, a->stream, a->images, a->segments, index, a->qtabs, c, band_status,
                       scratch, (uint8_t*)a->out, a->sizes, a->status, moved, moved + (long)m * PW_BOX_INTS);
    return istvt_check_launch();
}

}  // namespace

// The batch of istvt_png_decode_alone_u8 through one box per file; include/istvt_hip.h describes the arguments.  The block and
// the host tables are checked as istvt_png_decode_bands_u8 checks them (png_bands_tables_ok: that entry's checks but for its
// canvas and its scratch row); the window's canvas and scratch are checked here.
extern "C" int istvt_png_decode_window_u8(const istvt_jpeg_decode_args* a, int win_bands, int win_stride) {
    if (!png_bands_tables_ok(a) || !pw_args_ok(a, a->n, win_bands, win_stride)) return ISTVT_ERR_SHAPE;
    if (a->Hc < 1 || a->Wc < 1 || a->Hc > PK_MAX_SIDE || a->Wc > PK_MAX_SIDE) return ISTVT_ERR_SHAPE;
    const uint8_t* src = (const uint8_t*)a->bytes;
    const uint8_t* dst = (const uint8_t*)a->out;
    if (dst < src + a->nbytes && src < dst + (long)a->n * a->Hc * a->Wc * 3) return ISTVT_ERR_SHAPE;
    if (!a->htabs || a->nh != a->n) return ISTVT_ERR_SHAPE;
    const int no_stride = 0x7ffffff0;                             // a batch's files have no bound but their own tables'
    for (int i = 0; i < a->n; ++i) {                               // every file carries the flag, and its band rows are an index's
        if (a->htabs[i] != 1) return ISTVT_ERR_SHAPE;
        const int* im = a->images_host + (long)i * ISTVT_PNG_IMAGE_INTS;
        if (im[PK_W] > a->Wc) return ISTVT_ERR_SHAPE;
        const int* rows = a->segments_host + (long)im[6] * PA_BAND_INTS;
        const long stride = 1 + (long)im[PK_W] * im[PK_BPP];
        const int R = pa_alone_rows(rows[PAB_OUT_BYTES], stride);
        if (R < 1 || !pa_rows_fit(rows, im[PK_H], stride, R, im[7], 0, 1)) return ISTVT_ERR_SHAPE;
    }
    const PwCall c = {{a->nbytes, a->n, a->nseg, a->nseg, no_stride, a->Hc, a->Wc}, win_bands, win_stride, 0};
    return pw_launch(a, a->n, nullptr, c);
}

// The bank of istvt_png_decode_bank_alone_u8 through one box per place.  Scalars only, once per call: png_bank_args_ok with
// the window's slots and bytes in the place of the canvas's bands and rows, then what the window adds.
extern "C" int istvt_png_decode_bank_window_u8(const istvt_jpeg_decode_args* a, int m, int band_max, int raw_stride, int win_bands,
                                               int win_stride) {
    PwCall c;
    if (band_max < 1 || raw_stride < 16 || (raw_stride & 15) || win_bands > band_max) return ISTVT_ERR_SHAPE;
    if (!png_bank_args_ok(a, m, win_bands, win_stride, &c.k) || !pw_args_ok(a, m, win_bands, win_stride)) return ISTVT_ERR_SHAPE;
    c.k.band_max = band_max, c.k.raw_stride = raw_stride;
    c.win_bands = win_bands, c.win_stride = win_stride, c.bank = 1;
    return pw_launch(a, m, a->images_host, c);
}
