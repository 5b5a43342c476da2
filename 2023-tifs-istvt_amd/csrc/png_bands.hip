// PNG files by their bands (DESIGN.md "PNG files by their bands"): the batch of csrc/png.hip packed with
// clips.png_batch(bands='index'), every file's stream taken apart where its baND chunk says a band begins.
// png_inflate_bands_kernel runs one wave per band, each into its own rows of the scratch with a status word of its own;
// png_unfilter_bands_kernel, still one wave per file, takes the first band status that is not 0 as the file's.  The bytes and
// statuses of clips.png_decode_bands_host.  A file of its own, so that the sequential kernels compile as they did.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "common.h"
#include "istvt_hip.h"
#include "png_inflate.h"
#include "png_launch.h"
#include "png_unfilter.h"

namespace {

constexpr int PB_FILE = 0, PB_BEGIN = 1, PB_END = 2, PB_OUT = 3, PB_OUT_BYTES = 4;

// One wave per band: bytes [begin, end) of the band -> its rows of its file's filtered bytes.  The band's window, count and
// status are its own; a band that is not its file's last stops at the stored block that closes it (csrc/png_inflate.h).
__global__ __launch_bounds__(64) void png_inflate_bands_kernel(const uint8_t* __restrict__ bytes, const int* __restrict__ images,
                                                               const int* __restrict__ bands, uint8_t* __restrict__ scratch,
                                                               long raw_stride, int* __restrict__ band_status) {
    __shared__ PiTables T;
    const int b = blockIdx.x, lane = threadIdx.x;
    const int* row = bands + (long)b * ISTVT_PNG_BAND_INTS;
    const int f = row[PB_FILE];
    const int* im = images + (long)f * ISTVT_PNG_IMAGE_INTS;
    const bool middle = b != im[PG_FIRST_BAND] + im[PG_BANDS] - 1;
    const int st = pi_inflate<true>(bytes, row[PB_BEGIN], row[PB_END], scratch + (long)f * raw_stride + row[PB_OUT],
                                    row[PB_OUT_BYTES], &T, lane, middle);
    if (lane == 0) band_status[b] = st;
}

// The rows stay serial over the file: a band's first row may be filtered against the row above it, which another band made.
__global__ __launch_bounds__(64) void png_unfilter_bands_kernel(const int* __restrict__ images, const int* __restrict__ band_status,
                                                                uint8_t* scratch, long raw_stride, uint8_t* __restrict__ out, int Hc,
                                                                int Wc, int* __restrict__ sizes, int* status) {
    const int f = blockIdx.x, lane = threadIdx.x;
    png_unfilter_file<true>(images, band_status, scratch, raw_stride, out, Hc, Wc, sizes, status, f, lane);
}

// the host copy of the band table against the image table: the rows of file i are images[i][6] .. + images[i][7], in file
// order without a gap; every band lies inside its file's bytes; a file's output ranges follow one another from 0 and end at
// H (1 + W bpp).  png_decode_check has passed, so that is at most raw_stride.
bool png_bands_check(const istvt_jpeg_decode_args* a) {
    if (!a->segments || !a->segments_host || a->nseg < a->n) return false;
    long at = 0;
    for (int i = 0; i < a->n; ++i) {
        const int* im = a->images_host + (long)i * ISTVT_PNG_IMAGE_INTS;
        const int count = im[PG_BANDS];
        if (im[PG_FIRST_BAND] != at || count < 1 || count > a->nseg - at) return false;
        long produced = 0;
        for (int k = 0; k < count; ++k) {
            const int* row = a->segments_host + (at + k) * ISTVT_PNG_BAND_INTS;
            if (row[PB_FILE] != i || row[PB_BEGIN] < im[PG_BEGIN] || row[PB_BEGIN] > row[PB_END] || row[PB_END] > im[PG_END]) return false;
            if (row[PB_OUT] != produced || row[PB_OUT_BYTES] < 0) return false;
            produced += row[PB_OUT_BYTES];
        }
        if (produced != (long)im[PG_H] * (1 + (long)im[PG_W] * im[PG_BPP])) return false;
        at += count;
    }
    return at == a->nseg;
}

}  // namespace

// What istvt_png_decode_bands_u8 refuses, and its first launch: csrc/png_alone.hip puts its own unfilter behind the same two
// (csrc/png_launch.h declares them)
bool png_bands_args_ok(const istvt_jpeg_decode_args* a, int raw_stride) {
    if (!png_decode_args_ok(a, raw_stride) || !png_bands_check(a)) return false;
    return a->scratch_bytes >= (long)a->n * raw_stride + (long)a->nseg * (long)sizeof(int);
}

// ... and the part of it that knows no canvas and no scratch row: the block and the host tables alone, for csrc/png_window.hip
bool png_bands_tables_ok(const istvt_jpeg_decode_args* a) { return png_decode_block_ok(a) && png_bands_check(a); }

int png_bands_inflate_launch(const istvt_jpeg_decode_args* a, int raw_stride) {
    uint8_t* scratch = (uint8_t*)a->scratch;
    int* band_status = reinterpret_cast<int*>(scratch + (long)a->n * raw_stride);    // a multiple of 16: the status words start there
    hipLaunchKernelGGL(png_inflate_bands_kernel, dim3((unsigned)a->nseg), dim3(64), 0, a->stream, (const uint8_t*)a->bytes, a->images,
                       a->segments, scratch, (long)raw_stride, band_status);
    return istvt_check_launch();
}

// The same batch with a band table (clips.png_batch(bands='index')): one wave per band inflates, one wave per file unfilters.
// Two launches, no synchronisation, no global state; the band statuses live in the scratch behind the filtered rows.
extern "C" int istvt_png_decode_bands_u8(const istvt_jpeg_decode_args* a, int raw_stride) {
    if (!png_bands_args_ok(a, raw_stride)) return ISTVT_ERR_SHAPE;
    const int rc = png_bands_inflate_launch(a, raw_stride);
    if (rc != ISTVT_OK) return rc;
    uint8_t* scratch = (uint8_t*)a->scratch;
    const int* band_status = reinterpret_cast<const int*>(scratch + (long)a->n * raw_stride);
    hipLaunchKernelGGL(png_unfilter_bands_kernel, dim3((unsigned)a->n), dim3(64), 0, a->stream, a->images, band_status, scratch,
                       (long)raw_stride, (uint8_t*)a->out, a->Hc, a->Wc, a->sizes, a->status);
    return istvt_check_launch();
}
