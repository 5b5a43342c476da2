// PNG bands that stand alone (DESIGN.md "PNG bands that stand alone"): the unfilter launch of a batch packed with
// clips.png_batch(bands='index', alone=True) and of a bank packed with clips.png_bank(alone=True), one wave per band.  The
// inflate launches are those of csrc/png_bands.hip and csrc/png_bank.hip (csrc/png_launch.h).  A file whose index carries
// ISTVT_PNG_BAND_ALONE is unfiltered band by band, every wave settling the file's status for itself
// (csrc/png_unfilter_alone.h); a file without the flag is unfiltered whole by one wave as before.  The bytes and statuses of
// clips.png_decode_alone_host and clips.png_bank_decode_host.  A file of its own, so that the kernels of the other three
// decoders compile as they did.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "common.h"
#include "istvt_hip.h"
#include "png_alone.h"
#include "png_bank.h"
#include "png_launch.h"
#include "png_unfilter_alone.h"

static_assert(PA_BAND_INTS == ISTVT_PNG_BAND_INTS && PA_NO_ROW == PK_ROW && PA_FILTER == PG_FILTER, "csrc/png_alone.h and its siblings disagree");
static_assert(PK_FLAGS == ISTVT_PNG_BANK_IMAGE_INTS - 1, "the flags are the last word of a bank's image row");

namespace {

constexpr int PB_FILE = 0;

// One wave per row b of the band table, which the host has checked (png_bands_args_ok, pa_batch_ok): band k = b - the file's
// first row.  Every decision is uniform over the wave: a wave that leaves does so whole and before any barrier.
// A file without the flag is unfiltered whole by wave f of the launch, f its number (nseg >= n), not by the wave of its band
// 0: workgroups start in the order of their numbers, some 50 ns apart, and the long serial jobs have to start first, as the n
// waves of png_unfilter_bands_kernel do.  (Measured with them at the band-0 waves: 256 files of 224 x 224 at band_rows 8, 7168
// waves, 0.37 ms more than that kernel.)  The wave then goes on to its own row.
__global__ __launch_bounds__(64) void png_unfilter_alone_kernel(const int* __restrict__ images, const int* __restrict__ bands,
                                                                const int* __restrict__ flags, const int* __restrict__ band_status,
                                                                uint8_t* scratch, long raw_stride, uint8_t* out, int Hc, int Wc,
                                                                int* __restrict__ sizes, int* status, int n) {
    const int b = blockIdx.x, lane = threadIdx.x;
    if (b < n && !(flags[b] & 1)) png_unfilter_file<true>(images, band_status, scratch, raw_stride, out, Hc, Wc, sizes, status, b, lane);
    const int f = bands[(long)b * PA_BAND_INTS + PB_FILE];
    if (!(flags[f] & 1)) return;
    const int* im = images + (long)f * ISTVT_PNG_IMAGE_INTS;
    const int first = im[PG_FIRST_BAND], k = b - first;
    const int H = im[PG_H], W = im[PG_W], bpp = im[PG_BPP];
    const int R = pa_alone_rows(bands[(long)first * PA_BAND_INTS + PAB_OUT_BYTES], 1 + (long)W * bpp);
    png_unfilter_alone(H, W, bpp, R, k, band_status + first, im[PG_BANDS], scratch + (long)f * raw_stride, out + (long)f * Hc * Wc * 3, Hc,
                       Wc, sizes, status, f, lane);
}

// status st with size 0 x 0 and a canvas of zeros for place j
__device__ __forceinline__ void pa_refuse(int st, uint8_t* out, const PkCall& c, int* __restrict__ sizes, int* status, int j, int lane) {
    if (lane == 0) {
        status[j] = st;
        sizes[2 * j] = 0;
        sizes[2 * j + 1] = 0;
    }
    png_zero(out + (long)j * c.Hc * c.Wc * 3, (long)c.Hc * c.Wc * 3, lane);
}

// Wave b is band k = b % band_max of place j = b / band_max, as in png_bank_inflate_kernel.  First, wave b < m does for place
// b what png_bank_unfilter_kernel's wave b does where the place has no flagged file: the refusal pk_place_plan asks for, or the
// serial unfilter of a file without the flag -- the first m waves of the launch, so that the long jobs start first (see
// png_unfilter_alone_kernel).  Then every wave looks at its own (j, k): a flagged file whose band rows are not the R-row
// bands of an index (pa_rows_fit) is refused by the wave of band 0 and left by the others, else wave k takes band k.  Every
// wave of a place reads the same rows and decides the same, from values that are the same in all lanes.
__global__ __launch_bounds__(64) void png_bank_unfilter_alone_kernel(const int* __restrict__ images, const int* __restrict__ bands,
                                                                     const int* __restrict__ index, PkCall c,
                                                                     const int* __restrict__ band_status, uint8_t* scratch, uint8_t* out,
                                                                     int* __restrict__ sizes, int* status, int m) {
    const int b = (int)blockIdx.x, lane = threadIdx.x;
    const int* im = nullptr;
    if (b < m) {
        const int st = pk_place_plan(images, c, index[b], &im);
        if (st != 0) {
            pa_refuse(st, out, c, sizes, status, b, lane);
        } else if (!(im[PK_FLAGS] & 1)) {
            png_unfilter_file<true>(im[PK_H], im[PK_W], im[PK_BPP], band_status + (long)b * c.band_max, im[PK_BANDS], scratch,
                                    (long)c.raw_stride, out, c.Hc, c.Wc, sizes, status, b, lane);
            if (lane == 0 && status[b] == PK_ROW) {              // a band row that did not fit: lane 0 wrote the status itself
                sizes[2 * b] = 0;
                sizes[2 * b + 1] = 0;
            }
        }
    }
    int j, k;
    pk_wave(b, c.band_max, &j, &k);
    if (pk_place_plan(images, c, index[j], &im) != 0 || !(im[PK_FLAGS] & 1)) return;
    const int H = im[PK_H], W = im[PK_W], bpp = im[PK_BPP], count = im[PK_BANDS];
    const int* statuses = band_status + (long)j * c.band_max;
    const long stride = 1 + (long)W * bpp;
    const long at = pk_band_row(im, 0, c.nseg);
    const bool inside = at >= 0 && pk_band_row(im, count - 1, c.nseg) >= 0;       // rows [at, at + count) of the table
    const int* rows = bands + (inside ? at : 0) * PA_BAND_INTS;
    const int R = inside ? pa_alone_rows(rows[PAB_OUT_BYTES], stride) : 0;
    const bool fit = R > 0 && __all(pa_rows_fit(rows, H, stride, R, count, lane, 64));
    const int plan = pa_wave_plan(fit, k, count);
    if (plan == PA_REFUSE) pa_refuse(PK_ROW, out, c, sizes, status, j, lane);
    if (plan != PA_ROWS) return;
    png_unfilter_alone(H, W, bpp, R, k, statuses, count, scratch + (long)j * c.raw_stride, out + (long)j * c.Hc * c.Wc * 3, c.Hc, c.Wc, sizes,
                       status, j, lane);
}

// The host copies of the flags and of the band rows of the flagged files, behind png_bands_args_ok: a flag word is 0 or 1;
// the band rows of a flagged file are the R-row bands of its index, R from its band row 0.
bool pa_batch_ok(const istvt_jpeg_decode_args* a, const int* flags) {
    for (int i = 0; i < a->n; ++i) {
        if (flags[i] & ~1) return false;
        if (!(flags[i] & 1)) continue;
        const int* im = a->images_host + (long)i * ISTVT_PNG_IMAGE_INTS;
        const int* rows = a->segments_host + (long)im[PG_FIRST_BAND] * PA_BAND_INTS;
        const long stride = 1 + (long)im[PG_W] * im[PG_BPP];
        const int R = pa_alone_rows(rows[PAB_OUT_BYTES], stride);
        if (R < 1 || !pa_rows_fit(rows, im[PG_H], stride, R, im[PG_BANDS], 0, 1)) return false;
    }
    return true;
}

}  // namespace

// The batch of istvt_png_decode_bands_u8 with every file's flag; include/istvt_hip.h describes the arguments.  Two launches,
// no synchronisation, no global state, nothing allocated.
extern "C" int istvt_png_decode_alone_u8(const istvt_jpeg_decode_args* a, int raw_stride) {
    if (!png_bands_args_ok(a, raw_stride)) return ISTVT_ERR_SHAPE;
    if (!a->qtabs || !a->htabs || a->nq != a->n || a->nh != a->n || !pa_batch_ok(a, a->htabs)) return ISTVT_ERR_SHAPE;
    const int rc = png_bands_inflate_launch(a, raw_stride);
    if (rc != ISTVT_OK) return rc;
    uint8_t* scratch = (uint8_t*)a->scratch;
    const int* band_status = reinterpret_cast<const int*>(scratch + (long)a->n * raw_stride);
    hipLaunchKernelGGL(png_unfilter_alone_kernel, dim3((unsigned)a->nseg), dim3(64), 0, a->stream, a->images, a->segments, a->qtabs,
                       band_status, scratch, (long)raw_stride, (uint8_t*)a->out, a->Hc, a->Wc, a->sizes, a->status, a->n);
    return istvt_check_launch();
}

// The bank of istvt_png_decode_bank_u8 packed with clips.png_bank(alone=True): the same checks and inflate launch, then the
// unfilter with as many waves.  Two launches.
extern "C" int istvt_png_decode_bank_alone_u8(const istvt_jpeg_decode_args* a, int m, int band_max, int raw_stride) {
    PkCall c;
    if (!png_bank_args_ok(a, m, band_max, raw_stride, &c)) return ISTVT_ERR_SHAPE;
    const int rc = png_bank_inflate_launch(a, m, c);
    if (rc != ISTVT_OK) return rc;
    uint8_t* scratch = (uint8_t*)a->scratch;
    const int* band_status = reinterpret_cast<const int*>(scratch + (long)m * raw_stride);
    hipLaunchKernelGGL(png_bank_unfilter_alone_kernel, dim3((unsigned)(m * band_max)), dim3(64), 0, a->stream, a->images, a->segments,
                       a->images_host, c, band_status, scratch, (uint8_t*)a->out, a->sizes, a->status, m);
    return istvt_check_launch();
}
