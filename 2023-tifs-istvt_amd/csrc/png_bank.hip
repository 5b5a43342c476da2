// PNG bank (DESIGN.md "PNG bank"): the files of a clips.PngBank stay on the device, and the m of them that a device index
// names are decoded by their bands.  No plan kernel and no planned table: both kernels look the index up themselves
// (csrc/png_bank.h has the arithmetic and every check), form bytes + the file's 64-bit base once and hand the inflate
// file-relative 32-bit offsets, so the bank may hold more than 2^31 bytes.  png_bank_inflate_kernel runs one wave per
// (place, band) with band_max bands per place; png_bank_unfilter_kernel one wave per place.  The bytes and statuses of
// clips.png_bank_decode_host.  A file of its own, so that the kernels of csrc/png.hip and csrc/png_bands.hip compile as they did.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "common.h"
#include "istvt_hip.h"
#include "png_bank.h"
#include "png_inflate.h"
#include "png_launch.h"
#include "png_unfilter.h"

static_assert(PK_IMAGE_INTS == ISTVT_PNG_BANK_IMAGE_INTS && PK_BAND_INTS == ISTVT_PNG_BAND_INTS, "csrc/png_bank.h and the header disagree");

namespace {

// Wave b is band k = b % band_max of place j = b / band_max.  Every decision is pk_band_plan's, from values that are the same
// in all lanes: a wave that leaves does so whole and before any barrier.
__global__ __launch_bounds__(64) void png_bank_inflate_kernel(const uint8_t* __restrict__ bytes, const int* __restrict__ images,
                                                              const int* __restrict__ bands, const int* __restrict__ index, PkCall c,
                                                              uint8_t* __restrict__ scratch, int* __restrict__ band_status) {
    __shared__ PiTables T;
    const int lane = threadIdx.x;
    int j, k;
    pk_wave((int)blockIdx.x, c.band_max, &j, &k);
    const int i = index[j];
    const int* im = nullptr;
    const int* row = nullptr;
    const int plan = pk_band_plan(images, bands, c, i, k, &im, &row);
    if (plan == PK_SKIP) return;
    int st = PK_ROW;
    if (plan == PK_RUN)
        st = pi_inflate<true>(bytes + pk_base(im), row[PKB_BEGIN], row[PKB_END], scratch + (long)j * c.raw_stride + row[PKB_OUT],
                              row[PKB_OUT_BYTES], &T, lane, k != im[PK_BANDS] - 1);
    if (lane == 0) band_status[(long)j * c.band_max + k] = st;
}

// One wave per place: status 8 or 9 with size 0 x 0 and a canvas of zeros where pk_place_plan says so, else the unfilter of
// csrc/png_unfilter.h with the file's fields from the bank's row and the band statuses of this place.
__global__ __launch_bounds__(64) void png_bank_unfilter_kernel(const int* __restrict__ images, const int* __restrict__ index, PkCall c,
                                                               const int* __restrict__ band_status, uint8_t* scratch,
                                                               uint8_t* __restrict__ out, int* __restrict__ sizes, int* status) {
    const int j = blockIdx.x, lane = threadIdx.x;
    const int* im = nullptr;
    const int st = pk_place_plan(images, c, index[j], &im);
    if (st != 0) {
        if (lane == 0) {
            status[j] = st;
            sizes[2 * j] = 0;
            sizes[2 * j + 1] = 0;
        }
        png_zero(out + (long)j * c.Hc * c.Wc * 3, (long)c.Hc * c.Wc * 3, lane);
        return;
    }
    png_unfilter_file<true>(im[PK_H], im[PK_W], im[PK_BPP], band_status + (long)j * c.band_max, im[PK_BANDS], scratch, (long)c.raw_stride,
                            out, c.Hc, c.Wc, sizes, status, j, lane);
    if (lane == 0 && status[j] == PK_ROW) {                      // a band row that did not fit: lane 0 wrote the status itself
        sizes[2 * j] = 0;
        sizes[2 * j + 1] = 0;
    }
}

}  // namespace

// What istvt_png_decode_bank_u8 refuses, and its first launch: csrc/png_alone.hip puts its own unfilter behind the same two
// (csrc/png_launch.h declares them).  The checks are on scalars alone, once per call: the tables are on the device, and the
// kernels check the rows they use.
bool png_bank_args_ok(const istvt_jpeg_decode_args* a, int m, int band_max, int raw_stride, PkCall* call) {
    if (!a) return false;
    const PkCall c = {a->nbytes, a->n, a->nseg, band_max, raw_stride, a->Hc, a->Wc};
    if (!pk_scalars_ok(c, m, a->scratch_bytes)) return false;
    if (!a->bytes || !a->images || !a->segments || !a->images_host || !a->scratch || !a->out || !a->sizes || !a->status) return false;
    if ((reinterpret_cast<uintptr_t>(a->scratch) & 15) || (reinterpret_cast<uintptr_t>(a->bytes) & 15)) return false;
    const uint8_t* src = (const uint8_t*)a->bytes;
    const uint8_t* dst = (const uint8_t*)a->out;
    if (dst < src + a->nbytes && src < dst + (long)m * a->Hc * a->Wc * 3) return false;
    *call = c;
    return true;
}

int png_bank_inflate_launch(const istvt_jpeg_decode_args* a, int m, const PkCall& c) {
    uint8_t* scratch = (uint8_t*)a->scratch;
    int* band_status = reinterpret_cast<int*>(scratch + (long)m * c.raw_stride);     // a multiple of 16 behind the rows
    const int* index = a->images_host;                           // this entry's reading of the field: the index, on the device
    hipLaunchKernelGGL(png_bank_inflate_kernel, dim3((unsigned)(m * c.band_max)), dim3(64), 0, a->stream, (const uint8_t*)a->bytes,
                       a->images, a->segments, index, c, scratch, band_status);
    return istvt_check_launch();
}

// The indexed decode of a PNG bank; include/istvt_hip.h describes the arguments.  Two launches, no synchronisation, no global
// state, no atomics, nothing allocated; the band statuses live in the scratch behind the filtered rows.
extern "C" int istvt_png_decode_bank_u8(const istvt_jpeg_decode_args* a, int m, int band_max, int raw_stride) {
    PkCall c;
    if (!png_bank_args_ok(a, m, band_max, raw_stride, &c)) return ISTVT_ERR_SHAPE;
    const int rc = png_bank_inflate_launch(a, m, c);
    if (rc != ISTVT_OK) return rc;
    uint8_t* scratch = (uint8_t*)a->scratch;
    const int* band_status = reinterpret_cast<const int*>(scratch + (long)m * raw_stride);
    hipLaunchKernelGGL(png_bank_unfilter_kernel, dim3((unsigned)m), dim3(64), 0, a->stream, a->images, a->images_host, c, band_status,
                       scratch, (uint8_t*)a->out, a->sizes, a->status);
    return istvt_check_launch();
}
