// PNG files (DESIGN.md "PNG files"): a batch of 8-bit grey, RGB or RGBA files, packed by clips.png_batch, decoded from their
// DEFLATE streams to uint8 RGB on a canvas.  Two launches, one wave per file in each: png_inflate_kernel (csrc/png_inflate.h)
// writes the filtered rows into the file's row of the scratch, png_unfilter_kernel undoes the five row filters as a skewed
// wavefront of 64 rows and writes the canvas.  The bytes of clips.png_decode_host; a status per file in place of a fault.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "common.h"
#include "istvt_hip.h"
#include "png_inflate.h"
#include "png_unfilter.h"

namespace {

__global__ __launch_bounds__(64) void png_inflate_kernel(const uint8_t* __restrict__ bytes, const int* __restrict__ images,
                                                         uint8_t* __restrict__ scratch, long raw_stride, int* __restrict__ status) {
    __shared__ PiTables T;
    const int f = blockIdx.x, lane = threadIdx.x;
    const int* im = images + (long)f * ISTVT_PNG_IMAGE_INTS;
    const long expected = (long)im[PG_H] * (1 + (long)im[PG_W] * im[PG_BPP]);
    const int st = pi_inflate(bytes, im[PG_BEGIN], im[PG_END], scratch + (long)f * raw_stride, (int)expected, &T, lane);
    if (lane == 0) status[f] = st;
}

__global__ __launch_bounds__(64) void png_unfilter_kernel(const int* __restrict__ images, uint8_t* scratch, long raw_stride,
                                                          uint8_t* __restrict__ out, int Hc, int Wc, int* __restrict__ sizes,
                                                          int* status) {
    const int f = blockIdx.x, lane = threadIdx.x;
    png_unfilter_file<false>(images, nullptr, scratch, raw_stride, out, Hc, Wc, sizes, status, f, lane);
}

}  // namespace

// A batch of PNG files, packed by clips.png_batch, decoded to uint8 RGB on a canvas out [n][Hc][Wc][3]; include/istvt_hip.h
// describes the arguments.  Two launches, no synchronisation, no global state.
extern "C" int istvt_png_decode_u8(const istvt_jpeg_decode_args* a, int raw_stride) {
    if (!png_decode_args_ok(a, raw_stride) || a->scratch_bytes < (long)a->n * raw_stride) return ISTVT_ERR_SHAPE;
    const uint8_t* src = (const uint8_t*)a->bytes;
    uint8_t* out = (uint8_t*)a->out;
    hipLaunchKernelGGL(png_inflate_kernel, dim3((unsigned)a->n), dim3(64), 0, a->stream, src, a->images, (uint8_t*)a->scratch,
                       (long)raw_stride, a->status);
    int rc = istvt_check_launch();
    if (rc != ISTVT_OK) return rc;
    hipLaunchKernelGGL(png_unfilter_kernel, dim3((unsigned)a->n), dim3(64), 0, a->stream, a->images, (uint8_t*)a->scratch,
                       (long)raw_stride, out, a->Hc, a->Wc, a->sizes, a->status);
    return istvt_check_launch();
}
