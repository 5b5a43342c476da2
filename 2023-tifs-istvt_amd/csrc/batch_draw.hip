// The batch draw on the device (DESIGN.md "Batch draw"): one kernel reads the sampling plan and the step counter of a draw
// block and writes the batch's file index, per-frame boxes, flips, JPEG qualities, perturbation rows and labels into the same
// block; the kernels that take such tables then run from them unchanged.  csrc/batch_draw.h has the arithmetic, which
// tools/batch_draw_check.cpp compiles for the host; clips.batch_draw_host is the definition.
#include "common.h"
#include "batch_draw.h"

namespace {

constexpr int BD_LANES = 256;

// ONE workgroup: every lane reads the step, and only behind the barrier that follows does lane 0 store step + 1 -- a lane
// of a second workgroup could read the counter after it moved.  The lanes then loop over the clips.  A block that is
// refused (its header, or a row of videos) gets its status word and nothing else: no output row, no new step.
__global__ __launch_bounds__(BD_LANES) void batch_draw_kernel(int* __restrict__ block, int B, int T, int block_ints) {
    __shared__ int bad;
    const int tid = threadIdx.x;
    BdPlan p;
    const int refused = bd_check(block, B, T, block_ints, p);    // the same for every lane: the header is not written yet
    const uint64_t step = bd_u64(block, BD_STEP);
    if (tid == 0) bad = 0;
    __syncthreads();
    if (refused) {
        if (tid == 0) block[BD_STATUS] = refused;
        return;
    }
    bool mine = false;
    for (int v = tid; v < p.V; v += BD_LANES) mine |= !bd_video_ok(p, block, v);
    if (mine) bad = 1;                                           // every writer stores the same value
    __syncthreads();
    if (bad) {
        if (tid == 0) block[BD_STATUS] = BD_STATUS_VIDEOS;
        return;
    }
    for (int b = tid; b < B; b += BD_LANES) bd_clip(p, block, step, b);
    if (tid == 0) {
        const uint64_t next = step + 1;
        block[BD_STEP] = (int)(uint32_t)next, block[BD_STEP + 1] = (int)(uint32_t)(next >> 32);
        block[BD_DRAWN] = (int)(uint32_t)step, block[BD_DRAWN + 1] = (int)(uint32_t)(step >> 32);
        block[BD_STATUS] = 0;
    }
}

// what both entries ask of their scalars: the block holds its header and the index at least
bool bd_scalars_ok(const istvt_jpeg_decode_args* a, int B, int T, int block_ints) {
    if (!a || !a->images_host || B < 1 || T < 1 || (long)B * T > 0x7fffffffL / 8) return false;
    return (long)block_ints >= BD_HEADER_INTS + (long)B * T;
}

// The front of both drawn entries: the draw (istvt_batch_draw, which asks the scalars first) -> its return code, and the
// caller's block with images_host moved on to the index
int bd_draw_then(const istvt_jpeg_decode_args* a, int B, int T, int block_ints, istvt_jpeg_decode_args& indexed) {
    const int rc = istvt_batch_draw(a, B, T, block_ints);
    if (rc != ISTVT_OK) return rc;
    indexed = *a;
    indexed.images_host = a->images_host + BD_HEADER_INTS;
    return ISTVT_OK;
}

}  // namespace

// The draw alone; include/istvt_hip.h describes the block.  One launch, no synchronisation, nothing allocated.
extern "C" int istvt_batch_draw(const istvt_jpeg_decode_args* a, int B, int T, int block_ints) {
    if (!bd_scalars_ok(a, B, T, block_ints)) return ISTVT_ERR_SHAPE;
    int* block = const_cast<int*>(a->images_host);               // this entry's reading of the field: the draw block, on the device
    hipLaunchKernelGGL(batch_draw_kernel, dim3(1), dim3(BD_LANES), 0, a->stream, block, B, T, block_ints);
    return istvt_check_launch();
}

// The draw, then the indexed decode of the bank on the index the draw has just written: five launches.  A block that the
// draw refuses keeps the index it held, which the plan kernel of the bank checks like any other (status 4 outside the
// bank), so nothing outside the block or the bank is read either way.  The draw is launched before the indexed entry looks at
// its own scalars: a call that entry then refuses has drawn, and advanced the step, all the same.
extern "C" int istvt_jpeg_decode_drawn_u8(const istvt_jpeg_decode_args* a, int B, int T, int block_ints, int seg_max,
                                          int block_stride, int Hmax, int Wmax) {
    istvt_jpeg_decode_args indexed;
    const int rc = bd_draw_then(a, B, T, block_ints, indexed);
    return rc != ISTVT_OK ? rc : istvt_jpeg_decode_indexed_u8(&indexed, B * T, seg_max, block_stride, Hmax, Wmax);
}

// The same with the split decode of the bank behind the draw (istvt_jpeg_decode_indexed_split_u8): five launches.
extern "C" int istvt_jpeg_decode_drawn_split_u8(const istvt_jpeg_decode_args* a, int B, int T, int block_ints, int seg_max,
                                                int block_stride, int Hmax, int Wmax, int chunk_bytes, int chunk_rows,
                                                int seg_bytes_max) {
    istvt_jpeg_decode_args indexed;
    const int rc = bd_draw_then(a, B, T, block_ints, indexed);
    return rc != ISTVT_OK ? rc : istvt_jpeg_decode_indexed_split_u8(&indexed, B * T, seg_max, block_stride, Hmax, Wmax, chunk_bytes,
                                                                    chunk_rows, seg_bytes_max);
}

// The draw, then the indexed decode of a PNG bank (csrc/png_bank.hip) on the index the draw has just written: three launches.
// A refused block keeps the index it held, which the bank's kernels check like any other (status 8 outside the bank).
extern "C" int istvt_png_decode_bank_drawn_u8(const istvt_jpeg_decode_args* a, int B, int T, int block_ints, int band_max,
                                              int raw_stride) {
    istvt_jpeg_decode_args indexed;
    const int rc = bd_draw_then(a, B, T, block_ints, indexed);
    return rc != ISTVT_OK ? rc : istvt_png_decode_bank_u8(&indexed, B * T, band_max, raw_stride);
}

// The same in front of istvt_png_decode_bank_alone_u8 (csrc/png_alone.hip), for a bank packed with clips.png_bank(alone=True)
extern "C" int istvt_png_decode_bank_alone_drawn_u8(const istvt_jpeg_decode_args* a, int B, int T, int block_ints, int band_max,
                                                    int raw_stride) {
    istvt_jpeg_decode_args indexed;
    const int rc = bd_draw_then(a, B, T, block_ints, indexed);
    return rc != ISTVT_OK ? rc : istvt_png_decode_bank_alone_u8(&indexed, B * T, band_max, raw_stride);
}

// The same in front of istvt_png_decode_bank_window_u8 (csrc/png_window.hip): the caller's qtabs points at the boxes of the
// block, which the draw has written when the decode's kernels read them
extern "C" int istvt_png_decode_bank_window_drawn_u8(const istvt_jpeg_decode_args* a, int B, int T, int block_ints, int band_max,
                                                     int raw_stride, int win_bands, int win_stride) {
    istvt_jpeg_decode_args indexed;
    const int rc = bd_draw_then(a, B, T, block_ints, indexed);
    return rc != ISTVT_OK ? rc : istvt_png_decode_bank_window_u8(&indexed, B * T, band_max, raw_stride, win_bands, win_stride);
}
