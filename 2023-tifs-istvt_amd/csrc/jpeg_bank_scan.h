// The JPEG bank (DESIGN.md "JPEG bank"): the two pieces of arithmetic that can go wrong on unseen bytes or indices, as
// __host__ __device__ functions that the kernels of jpeg.hip and a host program (tools/jpeg_bank_check.cpp, built with
// sanitizers) both compile.
//
//   jb_markers        a lane's share of the marker scan of the device ingest: which of its 16 bytes start an RSTn pair
//   jb_plan_status    what place j of an indexed decode is: decodable (0), an index outside the bank (4), a bank row that
//                     holds no decodable file (5); for the split decode also a row with a segment longer than the bank says (5)
//   jb_plan_image     the batch-local images row of place j;  jb_plan_segment: row k of its seg_max segment rows
//
// clips.jpeg_scan_segments_host and clips.jpeg_bank_decode_host are the definitions on the host.
#ifndef ISTVT_JPEG_BANK_SCAN_H
#define ISTVT_JPEG_BANK_SCAN_H

#include "jpeg_entropy.h"

// the lanes of a scan workgroup take JB_LANE_BYTES each, a tile of JB_TILE_BYTES per trip
constexpr int JB_LANE_BYTES = 16;
constexpr int JB_TILE_BYTES = 256 * JB_LANE_BYTES;
// a row of the per-image table (the JD_* of jpeg.hip) and of the per-segment table
enum { JB_H = 0, JB_W, JB_SUB, JB_MCUX, JB_MCUY, JB_QUANT, JB_HUFF = 8, JB_BLOCK0 = 14, JB_GROUP0, JB_SEG0, JB_NSEG, JB_NBLOCKS,
       JB_LAYOUT };
constexpr int JB_IMAGE_INTS = ISTVT_JPEG_IMAGE_INTS;
constexpr int JB_SEGMENT_INTS = ISTVT_JPEG_SEGMENT_INTS;
constexpr int JB_STATUS_INDEX = 4, JB_STATUS_EMPTY = 5;

// Bit b is set where data[lo + b], data[lo + b + 1] is FF D0..D7, for lo + b in [lo, hi) and lo + b + 1 < end: the pairs that
// START in the lane's bytes, the last of which may end one byte behind them.  hi - lo <= 32; reads data[lo .. min(hi, end -
// 1)], nothing else.  Inside the entropy-coded bytes of a file an FF is followed by 00 (a data byte FF), RSTn or EOI, so a
// pair found this way is a restart marker whatever stands in front of it.
JE_HD uint32_t jb_markers(const uint8_t* data, long lo, long hi, long end) {
    uint32_t mask = 0;
    if (lo >= hi || lo + 1 >= end) return 0;
    uint32_t here = data[lo];
    for (long p = lo; p < hi && p + 1 < end; ++p) {
        const uint32_t next = data[p + 1];
        if (here == 0xFF && (next & 0xF8) == 0xD0) mask |= 1u << (int)(p - lo);
        here = next;
    }
    return mask;
}

// Place j of an indexed decode draws bank row `index`.  A row is decodable where its geometry fits the strides and the
// canvas of this call: the tables were checked when the bank was built, and these comparisons keep a device table that
// differs from them inside the scratch all the same.
JE_HD int jb_plan_status(const int* bank_images, int n, int bank_nseg, int index, int seg_max, int block_stride, int Hc, int Wc) {
    if (index < 0 || index >= n) return JB_STATUS_INDEX;
    const int* b = bank_images + (long)index * JB_IMAGE_INTS;
    const JeLayout lay = je_layout(b[JB_LAYOUT], b[JB_SUB]);
    const int mcux = b[JB_MCUX], mcuy = b[JB_MCUY], H = b[JB_H], W = b[JB_W];
    const bool ok = b[JB_NSEG] >= 1 && b[JB_NSEG] <= seg_max && b[JB_SEG0] >= 0 && (long)b[JB_SEG0] + b[JB_NSEG] <= bank_nseg &&
                    mcux >= 1 && mcuy >= 1 && mcux <= 2048 && mcuy <= 2048 &&
                    (long)mcux * mcuy * (lay.h * lay.v + lay.nc) <= block_stride && H >= 1 && W >= 1 && H <= Hc && W <= Wc &&
                    H <= mcuy * 8 * lay.v && W <= mcux * 8 * lay.h;
    return ok ? 0 : JB_STATUS_EMPTY;
}

// The same for the split decode of a bank (DESIGN.md "JPEG bank, split"), whose state rows are reserved for segments of at
// most seg_bytes_max bytes: a row with a longer segment is not decodable either, by the same rule -- the bound is the host's
// number, and a device table that exceeds it is kept inside the scratch.  seg_bytes_max < 0: no limit, the function above.
JE_HD int jb_plan_status(const int* bank_images, int n, const int* bank_segments, int bank_nseg, int index, int seg_max,
                         int block_stride, int Hc, int Wc, int seg_bytes_max) {
    const int st = jb_plan_status(bank_images, n, bank_nseg, index, seg_max, block_stride, Hc, Wc);
    if (st != 0 || seg_bytes_max < 0) return st;
    const int* b = bank_images + (long)index * JB_IMAGE_INTS;
    for (int k = 0; k < b[JB_NSEG]; ++k) {                       // 1 <= segments <= seg_max, all inside the table: checked above
        const int* s = bank_segments + ((long)b[JB_SEG0] + k) * JB_SEGMENT_INTS;
        if ((long)s[2] - s[1] > seg_bytes_max) return JB_STATUS_EMPTY;
    }
    return 0;
}

// The images row of place j of m.  Decodable: the bank's row with the first block, first IDCT workgroup and first segment of
// the uniform strides.  Otherwise an image of no pixels, no blocks and ONE segment, status word m * seg_max + j: the plan
// kernel stores 4 or 5 there, behind the words the entropy kernel writes, and the IDCT kernel's first workgroup of the
// image hands it on as the image's status with size (0, 0).
JE_HD void jb_plan_image(const int* bank_images, int index, int status, int j, int m, int seg_max, int block_stride, int* row) {
    if (status == 0) {
        const int* b = bank_images + (long)index * JB_IMAGE_INTS;
        for (int f = 0; f < JB_IMAGE_INTS; ++f) row[f] = b[f];
        row[JB_SEG0] = j * seg_max;
    } else {
        for (int f = 0; f < JB_IMAGE_INTS; ++f) row[f] = 0;
        row[JB_SUB] = 1;
        row[JB_SEG0] = m * seg_max + j;
        row[JB_NSEG] = 1;
    }
    row[JB_BLOCK0] = j * block_stride;
    row[JB_GROUP0] = j * (block_stride / ISTVT_JPEG_IDCT_BLOCKS);
}

// Segment row k < seg_max of place j: the bank's row with the image rewritten, or, behind the image's real count (and for
// an image that is not decodable), a row the entropy kernel rejects by its image, -1.  The IDCT kernel reads the statuses of
// the real count alone, so the 2 such a row reports never reaches an image.
JE_HD void jb_plan_segment(const int* bank_images, const int* bank_segments, int index, int status, int j, int k, int* row) {
    const int* b = bank_images + (long)(status == 0 ? index : 0) * JB_IMAGE_INTS;
    if (status == 0 && k < b[JB_NSEG]) {
        const int* s = bank_segments + ((long)b[JB_SEG0] + k) * JB_SEGMENT_INTS;
        row[0] = j, row[1] = s[1], row[2] = s[2], row[3] = s[3], row[4] = s[4];
    } else {
        row[0] = -1, row[1] = row[2] = row[3] = row[4] = 0;
    }
}

#endif
