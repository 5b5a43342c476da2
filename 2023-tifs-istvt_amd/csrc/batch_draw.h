// The batch draw (DESIGN.md "Batch draw"): which clips a training step takes and how each is augmented, as a pure function of
// (seed, step), in integer arithmetic that the kernel of batch_draw.hip and a host program (tools/batch_draw_check.cpp, built
// with sanitizers) both compile.  clips.batch_draw_host is the definition on the host.
//
// Everything lives in one int32 tensor, the draw block:
//
//   [0, 36)    the header, BD_* below: counts, thresholds, the seed, the 64-bit step, the status, the step that was drawn,
//              and the offsets (in ints from the block's start) of the nine parts that follow the index
//   [36, ...)  index int32 [B*T], at a fixed place: istvt_jpeg_decode_drawn_u8 hands it to the plan kernel of the bank
//   then, each at its offset and in this order, with whatever lies between them left alone:
//     videos  [V][3]   (first place of the bank, frame count, label)          read
//     base    [N][4]   (y0, x0, h, w) of every place of the bank              read
//     shapes  [K][2]   Q16 factors (rh, rw) of the box sides                  read
//     kinds   [nk][3]  (kind, lo, hi) of the perturbations                    read
//     boxes   [B*T][4], quality [B*T], view [B][3], perturb [B][4], label [B]  written
//
//   bd_check    the header against the scalars of the call and the block's length: 0, or BD_STATUS_HEADER
//   bd_video_ok a row of videos inside the base table and long enough for a clip
//   bd_clip     the draw of clip b at a step: twelve Philox words -> its rows of the five output tables and of the index
#ifndef ISTVT_BATCH_DRAW_H
#define ISTVT_BATCH_DRAW_H

#include <stdint.h>
#include "philox.h"
#define BD_HD PHILOX_HD

enum { BD_MAGIC = 0, BD_INTS, BD_B, BD_T, BD_STRIDE, BD_V, BD_N, BD_K, BD_NK, BD_JPEG_LO, BD_JPEG_HI, BD_RESERVED0,
       BD_THR_FLIP = 12, BD_THR_JPEG = 14, BD_THR_PERTURB = 16, BD_SEED = 18, BD_STEP = 20, BD_STATUS = 22, BD_RESERVED1,
       BD_DRAWN = 24, BD_OFF_VIDEOS = 26, BD_OFF_BASE, BD_OFF_SHAPES, BD_OFF_KINDS, BD_OFF_BOXES, BD_OFF_QUALITY, BD_OFF_VIEW,
       BD_OFF_PERTURB, BD_OFF_LABEL, BD_RESERVED2 };
constexpr int BD_HEADER_INTS = 36;           // the index starts here
constexpr int BD_PARTS = 9;                  // offsets BD_OFF_VIDEOS .. BD_OFF_LABEL
constexpr int BD_MAGIC_VALUE = 0x57524442;   // 'BDRW'
constexpr int BD_STATUS_HEADER = 1;          // the header disagrees with the call, or a part leaves the block: nothing drawn
constexpr int BD_STATUS_VIDEOS = 2;          // a row of videos leaves the base table or is shorter than a clip: nothing drawn
constexpr int BD_MAX_SIDE = 16384;

struct BdPlan {
    int B, T, stride, V, N, K, nk, jpeg_lo, jpeg_hi;
    uint64_t thr_flip, thr_jpeg, thr_perturb;
    uint32_t seed_lo, seed_hi;
    long off[BD_PARTS];                      // videos, base, shapes, kinds, boxes, quality, view, perturb, label
};

BD_HD uint64_t bd_u64(const int* h, int at) { return (uint64_t)(uint32_t)h[at] | ((uint64_t)(uint32_t)h[at + 1] << 32); }

// an integer in [0, n) from a word: the high half of the 64-bit product
BD_HD int bd_u(uint32_t w, int n) { return (int)(((uint64_t)w * (uint32_t)n) >> 32); }

// The header of a block of block_ints ints (the caller's count of what is allocated: at least BD_HEADER_INTS + B * T)
// against the B and T of the call.  Reads block[0 .. BD_HEADER_INTS) alone.  After a 0 every part lies behind the index and
// inside the block, in the order of the header, so no two overlap.
BD_HD int bd_check(const int* h, int B, int T, long block_ints, BdPlan& p) {
    if (h[BD_MAGIC] != BD_MAGIC_VALUE || (long)h[BD_INTS] != block_ints || h[BD_B] != B || h[BD_T] != T) return BD_STATUS_HEADER;
    p.B = B, p.T = T, p.stride = h[BD_STRIDE], p.V = h[BD_V], p.N = h[BD_N], p.K = h[BD_K], p.nk = h[BD_NK];
    p.jpeg_lo = h[BD_JPEG_LO], p.jpeg_hi = h[BD_JPEG_HI];
    p.thr_flip = bd_u64(h, BD_THR_FLIP), p.thr_jpeg = bd_u64(h, BD_THR_JPEG), p.thr_perturb = bd_u64(h, BD_THR_PERTURB);
    p.seed_lo = (uint32_t)h[BD_SEED], p.seed_hi = (uint32_t)h[BD_SEED + 1];
    const uint64_t one = (uint64_t)1 << 32;
    if (p.stride < 1 || p.V < 1 || p.N < 1 || p.K < 1 || p.nk < 0) return BD_STATUS_HEADER;
    if (p.thr_flip > one || p.thr_jpeg > one || p.thr_perturb > one) return BD_STATUS_HEADER;
    if (p.thr_jpeg > 0 && !(1 <= p.jpeg_lo && p.jpeg_lo <= p.jpeg_hi && p.jpeg_hi <= 100)) return BD_STATUS_HEADER;
    if (p.thr_perturb > 0 && p.nk < 1) return BD_STATUS_HEADER;
    if ((long)(T - 1) * p.stride + 1 > p.N) return BD_STATUS_HEADER;
    const long n = (long)B * T;
    const long len[BD_PARTS] = {3L * p.V, 4L * p.N, 2L * p.K, 3L * p.nk, 4 * n, n, 3L * B, 4L * B, (long)B};
    long at = BD_HEADER_INTS + n;            // where the index ends
    for (int i = 0; i < BD_PARTS; ++i) {
        const long off = h[BD_OFF_VIDEOS + i];
        if (off < at || off + len[i] > block_ints) return BD_STATUS_HEADER;
        p.off[i] = off;
        at = off + len[i];
    }
    return 0;
}

// row v of videos: its places lie in the base table and hold a clip of T frames at the stride
BD_HD bool bd_video_ok(const BdPlan& p, const int* block, int v) {
    const int* row = block + p.off[0] + 3L * v;
    const long first = row[0], count = row[1];
    return first >= 0 && count >= (long)(p.T - 1) * p.stride + 1 && first + count <= p.N;
}

// Clip b of the batch at `step`: words w0..w11 = philox4x32_10((step low, step high, b, j), seed), j = 0, 1, 2.  Writes rows
// b * T .. b * T + T - 1 of index, boxes and quality and row b of view, perturb and label; reads videos, base, shapes and
// kinds.  The video rows have passed bd_video_ok, so every place read from base lies in it.
BD_HD void bd_clip(const BdPlan& p, int* block, uint64_t step, int b) {
    uint32_t w[12];
    for (int j = 0; j < 3; ++j) {
        uint32_t r[4];
        philox4x32_10((uint32_t)step, (uint32_t)(step >> 32), (uint32_t)b, (uint32_t)j, p.seed_lo, p.seed_hi, r);
        w[4 * j] = r[0], w[4 * j + 1] = r[1], w[4 * j + 2] = r[2], w[4 * j + 3] = r[3];
    }
    const int* videos = block + p.off[0];
    const int* base = block + p.off[1];
    const int* shapes = block + p.off[2];
    const int* kinds = block + p.off[3];
    int* index = block + BD_HEADER_INTS;
    int* boxes = block + p.off[4];
    int* quality = block + p.off[5];
    int* view = block + p.off[6];
    int* perturb = block + p.off[7];
    int* label = block + p.off[8];

    const int* vid = videos + 3L * bd_u(w[0], p.V);
    const int span = (p.T - 1) * p.stride;
    const int place0 = vid[0] + bd_u(w[1], vid[1] - span);
    const int flip = (uint64_t)w[2] < p.thr_flip;
    const int* shape = shapes + 2L * bd_u(w[3], p.K);
    const long rh = shape[0], rw = shape[1];
    const int q = (uint64_t)w[6] < p.thr_jpeg ? p.jpeg_lo + bd_u(w[7], p.jpeg_hi - p.jpeg_lo + 1) : 0;
    for (int t = 0; t < p.T; ++t) {
        const long f = (long)b * p.T + t;
        const int place = place0 + t * p.stride;
        const int* bb = base + 4L * place;
        const int by = bb[0], bx = bb[1], bh = bb[2], bw = bb[3];
        const long m = bh < bw ? bh : bw;
        long h = (m * rh + 32768) >> 16, wd = (m * rw + 32768) >> 16;
        h = h < 1 ? 1 : h > bh ? bh : h;
        wd = wd < 1 ? 1 : wd > bw ? bw : wd;
        index[f] = place;
        boxes[4 * f] = by + bd_u(w[4], bh - (int)h + 1);
        boxes[4 * f + 1] = bx + bd_u(w[5], bw - (int)wd + 1);
        boxes[4 * f + 2] = (int)h;
        boxes[4 * f + 3] = (int)wd;
        quality[f] = q;
    }
    view[3L * b] = 0, view[3L * b + 1] = 0, view[3L * b + 2] = flip;
    int kind = 0, param = 0;
    if ((uint64_t)w[8] < p.thr_perturb) {
        const int* row = kinds + 3L * bd_u(w[9], p.nk);
        kind = row[0];
        param = row[1] + bd_u(w[10], row[2] - row[1] + 1);
    }
    perturb[4L * b] = kind, perturb[4L * b + 1] = param, perturb[4L * b + 2] = (int)(w[11] & 0x3fffffffu), perturb[4L * b + 3] = b;
    label[b] = vid[2];
}

#endif
