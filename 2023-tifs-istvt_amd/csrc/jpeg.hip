// JPEG round trip (DESIGN.md "JPEG round trip"): frames uint8 [n][H][W][3] -> the uint8 RGB a baseline JPEG encoder and
// decoder hand back at each frame's quality, bytes to bytes and without a bitstream.  clips.jpeg_roundtrip_host is the
// definition and this file gives its bits: int32 arithmetic only (libjpeg's fixed-point colour transforms and its 13-bit
// "slow integer" DCT / IDCT), no floating point, no atomics, one writer per byte.
//
//   colour in    Y = (19595 R + 38470 G + 7471 B + 32768) >> 16, Cb / Cr likewise around 128
//   padding      to whole MCUs (16 x 16 pixels at 4:2:0, 8 x 8 at 4:4:4) by edge replication: every source read goes through
//                clamped coordinates
//   downsample   4:2:0: 2 x 2 box, (sum + 1 or 2) >> 2; chroma rows below the frame's ceil(H / 2) repeat the last of those
//   blocks       - 128, rows then columns forward (8 x the DCT), k = (|c| + 4 q) / (8 q) with the sign of c, k * q, columns
//                then rows inverse, + 128, clamp.  q = the Annex K entry scaled by the frame's quality
//   upsample     4:2:0: 3/4 + 1/4 vertically, then horizontally with + 8 / + 7 and >> 4; the chroma plane's edges replicate
//   colour out   R = Y + ((91881 Cr' + 32768) >> 16), ... ; clamp
//
// Two launches.  jpeg_planes_kernel: a workgroup takes a tile of one MCU row x 64 pixels of a frame, stages its source bytes
// in LDS with 16-byte loads (u8_stage_rows), converts them into 24 blocks of 8 x 8 samples in LDS -- 16 Y + 4 Cb + 4 Cr at
// 4:2:0, 8 + 8 + 8 at 4:4:4 -- and runs the 192 row and column transforms of a pass one per lane: forward rows | forward
// columns, quantise, multiply back, inverse columns (all in the lane's registers) | inverse rows, whose 8 bytes leave as one
// store into the caller's scratch planes (per frame Y [Hp][Wp], then Cb and Cr [Hp / s][Wp / s], s = 2 or 1; Hp, Wp = H, W
// rounded up to whole MCUs).  jpeg_rgb_kernel: a lane takes 4 consecutive pixels of the batch, reads Y and the (up to 4 + 4)
// chroma samples around each from the planes, and stores their 12 bytes as three dwords.  A frame whose quality is <= 0 is
// skipped by the first kernel and copied by the second.
//
// JPEG files (DESIGN.md "JPEG files") are the second half of this file: istvt_jpeg_decode_u8 decodes a batch of baseline
// files from their compressed bytes in three launches that share jp_idct8, jp_chroma and the colour-out expression with the
// round trip.  jpeg_entropy_kernel: one lane per restart interval (jpeg_entropy.h) -> int16 coefficients.
// jpeg_idct_kernel: the back half of jpeg_planes_kernel with the file's own tables -> the planes.  jpeg_canvas_kernel:
// jpeg_rgb_kernel over a canvas [n][Hc][Wc][3] that holds images of several sizes.  istvt_jpeg_decode_split_u8 (DESIGN.md
// "JPEG files without restart markers") puts jpeg_entropy_split_kernel in front instead: one workgroup per restart interval,
// one lane per chunk of it (jpeg_entropy_split.h), for files whose intervals are long.  istvt_jpeg_decode_indexed_u8 (DESIGN.md
// "JPEG bank") puts jpeg_bank_plan_kernel in front of the three kernels: files that stay on the device, drawn by an index
// that lives there; istvt_jpeg_bank_ingest builds such a bank from the encoder's result (jpeg_bank_scan.h).
// istvt_jpeg_decode_indexed_split_u8 (DESIGN.md "JPEG bank, split") is the indexed decode with the split kernel behind the
// plan, its state rows at a stride per planned segment.
//
// JPEG files out (DESIGN.md "JPEG files out") are the third part: istvt_jpeg_encode_u8 writes a batch of frames as baseline
// files in four launches.  jpeg_planes_kernel<SUB, true>: the front half of the round trip -> int16 coefficients.
// jpeg_count_kernel / jpeg_write_kernel: one lane per restart interval (jpeg_entropy_enc.h), first counting, then storing.
// jpeg_offsets_kernel between them: the prefix sum that lays the files end to end.  istvt_jpeg_encode_opt_u8 (DESIGN.md
// "JPEG files out, optimised tables") codes every file with its own Huffman tables: jpeg_tables_kernel counts an image's
// symbols in LDS and builds the four tables (jpeg_entropy_opt.h), then count, offsets and write with the image's codes.
// istvt_jpeg_encode_layout_u8 (DESIGN.md "JPEG files out, 4:2:2 and greyscale") is both of them in the decoder's other two
// layouts: jpeg_coef_kernel in front, whose MCUs are 16 x 8 or 8 x 8 pixels, and the same entropy kernels on a JeLayout.
#include "istvt_hip.h"
#include "jpeg_bank_scan.h"
#include "jpeg_entropy.h"
#include "jpeg_entropy_enc.h"
#include "jpeg_entropy_opt.h"
#include "jpeg_entropy_split.h"
#include "u8_view.h"

namespace {

constexpr int JP_TILE_W = 64;               // pixels per tile row: 8 blocks of Y
constexpr int JP_BLOCKS = ISTVT_JPEG_IDCT_BLOCKS;  // 8 x 8 blocks of a tile, either subsampling
constexpr int JP_BLOCK_LD = 72;             // ints between blocks in LDS: 64 + 8, so a column pass meets no bank twice
constexpr int JP_PITCH = 208;               // u8_row_pitch(JP_TILE_W)

// ITU-T T.81 Annex K.1 (luminance) and K.2 (chrominance), row = vertical frequency
__constant__ unsigned char JP_BASE[128] = {
    16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56,
    14, 17, 22, 29, 51, 87, 80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92,
    49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99,
    17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99,
    47, 66, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99,
    99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99};

__device__ __forceinline__ int jp_descale(int x, int n) { return (x + (1 << (n - 1))) >> n; }
__device__ __forceinline__ int jp_byte(int v) { return min(max(v, 0), 255); }

// One pass of the forward DCT (clips._fdct8): the first leaves 2 extra bits, the second takes them out; 8 x the DCT
template <bool FIRST> __device__ __forceinline__ void jp_fdct8(int (&d)[8]) {
    int t0 = d[0] + d[7], t7 = d[0] - d[7], t1 = d[1] + d[6], t6 = d[1] - d[6];
    int t2 = d[2] + d[5], t5 = d[2] - d[5], t3 = d[3] + d[4], t4 = d[3] - d[4];
    const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    constexpr int N = FIRST ? 11 : 15;
    d[0] = FIRST ? (t10 + t11) * 4 : jp_descale(t10 + t11, 2);
    d[4] = FIRST ? (t10 - t11) * 4 : jp_descale(t10 - t11, 2);
    int z1 = (t12 + t13) * 4433;
    d[2] = jp_descale(z1 + t13 * 6270, N);
    d[6] = jp_descale(z1 - t12 * 15137, N);
    z1 = t4 + t7;
    int z2 = t5 + t6, z3 = t4 + t6, z4 = t5 + t7;
    const int z5 = (z3 + z4) * 9633;
    t4 *= 2446, t5 *= 16819, t6 *= 25172, t7 *= 12299;
    z1 *= -7373, z2 *= -20995;
    z3 = z3 * -16069 + z5, z4 = z4 * -3196 + z5;
    d[7] = jp_descale(t4 + z1 + z3, N);
    d[5] = jp_descale(t5 + z2 + z4, N);
    d[3] = jp_descale(t6 + z2 + z3, N);
    d[1] = jp_descale(t7 + z1 + z4, N);
}

// One pass of the inverse DCT (clips._idct8): the first keeps 2 extra bits, the second removes them and the factor 8
template <bool FIRST> __device__ __forceinline__ void jp_idct8(int (&d)[8]) {
    int z1 = (d[2] + d[6]) * 4433;
    int t2 = z1 - d[6] * 15137, t3 = z1 + d[2] * 6270;
    int t0 = (d[0] + d[4]) * 8192, t1 = (d[0] - d[4]) * 8192;
    const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    t0 = d[7], t1 = d[5], t2 = d[3], t3 = d[1];
    z1 = t0 + t3;
    int z2 = t1 + t2, z3 = t0 + t2, z4 = t1 + t3;
    const int z5 = (z3 + z4) * 9633;
    t0 *= 2446, t1 *= 16819, t2 *= 25172, t3 *= 12299;
    z1 *= -7373, z2 *= -20995;
    z3 = z3 * -16069 + z5, z4 = z4 * -3196 + z5;
    t0 += z1 + z3, t1 += z2 + z4, t2 += z2 + z3, t3 += z1 + z4;
    constexpr int N = FIRST ? 11 : 18;
    d[0] = jp_descale(t10 + t3, N), d[7] = jp_descale(t10 - t3, N);
    d[1] = jp_descale(t11 + t2, N), d[6] = jp_descale(t11 - t2, N);
    d[2] = jp_descale(t12 + t1, N), d[5] = jp_descale(t12 - t1, N);
    d[3] = jp_descale(t13 + t0, N), d[4] = jp_descale(t13 - t0, N);
}

struct JpYcc {
    int y, cb, cr;
};

__device__ __forceinline__ JpYcc jp_ycc(const unsigned char* px) {
    const int r = px[0], g = px[1], b = px[2];
    JpYcc v;
    v.y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16;
    v.cb = (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16;
    v.cr = (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16;
    return v;
}

// bytes of one frame's planes in the scratch: Hp, Wp are whole MCUs, so every plane starts on an 8-byte boundary
template <int SUB> __host__ __device__ __forceinline__ long jp_frame_bytes(int Hp, int Wp) {
    return SUB == 2 ? (long)Hp * Wp / 2 * 3 : (long)Hp * Wp * 3;
}

// SUB = chroma step per axis: 2 (4:2:0, MCU 16 x 16) or 1 (4:4:4, MCU 8 x 8).  A tile is one MCU row x JP_TILE_W pixels.
// ENC: the encoder's front half (JPEG files out, below).  The kernel stops behind the quantiser and stores what a file
// holds: `planes` then takes int16 coefficients, per frame the blocks of Y row by row, then Cb's, then Cr's, 64 per block in
// zig-zag order, one 16-byte store per lane.
template <int SUB, bool ENC>
__global__ __launch_bounds__(256) void jpeg_planes_kernel(const uint8_t* __restrict__ x, long total,
                                                          const int* __restrict__ quality, uint8_t* __restrict__ planes,
                                                          int H, int W, int Hp, int Wp, int tiles_y, int tiles_x) {
    constexpr int TH = 8 * SUB;
    __shared__ int ws[JP_BLOCKS * JP_BLOCK_LD];
    __shared__ int qt[128];
    __shared__ __align__(16) unsigned char stage[TH * JP_PITCH];

    const int tid = threadIdx.x;
    const int per = tiles_y * tiles_x;
    const long f = blockIdx.x / per;
    const int rem = (int)(blockIdx.x - f * per);
    const int y0 = (rem / tiles_x) * TH, x0 = (rem % tiles_x) * JP_TILE_W;
    const int q = min(quality[f], 100);
    if (q <= 0) return;                                          // the whole workgroup: jpeg_rgb_kernel copies this frame

    if (tid < 128) {
        const int s = q < 50 ? 5000 / q : 200 - 2 * q;
        qt[tid] = min(max((JP_BASE[tid] * s + 50) / 100, 1), 255);
    }
    // the tile's part of the frame (y0 < H and x0 < W: padding adds less than one MCU); pixels past it replicate its edge
    const int rows = min(TH, H - y0), cols = min(JP_TILE_W, W - x0);
    const int rstride = W * 3;
    const int lead0 = u8_stage_rows(x, total, ((f * H + y0) * (long)W + x0) * 3, rstride, rows, cols, stage, JP_PITCH, tid, 256);
    __syncthreads();

    auto pixel = [&](int r, int c) -> const unsigned char* {
        r = min(r, rows - 1);
        return stage + r * JP_PITCH + u8_row_lead(lead0, r, rstride) + min(c, cols - 1) * 3;
    };
    if (SUB == 2) {                                              // one 2 x 2 quad per lane: 8 x 32 quads
        const int qy = tid >> 5, qx = tid & 31;
        // chroma row y0 / 2 + qy of the frame, or the last one the frame has (its two source rows lie in this tile)
        const int cr0 = 2 * min(y0 / 2 + qy, (H + 1) / 2 - 1) - y0;
        int cb = 0, cr = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int dy = j >> 1, dx = j & 1;
            const int ty = 2 * qy + dy, tx = 2 * qx + dx;
            ws[((ty >> 3) * 8 + (tx >> 3)) * JP_BLOCK_LD + (ty & 7) * 8 + (tx & 7)] = jp_ycc(pixel(ty, tx)).y - 128;
            const JpYcc c = jp_ycc(pixel(cr0 + dy, tx));
            cb += c.cb, cr += c.cr;
        }
        const int bias = 1 + (qx & 1);
        const int at = (qx >> 3) * JP_BLOCK_LD + qy * 8 + (qx & 7);
        ws[16 * JP_BLOCK_LD + at] = ((cb + bias) >> 2) - 128;
        ws[20 * JP_BLOCK_LD + at] = ((cr + bias) >> 2) - 128;
    } else {                                                     // 8 x 64 pixels, two per lane
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int p = tid + 256 * j;
            const int ty = p >> 6, tx = p & 63;
            const JpYcc c = jp_ycc(pixel(ty, tx));
            const int at = (tx >> 3) * JP_BLOCK_LD + ty * 8 + (tx & 7);
            ws[at] = c.y - 128;
            ws[8 * JP_BLOCK_LD + at] = c.cb - 128;
            ws[16 * JP_BLOCK_LD + at] = c.cr - 128;
        }
    }
    __syncthreads();

    const int b = tid >> 3, k = tid & 7;                         // block and its row (passes 1, 3) or column (pass 2)
    const bool on = tid < JP_BLOCKS * 8;
    int d[8];
    if (on) {                                                    // forward, rows
        int* row = ws + b * JP_BLOCK_LD + k * 8;
#pragma unroll
        for (int i = 0; i < 8; ++i) d[i] = row[i];
        jp_fdct8<true>(d);
#pragma unroll
        for (int i = 0; i < 8; ++i) row[i] = d[i];
    }
    __syncthreads();
    if (on) {                                                    // forward columns, quantise, multiply back, inverse columns
        int* col = ws + b * JP_BLOCK_LD + k;
        const int* qc = qt + (b < (SUB == 2 ? 16 : 8) ? 0 : 64) + k;
#pragma unroll
        for (int i = 0; i < 8; ++i) d[i] = col[i * 8];
        jp_fdct8<false>(d);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int qv = qc[i * 8];
            const int n = (abs(d[i]) + 4 * qv) / (8 * qv);
            d[i] = (d[i] < 0 ? -n : n) * (ENC ? 1 : qv);
        }
        if (!ENC) jp_idct8<true>(d);
#pragma unroll
        for (int i = 0; i < 8; ++i) col[i * 8] = d[i];
    }
    __syncthreads();
    if (ENC) {                                                   // coefficients 8 k .. 8 k + 7 of the block's zig-zag order
        if (!on) return;
        const int bw = Wp / 8, cw = Wp / (8 * SUB);              // blocks per row of Y / of a chroma plane
        const long ny = (long)bw * (Hp / 8), nc = (long)cw * (Hp / (8 * SUB));
        long at;
        int bcol, lim;
        if (SUB == 2) {
            if (b < 16) bcol = x0 / 8 + (b & 7), lim = bw, at = (long)(y0 / 8 + (b >> 3)) * bw + bcol;
            else bcol = x0 / 16 + ((b - 16) & 3), lim = cw, at = ny + ((b - 16) >> 2) * nc + (long)(y0 / 16) * cw + bcol;
        } else {
            bcol = x0 / 8 + (b & 7), lim = bw, at = (b >> 3) * nc + (long)(y0 / 8) * bw + bcol;
        }
        if (bcol < lim) {                                        // a tile may reach past the last MCU of the row
            const int* blk = ws + b * JP_BLOCK_LD;
            unsigned v[4];
#pragma unroll
            for (int j = 0; j < 4; ++j)
                v[j] = (unsigned)(blk[je_zigzag(8 * k + 2 * j)] & 0xFFFF) | (unsigned)blk[je_zigzag(8 * k + 2 * j + 1)] << 16;
            *reinterpret_cast<uint4*>(planes + ((f * (ny + 2 * nc) + at) * 64 + 8 * k) * 2) = make_uint4(v[0], v[1], v[2], v[3]);
        }
        return;
    }
    if (on) {                                                    // inverse rows -> 8 bytes of a plane
        const int* row = ws + b * JP_BLOCK_LD + k * 8;
#pragma unroll
        for (int i = 0; i < 8; ++i) d[i] = row[i];
        jp_idct8<false>(d);
        int comp, py, px, pw;                                    // component, row and first column in its plane, plane width
        if (SUB == 2) {
            if (b < 16) comp = 0, py = y0 + (b >> 3) * 8 + k, px = x0 + (b & 7) * 8, pw = Wp;
            else comp = 1 + ((b - 16) >> 2), py = y0 / 2 + k, px = x0 / 2 + ((b - 16) & 3) * 8, pw = Wp / 2;
        } else {
            comp = b >> 3, py = y0 + k, px = x0 + (b & 7) * 8, pw = Wp;
        }
        if (px < pw) {                                           // a tile may reach past the last MCU of the row
            const long plane = (long)Hp * Wp;                    // Y; a chroma plane has plane / (SUB * SUB) bytes
            uint8_t* dst = planes + f * jp_frame_bytes<SUB>(Hp, Wp) + (comp ? plane + (comp - 1) * (plane / (SUB * SUB)) : 0) +
                           (long)py * pw + px;
            uint2 v;
            v.x = jp_byte(d[0] + 128) | jp_byte(d[1] + 128) << 8 | jp_byte(d[2] + 128) << 16 | jp_byte(d[3] + 128) << 24;
            v.y = jp_byte(d[4] + 128) | jp_byte(d[5] + 128) << 8 | jp_byte(d[6] + 128) << 16 | jp_byte(d[7] + 128) << 24;
            *reinterpret_cast<uint2*>(dst) = v;
        }
    }
}

// jpeg_planes_kernel<SUB, true> for the two layouts whose MCU is 8 rows high (DESIGN.md "JPEG files out, 4:2:2 and
// greyscale"): GREY = false is 4:2:2, MCUs of 16 x 8 pixels, chroma halved along a row as libjpeg's h2v1_downsample does it,
// (a + b + (chroma column & 1)) >> 1; GREY = true keeps Y alone, MCUs of 8 x 8.  A tile is one MCU row (8 pixel rows) x
// JP_TILE_W pixels: 8 Y blocks, then at 4:2:2 4 Cb and 4 Cr.  Hp, Wp: H, W rounded up to whole MCUs; pixels past the frame
// replicate its edge, so the pair at an odd W's last column averages the last pixel with itself.  -> int16 coefficients,
// per frame the blocks of Y row by row, then Cb's, then Cr's, 64 per block in zig-zag order, one 16-byte store per lane.
template <bool GREY>
__global__ __launch_bounds__(256) void jpeg_coef_kernel(const uint8_t* __restrict__ x, long total, const int* __restrict__ quality,
                                                        uint8_t* __restrict__ coef, int H, int W, int Hp, int Wp, int tiles_y,
                                                        int tiles_x) {
    constexpr int NB = GREY ? 8 : 16;                            // live blocks of a tile
    __shared__ int ws[NB * JP_BLOCK_LD];
    __shared__ int qt[128];
    __shared__ __align__(16) unsigned char stage[8 * JP_PITCH];

    const int tid = threadIdx.x;
    const int per = tiles_y * tiles_x;
    const long f = blockIdx.x / per;
    const int rem = (int)(blockIdx.x - f * per);
    const int y0 = (rem / tiles_x) * 8, x0 = (rem % tiles_x) * JP_TILE_W;
    const int q = min(quality[f], 100);
    if (q <= 0) return;                                          // the whole workgroup: no coefficients, an empty file

    if (tid < 128) {
        const int s = q < 50 ? 5000 / q : 200 - 2 * q;
        qt[tid] = min(max((JP_BASE[tid] * s + 50) / 100, 1), 255);
    }
    // the tile's part of the frame (y0 < H and x0 < W: padding adds less than one MCU); pixels past it replicate its edge
    const int rows = min(8, H - y0), cols = min(JP_TILE_W, W - x0);
    const int rstride = W * 3;
    const int lead0 = u8_stage_rows(x, total, ((f * H + y0) * (long)W + x0) * 3, rstride, rows, cols, stage, JP_PITCH, tid, 256);
    __syncthreads();

    auto pixel = [&](int r, int c) -> const unsigned char* {
        r = min(r, rows - 1);
        return stage + r * JP_PITCH + u8_row_lead(lead0, r, rstride) + min(c, cols - 1) * 3;
    };
    if (GREY) {                                                  // 8 x 64 pixels, two per lane
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int p = tid + 256 * j;
            const int ty = p >> 6, tx = p & 63;
            ws[(tx >> 3) * JP_BLOCK_LD + ty * 8 + (tx & 7)] = jp_ycc(pixel(ty, tx)).y - 128;
        }
    } else {                                                     // one horizontal pair per lane: 8 x 32 pairs
        const int ty = tid >> 5, px = tid & 31;
        const JpYcc a = jp_ycc(pixel(ty, 2 * px)), b = jp_ycc(pixel(ty, 2 * px + 1));
        const int at = (px >> 2) * JP_BLOCK_LD + ty * 8 + 2 * (px & 3);
        ws[at] = a.y - 128;
        ws[at + 1] = b.y - 128;
        const int bias = px & 1;                                 // x0 / 2 is even: the chroma column's parity is the lane's
        const int cat = (8 + (px >> 3)) * JP_BLOCK_LD + ty * 8 + (px & 7);
        ws[cat] = ((a.cb + b.cb + bias) >> 1) - 128;
        ws[cat + 4 * JP_BLOCK_LD] = ((a.cr + b.cr + bias) >> 1) - 128;
    }
    __syncthreads();

    const int b = tid >> 3, k = tid & 7;                         // block and its row (first pass) or column (second)
    const bool on = tid < NB * 8;
    int d[8];
    if (on) {                                                    // forward, rows
        int* row = ws + b * JP_BLOCK_LD + k * 8;
#pragma unroll
        for (int i = 0; i < 8; ++i) d[i] = row[i];
        jp_fdct8<true>(d);
#pragma unroll
        for (int i = 0; i < 8; ++i) row[i] = d[i];
    }
    __syncthreads();
    if (on) {                                                    // forward columns, quantise
        int* col = ws + b * JP_BLOCK_LD + k;
        const int* qc = qt + (b < 8 ? 0 : 64) + k;
#pragma unroll
        for (int i = 0; i < 8; ++i) d[i] = col[i * 8];
        jp_fdct8<false>(d);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int qv = qc[i * 8];
            const int n = (abs(d[i]) + 4 * qv) / (8 * qv);
            col[i * 8] = d[i] < 0 ? -n : n;
        }
    }
    __syncthreads();
    if (!on) return;
    const int bw = Wp / 8, cw = Wp / 16;                         // blocks per row of Y / of a 4:2:2 chroma plane
    const long ny = (long)bw * (Hp / 8), nc = GREY ? 0 : (long)cw * (Hp / 8);
    long at;
    int bcol, lim;
    if (b < 8) bcol = x0 / 8 + b, lim = bw, at = (long)(y0 / 8) * bw + bcol;
    else bcol = x0 / 16 + ((b - 8) & 3), lim = cw, at = ny + ((b - 8) >> 2) * nc + (long)(y0 / 8) * cw + bcol;
    if (bcol < lim) {                                            // a tile may reach past the last MCU of the row
        const int* blk = ws + b * JP_BLOCK_LD;
        unsigned v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j)
            v[j] = (unsigned)(blk[je_zigzag(8 * k + 2 * j)] & 0xFFFF) | (unsigned)blk[je_zigzag(8 * k + 2 * j + 1)] << 16;
        *reinterpret_cast<uint4*>(coef + ((f * (ny + 2 * nc) + at) * 64 + 8 * k) * 2) = make_uint4(v[0], v[1], v[2], v[3]);
    }
}

// chroma at pixel (y, x) of the frame from a plane of the frame's Hc x Wc samples (row pitch pw)
template <int SUB> __device__ __forceinline__ int jp_chroma(const uint8_t* __restrict__ c, int pw, int Hc, int Wc, int y, int x) {
    if (SUB == 1) return c[(long)y * pw + x];
    const int cy = y >> 1, cx = x >> 1;
    const uint8_t* near = c + (long)cy * pw;
    const uint8_t* far = c + (long)min(max(cy + (y & 1) * 2 - 1, 0), Hc - 1) * pw;
    const int ox = min(max(cx + (x & 1) * 2 - 1, 0), Wc - 1);
    return (3 * (3 * near[cx] + far[cx]) + 3 * near[ox] + far[ox] + 8 - (x & 1)) >> 4;
}

// the same at 4:2:2, where the plane has the frame's H x Wc samples and only the columns are interpolated (libjpeg's h2v1
// "fancy" triangle): 3/4 of the nearer and 1/4 of the farther sample of row y, + 1 (even columns) or + 2 (odd ones), >> 2
__device__ __forceinline__ int jp_chroma_h2v1(const uint8_t* __restrict__ c, int pw, int Wc, int y, int x) {
    const int cx = x >> 1;
    const uint8_t* near = c + (long)y * pw;
    const int ox = min(max(cx + (x & 1) * 2 - 1, 0), Wc - 1);
    return (3 * near[cx] + near[ox] + 1 + (x & 1)) >> 2;
}

// 4 consecutive pixels of the batch per lane; out4 = the output may be written as dwords
template <int SUB>
__global__ __launch_bounds__(256) void jpeg_rgb_kernel(const uint8_t* __restrict__ x, const int* __restrict__ quality,
                                                       const uint8_t* __restrict__ planes, uint8_t* __restrict__ out, long npix,
                                                       int H, int W, int Hp, int Wp, int out4) {
    const long p0 = ((long)blockIdx.x * 256 + threadIdx.x) * 4;
    if (p0 >= npix) return;
    const long hw = (long)H * W;
    long f = p0 / hw;
    int rest = (int)(p0 - f * hw);
    int y = rest / W, xx = rest - y * W;
    const long plane = (long)Hp * Wp, cplane = plane / (SUB * SUB);
    const int pw = Wp / SUB, Hc = (H + SUB - 1) / SUB, Wc = (W + SUB - 1) / SUB;
    unsigned char o[12];
    const int cnt = (int)min(4L, npix - p0);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (j < cnt) {
            const long g = (p0 + j) * 3;
            if (quality[f] <= 0) {
                o[3 * j] = x[g], o[3 * j + 1] = x[g + 1], o[3 * j + 2] = x[g + 2];
            } else {
                const uint8_t* fp = planes + f * jp_frame_bytes<SUB>(Hp, Wp);
                const int yv = fp[(long)y * Wp + xx];
                const int cb = jp_chroma<SUB>(fp + plane, pw, Hc, Wc, y, xx) - 128;
                const int cr = jp_chroma<SUB>(fp + plane + cplane, pw, Hc, Wc, y, xx) - 128;
                o[3 * j] = (unsigned char)jp_byte(yv + ((91881 * cr + 32768) >> 16));
                o[3 * j + 1] = (unsigned char)jp_byte(yv + ((-22554 * cb - 46802 * cr + 32768) >> 16));
                o[3 * j + 2] = (unsigned char)jp_byte(yv + ((116130 * cb + 32768) >> 16));
            }
            if (++xx == W) {
                xx = 0;
                if (++y == H) y = 0, ++f;
            }
        } else {
            o[3 * j] = o[3 * j + 1] = o[3 * j + 2] = 0;
        }
    }
    uint8_t* dst = out + p0 * 3;
    if (out4 && cnt == 4) {
        unsigned* d4 = reinterpret_cast<unsigned*>(dst);
#pragma unroll
        for (int j = 0; j < 3; ++j) d4[j] = o[4 * j] | o[4 * j + 1] << 8 | o[4 * j + 2] << 16 | (unsigned)o[4 * j + 3] << 24;
    } else {
#pragma unroll
        for (int j = 0; j < 12; ++j)
            if (j < 3 * cnt) dst[j] = o[j];
    }
}

template <int SUB>
int jpeg_launch(const uint8_t* x, long total, int n, int H, int W, const int* quality, uint8_t* scratch, long scratch_bytes,
                uint8_t* out, hipStream_t stream) {
    constexpr int MCU = 8 * SUB;
    const int Hp = (H + MCU - 1) / MCU * MCU, Wp = (W + MCU - 1) / MCU * MCU;
    if (scratch_bytes < n * jp_frame_bytes<SUB>(Hp, Wp)) return ISTVT_ERR_SHAPE;
    const int tiles_y = Hp / MCU, tiles_x = (Wp + JP_TILE_W - 1) / JP_TILE_W;
    const long tiles = (long)n * tiles_y * tiles_x;
    const long npix = (long)n * H * W;
    const long groups = (npix + 1023) / 1024;
    if (tiles > 0x7fffffffL || groups > 0x7fffffffL) return ISTVT_ERR_SHAPE;
    hipLaunchKernelGGL((jpeg_planes_kernel<SUB, false>), dim3((unsigned)tiles), dim3(256), 0, stream, x, total, quality, scratch, H, W,
                       Hp, Wp, tiles_y, tiles_x);
    int rc = istvt_check_launch();
    if (rc != ISTVT_OK) return rc;
    hipLaunchKernelGGL(jpeg_rgb_kernel<SUB>, dim3((unsigned)groups), dim3(256), 0, stream, x, quality, scratch, out, npix, H, W,
                       Hp, Wp, (int)((reinterpret_cast<uintptr_t>(out) & 3) == 0));
    return istvt_check_launch();
}

}  // namespace

// frames uint8 [n][H][W][3] (total bytes readable at frames; no alignment needed), quality int32 [n] on the device (1..100
// compress, larger counts as 100, <= 0 copies the frame), subsampling 2 (4:2:0) or 0 (4:4:4) as JPEG libraries number them
// -> out uint8 [n][H][W][3], which must not overlap frames.  scratch: the planes, 8-byte aligned, n * Hp * Wp * 3 / 2 bytes
// at 4:2:0 and n * Hp * Wp * 3 at 4:4:4 with Hp, Wp = H, W rounded up to multiples of 16 / 8.
extern "C" int istvt_jpeg_roundtrip_u8(const void* frames, long total, int n, int H, int W, const int* quality,
                                       int subsampling, void* scratch, long scratch_bytes, void* out, hipStream_t stream) {
    if (n <= 0 || !frames || !quality || !scratch || !out) return ISTVT_ERR_SHAPE;
    if (H < 1 || W < 1 || H > 16384 || W > 16384) return ISTVT_ERR_SHAPE;
    if (subsampling != 0 && subsampling != 2) return ISTVT_ERR_SHAPE;
    const long bytes = (long)n * H * W * 3;
    if (total < bytes || (reinterpret_cast<uintptr_t>(scratch) & 7)) return ISTVT_ERR_SHAPE;
    const uint8_t* a = (const uint8_t*)frames;
    const uint8_t* o = (const uint8_t*)out;
    if (o < a + bytes && a < o + bytes) return ISTVT_ERR_SHAPE;              // in place: the upsample reads its neighbours
    if (subsampling == 2) return jpeg_launch<2>(a, total, n, H, W, quality, (uint8_t*)scratch, scratch_bytes, (uint8_t*)out, stream);
    return jpeg_launch<1>(a, total, n, H, W, quality, (uint8_t*)scratch, scratch_bytes, (uint8_t*)out, stream);
}

// ---- JPEG files ----------------------------------------------------------------------------------------------------------
// A row of the per-image table (clips.JpegBatch.images) and of the per-segment table
enum { JD_H = 0, JD_W, JD_SUB, JD_MCUX, JD_MCUY, JD_QUANT, JD_HUFF = 8, JD_BLOCK0 = 14, JD_GROUP0, JD_SEG0, JD_NSEG, JD_NBLOCKS,
       JD_LAYOUT };
constexpr int JD_IMAGE_INTS = ISTVT_JPEG_IMAGE_INTS;
constexpr int JD_SEGMENT_INTS = ISTVT_JPEG_SEGMENT_INTS;  // image, first byte, end byte, first MCU, MCUs
// the scratch, for B blocks in the batch and s segments: int16 coefficients [B][64] | planes, 64 B bytes, per image Y
// [Hp][Wp], Cb, Cr [Hp / v][Wp / h] as the round trip lays them out (h, v: the luma blocks of an MCU per axis, JeLayout; no
// Cb, Cr for greyscale) | int32 status [s]
constexpr long JD_BLOCK_BYTES = 128 + 64;

namespace {

__host__ __device__ __forceinline__ JeLayout jd_layout(const int* im) { return je_layout(im[JD_LAYOUT], im[JD_SUB]); }

// where the entropy decoder puts the blocks of one image: int16 [block][64] in natural order
struct JdWriter {
    short* coef;
    long block0, total;                     // the image's first block; blocks of the batch
    int ybw, cbw, ny, nc;                   // blocks per row of Y / of a chroma plane; blocks of Y / of a chroma plane
    __host__ __device__ long block(int c, int row, int col) const {
        const long b = block0 + (c == 0 ? (long)row * ybw + col : ny + (long)(c - 1) * nc + (long)row * cbw + col);
        return b >= 0 && b < total ? b : -1;
    }
    __host__ __device__ void clear(long b) const {
        if (b < 0) return;
        uint4* p = reinterpret_cast<uint4*>(coef + b * 64);
#pragma unroll
        for (int i = 0; i < 8; ++i) p[i] = make_uint4(0u, 0u, 0u, 0u);
    }
    __host__ __device__ void put(long b, int at, int v) const {
        if (b >= 0) coef[b * 64 + at] = (short)v;
    }
};

// One lane per restart interval.  The entry has checked the host copies of both tables; the comparisons here keep a device
// table that differs from them inside the buffers all the same (its segment then reports status 2).
__global__ __launch_bounds__(64) void jpeg_entropy_kernel(const uint8_t* __restrict__ bytes, long nbytes,
                                                          const int* __restrict__ images, int n,
                                                          const int* __restrict__ segments, int nseg,
                                                          const int* __restrict__ htabs, int nh, short* __restrict__ coef,
                                                          long total_blocks, int* __restrict__ seg_status) {
    const int s = blockIdx.x * 64 + threadIdx.x;
    if (s >= nseg) return;
    const int* sg = segments + (long)s * JD_SEGMENT_INTS;
    const int img = sg[0], first = sg[3], count = sg[4];
    const long begin = sg[1], end = sg[2];
    int ok = img >= 0 && img < n && begin >= 0 && begin <= end && end <= nbytes && first >= 0 && count >= 0;
    const int* im = images + (long)(ok ? img : 0) * JD_IMAGE_INTS;
    const JeLayout lay = jd_layout(im);
    const int mcux = max(im[JD_MCUX], 1), mcuy = max(im[JD_MCUY], 1);
    ok = ok && (long)first + count <= (long)mcux * mcuy;
    const int* huff[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        const int slot = im[JD_HUFF + k];
        ok = ok && slot >= 0 && slot < nh;
        huff[k] = htabs + (long)(ok ? slot : 0) * JE_HUFF_INTS;
    }
    if (!ok) {
        seg_status[s] = 2;
        return;
    }
    const JdWriter w = {coef, (long)im[JD_BLOCK0], total_blocks, mcux * lay.h, mcux, mcux * lay.h * mcuy * lay.v, mcux * mcuy};
    seg_status[s] = je_decode_segment(bytes, begin, end, huff, lay, mcux, first, count, w);
}

// The state rows of the split path (js_chunk_bytes, js_chunks: the chunk rule): js_row0 says where those of segment s lie in
// the table behind the statuses, by the segment's byte offset (the batch call: a table of nbytes / chunk_bytes + nseg rows) or
// at a stride per segment (the bank's calls: segment s owns rows [s * R, (s + 1) * R)).
constexpr int JS_STATE_INTS = ISTVT_JPEG_STATE_INTS;

// One workgroup per restart interval, one lane per chunk (jpeg_entropy_split.h).  All lanes clear the interval's blocks;
// the lanes relax their entry states until no exit state changes, at most S - 1 rounds; the tallies of the last transition
// are scanned into each lane's first block and DC predictions; the lanes up to the first that met an error decode once more
// with stores.  The barriers of the rounds lie between the clears and every put.  A state row: entry pos, bit, blk, k,
// blocks started, first block, status of the lane's decode, rounds in which a state changed.  LANES: the workgroup's size,
// 256, or 64 where no interval of the batch has more chunks than that (the entry knows from the host table, or from the
// bank's row stride).  STRIDED: the row addressing; `nrows` is then the row stride R, not the table's size, and an interval of
// more than R chunks is refused with status 2 like one that fails the other comparisons: nothing of it is written.
template <int LANES, bool STRIDED>
__global__ __launch_bounds__(LANES) void jpeg_entropy_split_kernel(const uint8_t* __restrict__ bytes, long nbytes,
                                                                   const int* __restrict__ images, int n,
                                                                   const int* __restrict__ segments, int nseg,
                                                                   const int* __restrict__ htabs, int nh,
                                                                   short* __restrict__ coef, long total_blocks,
                                                                   int* __restrict__ seg_status, int* __restrict__ rows,
                                                                   long nrows, int chunk_bytes) {
    __shared__ int sh_pos[LANES], sh_pk[LANES];
    __shared__ int sh_scan[2][4][LANES];
    __shared__ int sh_dead, sh_status;
    const int s = blockIdx.x, tid = threadIdx.x;
    const int* sg = segments + (long)s * JD_SEGMENT_INTS;
    const int img = sg[0], first = sg[3], count = sg[4];
    const long begin = sg[1], end = sg[2];
    int ok = img >= 0 && img < n && begin >= 0 && begin <= end && end <= nbytes && first >= 0 && count >= 0;
    const int* im = images + (long)(ok ? img : 0) * JD_IMAGE_INTS;
    const JeLayout lay = jd_layout(im);
    const int mcux = max(im[JD_MCUX], 1), mcuy = max(im[JD_MCUY], 1);
    ok = ok && (long)first + count <= (long)mcux * mcuy;
    const int* huff[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        const int slot = im[JD_HUFF + k];
        ok = ok && slot >= 0 && slot < nh;
        huff[k] = htabs + (long)(ok ? slot : 0) * JE_HUFF_INTS;
    }
    const long chunk = ok ? js_chunk_bytes(end - begin, chunk_bytes) : chunk_bytes;
    const int S = ok ? js_chunks(end - begin, chunk_bytes) : 1;
    const long row0 = js_row0<STRIDED>(begin, chunk_bytes, s, S, nrows);
    ok = ok && S <= LANES && row0 >= 0;
    if (!ok) {                                                   // the same for every lane of the workgroup
        if (tid == 0) seg_status[s] = 2;
        return;
    }
    const JdWriter w = {coef, (long)im[JD_BLOCK0], total_blocks, mcux * lay.h, mcux, mcux * lay.h * mcuy * lay.v, mcux * mcuy};
    const long total = (long)count * js_mcu_blocks(lay);         // blocks of the interval
    for (long at = tid; at < total * 8; at += LANES) {           // a lane clears 16 bytes at a time
        int c;
        const long b = js_place(lay, mcux, first, at >> 3, w, c);
        if (b >= 0) reinterpret_cast<uint4*>(coef + b * 64)[at & 7] = make_uint4(0u, 0u, 0u, 0u);
    }
    if (tid == 0) sh_dead = JS_LANES, sh_status = 0;

    const bool lane = tid < S, inner = tid < S - 1;              // inner: a lane whose exit state another lane reads
    const long limit = begin + (long)(tid + 1) * chunk;          // <= end for an inner lane
    JsState in = {begin, 0, 0, 0}, out = in;
    JsTally t = {0, 0, {0, 0, 0}};
    if (lane && tid > 0) in = js_guess(bytes, begin, end, begin + (long)tid * chunk);
    if (inner) out = js_chunk(bytes, end, limit, huff, lay, in, t);
    sh_pos[tid] = (int)out.pos, sh_pk[tid] = out.bit | out.blk << 3 | out.k << 6;
    __syncthreads();
    int rounds = 0;
    for (int r = 1; r < S; ++r) {                                // S is the workgroup's: every lane takes the same trips
        JsState nin = in;
        if (lane && tid > 0) {
            const int pk = sh_pk[tid - 1];
            nin.pos = sh_pos[tid - 1], nin.bit = pk & 7, nin.blk = (pk >> 3) & 7, nin.k = pk >> 6;
        }
        __syncthreads();                                         // every exit state of the last round is read
        int changed = 0;
        if (!js_same(nin, in)) {
            in = nin;
            if (inner) {
                const JsState o = js_chunk(bytes, end, limit, huff, lay, in, t);
                changed = !js_same(o, out);
                out = o;
                sh_pos[tid] = (int)out.pos, sh_pk[tid] = out.bit | out.blk << 3 | out.k << 6;
            }
        }
        if (!__syncthreads_or(changed)) break;
        ++rounds;
    }

    // each lane's first block and predictions: an inclusive scan of the inner lanes' tallies, read one lane to the left
    int v[4] = {inner ? t.blocks : 0, inner ? t.pred[0] : 0, inner ? t.pred[1] : 0, inner ? t.pred[2] : 0};
    if (inner && t.err) atomicMin(&sh_dead, tid);
    int side = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) sh_scan[0][q][tid] = v[q];
    __syncthreads();
    for (int d = 1; d < S; d <<= 1) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            if (tid >= d) v[q] += sh_scan[side][q][tid - d];
            sh_scan[side ^ 1][q][tid] = v[q];
        }
        side ^= 1;
        __syncthreads();
    }
    long next = 0;
    int pred[3] = {0, 0, 0};
    if (tid > 0) {
        next = sh_scan[side][0][tid - 1];
#pragma unroll
        for (int q = 0; q < 3; ++q) pred[q] = (int16_t)sh_scan[side][1 + q][tid - 1];
    }
    int started = 0, st = 0;
    if (lane && tid <= sh_dead) {
        st = js_write(bytes, end, limit, tid == S - 1, huff, lay, mcux, first, total, in, next, pred, w, started);
        if (st) atomicMax(&sh_status, st);
    }
    if (lane) {
        int* row = rows + (row0 + tid) * JS_STATE_INTS;
        row[0] = (int)in.pos, row[1] = in.bit, row[2] = in.blk, row[3] = in.k;
        row[4] = started, row[5] = (int)min(next, total), row[6] = st, row[7] = rounds;
    }
    __syncthreads();
    if (tid == 0) seg_status[s] = sh_status;
}

// The back half of jpeg_planes_kernel on decoded coefficients: a workgroup takes JP_BLOCKS consecutive blocks of one image,
// a lane one 8-point transform of each pass: times the image's table and inverse columns | inverse rows, + 128, clamp, one
// 8-byte store.  The first workgroup of an image also writes its size and the largest status of its segments.
__global__ __launch_bounds__(256) void jpeg_idct_kernel(const short* __restrict__ coef, const int* __restrict__ images, int n,
                                                        const int* __restrict__ qtabs, int nq,
                                                        const int* __restrict__ seg_status, int nseg,
                                                        uint8_t* __restrict__ planes, int* __restrict__ sizes,
                                                        int* __restrict__ status) {
    __shared__ int ws[JP_BLOCKS * JP_BLOCK_LD];
    __shared__ int qt[3 * 64];
    __shared__ int worst;
    const int tid = threadIdx.x, g = blockIdx.x;
    int lo = 0, hi = n - 1;                                      // the last image whose first workgroup is <= g
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (images[(long)mid * JD_IMAGE_INTS + JD_GROUP0] <= g) lo = mid;
        else hi = mid - 1;
    }
    const int* im = images + (long)lo * JD_IMAGE_INTS;
    const JeLayout lay = jd_layout(im);
    const int mcux = im[JD_MCUX], mcuy = im[JD_MCUY];
    const int ybw = mcux * lay.h, ny = ybw * mcuy * lay.v, nc = mcux * mcuy, nb = ny + lay.nc * nc;
    const long block0 = im[JD_BLOCK0];
    const int local0 = (g - im[JD_GROUP0]) * JP_BLOCKS;
    if (tid < 192) {
        const int slot = im[JD_QUANT + (tid >> 6)];
        qt[tid] = slot >= 0 && slot < nq ? qtabs[(long)slot * 64 + (tid & 63)] : 1;
    }
    if (tid == 0) worst = 0;
    __syncthreads();
    if (local0 == 0) {
        int m = 0;
        for (int s = tid; s < im[JD_NSEG]; s += 256) {
            const long at = (long)im[JD_SEG0] + s;
            if (at >= 0 && at < nseg) m = max(m, seg_status[at]);
        }
        if (m) atomicMax(&worst, m);
    }

    const int b = tid >> 3, k = tid & 7;                         // block and its column (first pass) or row (second)
    const int bi = local0 + b;
    const bool on = tid < JP_BLOCKS * 8 && bi < nb;
    const int comp = bi < ny ? 0 : bi < ny + nc ? 1 : 2;
    int d[8];
    if (on) {
        const short* src = coef + (block0 + bi) * 64 + k;
        const int* q = qt + comp * 64 + k;
#pragma unroll
        for (int i = 0; i < 8; ++i) d[i] = src[i * 8] * q[i * 8];
        jp_idct8<true>(d);
        int* col = ws + b * JP_BLOCK_LD + k;
#pragma unroll
        for (int i = 0; i < 8; ++i) col[i * 8] = d[i];
    }
    __syncthreads();
    if (on) {
        const int* row = ws + b * JP_BLOCK_LD + k * 8;
#pragma unroll
        for (int i = 0; i < 8; ++i) d[i] = row[i];
        jp_idct8<false>(d);
        const int c = comp ? bi - ny - (comp - 1) * nc : bi;     // the block's number in its plane
        const int bw = comp ? mcux : ybw, brow = c / bw, bcol = c - brow * bw;
        uint8_t* dst = planes + block0 * 64 + (comp ? (long)ny * 64 + (long)(comp - 1) * nc * 64 : 0) +
                       (long)(brow * 8 + k) * (bw * 8) + bcol * 8;
        uint2 v;
        v.x = jp_byte(d[0] + 128) | jp_byte(d[1] + 128) << 8 | jp_byte(d[2] + 128) << 16 | jp_byte(d[3] + 128) << 24;
        v.y = jp_byte(d[4] + 128) | jp_byte(d[5] + 128) << 8 | jp_byte(d[6] + 128) << 16 | jp_byte(d[7] + 128) << 24;
        *reinterpret_cast<uint2*>(dst) = v;
    }
    if (local0 == 0 && tid == 0) {                               // `worst` is complete since the barrier between the passes
        status[lo] = worst;
        sizes[2 * lo] = im[JD_H], sizes[2 * lo + 1] = im[JD_W];
    }
}

// jpeg_rgb_kernel over a canvas [n][Hc][Wc][3]: 4 consecutive pixels of the canvas per lane; inside its image's H x W a pixel
// is the upsampled, converted sample, outside it is 0, so every byte of the canvas is written
__global__ __launch_bounds__(256) void jpeg_canvas_kernel(const int* __restrict__ images, const uint8_t* __restrict__ planes,
                                                          uint8_t* __restrict__ out, long npix, int Hc, int Wc, int out4) {
    const long p0 = ((long)blockIdx.x * 256 + threadIdx.x) * 4;
    if (p0 >= npix) return;
    const long hw = (long)Hc * Wc;
    long f = p0 / hw;
    const int rest = (int)(p0 - f * hw);
    int y = rest / Wc, xx = rest - y * Wc;
    unsigned char o[12];
    const int cnt = (int)min(4L, npix - p0);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        o[3 * j] = o[3 * j + 1] = o[3 * j + 2] = 0;
        if (j < cnt) {
            const int* im = images + f * JD_IMAGE_INTS;
            const int H = im[JD_H], W = im[JD_W];
            if (y < H && xx < W) {
                const JeLayout lay = jd_layout(im);
                const int pw = im[JD_MCUX] * 8, Wp = pw * lay.h, Hp = im[JD_MCUY] * 8 * lay.v;
                const long plane = (long)Hp * Wp, cplane = (long)im[JD_MCUY] * 8 * pw;
                const int Hs = (H + lay.v - 1) / lay.v, Ws = (W + lay.h - 1) / lay.h;
                const uint8_t* fp = planes + (long)im[JD_BLOCK0] * 64;
                const int yv = fp[(long)y * Wp + xx];
                int cb = 0, cr = 0;                               // greyscale: no chroma is read, R = G = B = Y
                if (lay.nc != 0 && lay.v == 2) {
                    cb = jp_chroma<2>(fp + plane, pw, Hs, Ws, y, xx) - 128;
                    cr = jp_chroma<2>(fp + plane + cplane, pw, Hs, Ws, y, xx) - 128;
                } else if (lay.nc != 0 && lay.h == 2) {
                    cb = jp_chroma_h2v1(fp + plane, pw, Ws, y, xx) - 128;
                    cr = jp_chroma_h2v1(fp + plane + cplane, pw, Ws, y, xx) - 128;
                } else if (lay.nc != 0) {
                    cb = jp_chroma<1>(fp + plane, pw, Hs, Ws, y, xx) - 128;
                    cr = jp_chroma<1>(fp + plane + cplane, pw, Hs, Ws, y, xx) - 128;
                }
                o[3 * j] = (unsigned char)jp_byte(yv + ((91881 * cr + 32768) >> 16));
                o[3 * j + 1] = (unsigned char)jp_byte(yv + ((-22554 * cb - 46802 * cr + 32768) >> 16));
                o[3 * j + 2] = (unsigned char)jp_byte(yv + ((116130 * cb + 32768) >> 16));
            }
            if (++xx == Wc) {
                xx = 0;
                if (++y == Hc) y = 0, ++f;
            }
        }
    }
    uint8_t* dst = out + p0 * 3;
    if (out4 && cnt == 4) {
        unsigned* d4 = reinterpret_cast<unsigned*>(dst);
#pragma unroll
        for (int j = 0; j < 3; ++j) d4[j] = o[4 * j] | o[4 * j + 1] << 8 | o[4 * j + 2] << 16 | (unsigned)o[4 * j + 3] << 24;
    } else {
#pragma unroll
        for (int j = 0; j < 12; ++j)
            if (j < 3 * cnt) dst[j] = o[j];
    }
}

// the host copies of the two tables against the counts, the byte range, the canvas and each other -> blocks of the batch, or -1
long jpeg_decode_check(const istvt_jpeg_decode_args* a, long* groups) {
    long blocks = 0, grp = 0, seg = 0;
    for (int i = 0; i < a->n; ++i) {
        const int* im = a->images_host + (long)i * JD_IMAGE_INTS;
        const int H = im[JD_H], W = im[JD_W], sub = im[JD_SUB], code = im[JD_LAYOUT];
        if (H < 1 || W < 1 || H > 16384 || W > 16384 || H > a->Hc || W > a->Wc || (sub != 1 && sub != 2)) return -1;
        if (code != 0 && !(code == ISTVT_JPEG_LAYOUT_422 && sub == 2) && !(code == ISTVT_JPEG_LAYOUT_GREY && sub == 1)) return -1;
        const JeLayout lay = je_layout(code, sub);               // the MCU is 8 h x 8 v pixels
        const int mcux = (W + 8 * lay.h - 1) / (8 * lay.h), mcuy = (H + 8 * lay.v - 1) / (8 * lay.v);
        if (im[JD_MCUX] != mcux || im[JD_MCUY] != mcuy) return -1;
        for (int c = 0; c < 3; ++c)
            if (im[JD_QUANT + c] < 0 || im[JD_QUANT + c] >= a->nq) return -1;
        for (int k = 0; k < 6; ++k)
            if (im[JD_HUFF + k] < 0 || im[JD_HUFF + k] >= a->nh) return -1;
        const long mcus = (long)mcux * mcuy, nb = mcus * js_mcu_blocks(lay);
        if (im[JD_BLOCK0] != blocks || im[JD_GROUP0] != grp || im[JD_SEG0] != seg || im[JD_NBLOCKS] != nb) return -1;
        if (im[JD_NSEG] < 1 || seg + im[JD_NSEG] > a->nseg) return -1;
        long mcu = 0;
        for (int s = 0; s < im[JD_NSEG]; ++s) {
            const int* sg = a->segments_host + (seg + s) * JD_SEGMENT_INTS;
            if (sg[0] != i || sg[1] < 0 || sg[1] > sg[2] || sg[2] > a->nbytes || sg[3] != mcu || sg[4] < 1) return -1;
            mcu += sg[4];
        }
        if (mcu != mcus) return -1;
        seg += im[JD_NSEG];
        blocks += nb;
        grp += (nb + JP_BLOCKS - 1) / JP_BLOCKS;
        if (blocks > 0x7fffffffL / 64) return -1;                 // block0 * 64 and the group count stay ints
    }
    if (seg != a->nseg) return -1;
    *groups = grp;
    return blocks;
}

// ---- what the four decode entries share: they check, lay the scratch out, (plan,) decode the entropy, finish ------------------
// The argument checks: the block, its pointers, the counts, the canvas -> blocks of the batch, or -1.  A direct call names
// host copies of both tables, which jpeg_decode_check reads.  A bank's call (bank: the largest image Hmax x Wmax lies against
// the canvas) checks scalars alone -- the bank's tables were checked when it was built -- and reads images_host as the index,
// on the device; segments_host is not used, nbytes stays an int, and the blocks follow from the entry's own scalars: 0 here.
long jd_args_check(const istvt_jpeg_decode_args* a, bool bank, int Hmax, int Wmax, long* groups) {
    if (!a || a->n <= 0 || a->nq <= 0 || a->nh <= 0 || a->nbytes < 0) return -1;
    if (bank ? a->nseg <= 0 || a->nbytes > 0x7fffffffL : a->nseg < a->n) return -1;
    if (!a->bytes || !a->images || !a->images_host || !a->segments || (!bank && !a->segments_host) || !a->qtabs || !a->htabs ||
        !a->scratch || !a->out || !a->sizes || !a->status)
        return -1;
    if (Hmax < 1 || Wmax < 1 || a->Hc < Hmax || a->Wc < Wmax || a->Hc > 16384 || a->Wc > 16384) return -1;
    return bank ? 0 : jpeg_decode_check(a, groups);
}

// The scratch of a call (the layout above JD_BLOCK_BYTES) and what follows it: for a bank's m places of seg_max segment rows,
// from the next multiple of 16 bytes, the planned images and segments; for the split kernel, from the next multiple of 16
// bytes again, nrows state rows.  clips.py and tools/jpeg_bank_split_check.cpp compute the same offsets.
struct JdScratch {
    short* coef;
    uint8_t* planes;
    int *seg_status, *images, *segments, *rows;                  // images, segments: planned (m > 0); rows: the states (nrows > 0)
};

// -> whether the caller's scratch is aligned and holds the layout for `words` status words
bool jd_scratch(const istvt_jpeg_decode_args* a, long blocks, long words, long m, long seg_max, long nrows, JdScratch& s) {
    uint8_t* base = (uint8_t*)a->scratch;
    long at = blocks * JD_BLOCK_BYTES + 4 * words;
    s.coef = (short*)base, s.planes = base + blocks * 128, s.seg_status = (int*)(base + blocks * JD_BLOCK_BYTES);
    s.images = s.segments = s.rows = nullptr;
    if (m > 0) {
        at = (at + 15) & ~15L;
        s.images = (int*)(base + at), s.segments = s.images + m * JD_IMAGE_INTS;
        at += 4 * m * JD_IMAGE_INTS + 4 * m * seg_max * JD_SEGMENT_INTS;
    }
    if (nrows > 0) {
        at = (at + 15) & ~15L;
        s.rows = (int*)(base + at);
        at += nrows * JS_STATE_INTS * 4;
    }
    return (reinterpret_cast<uintptr_t>(base) & 15) == 0 && a->scratch_bytes >= at;
}

// The output side, a canvas of n images: its pixels, which the colour kernel takes 1024 per workgroup, and `out` clear of
// the bytes the call reads
bool jd_out_ok(const istvt_jpeg_decode_args* a, long n, long& npix) {
    npix = n * a->Hc * a->Wc;
    const uint8_t *src = (const uint8_t*)a->bytes, *out = (const uint8_t*)a->out;
    return (npix + 1023) / 1024 <= 0x7fffffffL && !(out < src + a->nbytes && src < out + npix * 3);
}

// The entropy stage on the tables (images [n], segments [nseg]): one lane per segment, or where the scratch has state rows
// the split kernel, in workgroups of 64 where no segment has more chunks (`most`) and of JS_LANES elsewhere.  STRIDED, nrows:
// how the rows are addressed (jpeg_entropy_split_kernel).
template <bool STRIDED>
int jd_entropy(const istvt_jpeg_decode_args* a, const int* images, int n, const int* segments, int nseg, long blocks,
               const JdScratch& s, int most = 0, long nrows = 0, int chunk_bytes = 0) {
    const uint8_t* src = (const uint8_t*)a->bytes;
    if (!s.rows)
        hipLaunchKernelGGL(jpeg_entropy_kernel, dim3((unsigned)((nseg + 63) / 64)), dim3(64), 0, a->stream, src, a->nbytes, images,
                           n, segments, nseg, a->htabs, a->nh, s.coef, blocks, s.seg_status);
    else if (most <= 64)
        hipLaunchKernelGGL((jpeg_entropy_split_kernel<64, STRIDED>), dim3((unsigned)nseg), dim3(64), 0, a->stream, src, a->nbytes,
                           images, n, segments, nseg, a->htabs, a->nh, s.coef, blocks, s.seg_status, s.rows, nrows, chunk_bytes);
    else
        hipLaunchKernelGGL((jpeg_entropy_split_kernel<JS_LANES, STRIDED>), dim3((unsigned)nseg), dim3(JS_LANES), 0, a->stream, src,
                           a->nbytes, images, n, segments, nseg, a->htabs, a->nh, s.coef, blocks, s.seg_status, s.rows, nrows,
                           chunk_bytes);
    return istvt_check_launch();
}

// The IDCT in `groups` workgroups, which also folds the `words` status words into the statuses, then the colour kernel
int jd_finish(const istvt_jpeg_decode_args* a, const int* images, int n, int words, long groups, const JdScratch& s, long npix) {
    hipLaunchKernelGGL(jpeg_idct_kernel, dim3((unsigned)groups), dim3(256), 0, a->stream, s.coef, images, n, a->qtabs, a->nq,
                       s.seg_status, words, s.planes, a->sizes, a->status);
    const int rc = istvt_check_launch();
    if (rc != ISTVT_OK) return rc;
    uint8_t* out = (uint8_t*)a->out;
    hipLaunchKernelGGL(jpeg_canvas_kernel, dim3((unsigned)((npix + 1023) / 1024)), dim3(256), 0, a->stream, images, s.planes, out,
                       npix, a->Hc, a->Wc, (int)((reinterpret_cast<uintptr_t>(out) & 3) == 0));
    return istvt_check_launch();
}

}  // namespace

// A batch of baseline JPEG files, packed by clips.jpeg_batch, decoded to uint8 RGB on a canvas out [n][Hc][Wc][3]; the
// argument block is described in include/istvt_hip.h.  Three launches, no synchronisation, no global state.
extern "C" int istvt_jpeg_decode_u8(const istvt_jpeg_decode_args* a) {
    long groups = 0, npix;
    JdScratch s;
    const long blocks = jd_args_check(a, false, 1, 1, &groups);
    if (blocks < 0 || !jd_scratch(a, blocks, a->nseg, 0, 0, 0, s) || !jd_out_ok(a, a->n, npix)) return ISTVT_ERR_SHAPE;
    const int rc = jd_entropy<false>(a, a->images, a->n, a->segments, a->nseg, blocks, s);
    return rc != ISTVT_OK ? rc : jd_finish(a, a->images, a->n, a->nseg, groups, s, npix);
}

// istvt_jpeg_decode_u8 with the split entropy kernel in front: a workgroup per restart interval, a lane per chunk of
// chunk_bytes (at least 16) of it, for files whose intervals are long (DESIGN.md "JPEG files without restart markers").  The
// same checks, the same IDCT and colour launches, the same bytes out.  The scratch keeps the layout above in front; the state
// rows follow the statuses at the next multiple of 16 bytes.
extern "C" int istvt_jpeg_decode_split_u8(const istvt_jpeg_decode_args* a, int chunk_bytes) {
    long groups = 0, npix;
    JdScratch s;
    const long blocks = chunk_bytes < 16 ? -1 : jd_args_check(a, false, 1, 1, &groups);
    if (blocks < 0) return ISTVT_ERR_SHAPE;
    long chunks = 0;
    int most = 0;                                                 // chunks of the longest segment
    for (int s = 0; s < a->nseg; ++s) {                          // segments in the order of their bytes: what the rows rely on
        const int* sg = a->segments_host + (long)s * JD_SEGMENT_INTS;
        if (s > 0 && sg[1] < sg[-JD_SEGMENT_INTS + 2]) return ISTVT_ERR_SHAPE;
        const int c = js_chunks((long)sg[2] - sg[1], chunk_bytes);
        chunks += c;
        most = c > most ? c : most;
    }
    const long nrows = a->nbytes / chunk_bytes + a->nseg;         // chunks <= nrows
    if (chunks > nrows || !jd_scratch(a, blocks, a->nseg, 0, 0, nrows, s) || !jd_out_ok(a, a->n, npix)) return ISTVT_ERR_SHAPE;
    const int rc = jd_entropy<false>(a, a->images, a->n, a->segments, a->nseg, blocks, s, most, nrows, chunk_bytes);
    return rc != ISTVT_OK ? rc : jd_finish(a, a->images, a->n, a->nseg, groups, s, npix);
}

// ---- JPEG bank -------------------------------------------------------------------------------------------------------------
// DESIGN.md "JPEG bank": files parsed once and kept on the device, decoded through an index that lives there too.  The plan
// kernel turns the index into the two tables the three kernels above read, at uniform strides (seg_max segment rows and
// block_stride blocks per place), so every grid is known on the host; the ingest builds a bank's tables from the encoder's
// files without a host parse.  csrc/jpeg_bank_scan.h has the arithmetic both share with tools/jpeg_bank_check.cpp.

namespace {

// One workgroup per place j of the index: its images row, its seg_max segment rows and its word behind the segment
// statuses (jb_plan_image says what that word is for).  seg_bytes_max: the longest segment a place may have, which the split
// entries name (their state rows are reserved for it); -1: no limit.
__global__ __launch_bounds__(64) void jpeg_bank_plan_kernel(const int* __restrict__ bank_images, int n,
                                                            const int* __restrict__ bank_segments, int bank_nseg,
                                                            const int* __restrict__ index, int m, int seg_max, int block_stride,
                                                            int Hc, int Wc, int* __restrict__ images, int* __restrict__ segments,
                                                            int* __restrict__ place_status, int seg_bytes_max) {
    const int j = blockIdx.x, tid = threadIdx.x;
    const int idx = index[j];
    const int st = jb_plan_status(bank_images, n, bank_segments, bank_nseg, idx, seg_max, block_stride, Hc, Wc, seg_bytes_max);
    if (tid == 0) {
        int row[JB_IMAGE_INTS];
        jb_plan_image(bank_images, idx, st, j, m, seg_max, block_stride, row);
#pragma unroll
        for (int f = 0; f < JB_IMAGE_INTS; ++f) images[(long)j * JB_IMAGE_INTS + f] = row[f];
        place_status[j] = st;
    }
    for (int k = tid; k < seg_max; k += 64) {
        int row[JB_SEGMENT_INTS];
        jb_plan_segment(bank_images, bank_segments, idx, st, j, k, row);
        int* dst = segments + ((long)j * seg_max + k) * JB_SEGMENT_INTS;
#pragma unroll
        for (int f = 0; f < JB_SEGMENT_INTS; ++f) dst[f] = row[f];
    }
}

// what all files of one encoder call share
struct JbGeometry {
    int H, W, sub, mcux, mcuy, layout, blocks, ri, seg_max;    // ri: MCUs per restart interval, never 0
};

// whether file i of the encoder's result can be read: fine by the encoder, inside data, long enough for a header and EOI
__device__ __forceinline__ bool jb_file_ok(const long* __restrict__ offsets, const int* __restrict__ enc_status, int i,
                                           long capacity, int header_bytes) {
    const long start = offsets[i], stop = offsets[i + 1];
    return enc_status[i] == 0 && start >= 0 && stop <= capacity && stop <= 0x7fffffffL && stop - start >= header_bytes + 2;
}

// One lane per table entry: the 2 x 64 bytes at dqt0 / dqt1 of file i, zig-zag order -> qtabs rows 2 i, 2 i + 1, natural
// order; all 1 for a file that cannot be read
__global__ __launch_bounds__(256) void jpeg_bank_qtabs_kernel(const uint8_t* __restrict__ data, long capacity,
                                                              const long* __restrict__ offsets,
                                                              const int* __restrict__ enc_status, int n, int header_bytes,
                                                              int dqt0, int dqt1, int* __restrict__ qtabs) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= (long)n * 128) return;
    const int i = (int)(e >> 7), t = (int)(e >> 6) & 1, k = (int)e & 63;
    int v = 1;
    if (jb_file_ok(offsets, enc_status, i, capacity, header_bytes)) v = data[offsets[i] + (t ? dqt1 : dqt0) + k];
    qtabs[((long)2 * i + t) * 64 + je_zigzag(k)] = v;
}

// One workgroup per file: the restart markers of its scan -> its seg_max segment rows, and its images row.  The lanes walk
// the scan in tiles of 256 x 16 bytes; a lane finds the pairs that start in its bytes (jb_markers), an inclusive scan of
// the counts in LDS plus the count of the tiles before orders them, and marker r ends interval r and starts interval r +
// 1.  A file the encoder did not finish, one too short for its header, one that does not end with EOI or whose marker count
// is not seg_max - 1 gets 0 segments in its images row: an empty place, status 5 when it is drawn.
__global__ __launch_bounds__(256) void jpeg_bank_scan_kernel(const uint8_t* __restrict__ data, long capacity,
                                                             const long* __restrict__ offsets,
                                                             const int* __restrict__ enc_status, int header_bytes, JbGeometry g,
                                                             int* __restrict__ segments, int* __restrict__ images) {
    __shared__ int counts[256];
    const int i = blockIdx.x, tid = threadIdx.x;
    bool ok = jb_file_ok(offsets, enc_status, i, capacity, header_bytes);        // the same for every lane
    const long begin = ok ? offsets[i] + header_bytes : 0, end = ok ? offsets[i + 1] - 2 : 0;   // end: where EOI stands
    ok = ok && data[end] == 0xFF && data[end + 1] == 0xD9;
    int* seg = segments + (long)i * g.seg_max * JB_SEGMENT_INTS;
    const int mcus = g.mcux * g.mcuy;
    for (int k = tid; k < g.seg_max; k += 256) {
        int* row = seg + (long)k * JB_SEGMENT_INTS;
        row[0] = i, row[3] = k * g.ri, row[4] = min(g.ri, mcus - k * g.ri);
        if (!ok) row[1] = row[2] = 0;
    }
    int found = 0;                                               // markers in the tiles before this one
    if (ok) {
        if (tid == 0) seg[1] = (int)begin, seg[(long)(g.seg_max - 1) * JB_SEGMENT_INTS + 2] = (int)end;
        for (long tile = begin; tile < end; tile += JB_TILE_BYTES) {
            const long lo = tile + (long)tid * JB_LANE_BYTES, hi = min(lo + JB_LANE_BYTES, end);
            uint32_t mask = jb_markers(data, lo, hi, end);
            const int mine = __popc(mask);
            int sum = mine;
            counts[tid] = sum;
            __syncthreads();
            for (int d = 1; d < 256; d <<= 1) {
                const int add = tid >= d ? counts[tid - d] : 0;
                __syncthreads();
                sum += add;
                counts[tid] = sum;
                __syncthreads();
            }
            int r = found + sum - mine;
            while (mask) {
                const long p = lo + __ffs(mask) - 1;
                mask &= mask - 1;
                if (r < g.seg_max - 1) {
                    seg[(long)r * JB_SEGMENT_INTS + 2] = (int)p;
                    seg[(long)(r + 1) * JB_SEGMENT_INTS + 1] = (int)p + 2;
                }
                ++r;
            }
            found += counts[255];
            __syncthreads();                                     // counts[255] is read before the next tile writes it
        }
    }
    const bool whole = ok && found == g.seg_max - 1;
    __syncthreads();                                             // the marker stores of other lanes lie before the next ones
    if (ok && !whole)
        for (int k = tid; k < g.seg_max; k += 256) seg[(long)k * JB_SEGMENT_INTS + 1] = seg[(long)k * JB_SEGMENT_INTS + 2] = 0;
    if (tid < JB_IMAGE_INTS) {
        const bool grey = g.layout == ISTVT_JPEG_LAYOUT_GREY;
        int v = 0;
        if (tid == JB_H) v = g.H;
        else if (tid == JB_W) v = g.W;
        else if (tid == JB_SUB) v = g.sub;
        else if (tid == JB_MCUX) v = g.mcux;
        else if (tid == JB_MCUY) v = g.mcuy;
        else if (tid < JB_HUFF) v = 2 * i + (tid > JB_QUANT && !grey);        // Y: the file's first table; Cb, Cr: its second
        else if (tid < JB_BLOCK0) v = grey ? (tid - JB_HUFF) & 1 : tid < JB_HUFF + 2 ? tid - JB_HUFF : 2 + ((tid - JB_HUFF) & 1);
        else if (tid == JB_BLOCK0) v = i * g.blocks;
        else if (tid == JB_GROUP0) v = i * ((g.blocks + JP_BLOCKS - 1) / JP_BLOCKS);
        else if (tid == JB_SEG0) v = i * g.seg_max;
        else if (tid == JB_NSEG) v = whole ? g.seg_max : 0;
        else if (tid == JB_NBLOCKS) v = g.blocks;
        else v = g.layout;
        images[(long)i * JB_IMAGE_INTS + tid] = v;
    }
}

// Both bank entries behind their own scalars: m places planned at seg_max segment rows and block_stride blocks each, then
// the kernels of the direct entries on the planned tables, with one status word per planned segment row and one per place.
// chunk_bytes = 0: one lane per segment; else the split kernel with chunk_rows state rows per segment.
int jb_decode(const istvt_jpeg_decode_args* a, int m, int seg_max, int block_stride, int Hmax, int Wmax, int chunk_bytes,
              int chunk_rows, int seg_bytes_max) {
    if (jd_args_check(a, true, Hmax, Wmax, nullptr) < 0) return ISTVT_ERR_SHAPE;
    if (m <= 0 || seg_max < 1 || block_stride < JP_BLOCKS || block_stride % JP_BLOCKS != 0) return ISTVT_ERR_SHAPE;
    const long blocks = (long)m * block_stride, nseg = (long)m * seg_max, words = nseg + m;
    if (blocks > 0x7fffffffL / 64 || words > 0x7fffffffL / JD_SEGMENT_INTS) return ISTVT_ERR_SHAPE;
    long npix;
    JdScratch s;
    if (!jd_scratch(a, blocks, words, m, seg_max, chunk_bytes ? nseg * chunk_rows : 0, s) || !jd_out_ok(a, m, npix))
        return ISTVT_ERR_SHAPE;
    const int* index = a->images_host;                           // these entries' reading of the field: on the device
    hipLaunchKernelGGL(jpeg_bank_plan_kernel, dim3((unsigned)m), dim3(64), 0, a->stream, a->images, a->n, a->segments, a->nseg,
                       index, m, seg_max, block_stride, a->Hc, a->Wc, s.images, s.segments, s.seg_status + nseg, seg_bytes_max);
    int rc = istvt_check_launch();
    if (rc != ISTVT_OK) return rc;
    rc = jd_entropy<true>(a, s.images, m, s.segments, (int)nseg, blocks, s, chunk_rows, (long)chunk_rows, chunk_bytes);
    return rc != ISTVT_OK ? rc : jd_finish(a, s.images, m, (int)words, blocks / JP_BLOCKS, s, npix);
}

}  // namespace

// A bank decoded through an index; the argument block is described in include/istvt_hip.h.  Four launches: the plan, then
// the three kernels of istvt_jpeg_decode_u8 on the planned tables.  No synchronisation, no global state, no atomics of its
// own, nothing allocated.  The checks here are on scalars alone: the bank's tables were checked when it was built.
extern "C" int istvt_jpeg_decode_indexed_u8(const istvt_jpeg_decode_args* a, int m, int seg_max, int block_stride, int Hmax,
                                            int Wmax) {
    return jb_decode(a, m, seg_max, block_stride, Hmax, Wmax, 0, 0, -1);
}

// istvt_jpeg_decode_indexed_u8 with the split entropy kernel behind the plan, for a bank of files whose restart intervals are
// long (DESIGN.md "JPEG bank, split"): four launches, the same checks on scalars alone, the same bytes out.  A workgroup per
// planned segment row, m * seg_max of them; segment s keeps its state rows at [s * chunk_rows, (s + 1) * chunk_rows) behind the
// layout above, from the next multiple of 16 bytes, so the table's size comes from m alone and not from where the drawn
// files lie in the bank.  chunk_rows >= the chunks of any segment of up to seg_bytes_max bytes (the bank knows both); the plan
// turns a place with a longer segment into status 5, and the kernel refuses more than chunk_rows chunks by itself.
extern "C" int istvt_jpeg_decode_indexed_split_u8(const istvt_jpeg_decode_args* a, int m, int seg_max, int block_stride, int Hmax,
                                                  int Wmax, int chunk_bytes, int chunk_rows, int seg_bytes_max) {
    if (chunk_bytes < 16 || chunk_rows < 1 || chunk_rows > JS_LANES) return ISTVT_ERR_SHAPE;
    return jb_decode(a, m, seg_max, block_stride, Hmax, Wmax, chunk_bytes, chunk_rows, seg_bytes_max < 0 ? -1 : seg_bytes_max);
}

// The encoder's files -> the tables of a bank, on the device; the argument block is described in include/istvt_hip.h.  Two
// launches, no synchronisation, no atomics, nothing allocated.
extern "C" int istvt_jpeg_bank_ingest(const istvt_jpeg_encode_args* a, int layout) {
    if (!a || a->n <= 0 || a->H < 1 || a->W < 1 || a->H > 16384 || a->W > 16384) return ISTVT_ERR_SHAPE;
    if (!a->data || !a->offsets || !a->status || !a->scratch) return ISTVT_ERR_SHAPE;
    if (a->capacity < 1 || a->capacity > 0x7fffffffL || a->restart_interval < 0 || a->restart_interval > 65535)
        return ISTVT_ERR_SHAPE;
    if (a->dqt0 < 0 || a->dqt1 < a->dqt0 + 64 || a->header_bytes < a->dqt1 + 64 || a->header_bytes > 0x7fffffffL)
        return ISTVT_ERR_SHAPE;
    int sub;
    if (layout == 0 && (a->subsampling == 2 || a->subsampling == 0)) sub = a->subsampling == 2 ? 2 : 1;
    else if (layout == ISTVT_JPEG_LAYOUT_422 && a->subsampling == 0) sub = 2;
    else if (layout == ISTVT_JPEG_LAYOUT_GREY && a->subsampling == 0) sub = 1;
    else return ISTVT_ERR_SHAPE;
    const JeLayout lay = je_layout(layout, sub);
    JbGeometry g;
    g.H = a->H, g.W = a->W, g.sub = sub, g.layout = layout;
    g.mcux = (a->W + 8 * lay.h - 1) / (8 * lay.h), g.mcuy = (a->H + 8 * lay.v - 1) / (8 * lay.v);
    const int mcus = g.mcux * g.mcuy;
    g.blocks = mcus * js_mcu_blocks(lay);
    g.ri = a->restart_interval > 0 && a->restart_interval < mcus ? a->restart_interval : mcus;
    g.seg_max = (mcus + g.ri - 1) / g.ri;
    const long rows = (long)a->n * g.seg_max;
    if (rows > 0x7fffffffL / JD_SEGMENT_INTS || (long)a->n * g.blocks > 0x7fffffffL / 64) return ISTVT_ERR_SHAPE;
    if ((reinterpret_cast<uintptr_t>(a->scratch) & 15) ||
        a->scratch_bytes < 4 * (rows * JD_SEGMENT_INTS + (long)a->n * (128 + JD_IMAGE_INTS)))
        return ISTVT_ERR_SHAPE;
    const uint8_t* data = (const uint8_t*)a->data;
    int* segments = (int*)a->scratch;
    int* qtabs = segments + rows * JD_SEGMENT_INTS;
    int* images = qtabs + (long)a->n * 128;
    hipLaunchKernelGGL(jpeg_bank_qtabs_kernel, dim3((unsigned)(((long)a->n * 128 + 255) / 256)), dim3(256), 0, a->stream, data,
                       a->capacity, a->offsets, a->status, a->n, (int)a->header_bytes, a->dqt0, a->dqt1, qtabs);
    const int rc = istvt_check_launch();
    if (rc != ISTVT_OK) return rc;
    hipLaunchKernelGGL(jpeg_bank_scan_kernel, dim3((unsigned)a->n), dim3(256), 0, a->stream, data, a->capacity, a->offsets,
                       a->status, (int)a->header_bytes, g, segments, images);
    return istvt_check_launch();
}

// ---- JPEG files out ------------------------------------------------------------------------------------------------------
// istvt_jpeg_encode_u8 (DESIGN.md "JPEG files out"): frames -> baseline files laid end to end in one buffer, the bytes of
// clips.jpeg_encode_host.  Four launches: jpeg_planes_kernel<SUB, true> (coefficients) | jpeg_count_kernel (one lane per
// restart interval: its length) | jpeg_offsets_kernel (one workgroup: where every file and segment starts, the statuses) |
// jpeg_write_kernel (the same lanes store; one workgroup per image copies the header).

namespace {

// a row of the per-segment table behind the coefficients in the scratch: where the segment's first byte goes (written by
// jpeg_offsets_kernel) and its length in the low 56 bits with its status above them (written by jpeg_count_kernel)
struct JeSegment {
    long begin;
    unsigned long size;
};
constexpr int JE_STATUS_SHIFT = 56;
constexpr unsigned long JE_LENGTH_MASK = (1ul << JE_STATUS_SHIFT) - 1;

// what the three kernels behind the coefficients share
struct JeGeometry {
    int n, mcux, mcuy, ri, nseg;            // frames; MCUs per row / column; MCUs per segment; segments per image
    JeLayout lay;                           // the blocks of an MCU: (sub, sub, 2) for the chroma step of the first two entries
    long nb;                                // blocks per image
};

__device__ __forceinline__ void je_stage_codes(uint32_t* codes, int tid, int lanes) {
    for (int i = tid; i < JE_CODE_WORDS; i += lanes) codes[i] = je_code_word(i);
    __syncthreads();
}

// segment s of the batch through je_encode_segment -> its length and status
template <class Sink>
__device__ __forceinline__ long je_run_segment(const JeGeometry& g, const short* coef, long s, const uint32_t* codes, Sink& sink,
                                               int& status) {
    const long img = s / g.nseg;
    const int k = (int)(s - img * g.nseg);
    const long mcus = (long)g.mcux * g.mcuy;
    const long first = (long)k * g.ri;
    const int count = (int)min((long)g.ri, mcus - first);
    const int marker = k == g.nseg - 1 ? 0xD9 : 0xD0 + (k & 7);
    return je_encode_segment(coef + img * g.nb * 64, g.lay, g.mcux, g.mcuy, (int)first, count, codes, marker, sink, status);
}

__global__ __launch_bounds__(64) void jpeg_count_kernel(JeGeometry g, const int* __restrict__ quality,
                                                        const short* __restrict__ coef, JeSegment* __restrict__ seg) {
    __shared__ uint32_t codes[JE_CODE_WORDS];
    je_stage_codes(codes, threadIdx.x, 64);
    const long s = (long)blockIdx.x * 64 + threadIdx.x;
    if (s >= (long)g.n * g.nseg) return;
    if (quality[s / g.nseg] <= 0) {                              // no coefficients, an empty file
        seg[s].size = 2ul << JE_STATUS_SHIFT;
        return;
    }
    JeCount sink = {0};
    int status = 0;
    const long len = je_run_segment(g, coef, s, codes, sink, status);
    seg[s].size = ((unsigned long)len & JE_LENGTH_MASK) | (unsigned long)status << JE_STATUS_SHIFT;
}

// One workgroup.  The exclusive prefix sum, in one fixed order, of header + segments over the images: lane t sums the t-th
// run of consecutive segments, the 256 sums are scanned in LDS, lane t walks its run again and writes the places.
// header_of(img): the bytes in front of the first segment of a file that has one
template <class HeaderOf>
__device__ __forceinline__ void je_offsets(const JeGeometry& g, const int* __restrict__ quality, HeaderOf header_of, long capacity,
                                           JeSegment* __restrict__ seg, long* __restrict__ offsets, int* __restrict__ status) {
    __shared__ long part[256];
    const int tid = threadIdx.x;
    const long N = (long)g.n * g.nseg, per = (N + 255) / 256;
    const long lo = min(N, tid * per), hi = min(N, lo + per);
    for (int i = tid; i < g.n; i += 256) status[i] = 0;
    long sum = 0;
    for (long e = lo; e < hi; ++e) {
        const long img = e / g.nseg;
        sum += (long)(seg[e].size & JE_LENGTH_MASK) + (e == img * g.nseg && quality[img] > 0 ? header_of(img) : 0);
    }
    part[tid] = sum;
    __syncthreads();
    for (int d = 1; d < 256; d <<= 1) {                          // inclusive scan of the 256 sums
        const long add = tid >= d ? part[tid - d] : 0;
        __syncthreads();
        part[tid] += add;
        __syncthreads();
    }
    long at = part[tid] - sum;
    for (long e = lo; e < hi; ++e) {
        const long img = e / g.nseg;
        const unsigned long size = seg[e].size;
        long head = 0;
        if (e == img * g.nseg) {
            offsets[img] = at;
            head = quality[img] > 0 ? header_of(img) : 0;
        }
        seg[e].begin = at + head;
        at += head + (long)(size & JE_LENGTH_MASK);
        const int st = (int)(size >> JE_STATUS_SHIFT);
        if (st) atomicMax(status + img, st);
    }
    if (tid == 255) offsets[g.n] = part[255];
    __syncthreads();
    for (int i = tid; i < g.n; i += 256)
        if (offsets[i + 1] > capacity) status[i] = 1;            // the file does not fit: nothing of it is written
}

__global__ __launch_bounds__(256) void jpeg_offsets_kernel(JeGeometry g, const int* __restrict__ quality, long header_bytes,
                                                           long capacity, JeSegment* __restrict__ seg, long* __restrict__ offsets,
                                                           int* __restrict__ status) {
    je_offsets(g, quality, [header_bytes](long) { return header_bytes; }, capacity, seg, offsets, status);
}

// byte i of the shared header for a frame whose quality scales the Annex K tables by s: the two quantisation tables at dqt0
// and dqt1 are filled in, in zig-zag order as the file holds them
__device__ __forceinline__ uint8_t je_header_byte(const uint8_t* __restrict__ header, int i, int dqt0, int dqt1, int s) {
    const int t = i >= dqt0 && i < dqt0 + 64 ? i - dqt0 : i >= dqt1 && i < dqt1 + 64 ? 64 + i - dqt1 : -1;
    if (t < 0) return header[i];
    return (uint8_t)min(max((JP_BASE[(t & 64) + je_zigzag(t & 63)] * s + 50) / 100, 1), 255);
}

// Workgroups [0, seg_groups): one lane per segment stores what it counted.  Workgroups behind them: one per image copies
// the header, with the two quantisation tables of the frame's quality in their places.
__global__ __launch_bounds__(64) void jpeg_write_kernel(JeGeometry g, int seg_groups, const int* __restrict__ quality,
                                                        const short* __restrict__ coef, const JeSegment* __restrict__ seg,
                                                        const uint8_t* __restrict__ header, int header_bytes, int dqt0, int dqt1,
                                                        const long* __restrict__ offsets, const int* __restrict__ status,
                                                        uint8_t* __restrict__ data, long capacity) {
    __shared__ uint32_t codes[JE_CODE_WORDS];
    const int tid = threadIdx.x;
    if ((int)blockIdx.x >= seg_groups) {
        const int img = blockIdx.x - seg_groups;
        const int st = status[img];
        const long at = offsets[img];
        if (st == 1 || st == 2 || at < 0 || at + header_bytes > capacity) return;
        const int q = min(quality[img], 100);
        const int s = q < 50 ? 5000 / max(q, 1) : 200 - 2 * q;
        for (int i = tid; i < header_bytes; i += 64) data[at + i] = je_header_byte(header, i, dqt0, dqt1, s);
        return;
    }
    je_stage_codes(codes, tid, 64);
    const long s = (long)blockIdx.x * 64 + tid;
    if (s >= (long)g.n * g.nseg) return;
    const int st = status[s / g.nseg];
    if (st == 1 || st == 2) return;
    const long begin = seg[s].begin, len = (long)(seg[s].size & JE_LENGTH_MASK);
    if (begin < 0 || begin + len > capacity) return;              // cannot be, with status 0 or 3; keeps a store inside data
    JeStore sink = {data, begin, len, 0};
    int ignored = 0;
    je_run_segment(g, coef, s, codes, sink, ignored);
}

// The geometry of a call whose MCUs hold LV rows of LH Y blocks and LNC chroma blocks (JeLayout) and its first launch, the
// coefficients: jpeg_planes_kernel<SUB, true> where the chroma step SUB is that of both axes, jpeg_coef_kernel otherwise.
// row_bytes: what an image adds to the scratch behind the segment table.  -> blocks of the batch in `blocks`
template <int LH, int LV, int LNC> int jpeg_encode_front(const istvt_jpeg_encode_args* a, long row_bytes, JeGeometry& g, long& blocks) {
    constexpr int MW = 8 * LH, MH = 8 * LV;
    const int H = a->H, W = a->W, n = a->n;
    const int Hp = (H + MH - 1) / MH * MH, Wp = (W + MW - 1) / MW * MW;
    g.n = n, g.lay = JeLayout{LH, LV, LNC}, g.mcux = Wp / MW, g.mcuy = Hp / MH;
    const long mcus = (long)g.mcux * g.mcuy;
    g.ri = (int)(a->restart_interval ? min((long)a->restart_interval, mcus) : mcus);
    const long nseg = (mcus + g.ri - 1) / g.ri;
    g.nb = mcus * (LH * LV + LNC);
    blocks = g.nb * n;
    const long segments = nseg * n;
    const int tiles_y = Hp / MH, tiles_x = (Wp + JP_TILE_W - 1) / JP_TILE_W;
    const long tiles = (long)n * tiles_y * tiles_x;
    // a segment's length stays far inside 56 bits: at most 64 symbols of 27 bits per block, each byte stuffed
    if (tiles > 0x7fffffffL || segments > 0x7fffffffL - 64 - n || blocks > 0x7fffffffL || 2L * n > 0x7fffffffL) return ISTVT_ERR_SHAPE;
    if (a->scratch_bytes < blocks * 128 + segments * (long)sizeof(JeSegment) + n * row_bytes) return ISTVT_ERR_SHAPE;
    g.nseg = (int)nseg;
    uint8_t* coef = (uint8_t*)a->scratch;
    const uint8_t* x = (const uint8_t*)a->frames;
    if constexpr (LH == LV && LNC == 2)
        hipLaunchKernelGGL((jpeg_planes_kernel<LH, true>), dim3((unsigned)tiles), dim3(256), 0, a->stream, x, a->total, a->quality,
                           coef, H, W, Hp, Wp, tiles_y, tiles_x);
    else
        hipLaunchKernelGGL((jpeg_coef_kernel<LNC == 0>), dim3((unsigned)tiles), dim3(256), 0, a->stream, x, a->total, a->quality,
                           coef, H, W, Hp, Wp, tiles_y, tiles_x);
    return istvt_check_launch();
}

template <int LH, int LV, int LNC> int jpeg_encode_launch(const istvt_jpeg_encode_args* a) {
    JeGeometry g;
    long blocks = 0;
    int rc = jpeg_encode_front<LH, LV, LNC>(a, 0, g, blocks);
    if (rc != ISTVT_OK) return rc;
    const int n = a->n;
    const long segments = (long)g.nseg * n;
    uint8_t* coef = (uint8_t*)a->scratch;
    JeSegment* seg = (JeSegment*)(coef + blocks * 128);
    const int seg_groups = (int)((segments + 63) / 64);
    hipLaunchKernelGGL(jpeg_count_kernel, dim3((unsigned)seg_groups), dim3(64), 0, a->stream, g, a->quality, (const short*)coef, seg);
    rc = istvt_check_launch();
    if (rc != ISTVT_OK) return rc;
    hipLaunchKernelGGL(jpeg_offsets_kernel, dim3(1), dim3(256), 0, a->stream, g, a->quality, a->header_bytes, a->capacity, seg,
                       a->offsets, a->status);
    rc = istvt_check_launch();
    if (rc != ISTVT_OK) return rc;
    hipLaunchKernelGGL(jpeg_write_kernel, dim3((unsigned)(seg_groups + n)), dim3(64), 0, a->stream, g, seg_groups, a->quality,
                       (const short*)coef, (const JeSegment*)seg, (const uint8_t*)a->header, (int)a->header_bytes, a->dqt0, a->dqt1,
                       (const long*)a->offsets, (const int*)a->status, (uint8_t*)a->data, a->capacity);
    return istvt_check_launch();
}

// ---- JPEG files out, optimised tables ------------------------------------------------------------------------------------
// istvt_jpeg_encode_opt_u8 (DESIGN.md "JPEG files out, optimised tables"): the files above, each coded with its own four
// Huffman tables.  Five launches: jpeg_planes_kernel<SUB, true> | jpeg_tables_kernel (one workgroup per image: symbol counts
// in LDS, jo_optimal_table, the image's row of the scratch) | jpeg_count_opt_kernel (one workgroup per image, its code
// words staged in LDS, one lane per restart interval) | jpeg_offsets_opt_kernel | jpeg_write_opt_kernel.

// an image's row behind the segment table: int32 header length | 4 DHT segments JO_DHT_STRIDE apart | JE_CODE_WORDS words
constexpr int JO_DHT_STRIDE = 288, JO_DHT_MAX = 21 + 256;
constexpr int JO_ROW_DHT = 16, JO_ROW_CODES = JO_ROW_DHT + 4 * JO_DHT_STRIDE;
constexpr int JO_ROW_BYTES = ISTVT_JPEG_OPT_ROW_BYTES;
static_assert(JO_ROW_BYTES == JO_ROW_CODES + 4 * JE_CODE_WORDS && JO_ROW_BYTES % 16 == 0 && JO_ROW_CODES % 16 == 0 &&
              JO_DHT_MAX <= JO_DHT_STRIDE, "the row of include/istvt_hip.h");

// the sink of jo_count_block on four LDS histograms (JoHistogram's order); integer adds, so the order does not matter
struct JoLdsHistogram {
    uint32_t* counts;
    __device__ __forceinline__ void dc(int id, int sym) { atomicAdd(counts + (id & 1) * 256 + (sym & 255), 1u); }
    __device__ __forceinline__ void ac(int id, int sym, uint32_t times) { atomicAdd(counts + (2 + (id & 1)) * 256 + (sym & 255), times); }
};

// the bytes of image img's table segment t as the file holds it: FF C4, length, class and id, 16 counts, the values
__device__ __forceinline__ int jo_dht_length(const uint8_t* dht) { return min(2 + ((dht[2] << 8) | dht[3]), JO_DHT_MAX); }

// One workgroup per image.  fixed_bytes: the header's bytes outside its table segments
__global__ __launch_bounds__(256) void jpeg_tables_kernel(JeGeometry g, const int* __restrict__ quality, const short* __restrict__ coef,
                                                          uint8_t* __restrict__ rows, int fixed_bytes) {
    __shared__ uint32_t hist[4 * 256];
    __shared__ JoWork work[4];
    __shared__ uint32_t words[JE_CODE_WORDS];
    __shared__ uint8_t dht[4][JO_DHT_STRIDE];
    const int tid = threadIdx.x, img = blockIdx.x;
    if (quality[img] <= 0) return;                                // no coefficients, no file: its row stays unwritten
    for (int i = tid; i < 4 * 256; i += 256) hist[i] = 0;
    __syncthreads();
    const JeQuad* blocks = reinterpret_cast<const JeQuad*>(coef + (long)img * g.nb * 64);
    JoLdsHistogram sink = {hist};
    for (long b = tid; b < g.nb; b += 256) {
        int id = 0;
        const long p = jo_previous_block(b, g.lay, g.mcux, g.mcuy, g.ri, id);
        const int pred = p < 0 || p >= g.nb ? 0 : (int16_t)(blocks[p * 8].lo & 0xFFFF);
        jo_count_block(sink, blocks + b * 8, pred, id);
    }
    __syncthreads();
    if ((tid & 63) == 0) {                                        // one table per wave
        const int t = tid >> 6;
        uint8_t* d = dht[t];
        int total = 0;
        jo_optimal_table(hist + t * 256, d + 5, d + 21, &total, work[t]);
        total = min(max(total, 0), 256);
        d[0] = 0xFF, d[1] = 0xC4, d[2] = (uint8_t)((19 + total) >> 8), d[3] = (uint8_t)((19 + total) & 255);
        d[4] = (uint8_t)(((t >> 1) << 4) | (t & 1));
        jo_code_words(d + 5, d + 21, total, words + (t < 2 ? JE_CODE_DC + 16 * t : JE_CODE_AC + 256 * (t - 2)), t < 2 ? 16 : 256);
    }
    __syncthreads();
    uint8_t* row = rows + (long)img * JO_ROW_BYTES;
    if (tid == 0) {
        int head = fixed_bytes;
        for (int t = 0; t < 4; ++t) head += jo_dht_length(dht[t]);
        *reinterpret_cast<int*>(row) = head;
    }
    for (int t = 0; t < 4; ++t) {
        const int len = jo_dht_length(dht[t]);
        for (int i = tid; i < len; i += 256) row[JO_ROW_DHT + t * JO_DHT_STRIDE + i] = dht[t][i];
    }
    uint32_t* codes = reinterpret_cast<uint32_t*>(row + JO_ROW_CODES);
    for (int i = tid; i < JE_CODE_WORDS; i += 256) codes[i] = words[i];
}

__device__ __forceinline__ void jo_stage_codes(uint32_t* codes, const uint8_t* rows, int img, int tid, int lanes) {
    const uint32_t* from = reinterpret_cast<const uint32_t*>(rows + (long)img * JO_ROW_BYTES + JO_ROW_CODES);
    for (int i = tid; i < JE_CODE_WORDS; i += lanes) codes[i] = from[i];
    __syncthreads();
}

// One workgroup per image: lane t takes the image's restart intervals t, t + 64, ...
__global__ __launch_bounds__(64) void jpeg_count_opt_kernel(JeGeometry g, const int* __restrict__ quality, const short* __restrict__ coef,
                                                            const uint8_t* __restrict__ rows, JeSegment* __restrict__ seg) {
    __shared__ uint32_t codes[JE_CODE_WORDS];
    const int tid = threadIdx.x, img = blockIdx.x;
    if (quality[img] <= 0) {                                      // no coefficients, an empty file
        for (int k = tid; k < g.nseg; k += 64) seg[(long)img * g.nseg + k].size = 2ul << JE_STATUS_SHIFT;
        return;
    }
    jo_stage_codes(codes, rows, img, tid, 64);
    for (int k = tid; k < g.nseg; k += 64) {
        const long s = (long)img * g.nseg + k;
        JeCount sink = {0};
        int status = 0;
        const long len = je_run_segment(g, coef, s, codes, sink, status);
        seg[s].size = ((unsigned long)len & JE_LENGTH_MASK) | (unsigned long)status << JE_STATUS_SHIFT;
    }
}

__global__ __launch_bounds__(256) void jpeg_offsets_opt_kernel(JeGeometry g, const int* __restrict__ quality,
                                                               const uint8_t* __restrict__ rows, long capacity,
                                                               JeSegment* __restrict__ seg, long* __restrict__ offsets,
                                                               int* __restrict__ status) {
    je_offsets(g, quality, [rows](long img) { return (long)*reinterpret_cast<const int*>(rows + img * JO_ROW_BYTES); }, capacity,
               seg, offsets, status);
}

// Workgroups [0, n): the lanes of jpeg_count_opt_kernel store what they counted.  Workgroups [n, 2 n): one per image writes
// the header: the shared bytes in front of dht0 with the quality's two quantisation tables, the image's four table
// segments, the shared bytes from dht1 on (DRI, SOS)
__global__ __launch_bounds__(64) void jpeg_write_opt_kernel(JeGeometry g, const int* __restrict__ quality, const short* __restrict__ coef,
                                                            const JeSegment* __restrict__ seg, const uint8_t* __restrict__ rows,
                                                            const uint8_t* __restrict__ header, int header_bytes, int dqt0, int dqt1,
                                                            int dht0, int dht1, const long* __restrict__ offsets,
                                                            const int* __restrict__ status, uint8_t* __restrict__ data, long capacity) {
    __shared__ uint32_t codes[JE_CODE_WORDS];
    const int tid = threadIdx.x;
    const int img = (int)blockIdx.x < g.n ? blockIdx.x : blockIdx.x - g.n;
    const int st = status[img];
    if (st == 1 || st == 2) return;
    if ((int)blockIdx.x >= g.n) {
        const uint8_t* row = rows + (long)img * JO_ROW_BYTES;
        const long at = offsets[img];
        int len[4], head = header_bytes - (dht1 - dht0);
        for (int t = 0; t < 4; ++t) head += len[t] = jo_dht_length(row + JO_ROW_DHT + t * JO_DHT_STRIDE);
        if (at < 0 || at + head > capacity || offsets[img + 1] - at < head) return;
        const int q = min(quality[img], 100);
        const int s = q < 50 ? 5000 / max(q, 1) : 200 - 2 * q;
        for (int i = tid; i < dht0; i += 64) data[at + i] = je_header_byte(header, i, dqt0, dqt1, s);
        long to = at + dht0;
        for (int t = 0; t < 4; ++t) {
            for (int i = tid; i < len[t]; i += 64) data[to + i] = row[JO_ROW_DHT + t * JO_DHT_STRIDE + i];
            to += len[t];
        }
        for (int i = dht1 + tid; i < header_bytes; i += 64) data[to + i - dht1] = header[i];
        return;
    }
    jo_stage_codes(codes, rows, img, tid, 64);
    for (int k = tid; k < g.nseg; k += 64) {
        const long s = (long)img * g.nseg + k;
        const long begin = seg[s].begin, len = (long)(seg[s].size & JE_LENGTH_MASK);
        if (begin < 0 || begin + len > capacity) continue;        // cannot be, with status 0 or 3; keeps a store inside data
        JeStore sink = {data, begin, len, 0};
        int ignored = 0;
        je_run_segment(g, coef, s, codes, sink, ignored);
    }
}

template <int LH, int LV, int LNC> int jpeg_encode_opt_launch(const istvt_jpeg_encode_args* a, int dht0, int dht1) {
    JeGeometry g;
    long blocks = 0;
    int rc = jpeg_encode_front<LH, LV, LNC>(a, JO_ROW_BYTES, g, blocks);
    if (rc != ISTVT_OK) return rc;
    const int n = a->n;
    const long segments = (long)g.nseg * n;
    uint8_t* coef = (uint8_t*)a->scratch;
    JeSegment* seg = (JeSegment*)(coef + blocks * 128);
    uint8_t* rows = (uint8_t*)(seg + segments);
    hipLaunchKernelGGL(jpeg_tables_kernel, dim3((unsigned)n), dim3(256), 0, a->stream, g, a->quality, (const short*)coef, rows,
                       (int)a->header_bytes - (dht1 - dht0));
    rc = istvt_check_launch();
    if (rc != ISTVT_OK) return rc;
    hipLaunchKernelGGL(jpeg_count_opt_kernel, dim3((unsigned)n), dim3(64), 0, a->stream, g, a->quality, (const short*)coef,
                       (const uint8_t*)rows, seg);
    rc = istvt_check_launch();
    if (rc != ISTVT_OK) return rc;
    hipLaunchKernelGGL(jpeg_offsets_opt_kernel, dim3(1), dim3(256), 0, a->stream, g, a->quality, (const uint8_t*)rows, a->capacity,
                       seg, a->offsets, a->status);
    rc = istvt_check_launch();
    if (rc != ISTVT_OK) return rc;
    hipLaunchKernelGGL(jpeg_write_opt_kernel, dim3(2u * (unsigned)n), dim3(64), 0, a->stream, g, a->quality, (const short*)coef,
                       (const JeSegment*)seg, (const uint8_t*)rows, (const uint8_t*)a->header, (int)a->header_bytes, a->dqt0, a->dqt1,
                       dht0, dht1, (const long*)a->offsets, (const int*)a->status, (uint8_t*)a->data, a->capacity);
    return istvt_check_launch();
}

// what both encoder entries refuse before any launch, but for the size of the scratch
bool jpeg_encode_dht_refused(const istvt_jpeg_encode_args* a, int dht0, int dht1) {
    return dht0 < a->dqt1 + 64 || dht1 <= dht0 || dht1 > a->header_bytes;
}

int jpeg_encode_refusal(const istvt_jpeg_encode_args* a) {
    if (!a || a->n <= 0 || !a->frames || !a->quality || !a->header || !a->scratch || !a->data || !a->offsets || !a->status)
        return ISTVT_ERR_SHAPE;
    if (a->H < 1 || a->W < 1 || a->H > 16384 || a->W > 16384) return ISTVT_ERR_SHAPE;
    if (a->subsampling != 0 && a->subsampling != 2) return ISTVT_ERR_SHAPE;
    if (a->restart_interval < 0 || a->restart_interval > 65535 || a->capacity < 0) return ISTVT_ERR_SHAPE;
    // the header: both 64-byte tables inside it, one behind the other
    if (a->header_bytes < 128 || a->header_bytes > 4096 || a->dqt0 < 0 || a->dqt1 < a->dqt0 + 64 || a->dqt1 + 64 > a->header_bytes)
        return ISTVT_ERR_SHAPE;
    const long bytes = (long)a->n * a->H * a->W * 3;
    if (a->total < bytes || (reinterpret_cast<uintptr_t>(a->scratch) & 15) || (reinterpret_cast<uintptr_t>(a->offsets) & 7) ||
        (reinterpret_cast<uintptr_t>(a->status) & 3))
        return ISTVT_ERR_SHAPE;
    const uint8_t* x = (const uint8_t*)a->frames;
    const uint8_t* d = (const uint8_t*)a->data;
    if (d < x + bytes && x < d + a->capacity) return ISTVT_ERR_SHAPE;
    return ISTVT_OK;
}

}  // namespace

// Frames uint8 [n][H][W][3] -> n baseline JPEG files end to end in data[0 .. capacity), offsets int64 [n + 1] and status
// int32 [n] on the device; the argument block is described in include/istvt_hip.h.  Four launches, no synchronisation, no
// global state, nothing allocated.
extern "C" int istvt_jpeg_encode_u8(const istvt_jpeg_encode_args* a) {
    const int rc = jpeg_encode_refusal(a);
    if (rc != ISTVT_OK) return rc;
    return a->subsampling == 2 ? jpeg_encode_launch<2, 2, 2>(a) : jpeg_encode_launch<1, 1, 2>(a);
}

// The same with every file's own Huffman tables in the place of header[dht0 .. dht1): five launches
extern "C" int istvt_jpeg_encode_opt_u8(const istvt_jpeg_encode_args* a, int dht0, int dht1) {
    const int rc = jpeg_encode_refusal(a);
    if (rc != ISTVT_OK) return rc;
    if (jpeg_encode_dht_refused(a, dht0, dht1)) return ISTVT_ERR_SHAPE;
    return a->subsampling == 2 ? jpeg_encode_opt_launch<2, 2, 2>(a, dht0, dht1) : jpeg_encode_opt_launch<1, 1, 2>(a, dht0, dht1);
}

// Both of the above in the layouts 4:2:2 (MCUs of 16 x 8 pixels, 4 blocks) and greyscale (8 x 8, one block, Y of the colour
// transform alone): the bytes of clips.jpeg_encode_host(layout=).  dht0 == dht1 == 0: the Annex K.3 tables, four launches;
// otherwise every file's own tables in the place of header[dht0 .. dht1), five launches
extern "C" int istvt_jpeg_encode_layout_u8(const istvt_jpeg_encode_args* a, int layout, int dht0, int dht1) {
    const int rc = jpeg_encode_refusal(a);
    if (rc != ISTVT_OK) return rc;
    if (a->subsampling != 0 || (layout != ISTVT_JPEG_LAYOUT_422 && layout != ISTVT_JPEG_LAYOUT_GREY)) return ISTVT_ERR_SHAPE;
    if (dht0 == 0 && dht1 == 0) return layout == ISTVT_JPEG_LAYOUT_422 ? jpeg_encode_launch<2, 1, 2>(a) : jpeg_encode_launch<1, 1, 0>(a);
    if (jpeg_encode_dht_refused(a, dht0, dht1)) return ISTVT_ERR_SHAPE;
    return layout == ISTVT_JPEG_LAYOUT_422 ? jpeg_encode_opt_launch<2, 1, 2>(a, dht0, dht1)
                                           : jpeg_encode_opt_launch<1, 1, 0>(a, dht0, dht1);
}
