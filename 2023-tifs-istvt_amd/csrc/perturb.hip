// Perturbations (DESIGN.md "Perturbations"): frames uint8 [n][H][W][3] -> uint8 [n][H][W][3], every frame through its row
// (kind, param, frame_id, stream) of a device table.  clips.perturb_host is the definition and this file gives its bits:
// int32 arithmetic with arithmetic shifts, no floating point, no atomics, one writer per byte.
//
//   0 copy        v
//   1 brightness  clamp((v p + 128) >> 8)
//   2 contrast    clamp(m + (((v - m) p + 128) >> 8)), m = (sum of Y over the frame + H W / 2) / (H W)
//   3 saturation  clamp(Y + (((v - Y) p + 128) >> 8)), Y = (19595 R + 38470 G + 7471 B + 32768) >> 16 of the pixel
//   4 noise       clamp(v + (((z p) 887 + (1 << 21)) >> 22)), z = the 16 bytes of Philox4x32-10(((y W + x) 3 + c, frame_id,
//                 stream, 0), seed) added up, less 2040
//   5 blur        clamp((sum_j t[j] sum_i t[i] v(y + j - 10, x + i - 10) + (1 << 21)) >> 22), t = taps[p], border replicated
//   6 pixelate    (S + cnt / 2) / cnt over the p x p block that holds the pixel, blocks cut to the frame
//
// Three launches, whatever the table holds.  perturb_mean_kernel: a workgroup adds up Y over one strip of a kind 2 frame and
// stores the 64-bit partial into the caller's scratch.  perturb_point_kernel (kinds 0 to 4): a lane takes 4 consecutive pixels
// of the batch, reads its frame's row once (again where the group crosses into the next frame) and stores three dwords;
// frames of kinds 5 and 6 are left to perturb_tile_kernel, where a workgroup takes a tile of PT_TILE_H rows x PT_TILE_W
// pixels, stages the source rows of tile + halo (blur: the radius of the frame's row of taps, read first) or of the blocks the
// tile meets (pixelate), cut to the frame, with u8_stage_rows, and works in LDS: blur = horizontal pass bytes -> int32 plane,
// unrounded, then vertical pass plane -> bytes; pixelate = row sums per block, block values, look-up.  A workgroup whose frame
// is not of its kernel's kinds returns at once.
#include "istvt_hip.h"
#include "philox.h"
#include "u8_view.h"

namespace {

constexpr int PT_TILE_H = 16, PT_TILE_W = 64;
constexpr int PT_RADIUS = 10, PT_TAPS = 2 * PT_RADIUS + 1;
constexpr int PT_MAX_BLOCK = 32;
// pixelate: the blocks a tile meets span < tile + 2 k - 1 pixels per axis in whole blocks of k <= 32: at most 64 rows (k = 32)
// and 124 columns (k = 31); blur: at most 16 + 20 rows and 64 + 20 columns
constexpr int PT_STAGE_ROWS = 64, PT_STAGE_COLS = 124;
constexpr int PT_PITCH = 400;                                   // u8_row_pitch(PT_STAGE_COLS)
constexpr int PT_ROW_INTS = PT_TILE_W * 3;                      // a tile row of the int32 plane: one int per byte
constexpr int PT_PLANE_INTS = (PT_TILE_H + 2 * PT_RADIUS) * PT_ROW_INTS;
// pixelate in the plane: row sums [rows][block columns][3] (at most 18 x 33 x 3 ints, at k = 2) in front, block values
// [block rows][block columns][3] (at most 9 x 33 x 3) from PT_VAL_AT
constexpr int PT_VAL_AT = 2048;
constexpr int PT_MAX_STRIPS = 32, PT_STRIP_PIXELS = 2048;       // contrast: partial sums of Y per frame

static_assert(PT_PITCH >= 15 + PT_STAGE_COLS * 3 && PT_PITCH % 16 == 0, "a staged row holds its lead and its bytes");
static_assert(PT_VAL_AT + 9 * 33 * 3 <= PT_PLANE_INTS, "both pixelate tables fit the plane");

struct PtRow {
    int kind, param;
    unsigned fid, stream;
};

// The row of frame f: per_clip_T = 0: row f; T: row f / T with f % T added to the frame id
__device__ __forceinline__ PtRow pt_row(const int* __restrict__ table, long f, int T) {
    const long r = T > 0 ? f / T : f;
    PtRow v;
    v.kind = table[r * 4], v.param = table[r * 4 + 1];
    v.fid = (unsigned)table[r * 4 + 2] + (T > 0 ? (unsigned)(f - r * T) : 0u);
    v.stream = (unsigned)table[r * 4 + 3];
    return v;
}

__host__ __device__ __forceinline__ int pt_strips(int hw) {
    const int s = (hw + PT_STRIP_PIXELS - 1) / PT_STRIP_PIXELS;
    return s < PT_MAX_STRIPS ? s : PT_MAX_STRIPS;
}

__device__ __forceinline__ int pt_byte(int v) { return min(max(v, 0), 255); }
__device__ __forceinline__ int pt_luma(int r, int g, int b) { return (19595 * r + 38470 * g + 7471 * b + 32768) >> 16; }
__device__ __forceinline__ unsigned pt_pack(const int (&b)[4]) {
    return (unsigned)b[0] | (unsigned)b[1] << 8 | (unsigned)b[2] << 16 | (unsigned)b[3] << 24;
}

// Contrast: part[f][s] = the sum of Y over pixels [s * len, (s + 1) * len) of frame f, len = ceil(HW / strips).  A lane adds
// at most 2^28 / 32 / 256 pixels (8.4e6 < 2^32); the workgroup's sum is kept in 64 bits.
__global__ __launch_bounds__(256) void perturb_mean_kernel(const uint8_t* __restrict__ x, const int* __restrict__ table, int T,
                                                           unsigned long long* __restrict__ part, int HW, int strips) {
    __shared__ unsigned long long red[256];
    const int tid = threadIdx.x;
    const long f = blockIdx.x / strips;
    const int s = (int)(blockIdx.x - f * strips);
    if (pt_row(table, f, T).kind != 2) return;                   // the whole workgroup
    const int len = (HW + strips - 1) / strips;
    const int lo = s * len, hi = min(lo + len, HW);
    const uint8_t* fp = x + f * (long)HW * 3;
    unsigned sum = 0;
    for (int i = lo + tid; i < hi; i += 256) sum += (unsigned)pt_luma(fp[3L * i], fp[3L * i + 1], fp[3L * i + 2]);
    red[tid] = sum;
    __syncthreads();
#pragma unroll
    for (int w = 128; w > 0; w >>= 1) {
        if (tid < w) red[tid] += red[tid + w];
        __syncthreads();
    }
    if (tid == 0) part[f * strips + s] = red[0];
}

// 4 consecutive pixels of the batch per lane.  io4 bit 0: the input may be read as dwords, bit 1: the output written as dwords
__global__ __launch_bounds__(256) void perturb_point_kernel(const uint8_t* __restrict__ x, const int* __restrict__ table, int T,
                                                            const unsigned long long* __restrict__ part, int strips, unsigned k0,
                                                            unsigned k1, uint8_t* __restrict__ out, long npix, int HW, int io4) {
    const long p0 = ((long)blockIdx.x * 256 + threadIdx.x) * 4;
    if (p0 >= npix) return;
    long f = p0 / HW;
    int rest = (int)(p0 - f * HW);                               // the pixel's index in its frame: y W + x
    const int cnt = (int)min(4L, npix - p0);
    PtRow row;
    int mean = 0;
    auto frame = [&]() {                                         // the frame's row, once per group (and per frame it enters)
        row = pt_row(table, f, T);
        if (row.kind == 2) {
            unsigned long long s = 0;
            for (int i = 0; i < strips; ++i) s += part[f * strips + i];
            mean = (int)((s + (unsigned long long)(HW / 2)) / (unsigned long long)HW);
        }
    };
    frame();
    int v[12];
    const uint8_t* src = x + p0 * 3;
    if ((io4 & 1) && cnt == 4) {
        const unsigned* s4 = reinterpret_cast<const unsigned*>(src);
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const unsigned w = s4[j];
            v[4 * j] = w & 255, v[4 * j + 1] = (w >> 8) & 255, v[4 * j + 2] = (w >> 16) & 255, v[4 * j + 3] = w >> 24;
        }
    } else {
#pragma unroll
        for (int j = 0; j < 12; ++j) v[j] = j < 3 * cnt ? src[j] : 0;
    }
    int o[12];
    unsigned skip = 0;                                           // pixels of frames the tile kernel writes
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (j < cnt) {
            const int p = row.param;
            const int y = pt_luma(v[3 * j], v[3 * j + 1], v[3 * j + 2]);
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const int u = v[3 * j + c];
                int w = u;
                if (row.kind == 1) {
                    w = pt_byte((u * p + 128) >> 8);
                } else if (row.kind == 2) {
                    w = pt_byte(mean + (((u - mean) * p + 128) >> 8));
                } else if (row.kind == 3) {
                    w = pt_byte(y + (((u - y) * p + 128) >> 8));
                } else if (row.kind == 4) {
                    unsigned r[4];
                    philox4x32_10((unsigned)rest * 3u + c, row.fid, row.stream, 0u, k0, k1, r);
                    unsigned z = 0;                              // v_sad_u8 against 0: the four bytes of a word added up
#pragma unroll
                    for (int i = 0; i < 4; ++i) z = __builtin_amdgcn_sad_u8(r[i], 0u, z);
                    w = pt_byte(u + ((((int)z - 2040) * p * 887 + (1 << 21)) >> 22));
                }
                o[3 * j + c] = w;
            }
            if (row.kind == 5 || row.kind == 6) skip |= 1u << j;
            if (++rest == HW) {
                rest = 0, ++f;
                if (j + 1 < cnt) frame();
            }
        } else {
            o[3 * j] = o[3 * j + 1] = o[3 * j + 2] = 0;
        }
    }
    uint8_t* dst = out + p0 * 3;
    if ((io4 & 2) && cnt == 4 && skip == 0) {
        unsigned* d4 = reinterpret_cast<unsigned*>(dst);
#pragma unroll
        for (int j = 0; j < 3; ++j)
            d4[j] = (unsigned)o[4 * j] | (unsigned)o[4 * j + 1] << 8 | (unsigned)o[4 * j + 2] << 16 | (unsigned)o[4 * j + 3] << 24;
    } else {
#pragma unroll
        for (int j = 0; j < 12; ++j)
            if (j < 3 * cnt && !((skip >> (j / 3)) & 1)) dst[j] = (uint8_t)o[j];
    }
}

// Kinds 5 and 6: one tile of PT_TILE_H rows x PT_TILE_W pixels of one frame per workgroup of 256
__global__ __launch_bounds__(256) void perturb_tile_kernel(const uint8_t* __restrict__ x, long total, const int* __restrict__ table,
                                                           int T, const int* __restrict__ taps, int taps_rows,
                                                           uint8_t* __restrict__ out, int H, int W, int tiles_y, int tiles_x) {
    __shared__ __align__(16) int plane[PT_PLANE_INTS];
    __shared__ int tp[PT_TAPS + 3];
    __shared__ __align__(16) unsigned char stage[PT_STAGE_ROWS * PT_PITCH];

    const int tid = threadIdx.x;
    const int per = tiles_y * tiles_x;
    const long f = blockIdx.x / per;
    const int rem = (int)(blockIdx.x - f * per);
    const int ty0 = (rem / tiles_x) * PT_TILE_H, tx0 = (rem % tiles_x) * PT_TILE_W;
    const PtRow row = pt_row(table, f, T);
    if (row.kind != 5 && row.kind != 6) return;                  // the whole workgroup: perturb_point_kernel writes this frame

    const int rstride = W * 3;
    const int th = min(PT_TILE_H, H - ty0), tw = min(PT_TILE_W, W - tx0);       // the tile's part of the frame
    const int tb = tw * 3;                                       // bytes of a tile row
    uint8_t* const orow0 = out + ((f * H + ty0) * (long)W + tx0) * 3;
    // 4 bytes of tile row r from byte 4 d on: tx0 * 3 is a multiple of 4, so the row's address decides on the dword store
    auto emit = [&](int r, int d, const int (&b)[4]) {
        uint8_t* dst = orow0 + (long)r * rstride + 4 * d;
        const int left = tb - 4 * d;
        if (left >= 4 && (reinterpret_cast<uintptr_t>(dst) & 3) == 0) {
            *reinterpret_cast<unsigned*>(dst) = pt_pack(b);
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (e < left) dst[e] = (uint8_t)b[e];
        }
    };

    if (row.kind == 5) {
        if (tid < PT_TAPS)                                       // no bank: the identity row
            tp[tid] = taps ? taps[min(max(row.param, 0), taps_rows - 1) * PT_TAPS + tid] : (tid == PT_RADIUS ? 2048 : 0);
        __syncthreads();
        int R = 0;                                               // the row's real radius: the halo that is staged and summed
#pragma unroll
        for (int i = 1; i <= PT_RADIUS; ++i)
            if (tp[PT_RADIUS + i] | tp[PT_RADIUS - i]) R = i;
        const int sy0 = max(ty0 - R, 0), sy1 = min(ty0 + th + R, H), sx0 = max(tx0 - R, 0), sx1 = min(tx0 + tw + R, W);
        const int rows = sy1 - sy0, cols = sx1 - sx0;            // <= 36 x 84
        const int lead0 = u8_stage_rows(x, total, ((f * H + sy0) * (long)W + sx0) * 3, rstride, rows, cols, stage, PT_PITCH, tid, 256);
        __syncthreads();
        // A tap is at most 2048, a byte 255 and a horizontal sum 255 * 2048 < 2^23: the products are 24-bit multiplies.
        // horizontal: staged row r, byte b of the tile row (pixel b / 3) -> plane[r][b], unrounded
        for (int item = tid; item < rows * PT_ROW_INTS; item += 256) {
            const int r = item / PT_ROW_INTS, b = item - r * PT_ROW_INTS;
            if (b >= tb) continue;
            const int c = b / 3, ch = b - 3 * c;
            const unsigned char* sr = stage + r * PT_PITCH + u8_row_lead(lead0, r, rstride) + ch;
            int acc = 0;
            for (int i = -R; i <= R; ++i) acc += __mul24(tp[PT_RADIUS + i], sr[(min(max(tx0 + c + i, 0), W - 1) - sx0) * 3]);
            plane[item] = acc;
        }
        __syncthreads();
        // vertical: 4 bytes of a tile row per item; consecutive lanes read consecutive 16 bytes of the plane
        for (int item = tid; item < th * (PT_ROW_INTS / 4); item += 256) {
            const int r = item / (PT_ROW_INTS / 4), d = item - r * (PT_ROW_INTS / 4);
            if (4 * d >= tb) continue;
            int acc[4] = {0, 0, 0, 0};
            for (int j = -R; j <= R; ++j) {
                const int t = tp[PT_RADIUS + j];
                const int4 h = *reinterpret_cast<const int4*>(plane + (min(max(ty0 + r + j, 0), H - 1) - sy0) * PT_ROW_INTS + 4 * d);
                acc[0] += __mul24(t, h.x), acc[1] += __mul24(t, h.y), acc[2] += __mul24(t, h.z), acc[3] += __mul24(t, h.w);
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[e] = pt_byte((acc[e] + (1 << 21)) >> 22);
            emit(r, d, acc);
        }
    } else {
        const int k = min(max(row.param, 2), PT_MAX_BLOCK);
        // the blocks the tile meets, cut to the frame
        const int by0 = ty0 / k * k, by1 = min((ty0 + th + k - 1) / k * k, H);
        const int bx0 = tx0 / k * k, bx1 = min((tx0 + tw + k - 1) / k * k, W);
        const int rows = min(by1 - by0, PT_STAGE_ROWS), cols = min(bx1 - bx0, PT_STAGE_COLS);
        const int nbr = (rows + k - 1) / k, nbc = (cols + k - 1) / k, nq = nbc * 3;
        const int lead0 = u8_stage_rows(x, total, ((f * H + by0) * (long)W + bx0) * 3, rstride, rows, cols, stage, PT_PITCH, tid, 256);
        __syncthreads();
        for (int item = tid; item < min(rows * nq, PT_VAL_AT); item += 256) {          // row sums per block column and channel
            const int r = item / nq, q = item - r * nq;
            const int bc = q / 3, ch = q - 3 * bc;
            const unsigned char* sr = stage + r * PT_PITCH + u8_row_lead(lead0, r, rstride) + ch;
            const int c1 = min(bc * k + k, cols);
            int s = 0;
            for (int c = bc * k; c < c1; ++c) s += sr[c * 3];
            plane[item] = s;
        }
        __syncthreads();
        for (int item = tid; item < min(nbr * nq, PT_PLANE_INTS - PT_VAL_AT); item += 256) {   // block values
            const int br = item / nq, q = item - br * nq;
            const int r1 = min(br * k + k, rows), bc = q / 3;
            int s = 0;
            for (int r = br * k; r < r1; ++r) s += plane[r * nq + q];
            const int cnt = (r1 - br * k) * (min(bc * k + k, cols) - bc * k);
            plane[PT_VAL_AT + item] = (s + cnt / 2) / cnt;
        }
        __syncthreads();
        for (int item = tid; item < th * (PT_ROW_INTS / 4); item += 256) {
            const int r = item / (PT_ROW_INTS / 4), d = item - r * (PT_ROW_INTS / 4);
            if (4 * d >= tb) continue;
            const int br = (ty0 + r - by0) / k;
            int b[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int at = min(4 * d + e, tb - 1);           // bytes past the tile row are not stored
                const int c = at / 3, ch = at - 3 * c;
                b[e] = plane[PT_VAL_AT + (br * nbc + (tx0 + c - bx0) / k) * 3 + ch];
            }
            emit(r, d, b);
        }
    }
}

}  // namespace

// frames uint8 [n][H][W][3] (total bytes readable at frames; no alignment needed), table int32 [n][4] on the device, or
// [n / per_clip_T][4] when per_clip_T > 0 (frame f reads row f / per_clip_T and adds f % per_clip_T to its frame id), taps int32
// [taps_rows][21] on the device or null, seed the Philox key -> out uint8 [n][H][W][3], which must not overlap frames.
// scratch: 8-byte aligned, n * min(32, ceil(H W / 2048)) * 8 bytes (the partial sums of kind 2).
extern "C" int istvt_perturb_u8(const void* frames, long total, int n, int H, int W, const int* table, int per_clip_T,
                                const int* taps, int taps_rows, unsigned long long seed, void* scratch, long scratch_bytes,
                                void* out, hipStream_t stream) {
    if (n <= 0 || !frames || !table || !scratch || !out) return ISTVT_ERR_SHAPE;
    if (H < 1 || W < 1 || H > 16384 || W > 16384) return ISTVT_ERR_SHAPE;
    if (per_clip_T < 0 || (per_clip_T > 0 && n % per_clip_T != 0)) return ISTVT_ERR_SHAPE;
    if (taps && (taps_rows < 1 || taps_rows > 16)) return ISTVT_ERR_SHAPE;
    const int HW = H * W;
    const long npix = (long)n * HW, bytes = npix * 3;
    const int strips = pt_strips(HW);
    if (total < bytes || (reinterpret_cast<uintptr_t>(scratch) & 7) || scratch_bytes < (long)n * strips * 8) return ISTVT_ERR_SHAPE;
    const uint8_t* a = (const uint8_t*)frames;
    const uint8_t* o = (const uint8_t*)out;
    if (o < a + bytes && a < o + bytes) return ISTVT_ERR_SHAPE;              // in place: blur and pixelate read neighbours
    const int tiles_y = (H + PT_TILE_H - 1) / PT_TILE_H, tiles_x = (W + PT_TILE_W - 1) / PT_TILE_W;
    const long tiles = (long)n * tiles_y * tiles_x, groups = (npix + 1023) / 1024;
    if (tiles > 0x7fffffffL || groups > 0x7fffffffL || (long)n * strips > 0x7fffffffL) return ISTVT_ERR_SHAPE;
    hipLaunchKernelGGL(perturb_mean_kernel, dim3((unsigned)(n * strips)), dim3(256), 0, stream, a, table, per_clip_T,
                       (unsigned long long*)scratch, HW, strips);
    int rc = istvt_check_launch();
    if (rc != ISTVT_OK) return rc;
    const int io4 = (int)((reinterpret_cast<uintptr_t>(a) & 3) == 0) | (int)((reinterpret_cast<uintptr_t>(o) & 3) == 0) << 1;
    hipLaunchKernelGGL(perturb_point_kernel, dim3((unsigned)groups), dim3(256), 0, stream, a, table, per_clip_T,
                       (const unsigned long long*)scratch, strips, (unsigned)seed, (unsigned)(seed >> 32), (uint8_t*)out, npix, HW,
                       io4);
    rc = istvt_check_launch();
    if (rc != ISTVT_OK) return rc;
    hipLaunchKernelGGL(perturb_tile_kernel, dim3((unsigned)tiles), dim3(256), 0, stream, a, total, table, per_clip_T, taps,
                       taps_rows, (uint8_t*)out, H, W, tiles_y, tiles_x);
    return istvt_check_launch();
}
