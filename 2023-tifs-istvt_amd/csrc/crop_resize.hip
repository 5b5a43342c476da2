// Frames and boxes (DESIGN.md "Frames and boxes"): cut one box per frame out of decoded frames, uint8 [n][Hs][Ws][3], and
// resize it to S x S bytes with the antialiased bilinear filter of torch's interpolate(mode='bilinear',
// align_corners=False, antialias=True) on the cropped image.  Per axis, n_in = the box side, n_out = S:
//
//   scale = n_in / n_out;  sup = max(scale, 1);  c = (i + 0.5) * scale
//   lo = max(int(c - sup + 0.5), 0);  hi = min(int(c + sup + 0.5), n_in)
//   w_j = max(0, 1 - |(j - c + 0.5) / sup|) for j in [lo, hi), divided by their sum           (resize_taps, in double)
//
// horizontal pass first, kept in fp32, then the vertical pass; byte = clamp(floor(v + 0.5), 0, 255).  1 <= h, w <= 8 S, so
// an axis has at most 17 taps.  An identity box (h = w = S) has the weights 1 and 0 and reproduces the slice.
//
// Work item = (frame, R output rows).  The workgroup builds the tap tables of the S columns and of its R rows once in LDS,
// then walks its rows in passes of as many output rows as the box's scale lets the fp32 tile (TR source rows of S * 3
// floats) hold: the source rows of a pass are staged a few at a time (u8_stage_rows: row width w, not S), filtered
// horizontally into the tile, and the tile is filtered vertically into bytes in LDS, which leave as whole 16-byte chunks
// where the output range allows it.  One writer per byte, no scratch, no atomics: a second run gives the same bits, and
// the bits do not depend on R, TR or the passes (a tile row is the same sum whichever pass makes it).
#include "u8_view.h"

namespace {

constexpr int CR_TAPS = 17;                 // 2 * 8 + 1: the widest triangle at the 8 x downscale
constexpr int CR_ROWS = 8;                  // output rows per work item
constexpr int CR_LDS_TARGET = 64 * 1024;    // LDS budget: spare room up to here goes to the tile; above only if 17 rows need it
constexpr int CR_LDS_MAX = 160 * 1024;      // the CU's LDS

struct CropBox {
    int y0, x0, h, w;
};

// The box of frame f, forced into its frame and into 1 <= h, w <= 8 S (a table that was not validated can then still read
// nothing it must not, as u8_view_of does for views)
__device__ __forceinline__ CropBox crop_box_of(const int* __restrict__ boxes, long f, int Hs, int Ws, int S) {
    CropBox b;
    b.h = min(max(boxes[f * 4 + 2], 1), min(Hs, 8 * S));
    b.w = min(max(boxes[f * 4 + 3], 1), min(Ws, 8 * S));
    b.y0 = min(max(boxes[f * 4 + 0], 0), Hs - b.h);
    b.x0 = min(max(boxes[f * 4 + 1], 0), Ws - b.w);
    return b;
}

// Taps of output index i of an axis n_in -> n_out, in the order of the definition and in double (the multiply and the
// divisions explicitly rounded: nothing for -ffp-contract=fast to fuse); w[k] is the weight of source index lo + k
__device__ __forceinline__ void resize_taps(int i, int n_in, int n_out, int* lo_out, int* cnt_out, float* w) {
    const double scale = __ddiv_rn((double)n_in, (double)n_out);
    const double sup = scale > 1.0 ? scale : 1.0;
    const double c = __dmul_rn((double)i + 0.5, scale);
    const int lo = max((int)(c - sup + 0.5), 0);
    const int hi = min((int)(c + sup + 0.5), n_in);
    double sum = 0.0;
    for (int j = lo; j < hi; ++j) sum += fmax(0.0, 1.0 - fabs(__ddiv_rn((double)j - c + 0.5, sup)));
    for (int k = 0; k < CR_TAPS; ++k) {
        const int j = lo + k;
        const double t = j < hi ? fmax(0.0, 1.0 - fabs(__ddiv_rn((double)j - c + 0.5, sup))) : 0.0;
        w[k] = (float)__ddiv_rn(t, sum);
    }
    *lo_out = lo;
    *cnt_out = hi - lo;
}

// LDS: col_lo[S] col_n[S] row_lo[R] row_n[R] (int) | col_w[S][17] row_w[R][17] (float) | tile[TR][S * 3] (float) |
// stage[stage_bytes]: the staged source rows of a chunk, then the output bytes of a pass
__global__ __launch_bounds__(256) void crop_resize_u8_kernel(const uint8_t* __restrict__ x, const int* __restrict__ boxes,
                                                             uint8_t* __restrict__ out, long total, int Hs, int Ws, int S,
                                                             int R, int ngroups, int TR, int stage_bytes) {
    extern __shared__ __align__(16) unsigned char smem[];
    const int S3 = S * 3;
    int* col_lo = reinterpret_cast<int*>(smem);
    int* col_n = col_lo + S;
    int* row_lo = col_n + S;
    int* row_n = row_lo + R;
    float* col_w = reinterpret_cast<float*>(row_n + R);
    float* row_w = col_w + S * CR_TAPS;
    float* tile = row_w + R * CR_TAPS;
    unsigned char* stage = reinterpret_cast<unsigned char*>(tile + (size_t)TR * S3);
    stage += (16 - (int)(reinterpret_cast<uintptr_t>(stage) & 15)) & 15;

    const int tid = threadIdx.x;
    const int grp = (int)(blockIdx.x % ngroups);
    const long f = blockIdx.x / ngroups;
    const int yb = grp * R;
    const int rows = min(R, S - yb);
    const CropBox b = crop_box_of(boxes, f, Hs, Ws, S);

    for (int i = tid; i < S + rows; i += 256) {
        if (i < S) resize_taps(i, b.w, S, col_lo + i, col_n + i, col_w + i * CR_TAPS);
        else resize_taps(yb + i - S, b.h, S, row_lo + (i - S), row_n + (i - S), row_w + (i - S) * CR_TAPS);
    }
    __syncthreads();

    const int pitch = u8_row_pitch(b.w), rstride = Ws * 3;
    const int CH = max(stage_bytes / pitch, 1);                  // the host sizes the stage for one widest row at least
    uint8_t* const obase = out + (f * S + yb) * (long)S3;         // first output byte of this work item

    for (int y = 0; y < rows;) {
        // the rows of this pass: as many as the tile holds source rows for (one always fits: at most 17 <= TR)
        const int s_lo = row_lo[y];
        int r = 1;
        while (y + r < rows && row_lo[y + r] + row_n[y + r] - s_lo <= TR) ++r;
        const int s_hi = row_lo[y + r - 1] + row_n[y + r - 1];

        for (int s0 = s_lo; s0 < s_hi; s0 += CH) {
            const int ch = min(CH, s_hi - s0);
            const long g0 = ((f * Hs + b.y0 + s0) * (long)Ws + b.x0) * 3;
            const int lead0 = u8_stage_rows(x, total, g0, rstride, ch, b.w, stage, pitch, tid, 256);
            __syncthreads();
            for (int e = tid; e < ch * S3; e += 256) {            // horizontal: (source row, output column, channel)
                const int rr = e / S3, xc = e - rr * S3;
                const int xo = xc / 3, c = xc - xo * 3;
                const unsigned char* px = stage + rr * pitch + u8_row_lead(lead0, rr, rstride) + col_lo[xo] * 3 + c;
                const float* w = col_w + xo * CR_TAPS;
                const int n = col_n[xo];
                float acc = 0.f;
                for (int k = 0; k < n; ++k) acc = fmaf(w[k], (float)px[3 * k], acc);
                tile[(size_t)(s0 - s_lo + rr) * S3 + xc] = acc;
            }
            __syncthreads();
        }

        // vertical: the pass's r * S3 output bytes are one contiguous range of `out`; they are laid down in LDS at the
        // range's own offset inside its first 16-byte piece, four per thread
        uint8_t* const o0 = obase + (long)y * S3;
        const int lead = (int)(reinterpret_cast<uintptr_t>(o0) & 15);
        const int len = r * S3;
        for (int d = tid; 4 * d < lead + len; d += 256) {
            unsigned packed = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int q = 4 * d + j - lead;
                if (q < 0 || q >= len) continue;
                const int yy = q / S3, xc = q - yy * S3;
                const float* w = row_w + (y + yy) * CR_TAPS;
                const float* t = tile + (size_t)(row_lo[y + yy] - s_lo) * S3 + xc;
                const int n = row_n[y + yy];
                float acc = 0.f;
                for (int k = 0; k < n; ++k) acc = fmaf(w[k], t[(size_t)k * S3], acc);
                const float v = fminf(fmaxf(floorf(acc + 0.5f), 0.f), 255.f);
                packed |= (unsigned)(int)v << (8 * j);
            }
            reinterpret_cast<unsigned*>(stage)[d] = packed;
        }
        __syncthreads();
        for (int ck = tid; 16 * ck < lead + len; ck += 256) {
            const int a = 16 * ck;
            if (a >= lead && a + 16 <= lead + len) {
                *reinterpret_cast<uint4*>(o0 - lead + a) = *reinterpret_cast<const uint4*>(stage + a);
            } else {
                for (int j = max(a, lead); j < min(a + 16, lead + len); ++j) o0[j - lead] = stage[j];
            }
        }
        __syncthreads();                                         // the next pass stages over these bytes
        y += r;
    }
}

}  // namespace

// frames uint8 [n][Hs][Ws][3] (total bytes readable at frames; no alignment needed), boxes int32 [n][4] = (y0, x0, h, w)
// on the device -> out uint8 [n][S][S][3].  LDS: the tables (76 bytes per column and per row), 17 tile rows at least, and a
// stage of two widest source rows or one pass of output bytes; spare room up to 64 KiB becomes more tile rows (fewer
// passes and fewer source rows filtered twice at small scales), and only a side whose 17 rows do not fit gets more, up to
// the CU's 160 KiB (S = 224 from wide frames: 72 KiB, two workgroups per CU; any S <= 480 fits).
extern "C" int istvt_crop_resize_u8(const void* frames, long total, int Hs, int Ws, const int* boxes, void* out, int n,
                                    int S, hipStream_t stream) {
    if (n <= 0 || S < 1 || S > 4096 || !frames || !boxes || !out) return ISTVT_ERR_SHAPE;
    if (Hs < 1 || Ws < 1 || Hs > 16384 || Ws > 16384) return ISTVT_ERR_SHAPE;
    if (total < (long)n * Hs * Ws * 3) return ISTVT_ERR_SHAPE;
    const int R = S < CR_ROWS ? S : CR_ROWS;
    const int S3 = S * 3;
    const int wmax = Ws < 8 * S ? Ws : 8 * S;
    int stage_bytes = 2 * u8_row_pitch(wmax);
    if (stage_bytes < ((R * S3 + 47) & ~15)) stage_bytes = (R * S3 + 47) & ~15;     // lead <= 15, whole dwords
    const long fixed = (long)(S + R) * (8 + 4 * CR_TAPS) + 16 + stage_bytes;
    const long tile_row = (long)S3 * 4;
    int TR = CR_TAPS;
    if (fixed + TR * tile_row < CR_LDS_TARGET) TR = (int)((CR_LDS_TARGET - fixed) / tile_row);
    if (TR > 8 * (R - 1) + CR_TAPS) TR = 8 * (R - 1) + CR_TAPS;            // no pass needs more
    const long lds = fixed + TR * tile_row;
    if (lds > CR_LDS_MAX) return ISTVT_ERR_SHAPE;
    const int ngroups = (S + R - 1) / R;
    const long nblocks = (long)n * ngroups;
    if (nblocks > 0x7fffffffL) return ISTVT_ERR_SHAPE;
    if (lds > 64 * 1024) {
        static std::atomic<unsigned long long> lds_raised{0};
        if (istvt_raise_lds_limit(lds_raised, reinterpret_cast<const void*>(crop_resize_u8_kernel), CR_LDS_MAX) != ISTVT_OK)
            return ISTVT_ERR_LAUNCH;
    }
    hipLaunchKernelGGL(crop_resize_u8_kernel, dim3((unsigned)nblocks), dim3(256), (size_t)lds, stream,
                       (const uint8_t*)frames, boxes, (uint8_t*)out, total, Hs, Ws, S, R, ngroups, TR, stage_bytes);
    return istvt_check_launch();
}
