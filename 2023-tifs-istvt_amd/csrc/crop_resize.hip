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
//
// Further down: whole NV12 frames to packed RGB (DESIGN.md "NV12 frames"), and the similarity warp (DESIGN.md "Aligned
// crops"), a second kernel over the same two sources: one 2 x 3 map per frame instead of a box, the same triangle in the
// rotated frame of the output, in double.
#include "istvt_hip.h"
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

// ---- where the bytes of a box come from ----------------------------------------------------------------------------------
// The kernel below is written once and instantiated per source.  A source says how many rows of a box one chunk stages
// (chunk_rows), fills the stage with the packed RGB bytes of `ch` box rows from s0 on (fill: row rr at stage + rr * pitch +
// lead(rr), lead(rr) = u8_row_lead(fill's result, rr, lead_stride())), and nothing else: the tap tables, the passes, the
// two filters and the output path do not know which source they read.

// Packed RGB frames, uint8 [n][Hs][Ws][3]: a box row is one contiguous piece of the source and is staged as it lies
struct RgbSource {
    const uint8_t* x;
    long total;
    int Hs, Ws;
    __device__ __forceinline__ int lead_stride() const { return Ws * 3; }
    __device__ __forceinline__ int chunk_rows(int stage_bytes, int pitch, int) const { return max(stage_bytes / pitch, 1); }
    __device__ __forceinline__ int fill(long f, const CropBox& b, int s0, int ch, unsigned char* stage, int pitch,
                                        unsigned char*, int tid) const {
        const long g0 = ((f * Hs + b.y0 + s0) * (long)Ws + b.x0) * 3;
        return u8_stage_rows(x, total, g0, Ws * 3, ch, b.w, stage, pitch, tid, 256);
    }
};

// NV12 (DESIGN.md "NV12 frames"): per frame Hs rows of Y, then Hs / 2 rows of Ws / 2 interleaved (Cb, Cr) pairs, `pitch`
// bytes from row to row and `fstride` from frame to frame; pixel (y, x) takes the pair (y >> 1, x >> 1).  One integer
// expression for every matrix, int32 only (|k| < 2^20 and 8-bit samples: no sum leaves 2^30):
//   yy = ky (Y - yoff);  R = clamp((yy + krv Cr' + 32768) >> 16);  G = clamp((yy - kgu Cb' - kgv Cr' + 32768) >> 16);
//   B = clamp((yy + kbu Cb' + 32768) >> 16);  Cb' = Cb - 128, Cr' = Cr - 128; arithmetic shifts, clamp to 0..255
struct Nv12Matrix {
    int ky, yoff, krv, kgu, kgv, kbu;
};

__device__ __forceinline__ int nv12_byte(int v) { return min(max(v >> 16, 0), 255); }

// channel c of a pixel
__device__ __forceinline__ int nv12_channel(const Nv12Matrix& m, int c, int y, int cb, int cr) {
    const int yy = m.ky * (y - m.yoff) + 32768;
    cb -= 128, cr -= 128;
    return nv12_byte(c == 0 ? yy + m.krv * cr : c == 1 ? yy - m.kgu * cb - m.kgv * cr : yy + m.kbu * cb);
}

// pitch of a staged raw row piece of a box of width w: lead (<= 15) + at most w + 2 bytes (the chroma pairs of w columns
// from an odd origin), in whole 16-byte pieces
__host__ __device__ __forceinline__ int nv12_raw_pitch(int w) { return ((w + 32) >> 4) << 4; }

struct Nv12Source {
    const uint8_t* x;
    long total, fstride;
    int Hs, Ws, pitch;
    Nv12Matrix m;
    int raw_bytes;
    __device__ __forceinline__ int lead_stride() const { return 0; }          // converted rows start at their pitch
    // ch box rows need ch raw Y pieces and at most ch / 2 + 1 chroma pieces: 3 ch / 2 + 1 <= the raw area's rows
    __device__ __forceinline__ int chunk_rows(int stage_bytes, int pitch_, int w) const {
        const int nr = raw_bytes / nv12_raw_pitch(w);
        return max(min(stage_bytes / pitch_, (nr - 1) * 2 / 3), 1);
    }
    __device__ __forceinline__ int fill(long f, const CropBox& b, int s0, int ch, unsigned char* stage, int spitch,
                                        unsigned char* raw, int tid) const {
        const int rp = nv12_raw_pitch(b.w);
        const int y0 = b.y0 + s0;                                  // first frame row of the chunk
        const int c0 = y0 >> 1, nc = ((y0 + ch - 1) >> 1) - c0 + 1;  // its chroma rows: two box rows share one
        const int cx0 = b.x0 >> 1, clen = 2 * (((b.x0 + b.w - 1) >> 1) - cx0 + 1);
        unsigned char* const rawc = raw + ch * rp;
        const int ly = u8_stage_byte_rows(x, total, f * fstride + (long)y0 * pitch + b.x0, pitch, ch, b.w, raw, rp, tid, 256);
        const int lc = u8_stage_byte_rows(x, total, f * fstride + (long)(Hs + c0) * pitch + 2 * cx0, pitch, nc, clen, rawc, rp,
                                          tid, 256);
        __syncthreads();
        const int q4 = (b.w + 3) >> 2;                             // four pixels = three dwords of the stage per thread
        for (int e = tid; e < ch * q4; e += 256) {
            const int rr = e / q4, q = e - rr * q4;
            const unsigned char* yrow = raw + rr * rp + u8_row_lead(ly, rr, pitch);
            const int cr_ = ((y0 + rr) >> 1) - c0;
            const unsigned char* crow = rawc + cr_ * rp + u8_row_lead(lc, cr_, pitch);
            unsigned o[3] = {0u, 0u, 0u};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int px = 4 * q + j;
                if (px >= b.w) continue;
                const int p = 2 * (((b.x0 + px) >> 1) - cx0);
                const int yv = yrow[px], cb = crow[p], cr = crow[p + 1];
#pragma unroll
                for (int c = 0; c < 3; ++c) o[(3 * j + c) >> 2] |= (unsigned)nv12_channel(m, c, yv, cb, cr) << (8 * ((3 * j + c) & 3));
            }
            unsigned* dst = reinterpret_cast<unsigned*>(stage + rr * spitch + 12 * q);
            dst[0] = o[0], dst[1] = o[1], dst[2] = o[2];
        }
        return 0;
    }
};

// LDS: col_lo[S] col_n[S] row_lo[R] row_n[R] (int) | col_w[S][17] row_w[R][17] (float) | tile[TR][S * 3] (float) |
// stage[stage_bytes]: the staged source rows of a chunk, then the output bytes of a pass | raw[src.raw_bytes] (NV12 only):
// the Y and chroma pieces of a chunk before their conversion into the stage
template <typename Src>
__global__ __launch_bounds__(256) void crop_resize_u8_kernel(const Src src, const int* __restrict__ boxes,
                                                             uint8_t* __restrict__ out, int S, int R, int ngroups, int TR,
                                                             int stage_bytes) {
    const int Hs = src.Hs, Ws = src.Ws;
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

    const int pitch = u8_row_pitch(b.w), rstride = src.lead_stride();
    const int CH = src.chunk_rows(stage_bytes, pitch, b.w);      // the host sizes the stage for one widest row at least
    uint8_t* const obase = out + (f * S + yb) * (long)S3;         // first output byte of this work item

    for (int y = 0; y < rows;) {
        // the rows of this pass: as many as the tile holds source rows for (one always fits: at most 17 <= TR)
        const int s_lo = row_lo[y];
        int r = 1;
        while (y + r < rows && row_lo[y + r] + row_n[y + r] - s_lo <= TR) ++r;
        const int s_hi = row_lo[y + r - 1] + row_n[y + r - 1];

        for (int s0 = s_lo; s0 < s_hi; s0 += CH) {
            const int ch = min(CH, s_hi - s0);
            const int lead0 = src.fill(f, b, s0, ch, stage, pitch, stage + stage_bytes, tid);
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

// Whole NV12 frames -> packed RGB.  Work item = (frame, row pair, tile of NV_TW columns): the two Y pieces and the chroma
// piece they share are staged with 16-byte loads, then every thread makes one 16-byte piece of one of the two output rows
// (a contiguous range of `out` each) and stores it whole where the range allows, byte by byte at its ends.
constexpr int NV_TW = 640;                                       // 2 rows x 1920 output bytes = 240 pieces: one per thread
constexpr int NV_RP = ((NV_TW + 32) >> 4) << 4;                  // nv12_raw_pitch(NV_TW)

__global__ __launch_bounds__(256) void nv12_to_rgb_u8_kernel(const Nv12Source src, uint8_t* __restrict__ out, int tiles) {
    __shared__ __align__(16) unsigned char raw[3 * NV_RP];
    const int tid = threadIdx.x;
    const int tile = (int)(blockIdx.x % tiles);
    const long t = blockIdx.x / tiles;
    const int pr = (int)(t % (src.Hs >> 1));
    const long f = t / (src.Hs >> 1);
    const int xa = tile * NV_TW, tw = min(NV_TW, src.Ws - xa);   // both even
    const int ly = u8_stage_byte_rows(src.x, src.total, f * src.fstride + (long)(2 * pr) * src.pitch + xa, src.pitch, 2, tw, raw,
                                      NV_RP, tid, 256);
    const int lc = u8_stage_byte_rows(src.x, src.total, f * src.fstride + (long)(src.Hs + pr) * src.pitch + xa, src.pitch, 1, tw,
                                      raw + 2 * NV_RP, NV_RP, tid, 256);
    __syncthreads();
    const int rr = tid >> 7, ck = tid & 127;                     // a row has at most (15 + 1920 + 15) / 16 = 121 pieces
    uint8_t* const o0 = out + ((f * src.Hs + 2 * pr + rr) * (long)src.Ws + xa) * 3;
    const int lead = (int)(reinterpret_cast<uintptr_t>(o0) & 15);
    const int len = tw * 3, a = 16 * ck;
    if (a >= lead + len) return;
    const unsigned char* yrow = raw + rr * NV_RP + u8_row_lead(ly, rr, src.pitch);
    const unsigned char* crow = raw + 2 * NV_RP + lc;
    unsigned w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        const int q = a + j - lead;
        if (q < 0 || q >= len) continue;
        const int px = q / 3, c = q - px * 3;
        w[j >> 2] |= (unsigned)nv12_channel(src.m, c, yrow[px], crow[px & ~1], crow[(px & ~1) + 1]) << (8 * (j & 3));
    }
    if (a >= lead && a + 16 <= lead + len) {
        *reinterpret_cast<uint4*>(o0 - lead + a) = make_uint4(w[0], w[1], w[2], w[3]);
    } else {
#pragma unroll
        for (int j = 0; j < 16; ++j)
            if (a + j >= lead && a + j < lead + len) o0[a + j - lead] = (uint8_t)(w[j >> 2] >> (8 * (j & 3)));
    }
}

// What both NV12 entries check of their source: even sizes, a pitch and a frame stride that keep every row inside `total`
static int nv12_source_of(const void* frames, long total, int Hs, int Ws, long pitch, long fstride, int n, const int* coef,
                          Nv12Source* src) {
    if (n <= 0 || !frames || !coef) return ISTVT_ERR_SHAPE;
    if (Hs < 2 || Ws < 2 || (Hs & 1) || (Ws & 1) || Hs > 16384 || Ws > 16384) return ISTVT_ERR_SHAPE;
    if (pitch < 0 || pitch > (1L << 20) || fstride < 0) return ISTVT_ERR_SHAPE;
    if (total < (long)(n - 1) * fstride + (long)(Hs + Hs / 2 - 1) * pitch + Ws) return ISTVT_ERR_SHAPE;
    if (coef[1] < 0 || coef[1] > 255) return ISTVT_ERR_SHAPE;
    for (int i = 0; i < 6; ++i)
        if (coef[i] < 0 || coef[i] >= (1 << 20)) return ISTVT_ERR_SHAPE;      // int32 holds every sum
    *src = Nv12Source{(const uint8_t*)frames, total, fstride, Hs, Ws, (int)pitch,
                      Nv12Matrix{coef[0], coef[1], coef[2], coef[3], coef[4], coef[5]}, 0};
    return ISTVT_OK;
}

// The launch both crop entries share.  LDS: the tables (76 bytes per column and per row), 17 tile rows at least, a stage of
// `srows` widest source rows or one pass of output bytes, and `raw_bytes` more for a source that converts into the stage;
// spare room up to 64 KiB becomes more tile rows (fewer passes and fewer source rows filtered twice at small scales), and
// only a side whose 17 rows do not fit gets more, up to the CU's 160 KiB.  -> ISTVT_ERR_SHAPE when that does not suffice.
template <typename Src>
static int crop_resize_launch(const Src& src, const int* boxes, void* out, int n, int S, int srows, int raw_bytes,
                              hipStream_t stream) {
    const int R = S < CR_ROWS ? S : CR_ROWS;
    const int S3 = S * 3;
    const int wmax = src.Ws < 8 * S ? src.Ws : 8 * S;
    int stage_bytes = srows * u8_row_pitch(wmax);
    if (stage_bytes < ((R * S3 + 47) & ~15)) stage_bytes = (R * S3 + 47) & ~15;     // lead <= 15, whole dwords
    const long fixed = (long)(S + R) * (8 + 4 * CR_TAPS) + 16 + stage_bytes + raw_bytes;
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
        static std::atomic<unsigned long long> lds_raised{0};              // one per instantiation
        if (istvt_raise_lds_limit(lds_raised, reinterpret_cast<const void*>(crop_resize_u8_kernel<Src>), CR_LDS_MAX) != ISTVT_OK)
            return ISTVT_ERR_LAUNCH;
    }
    hipLaunchKernelGGL(crop_resize_u8_kernel<Src>, dim3((unsigned)nblocks), dim3(256), (size_t)lds, stream, src, boxes,
                       (uint8_t*)out, S, R, ngroups, TR, stage_bytes);
    return istvt_check_launch();
}


// ---- similarity warp (DESIGN.md "Aligned crops") ---------------------------------------------------------------------
// One 2 x 3 map per frame, float32 M[f] = (m00 m01 m02; m10 m11 m12), takes the centre of output pixel (ox, oy) to the
// continuous source point c = M (ox + .5, oy + .5, 1); source pixel j covers [j, j + 1).  With u = (m00, m10), v = (m01, m11),
// e1 = u / |u|, e2 = v / |v|, s = sqrt|det|, sup = max(s, 1) and d = (jx + .5, jy + .5) - c:
//
//   w(jx, jy) = max(0, 1 - |d . e1| / sup) * max(0, 1 - |d . e2| / sup)
//   value_c = sum w * frame[clamp(jy, 0, Hs - 1)][clamp(jx, 0, Ws - 1)][c] / sum w;  byte = clamp(floor(value + .5), 0, 255)
//
// over every integer (jx, jy): the crop's antialiased triangle in the rotated frame of the output, the border replicated.
// Positions, weights and the four sums are double (under rotation every output pixel has its own sub-pixel phase: no
// per-axis table exists, and float32 sums over up to ~260 taps would be good to 4e-3 only).
//
// Work item = (frame, output tile), 256 threads: 16 x 16 pixels with one thread each while s <= 4, 8 x 8 with four threads
// each above (thread q takes the tap rows jy_lo + q, + 4, ...; the four are neighbouring lanes of one wave, and lane q = 0
// adds their partial sums, fetched with shuffles, in the order of q).  The tile's footprint -- the bounding rectangle of its pixels' tap ranges, clamped into the frame, never empty
// and never larger than WS_SPAN x WS_SPAN for a similarity with s <= 8 -- is staged once as packed RGB through the same
// Src::fill the crop uses (an NV12 pixel is converted once per tile, not once per tap); taps read the stage at
// coordinates clamped into that rectangle, which for a similarity is the clamp into the frame.  A block walks the tiles of
// its frame in a strided loop: the grid does not depend on the table.  One writer per byte, no atomics, no scratch.
//
// The kernel's own check of an entry (a table that was not validated reads nothing it must not): every number finite,
// 2^-6 <= s <= 8, |u| and |v| in [2^-7, 16], the image of the output centre inside [0, Ws] x [0, Hs].  An entry that fails
// gives a frame of zeros and nothing of that frame is read.  A sheared entry that passes gives defined garbage: its tap
// ranges follow sup and its rectangle is cut to WS_SPAN.
constexpr int WS_SPAN = 108;               // (7 * 8 + 2 * 8) * sqrt 2 + margins = 105 at s = 8, 100 at s = 4 with 16 x 16
constexpr int WS_RAW_PIECES = 48;          // NV12: row pieces of the raw area (31 rectangle rows per chunk)

struct WarpMap {
    double m00, m01, m02, m10, m11, m12;   // the entry
    double g1x, g1y, g2x, g2y;             // e1 / sup, e2 / sup
    double Rx, Ry;                         // half width of a pixel's tap range per source axis
    double s;
    bool ok;
};

__device__ __forceinline__ WarpMap warp_map_of(const float* __restrict__ M, long f, int Hs, int Ws, int S) {
    WarpMap w;
    const float* m = M + f * 6;
    bool fin = true;
#pragma unroll
    for (int i = 0; i < 6; ++i) fin = fin && fabsf(m[i]) <= 3.402823466e38f;     // FLT_MAX: false for NaN and the infinities
    w.m00 = m[0], w.m01 = m[1], w.m02 = m[2], w.m10 = m[3], w.m11 = m[4], w.m12 = m[5];
    const double det = __dsub_rn(__dmul_rn(w.m00, w.m11), __dmul_rn(w.m01, w.m10));      // the products are exact
    w.s = __dsqrt_rn(fabs(det));
    const double nu = __dsqrt_rn(__dadd_rn(__dmul_rn(w.m00, w.m00), __dmul_rn(w.m10, w.m10)));
    const double nv = __dsqrt_rn(__dadd_rn(__dmul_rn(w.m01, w.m01), __dmul_rn(w.m11, w.m11)));
    const double h = 0.5 * (double)S;
    const double px = __dadd_rn(__dadd_rn(__dmul_rn(w.m00, h), __dmul_rn(w.m01, h)), w.m02);
    const double py = __dadd_rn(__dadd_rn(__dmul_rn(w.m10, h), __dmul_rn(w.m11, h)), w.m12);
    w.ok = fin && w.s >= 0.015625 && w.s <= 8.0 && nu >= 0.0078125 && nu <= 16.0 && nv >= 0.0078125 && nv <= 16.0 &&
           px >= 0.0 && px <= (double)Ws && py >= 0.0 && py <= (double)Hs;
    if (!w.ok) return w;
    const double sup = w.s > 1.0 ? w.s : 1.0;
    const double e1x = __ddiv_rn(w.m00, nu), e1y = __ddiv_rn(w.m10, nu);
    const double e2x = __ddiv_rn(w.m01, nv), e2y = __ddiv_rn(w.m11, nv);
    w.g1x = __ddiv_rn(e1x, sup), w.g1y = __ddiv_rn(e1y, sup);
    w.g2x = __ddiv_rn(e2x, sup), w.g2y = __ddiv_rn(e2y, sup);
    // |d . e1|, |d . e2| < sup puts |dx| below sup (|e1x| + |e2x|) when e1 and e2 are orthogonal; the margin covers the
    // 1e-4 a validated table may be off, and .5 turns pixel centres into indices
    w.Rx = sup * (fabs(e1x) + fabs(e2x)) * 1.001 + 0.51;
    w.Ry = sup * (fabs(e1y) + fabs(e2y)) * 1.001 + 0.51;
    return w;
}

__device__ __forceinline__ double warp_cx(const WarpMap& w, double px, double py) {
    return __dadd_rn(__dadd_rn(__dmul_rn(w.m00, px), __dmul_rn(w.m01, py)), w.m02);
}
__device__ __forceinline__ double warp_cy(const WarpMap& w, double px, double py) {
    return __dadd_rn(__dadd_rn(__dmul_rn(w.m10, px), __dmul_rn(w.m11, py)), w.m12);
}

// LDS: the frame's WarpMap (static: thread 0 works it out -- three square roots, eight divisions -- and all read it) |
// stage[stage_bytes]: the rectangle | raw[src.raw_bytes] (NV12 only)
template <typename Src>
__global__ __launch_bounds__(256) void warp_similarity_kernel(const Src src, const float* __restrict__ M,
                                                              uint8_t* __restrict__ out, int S, int G, int stage_bytes) {
    const int Hs = src.Hs, Ws = src.Ws;
    extern __shared__ __align__(16) unsigned char smem[];
    unsigned char* stage = smem;
    __shared__ WarpMap shared_map;

    const int tid = threadIdx.x;
    const long f = blockIdx.x / G;
    const int t0 = (int)(blockIdx.x % G);
    if (tid == 0) shared_map = warp_map_of(M, f, Hs, Ws, S);
    __syncthreads();
    const WarpMap w = shared_map;
    const bool wide = w.ok && w.s > 4.0;                         // 8 x 8 tiles, four threads per pixel
    const int P = wide ? 8 : 16, Q = wide ? 4 : 1;
    const int tp = (S + P - 1) / P;
    const int pid = tid / Q, q = tid - pid * Q;
    const int ly = pid / P, lx = pid - ly * P;
    uint8_t* const obase = out + f * (long)S * S * 3;

    for (int t = t0; t < tp * tp; t += G) {
        const int ty = t / tp, tx = t - ty * tp;
        const int ox0 = tx * P, oy0 = ty * P;
        const int ox = ox0 + lx, oy = oy0 + ly;
        const bool live = ox < S && oy < S;
        if (!w.ok) {
            if (live) {
                uint8_t* o = obase + ((long)oy * S + ox) * 3;
                o[0] = 0, o[1] = 0, o[2] = 0;
            }
            continue;
        }
        // the rectangle: the map is affine, so the centres of the tile's corner pixels bound those of all its pixels
        const double xa = (double)ox0 + 0.5, xb = (double)min(ox0 + P, S) - 0.5;
        const double ya = (double)oy0 + 0.5, yb = (double)min(oy0 + P, S) - 0.5;
        const double c0 = warp_cx(w, xa, ya), c1 = warp_cx(w, xb, ya), c2 = warp_cx(w, xa, yb), c3 = warp_cx(w, xb, yb);
        const double r0 = warp_cy(w, xa, ya), r1 = warp_cy(w, xb, ya), r2 = warp_cy(w, xa, yb), r3 = warp_cy(w, xb, yb);
        const int x_lo = (int)floor(fmin(fmin(c0, c1), fmin(c2, c3)) - w.Rx);
        const int x_hi = (int)floor(fmax(fmax(c0, c1), fmax(c2, c3)) + w.Rx);
        const int y_lo = (int)floor(fmin(fmin(r0, r1), fmin(r2, r3)) - w.Ry);
        const int y_hi = (int)floor(fmax(fmax(r0, r1), fmax(r2, r3)) + w.Ry);
        CropBox b;
        b.x0 = min(max(x_lo, 0), Ws - 1);
        b.y0 = min(max(y_lo, 0), Hs - 1);
        b.w = min(min(max(x_hi, 0), Ws - 1) - b.x0 + 1, WS_SPAN);
        b.h = min(min(max(y_hi, 0), Hs - 1) - b.y0 + 1, WS_SPAN);

        const int pitch = u8_row_pitch(b.w), rstride = src.lead_stride();
        const int CH = src.chunk_rows(stage_bytes, pitch, b.w);  // the host sizes the stage for WS_SPAN widest rows
        int lead0 = 0;
        for (int s0 = 0; s0 < b.h; s0 += CH) {
            const int l = src.fill(f, b, s0, min(CH, b.h - s0), stage + s0 * pitch, pitch, stage + stage_bytes, tid);
            if (s0 == 0) lead0 = l;
            __syncthreads();                                     // the next chunk converts from the same raw area
        }

        double sw = 0.0, a0 = 0.0, a1 = 0.0, a2 = 0.0;
        if (live) {
            const double cx = warp_cx(w, (double)ox + 0.5, (double)oy + 0.5);
            const double cy = warp_cy(w, (double)ox + 0.5, (double)oy + 0.5);
            const int jx_lo = (int)floor(cx - w.Rx), jx_hi = (int)floor(cx + w.Rx);
            const int jy_lo = (int)floor(cy - w.Ry), jy_hi = (int)floor(cy + w.Ry);
            const int xe = b.x0 + b.w - 1, ye = b.y0 + b.h - 1;
            for (int jy = jy_lo + q; jy <= jy_hi; jy += Q) {
                const int sy = min(max(jy, b.y0), ye) - b.y0;
                const unsigned char* row = stage + sy * pitch + u8_row_lead(lead0, sy, rstride);
                const double dy = __dsub_rn((double)jy + 0.5, cy);
                const double ay = __dmul_rn(dy, w.g1y), by = __dmul_rn(dy, w.g2y);
                for (int jx = jx_lo; jx <= jx_hi; ++jx) {
                    const double dx = __dsub_rn((double)jx + 0.5, cx);
                    const double wa = 1.0 - fabs(__fma_rn(dx, w.g1x, ay));
                    const double wb = 1.0 - fabs(__fma_rn(dx, w.g2x, by));
                    if (wa <= 0.0 || wb <= 0.0) continue;
                    const double wt = __dmul_rn(wa, wb);
                    const unsigned char* p = row + (min(max(jx, b.x0), xe) - b.x0) * 3;
                    sw = __dadd_rn(sw, wt);
                    a0 = __fma_rn(wt, (double)p[0], a0);
                    a1 = __fma_rn(wt, (double)p[1], a1);
                    a2 = __fma_rn(wt, (double)p[2], a2);
                }
            }
        }
        if (Q == 4) {                                            // every lane shuffles; what lanes q != 0 get is not used
            const double own[4] = {sw, a0, a1, a2};
#pragma unroll
            for (int k = 1; k < 4; ++k) {                        // the sums of lane q = k, fetched from the lanes' own values
                sw = __dadd_rn(sw, __shfl_down(own[0], k));
                a0 = __dadd_rn(a0, __shfl_down(own[1], k));
                a1 = __dadd_rn(a1, __shfl_down(own[2], k));
                a2 = __dadd_rn(a2, __shfl_down(own[3], k));
            }
        }
        if (live && q == 0) {
            uint8_t* o = obase + ((long)oy * S + ox) * 3;
            const double acc[3] = {a0, a1, a2};
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const double v = sw > 0.0 ? __ddiv_rn(acc[c], sw) : 0.0;
                o[c] = (uint8_t)(int)fmin(fmax(floor(v + 0.5), 0.0), 255.0);
            }
        }
        __syncthreads();                                         // the next tile stages over these bytes
    }
}

static int src_raw_bytes(const RgbSource&) { return 0; }
static int src_raw_bytes(const Nv12Source& s) { return s.raw_bytes; }

// The launch both warp entries share: n * G blocks, G = the 16 x 16 tiles of an output.  LDS: a stage of min(Hs, WS_SPAN)
// rows of min(Ws, WS_SPAN) pixels (at most 37.1 KiB) and the source's raw area, next to the kernel's static WarpMap.
template <typename Src>
static int warp_similarity_launch(const Src& src, const float* M, void* out, int n, int S, hipStream_t stream) {
    const int wcap = src.Ws < WS_SPAN ? src.Ws : WS_SPAN, hcap = src.Hs < WS_SPAN ? src.Hs : WS_SPAN;
    const int stage_bytes = hcap * u8_row_pitch(wcap);
    const long lds = (long)stage_bytes + src_raw_bytes(src);
    const int tp = (S + 15) / 16;
    const int G = tp * tp;
    const long nblocks = (long)n * G;
    if (nblocks > 0x7fffffffL) return ISTVT_ERR_SHAPE;
    hipLaunchKernelGGL(warp_similarity_kernel<Src>, dim3((unsigned)nblocks), dim3(256), (size_t)lds, stream, src, M,
                       (uint8_t*)out, S, G, stage_bytes);
    return istvt_check_launch();
}

}  // namespace

// frames uint8 [n][Hs][Ws][3] (total bytes readable at frames; no alignment needed), boxes int32 [n][4] = (y0, x0, h, w)
// on the device -> out uint8 [n][S][S][3].  LDS as crop_resize_launch says, with a stage of two widest source rows and no
// raw area (S = 224 from wide frames: 72 KiB, two workgroups per CU; any S <= 480 fits).
extern "C" int istvt_crop_resize_u8(const void* frames, long total, int Hs, int Ws, const int* boxes, void* out, int n,
                                    int S, hipStream_t stream) {
    if (n <= 0 || S < 1 || S > 4096 || !frames || !boxes || !out) return ISTVT_ERR_SHAPE;
    if (Hs < 1 || Ws < 1 || Hs > 16384 || Ws > 16384) return ISTVT_ERR_SHAPE;
    if (total < (long)n * Hs * Ws * 3) return ISTVT_ERR_SHAPE;
    return crop_resize_launch(RgbSource{(const uint8_t*)frames, total, Hs, Ws}, boxes, out, n, S, 2, 0, stream);
}

// The same from NV12 frames (n frames of Hs + Hs / 2 rows of Ws bytes, `pitch` bytes from row to row, `fstride` from frame
// to frame, `total` bytes readable at frames; Hs, Ws even, no alignment needed; coef = ky, yoff, krv, kgu, kgv, kbu on the
// host): the bits of istvt_crop_resize_u8 on istvt_nv12_to_rgb_u8's frames, which are never made.  LDS: the RGB entry's,
// plus a raw area of three row pieces of nv12_raw_pitch(widest box) = min(Ws, 8 S) + 32 bytes (two Y rows and the chroma
// row they share; narrower boxes stage more rows per chunk): S = 224 from wide frames 77.7 KiB, still two workgroups per
// CU.  Where that does not fit the CU (S > 440 from frames wider than 8 S), the stage and the raw area shrink to one source
// row each (one Y and one chroma piece), so any S <= 480 fits here too.
extern "C" int istvt_crop_resize_nv12(const void* frames, long total, int Hs, int Ws, long pitch, long fstride, const int* coef,
                                      const int* boxes, void* out, int n, int S, hipStream_t stream) {
    if (S < 1 || S > 4096 || !boxes || !out) return ISTVT_ERR_SHAPE;
    Nv12Source src;
    const int rc = nv12_source_of(frames, total, Hs, Ws, pitch, fstride, n, coef, &src);
    if (rc != ISTVT_OK) return rc;
    const int rp = nv12_raw_pitch(Ws < 8 * S ? Ws : 8 * S);
    src.raw_bytes = 3 * rp;
    const int r3 = crop_resize_launch(src, boxes, out, n, S, 2, src.raw_bytes, stream);
    if (r3 != ISTVT_ERR_SHAPE) return r3;
    src.raw_bytes = 2 * rp;
    return crop_resize_launch(src, boxes, out, n, S, 1, src.raw_bytes, stream);
}

// NV12 frames as above -> out uint8 [n][Hs][Ws][3], contiguous, no alignment needed, no overlap with the frames
extern "C" int istvt_nv12_to_rgb_u8(const void* frames, long total, int Hs, int Ws, long pitch, long fstride, const int* coef,
                                    void* out, int n, hipStream_t stream) {
    if (!out) return ISTVT_ERR_SHAPE;
    Nv12Source src;
    const int rc = nv12_source_of(frames, total, Hs, Ws, pitch, fstride, n, coef, &src);
    if (rc != ISTVT_OK) return rc;
    const int tiles = (Ws + NV_TW - 1) / NV_TW;
    const long nblocks = (long)n * (Hs / 2) * tiles;
    if (nblocks > 0x7fffffffL) return ISTVT_ERR_SHAPE;
    hipLaunchKernelGGL(nv12_to_rgb_u8_kernel, dim3((unsigned)nblocks), dim3(256), 0, stream, src, (uint8_t*)out, tiles);
    return istvt_check_launch();
}

// Similarity warp: frames as istvt_crop_resize_u8 takes them, M float32 [n][2][3] on the device (the map of every frame, as
// the comment above warp_similarity_kernel defines it) -> out uint8 [n][S][S][3].  An entry that fails the kernel's check
// gives zeros.
extern "C" int istvt_warp_similarity_u8(const void* frames, long total, int Hs, int Ws, const float* M, void* out, int n,
                                        int S, hipStream_t stream) {
    if (n <= 0 || S < 1 || S > 4096 || !frames || !M || !out) return ISTVT_ERR_SHAPE;
    if (Hs < 1 || Ws < 1 || Hs > 16384 || Ws > 16384) return ISTVT_ERR_SHAPE;
    if (total < (long)n * Hs * Ws * 3) return ISTVT_ERR_SHAPE;
    return warp_similarity_launch(RgbSource{(const uint8_t*)frames, total, Hs, Ws}, M, out, n, S, stream);
}

// The same from NV12 frames as istvt_crop_resize_nv12 takes them: the bits of istvt_warp_similarity_u8 on
// istvt_nv12_to_rgb_u8's frames, which are never made.  The raw area holds WS_RAW_PIECES row pieces of the widest rectangle.
extern "C" int istvt_warp_similarity_nv12(const void* frames, long total, int Hs, int Ws, long pitch, long fstride,
                                          const int* coef, const float* M, void* out, int n, int S, hipStream_t stream) {
    if (S < 1 || S > 4096 || !M || !out) return ISTVT_ERR_SHAPE;
    Nv12Source src;
    const int rc = nv12_source_of(frames, total, Hs, Ws, pitch, fstride, n, coef, &src);
    if (rc != ISTVT_OK) return rc;
    src.raw_bytes = WS_RAW_PIECES * nv12_raw_pitch(Ws < WS_SPAN ? Ws : WS_SPAN);
    return warp_similarity_launch(src, M, out, n, S, stream);
}
