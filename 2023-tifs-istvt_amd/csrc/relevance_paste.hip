// Pasting relevance maps onto whole frames (DESIGN.md "Pasting maps onto frames"), in place, in the frame's own format.
//
// Per frame f: a g x g float32 map (g <= 19, crop coordinates), a 2 x 3 double map A that takes the CENTRE of source pixel
// (sx, sy) to crop coordinates,  u = (a00 (sx + .5) + a01 (sy + .5)) + a02,  v likewise with the second row, the crop
// covering [0, S) x [0, S); a rectangle (y0, x0, h, w) that says where to look; a weight alpha.  clips.paste_maps_host is
// the definition:
//
//   mhat = (map - min) / (max - min) over the cells, in double (a constant map pastes nothing)
//   in the region (0 <= u < S, 0 <= v < S): gu = u (g / S) - .5, gv likewise; x = floor(gu), fx = gu - x; the cells at
//   clamp(x), clamp(x + 1), clamp(y), clamp(y + 1); a + fx (b - a) along x for both rows, then along y: m
//   k = clamp(floor(255 m + .5), 0, 255);  w = clamp(floor((256 alpha) m + .5), 0, 256);  outside the region w = 0
//   packed RGB:  out_c = (frame_c (256 - w) + lut[k][c] w + 128) >> 8
//   NV12:        Y_out = (Y (256 - w) + lut[k][0] w + 128) >> 8 per pixel; per 2 x 2 block with its four (k_i, w_i)
//                C_out = (C (1024 - sum w_i) + sum w_i lut[k_i][c] + 512) >> 10 for Cb (c = 1) and Cr (c = 2)
//
// Every double operation is one explicitly rounded intrinsic, in the host's order, so (k, w) are the host's wherever 255 m
// and 256 alpha m are not within rounding of a half-integer; the blend is int32.
//
// Work item = (frame, tile).  A tile is TR rows (NV12: row pairs) of PASTE_CHUNKS 16-byte chunks each, the chunks counted
// from the 16-byte boundary at or below the rectangle's first byte of that row: tiles own whole aligned chunks, so no two
// blocks ever touch one byte.  Phase 1: one (k, w) per pixel that has a byte in the tile, into LDS (a packed RGB pixel that
// straddles two tiles is worked out by both, to the same bits).  Phase 2: one thread per (row, chunk) blends its 16 bytes --
// one 16-byte load and store where the chunk lies whole inside the row's span, byte by byte at the ragged ends -- and stores
// only where some weight is not zero.  NV12 threads own the 2 x 2 blocks of 16 columns: two Y chunks and the chroma chunk
// under them; that needs the three rows in one phase, i.e. a pitch that is a multiple of 16 and an even frame address, and
// runs byte by byte otherwise.  A fixed number of blocks per frame walks the tiles in a strided loop: the grid does not
// depend on the tables.  One writer per byte, no atomics, no scratch.
//
// Nothing is trusted: the rectangle is clamped into the frame here (NV12: then aligned outward to even coordinates), and a
// frame whose A, alpha or map holds a non-finite number is left untouched, as is one with a constant map or alpha <= 0.
#include "common.h"

namespace {

constexpr int PASTE_MAX_GRID = 19;
constexpr int PASTE_CHUNKS = 16;           // 16-byte chunks per tile row: 256 bytes

struct PasteRgb {                          // packed RGB, contiguous frames
    uint8_t* base;
    int Hs, Ws;
    static constexpr int BPP = 3, ROWS = 1, TR = 16;
    static constexpr int PW = 88;          // pixels with a byte in 256 bytes: 85 whole and a part at each end
    __device__ __forceinline__ uint8_t* frame(long f) const { return base + f * (long)Hs * Ws * 3; }
    __device__ __forceinline__ long pitch_of() const { return (long)Ws * 3; }
    __device__ __forceinline__ bool vector_ok(const uint8_t*) const { return true; }       // every row has its own phase
};

struct PasteNv12 {                         // NV12, pitch and frame stride as the tensor has them
    uint8_t* base;
    long fstride;
    int Hs, Ws, pitch;
    static constexpr int BPP = 1, ROWS = 2, TR = 16;
    static constexpr int PW = 256;
    __device__ __forceinline__ uint8_t* frame(long f) const { return base + f * fstride; }
    __device__ __forceinline__ long pitch_of() const { return pitch; }
    __device__ __forceinline__ bool vector_ok(const uint8_t* fp) const {
        return (pitch & 15) == 0 && (reinterpret_cast<uintptr_t>(fp) & 1) == 0;
    }
};

struct PasteMap {
    double a00, a01, a02, a10, a11, a12;
    double r;                              // g / S
    double a256;                           // 256 alpha
    double Sd;
    int g;
};

// (w << 8) | k of the pixel (sx, sy); 0 outside the region
__device__ __forceinline__ unsigned paste_wk(const PasteMap& m, const double* __restrict__ mhat, int sx, int sy) {
    const double px = (double)sx + 0.5, py = (double)sy + 0.5;
    const double u = __dadd_rn(__dadd_rn(__dmul_rn(m.a00, px), __dmul_rn(m.a01, py)), m.a02);
    const double v = __dadd_rn(__dadd_rn(__dmul_rn(m.a10, px), __dmul_rn(m.a11, py)), m.a12);
    if (!(u >= 0.0 && u < m.Sd && v >= 0.0 && v < m.Sd)) return 0u;        // false for a NaN too
    const double gu = __dsub_rn(__dmul_rn(u, m.r), 0.5), gv = __dsub_rn(__dmul_rn(v, m.r), 0.5);
    const double xf = floor(gu), yf = floor(gv);                            // in [-1, g - 1]
    const double fx = __dsub_rn(gu, xf), fy = __dsub_rn(gv, yf);
    const int g1 = m.g - 1;
    const int xi = (int)xf, yi = (int)yf;
    const int x0 = min(max(xi, 0), g1), x1 = min(max(xi + 1, 0), g1);
    const int y0 = min(max(yi, 0), g1), y1 = min(max(yi + 1, 0), g1);
    const double m00 = mhat[y0 * m.g + x0], m01 = mhat[y0 * m.g + x1];
    const double m10 = mhat[y1 * m.g + x0], m11 = mhat[y1 * m.g + x1];
    const double top = __dadd_rn(m00, __dmul_rn(fx, __dsub_rn(m01, m00)));
    const double bot = __dadd_rn(m10, __dmul_rn(fx, __dsub_rn(m11, m10)));
    const double mm = __dadd_rn(top, __dmul_rn(fy, __dsub_rn(bot, top)));
    const double kf = floor(__dadd_rn(__dmul_rn(255.0, mm), 0.5));
    const double wf = floor(__dadd_rn(__dmul_rn(m.a256, mm), 0.5));
    const unsigned k = (unsigned)(int)fmin(fmax(kf, 0.0), 255.0);
    const unsigned w = (unsigned)(int)fmin(fmax(wf, 0.0), 256.0);
    return (w << 8) | k;
}

__device__ __forceinline__ unsigned blend8(unsigned b, unsigned l, unsigned w) { return (b * (256u - w) + l * w + 128u) >> 8; }

// The span of tile column tx in a row whose rectangle bytes are [lo, hi) and whose first rectangle byte sits `phase` bytes
// above a 16-byte boundary: row byte offsets [b0, b1), empty when b0 >= b1
__device__ __forceinline__ void tile_span(int lo, int hi, int phase, int tx, int& b0, int& b1) {
    const int s = lo - phase + tx * (16 * PASTE_CHUNKS);
    b0 = max(s, lo);
    b1 = min(s + 16 * PASTE_CHUNKS, hi);
}

// ---- phase 2, packed RGB: thread (r, c) blends chunk c of tile row r -----------------------------------------------------
__device__ __forceinline__ void paste_chunk(const PasteRgb&, uint8_t* fp, long pitch, int y, int, int lo, int hi, int phase,
                                            int tx, int c, bool, const unsigned* __restrict__ wk,
                                            const uint8_t* __restrict__ slut) {
    uint8_t* row = fp + (long)y * pitch;
    int t0, t1;
    tile_span(lo, hi, phase, tx, t0, t1);
    const int cs = lo - phase + tx * (16 * PASTE_CHUNKS) + 16 * c;
    const int b0 = max(cs, lo), b1 = min(cs + 16, hi);
    if (b0 >= b1) return;
    const int pfirst = t0 / 3;
    if (b1 - b0 == 16) {                                                   // row + cs is 16-byte aligned
        uint4* p = reinterpret_cast<uint4*>(row + cs);
        const uint4 in = *p;
        const unsigned src[4] = {in.x, in.y, in.z, in.w};
        unsigned dst[4], any = 0;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            unsigned o = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int bo = cs + 4 * q + j;
                const int pix = bo / 3, ch = bo - 3 * pix;
                const unsigned e = wk[pix - pfirst], w = e >> 8;
                any |= w;
                o |= blend8((src[q] >> (8 * j)) & 255u, slut[(e & 255u) * 3 + ch], w) << (8 * j);
            }
            dst[q] = o;
        }
        if (any) *p = make_uint4(dst[0], dst[1], dst[2], dst[3]);
        return;
    }
    for (int bo = b0; bo < b1; ++bo) {
        const int pix = bo / 3, ch = bo - 3 * pix;
        const unsigned e = wk[pix - pfirst], w = e >> 8;
        if (w) row[bo] = (uint8_t)blend8(row[bo], slut[(e & 255u) * 3 + ch], w);
    }
}

// ---- phase 2, NV12: thread (r, c) blends the 2 x 2 blocks of 16 columns of row pair r ------------------------------------
__device__ __forceinline__ void nv12_block(unsigned e00, unsigned e01, unsigned e10, unsigned e11,
                                           const uint8_t* __restrict__ slut, unsigned& sw, unsigned& scb, unsigned& scr) {
    const unsigned w0 = e00 >> 8, w1 = e01 >> 8, w2 = e10 >> 8, w3 = e11 >> 8;
    const uint8_t* l0 = slut + (e00 & 255u) * 3;
    const uint8_t* l1 = slut + (e01 & 255u) * 3;
    const uint8_t* l2 = slut + (e10 & 255u) * 3;
    const uint8_t* l3 = slut + (e11 & 255u) * 3;
    sw = w0 + w1 + w2 + w3;
    scb = w0 * l0[1] + w1 * l1[1] + w2 * l2[1] + w3 * l3[1];
    scr = w0 * l0[2] + w1 * l1[2] + w2 * l2[2] + w3 * l3[2];
}

__device__ __forceinline__ void paste_chunk(const PasteNv12& fr, uint8_t* fp, long pitch, int y, int, int lo, int hi,
                                            int phase, int tx, int c, bool vec, const unsigned* __restrict__ wk,
                                            const uint8_t* __restrict__ slut) {
    uint8_t* ya = fp + (long)y * pitch;                                   // y even: rows y, y + 1 and chroma row Hs + y / 2
    uint8_t* yb = ya + pitch;
    uint8_t* uv = fp + (long)(fr.Hs + (y >> 1)) * pitch;
    int t0, t1;
    tile_span(lo, hi, phase, tx, t0, t1);
    const int cs = lo - phase + tx * (16 * PASTE_CHUNKS) + 16 * c;        // even: lo and phase are
    const int b0 = max(cs, lo), b1 = min(cs + 16, hi);
    if (b0 >= b1) return;
    const unsigned* wa = wk - t0;                                          // row y of the pair; row y + 1 is PW further
    const unsigned* wb = wa + PasteNv12::PW;
    if (vec && b1 - b0 == 16) {
        const uint4 ia = *reinterpret_cast<const uint4*>(ya + cs), ib = *reinterpret_cast<const uint4*>(yb + cs);
        const uint4 ic = *reinterpret_cast<const uint4*>(uv + cs);
        const unsigned sa[4] = {ia.x, ia.y, ia.z, ia.w}, sb[4] = {ib.x, ib.y, ib.z, ib.w}, sc[4] = {ic.x, ic.y, ic.z, ic.w};
        unsigned da[4], db[4], dc[4], any = 0;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            unsigned oa = 0, ob = 0, oc = 0;
#pragma unroll
            for (int j = 0; j < 4; j += 2) {                               // the block at columns cs + 4 q + j, + 1
                const int x = cs + 4 * q + j;
                const unsigned e00 = wa[x], e01 = wa[x + 1], e10 = wb[x], e11 = wb[x + 1];
                unsigned sw, scb, scr;
                nv12_block(e00, e01, e10, e11, slut, sw, scb, scr);
                any |= sw;
                oa |= blend8((sa[q] >> (8 * j)) & 255u, slut[(e00 & 255u) * 3], e00 >> 8) << (8 * j);
                oa |= blend8((sa[q] >> (8 * j + 8)) & 255u, slut[(e01 & 255u) * 3], e01 >> 8) << (8 * j + 8);
                ob |= blend8((sb[q] >> (8 * j)) & 255u, slut[(e10 & 255u) * 3], e10 >> 8) << (8 * j);
                ob |= blend8((sb[q] >> (8 * j + 8)) & 255u, slut[(e11 & 255u) * 3], e11 >> 8) << (8 * j + 8);
                oc |= ((((sc[q] >> (8 * j)) & 255u) * (1024u - sw) + scb + 512u) >> 10) << (8 * j);
                oc |= ((((sc[q] >> (8 * j + 8)) & 255u) * (1024u - sw) + scr + 512u) >> 10) << (8 * j + 8);
            }
            da[q] = oa, db[q] = ob, dc[q] = oc;
        }
        if (any) {
            *reinterpret_cast<uint4*>(ya + cs) = make_uint4(da[0], da[1], da[2], da[3]);
            *reinterpret_cast<uint4*>(yb + cs) = make_uint4(db[0], db[1], db[2], db[3]);
            *reinterpret_cast<uint4*>(uv + cs) = make_uint4(dc[0], dc[1], dc[2], dc[3]);
        }
        return;
    }
    for (int x = b0; x < b1; x += 2) {
        const unsigned e00 = wa[x], e01 = wa[x + 1], e10 = wb[x], e11 = wb[x + 1];
        unsigned sw, scb, scr;
        nv12_block(e00, e01, e10, e11, slut, sw, scb, scr);
        if (!sw) continue;
        ya[x] = (uint8_t)blend8(ya[x], slut[(e00 & 255u) * 3], e00 >> 8);
        ya[x + 1] = (uint8_t)blend8(ya[x + 1], slut[(e01 & 255u) * 3], e01 >> 8);
        yb[x] = (uint8_t)blend8(yb[x], slut[(e10 & 255u) * 3], e10 >> 8);
        yb[x + 1] = (uint8_t)blend8(yb[x + 1], slut[(e11 & 255u) * 3], e11 >> 8);
        uv[x] = (uint8_t)(((unsigned)uv[x] * (1024u - sw) + scb + 512u) >> 10);
        uv[x + 1] = (uint8_t)(((unsigned)uv[x + 1] * (1024u - sw) + scr + 512u) >> 10);
    }
}

// LDS: the raw map, the normalised map (double), the colour table, one (w << 8) | k per pixel of the tile: 11.5 KiB for
// packed RGB, 38 KiB for NV12
template <typename Fmt>
__global__ __launch_bounds__(256) void relevance_paste_kernel(const Fmt fr, const float* __restrict__ maps, int g,
                                                              const double* __restrict__ A, const int* __restrict__ rect,
                                                              const uint8_t* __restrict__ lut,
                                                              const float* __restrict__ alpha, int S, int G) {
    constexpr int BPP = Fmt::BPP, ROWS = Fmt::ROWS, TR = Fmt::TR, PW = Fmt::PW;
    __shared__ double mhat[PASTE_MAX_GRID * PASTE_MAX_GRID];
    __shared__ float raw[PASTE_MAX_GRID * PASTE_MAX_GRID];
    __shared__ __align__(16) uint8_t slut[768];
    __shared__ unsigned wk[TR * ROWS * PW];

    const int tid = threadIdx.x;
    const long f = blockIdx.x / G;
    const int t0 = (int)(blockIdx.x % G);
    const int gg = g * g;
    for (int i = tid; i < gg; i += 256) raw[i] = maps[f * gg + i];
    for (int i = tid; i < 768; i += 256) slut[i] = lut[i];
    __syncthreads();

    // every thread walks the whole map: min and max of floats are exact in any order, and all threads agree
    float mn = raw[0], mx = raw[0];
    bool fin = true;
    for (int i = 0; i < gg; ++i) {
        const float v = raw[i];
        fin = fin && fabsf(v) <= 3.402823466e38f;                          // false for NaN and the infinities
        mn = fminf(mn, v), mx = fmaxf(mx, v);
    }
    PasteMap m;
    const double* a = A + f * 6;
    m.a00 = a[0], m.a01 = a[1], m.a02 = a[2], m.a10 = a[3], m.a11 = a[4], m.a12 = a[5];
#pragma unroll
    for (int i = 0; i < 6; ++i) fin = fin && fabs(a[i]) <= 1.7976931348623157e308;
    const float al = alpha[f];
    fin = fin && fabsf(al) <= 3.402823466e38f;
    if (!fin || !(mx > mn) || !(al > 0.0f)) return;                        // the whole block: nothing of the frame is touched
    m.a256 = __dmul_rn(256.0, (double)al);
    m.r = __ddiv_rn((double)g, (double)S);
    m.Sd = (double)S;
    m.g = g;
    const double dmn = (double)mn, range = __dsub_rn((double)mx, dmn);
    for (int i = tid; i < gg; i += 256) mhat[i] = __ddiv_rn(__dsub_rn((double)raw[i], dmn), range);
    __syncthreads();

    // the rectangle, clamped into the frame; NV12: aligned outward to even coordinates (Hs and Ws are even)
    const int* rc = rect + f * 4;
    const int Hs = fr.Hs, Ws = fr.Ws;
    int y0 = (int)min(max((long)rc[0], 0L), (long)Hs), x0 = (int)min(max((long)rc[1], 0L), (long)Ws);
    int y1 = (int)min(max((long)rc[0] + rc[2], (long)y0), (long)Hs), x1 = (int)min(max((long)rc[1] + rc[3], (long)x0), (long)Ws);
    if (ROWS == 2) y0 &= ~1, x0 &= ~1, y1 = (y1 + 1) & ~1, x1 = (x1 + 1) & ~1;
    if (y1 <= y0 || x1 <= x0) return;

    uint8_t* const fp = fr.frame(f);
    const long pitch = fr.pitch_of();
    const bool vec = fr.vector_ok(fp);
    const int lo = x0 * BPP, hi = x1 * BPP;
    const int units = (y1 - y0) / ROWS;                                    // rows, or row pairs
    const int tiles_y = (units + TR - 1) / TR;
    const int tiles_x = (hi - lo + 15 + 16 * PASTE_CHUNKS - 1) / (16 * PASTE_CHUNKS);      // a phase of up to 15 bytes in front

    for (int t = t0; t < tiles_y * tiles_x; t += G) {
        const int ty = t / tiles_x, tx = t - ty * tiles_x;
        const int u0 = ty * TR;
        // phase 1: slot i = (unit row r, frame row d of the unit, pixel p of the tile's span in that row)
        for (int i = tid; i < TR * ROWS * PW; i += 256) {
            const int rr = i / PW, p = i - rr * PW;
            const int r = rr / ROWS, d = rr - r * ROWS;
            if (u0 + r >= units) break;                                    // slots are ordered by row
            const int y = y0 + (u0 + r) * ROWS;
            const int phase = vec ? (int)((reinterpret_cast<uintptr_t>(fp + (long)y * pitch) + lo) & 15) : 0;
            int b0, b1;
            tile_span(lo, hi, phase, tx, b0, b1);
            if (b0 >= b1) continue;
            const int pfirst = b0 / BPP, plast = (b1 - 1) / BPP;
            if (pfirst + p <= plast) wk[i] = paste_wk(m, mhat, pfirst + p, y + d);
        }
        __syncthreads();
        // phase 2: thread (r, c)
        {
            const int r = tid / PASTE_CHUNKS, c = tid - r * PASTE_CHUNKS;
            if (u0 + r < units) {
                const int y = y0 + (u0 + r) * ROWS;
                const int phase = vec ? (int)((reinterpret_cast<uintptr_t>(fp + (long)y * pitch) + lo) & 15) : 0;
                paste_chunk(fr, fp, pitch, y, x0, lo, hi, phase, tx, c, vec, wk + r * ROWS * PW, slut);
            }
        }
        __syncthreads();                                                   // the next tile writes over these slots
    }
}

template <typename Fmt>
static int relevance_paste_launch(const Fmt& fr, const float* maps, int g, const double* A, const int* rect, const void* lut,
                                  const float* alpha, int n, int S, hipStream_t stream) {
    static_assert(Fmt::TR * PASTE_CHUNKS == 256, "one thread per (row, chunk) of a tile");
    // blocks per frame: enough to fill the device from a few frames, few enough that a long video is not all prologue
    long G = 4096 / n;
    G = G < 4 ? 4 : G > 64 ? 64 : G;
    const long nblocks = (long)n * G;
    if (nblocks > 0x7fffffffL) return ISTVT_ERR_SHAPE;
    hipLaunchKernelGGL(relevance_paste_kernel<Fmt>, dim3((unsigned)nblocks), dim3(256), 0, stream, fr, maps, g, A, rect,
                       (const uint8_t*)lut, alpha, S, (int)G);
    return istvt_check_launch();
}

static bool paste_args_ok(const void* frames, const float* maps, int g, const double* A, const int* rect, const void* lut,
                          const float* alpha, int n, int S) {
    return n > 0 && frames && maps && A && rect && lut && alpha && g >= 1 && g <= PASTE_MAX_GRID && S >= 1 && S <= 65536;
}

}  // namespace

// frames uint8 [n][Hs][Ws][3], written in place (`total` bytes at frames, >= n*Hs*Ws*3; no alignment needed); maps float32
// [n][g][g], A double [n][2][3], rect int32 [n][4] = (y0, x0, h, w), lut uint8 [256][3], alpha float32 [n], all on the
// device.  Only bytes inside the rectangle, clamped into the frame, are read or written.
extern "C" int istvt_relevance_paste_u8(void* frames, long total, int Hs, int Ws, const float* maps, int g, const double* A,
                                        const int* rect, const void* lut, const float* alpha, int n, int S,
                                        hipStream_t stream) {
    if (!paste_args_ok(frames, maps, g, A, rect, lut, alpha, n, S)) return ISTVT_ERR_SHAPE;
    if (Hs < 1 || Ws < 1 || Hs > 16384 || Ws > 16384) return ISTVT_ERR_SHAPE;
    if (total < (long)n * Hs * Ws * 3) return ISTVT_ERR_SHAPE;
    return relevance_paste_launch(PasteRgb{(uint8_t*)frames, Hs, Ws}, maps, g, A, rect, lut, alpha, n, S, stream);
}

// NV12 frames as istvt_crop_resize_nv12 takes them, written in place; frames may not overlap (fstride covers a frame when
// n > 1).  lut holds (Y, Cb, Cr) per entry.
extern "C" int istvt_relevance_paste_nv12(void* frames, long total, int Hs, int Ws, long pitch, long fstride,
                                          const float* maps, int g, const double* A, const int* rect, const void* lut,
                                          const float* alpha, int n, int S, hipStream_t stream) {
    if (!paste_args_ok(frames, maps, g, A, rect, lut, alpha, n, S)) return ISTVT_ERR_SHAPE;
    if (Hs < 2 || Ws < 2 || (Hs & 1) || (Ws & 1) || Hs > 16384 || Ws > 16384) return ISTVT_ERR_SHAPE;
    if (pitch < Ws || pitch > (1L << 20) || fstride < 0) return ISTVT_ERR_SHAPE;
    const long frame_bytes = (long)(Hs + Hs / 2 - 1) * pitch + Ws;
    if (n > 1 && fstride < frame_bytes) return ISTVT_ERR_SHAPE;
    if (total < (long)(n - 1) * fstride + frame_bytes) return ISTVT_ERR_SHAPE;
    return relevance_paste_launch(PasteNv12{(uint8_t*)frames, fstride, Hs, Ws, (int)pitch}, maps, g, A, rect, lut, alpha, n, S,
                                  stream);
}
