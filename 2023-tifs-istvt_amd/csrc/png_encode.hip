// PNG files out (DESIGN.md "PNG files out"): a batch of uint8 grey, RGB or RGBA frames -> complete PNG files end to end in
// `data`, the bytes of clips.png_encode_banded_host.  Four launches: png_filter_count_kernel, one wave per (file, band), filters
// the band's rows into the scratch, histograms its tokens in LDS and builds its code tables, header bits and size
// (csrc/png_deflate.h); png_prefix_kernel, one workgroup, places bands in files and files in data; png_store_kernel, the same
// waves, codes the bands; png_container_kernel, one workgroup per file, writes the chunks around the stream with the Adler-32 and
// the CRC-32s.  No synchronisation with the host, no global atomics, nothing allocated, nothing that has to be zeroed.
// istvt_png_encode_indexed_u8 is the same four launches with `extra` > 0: the bytes of the baND chunk that every file then
// carries between IHDR and IDAT (clips._png_band_chunk), which the container kernel writes from the bands' offsets.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "common.h"
#include "istvt_hip.h"
#include "png_deflate.h"

namespace {

constexpr int PE_ADAPTIVE = 5;
constexpr int PE_IHDR_END = 33;            // signature 8, IHDR 25: where the band index stands, if there is one
constexpr int PE_STREAM = 41;              // + the IDAT's length and type 8: where the zlib stream begins (+ the index's bytes)
constexpr int PE_CONTAINER = 57 + 6;       // + the IDAT's CRC 4 and IEND 12; the zlib header 2 and the Adler-32 4

__device__ __forceinline__ int pe_paeth(int a, int b, int c) {
    const int pa = abs(b - c), pb = abs(a - c), pc = abs(a + b - 2 * c);
    return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}

__device__ __forceinline__ int pe_residual(int ft, int v, int a, int b, int c) {
    const int pred = ft == 0 ? 0 : ft == 1 ? a : ft == 2 ? b : ft == 3 ? (a + b) >> 1 : pe_paeth(a, b, c);
    return (v - pred) & 255;
}

__device__ __forceinline__ uint32_t pe_cost(int r) { return (uint32_t)(r <= 128 ? r : 256 - r); }

// what the wave stored is read by other lanes of the wave: the stores have landed before the loads are issued
__device__ __forceinline__ void pe_fence() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    __syncthreads();
}

// ALONE: the band's first row takes a type that does not read the row above (clips.png_filter_rows_host(alone_rows=)): the
// cheaper of 0 and 1 where the filter is adaptive, of equal sums 0; else 0 for a fixed 0 or 2 and 1 for a fixed 1, 3 or 4
template <bool ALONE>
__global__ __launch_bounds__(64) void png_filter_count_kernel(const uint8_t* __restrict__ frames, int H, int W, int bpp, int band_rows,
                                                              int filter, int bands, uint8_t* scratch, long raw_stride,
                                                              int* __restrict__ rows) {
    __shared__ PdWork w;
    const int f = blockIdx.x / bands, k = blockIdx.x % bands, lane = threadIdx.x;
    const int rowbytes = W * bpp;
    const long stride = 1 + (long)rowbytes;
    const int r0 = k * band_rows, r1 = min(H, r0 + band_rows);
    const uint8_t* src = frames + (long)f * H * rowbytes;
    uint8_t* raw = scratch + (long)f * raw_stride;
    for (int r = r0; r < r1; ++r) {
        const uint8_t* cur = src + (long)r * rowbytes;
        const uint8_t* up = cur - rowbytes;                       // read where r > 0 only
        int ft = filter;
        if (filter == PE_ADAPTIVE) {
            uint32_t s0 = 0, s1 = 0, s2 = 0, s3 = 0, s4 = 0;      // a row costs at most 65536 * 128
            for (int x = lane; x < rowbytes; x += 64) {
                const int v = cur[x], a = x >= bpp ? cur[x - bpp] : 0, b = r > 0 ? up[x] : 0, c = (r > 0 && x >= bpp) ? up[x - bpp] : 0;
                s0 += pe_cost(v);
                s1 += pe_cost((v - a) & 255);
                s2 += pe_cost((v - b) & 255);
                s3 += pe_cost((v - ((a + b) >> 1)) & 255);
                s4 += pe_cost((v - pe_paeth(a, b, c)) & 255);
            }
            s0 = pd_sum(s0), s1 = pd_sum(s1), s2 = pd_sum(s2), s3 = pd_sum(s3), s4 = pd_sum(s4);
            ft = 0;
            uint32_t best = s0;
            if (s1 < best) best = s1, ft = 1;
            if (s2 < best) best = s2, ft = 2;
            if (s3 < best) best = s3, ft = 3;
            if (s4 < best) best = s4, ft = 4;
            if (ALONE && r == r0) ft = s1 < s0 ? 1 : 0;
        }
        if (ALONE && r == r0 && filter != PE_ADAPTIVE) ft = (filter == 0 || filter == 2) ? 0 : 1;
        uint8_t* dst = raw + (long)r * stride;
        if (lane == 0) dst[0] = (uint8_t)ft;
        for (int x = lane; x < rowbytes; x += 64) {
            const int v = cur[x], a = x >= bpp ? cur[x - bpp] : 0, b = r > 0 ? up[x] : 0, c = (r > 0 && x >= bpp) ? up[x - bpp] : 0;
            dst[1 + x] = (uint8_t)pe_residual(ft, v, a, b, c);
        }
    }
    for (int i = lane; i < PD_SLOTS; i += 64) w.counts[i] = 0;
    pe_fence();
    const int nb = (int)((r1 - r0) * stride);                     // H (1 + 4 W) < 2^31
    uint32_t adler_a = 0, adler_b = 0;
    pd_count_band(raw + (long)r0 * stride, nb, w.counts, &adler_a, &adler_b, lane);
    if (lane == 0) pd_build(w);
    __syncthreads();
    int* row = rows + ((long)f * bands + k) * PD_ROW_INTS;
    for (int i = lane; i < PD_SLOTS; i += 64) row[PD_ROW_WORDS + i] = (int)w.words[i];
    for (int i = lane; i < PD_HEADER_WORDS; i += 64) row[PD_ROW_HEADER + i] = (int)w.header[i];
    if (lane < 8) {
        const int meta[8] = {w.header_bits, w.band_bytes, (int)adler_a, (int)adler_b, nb, (0 << 8) | 1, 0, 0};
        row[PD_ROW_META + lane] = meta[lane];
    }
}

// bands in their file's stream, files in data; 256 files at a time
__global__ __launch_bounds__(256) void png_prefix_kernel(int* __restrict__ rows, int bands, int n, long capacity, long* __restrict__ offsets,
                                                         int* __restrict__ status, int extra) {
    __shared__ long sizes[256];
    __shared__ long carry;
    const int tid = threadIdx.x;
    if (tid == 0) carry = 0;
    __syncthreads();
    for (int base = 0; base < n; base += 256) {
        const int f = base + tid;
        if (f < n) {
            long at = 2;                                          // behind the zlib header
            for (int k = 0; k < bands; ++k) {
                int* meta = rows + ((long)f * bands + k) * PD_ROW_INTS + PD_ROW_META;
                meta[PD_META_OFFSET] = (int)at;
                at += meta[PD_META_BYTES];
            }
            sizes[tid] = at + 4 + (PE_CONTAINER - 6) + extra;
        }
        __syncthreads();
        if (tid == 0) {
            long c = carry;
            for (int t = 0; t < 256 && base + t < n; ++t) {
                offsets[base + t] = c;
                c += sizes[t];
                status[base + t] = c > capacity ? 1 : 0;
            }
            carry = c;
        }
        __syncthreads();
    }
    if (tid == 0) offsets[n] = carry;
}

__global__ __launch_bounds__(64) void png_store_kernel(const uint8_t* __restrict__ scratch, long raw_stride, const int* __restrict__ rows,
                                                       int H, int W, int bpp, int band_rows, int bands, uint8_t* data,
                                                       const long* __restrict__ offsets, const int* __restrict__ status, int extra) {
    __shared__ PdStage s;
    const int f = blockIdx.x / bands, k = blockIdx.x % bands, lane = threadIdx.x;
    if (status[f] != 0) return;
    const int* row = rows + ((long)f * bands + k) * PD_ROW_INTS;
    for (int i = lane; i < PD_SLOTS; i += 64) s.words[i] = (uint32_t)row[PD_ROW_WORDS + i];
    __syncthreads();
    const long stride = 1 + (long)W * bpp;
    const int r0 = k * band_rows, r1 = min(H, r0 + band_rows);
    const int* meta = row + PD_ROW_META;
    uint8_t* dst = data + offsets[f] + PE_STREAM + extra + meta[PD_META_OFFSET];
    pd_store_band(scratch + (long)f * raw_stride + (long)r0 * stride, (int)((r1 - r0) * stride), k == bands - 1 ? 1 : 0, s.words,
                  reinterpret_cast<const uint32_t*>(row + PD_ROW_HEADER), meta[PD_META_HEADER_BITS], dst, s.stage, lane);
}

// The CRC-32 of `total` bytes, byte(i) the i-th, by the PE_CRC_THREADS threads of a workgroup together: a contiguous slice per
// thread, equal lengths but for the last; the first wave folds them, eight neighbours per lane and then the 64 lanes, with
// x^(8 length) mod P.  -> the CRC in the threads of the first wave; part is free again behind the call.
constexpr int PE_CRC_THREADS = 512;

template <class Byte>
__device__ __forceinline__ uint32_t pe_crc_fold(long total, Byte byte, const uint32_t* table, uint32_t* part, int lane) {
    const long slice = (total + PE_CRC_THREADS - 1) / PE_CRC_THREADS;
    const long lo = min(total, lane * slice), hi = min(total, lo + slice);
    uint32_t crc = 0xffffffffu;
    for (long i = lo; i < hi; ++i) crc = table[(crc ^ byte(i)) & 255] ^ (crc >> 8);
    part[lane] = hi > lo ? ~crc : 0u;
    __syncthreads();
    uint32_t all = 0;
    if (lane < 64) {
        constexpr int group = PE_CRC_THREADS / 64;
        const uint32_t full = pd_crc_shift((uint64_t)slice);
        uint32_t mine_crc = 0;
        long mine_len = 0;
        for (int j = 0; j < group; ++j) {                         // the slices of threads [group lane, group (lane + 1))
            const int t = group * lane + j;
            const long tlo = min(total, t * slice), len = min(total, tlo + slice) - tlo;
            mine_crc = j == 0 ? part[t] : pd_crc_combine(mine_crc, part[t], len == slice ? full : pd_crc_shift((uint64_t)len));
            mine_len += len;
        }
        const uint32_t mine = pd_crc_shift((uint64_t)mine_len);
        all = __shfl(mine_crc, 0);
        for (int l = 1; l < 64; ++l) all = pd_crc_combine(all, __shfl(mine_crc, l), __shfl(mine, l));
    }
    __syncthreads();
    return all;
}

// Byte i of what the IDAT's CRC-32 covers lies at file[37 + extra + i]; the type, the zlib header and the Adler-32 are this
// kernel's own stores and are taken from registers.  One workgroup of PE_CRC_THREADS per file.  extra > 0: the band index,
// `extra` bytes at file[33]: words of 4 bytes, most significant first -- the body's length, 'baND', R, the band count, the
// bands' offsets in the stream (the scratch rows have them), the stream's length - 4, the CRC-32 of all but the first.
__global__ __launch_bounds__(PE_CRC_THREADS) void png_container_kernel(const int* __restrict__ rows, int H, int W, int bpp, int band_rows,
                                                                       int bands, uint8_t* data, const long* __restrict__ offsets,
                                                                       const int* __restrict__ status, int extra) {
    __shared__ uint32_t table[256];
    __shared__ uint8_t head[48];
    __shared__ uint32_t part[PE_CRC_THREADS];
    const int f = blockIdx.x, lane = threadIdx.x;                 // lane: the thread of the workgroup
    if (status[f] != 0) return;
    for (int i = lane; i < 256; i += PE_CRC_THREADS) table[i] = pd_crc_entry((uint32_t)i);
    uint8_t* file = data + offsets[f];
    const long size = offsets[f + 1] - offsets[f];
    const long stream = size - (PE_CONTAINER - 6) - extra;        // the IDAT's body
    uint32_t A = 1, B = 0;
    for (int k = 0; k < bands; ++k) {                             // uniform: every lane holds the sum
        const int* meta = rows + ((long)f * bands + k) * PD_ROW_INTS + PD_ROW_META;
        pd_adler_append(A, B, (uint32_t)meta[PD_META_ADLER_A], (uint32_t)meta[PD_META_ADLER_B], (uint32_t)meta[PD_META_LENGTH]);
    }
    const uint32_t adler = (B << 16) | A;
    __syncthreads();
    if (lane == 0) {
        const uint8_t sig[8] = {0x89, 'P', 'N', 'G', '\r', '\n', 0x1a, '\n'};
        for (int i = 0; i < 8; ++i) head[i] = sig[i];
        const uint8_t ihdr[21] = {0, 0, 0, 13, 'I', 'H', 'D', 'R', (uint8_t)(W >> 24), (uint8_t)(W >> 16), (uint8_t)(W >> 8), (uint8_t)W,
                                  (uint8_t)(H >> 24), (uint8_t)(H >> 16), (uint8_t)(H >> 8), (uint8_t)H, 8,
                                  (uint8_t)(bpp == 1 ? 0 : bpp == 3 ? 2 : 6), 0, 0, 0};
        uint32_t crc = 0xffffffffu;
        for (int i = 0; i < 21; ++i) {
            head[8 + i] = ihdr[i];
            if (i >= 4) crc = table[(crc ^ ihdr[i]) & 255] ^ (crc >> 8);
        }
        crc = ~crc;
        const uint8_t rest[14] = {(uint8_t)(crc >> 24), (uint8_t)(crc >> 16), (uint8_t)(crc >> 8), (uint8_t)crc,
                                  (uint8_t)(stream >> 24), (uint8_t)(stream >> 16), (uint8_t)(stream >> 8), (uint8_t)stream,
                                  'I', 'D', 'A', 'T', 0x78, 0x01};
        for (int i = 0; i < 14; ++i) head[29 + i] = rest[i];
    }
    __syncthreads();
    if (lane < PE_IHDR_END) file[lane] = head[lane];
    if (lane >= PE_IHDR_END && lane < 43) file[extra + lane] = head[lane];
    if (extra > 0) {
        // word j of the chunk, j = 0 .. bands + 4; the CRC-32 covers words 1 .. bands + 4 and is word bands + 5
        const auto word = [&](int j) -> uint32_t {
            if (j == 0) return (uint32_t)(extra - 12);
            if (j == 1) return 0x62614e44u;                       // 'baND'
            if (j == 2) return (uint32_t)band_rows;
            if (j == 3) return (uint32_t)bands;
            if (j - 4 < bands) return (uint32_t)rows[((long)f * bands + (j - 4)) * PD_ROW_INTS + PD_ROW_META + PD_META_OFFSET];
            return (uint32_t)(stream - 4);
        };
        uint8_t* chunk = file + PE_IHDR_END;
        for (int j = lane; j < bands + 5; j += PE_CRC_THREADS) {
            const uint32_t v = word(j);
            chunk[4 * j] = (uint8_t)(v >> 24), chunk[4 * j + 1] = (uint8_t)(v >> 16), chunk[4 * j + 2] = (uint8_t)(v >> 8), chunk[4 * j + 3] = (uint8_t)v;
        }
        const uint32_t crc = pe_crc_fold(4L * (bands + 4), [&](long i) -> uint32_t { return (word(1 + (int)(i >> 2)) >> (8 * (3 - (i & 3)))) & 255u; },
                                         table, part, lane);
        if (lane < 4) chunk[4 * (bands + 5) + lane] = (uint8_t)(crc >> (8 * (3 - lane)));
    }
    // the CRC-32 of type + body
    const long total = 4 + stream;
    const uint8_t* body = file + 37 + extra;
    const uint32_t all = pe_crc_fold(total, [&](long i) -> uint32_t {
        return i < 6 ? head[37 + i] : i >= total - 4 ? (adler >> (8 * (total - 1 - i))) & 255u : body[i];
    }, table, part, lane);
    if (lane < 20) {
        const uint8_t tail[20] = {(uint8_t)(adler >> 24), (uint8_t)(adler >> 16), (uint8_t)(adler >> 8), (uint8_t)adler,
                                  (uint8_t)(all >> 24), (uint8_t)(all >> 16), (uint8_t)(all >> 8), (uint8_t)all,
                                  0, 0, 0, 0, 'I', 'E', 'N', 'D', 0xae, 0x42, 0x60, 0x82};
        file[size - 20 + lane] = tail[lane];
    }
}

// the checks and the four launches of the three entries; extra: the bytes of a file's band index, 0 for none; alone (with
// an index only): the filter kernel's restriction, and ISTVT_PNG_BAND_ALONE in the word the container kernel writes as R
int pe_encode(const istvt_jpeg_encode_args* a, int bpp, int band_rows, int filter, int raw_stride, bool index, bool alone = false) {
    if (!a || a->n <= 0 || a->H < 1 || a->W < 1 || a->H > 16384 || a->W > 16384) return ISTVT_ERR_SHAPE;
    if ((bpp != 1 && bpp != 3 && bpp != 4) || band_rows < 1 || filter < 0 || filter > PE_ADAPTIVE) return ISTVT_ERR_SHAPE;
    if (!a->frames || !a->scratch || !a->data || !a->offsets || !a->status || a->capacity < 1) return ISTVT_ERR_SHAPE;
    const long raw = (long)a->H * (1 + (long)a->W * bpp), pixels = (long)a->n * a->H * a->W * bpp;
    if (a->total < pixels || raw_stride < raw || (raw_stride & 15)) return ISTVT_ERR_SHAPE;
    const int R = band_rows < a->H ? band_rows : a->H;
    const int bands = (a->H + R - 1) / R;
    const int extra = index ? 12 + 8 + 4 * (bands + 1) : 0;
    const long waves = (long)a->n * bands;
    if (waves > 0x7fffffffL) return ISTVT_ERR_SHAPE;
    const long need = (long)a->n * raw_stride + waves * PD_ROW_INTS * (long)sizeof(int);
    if ((reinterpret_cast<uintptr_t>(a->scratch) & 15) || a->scratch_bytes < need) return ISTVT_ERR_SHAPE;
    const uint8_t* src = (const uint8_t*)a->frames;
    uint8_t* data = (uint8_t*)a->data;
    if (data < src + a->total && src < data + a->capacity) return ISTVT_ERR_SHAPE;
    uint8_t* scratch = (uint8_t*)a->scratch;
    int* rows = reinterpret_cast<int*>(scratch + (long)a->n * raw_stride);
    if (alone)
        hipLaunchKernelGGL(png_filter_count_kernel<true>, dim3((unsigned)waves), dim3(64), 0, a->stream, src, a->H, a->W, bpp, R, filter,
                           bands, scratch, (long)raw_stride, rows);
    else
        hipLaunchKernelGGL(png_filter_count_kernel<false>, dim3((unsigned)waves), dim3(64), 0, a->stream, src, a->H, a->W, bpp, R, filter,
                           bands, scratch, (long)raw_stride, rows);
    int rc = istvt_check_launch();
    if (rc != ISTVT_OK) return rc;
    hipLaunchKernelGGL(png_prefix_kernel, dim3(1), dim3(256), 0, a->stream, rows, bands, a->n, a->capacity, a->offsets, a->status, extra);
    rc = istvt_check_launch();
    if (rc != ISTVT_OK) return rc;
    hipLaunchKernelGGL(png_store_kernel, dim3((unsigned)waves), dim3(64), 0, a->stream, (const uint8_t*)scratch, (long)raw_stride,
                       (const int*)rows, a->H, a->W, bpp, R, bands, data, (const long*)a->offsets, (const int*)a->status, extra);
    rc = istvt_check_launch();
    if (rc != ISTVT_OK) return rc;
    const int word = alone ? (int)((unsigned)R | ISTVT_PNG_BAND_ALONE) : R;       // the kernel reads it for the chunk's R word alone
    hipLaunchKernelGGL(png_container_kernel, dim3((unsigned)a->n), dim3(PE_CRC_THREADS), 0, a->stream, (const int*)rows, a->H, a->W, bpp, word,
                       bands, data, (const long*)a->offsets, (const int*)a->status, extra);
    return istvt_check_launch();
}

}  // namespace

// A batch of frames -> PNG files; include/istvt_hip.h describes the arguments and the scratch.
extern "C" int istvt_png_encode_u8(const istvt_jpeg_encode_args* a, int bpp, int band_rows, int filter, int raw_stride) {
    return pe_encode(a, bpp, band_rows, filter, raw_stride, false);
}

// ... and every file with its band index
extern "C" int istvt_png_encode_indexed_u8(const istvt_jpeg_encode_args* a, int bpp, int band_rows, int filter, int raw_stride) {
    return pe_encode(a, bpp, band_rows, filter, raw_stride, true);
}

// ... and every band's first row filtered without the row above, the index saying so
extern "C" int istvt_png_encode_alone_u8(const istvt_jpeg_encode_args* a, int bpp, int band_rows, int filter, int raw_stride) {
    return pe_encode(a, bpp, band_rows, filter, raw_stride, true, true);
}
