// Backward of one separable unit's 1x1 convolution and the BatchNorm behind it, in ONE pass over the data (bf16):
//
//   du = gamma * rstd * (dz - s1/M - xhat * s2/M)        BatchNorm-backward apply (bn_bwd.h: bn_bwd_apply_kernel's expression)
//   dd = du . W                [M][Cin]                   input gradient of the 1x1 convolution (W = weight [Cout][Cin])
//   dW += du^T . d             [Cout][Cin] fp32           its weight gradient
//
// The three launches this replaces (bn_bwd_apply_kernel, gemm256t_kernel + splitk_reduce, gemm256q_kernel) write du
// [M][Cout] once and read it twice; here it lives in LDS only.  Reads dz, u, d; writes dd.
//
// Persistent kernel, 512 threads, one workgroup per CU at the training step's size.  The rows are cut as the weight
// gradient it replaces cuts its reduction (pw_bwd_split: G contiguous chunks of kper rows, kper a multiple of 64, G = 256 for
// M >= 131072): workgroup g takes the rows [g kper, min(M, (g + 1) kper)) in blocks of PW_R = 128 rows, ascending, and
// feeds them to the weight gradient's MFMA chain in the order and at the fragment positions of gemm256t.h (32 rows per
// step, fragment element i of lane group g = row 32 s + 8 g + i).  With the same slabs summed in the same order the
// weight gradient has the BITS of ops.linear_wgrad(du, d) -- a training run keeps the parent's trajectory.  Per block:
//   1  the block's dz / u / d vectors (16 bytes, loaded two blocks ahead into registers) -> du (fp32 arithmetic,
//      rounded to bf16 exactly where bn_bwd_apply_kernel's store rounded it) -> LDS; d -> LDS; rows past M are zeros.
//      The loads of the block two ahead go out into the registers just freed.
//   2  barrier
//   3  dd^T tile = W . du^T: wavefront w owns 16 input channels (W fragments resident in registers for the whole kernel)
//      and contracts over Cout ascending, 32 channels per v_mfma_f32_16x16x32_bf16; a lane then holds 4 consecutive input
//      channels of one row, rounded to bf16 into the staging tile.
//      dW^T tile += d^T . du: wavefront w owns 16 output channels x all Cin; both operands are read with the transposing
//      fragment read (ds_read_b64_tr_b16), the contraction runs over the block's rows; fp32 accumulators live in registers
//      across all of the workgroup's blocks.
//   4  barrier
//   5  staging tile -> dd, 16 bytes per lane, range-checked against M.
// At the end workgroup g stores its accumulators to slab g of ws[G][Cout * Cin]; istvt_splitk_reduce adds the slabs in
// index order into wgrad_out.  No atomics: the row-to-workgroup map and the slab order depend on M only, so two runs give
// the same bits.  Workgroup 0 adds s2 / s1 into dgamma / dbeta as
// bn_bwd_apply_kernel does.
//
// LDS images: rows of C + 16 elements (stride = 8 dwords mod 64), and row p of a group of 32 block rows sits at image
// row pw_lds_row(p) = bits (p2 p4 p3 p1 p0) of p: the fragment rows 8 g + i of a transposing read's 32-lane group (g = 0,
// 1; i < 4, then i >= 4) are the image rows 4 g + i, then 16 + 4 g + i - 4 -- 8 consecutive image rows per read, 8
// distinct 32-byte bank groups (in block order they would be rows 0-3 and 8-11: two-way conflicts at any row stride
// that keeps rows 16-byte aligned).  The products of dd work on image rows (every row is independent) and phase 5 reads
// the staging tile through the same map.  The row-contiguous 16-byte reads of du are conflict-free at this stride too.
#include "common.h"
#include "bn_bwd.h"

constexpr int PW_R = 128;           // rows per block
constexpr int PW_THREADS = 512;

// image row of block row p (see above): a permutation inside every group of 32 rows
__host__ __device__ constexpr int pw_lds_row(int p) { return (p & ~31) | ((p & 4) << 2) | ((p & 24) >> 1) | (p & 3); }

// The reduction split of the weight gradient this kernel replaces (ops.linear_wgrad for a one-tile bf16 gradient:
// _pick_splitk with 256 workgroups aimed for, then istvt_gemm's rounding of the chunk to the 64-row K tile).
static inline int pw_bwd_split(long M, long* kper_out) {
    long splits = M / 512 < 1 ? 1 : (M / 512 > 256 ? 256 : M / 512);
    if (splits > (M + 63) / 64) splits = (M + 63) / 64;
    long kper = (M + splits - 1) / splits;
    kper = (kper + 63) / 64 * 64;
    if (kper_out) *kper_out = kper;
    return (int)((M + kper - 1) / kper);
}

template <int CIN, int COUT>
struct PwTile {                     // one block's operands in flight
    static constexpr int NU = PW_R * (COUT / 8) / PW_THREADS;
    static constexpr int ND = PW_R * (CIN / 8) / PW_THREADS;
    bf16x8 dz[NU], u[NU], d[ND];
};

template <int CIN, int COUT>
__global__ __launch_bounds__(PW_THREADS) void pw_bwd_kernel(
    const bf16_t* __restrict__ dz, const bf16_t* __restrict__ u, const float* __restrict__ bnp,
    const float* __restrict__ gamma, const double* s1, const double* s2, const bf16_t* __restrict__ d, long ldd,
    const bf16_t* __restrict__ wt, long ldwt, bf16_t* __restrict__ dd, float* __restrict__ ws, float* dgamma,
    float* dbeta, long M, long kper, int batch_stats) {
    static_assert(COUT == 128 && (CIN == 64 || CIN == 128), "instantiated shapes");
    constexpr int LDU = COUT + 16, LDD = CIN + 16;                 // LDS row strides, elements
    constexpr int UCH = COUT / 8, DCH = CIN / 8;                   // 16-byte chunks per row
    constexpr int UROWS = PW_THREADS / UCH, DROWS = PW_THREADS / DCH;
    constexpr int KT = CIN / 16, KS = COUT / 32;                   // input-channel tiles; contraction steps of dd
    constexpr int MT = (PW_R / 16) * KT / 8;                       // row tiles per wavefront in the dd product
    typedef PwTile<CIN, COUT> Tile;
    __shared__ __attribute__((aligned(16))) bf16_t s_du[PW_R * LDU];
    __shared__ __attribute__((aligned(16))) bf16_t s_d[PW_R * LDD];
    __shared__ __attribute__((aligned(16))) bf16_t s_dd[PW_R * LDD];
    __shared__ __attribute__((aligned(16))) BnBwdChunk s_kc[UCH];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int g = lane >> 4, r = lane & 15;
    const long row_begin = (long)blockIdx.x * kper;                // this workgroup's rows: [row_begin, row_end)
    const long row_end = min(M, row_begin + kper);
    const long nblk = (row_end - row_begin + PW_R - 1) / PW_R;

    // phase-1 / phase-5 maps: a thread keeps one channel chunk, so its per-channel constants never change
    const int uc = tid % UCH, ur = tid / UCH;
    const int dc = tid % DCH, dr = tid / DCH;
    // ... and they would take 40 registers for the whole kernel: they wait in LDS and are read back in phase 1, when the
    // products' accumulators and fragments are dead
    const float invM = batch_stats ? 1.0f / (float)M : 0.0f;
    if (tid < UCH) bn_bwd_chunk_load(s_kc[tid], bnp, gamma, s1, s2, COUT, tid * 8, invM);
    __syncthreads();

    // W fragments of this wavefront's 16 input channels: A operand, row = input channel, 8 consecutive output channels
    const int kt_dd = wave % KT, mt0 = (wave / KT) * MT;
    bf16x8 wf[KS];
#pragma unroll
    for (int s = 0; s < KS; ++s)
        wf[s] = *reinterpret_cast<const bf16x8*>(wt + (long)(kt_dd * 16 + r) * ldwt + s * 32 + g * 8);

    f32x4 accw[KT];
#pragma unroll
    for (int kt = 0; kt < KT; ++kt) accw[kt] = f32x4{0.f, 0.f, 0.f, 0.f};

    // Operand loads are buffer loads over [0, row_end rows): a row past the end gets an offset outside the descriptor and
    // reads as zeros without a branch, so the loads of a block go out back to back and the compiler counts them (vmcnt) across
    // the two tiles in flight.  The host refuses operands of 2 GiB or more (32-bit offsets).
    constexpr unsigned OOB = 0x80000000u, RSRC_FLAGS = 0x00020000u;
    const __amdgpu_buffer_rsrc_t dz_rs = __builtin_amdgcn_make_buffer_rsrc((void*)dz, 0, (int)(row_end * COUT * 2), RSRC_FLAGS);
    const __amdgpu_buffer_rsrc_t u_rs = __builtin_amdgcn_make_buffer_rsrc((void*)u, 0, (int)(row_end * COUT * 2), RSRC_FLAGS);
    const __amdgpu_buffer_rsrc_t d_rs = __builtin_amdgcn_make_buffer_rsrc((void*)d, 0, (int)(row_end * ldd * 2), RSRC_FLAGS);
    const __amdgpu_buffer_rsrc_t dd_rs = __builtin_amdgcn_make_buffer_rsrc((void*)dd, 0, (int)(row_end * CIN * 2), RSRC_FLAGS);
    const int ldd2 = (int)ldd * 2;

    auto load = [&](Tile& t, const long b) {            // b >= nblk: every row is past the end, nothing is read
        const long row0 = row_begin + b * PW_R;
#pragma unroll
        for (int i = 0; i < Tile::NU; ++i) {
            const long row = row0 + ur + i * UROWS;
            const unsigned off = row < row_end ? (unsigned)((int)row * (COUT * 2) + uc * 16) : OOB;
            t.dz[i] = __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(dz_rs, off, 0, 0));
            t.u[i] = __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(u_rs, off, 0, 0));
        }
#pragma unroll
        for (int i = 0; i < Tile::ND; ++i) {
            const long row = row0 + dr + i * DROWS;
            const unsigned off = row < row_end ? (unsigned)((int)row * ldd2 + dc * 16) : OOB;
            t.d[i] = __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(d_rs, off, 0, 0));
        }
    };

    auto block = [&](Tile& t, const long b, const long bnext) {
        const long row0 = row_begin + b * PW_R;
        // ---- 1: du and d into LDS
        const BnBwdChunk kc = s_kc[uc];
#pragma unroll
        for (int i = 0; i < Tile::NU; ++i) {
            const int lr = ur + i * UROWS;
            const unsigned keep = row0 + lr < row_end ? 0xffffffffu : 0u;   // rows past the end: zeros (a mask, not a branch)
            bf16x8 o;
#pragma unroll
            for (int j = 0; j < 8; ++j) o[j] = (bf16_t)bn_bwd_du((float)t.dz[i][j], (float)t.u[i][j], kc, j);
            *reinterpret_cast<u32x4*>(s_du + pw_lds_row(lr) * LDU + uc * 8) = __builtin_bit_cast(u32x4, o) & keep;
        }
#pragma unroll
        for (int i = 0; i < Tile::ND; ++i)
            *reinterpret_cast<bf16x8*>(s_d + pw_lds_row(dr + i * DROWS) * LDD + dc * 8) = t.d[i];
        load(t, bnext);
        __syncthreads();
        // ---- 3a: dd^T = W . du^T  (m: an image row)
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
            const int m = (mt0 + mt) * 16 + r;
            f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int s = 0; s < KS; ++s) {
                const bf16x8 bu = *reinterpret_cast<const bf16x8*>(s_du + m * LDU + s * 32 + g * 8);
                acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[s], bu, acc, 0, 0, 0);
            }
            bf16x4 o;
#pragma unroll
            for (int e = 0; e < 4; ++e) o[e] = (bf16_t)acc[e];
            *reinterpret_cast<bf16x4*>(s_dd + m * LDD + kt_dd * 16 + g * 4) = o;
        }
        // ---- 3b: dW^T += d^T . du  (image rows ka .. ka+3, kb .. kb+3 = block rows 32 s + 8 g .. + 7)
#pragma unroll
        for (int s = 0; s < PW_R / 32; ++s) {
            const int ka = s * 32 + g * 4, kb = ka + 16;
            const bf16x8 bu = frag_load_tr(s_du, LDU, ka, kb, wave * 16, r);
#pragma unroll
            for (int kt = 0; kt < KT; ++kt) {
                const bf16x8 ad = frag_load_tr(s_d, LDD, ka, kb, kt * 16, r);
                accw[kt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ad, bu, accw[kt], 0, 0, 0);
            }
        }
        __syncthreads();
        // ---- 5: dd rows out
#pragma unroll
        for (int i = 0; i < Tile::ND; ++i) {
            const int lr = dr + i * DROWS;
            const long row = row0 + lr;
            const unsigned off = row < row_end ? (unsigned)((int)row * (CIN * 2) + dc * 16) : OOB;      // past the end: dropped
            __builtin_amdgcn_raw_buffer_store_b128(*reinterpret_cast<const u32x4*>(s_dd + pw_lds_row(lr) * LDD + dc * 8), dd_rs,
                                                   off, 0, 0);
        }
        // (the next block's phase 1 writes s_du / s_d, which every wavefront left at the barrier above; its phase 3
        //  writes s_dd behind the next barrier, which this phase's reads precede)
    };

    Tile t0, t1;
    load(t0, 0);
    __builtin_amdgcn_sched_barrier(0);                   // keep the issue order: the vmcnt counts of the loop rely on it
    load(t1, 1);
    __builtin_amdgcn_sched_barrier(0);
    // Two blocks per trip, without a branch between them (the compiler's vmcnt counts then hold across the two tiles in
    // flight): a second block past the end is a tile of zeros whose stores are all out of range.  The trip count is
    // uniform over the workgroup, so the barriers inside are safe.
    for (long b = 0; b < nblk; b += 2) {
        block(t0, b, b + 2);
        block(t1, b + 1, b + 3);
    }

    // ---- this workgroup's partial weight gradient: lane (r, g) of tile kt holds dW[16 wave + r][16 kt + 4 g .. + 3]
    float* slab = ws + (long)blockIdx.x * (COUT * CIN);
#pragma unroll
    for (int kt = 0; kt < KT; ++kt)
        *reinterpret_cast<f32x4*>(slab + (wave * 16 + r) * CIN + kt * 16 + g * 4) = accw[kt];

    if (blockIdx.x == 0) {
        for (int c = tid; c < COUT; c += PW_THREADS) {
            if (dgamma) dgamma[c] += (float)s2[c];
            if (dbeta) dbeta[c] += (float)s1[c];
        }
    }
}

// workgroups of a launch over M rows (= slabs of the workspace: the caller sizes ws[G][Cout * Cin] from it) and rows per block
extern "C" int istvt_pw_bwd_grid(long M) { return M > 0 ? pw_bwd_split(M, nullptr) : 0; }
extern "C" int istvt_pw_bwd_rows() { return PW_R; }

extern "C" int istvt_pw_bwd(const void* dz, const void* u, const float* bnp, const float* gamma, const double* s1,
                            const double* s2, const void* d, long ldd, const void* wt, long ldwt, void* dd, float* ws,
                            float* wgrad_out, float* dgamma, float* dbeta, long M, int Cin, int Cout, int batch_stats,
                            int dtype, hipStream_t stream) {
    if (dtype != DT_BF16) return ISTVT_ERR_DTYPE;
    if (M <= 0 || Cout != 128 || (Cin != 64 && Cin != 128)) return ISTVT_ERR_SHAPE;
    if (ldd < Cin || ldd % 8 != 0 || ldwt < Cout || ldwt % 8 != 0) return ISTVT_ERR_SHAPE;
    if (M * Cout * 2 >= 0x7fffffffL || M * ldd * 2 >= 0x7fffffffL) return ISTVT_ERR_SHAPE;       // 32-bit operand offsets
    if (!dz || !u || !bnp || !gamma || !s1 || !s2 || !d || !wt || !dd || !ws || !wgrad_out) return ISTVT_ERR_SHAPE;
    long kper = 0;
    const int G = pw_bwd_split(M, &kper);
#define PW_LAUNCH(CI, CO)                                                                                              \
    hipLaunchKernelGGL((pw_bwd_kernel<CI, CO>), dim3((unsigned)G), dim3(PW_THREADS), 0, stream, (const bf16_t*)dz,      \
                       (const bf16_t*)u, bnp, gamma, s1, s2, (const bf16_t*)d, ldd, (const bf16_t*)wt, ldwt,           \
                       (bf16_t*)dd, ws, dgamma, dbeta, M, kper, batch_stats)
    if (Cin == 64) PW_LAUNCH(64, 128);
    else PW_LAUNCH(128, 128);
#undef PW_LAUNCH
    const int rc = istvt_check_launch();
    if (rc != ISTVT_OK) return rc;
    return istvt_splitk_reduce(ws, G, (long)Cout * Cin, wgrad_out, stream);
}
