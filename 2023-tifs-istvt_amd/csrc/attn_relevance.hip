// Gradient-weighted attention rollout (Chefer, Gur, Wolf, ICCV 2021, "Generic Attention-model Explainability"): one
// rollout step per attention layer, launched from the attention Functions' backward while a relevance context is active
// (functional.relevance_mode).  The training kernels are not touched: these recompute what they need from the same
// saved operands.
//
//   E_h[i, j] = max(0, A_h[i, j] * dA_h[i, j]),  A = softmax(q k^T scale),  dA = dO v^T   (the gradient w.r.t. the
//   probabilities, not the scores)
//   r_out[j]  = r[j] + (1/H) sum_h sum_i r[i] E_h[i, j]
//
// No P x P (or F x F) tile is written to memory and no float atomics are used: every sum has one writer and a fixed
// order, so two runs give the same bits.  fp32 math and output; f32 or bf16 operands.
#include "common.h"

// ---- spatial: one workgroup per (frame, tile of 64 keys) -------------------------------------------------------------
// Keys on the lane (lane j holds k_j, v_j of the current head in registers), query rows staged through LDS in chunks
// of 64 rows and read as broadcasts; wave w takes rows w, w+4, ... of a chunk, so sum_i r[i] E[i, j] is a per-lane FMA
// chain.  The four wave partials are summed in wave order at the end.  A query row whose r[i] is 0 contributes nothing
// and is skipped (the rollout starts from e_0: the last layer's step reads one row per frame).
// P is recomputed from q, k and the forward's statistics: p = exp2(s * scale * log2e - m) * inv, (m, inv) = lse[row][h],
// the same normalisation the forward and the training backward use.
constexpr int SREL_ROWS = 64;

template <typename T, int DH>
__global__ void __launch_bounds__(256) srel_kernel(const T* __restrict__ qkv, long ldqkv, const T* __restrict__ dout, long ldo,
                                                   const float* __restrict__ lse, const float* __restrict__ r,
                                                   float* __restrict__ r_out, int P, int heads, float scale) {
    __shared__ float sq[SREL_ROWS][DH];
    __shared__ float sd[SREL_ROWS][DH];
    __shared__ float sm[SREL_ROWS], si[SREL_ROWS], sr[SREL_ROWS];
    __shared__ float red[4][WAVE];
    const int bf = blockIdx.y;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int j = blockIdx.x * WAVE + lane;
    const bool jok = j < P;
    const long row0 = (long)bf * P;
    const int inner = heads * DH;
    const float c = scale * 1.4426950408889634f;
    const float* rf = r + row0;
    float acc = 0.f;
    for (int h = 0; h < heads; ++h) {
        float kj[DH], vj[DH];
        const T* kp = qkv + (row0 + (jok ? j : 0)) * ldqkv + inner + h * DH;
#pragma unroll
        for (int e = 0; e < DH; e += 8) {
            float t[8];
            load8(kp + e, t);
#pragma unroll
            for (int u = 0; u < 8; ++u) kj[e + u] = t[u];
            load8(kp + inner + e, t);
#pragma unroll
            for (int u = 0; u < 8; ++u) vj[e + u] = t[u];
        }
        for (int i0 = 0; i0 < P; i0 += SREL_ROWS) {
            const int n = min(SREL_ROWS, P - i0);
            __syncthreads();                           // the previous chunk's readers are done
            for (int t = threadIdx.x; t < n * (DH / 8); t += 256) {
                const int ri = t / (DH / 8), e = (t % (DH / 8)) * 8;
                float a[8], b[8];
                load8(qkv + (row0 + i0 + ri) * ldqkv + h * DH + e, a);
                load8(dout + (row0 + i0 + ri) * ldo + h * DH + e, b);
#pragma unroll
                for (int u = 0; u < 8; ++u) { sq[ri][e + u] = a[u]; sd[ri][e + u] = b[u]; }
            }
            if (threadIdx.x < n) {
                const float2 st = reinterpret_cast<const float2*>(lse)[(row0 + i0 + threadIdx.x) * heads + h];
                sm[threadIdx.x] = st.x;
                si[threadIdx.x] = st.y;
                sr[threadIdx.x] = rf[i0 + threadIdx.x];
            }
            __syncthreads();
            for (int ri = w; ri < n; ri += 4) {
                const float ri_w = sr[ri];
                if (ri_w == 0.f) continue;             // uniform across the wave
                float s = 0.f, dp = 0.f;
#pragma unroll
                for (int e = 0; e < DH; e += 4) {
                    const float4 qa = *reinterpret_cast<const float4*>(&sq[ri][e]);
                    const float4 da = *reinterpret_cast<const float4*>(&sd[ri][e]);
                    s += qa.x * kj[e] + qa.y * kj[e + 1] + qa.z * kj[e + 2] + qa.w * kj[e + 3];
                    dp += da.x * vj[e] + da.y * vj[e + 1] + da.z * vj[e + 2] + da.w * vj[e + 3];
                }
                const float p = exp2f(s * c - sm[ri]) * si[ri];
                acc += ri_w * fmaxf(0.f, p * dp);
            }
        }
    }
    red[w][lane] = acc;
    __syncthreads();
    if (w == 0 && jok) {
        const float sum = ((red[0][lane] + red[1][lane]) + red[2][lane]) + red[3][lane];
        r_out[row0 + j] = rf[j] + sum / (float)heads;
    }
}

extern "C" int istvt_attn_spatial_relevance(const void* qkv, long ldqkv, const void* dout, long ldo, const float* lse,
                                            const float* r, float* r_out, int BF, int P, int heads, int dh, float scale,
                                            int dtype, hipStream_t stream) {
    if (BF <= 0 || P <= 0 || heads <= 0 || BF > 65535 || (dh != 32 && dh != 64)) return ISTVT_ERR_SHAPE;
    if (ldqkv < 3L * heads * dh || ldo < (long)heads * dh || ldqkv % 8 || ldo % 8) return ISTVT_ERR_SHAPE;
    if (r == r_out) return ISTVT_ERR_SHAPE;          // other key tiles of the frame still read r
    dim3 grid((unsigned)((P + WAVE - 1) / WAVE), (unsigned)BF), block(256);
    DISPATCH_DTYPE(dtype, {
        if (dh == 64) hipLaunchKernelGGL((srel_kernel<T, 64>), grid, block, 0, stream, (const T*)qkv, ldqkv, (const T*)dout, ldo, lse, r, r_out, P, heads, scale);
        else hipLaunchKernelGGL((srel_kernel<T, 32>), grid, block, 0, stream, (const T*)qkv, ldqkv, (const T*)dout, ldo, lse, r, r_out, P, heads, scale);
    });
    return istvt_check_launch();
}

// ---- temporal: one wavefront per (clip, position) -------------------------------------------------------------------
// Per head the F rows of q, k, v and dO are staged into the wavefront's LDS slice with 16-byte loads (the frame
// difference of diff == 1 taken on the way), the F x F scores and dA = dO v^T are formed one (i, j) pair per lane, the
// softmax is recomputed in full (nothing is saved by the forward), and lane j < F folds column j, sum_i r[i] E[i, j], in
// row order.  Memory-bound: q, k, v and dO are read once.
constexpr int TREL_FMAX = 17;

template <typename T, int DH, int FMAX>
__global__ void __launch_bounds__(256) trel_kernel(const T* __restrict__ qkv, long ldqkv, const T* __restrict__ dout, long ldo,
                                                   const float* __restrict__ r, float* __restrict__ r_out, int B, int F, int P,
                                                   int heads, float scale, int diff) {
    constexpr int LD = DH + 4;                         // row pitch in floats (16-byte aligned, breaks the bank stride)
    __shared__ float img[4][4][FMAX][LD];              // [wave][q | k | v | dO][frame][element]
    __shared__ float sS[4][FMAX][FMAX + 1], sD[4][FMAX][FMAX + 1];
    __shared__ float sR[4][FMAX];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const long prob_w = (long)blockIdx.x * 4 + w;
    const bool ok = prob_w < (long)B * P;              // a wavefront past the end computes problem 0 and stores nothing
    const long prob = ok ? prob_w : 0;
    const int b = (int)(prob / P), n = (int)(prob % P);
    const int inner = heads * DH;
    const float c = scale * 1.4426950408889634f;
    float (*q)[LD] = img[w][0];
    float (*k)[LD] = img[w][1];
    float (*v)[LD] = img[w][2];
    float (*d)[LD] = img[w][3];
    float acc = 0.f;                                   // lane j < F: sum_h sum_i r[i] E_h[i, j]
    if (lane < F) sR[w][lane] = r[prob * F + lane];
    for (int h = 0; h < heads; ++h) {
        for (int t = lane; t < F * (DH / 8); t += WAVE) {
            const int f = t / (DH / 8), e = (t % (DH / 8)) * 8;
            const long row = ((long)b * F + f) * P + n;
            const T* src = qkv + row * ldqkv + h * DH + e;
            float a[8], bk[8], cv[8], dd[8];
            load8(src, a);
            load8(src + inner, bk);
            load8(src + 2 * inner, cv);
            load8(dout + row * ldo + h * DH + e, dd);
            if (diff == 1 && f >= 2) {
                const T* prv = src - (long)P * ldqkv;
                float a0[8], b0[8];
                load8(prv, a0);
                load8(prv + inner, b0);
#pragma unroll
                for (int u = 0; u < 8; ++u) { a[u] -= a0[u]; bk[u] -= b0[u]; }
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) { q[f][e + u] = a[u]; k[f][e + u] = bk[u]; v[f][e + u] = cv[u]; d[f][e + u] = dd[u]; }
        }
        __syncthreads();
        for (int t = lane; t < F * F; t += WAVE) {
            const int i = t / F, jj = t % F;
            float s = 0.f, dp = 0.f;
#pragma unroll
            for (int e = 0; e < DH; e += 4) {
                const float4 qa = *reinterpret_cast<const float4*>(&q[i][e]);
                const float4 ka = *reinterpret_cast<const float4*>(&k[jj][e]);
                const float4 da = *reinterpret_cast<const float4*>(&d[i][e]);
                const float4 va = *reinterpret_cast<const float4*>(&v[jj][e]);
                s += qa.x * ka.x + qa.y * ka.y + qa.z * ka.z + qa.w * ka.w;
                dp += da.x * va.x + da.y * va.y + da.z * va.z + da.w * va.w;
            }
            sS[w][i][jj] = s * c;
            sD[w][i][jj] = dp;
        }
        __syncthreads();
        if (lane < F) {                                // row `lane`: softmax, then E in place
            const int i = lane;
            float m = -INFINITY;
            for (int jj = 0; jj < F; ++jj) m = fmaxf(m, sS[w][i][jj]);
            float sum = 0.f;
            for (int jj = 0; jj < F; ++jj) sum += exp2f(sS[w][i][jj] - m);
            const float inv = 1.f / sum;
            for (int jj = 0; jj < F; ++jj) sS[w][i][jj] = fmaxf(0.f, exp2f(sS[w][i][jj] - m) * inv * sD[w][i][jj]);
        }
        __syncthreads();
        if (lane < F) {                                // column `lane`, rows in order
            float cs = 0.f;
            for (int i = 0; i < F; ++i) cs += sR[w][i] * sS[w][i][lane];
            acc += cs;
        }
        __syncthreads();                               // the next head overwrites the images and sS
    }
    if (ok && lane < F) r_out[prob * F + lane] = sR[w][lane] + acc / (float)heads;
}

extern "C" int istvt_attn_temporal_relevance(const void* qkv, long ldqkv, const void* dout, long ldo, const float* r,
                                             float* r_out, int B, int F, int P, int heads, int dh, float scale, int diff,
                                             int dtype, hipStream_t stream) {
    if (B <= 0 || F <= 0 || F > TREL_FMAX || P <= 0 || heads <= 0 || diff < 0 || diff > 2 || (dh != 32 && dh != 64))
        return ISTVT_ERR_SHAPE;
    if (ldqkv < 3L * heads * dh || ldo < (long)heads * dh || ldqkv % 8 || ldo % 8) return ISTVT_ERR_SHAPE;
    const long nprob = (long)B * P;
    if ((nprob + 3) / 4 > 0x7fffffffL) return ISTVT_ERR_SHAPE;
    // diff == 2: q and k arrive differenced, the softmax is the plain one (as in the forward)
    const int d = diff == 1 ? 1 : 0;
    dim3 grid((unsigned)((nprob + 3) / 4)), block(256);
    // FMAX 9 (T <= 8) halves the LDS images: 4 workgroups per CU instead of 1 at dh 64
#define TREL(DHV, FM) hipLaunchKernelGGL((trel_kernel<T, DHV, FM>), grid, block, 0, stream, (const T*)qkv, ldqkv, (const T*)dout, ldo, r, r_out, B, F, P, heads, scale, d)
    DISPATCH_DTYPE(dtype, {
        if (dh == 64) { if (F <= 9) TREL(64, 9); else TREL(64, 17); }
        else { if (F <= 9) TREL(32, 9); else TREL(32, 17); }
    });
#undef TREL
    return istvt_check_launch();
}

// ---- heat maps: bilinear upsampling by an integer factor + per-map min-max ------------------------------------------
// F.interpolate(mode='bilinear', align_corners=False, scale_factor=s): src = (dst + 0.5) / s - 0.5 clamped at 0,
// i0 = floor(src), i1 = min(i0 + 1, g - 1), lambda = src - i0; then (x - min) / (max - min) per map, the reference's
// post-processing (visualize_rel.py:262-265; a constant map gives 0 / 0 there too).  One workgroup per map.
constexpr int HEAT_GMAX = 64;

__device__ __forceinline__ void heat_src(int o, float inv_s, int g, int& i0, int& i1, float& l1) {
    float src = ((float)o + 0.5f) * inv_s - 0.5f;
    src = src < 0.f ? 0.f : src;
    i0 = (int)src;
    i1 = i0 < g - 1 ? i0 + 1 : i0;
    l1 = src - (float)i0;
}

__global__ void __launch_bounds__(256) heatmap_kernel(const float* __restrict__ cam, float* __restrict__ out, int g, int s) {
    __shared__ float x[HEAT_GMAX * HEAT_GMAX];
    __shared__ float rmin[4], rmax[4];
    const int map = blockIdx.x;
    const int G = g * s;
    const float inv_s = 1.f / (float)s;
    const float* src = cam + (long)map * g * g;
    float* dst = out + (long)map * G * G;
    for (int t = threadIdx.x; t < g * g; t += 256) x[t] = src[t];
    __syncthreads();
    float mn = INFINITY, mx = -INFINITY;
    for (int pass = 0; pass < 2; ++pass) {
        float lo = 0.f, den = 1.f;
        if (pass == 1) { lo = mn; den = mx - mn; }
        for (int t = threadIdx.x; t < G * G; t += 256) {
            const int oy = t / G, ox = t % G;
            int y0, y1, x0, x1;
            float ly, lx;
            heat_src(oy, inv_s, g, y0, y1, ly);
            heat_src(ox, inv_s, g, x0, x1, lx);
            const float v = (1.f - ly) * ((1.f - lx) * x[y0 * g + x0] + lx * x[y0 * g + x1]) +
                            ly * ((1.f - lx) * x[y1 * g + x0] + lx * x[y1 * g + x1]);
            if (pass == 0) { mn = fminf(mn, v); mx = fmaxf(mx, v); }
            else dst[t] = (v - lo) / den;
        }
        if (pass == 0) {
            const float a = -wave_max(-mn), b = wave_max(mx);
            if ((threadIdx.x & 63) == 0) { rmin[threadIdx.x >> 6] = a; rmax[threadIdx.x >> 6] = b; }
            __syncthreads();
            mn = fminf(fminf(rmin[0], rmin[1]), fminf(rmin[2], rmin[3]));
            mx = fmaxf(fmaxf(rmax[0], rmax[1]), fmaxf(rmax[2], rmax[3]));
        }
    }
}

extern "C" int istvt_relevance_heatmap(const float* cam, float* out, int maps, int g, int s, hipStream_t stream) {
    if (maps <= 0 || g <= 0 || g > HEAT_GMAX || s <= 0 || (long)g * s > 8192) return ISTVT_ERR_SHAPE;
    hipLaunchKernelGGL(heatmap_kernel, dim3((unsigned)maps), dim3(256), 0, stream, cam, out, g, s);
    return istvt_check_launch();
}
