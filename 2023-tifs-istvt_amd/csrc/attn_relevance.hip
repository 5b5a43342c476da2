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

// the upsampled map at output pixel (oy, ox); x: the g x g map
__device__ __forceinline__ float heat_value(const float* x, int g, float inv_s, int oy, int ox) {
    int y0, y1, x0, x1;
    float ly, lx;
    heat_src(oy, inv_s, g, y0, y1, ly);
    heat_src(ox, inv_s, g, x0, x1, lx);
    return (1.f - ly) * ((1.f - lx) * x[y0 * g + x0] + lx * x[y0 * g + x1]) +
           ly * ((1.f - lx) * x[y1 * g + x0] + lx * x[y1 * g + x1]);
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
            const float v = heat_value(x, g, inv_s, t / G, t % G);
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

// ---- whole videos: the per-window rollouts fused into per-frame maps (DESIGN.md "Explaining whole videos") -----------
// Window w starts at frame starts[w] (ascending) and covers frame n as its frame t = n - starts[w] when 0 <= t < T.  Per
// frame: the plain mean over the covering windows, in ascending window order, of cam_s[w][t][j] = r_s[w][t+1][j+1],
// cam_t[w][t][j] = r_t[w][j+1][t+1], the temporal rollout at the space-class position r_t[w][0][t+1] and logits[w][index];
// and the number of covering windows.  One workgroup per frame, one thread per output element: every sum has one writer
// and a fixed order (no atomics), so two runs give the same bits.  A frame no window covers gets zeros.
__global__ void __launch_bounds__(256) fuse_windows_kernel(const float* __restrict__ r_s, const float* __restrict__ r_t,
                                                           const float* __restrict__ logits, const int* __restrict__ starts,
                                                           float* __restrict__ frame_s, float* __restrict__ frame_t,
                                                           float* __restrict__ frame_weight, float* __restrict__ frame_logit,
                                                           int* __restrict__ count, int W, int T, int P, int nc, int index) {
    const int n = blockIdx.x;
    const int F = T + 1, hw = P - 1;
    // first window with starts[w] > n - T (uniform binary search), then every window up to the first with starts[w] > n
    int lo = 0, hi = W;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (starts[mid] > n - T) hi = mid; else lo = mid + 1;
    }
    const int w0 = lo;
    int w1 = w0;
    while (w1 < W && starts[w1] <= n && starts[w1] > n - T) ++w1;       // the second test holds for ascending starts
    const int cnt = w1 - w0;
    const float inv = cnt > 0 ? 1.f / (float)cnt : 0.f;
    for (int j = threadIdx.x; j < hw; j += 256) {
        float as = 0.f, at = 0.f;
        for (int w = w0; w < w1; ++w) {
            const int t = n - starts[w];
            as += r_s[((long)w * F + t + 1) * P + j + 1];
            at += r_t[((long)w * P + j + 1) * F + t + 1];
        }
        frame_s[(long)n * hw + j] = as * inv;
        frame_t[(long)n * hw + j] = at * inv;
    }
    if (threadIdx.x == 0) {
        float aw = 0.f, al = 0.f;
        for (int w = w0; w < w1; ++w) {
            aw += r_t[(long)w * P * F + (n - starts[w]) + 1];
            al += logits[(long)w * nc + index];
        }
        frame_weight[n] = aw * inv;
        frame_logit[n] = al * inv;
        count[n] = cnt;
    }
}

extern "C" int istvt_relevance_fuse_windows(const float* r_s, const float* r_t, const float* logits, const int* starts,
                                            float* frame_s, float* frame_t, float* frame_weight, float* frame_logit, int* count,
                                            int W, int T, int P, int nc, int index, int N, hipStream_t stream) {
    if (W <= 0 || T <= 0 || P < 2 || nc <= 0 || index < 0 || index >= nc || N < T) return ISTVT_ERR_SHAPE;
    hipLaunchKernelGGL(fuse_windows_kernel, dim3((unsigned)N), dim3(256), 0, stream, r_s, r_t, logits, starts, frame_s, frame_t,
                       frame_weight, frame_logit, count, W, T, P, nc, index);
    return istvt_check_launch();
}

// ---- overlay: the heat map on the frame, bytes in and bytes out (the reference's show_cam_on_image, ----------------------
// visualize_rel.py:39-44, for a batch of frames).  Per frame: m = the map upsampled by s and min-max normalised (the
// arithmetic of heatmap_kernel), k = trunc(255 m) (a constant map's 0 / 0 takes k = 0), heat = lut[k] / 255,
// img = frame / 255 at the output pixel (read directly when S == g s, sampled bilinearly with half-pixel centres
// otherwise), cam = heat + img, out = trunc(255 cam / max(cam over the frame)).
// Three launches on one stream: the map's min / max (one workgroup per frame), the frame's max of cam, the write.  The two
// later ones are one kernel (the same cam arithmetic), a thread takes 16 consecutive pixels: 48 bytes, three 16-byte
// accesses when the frame size and the pointers allow.  The maximum crosses workgroups as an integer atomic max on the
// bits of a non-negative float: exact, so the order does not matter.  ws: 4 floats per frame (min, max, max of cam, pad).
__global__ void __launch_bounds__(256) overlay_minmax_kernel(const float* __restrict__ maps, float* __restrict__ ws, int g, int s) {
    __shared__ float x[HEAT_GMAX * HEAT_GMAX];
    __shared__ float rmin[4], rmax[4];
    const int n = blockIdx.x;
    const int G = g * s;
    const float inv_s = 1.f / (float)s;
    for (int t = threadIdx.x; t < g * g; t += 256) x[t] = maps[(long)n * g * g + t];
    __syncthreads();
    float mn = INFINITY, mx = -INFINITY;
    for (int t = threadIdx.x; t < G * G; t += 256) {
        const float v = heat_value(x, g, inv_s, t / G, t % G);
        mn = fminf(mn, v);
        mx = fmaxf(mx, v);
    }
    const float a = -wave_max(-mn), b = wave_max(mx);
    if ((threadIdx.x & 63) == 0) { rmin[threadIdx.x >> 6] = a; rmax[threadIdx.x >> 6] = b; }
    __syncthreads();
    if (threadIdx.x == 0) {
        ws[4 * n + 0] = fminf(fminf(rmin[0], rmin[1]), fminf(rmin[2], rmin[3]));
        ws[4 * n + 1] = fmaxf(fmaxf(rmax[0], rmax[1]), fmaxf(rmax[2], rmax[3]));
        ws[4 * n + 2] = 0.f;
        ws[4 * n + 3] = 0.f;
    }
}

constexpr int OVL_PIX = 16;                     // pixels per thread

// source taps of F.interpolate(mode='bilinear', align_corners=False) from S to So samples: ratio = S / So
__device__ __forceinline__ void resample_src(int o, float ratio, int S, int& i0, int& i1, float& l1) {
    float src = ((float)o + 0.5f) * ratio - 0.5f;
    src = src < 0.f ? 0.f : src;
    i0 = (int)src;
    i0 = i0 < S - 1 ? i0 : S - 1;
    i1 = i0 < S - 1 ? i0 + 1 : i0;
    l1 = src - (float)i0;
}

template <bool WRITE>
__global__ void __launch_bounds__(256) overlay_kernel(const uint8_t* __restrict__ frames, const float* __restrict__ maps,
                                                      const uint8_t* __restrict__ lut, float* __restrict__ ws,
                                                      uint8_t* __restrict__ out, int S, int g, int s, int vec_in, int vec_out) {
    __shared__ float x[HEAT_GMAX * HEAT_GMAX];
    __shared__ float heat[256 * 3];
    __shared__ float rmax[4];
    const int n = blockIdx.y;
    const int So = g * s;
    const long npix = (long)So * So;
    const float inv_s = 1.f / (float)s;
    for (int t = threadIdx.x; t < g * g; t += 256) x[t] = maps[(long)n * g * g + t];
    for (int t = threadIdx.x; t < 256 * 3; t += 256) heat[t] = (float)lut[t] / 255.f;
    __syncthreads();
    const float lo = ws[4 * n + 0], den = ws[4 * n + 1] - lo;
    const float top = WRITE ? ws[4 * n + 2] : 1.f;
    const uint8_t* frame = frames + (long)n * S * S * 3;
    const long p0 = ((long)blockIdx.x * 256 + threadIdx.x) * OVL_PIX;
    const bool direct = S == So;
    const float ratio = (float)S / (float)So;

    uint32_t in[12], o[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) { in[i] = 0u; o[i] = 0u; }
    if (direct && p0 < npix) {
        if (vec_in) {                           // npix is a multiple of 16 then: the 16 pixels are all inside
            const uint4* q = reinterpret_cast<const uint4*>(frame + p0 * 3);
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                const uint4 v = q[i];
                in[4 * i] = v.x; in[4 * i + 1] = v.y; in[4 * i + 2] = v.z; in[4 * i + 3] = v.w;
            }
        } else {
#pragma unroll
            for (int b = 0; b < 48; ++b)
                if (p0 * 3 + b < npix * 3) in[b >> 2] |= (uint32_t)frame[p0 * 3 + b] << (8 * (b & 3));
        }
    }
    float mx = 0.f;
    int oy = (int)(p0 / So), ox = (int)(p0 % So);
#pragma unroll
    for (int i = 0; i < OVL_PIX; ++i) {
        if (p0 + i < npix) {
            const float m = (heat_value(x, g, inv_s, oy, ox) - lo) / den;
            int k = m >= 0.f ? (int)(255.f * m) : 0;        // NaN (a constant map) compares false
            k = k < 255 ? k : 255;
            float img[3];
            if (direct) {
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const int b = 3 * i + c;
                    img[c] = (float)((in[b >> 2] >> (8 * (b & 3))) & 0xffu) / 255.f;
                }
            } else {
                int y0, y1, x0, x1;
                float ly, lx;
                resample_src(oy, ratio, S, y0, y1, ly);
                resample_src(ox, ratio, S, x0, x1, lx);
                const uint8_t* a = frame + ((long)y0 * S + x0) * 3;
                const uint8_t* b = frame + ((long)y0 * S + x1) * 3;
                const uint8_t* c2 = frame + ((long)y1 * S + x0) * 3;
                const uint8_t* d = frame + ((long)y1 * S + x1) * 3;
#pragma unroll
                for (int c = 0; c < 3; ++c)
                    img[c] = ((1.f - ly) * ((1.f - lx) * (float)a[c] + lx * (float)b[c]) +
                              ly * ((1.f - lx) * (float)c2[c] + lx * (float)d[c])) / 255.f;
            }
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float cam = heat[3 * k + c] + img[c];
                if (WRITE) {
                    int v = top > 0.f ? (int)(255.f * (cam / top)) : 0;
                    v = v < 255 ? v : 255;
                    const int b = 3 * i + c;
                    o[b >> 2] |= (uint32_t)v << (8 * (b & 3));
                } else {
                    mx = fmaxf(mx, cam);
                }
            }
        }
        if (++ox == So) { ox = 0; ++oy; }
    }
    if (WRITE) {
        if (p0 < npix) {
            uint8_t* dst = out + ((long)n * npix + p0) * 3;
            if (vec_out) {
                uint4* q = reinterpret_cast<uint4*>(dst);
#pragma unroll
                for (int i = 0; i < 3; ++i) q[i] = make_uint4(o[4 * i], o[4 * i + 1], o[4 * i + 2], o[4 * i + 3]);
            } else {
#pragma unroll
                for (int b = 0; b < 48; ++b)
                    if (p0 * 3 + b < npix * 3) dst[b] = (uint8_t)((o[b >> 2] >> (8 * (b & 3))) & 0xffu);
            }
        }
    } else {
        mx = wave_max(mx);
        if ((threadIdx.x & 63) == 0) rmax[threadIdx.x >> 6] = mx;
        __syncthreads();
        if (threadIdx.x == 0) {
            mx = fmaxf(fmaxf(rmax[0], rmax[1]), fmaxf(rmax[2], rmax[3]));
            atomicMax(reinterpret_cast<unsigned*>(ws + 4 * n + 2), __float_as_uint(mx));       // cam >= 0: bits order as values
        }
    }
}

extern "C" int istvt_relevance_overlay_u8(const void* frames, const float* maps, const void* lut, float* ws, void* out,
                                          int N, int S, int g, int s, hipStream_t stream) {
    if (N <= 0 || N > 65535 || S <= 0 || g <= 0 || g > HEAT_GMAX || s <= 0 || (long)g * s > 8192) return ISTVT_ERR_SHAPE;
    const long npix = (long)g * s * g * s;
    const unsigned chunks = (unsigned)((npix + 256 * OVL_PIX - 1) / (256 * OVL_PIX));
    const bool whole = npix % OVL_PIX == 0;
    const int vec_in = whole && S == g * s && (uintptr_t)frames % 16 == 0 && ((long)S * S * 3) % 16 == 0;
    const int vec_out = whole && (uintptr_t)out % 16 == 0 && (npix * 3) % 16 == 0;
    const uint8_t* f = static_cast<const uint8_t*>(frames);
    const uint8_t* l = static_cast<const uint8_t*>(lut);
    uint8_t* o = static_cast<uint8_t*>(out);
    hipLaunchKernelGGL(overlay_minmax_kernel, dim3((unsigned)N), dim3(256), 0, stream, maps, ws, g, s);
    hipLaunchKernelGGL(overlay_kernel<false>, dim3(chunks, (unsigned)N), dim3(256), 0, stream, f, maps, l, ws, o, S, g, s, vec_in, vec_out);
    hipLaunchKernelGGL(overlay_kernel<true>, dim3(chunks, (unsigned)N), dim3(256), 0, stream, f, maps, l, ws, o, S, g, s, vec_in, vec_out);
    return istvt_check_launch();
}
