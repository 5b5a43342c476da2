// Scoring a set of videos (DESIGN.md "Scoring a set of videos"): the two reductions behind VideoScorer.score_videos.
//
// istvt_windows_reduce   window logits [W][nc] and the videos' window ranges offsets [V+1] -> per video the mean logit and
//                        the mean sigmoid, [V][nc] each.  One workgroup per video: lane t sums the windows lo + t,
//                        lo + t + 256, ... in ascending order in fp64, the lane partials are folded in lane order in LDS, and
//                        the mean is rounded once to fp32.  sigmoid = 1 / (1 + exp(-x)) in fp32.
// istvt_auc_pairs        scores [V], labels [V] -> the counts behind accuracy and the pairwise AUC
//                            AUC = (#{s_p > s_n} + 1/2 #{s_p = s_n}) / (P N)
//                        over all (positive, negative) pairs.  Stage 1: a workgroup owns 256 videos, one per lane, and walks
//                        all V videos through LDS tiles; a lane whose video is a positive with a finite score counts the
//                        negatives with a finite score below it (greater) and level with it (equal).  The lanes' 64-bit
//                        counts are folded in LDS and the workgroup writes its six totals to its own slot.  Stage 2: one
//                        workgroup sums the slots and forms the AUC in fp64.
//
// One writer per element and no atomics in either: the counts are integers (exact, independent of order), the fp64 sums
// have a fixed order, so a second run gives the same bits.
#include "common.h"

namespace {

constexpr int VR_THREADS = 256;
constexpr int AUC_SLOT = 6;                 // greater, equal, positives, negatives, nonfinite, correct

__global__ __launch_bounds__(VR_THREADS) void windows_reduce_kernel(const float* __restrict__ logits,
                                                                    const int* __restrict__ offsets,
                                                                    float* __restrict__ logit_mean,
                                                                    float* __restrict__ prob_mean, int W, int nc) {
    __shared__ double part[VR_THREADS][2];
    const int v = blockIdx.x, tid = threadIdx.x;
    // the table is validated by the caller; forced into [0, W] and into order all the same, so that nothing outside
    // logits is read whatever it holds
    const int lo = min(max(offsets[v], 0), W);
    const int hi = min(max(offsets[v + 1], lo), W);
    const int cnt = hi - lo;
    const int live = min(cnt, VR_THREADS);
    for (int c = 0; c < nc; ++c) {
        double sl = 0.0, sp = 0.0;
        for (int w = lo + tid; w < hi; w += VR_THREADS) {
            const float x = logits[(long)w * nc + c];
            sl += (double)x;
            sp += (double)(1.0f / (1.0f + expf(-x)));
        }
        part[tid][0] = sl;
        part[tid][1] = sp;
        __syncthreads();
        if (tid == 0) {
            double tl = 0.0, tp = 0.0;
            for (int t = 0; t < live; ++t) {
                tl += part[t][0];
                tp += part[t][1];
            }
            // cnt = 0 cannot occur (every video has a window); it would give NaN, not a fault
            logit_mean[(long)v * nc + c] = (float)(tl / (double)cnt);
            prob_mean[(long)v * nc + c] = (float)(tp / (double)cnt);
        }
        __syncthreads();
    }
}

__device__ __forceinline__ bool finite_f32(float x) { return (__float_as_uint(x) & 0x7f800000u) != 0x7f800000u; }

// sum of one 64-bit count per lane over the workgroup, in `red` (VR_THREADS entries); every lane gets the total
__device__ __forceinline__ unsigned long long block_sum_u64(unsigned long long v, unsigned long long* red, int tid) {
    __syncthreads();                         // the previous use of red is over
    red[tid] = v;
    __syncthreads();
    for (int s = VR_THREADS / 2; s > 0; s >>= 1) {
        if (tid < s) red[tid] += red[tid + s];
        __syncthreads();
    }
    return red[0];
}

__global__ __launch_bounds__(VR_THREADS) void auc_pairs_kernel(const float* __restrict__ scores, const int* __restrict__ labels,
                                                               float threshold, unsigned long long* __restrict__ ws, int V) {
    __shared__ float ts[VR_THREADS];
    __shared__ int tneg[VR_THREADS];         // 1: a negative with a finite score
    __shared__ unsigned long long red[VR_THREADS];
    const int tid = threadIdx.x;
    const long i = (long)blockIdx.x * VR_THREADS + tid;
    const bool mine = i < V;
    const float s = mine ? scores[i] : 0.f;
    const bool pos = mine && labels[i] != 0;
    const bool fin = finite_f32(s);
    const bool cmp = pos && fin;
    unsigned long long greater = 0, equal = 0;
    for (int j0 = 0; j0 < V; j0 += VR_THREADS) {
        const int j = j0 + tid;
        __syncthreads();                     // the previous tile has been read
        if (j < V) {
            const float sj = scores[j];
            ts[tid] = sj;
            tneg[tid] = (labels[j] == 0 && finite_f32(sj)) ? 1 : 0;
        } else {
            ts[tid] = 0.f;
            tneg[tid] = 0;
        }
        __syncthreads();
        if (cmp) {
            unsigned g = 0, e = 0;           // at most 256 per tile
#pragma unroll 8
            for (int k = 0; k < VR_THREADS; ++k) {
                const float sn = ts[k];
                const int n = tneg[k];
                g += (n && s > sn) ? 1u : 0u;
                e += (n && s == sn) ? 1u : 0u;
            }
            greater += g;
            equal += e;
        }
    }
    const bool correct = mine && fin && ((s > threshold) == pos);
    const unsigned long long tg = block_sum_u64(greater, red, tid);
    const unsigned long long te = block_sum_u64(equal, red, tid);
    const unsigned long long tp = block_sum_u64(pos ? 1ull : 0ull, red, tid);
    const unsigned long long tn = block_sum_u64(mine && !pos ? 1ull : 0ull, red, tid);
    const unsigned long long tf = block_sum_u64(mine && !fin ? 1ull : 0ull, red, tid);
    const unsigned long long tc = block_sum_u64(correct ? 1ull : 0ull, red, tid);
    if (tid == 0) {
        unsigned long long* slot = ws + (long)blockIdx.x * AUC_SLOT;
        slot[0] = tg;
        slot[1] = te;
        slot[2] = tp;
        slot[3] = tn;
        slot[4] = tf;
        slot[5] = tc;
    }
}

__global__ __launch_bounds__(VR_THREADS) void auc_finish_kernel(const unsigned long long* __restrict__ ws, int nslots,
                                                                long long* __restrict__ counts, double* __restrict__ auc) {
    __shared__ unsigned long long red[VR_THREADS];
    const int tid = threadIdx.x;
    unsigned long long tot[AUC_SLOT];
    for (int q = 0; q < AUC_SLOT; ++q) {
        unsigned long long a = 0;
        for (int b = tid; b < nslots; b += VR_THREADS) a += ws[(long)b * AUC_SLOT + q];
        tot[q] = block_sum_u64(a, red, tid);
    }
    if (tid == 0) {
        for (int q = 0; q < AUC_SLOT; ++q) counts[q] = (long long)tot[q];
        const double pairs = (double)tot[2] * (double)tot[3];
        // 0 / 0 with an empty class: NaN by IEEE division
        *auc = ((double)tot[0] + 0.5 * (double)tot[1]) / pairs;
    }
}

}  // namespace

extern "C" int istvt_windows_reduce(const float* logits, const int* offsets, float* logit_mean, float* prob_mean, int W, int V,
                                    int nc, hipStream_t stream) {
    if (W < 1 || V < 1 || nc < 1 || V > W || !logits || !offsets || !logit_mean || !prob_mean) return ISTVT_ERR_SHAPE;
    hipLaunchKernelGGL(windows_reduce_kernel, dim3((unsigned)V), dim3(VR_THREADS), 0, stream, logits, offsets, logit_mean,
                       prob_mean, W, nc);
    return istvt_check_launch();
}

extern "C" int istvt_auc_pairs(const float* scores, const int* labels, float threshold, void* ws, long ws_elems, long long* counts,
                               double* auc, int V, hipStream_t stream) {
    if (V < 1 || !scores || !labels || !ws || !counts || !auc) return ISTVT_ERR_SHAPE;
    const int nblocks = (V + VR_THREADS - 1) / VR_THREADS;
    if (ws_elems < (long)nblocks * AUC_SLOT) return ISTVT_ERR_SHAPE;
    hipLaunchKernelGGL(auc_pairs_kernel, dim3((unsigned)nblocks), dim3(VR_THREADS), 0, stream, scores, labels, threshold,
                       (unsigned long long*)ws, V);
    int rc = istvt_check_launch();
    if (rc != ISTVT_OK) return rc;
    hipLaunchKernelGGL(auc_finish_kernel, dim3(1), dim3(VR_THREADS), 0, stream, (const unsigned long long*)ws, nblocks, counts,
                       auc);
    return istvt_check_launch();
}
