// The training criterion (DESIGN.md "Fused criterion"): nn.BCEWithLogitsLoss on B logits, the accuracy count beside it and
// the epoch meters, train_CNN.py:526-536, in one launch forward and one launch backward.
//
// istvt_bce_logits       z[i * stride], y[i] (float32 / int64 / int32 / uint8), optional w[i], pos_weight p, label smoothing
//                        eps -> per-sample loss, reduced loss, the UNSCALED logit gradient d[i] and the meter block.
//                            y' = y (1 - eps) + eps / 2,   e = exp(-|z|),   L = log1p(e)
//                            l  = w [ (1 - y') (L + max(z, 0)) + p y' (L + max(-z, 0)) ]
//                            d  = w [ (1 - y') sigmoid(z) - p y' sigmoid(-z) ]        (times 1 / n for the mean)
//                        These are torch's  (1 - y') z + (1 + (p - 1) y') (L + max(-z, 0))  and its derivative with the terms
//                        regrouped (z + softplus(-z) = softplus(z), 1 - sigmoid(-z) = sigmoid(z)): the same function, but no
//                        term of size |z| (or 1) is added and subtracted again, so a confident correct sample keeps its
//                        small loss and gradient in fp32 instead of rounding to 0.  sigmoid(|z|) = 1 / (1 + e),
//                        sigmoid(-|z|) = e / (1 + e): finite for every finite z.
//                        ONE workgroup of T = min(1024, max(64, next power of two >= n)) lanes: lane t walks the samples
//                        t, t + T, ... in ascending order (fp32 per sample, the loss added into an fp64 partial, the
//                        confusion counts into integers), the partials are folded by a binary tree in LDS
//                        (s = T/2, T/4, ..., 1: slot t += slot t + s), and lane 0 rounds the reduced loss once, writes it and
//                        adds the call to the meter block with a plain read-modify-write.  T and the order depend on n
//                        alone: two calls give the same bits.  No atomics, no workspace.
// istvt_bce_logits_bwd   grad[i] = d[i] * g[0] (mean / sum) or d[i] * g[i] (none), g read from device memory.
#include "common.h"

namespace {

constexpr int BCE_MAX_THREADS = 1024;
constexpr long BCE_MAX_N = 1l << 30;        // per-call counts are 32-bit inside the kernel

using Meter = istvt_loss_meter;
static_assert(sizeof(Meter) == 80, "istvt_loss_meter is ten 8-byte words");

struct Partial {
    double loss;
    unsigned tp, tn, fp, fn;
};

template <int KIND> __device__ __forceinline__ float load_target(const void* y, long i) {
    if (KIND == ISTVT_TARGET_F32) return ((const float*)y)[i];
    if (KIND == ISTVT_TARGET_I64) return (float)((const long long*)y)[i];
    if (KIND == ISTVT_TARGET_I32) return (float)((const int*)y)[i];
    return (float)((const unsigned char*)y)[i];
}

template <int KIND>
__global__ __launch_bounds__(BCE_MAX_THREADS) void bce_logits_kernel(const float* __restrict__ z, long stride,
                                                                     const void* __restrict__ y, const float* __restrict__ w,
                                                                     float p, float eps, int reduction, float threshold, long n,
                                                                     float* __restrict__ loss, float* __restrict__ reduced,
                                                                     float* __restrict__ d, Meter* meter) {
    __shared__ Partial part[BCE_MAX_THREADS];
    const int tid = threadIdx.x, T = blockDim.x;
    const float dscale = reduction == ISTVT_REDUCE_MEAN ? 1.0f / (float)n : 1.0f;
    Partial acc = {0.0, 0u, 0u, 0u, 0u};
#pragma unroll 4
    for (long i = tid; i < n; i += T) {
        const float zi = z[i * stride];
        const float yi = load_target<KIND>(y, i);
        const float wi = w ? w[i] : 1.0f;
        const float ys = yi * (1.0f - eps) + 0.5f * eps;
        const float e = expf(-fabsf(zi));
        const float L = log1pf(e);
        const float r = 1.0f / (1.0f + e);
        const float sp_pos = L + fmaxf(zi, 0.0f);       // softplus(z)
        const float sp_neg = L + fmaxf(-zi, 0.0f);      // softplus(-z)
        const float sg_pos = zi >= 0.0f ? r : e * r;    // sigmoid(z)
        const float sg_neg = zi >= 0.0f ? e * r : r;    // sigmoid(-z)
        const float li = wi * ((1.0f - ys) * sp_pos + p * ys * sp_neg);
        if (loss) loss[i] = li;
        if (d) d[i] = wi * ((1.0f - ys) * sg_pos - p * ys * sg_neg) * dscale;
        acc.loss += (double)li;
        // NaN compares false on both sides: a NaN logit predicts "negative", as (outputs > 0) does
        const bool pred = zi > threshold, pos = yi > 0.5f;
        acc.tp += (pred && pos) ? 1u : 0u;
        acc.tn += (!pred && !pos) ? 1u : 0u;
        acc.fp += (pred && !pos) ? 1u : 0u;
        acc.fn += (!pred && pos) ? 1u : 0u;
    }
    part[tid] = acc;
    __syncthreads();
    for (int s = T >> 1; s > 0; s >>= 1) {
        if (tid < s) {
            part[tid].loss += part[tid + s].loss;
            part[tid].tp += part[tid + s].tp;
            part[tid].tn += part[tid + s].tn;
            part[tid].fp += part[tid + s].fp;
            part[tid].fn += part[tid + s].fn;
        }
        __syncthreads();
    }
    if (tid == 0) {
        const Partial tot = part[0];
        // what the caller gets back is what the meter adds up: the value rounded to fp32 once (mean divides by n, as torch)
        const float out = (float)(reduction == ISTVT_REDUCE_MEAN ? tot.loss / (double)n : tot.loss);
        if (reduced) *reduced = out;
        if (meter) {
            meter->loss_sum += tot.loss;
            meter->batch_loss_sum += (double)out;
            meter->seen += (long long)n;
            meter->correct += (long long)tot.tp + (long long)tot.tn;
            meter->tp += (long long)tot.tp;
            meter->tn += (long long)tot.tn;
            meter->fp += (long long)tot.fp;
            meter->fn += (long long)tot.fn;
            meter->calls += 1;
        }
    }
}

__global__ __launch_bounds__(256) void bce_logits_bwd_kernel(const float* __restrict__ d, const float* __restrict__ g,
                                                             int g_per_sample, float* __restrict__ grad, long n) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) grad[i] = d[i] * (g_per_sample ? g[i] : g[0]);
}

}  // namespace

extern "C" int istvt_bce_logits(const float* z, long stride, const void* y, int y_kind, const float* w, float pos_weight,
                                float label_smoothing, int reduction, float threshold, long n, float* loss, float* reduced,
                                float* d, void* meter, hipStream_t stream) {
    if (!z || !y || n < 1 || n > BCE_MAX_N || stride < 1) return ISTVT_ERR_SHAPE;
    if (reduction < ISTVT_REDUCE_NONE || reduction > ISTVT_REDUCE_SUM) return ISTVT_ERR_SHAPE;
    if (!(label_smoothing >= 0.0f && label_smoothing < 1.0f)) return ISTVT_ERR_SHAPE;
    if (y_kind < ISTVT_TARGET_F32 || y_kind > ISTVT_TARGET_U8) return ISTVT_ERR_DTYPE;
    int T = 64;
    while (T < BCE_MAX_THREADS && T < n) T <<= 1;
#define BCE_LAUNCH(KIND)                                                                                                   \
    hipLaunchKernelGGL(bce_logits_kernel<KIND>, dim3(1), dim3((unsigned)T), 0, stream, z, stride, y, w, pos_weight,         \
                       label_smoothing, reduction, threshold, n, loss, reduced, d, (Meter*)meter)
    switch (y_kind) {
        case ISTVT_TARGET_F32: BCE_LAUNCH(ISTVT_TARGET_F32); break;
        case ISTVT_TARGET_I64: BCE_LAUNCH(ISTVT_TARGET_I64); break;
        case ISTVT_TARGET_I32: BCE_LAUNCH(ISTVT_TARGET_I32); break;
        default: BCE_LAUNCH(ISTVT_TARGET_U8); break;
    }
#undef BCE_LAUNCH
    return istvt_check_launch();
}

extern "C" int istvt_bce_logits_bwd(const float* d, const float* g, int g_per_sample, float* grad, long n,
                                    hipStream_t stream) {
    if (!d || !g || !grad || n < 1 || n > BCE_MAX_N) return ISTVT_ERR_SHAPE;
    hipLaunchKernelGGL(bce_logits_bwd_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, d, g, g_per_sample, grad,
                       n);
    return istvt_check_launch();
}
