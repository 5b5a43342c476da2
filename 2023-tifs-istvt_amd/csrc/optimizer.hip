// Fused optimizer steps over the flat parameter / gradient buffers of parallel.GradBucket
// (reference: train_CNN.py:196-201 -- torch.optim.SGD(lr, momentum=0.9, weight_decay=0) or AdamW(betas, eps)).
// One pass over {p, g, state}: reads g once and (optionally) writes zeros back, so the separate zero-grad pass of the
// next step disappears.  HBM-bound: SGD-momentum moves 5 x 4 bytes per parameter (p r/w, buf r/w, g r) + the zero write.
//
// Around that pass (all optional; the plain entry points run exactly what they always ran):
//   * istvt_grad_norm: the global L2 norm of grad_scale * g, two stages in a fixed order (no atomics; the grid depends on n
//     alone, so every rank and every run gets the same bits).  Its second stage writes the step-info block: the norm, the
//     scale the update multiplies the gradients by (grad_scale x clip_grad_norm_'s coefficient; 0 for a skipped step),
//     whether the norm is finite, and -- in skip mode -- the applied / skipped step counters.
//   * istvt_*_groups: the same update arithmetic (one __device__ function per optimizer, shared with the plain kernels) with
//     {lr, weight_decay} per parameter group: a static device segment table (sorted end offsets + group id) says which
//     elements belong to which group, the hyper-parameters travel by value in the kernel arguments.
#include "common.h"

namespace {

// ---- the per-element updates: ONE function each, compiled into the plain and the grouped kernels alike ---------------------
// Every fused multiply-add is written out, and a product that has to reach a sum rounded goes through rounded(): which
// product the compiler fuses into which sum (-ffp-contract=fast lets the backend fuse wherever it finds a pair) depends on
// the code around the expression, and the two kernels of one optimizer have to round alike (the grouped entry points with
// one group are bit-identical to the plain ones).  The forms below are the ones the plain kernels have always been
// compiled to.

// x, opaque to the optimizer (no instruction): a multiply behind it cannot be contracted into the add in front of it
__device__ __forceinline__ float rounded(float x) {
    asm("" : "+v"(x));
    return x;
}

// torch.optim.SGD semantics: g' = g + wd * p;  first step buf = g', later buf = mu * buf + (1 - dampening) * g';
// d = nesterov ? g' + mu * buf : buf;  p -= lr * d.   (b is not read on the first step.)
// TAIL: the elementwise path behind the buffer's last whole 16-byte quad has always rounded both momentum products before
// adding them, where the vector path fuses one; kept, so that no bit of an existing run changes.
template <bool TAIL>
__device__ __forceinline__ void sgd_update(float& p, float g, float& b, float gscale, float lr, float wd, float mu,
                                           float dampening, int nesterov, int first) {
#pragma clang fp contract(off)
    const float gj = fmaf(g, gscale, wd * p);
    const float bn = TAIL ? rounded((1.f - dampening) * gj) + rounded(mu * b) : fmaf(1.f - dampening, gj, mu * b);
    b = first ? gj : bn;
    p = fmaf(-lr, nesterov ? fmaf(mu, b, gj) : b, p);
}

// torch.optim.AdamW semantics (amsgrad off): p *= 1 - lr * wd;  m = b1 m + (1 - b1) g;  v = b2 v + (1 - b2) g^2;
// p -= (lr / (1 - b1^t)) * m / (sqrt(v) / sqrt(1 - b2^t) + eps)
__device__ __forceinline__ void adamw_update(float& p, float g, float& m, float& v, float gscale, float lr, float wd,
                                             float b1, float b2, float eps, float step_size, float inv_sqrt_bc2) {
#pragma clang fp contract(off)
    const float gj = g * gscale;
    const float mj = fmaf(1.f - b1, gj, b1 * m);
    const float vj = rounded(b2 * v) + rounded(((1.f - b2) * gj) * gj);
    p = rounded(p * fmaf(-lr, wd, 1.f)) - (step_size * mj) / fmaf(sqrtf(vj), inv_sqrt_bc2, eps);
    m = mj; v = vj;
}

__global__ __launch_bounds__(256) void sgd_momentum_kernel(float* __restrict__ p, float* __restrict__ g,
                                                           float* __restrict__ buf, long n, float lr, float mu,
                                                           float dampening, float wd, int nesterov, int first,
                                                           int zero_grad, float gscale) {
    const long stride = (long)gridDim.x * 256 * 4;
    for (long i = ((long)blockIdx.x * 256 + threadIdx.x) * 4; i < n; i += stride) {
        if (i + 3 < n) {
            float4 pv = *reinterpret_cast<float4*>(p + i), gv = *reinterpret_cast<float4*>(g + i);
            float4 bv = first ? make_float4(0.f, 0.f, 0.f, 0.f) : *reinterpret_cast<float4*>(buf + i);
            float* pp = &pv.x; float* gg = &gv.x; float* bb = &bv.x;
#pragma unroll
            for (int j = 0; j < 4; ++j) sgd_update<false>(pp[j], gg[j], bb[j], gscale, lr, wd, mu, dampening, nesterov, first);
            *reinterpret_cast<float4*>(p + i) = pv;
            *reinterpret_cast<float4*>(buf + i) = bv;
            if (zero_grad) *reinterpret_cast<float4*>(g + i) = make_float4(0.f, 0.f, 0.f, 0.f);
        } else {
            for (long k = i; k < n; ++k) {
                float pk = p[k], b = first ? 0.f : buf[k];
                sgd_update<true>(pk, g[k], b, gscale, lr, wd, mu, dampening, nesterov, first);
                buf[k] = b;
                p[k] = pk;
                if (zero_grad) g[k] = 0.f;
            }
        }
    }
}

__global__ __launch_bounds__(256) void adamw_kernel(float* __restrict__ p, float* __restrict__ g, float* __restrict__ m,
                                                    float* __restrict__ v, long n, float lr, float b1, float b2,
                                                    float eps, float wd, float step_size, float inv_sqrt_bc2,
                                                    int zero_grad, float gscale) {
    const long stride = (long)gridDim.x * 256;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
        float pj = p[i], mj = m[i], vj = v[i];
        adamw_update(pj, g[i], mj, vj, gscale, lr, wd, b1, b2, eps, step_size, inv_sqrt_bc2);
        p[i] = pj; m[i] = mj; v[i] = vj;
        if (zero_grad) g[i] = 0.f;
    }
}

inline int opt_grid(long n, int per_thread) {
    long b = (n + 256L * per_thread - 1) / (256L * per_thread);
    if (b > 65536) b = 65536;
    return b < 1 ? 1 : (int)b;
}

// ---- the step-info block (device memory, 8 x 32-bit words) ---------------------------------------------------------------
using StepInfo = istvt_step_info;
static_assert(sizeof(StepInfo) == 32, "istvt_step_info is eight 32-bit words");

// fp64 sum over the workgroup in a fixed order: lanes by a shuffle tree, then the four wavefronts in index order.
// Valid in thread 0.
__device__ __forceinline__ double block_sum_f64(double d, double* lds4) {
#pragma unroll
    for (int off = WAVE / 2; off > 0; off >>= 1) d += __shfl_down(d, off, WAVE);
    if ((threadIdx.x & (WAVE - 1)) == 0) lds4[threadIdx.x / WAVE] = d;
    __syncthreads();
    return lds4[0] + lds4[1] + lds4[2] + lds4[3];
}

constexpr int NORM_ITERS = 16;                          // float4 loads per lane
constexpr long NORM_CHUNK = 256L * 4 * NORM_ITERS;      // elements per workgroup: a function of nothing but this file

// stage 1: workgroup b reduces g[b * NORM_CHUNK, (b + 1) * NORM_CHUNK): each lane squares 4 x NORM_ITERS elements into four
// fp32 accumulators (NORM_ITERS terms each), everything above that is fp64.  One double per workgroup.
__global__ __launch_bounds__(256) void grad_norm_partial_kernel(const float* __restrict__ g, long n, float gscale,
                                                                double* __restrict__ ws) {
    __shared__ double lds4[4];
    const long chunk0 = (long)blockIdx.x * NORM_CHUNK + threadIdx.x * 4;
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
    for (int it = 0; it < NORM_ITERS; ++it) {
        const long i = chunk0 + (long)it * 1024;
        if (i + 3 < n) {
            const float4 gv = *reinterpret_cast<const float4*>(g + i);
            const float x0 = gv.x * gscale, x1 = gv.y * gscale, x2 = gv.z * gscale, x3 = gv.w * gscale;
            acc[0] += x0 * x0; acc[1] += x1 * x1; acc[2] += x2 * x2; acc[3] += x3 * x3;
        } else {
            for (long k = i; k < n; ++k) {
                const float x = g[k] * gscale;
                acc[k - i] += x * x;
            }
        }
    }
    const double d = block_sum_f64(((double)acc[0] + (double)acc[1]) + ((double)acc[2] + (double)acc[3]), lds4);
    if (threadIdx.x == 0) ws[blockIdx.x] = d;
}

// stage 2 (one workgroup): thread t sums its contiguous run of partials in index order, the runs are combined in the same
// fixed order as above; thread 0 writes the step-info block.
__global__ __launch_bounds__(256) void grad_norm_final_kernel(const double* __restrict__ ws, long blocks, float gscale,
                                                              float max_norm, int skip_mode, StepInfo* __restrict__ info) {
    __shared__ double lds4[4];
    const long per = (blocks + 255) / 256;
    const long lo = threadIdx.x * per, hi = lo + per < blocks ? lo + per : blocks;
    double d = 0.0;
    for (long k = lo; k < hi; ++k) d += ws[k];
    d = block_sum_f64(d, lds4);
    if (threadIdx.x == 0) {
        const float total = (float)sqrt(d);
        const int finite = isfinite(total) ? 1 : 0;
        float scale = gscale;
        if (max_norm > 0.f) scale = gscale * fminf(1.f, max_norm / (total + 1e-6f));
        if (skip_mode) {
            if (finite) info->applied_steps += 1;
            else { info->skipped_steps += 1; scale = 0.f; }
        }
        info->total_norm = total;
        info->scale = scale;
        info->finite = finite;
    }
}

// ---- grouped steps -------------------------------------------------------------------------------------------------------
constexpr int MAX_GROUPS = 8;
constexpr int GROUP_ITERS = 8;                          // float4 quads per lane
constexpr long GROUP_CHUNK = 256L * 4 * GROUP_ITERS;    // a workgroup owns a contiguous chunk: its segment cursor only moves forward
constexpr int SEG_LDS = 128;                            // segment boundaries staged per workgroup (the rest is read from memory)

// by value in the kernel arguments.  a0 / a1: what the host derives per group from the step count (adamw: lr / bc1 and
// 1 / sqrt(bc2), the very floats the plain kernel is handed); in skip mode the device derives them from its own count.
struct GroupTable { float lr[MAX_GROUPS]; float wd[MAX_GROUPS]; float a0[MAX_GROUPS]; float a1[MAX_GROUPS]; };

__device__ __forceinline__ double ipow_f64(double b, long t) {   // b^t, t >= 0, by squaring
    double r = 1.0;
    for (; t > 0; t >>= 1, b *= b)
        if (t & 1) r *= b;
    return r;
}

struct SgdGroupOp {
    float* buf;
    float mu, dampening;
    int nesterov, first;
    // which step this is: from the host, or (skip mode) from the block's applied-step count, which already includes this step
    __device__ void resolve(const StepInfo* info, int dev_steps) { if (dev_steps) first = info->applied_steps == 1; }
    __device__ void group_aux(float, const StepInfo*, float*, float*) const {}
    __device__ void quad(long i, float* pp, const float* gg, const float* lr, const float* wd, const float*, const float*,
                         float gscale) const {
        float4 bv = first ? make_float4(0.f, 0.f, 0.f, 0.f) : *reinterpret_cast<const float4*>(buf + i);
        float* bb = &bv.x;
#pragma unroll
        for (int j = 0; j < 4; ++j) sgd_update<false>(pp[j], gg[j], bb[j], gscale, lr[j], wd[j], mu, dampening, nesterov, first);
        *reinterpret_cast<float4*>(buf + i) = bv;
    }
    __device__ void elem(long k, float& p, float g, float lr, float wd, float, float, float gscale) const {
        float b = first ? 0.f : buf[k];
        sgd_update<true>(p, g, b, gscale, lr, wd, mu, dampening, nesterov, first);
        buf[k] = b;
    }
};

struct AdamwGroupOp {
    float* m;
    float* v;
    float b1, b2, eps;
    __device__ void resolve(const StepInfo*, int) {}
    // skip mode, once per workgroup and group: the bias corrections of the block's applied-step count, in fp64 as the host
    // computes them from its own count otherwise -- lr / bc1 and 1 / sqrt(bc2)
    __device__ void group_aux(float lr, const StepInfo* info, float* a0, float* a1) const {
        const long t = info->applied_steps;
        *a0 = (float)((double)lr / (1.0 - ipow_f64((double)b1, t)));
        *a1 = (float)(1.0 / sqrt(1.0 - ipow_f64((double)b2, t)));
    }
    __device__ void quad(long i, float* pp, const float* gg, const float* lr, const float* wd, const float* a0,
                         const float* a1, float gscale) const {
        float4 mv = *reinterpret_cast<const float4*>(m + i), vv = *reinterpret_cast<const float4*>(v + i);
        float* mm = &mv.x; float* vq = &vv.x;
#pragma unroll
        for (int j = 0; j < 4; ++j) adamw_update(pp[j], gg[j], mm[j], vq[j], gscale, lr[j], wd[j], b1, b2, eps, a0[j], a1[j]);
        *reinterpret_cast<float4*>(m + i) = mv;
        *reinterpret_cast<float4*>(v + i) = vv;
    }
    __device__ void elem(long k, float& p, float g, float lr, float wd, float a0, float a1, float gscale) const {
        float mk = m[k], vk = v[k];
        adamw_update(p, g, mk, vk, gscale, lr, wd, b1, b2, eps, a0, a1);
        m[k] = mk; v[k] = vk;
    }
};

// Workgroup b owns elements [b * GROUP_CHUNK, (b + 1) * GROUP_CHUNK); lane t takes the 16-byte quads at t * 4 + it * 1024
// inside it.  Thread 0 finds the chunk's first segment (one binary search per workgroup), the boundaries from there on are
// staged in LDS, and every lane walks a cursor forward over them: a quad inside one segment (all but the few at a
// parameter boundary) takes one comparison and one group's hyper-parameters; a quad across a boundary is still loaded and
// stored 16 bytes wide, only its hyper-parameters are looked up per element.  The last, partial quad of the buffer is
// elementwise.  The table's last end offset is n (the host builds it so); the cursor never leaves the table whatever it holds.
template <class Op>
__global__ __launch_bounds__(256) void grouped_step_kernel(Op op, float* __restrict__ p, float* __restrict__ g, long n,
                                                           const long* __restrict__ seg_end,
                                                           const int* __restrict__ seg_group, int nseg, GroupTable tab,
                                                           int ngroups, const StepInfo* __restrict__ info, float gscale,
                                                           int skip_mode, int zero_grad) {
    __shared__ long s_end[SEG_LDS];
    __shared__ int s_gid[SEG_LDS];
    __shared__ float s_lr[MAX_GROUPS], s_wd[MAX_GROUPS], s_a0[MAX_GROUPS], s_a1[MAX_GROUPS];
    __shared__ int s_first;
    const int tid = threadIdx.x;
    const long chunk0 = (long)blockIdx.x * GROUP_CHUNK;
    const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);

    if (info) gscale = info->scale;
    if (skip_mode && info->finite == 0) {       // a skipped step: parameters and state stay as they are
        if (zero_grad) {
            for (int it = 0; it < GROUP_ITERS; ++it) {
                const long i = chunk0 + (long)it * 1024 + tid * 4;
                if (i + 3 < n) *reinterpret_cast<float4*>(g + i) = zero4;
                else for (long k = i; k < n; ++k) g[k] = 0.f;
            }
        }
        return;
    }
    op.resolve(info, skip_mode);

    if (tid == 0) {                             // first segment that ends behind the chunk's first element
        int lo = 0, hi = nseg - 1;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (seg_end[mid] > chunk0) hi = mid; else lo = mid + 1;
        }
        s_first = lo;
    }
    if (tid < ngroups) {
        const float lr = tid == 0 ? tab.lr[0] : tid == 1 ? tab.lr[1] : tid == 2 ? tab.lr[2] : tid == 3 ? tab.lr[3]
                       : tid == 4 ? tab.lr[4] : tid == 5 ? tab.lr[5] : tid == 6 ? tab.lr[6] : tab.lr[7];
        const float wd = tid == 0 ? tab.wd[0] : tid == 1 ? tab.wd[1] : tid == 2 ? tab.wd[2] : tid == 3 ? tab.wd[3]
                       : tid == 4 ? tab.wd[4] : tid == 5 ? tab.wd[5] : tid == 6 ? tab.wd[6] : tab.wd[7];
        float a0 = tid == 0 ? tab.a0[0] : tid == 1 ? tab.a0[1] : tid == 2 ? tab.a0[2] : tid == 3 ? tab.a0[3]
                 : tid == 4 ? tab.a0[4] : tid == 5 ? tab.a0[5] : tid == 6 ? tab.a0[6] : tab.a0[7];
        float a1 = tid == 0 ? tab.a1[0] : tid == 1 ? tab.a1[1] : tid == 2 ? tab.a1[2] : tid == 3 ? tab.a1[3]
                 : tid == 4 ? tab.a1[4] : tid == 5 ? tab.a1[5] : tid == 6 ? tab.a1[6] : tab.a1[7];
        if (skip_mode) op.group_aux(lr, info, &a0, &a1);
        s_lr[tid] = lr; s_wd[tid] = wd; s_a0[tid] = a0; s_a1[tid] = a1;
    }
    __syncthreads();
    const int first = s_first;
    const int last = nseg - 1 - first;          // cursor positions are relative to `first`
    if (tid < SEG_LDS && tid <= last) {
        s_end[tid] = seg_end[first + tid];
        s_gid[tid] = seg_group[first + tid];
    }
    __syncthreads();
    auto end_at = [&](int c) -> long { return c < SEG_LDS ? s_end[c] : seg_end[first + c]; };
    auto gid_at = [&](int c) -> int {
        const int gid = c < SEG_LDS ? s_gid[c] : seg_group[first + c];
        return gid < 0 ? 0 : gid >= ngroups ? ngroups - 1 : gid;
    };

    int cur = 0;
    for (int it = 0; it < GROUP_ITERS; ++it) {
        const long i = chunk0 + (long)it * 1024 + tid * 4;
        if (i >= n) break;
        while (cur < last && end_at(cur) <= i) ++cur;
        if (i + 3 < n) {
            float4 pv = *reinterpret_cast<float4*>(p + i);
            const float4 gv = *reinterpret_cast<const float4*>(g + i);
            float lr[4], wd[4], a0[4], a1[4];
            if (cur >= last || end_at(cur) >= i + 4) {
                const int gid = gid_at(cur);
#pragma unroll
                for (int j = 0; j < 4; ++j) { lr[j] = s_lr[gid]; wd[j] = s_wd[gid]; a0[j] = s_a0[gid]; a1[j] = s_a1[gid]; }
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    while (cur < last && end_at(cur) <= i + j) ++cur;
                    const int gid = gid_at(cur);
                    lr[j] = s_lr[gid]; wd[j] = s_wd[gid]; a0[j] = s_a0[gid]; a1[j] = s_a1[gid];
                }
            }
            op.quad(i, &pv.x, &gv.x, lr, wd, a0, a1, gscale);
            *reinterpret_cast<float4*>(p + i) = pv;
            if (zero_grad) *reinterpret_cast<float4*>(g + i) = zero4;
        } else {
            for (long k = i; k < n; ++k) {
                while (cur < last && end_at(cur) <= k) ++cur;
                const int gid = gid_at(cur);
                float pk = p[k];
                op.elem(k, pk, g[k], s_lr[gid], s_wd[gid], s_a0[gid], s_a1[gid], gscale);
                p[k] = pk;
                if (zero_grad) g[k] = 0.f;
            }
        }
    }
}

inline long chunks_of(long n, long chunk) { return (n + chunk - 1) / chunk; }

int fill_group_table(GroupTable* tab, const float* lr, const float* wd, int ngroups) {
    if (!lr || !wd || ngroups < 1 || ngroups > MAX_GROUPS) return ISTVT_ERR_SHAPE;
    for (int i = 0; i < MAX_GROUPS; ++i) {
        tab->lr[i] = lr[i < ngroups ? i : 0];
        tab->wd[i] = wd[i < ngroups ? i : 0];
        tab->a0[i] = tab->a1[i] = 0.f;
    }
    return ISTVT_OK;
}

}  // namespace

extern "C" int istvt_sgd_momentum(float* p, float* g, float* buf, long n, float lr, float momentum, float dampening,
                                  float weight_decay, int nesterov, int first_step, int zero_grad, float grad_scale,
                                  hipStream_t stream) {
    if (n <= 0 || !p || !g || !buf) return ISTVT_ERR_SHAPE;
    if (((uintptr_t)p | (uintptr_t)g | (uintptr_t)buf) & 15) return ISTVT_ERR_SHAPE;
    if (momentum == 0.f) dampening = 0.f;          // torch.optim.SGD ignores dampening without momentum (d_p = g')
    hipLaunchKernelGGL(sgd_momentum_kernel, dim3(opt_grid(n, 4)), dim3(256), 0, stream, p, g, buf, n, lr, momentum,
                       dampening, weight_decay, nesterov, first_step, zero_grad, grad_scale);
    return istvt_check_launch();
}

extern "C" int istvt_adamw(float* p, float* g, float* m, float* v, long n, float lr, float beta1, float beta2, float eps,
                           float weight_decay, long step, int zero_grad, float grad_scale, hipStream_t stream) {
    if (n <= 0 || step < 1 || !p || !g || !m || !v) return ISTVT_ERR_SHAPE;
    const double bc1 = 1.0 - pow((double)beta1, (double)step), bc2 = 1.0 - pow((double)beta2, (double)step);
    hipLaunchKernelGGL(adamw_kernel, dim3(opt_grid(n, 1)), dim3(256), 0, stream, p, g, m, v, n, lr, beta1, beta2, eps,
                       weight_decay, (float)(lr / bc1), (float)(1.0 / sqrt(bc2)), zero_grad, grad_scale);
    return istvt_check_launch();
}

extern "C" int istvt_grad_norm_ws_elems(long n) {
    const long b = n < 1 ? 1 : chunks_of(n, NORM_CHUNK);
    return b > 0x7fffffffL ? -1 : (int)b;
}

extern "C" int istvt_grad_norm(const float* g, long n, float grad_scale, float max_norm, int skip_nonfinite, double* ws,
                               long ws_elems, void* info, hipStream_t stream) {
    if (n <= 0 || !g || !ws || !info) return ISTVT_ERR_SHAPE;
    if (((uintptr_t)g & 15) || ((uintptr_t)ws & 7) || ((uintptr_t)info & 3)) return ISTVT_ERR_SHAPE;
    const long blocks = chunks_of(n, NORM_CHUNK);
    if (blocks > 0x7fffffffL || ws_elems < blocks) return ISTVT_ERR_SHAPE;
    hipLaunchKernelGGL(grad_norm_partial_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, g, n, grad_scale, ws);
    hipLaunchKernelGGL(grad_norm_final_kernel, dim3(1), dim3(256), 0, stream, (const double*)ws, blocks, grad_scale,
                       max_norm, skip_nonfinite != 0, (StepInfo*)info);
    return istvt_check_launch();
}

static int grouped_args_ok(long n, const long* seg_end, const int* seg_group, int nseg, const void* info, int skip) {
    if (n <= 0 || !seg_end || !seg_group || nseg < 1) return 0;
    if (skip && !info) return 0;
    return chunks_of(n, GROUP_CHUNK) <= 0x7fffffffL;
}

extern "C" int istvt_sgd_momentum_groups(float* p, float* g, float* buf, long n, const long* seg_end, const int* seg_group,
                                         int nseg, const float* group_lr, const float* group_wd, int ngroups,
                                         float momentum, float dampening, int nesterov, int first_step, int zero_grad,
                                         float grad_scale, const void* info, int skip_nonfinite, hipStream_t stream) {
    if (!p || !g || !buf || !grouped_args_ok(n, seg_end, seg_group, nseg, info, skip_nonfinite)) return ISTVT_ERR_SHAPE;
    if (((uintptr_t)p | (uintptr_t)g | (uintptr_t)buf) & 15) return ISTVT_ERR_SHAPE;
    GroupTable tab;
    if (fill_group_table(&tab, group_lr, group_wd, ngroups) != ISTVT_OK) return ISTVT_ERR_SHAPE;
    if (momentum == 0.f) dampening = 0.f;
    SgdGroupOp op{buf, momentum, dampening, nesterov, first_step};
    hipLaunchKernelGGL(grouped_step_kernel<SgdGroupOp>, dim3((unsigned)chunks_of(n, GROUP_CHUNK)), dim3(256), 0, stream, op,
                       p, g, n, seg_end, seg_group, nseg, tab, ngroups, (const StepInfo*)info, grad_scale,
                       skip_nonfinite != 0, zero_grad);
    return istvt_check_launch();
}

extern "C" int istvt_adamw_groups(float* p, float* g, float* m, float* v, long n, const long* seg_end, const int* seg_group,
                                  int nseg, const float* group_lr, const float* group_wd, int ngroups, float beta1,
                                  float beta2, float eps, long step, int zero_grad, float grad_scale, const void* info,
                                  int skip_nonfinite, hipStream_t stream) {
    if (!p || !g || !m || !v || !grouped_args_ok(n, seg_end, seg_group, nseg, info, skip_nonfinite)) return ISTVT_ERR_SHAPE;
    if (((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v) & 15) return ISTVT_ERR_SHAPE;
    if (!skip_nonfinite && step < 1) return ISTVT_ERR_SHAPE;
    GroupTable tab;
    if (fill_group_table(&tab, group_lr, group_wd, ngroups) != ISTVT_OK) return ISTVT_ERR_SHAPE;
    if (step < 1) step = 1;
    const double bc1 = 1.0 - pow((double)beta1, (double)step), bc2 = 1.0 - pow((double)beta2, (double)step);
    for (int i = 0; i < MAX_GROUPS; ++i) {      // what istvt_adamw hands its kernel, per group
        tab.a0[i] = (float)(tab.lr[i] / bc1);
        tab.a1[i] = (float)(1.0 / sqrt(bc2));
    }
    AdamwGroupOp op{m, v, beta1, beta2, eps};
    hipLaunchKernelGGL(grouped_step_kernel<AdamwGroupOp>, dim3((unsigned)chunks_of(n, GROUP_CHUNK)), dim3(256), 0, stream, op,
                       p, g, n, seg_end, seg_group, nseg, tab, ngroups, (const StepInfo*)info, grad_scale,
                       skip_nonfinite != 0, zero_grad);
    return istvt_check_launch();
}
