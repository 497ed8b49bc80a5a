// The optimizer step of the training loop (main.py:107: torch.optim.Adam, lr 1e-3, weight decay 1e-4) as ONE launch over the flat
// gradient bucket.  torch's fused Adam takes six multi-tensor launches for the model's 182 parameter tensors (0.16 ms at the very
// end of a step, where nothing overlaps it); here the gradients, first and second moments are three flat arrays in bucket order and
// only the parameters stay where the module holds them (a table of their addresses and bucket offsets).  Same update rule, in
// torch's order of operations (torch/optim/adam.py, `_fused_adam`; L2 weight decay added to the gradient, no amsgrad):
//   g' = g + wd p;  m += (1 - b1) (g' - m);  v = b2 v + (1 - b2) g' g';  p -= (lr / (1 - b1^t)) m / (sqrt(v) / sqrt(1 - b2^t) + eps)
#include <cmath>
#include <cstdint>
#include "cmf_common.h"
#include "../../include/cmflow_hip.h"

constexpr int AD_THREADS = 256;
constexpr int AD_CHUNK = 1024;                 // bucket elements per workgroup

// EMA: the running average of the parameters rides in the same launch -- ema[e] += omd (pn - ema[e]) with pn the value just stored, one
// explicit fmaf (no contraction choice), omd = (float)(1 - decay).  The lerp form's fixed point is pn itself: pn == ev gives ev back bit for
// bit, where d ev + (1 - d) pn carries a relative bias of 2^-24 / (1 - d).  EMA = false is the kernel without it, expression for expression.
template <bool EMA>
__global__ __launch_bounds__(AD_THREADS) void adam_flat_kernel(int n_tensors, const long long *__restrict__ offsets /* [n + 1] */,
                                                               float *const *__restrict__ params, long long total,
                                                               const float *__restrict__ grad, float *__restrict__ m, float *__restrict__ v,
                                                               float wd, float b1w, float b2, float b2w, float step_size, float bc2_sqrt, float eps,
                                                               float *__restrict__ ema, float omd)
{
    const long long e0 = (long long)blockIdx.x * AD_CHUNK;
    // the tensor that holds the chunk's first element (binary search, one lane's worth of work), then a walk: most chunks lie in one tensor
    int t = 0;
    {
        int lo = 0, hi = n_tensors;            // offsets[lo] <= e0 < offsets[hi]
        while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (offsets[mid] <= e0) lo = mid; else hi = mid; }
        t = lo;
    }
    for (int i = threadIdx.x; i < AD_CHUNK; i += AD_THREADS) {
        const long long e = e0 + i;
        if (e >= total) return;
        int tt = t;
        while (offsets[tt + 1] <= e) ++tt;
        float *p = params[tt] + (e - offsets[tt]);
        const float pv = *p;
        const float g = fmaf(wd, pv, grad[e]);
        const float mv = m[e], vv = v[e];
        const float mn = mv + b1w * (g - mv);
        const float vn = b2 * vv + b2w * (g * g);
        m[e] = mn; v[e] = vn;
        const float denom = sqrtf(vn) / bc2_sqrt + eps;
        const float pn = pv - step_size * (mn / denom);
        *p = pn;
        if (EMA) { const float ev = ema[e]; ema[e] = fmaf(omd, pn - ev, ev); }
    }
}

// The hyper-parameters arrive as doubles (Python floats) and every derived scalar is formed in double before it is rounded to fp32
// once, as torch does: 1 - beta is (float)(1.0 - beta), not 1.f - (float)beta (those differ by 1e-5 relative for beta2 = 0.999).
// ema == nullptr: the step without the average (ema_decay is not read).
static int adam_launch(int n_tensors, const long long *offsets, float *const *params, long long total, const float *grad, float *m, float *v,
                       double lr, double beta1, double beta2, double eps, double weight_decay, long long step, float *ema, double ema_decay,
                       void *stream)
{
    CMF_CHECK_ARG(n_tensors > 0 && offsets && params && total > 0 && grad && m && v && step >= 1 && lr >= 0.0);
    const double bc1 = 1.0 - pow(beta1, (double)step), bc2 = 1.0 - pow(beta2, (double)step);
    const auto kernel = ema ? adam_flat_kernel<true> : adam_flat_kernel<false>;
    hipLaunchKernelGGL(kernel, dim3((unsigned)cmf_divup(total, AD_CHUNK)), dim3(AD_THREADS), 0, (hipStream_t)stream, n_tensors, offsets,
                       params, total, grad, m, v, (float)weight_decay, (float)(1.0 - beta1), (float)beta2, (float)(1.0 - beta2), (float)(lr / bc1),
                       (float)sqrt(bc2), (float)eps, ema, ema ? (float)(1.0 - ema_decay) : 0.f);
    return cmf_launch_status();
}

static int ema_check(const float *ema, double ema_decay)
{
    CMF_CHECK_ARG(ema && ((uintptr_t)ema & 3) == 0 && ema_decay > 0.0 && ema_decay < 1.0);      // a NaN decay fails both comparisons
    return 0;
}

extern "C" int cmf_adam_step(int n_tensors, const long long *offsets, float *const *params, long long total, const float *grad, float *m,
                             float *v, double lr, double beta1, double beta2, double eps, double weight_decay, long long step, void *stream)
{
    return adam_launch(n_tensors, offsets, params, total, grad, m, v, lr, beta1, beta2, eps, weight_decay, step, nullptr, 0.0, stream);
}

extern "C" int cmf_adam_step_ema(int n_tensors, const long long *offsets, float *const *params, long long total, const float *grad, float *m,
                                 float *v, double lr, double beta1, double beta2, double eps, double weight_decay, long long step, float *ema,
                                 double ema_decay, void *stream)
{
    if (int err = ema_check(ema, ema_decay)) return err;
    return adam_launch(n_tensors, offsets, params, total, grad, m, v, lr, beta1, beta2, eps, weight_decay, step, ema, ema_decay, stream);
}

// Every parameter element swapped with flat[e], through the Adam kernel's address table and chunk walk: pure copies, so a second call
// undoes the first bit for bit.
__global__ __launch_bounds__(AD_THREADS) void param_exchange_kernel(int n_tensors, const long long *__restrict__ offsets /* [n + 1] */,
                                                                    float *const *__restrict__ params, long long total,
                                                                    float *__restrict__ flat)
{
    const long long e0 = (long long)blockIdx.x * AD_CHUNK;
    int t = 0;
    {
        int lo = 0, hi = n_tensors;            // offsets[lo] <= e0 < offsets[hi]
        while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (offsets[mid] <= e0) lo = mid; else hi = mid; }
        t = lo;
    }
    for (int i = threadIdx.x; i < AD_CHUNK; i += AD_THREADS) {
        const long long e = e0 + i;
        if (e >= total) return;
        int tt = t;
        while (offsets[tt + 1] <= e) ++tt;
        float *p = params[tt] + (e - offsets[tt]);
        const float pv = *p, fv = flat[e];
        *p = fv; flat[e] = pv;
    }
}

extern "C" int cmf_param_exchange(int n_tensors, const long long *offsets, float *const *params, long long total, float *flat, void *stream)
{
    CMF_CHECK_ARG(n_tensors > 0 && offsets && params && total > 0 && flat && ((uintptr_t)flat & 3) == 0);
    hipLaunchKernelGGL(param_exchange_kernel, dim3((unsigned)cmf_divup(total, AD_CHUNK)), dim3(AD_THREADS), 0, (hipStream_t)stream, n_tensors,
                       offsets, params, total, flat);
    return cmf_launch_status();
}

// ---- guarded step: gradient norm, clipping, non-finite skip ---------------------------------------------------------------------------
// The sum of squares of the bucket in double, deterministic: the partition below is a function of `total` alone, every lane adds its
// elements in a fixed order, and the folds are fixed trees -- no atomics.  The square of an fp32 value is exact in double (24 + 24 bits),
// so only the additions round: relative error <= (total - 1) 2^-53 whatever the order (all terms are >= 0).  A NaN or +-Inf element makes
// its partial non-finite by itself; finite fp32 values cannot overflow a double sum of squares (3.4e38^2 * 2^63 < 1.8e308).
constexpr int GN_SLAB = 1024;                  // elements; a workgroup owns whole slabs, so its float4 loads stay aligned
constexpr int GN_MAX_PARTS = 256;              // = the fold's one partial per lane
constexpr int GN_MIN_SLABS = 4;                // below 4 slabs a workgroup a launch of more workgroups buys nothing
static_assert(GN_MAX_PARTS == AD_THREADS, "the fold takes one partial per lane");

extern "C" int cmf_grad_norm_parts(long long total)
{
    if (total <= 0) return 0;
    const long long slabs = (total + GN_SLAB - 1) / GN_SLAB;
    const long long parts = (slabs + GN_MIN_SLABS - 1) / GN_MIN_SLABS;
    return (int)(parts < GN_MAX_PARTS ? parts : GN_MAX_PARTS);
}

// lanes 63..0 of every wave into lane 0 (fixed tree), the waves' sums through LDS, then ((w0 + w1) + (w2 + w3)) in EVERY lane.
// Once per kernel (a second call would need a barrier in front of the LDS stores).
__device__ __forceinline__ double gn_block_sum(double x)
{
    __shared__ double wave_sum[AD_THREADS / CMF_WAVE];
    for (int off = CMF_WAVE / 2; off > 0; off >>= 1) x += __shfl_down(x, off, CMF_WAVE);
    if ((threadIdx.x & (CMF_WAVE - 1)) == 0) wave_sum[threadIdx.x / CMF_WAVE] = x;
    __syncthreads();
    return (wave_sum[0] + wave_sum[1]) + (wave_sum[2] + wave_sum[3]);
}
static_assert(AD_THREADS / CMF_WAVE == 4, "gn_block_sum adds four waves");

// The fold of the partials, shared by the stand-alone norm and the guarded step so that both see the same bits: partial i in lane i
// (+0 where there is none: exact), then gn_block_sum.  Called by all AD_THREADS lanes of a workgroup; every lane gets the sum.
__device__ __forceinline__ double gn_fold_partials(const double *__restrict__ partials, int parts)
{
    return gn_block_sum((int)threadIdx.x < parts ? partials[threadIdx.x] : 0.0);
}

__global__ __launch_bounds__(AD_THREADS) void grad_sumsq_kernel(long long total, const float *__restrict__ grad, double *__restrict__ partials)
{
    const long long slabs = (total + GN_SLAB - 1) / GN_SLAB;
    const long long s0 = (long long)blockIdx.x * slabs / gridDim.x, s1 = (long long)(blockIdx.x + 1) * slabs / gridDim.x;
    const long long e0 = s0 * GN_SLAB, e1 = s1 * GN_SLAB < total ? s1 * GN_SLAB : total;      // only the last workgroup has a ragged end
    const long long nvec = (e1 - e0) >> 2;
    const float4 *__restrict__ g4 = reinterpret_cast<const float4 *>(grad + e0);
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
#pragma unroll 4
    for (long long i = threadIdx.x; i < nvec; i += AD_THREADS) {
        const float4 x = g4[i];
        a0 += (double)x.x * (double)x.x; a1 += (double)x.y * (double)x.y;
        a2 += (double)x.z * (double)x.z; a3 += (double)x.w * (double)x.w;
    }
    const long long et = e0 + (nvec << 2) + threadIdx.x;       // the last total % 4 elements, one lane each
    if (et < e1) { const float x = grad[et]; a0 += (double)x * (double)x; }
    const double sum = gn_block_sum((a0 + a1) + (a2 + a3));
    if (threadIdx.x == 0) partials[blockIdx.x] = sum;
}

__global__ __launch_bounds__(AD_THREADS) void grad_norm_fold_kernel(const double *__restrict__ partials, int parts, double *__restrict__ out)
{
    const double sumsq = gn_fold_partials(partials, parts);
    if (threadIdx.x == 0) { out[0] = sumsq; out[1] = sqrt(sumsq); }
}

// adam_flat_kernel behind a prologue: every workgroup folds the partials (2 KB, L2-resident) and derives the same decision.  The
// update below is adam_flat_kernel's, expression for expression; with scale = 1 (grad[e] * 1.f is grad[e]) it gives the same bits.
template <bool EMA>
__global__ __launch_bounds__(AD_THREADS) void adam_flat_guarded_kernel(int n_tensors, const long long *__restrict__ offsets /* [n + 1] */,
                                                                       float *const *__restrict__ params, long long total,
                                                                       const float *__restrict__ grad, float *__restrict__ m, float *__restrict__ v,
                                                                       float wd, float b1w, float b2, float b2w, float step_size, float bc2_sqrt,
                                                                       float eps, const double *__restrict__ partials, int parts, int clip_on,
                                                                       float max_norm, int skip, double *__restrict__ record,
                                                                       float *__restrict__ ema, float omd)
{
    const double sumsq = gn_fold_partials(partials, parts);
    const float normf = (float)sqrt(sumsq);
    const bool nonfinite = !isfinite(sumsq);
    float scale = 1.f;
    if (!nonfinite && clip_on) { const float coef = max_norm / (normf + 1e-6f); scale = coef < 1.f ? coef : 1.f; }
    if (blockIdx.x == 0 && threadIdx.x == 0) {                 // nobody else touches `record` in this launch
        record[0] += 1.0;
        if (nonfinite) record[1] += 1.0;
        else {
            if (scale < 1.f) record[2] += 1.0;
            record[3] += (double)normf;
            if ((double)normf > record[4]) record[4] = (double)normf;
        }
        record[5] = sumsq; record[6] = (double)normf; record[7] = (double)scale;
    }
    if (nonfinite && skip) return;                             // before any store to p, m, v, ema

    const long long e0 = (long long)blockIdx.x * AD_CHUNK;
    int t = 0;
    {
        int lo = 0, hi = n_tensors;            // offsets[lo] <= e0 < offsets[hi]
        while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (offsets[mid] <= e0) lo = mid; else hi = mid; }
        t = lo;
    }
    for (int i = threadIdx.x; i < AD_CHUNK; i += AD_THREADS) {
        const long long e = e0 + i;
        if (e >= total) return;
        int tt = t;
        while (offsets[tt + 1] <= e) ++tt;
        float *p = params[tt] + (e - offsets[tt]);
        const float pv = *p;
        const float gs = grad[e] * scale;
        const float g = fmaf(wd, pv, gs);
        const float mv = m[e], vv = v[e];
        const float mn = mv + b1w * (g - mv);
        const float vn = b2 * vv + b2w * (g * g);
        m[e] = mn; v[e] = vn;
        const float denom = sqrtf(vn) / bc2_sqrt + eps;
        const float pn = pv - step_size * (mn / denom);
        *p = pn;
        if (EMA) { const float ev = ema[e]; ema[e] = fmaf(omd, pn - ev, ev); }
    }
}

static int gn_check(long long total, const float *grad, const double *partials)
{
    CMF_CHECK_ARG(total > 0 && grad && partials && ((uintptr_t)grad & 15) == 0 && ((uintptr_t)partials & 7) == 0);
    return 0;
}

extern "C" int cmf_grad_sumsq(long long total, const float *grad, double *partials, void *stream)
{
    if (int err = gn_check(total, grad, partials)) return err;
    hipLaunchKernelGGL(grad_sumsq_kernel, dim3((unsigned)cmf_grad_norm_parts(total)), dim3(AD_THREADS), 0, (hipStream_t)stream, total, grad,
                       partials);
    return cmf_launch_status();
}

extern "C" int cmf_grad_norm(long long total, const float *grad, double *partials, double *out, void *stream)
{
    CMF_CHECK_ARG(out && ((uintptr_t)out & 7) == 0);
    if (int err = cmf_grad_sumsq(total, grad, partials, stream)) return err;
    hipLaunchKernelGGL(grad_norm_fold_kernel, dim3(1), dim3(AD_THREADS), 0, (hipStream_t)stream, partials, cmf_grad_norm_parts(total), out);
    return cmf_launch_status();
}

static int adam_guarded_launch(int n_tensors, const long long *offsets, float *const *params, long long total, const float *grad, float *m,
                               float *v, double lr, double beta1, double beta2, double eps, double weight_decay, long long step,
                               double max_grad_norm, int skip_nonfinite, const double *partials, double *record, float *ema,
                               double ema_decay, void *stream)
{
    CMF_CHECK_ARG(n_tensors > 0 && offsets && params && total > 0 && grad && m && v && step >= 1 && lr >= 0.0);
    CMF_CHECK_ARG(partials && record && ((uintptr_t)partials & 7) == 0 && ((uintptr_t)record & 7) == 0 && !std::isnan(max_grad_norm));
    const int clip_on = max_grad_norm > 0.0 && std::isfinite(max_grad_norm);
    const double bc1 = 1.0 - pow(beta1, (double)step), bc2 = 1.0 - pow(beta2, (double)step);
    const auto kernel = ema ? adam_flat_guarded_kernel<true> : adam_flat_guarded_kernel<false>;
    hipLaunchKernelGGL(kernel, dim3((unsigned)cmf_divup(total, AD_CHUNK)), dim3(AD_THREADS), 0, (hipStream_t)stream,
                       n_tensors, offsets, params, total, grad, m, v, (float)weight_decay, (float)(1.0 - beta1), (float)beta2,
                       (float)(1.0 - beta2), (float)(lr / bc1), (float)sqrt(bc2), (float)eps, partials, cmf_grad_norm_parts(total), clip_on,
                       clip_on ? (float)max_grad_norm : 0.f, skip_nonfinite != 0, record, ema, ema ? (float)(1.0 - ema_decay) : 0.f);
    return cmf_launch_status();
}

extern "C" int cmf_adam_step_guarded(int n_tensors, const long long *offsets, float *const *params, long long total, const float *grad,
                                     float *m, float *v, double lr, double beta1, double beta2, double eps, double weight_decay,
                                     long long step, double max_grad_norm, int skip_nonfinite, const double *partials, double *record,
                                     void *stream)
{
    return adam_guarded_launch(n_tensors, offsets, params, total, grad, m, v, lr, beta1, beta2, eps, weight_decay, step, max_grad_norm,
                               skip_nonfinite, partials, record, nullptr, 0.0, stream);
}

extern "C" int cmf_adam_step_guarded_ema(int n_tensors, const long long *offsets, float *const *params, long long total, const float *grad,
                                         float *m, float *v, double lr, double beta1, double beta2, double eps, double weight_decay,
                                         long long step, double max_grad_norm, int skip_nonfinite, const double *partials, double *record,
                                         float *ema, double ema_decay, void *stream)
{
    if (int err = ema_check(ema, ema_decay)) return err;
    return adam_guarded_launch(n_tensors, offsets, params, total, grad, m, v, lr, beta1, beta2, eps, weight_decay, step, max_grad_norm,
                               skip_nonfinite, partials, record, ema, ema_decay, stream);
}
