// optim.hip -- Keras Adam(amsgrad=True) (train_model.py:120) fused with the L2
// regulariser gradient 2*lambda*w of networks.py:456-460 (kernel AND bias; App. C-7), on flat fp32 buffers.
//   lr_t = lr*sqrt(1-b2^t)/(1-b1^t);  m,v EMA;  vhat = max(vhat, v);  w -= lr_t*m/(sqrt(vhat)+eps)
// lr and the step counter live in device memory so that a captured hipGraph can be replayed.
//
// The guarded step (Keras' clipvalue / global_clipnorm, plus a skip of non-finite gradients) is three more launches around the same
// update, all deciding on the device so that the captured step needs no host look at the gradient:
//   grad_norm_kernel     one fp64 partial of sum(clamp(gr)^2) per block into a workspace (no atomics, fixed grid)
//   grad_control_kernel  one block folds the partials in a fixed order and writes the 16-byte record m1_step_ctl_t
//   adam_amsgrad_kernel  <true>: the update on clamp(gr) * coef, or nothing at all when the record says apply == 0
//   step_inc_ctl_kernel  step += apply
// gr = g*grad_scale + 2*lambda*p is the regularised gradient: Keras clips what the optimiser receives, the regulariser's part included,
// clipvalue first, and takes the global norm over the clamped values.
#include "common.h"

__device__ __forceinline__ float adam_lambda(long long idx, long long n_kernel, long long n_bias, float l2k, float l2b) {
    return idx < n_kernel ? l2k : (idx < n_kernel + n_bias ? l2b : 0.f);
}
// the regularised gradient of one element
__device__ __forceinline__ float adam_gr(float g, float p, float lam, float gscale) { return g * gscale + 2.f * lam * p; }
// clip_by_value: NaN stays NaN (both comparisons are false), +-Inf becomes +-cv; cv = +Inf switches it off
__device__ __forceinline__ float adam_clamp(float gr, float cv) { return gr < -cv ? -cv : (gr > cv ? cv : gr); }
// one element of the update; returns the new weight
__device__ __forceinline__ float adam_update(float p, float gr, float& m, float& v, float& vhat, float lr_t, float b1, float b2,
                                             float eps) {
    m = b1 * m + (1.f - b1) * gr;
    v = b2 * v + (1.f - b2) * gr * gr;
    vhat = fmaxf(vhat, v);
    return p - lr_t * m / (sqrtf(vhat) + eps);
}

// CTL: the guarded update -- ctl (m1_step_ctl_t) holds coef at [1] and apply at [2]; cv = clipvalue or +Inf
template <bool CTL>
__global__ void __launch_bounds__(256) adam_amsgrad_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                           float* __restrict__ v, float* __restrict__ vhat, long long n,
                                                           long long n_kernel, long long n_bias, float l2k, float l2b,
                                                           float gscale, const float* __restrict__ lr_dev, float b1, float b2,
                                                           float eps, const int* __restrict__ step_dev, float cv,
                                                           const float* __restrict__ ctl) {
    float coef = 1.f;
    if (CTL) {
        if (reinterpret_cast<const int*>(ctl)[2] == 0) return;          // skipped step: p, m, v, vhat keep their bits
        coef = ctl[1];
    }
    const int t = step_dev[0];
    const float lr_t = lr_dev[0] * sqrtf(1.f - powf(b2, (float)t)) / (1.f - powf(b1, (float)t));
    const long long n4 = n >> 2;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n4 + (n & 3); i += (long long)gridDim.x * blockDim.x) {
        if (i < n4) {
            const long long e = i << 2;
            float4 pv = *reinterpret_cast<float4*>(p + e), gv = *reinterpret_cast<const float4*>(g + e);
            float4 mv = *reinterpret_cast<float4*>(m + e), vv = *reinterpret_cast<float4*>(v + e), hv = *reinterpret_cast<float4*>(vhat + e);
            float pp[4] = {pv.x, pv.y, pv.z, pv.w}, gg[4] = {gv.x, gv.y, gv.z, gv.w}, mm[4] = {mv.x, mv.y, mv.z, mv.w};
            float vq[4] = {vv.x, vv.y, vv.z, vv.w}, hh[4] = {hv.x, hv.y, hv.z, hv.w};
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                float gr = adam_gr(gg[k], pp[k], adam_lambda(e + k, n_kernel, n_bias, l2k, l2b), gscale);
                if (CTL) gr = adam_clamp(gr, cv) * coef;
                pp[k] = adam_update(pp[k], gr, mm[k], vq[k], hh[k], lr_t, b1, b2, eps);
            }
            *reinterpret_cast<float4*>(p + e) = make_float4(pp[0], pp[1], pp[2], pp[3]);
            *reinterpret_cast<float4*>(m + e) = make_float4(mm[0], mm[1], mm[2], mm[3]);
            *reinterpret_cast<float4*>(v + e) = make_float4(vq[0], vq[1], vq[2], vq[3]);
            *reinterpret_cast<float4*>(vhat + e) = make_float4(hh[0], hh[1], hh[2], hh[3]);
        } else {
            const long long idx = (n4 << 2) + (i - n4);
            float gr = adam_gr(g[idx], p[idx], adam_lambda(idx, n_kernel, n_bias, l2k, l2b), gscale);
            if (CTL) gr = adam_clamp(gr, cv) * coef;
            float mm = m[idx], vq = v[idx], hh = vhat[idx];
            const float pn = adam_update(p[idx], gr, mm, vq, hh, lr_t, b1, b2, eps);
            m[idx] = mm; v[idx] = vq; vhat[idx] = hh;
            p[idx] = pn;
        }
    }
}

// sum over a block of 256 threads, valid in thread 0: wave shuffles, then the four wave sums through LDS in a fixed order
__device__ __forceinline__ double block_sum_d(double acc) {
    __shared__ double ws_[4];
    acc = wave_sum_d(acc);
    if ((threadIdx.x & 63) == 0) ws_[threadIdx.x >> 6] = acc;
    __syncthreads();
    return (ws_[0] + ws_[1]) + (ws_[2] + ws_[3]);
}

// partial[blockIdx.x] = sum over this block's elements of clamp(gr)^2, squared and accumulated in fp64: a finite fp32 gradient cannot
// overflow the sum (|gr| <= 3.4e38 -> gr^2 <= 1.2e77), NaN and Inf reach it.  L2: some lambda is non-zero, p is read; otherwise
// gr = g*grad_scale and p is never touched.  Same element walk as adam_amsgrad_kernel: float4 body, scalar tail of n & 3 elements.
template <bool L2>
__global__ void __launch_bounds__(256) grad_norm_kernel(const float* __restrict__ g, const float* __restrict__ p, long long n,
                                                        long long n_kernel, long long n_bias, float l2k, float l2b, float gscale,
                                                        float cv, double* __restrict__ partial) {
    double acc = 0.0;
    const long long n4 = n >> 2;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n4 + (n & 3); i += (long long)gridDim.x * blockDim.x) {
        if (i < n4) {
            const long long e = i << 2;
            const float4 gv = *reinterpret_cast<const float4*>(g + e);
            float4 pv = make_float4(0.f, 0.f, 0.f, 0.f);
            if (L2) pv = *reinterpret_cast<const float4*>(p + e);
            const float gg[4] = {gv.x, gv.y, gv.z, gv.w}, pp[4] = {pv.x, pv.y, pv.z, pv.w};
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float lam = L2 ? adam_lambda(e + k, n_kernel, n_bias, l2k, l2b) : 0.f;
                const double d = (double)adam_clamp(adam_gr(gg[k], pp[k], lam, gscale), cv);
                acc += d * d;
            }
        } else {
            const long long idx = (n4 << 2) + (i - n4);
            const float lam = L2 ? adam_lambda(idx, n_kernel, n_bias, l2k, l2b) : 0.f;
            const double d = (double)adam_clamp(adam_gr(g[idx], L2 ? p[idx] : 0.f, lam, gscale), cv);
            acc += d * d;
        }
    }
    acc = block_sum_d(acc);
    if (threadIdx.x == 0) partial[blockIdx.x] = acc;
}

// one block: thread t adds partial[t], partial[t + 256], ... in that order, then the block fold; thread 0 writes the record
__global__ void __launch_bounds__(256) grad_control_kernel(const double* __restrict__ partial, int nparts, float clipnorm, int guard,
                                                           int* __restrict__ ctl) {
    double acc = 0.0;
    for (int i = threadIdx.x; i < nparts; i += 256) acc += partial[i];
    const double sum = block_sum_d(acc);
    if (threadIdx.x != 0) return;
    const bool finite = sum - sum == 0.0;                      // false for NaN and +Inf
    const double norm = sqrt(sum);
    const float normf = (float)norm;
    float coef = 1.f;
    int apply = 1, skipped = ctl[3];
    if (!finite && guard) { apply = 0; skipped += 1; }
    else if (clipnorm > 0.f) {
        if (!finite) coef = __int_as_float(0x7fc00000);        // tf.clip_by_global_norm: a non-finite norm poisons every gradient
        else if (normf > clipnorm) coef = (float)((double)clipnorm / norm);
    }
    *reinterpret_cast<int4*>(ctl) = make_int4(__float_as_int(normf), __float_as_int(coef), apply, skipped);
}

__global__ void step_inc_kernel(int* step, unsigned long long* rng) { if (step) step[0] += 1; if (rng) rng[1] += 1; }
__global__ void step_inc_ctl_kernel(int* step, const int* ctl) { step[0] += ctl[2]; }

static inline long long adam_blocks(long long n) { long long b = cdiv_ll((n >> 2) + 3, 256); return b > 4096 ? 4096 : b; }
// blocks of the norm pass: a function of n and M1_EW_BLOCKS only (never of the device or of what else runs), at most 2048 -- the
// partial sums, and with them every bit of the norm, are the same on every run
static inline int grad_norm_blocks(long long n, int cap) {
    if (cap < 1) cap = 1;
    if (cap > 2048) cap = 2048;
    const long long b = cdiv_ll((n >> 2) + 3, 256);
    return (int)(b > cap ? cap : b);
}

static bool adam_args_ok(const float* p, const float* g, const float* m, const float* v, const float* vhat, const float* lr_dev,
                         const int* step_dev, long long n) {
    if (!p || !g || !m || !v || !vhat || !lr_dev || !step_dev || n <= 0) return false;
    return !(((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v | (uintptr_t)vhat) & 15);
}
static inline bool clip_ok(float c) { return c >= 0.f && c <= 3.4028234e38f; }       // 0 = off; NaN, negative and Inf are rejected

extern "C" int m1_adam_amsgrad(float* p, const float* g, float* m, float* v, float* vhat, long long n, long long n_kernel,
                               long long n_bias, float l2_kernel, float l2_bias, float grad_scale, const float* lr_dev,
                               float beta1, float beta2, float eps, const int* step_dev, void* stream) {
    if (m1_debug_skip("adam")) return M1_OK;
    if (!adam_args_ok(p, g, m, v, vhat, lr_dev, step_dev, n)) return M1_ERR_BAD_ARG;
    M1ProfScope ps("adam_amsgrad", 0.0, 36.0 * n, (hipStream_t)stream);
    hipLaunchKernelGGL(adam_amsgrad_kernel<false>, dim3((unsigned)adam_blocks(n)), dim3(256), 0, (hipStream_t)stream, p, g, m, v, vhat,
                       n, n_kernel, n_bias, l2_kernel, l2_bias, grad_scale, lr_dev, beta1, beta2, eps, step_dev, 0.f,
                       (const float*)nullptr);
    return m1_check_launch();
}

extern "C" size_t m1_grad_norm_ws(long long n) {
    return n <= 0 ? 0 : sizeof(double) * (size_t)grad_norm_blocks(n, 2048);      // sized for the largest grid any M1_EW_BLOCKS gives
}

extern "C" int m1_grad_norm(const float* g, const float* p, long long n, long long n_kernel, long long n_bias, float l2_kernel,
                            float l2_bias, float grad_scale, float clipvalue, float global_clipnorm, int skip_nonfinite, void* ws,
                            size_t ws_bytes, m1_step_ctl_t* ctl, void* stream) {
    if (!g || !p || !ws || !ctl || n <= 0 || !clip_ok(clipvalue) || !clip_ok(global_clipnorm)) return M1_ERR_BAD_ARG;
    if ((((uintptr_t)g | (uintptr_t)p | (uintptr_t)ctl) & 15) || ((uintptr_t)ws & 7) || ws_bytes < m1_grad_norm_ws(n)) return M1_ERR_BAD_ARG;
    if (m1_debug_skip("grad_norm")) return M1_OK;
    const int blocks = grad_norm_blocks(n, M1_CFG("M1_EW_BLOCKS", 2048));
    const bool l2 = l2_kernel != 0.f || l2_bias != 0.f;
    const float cv = clipvalue > 0.f ? clipvalue : __builtin_inff();
    hipStream_t s = (hipStream_t)stream;
    {
        M1ProfScope ps("grad_norm", 2.0 * n, (l2 ? 8.0 : 4.0) * n + 8.0 * blocks, s);
        if (l2)
            hipLaunchKernelGGL(grad_norm_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, s, g, p, n, n_kernel, n_bias, l2_kernel,
                               l2_bias, grad_scale, cv, (double*)ws);
        else
            hipLaunchKernelGGL(grad_norm_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, s, g, p, n, n_kernel, n_bias, l2_kernel,
                               l2_bias, grad_scale, cv, (double*)ws);
    }
    {
        M1ProfScope ps("grad_control", 0.0, 8.0 * blocks + 20.0, s);
        hipLaunchKernelGGL(grad_control_kernel, dim3(1), dim3(256), 0, s, (const double*)ws, blocks, global_clipnorm,
                           skip_nonfinite ? 1 : 0, (int*)ctl);
    }
    return m1_check_launch();
}

extern "C" int m1_adam_amsgrad_ctl(float* p, const float* g, float* m, float* v, float* vhat, long long n, long long n_kernel,
                                   long long n_bias, float l2_kernel, float l2_bias, float grad_scale, const float* lr_dev,
                                   float beta1, float beta2, float eps, const int* step_dev, float clipvalue,
                                   const m1_step_ctl_t* ctl, void* stream) {
    if (!adam_args_ok(p, g, m, v, vhat, lr_dev, step_dev, n) || !ctl || ((uintptr_t)ctl & 15) || !clip_ok(clipvalue))
        return M1_ERR_BAD_ARG;
    if (m1_debug_skip("adam")) return M1_OK;
    M1ProfScope ps("adam_amsgrad_ctl", 0.0, 36.0 * n + 8.0, (hipStream_t)stream);
    hipLaunchKernelGGL(adam_amsgrad_kernel<true>, dim3((unsigned)adam_blocks(n)), dim3(256), 0, (hipStream_t)stream, p, g, m, v, vhat,
                       n, n_kernel, n_bias, l2_kernel, l2_bias, grad_scale, lr_dev, beta1, beta2, eps, step_dev,
                       clipvalue > 0.f ? clipvalue : __builtin_inff(), (const float*)ctl);
    return m1_check_launch();
}

// advances the optimizer step counter and the dropout/sampling stream counter (rng[1]) by one
extern "C" int m1_step_advance(int* step_dev, uint64_t* rng_dev, void* stream) {
    hipLaunchKernelGGL(step_inc_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, step_dev, (unsigned long long*)rng_dev);
    return m1_check_launch();
}

// step_dev[0] += ctl->apply: a skipped step leaves Adam's t where it was
extern "C" int m1_step_advance_ctl(int* step_dev, const m1_step_ctl_t* ctl, void* stream) {
    if (!step_dev || !ctl) return M1_ERR_BAD_ARG;
    hipLaunchKernelGGL(step_inc_ctl_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, step_dev, (const int*)ctl);
    return m1_check_launch();
}
