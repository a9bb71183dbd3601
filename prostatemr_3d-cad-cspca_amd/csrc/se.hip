// se.hip -- squeeze-excitation gate and the multiplicative-residual combine of SEResNetBottleNeck
// (network_blocks.py:68-78), forward and backward, with the block's dropout
// (networks.py:579-582,597,607,616,624; network_blocks.py:142-143) fused into the epilogue.
//
//   x_  = IN3(y3)            rho = IN4(y4)            g = sigmoid(W7 . lrelu(W6 . GAP(x_) + b6) + b7)
//   out = dropout( lrelu( x_ * g * rho ) )
// GAP(IN3(.)) over D,H,W equals beta3 exactly, so g depends on parameters only.
#include "common.h"
#include "reduce.h"
#include <stdlib.h>

#define SE_MAX_F 1024
#define SE_MAX_FR 256

// ---------------- gate (one block; every dot product is split over the block and folded through LDS) ----------------
// out[j] = sum_c v[c] * W[c*ldw + j]   for j < J, c < Cn  (W row-major [Cn][J]); 256 threads = (256/JP) c-slices x JP columns
__device__ __forceinline__ void block_matvec_cols(const float* __restrict__ v, const float* __restrict__ W, int Cn, int J,
                                                  float* __restrict__ red /*[256]*/, float* __restrict__ out_s /*[J]*/) {
    for (int j0 = 0; j0 < J; j0 += 256) {
        const int jn = J - j0 < 256 ? J - j0 : 256;
        int JP = 1; while (JP < jn) JP <<= 1;
        const int parts = 256 / JP, jl = threadIdx.x % JP, part = threadIdx.x / JP;
        float s = 0.f;
        if (jl < jn) {          // independent loads: keep 8 in flight (the single block is latency-bound otherwise)
#pragma unroll 8
            for (int c = part; c < Cn; c += parts) s = fmaf(v[c], W[(size_t)c * J + j0 + jl], s);
        }
        red[threadIdx.x] = s;
        __syncthreads();
        if (part == 0 && jl < jn) {
            float t = 0.f;
            for (int q = 0; q < parts; ++q) t += red[q * JP + jl];
            out_s[j0 + jl] = t;
        }
        __syncthreads();
    }
}

__device__ __forceinline__ void se_gate_fwd_body(const float* __restrict__ beta3, const float* __restrict__ W6,
                                                 const float* __restrict__ b6, const float* __restrict__ W7,
                                                 const float* __restrict__ b7, int F, int Fr,
                                                 float* __restrict__ hidden, float* __restrict__ g) {
    __shared__ float red[256];
    __shared__ float v_s[SE_MAX_F];
    __shared__ float o_s[SE_MAX_F];
    __shared__ float h_s[SE_MAX_FR];
    for (int c = threadIdx.x; c < F; c += 256) v_s[c] = beta3[c];
    __syncthreads();
    block_matvec_cols(v_s, W6, F, Fr, red, o_s);                 // hidden = W6^T beta3
    for (int j = threadIdx.x; j < Fr; j += 256) {
        const float s = o_s[j] + b6[j];
        hidden[j] = s; h_s[j] = lrelu_f(s, 0.1f);
    }
    __syncthreads();
    block_matvec_cols(h_s, W7, Fr, F, red, o_s);                 // gpre = W7^T h
    for (int c = threadIdx.x; c < F; c += 256) g[c] = 1.f / (1.f + expf(-(o_s[c] + b7[c])));
}
__global__ void __launch_bounds__(256) se_gate_fwd_kernel(const float* __restrict__ beta3, const float* __restrict__ W6,
                                                          const float* __restrict__ b6, const float* __restrict__ W7,
                                                          const float* __restrict__ b7, int F, int Fr,
                                                          float* __restrict__ hidden, float* __restrict__ g) {
    se_gate_fwd_body(beta3, W6, b6, W7, b7, F, Fr, hidden, g);
}
// one block per SE block of a core pass: the gates are functions of the parameters only, so a caller can evaluate all of
// them up front in one launch (m1_se_gate_fwd_batch)
struct SeGateFwdBatch { m1_se_gate_fwd_job_t job[M1_SE_GATE_BATCH]; };
__global__ void __launch_bounds__(256) se_gate_fwd_batch_kernel(SeGateFwdBatch b) {
    const m1_se_gate_fwd_job_t& j = b.job[blockIdx.x];
    se_gate_fwd_body(j.beta3, j.W6, j.b6, j.W7, j.b7, j.F, j.Fr, j.hidden, j.g);
}

// out[r] = sum_j W[r*J + j] * v[j]  for r < R (rows contiguous): one wave per row, lanes along j
__device__ __forceinline__ void block_matvec_rows(const float* __restrict__ W, const float* __restrict__ v, int R, int J,
                                                  float* __restrict__ out_s) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int r = wave; r < R; r += 4) {
        float s = 0.f;
#pragma unroll 8
        for (int j = lane; j < J; j += 64) s = fmaf(W[(size_t)r * J + j], v[j], s);
        s = wave_sum(s);
        if (lane == 0) out_s[r] = s;
    }
    __syncthreads();
}

// backward, phase A (one block): dgpre = dg*g*(1-g) -> db7; dhid = (W7 dgpre) * lrelu'(hidden) -> db6.
// dgpre overwrites dg (scratch), dhid goes to dg[F .. F+Fr) -- the caller sizes dg as F + Fr floats.
__device__ __forceinline__ void se_gate_bwd_a_body(const float* __restrict__ W7, const float* __restrict__ hidden,
                                                            const float* __restrict__ g, float* __restrict__ dg, int F, int Fr,
                                                            float* __restrict__ db6, float* __restrict__ db7, int acc) {
    __shared__ float dgp_s[SE_MAX_F];
    __shared__ float o_s[SE_MAX_FR];
    for (int c = threadIdx.x; c < F; c += 256) {
        const float t = dg[c] * g[c] * (1.f - g[c]);
        dgp_s[c] = t; db7[c] = (acc ? db7[c] : 0.f) + t;
    }
    __syncthreads();
    block_matvec_rows(W7, dgp_s, Fr, F, o_s);                     // dh[j] = sum_c W7[j][c] dgpre[c]
    for (int c = threadIdx.x; c < F; c += 256) dg[c] = dgp_s[c];
    for (int j = threadIdx.x; j < Fr; j += 256) {
        const float dhid = o_s[j] * lrelu_g(hidden[j], 0.1f);
        dg[F + j] = dhid; db6[j] = (acc ? db6[j] : 0.f) + dhid;
    }
}
__global__ void __launch_bounds__(256) se_gate_bwd_a_kernel(const float* __restrict__ W7, const float* __restrict__ hidden,
                                                            const float* __restrict__ g, float* __restrict__ dg, int F, int Fr,
                                                            float* __restrict__ db6, float* __restrict__ db7, int acc) {
    se_gate_bwd_a_body(W7, hidden, g, dg, F, Fr, db6, db7, acc);
}
// phase B (F*Fr threads): the two outer products and dbeta3 += W6 dhid
__device__ __forceinline__ void se_gate_bwd_b_body(int i, const float* __restrict__ beta3, const float* __restrict__ W6,
                                                   const float* __restrict__ hidden, const float* __restrict__ dg,
                                                   int F, int Fr, float* __restrict__ dbeta3_add,
                                                   float* __restrict__ dW6, float* __restrict__ dW7, int acc) {
    if (i >= F * Fr) return;
    {   // dW7[j][c] = h[j] * dgpre[c]
        const int j = i / F, c = i % F;
        dW7[i] = (acc ? dW7[i] : 0.f) + lrelu_f(hidden[j], 0.1f) * dg[c];
    }
    {   // dW6[c][j] = beta3[c] * dhid[j]
        const int c = i / Fr, j = i % Fr;
        dW6[i] = (acc ? dW6[i] : 0.f) + beta3[c] * dg[F + j];
    }
    if (i < F) {
        float s = 0.f;
        for (int j = 0; j < Fr; ++j) s = fmaf(W6[(size_t)i * Fr + j], dg[F + j], s);
        dbeta3_add[i] += s;
    }
}

__global__ void __launch_bounds__(256) se_gate_bwd_b_kernel(const float* __restrict__ beta3, const float* __restrict__ W6,
                                                            const float* __restrict__ hidden, const float* __restrict__ dg,
                                                            int F, int Fr, float* __restrict__ dbeta3_add,
                                                            float* __restrict__ dW6, float* __restrict__ dW7, int acc) {
    se_gate_bwd_b_body(blockIdx.x * 256 + threadIdx.x, beta3, W6, hidden, dg, F, Fr, dbeta3_add, dW6, dW7, acc);
}
// batched variants: blockIdx.y = job (the gate backward produces parameter gradients only, so the caller may collect the
// jobs of a whole backward pass and run them with two launches instead of two per SE block).  Jobs that accumulate into
// the same destination (one SE block used by several passes of the cores) form a chain that ONE block column walks in
// order: no two blocks read-modify-write the same gradient, and the sum order is fixed.
struct SeGateBatch { m1_se_gate_job_t job[M1_SE_GATE_BATCH]; signed char next[M1_SE_GATE_BATCH]; unsigned char head[M1_SE_GATE_BATCH]; };
__global__ void __launch_bounds__(256) se_gate_bwd_a_batch_kernel(SeGateBatch b) {
    if (!b.head[blockIdx.y]) return;
    for (int q = blockIdx.y; q >= 0; q = b.next[q]) {
        const m1_se_gate_job_t& j = b.job[q];
        se_gate_bwd_a_body(j.W7, j.hidden, j.g, j.dg, j.F, j.Fr, j.db6, j.db7, j.accumulate);
        __syncthreads();
    }
}
__global__ void __launch_bounds__(256) se_gate_bwd_b_batch_kernel(SeGateBatch b) {
    if (!b.head[blockIdx.y]) return;
    for (int q = blockIdx.y; q >= 0; q = b.next[q]) {
        const m1_se_gate_job_t& j = b.job[q];
        se_gate_bwd_b_body(blockIdx.x * 256 + threadIdx.x, j.beta3, j.W6, j.hidden, j.dg, j.F, j.Fr, j.dbeta3_add, j.dW6, j.dW7, j.accumulate);
    }
}
extern "C" int m1_se_gate_bwd_batch(const m1_se_gate_job_t* jobs, int njobs, void* stream) {
    if (njobs < 0 || (njobs > 0 && !jobs)) return M1_ERR_BAD_ARG;
    for (int j0 = 0; j0 < njobs; j0 += M1_SE_GATE_BATCH) {
        SeGateBatch b{}; int n = njobs - j0 < M1_SE_GATE_BATCH ? njobs - j0 : M1_SE_GATE_BATCH, maxffr = 0;
        for (int q = 0; q < n; ++q) {
            const m1_se_gate_job_t& j = jobs[j0 + q];
            if (!j.beta3 || !j.W6 || !j.W7 || !j.hidden || !j.g || !j.dg || !j.dbeta3_add || !j.dW6 || !j.db6 || !j.dW7 || !j.db7) return M1_ERR_BAD_ARG;
            if (j.F <= 0 || j.Fr <= 0 || j.F > SE_MAX_F || j.Fr > SE_MAX_FR) return M1_ERR_UNSUPPORTED;
            b.job[q] = j; b.next[q] = -1; b.head[q] = 1;
            if (j.F * j.Fr > maxffr) maxffr = j.F * j.Fr;
            for (int r = q - 1; r >= 0; --r) {           // same destination as an earlier job: append to its chain
                const m1_se_gate_job_t& e = b.job[r];
                if (e.dW6 == j.dW6 || e.dW7 == j.dW7 || e.db6 == j.db6 || e.db7 == j.db7 || e.dbeta3_add == j.dbeta3_add) {
                    if (e.F != j.F || e.Fr != j.Fr || !j.accumulate) return M1_ERR_BAD_ARG;
                    b.next[r] = (signed char)q; b.head[q] = 0; break;
                }
            }
        }
        hipLaunchKernelGGL(se_gate_bwd_a_batch_kernel, dim3(1, n), dim3(256), 0, (hipStream_t)stream, b);
        hipLaunchKernelGGL(se_gate_bwd_b_batch_kernel, dim3((maxffr + 255) / 256, n), dim3(256), 0, (hipStream_t)stream, b);
    }
    return m1_check_launch();
}

extern "C" int m1_se_gate_fwd(const float* beta3, const float* W6, const float* b6, const float* W7, const float* b7,
                              int F, int Fr, float* hidden, float* g, void* stream) {
    if (!beta3 || !W6 || !b6 || !W7 || !b7 || !hidden || !g || F <= 0 || Fr <= 0) return M1_ERR_BAD_ARG;
    if (F > SE_MAX_F || Fr > SE_MAX_FR) return M1_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(se_gate_fwd_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, beta3, W6, b6, W7, b7, F, Fr, hidden, g);
    return m1_check_launch();
}
extern "C" int m1_se_gate_fwd_batch(const m1_se_gate_fwd_job_t* jobs, int njobs, void* stream) {
    if (njobs < 0 || (njobs > 0 && !jobs)) return M1_ERR_BAD_ARG;
    for (int j0 = 0; j0 < njobs; j0 += M1_SE_GATE_BATCH) {
        SeGateFwdBatch b{}; const int n = njobs - j0 < M1_SE_GATE_BATCH ? njobs - j0 : M1_SE_GATE_BATCH;
        for (int q = 0; q < n; ++q) {
            const m1_se_gate_fwd_job_t& j = jobs[j0 + q];
            if (!j.beta3 || !j.W6 || !j.b6 || !j.W7 || !j.b7 || !j.hidden || !j.g || j.F <= 0 || j.Fr <= 0) return M1_ERR_BAD_ARG;
            if (j.F > SE_MAX_F || j.Fr > SE_MAX_FR) return M1_ERR_UNSUPPORTED;
            b.job[q] = j;
        }
        hipLaunchKernelGGL(se_gate_fwd_batch_kernel, dim3(n), dim3(256), 0, (hipStream_t)stream, b);
    }
    return m1_check_launch();
}
extern "C" int m1_se_gate_bwd(const float* beta3, const float* W6, const float* W7, const float* hidden, const float* g,
                              const float* dg, int F, int Fr, float* dbeta3_add, float* dW6, float* db6, float* dW7,
                              float* db7, int accumulate, void* stream) {
    if (!beta3 || !W6 || !W7 || !hidden || !g || !dg || !dbeta3_add || !dW6 || !db6 || !dW7 || !db7) return M1_ERR_BAD_ARG;
    if (F > SE_MAX_F || Fr > SE_MAX_FR) return M1_ERR_UNSUPPORTED;
    float* dgw = const_cast<float*>(dg);   // dg is scratch of F + Fr floats (see include/m1hip.h)
    hipLaunchKernelGGL(se_gate_bwd_a_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, W7, hidden, g, dgw, F, Fr, db6, db7, accumulate);
    hipLaunchKernelGGL(se_gate_bwd_b_kernel, dim3((F * Fr + 255) / 256), dim3(256), 0, (hipStream_t)stream, beta3, W6, hidden, dgw,
                       F, Fr, dbeta3_add, dW6, dW7, accumulate);
    return m1_check_launch();
}

// ---------------- combine forward ----------------
struct SeParams {
    const float *stats3, *stats4, *gamma3, *beta3, *gamma4, *beta4, *g;
    long long V; int F;
    float drop_rate; const uint64_t* rng; uint64_t layer_id;
    unsigned char* mask;      // optional keep-mask, bit (idx & 7) of byte (idx >> 3): written by the forward, read by the backward
    int identity4;            // network_blocks.py:63 false branch (C_in == filters): rho is the block input itself, no conv4 / norm4
    int dupB;                 // > 0: y3 / y4 / statistics hold dupB samples, out / dout / mask 2 * dupB -- the two stacked passes of a core
                              // share everything in front of their first dropout draw (M1Net.forward: posterior([x; x]), prior([img; img])),
                              // sample n of the output reads sample n % dupB of the inputs; the backward sums the two halves' gradients
};
// per-channel constants of the second factor: {mean, rstd, gamma, beta} of norm4, or {0, 1, 1, 0} for the identity residual --
// (y4 - 0) * 1 * 1 + 0 is y4 exactly, and the InstanceNorm backward with zero sums and unit scale is the identity
// (ID4 is a template parameter of every kernel: a run-time test of p.identity4 inside the per-element functor cost the ordinary path
//  2-3x -- 0.54 -> 1.60 ms forward, 1.6 -> 3.3 ms backward per C3 step -- measured before this was made compile-time)
template <bool ID4>
__device__ __forceinline__ void se_rho_consts(const SeParams& p, size_t sc, int c, float& m4, float& r4, float& g4, float& b4) {
    if constexpr (ID4) { m4 = 0.f; r4 = 1.f; g4 = 1.f; b4 = 0.f; }
    else { m4 = p.stats4[sc]; r4 = p.stats4[sc + 1]; g4 = p.gamma4[c]; b4 = p.beta4[c]; }
}

__device__ __forceinline__ void se_rng(const SeParams& p, uint64_t& seed, uint64_t& base) {
    seed = 0; base = 0;
    if (p.drop_rate > 0.f) { seed = p.rng[0] + p.layer_id * 0x9E3779B97F4A7C15ull; base = p.rng[1] << 36; }
}

template <typename T, int VEC, bool ID4 = false>
__global__ void __launch_bounds__(256, 3) se_combine_fwd_kernel(const T* __restrict__ y3, const T* __restrict__ y4, SeParams p,
                                                             T* __restrict__ out) {
    const int n_out = blockIdx.y, n = p.dupB ? n_out % p.dupB : n_out, F = p.F, cg = F / VEC;
    const long long per = p.V * cg;
    const size_t base_in = (size_t)n * p.V * F, base = (size_t)n_out * p.V * F;          // (base: output / dropout-stream / mask index)
    uint64_t seed, rbase; se_rng(p, seed, rbase);
    const float keep_scale = p.drop_rate > 0.f ? 1.f / (1.f - p.drop_rate) : 1.f;
    // the launch keeps gridDim.x*blockDim.x a multiple of the channel groups (m1_grid_for_n): a thread's channels never change and
    // their 9 parameters live in registers (re-loaded per vector they were 72 dword loads beside 2 data loads: TA bound)
    const long long i0 = (long long)blockIdx.x * blockDim.x + threadIdx.x, stride = (long long)gridDim.x * blockDim.x;
    const int c0 = (int)(i0 % cg) * VEC;
    float m3[VEC], r3[VEC], g3[VEC], b3[VEC], m4[VEC], r4[VEC], g4[VEC], b4[VEC], gt[VEC];
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
        const int c = c0 + k; const size_t sc = ((size_t)n * F + c) * 2;
        m3[k] = p.stats3[sc]; r3[k] = p.stats3[sc + 1]; g3[k] = p.gamma3[c]; b3[k] = p.beta3[c];
        se_rho_consts<ID4>(p, sc, c, m4[k], r4[k], g4[k], b4[k]); gt[k] = p.g[c];
    }
    auto body = [&](long long i, float* a, const float* b) {
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
            const float x_ = (a[k] - m3[k]) * r3[k] * g3[k] + b3[k];
            const float rho = (b[k] - m4[k]) * r4[k] * g4[k] + b4[k];
            a[k] = lrelu_f(x_ * gt[k] * rho, 0.1f);
        }
        if (p.drop_rate > 0.f) {
            bool keep[VEC];
            philox_keep_vec<VEC, VEC % 4 == 0>(seed, rbase, base + i * VEC, p.drop_rate, keep);
#pragma unroll
            for (int k = 0; k < VEC; ++k) a[k] = keep[k] ? a[k] * keep_scale : 0.f;
            if (VEC == 8 && p.mask) {                     // one byte per lane: the backward reads it instead of re-running Philox
                unsigned m = 0;
#pragma unroll
                for (int k = 0; k < VEC; ++k) m |= (keep[k] ? 1u : 0u) << k;
                p.mask[(base + i * VEC) >> 3] = (unsigned char)m;
            }
        }
        VecIO<T, VEC>::st(out + base + i * VEC, a);
    };
    long long i = i0;
    for (; i + stride < per; i += 2 * stride) {          // two vectors per tensor in flight per thread
        float a0[VEC], b0[VEC], a1[VEC], b1[VEC];
        VecIO<T, VEC>::ld(y3 + base_in + i * VEC, a0); VecIO<T, VEC>::ld(y4 + base_in + i * VEC, b0);
        VecIO<T, VEC>::ld(y3 + base_in + (i + stride) * VEC, a1); VecIO<T, VEC>::ld(y4 + base_in + (i + stride) * VEC, b1);
        body(i, a0, b0); body(i + stride, a1, b1);
    }
    for (; i < per; i += stride) {
        float a0[VEC], b0[VEC];
        VecIO<T, VEC>::ld(y3 + base_in + i * VEC, a0); VecIO<T, VEC>::ld(y4 + base_in + i * VEC, b0);
        body(i, a0, b0);
    }
}

// ---------------- combine backward ----------------
// DUP (SeParams::dupB): d(out) holds two halves of dupB samples over the SAME (y3, y4): lrelu'(u) is common, the incoming gradients
// (each behind its own dropout draw) add up before everything else
template <typename T, bool MASKED = false, bool ID4 = false, bool DUP = false>
struct SeBwdF {
    const T* y3; const T* y4; const T* dout; SeParams p;
    __device__ void operator()(int n, long long v, int c, float* acc) const {
        const int F = p.F;
        const size_t idx = ((size_t)n * p.V + v) * F + c; const size_t sc = ((size_t)n * F + c) * 2;
        float m4, r4, g4, b4; se_rho_consts<ID4>(p, sc, c, m4, r4, g4, b4);
        const float xh3 = (Act<T>::ld(y3 + idx) - p.stats3[sc]) * p.stats3[sc + 1];
        const float xh4 = (Act<T>::ld(y4 + idx) - m4) * r4;
        const float x_ = xh3 * p.gamma3[c] + p.beta3[c], rho = xh4 * g4 + b4;
        const float g = p.g[c], u = x_ * g * rho;
        float d = Act<T>::ld(dout + idx);
        if (p.drop_rate > 0.f) {
            uint64_t seed, rbase; se_rng(p, seed, rbase);
            d = philox_keep(seed, rbase, idx, p.drop_rate) ? d / (1.f - p.drop_rate) : 0.f;
        }
        if constexpr (DUP) {
            const size_t idx2 = idx + (size_t)p.dupB * p.V * F;
            float d2 = Act<T>::ld(dout + idx2);
            if (p.drop_rate > 0.f) {
                uint64_t seed, rbase; se_rng(p, seed, rbase);
                d2 = philox_keep(seed, rbase, idx2, p.drop_rate) ? d2 / (1.f - p.drop_rate) : 0.f;
            }
            d += d2;
        }
        const float du = d * lrelu_g(u, 0.1f);
        const float dx_ = du * g * rho, drho = du * g * x_;
        acc[0] += dx_; acc[1] += dx_ * xh3; acc[2] += drho; acc[3] += drho * xh4; acc[4] += du * x_ * rho;
    }
    static constexpr int kVec = sizeof(T) == 2 ? 8 : 4;
    static constexpr int kUnroll = MASKED ? 2 : 1;      // (the Philox form keeps one voxel in flight: its registers)
    __device__ void vec(int n, long long v, int c0, float (*acc)[kVec]) const {
        const int F = p.F;
        const size_t idx = ((size_t)n * p.V + v) * F + c0;
        float a[kVec], b[kVec], d[kVec];
        VecIO<T, kVec>::ld(y3 + idx, a); VecIO<T, kVec>::ld(y4 + idx, b); VecIO<T, kVec>::ld(dout + idx, d);
        bool keep[kVec];
        if (MASKED) {
            const unsigned m = p.mask[idx >> 3];
#pragma unroll
            for (int e = 0; e < kVec; ++e) keep[e] = (m >> e) & 1u;
        } else if (p.drop_rate > 0.f) { uint64_t seed, rbase; se_rng(p, seed, rbase); philox_keep_vec<kVec, kVec % 4 == 0>(seed, rbase, idx, p.drop_rate, keep); }
        const float keep_scale = p.drop_rate > 0.f ? 1.f / (1.f - p.drop_rate) : 1.f;
        if (p.drop_rate > 0.f) {
#pragma unroll
            for (int e = 0; e < kVec; ++e) d[e] = keep[e] ? d[e] * keep_scale : 0.f;
        }
        if constexpr (DUP) {
            const size_t idx2 = idx + (size_t)p.dupB * p.V * F;
            float d2[kVec];
            VecIO<T, kVec>::ld(dout + idx2, d2);
            if (MASKED) {
                const unsigned m = p.mask[idx2 >> 3];
#pragma unroll
                for (int e = 0; e < kVec; ++e) keep[e] = (m >> e) & 1u;
            } else if (p.drop_rate > 0.f) { uint64_t seed, rbase; se_rng(p, seed, rbase); philox_keep_vec<kVec, kVec % 4 == 0>(seed, rbase, idx2, p.drop_rate, keep); }
#pragma unroll
            for (int e = 0; e < kVec; ++e) d[e] += p.drop_rate > 0.f ? (keep[e] ? d2[e] * keep_scale : 0.f) : d2[e];
        }
#pragma unroll
        for (int e = 0; e < kVec; ++e) {
            const int c = c0 + e; const size_t sc = ((size_t)n * F + c) * 2;
            float m4, r4, g4, b4; se_rho_consts<ID4>(p, sc, c, m4, r4, g4, b4);
            const float xh3 = (a[e] - p.stats3[sc]) * p.stats3[sc + 1];
            const float xh4 = (b[e] - m4) * r4;
            const float x_ = xh3 * p.gamma3[c] + p.beta3[c], rho = xh4 * g4 + b4;
            const float g = p.g[c], u = x_ * g * rho;
            const float du = d[e] * lrelu_g(u, 0.1f);              // (d: behind the dropout, both halves summed under DUP)
            const float dx_ = du * g * rho, drho = du * g * x_;
            acc[0][e] += dx_; acc[1][e] += dx_ * xh3; acc[2][e] += drho; acc[3][e] += drho * xh4; acc[4][e] += du * x_ * rho;
        }
    }
};

template <typename T, int VEC, bool MASKED = false, int MINW = 2, bool ID4 = false, bool DUP = false>
__global__ void __launch_bounds__(256, MINW) se_combine_bwd_apply_kernel(const T* __restrict__ y3, const T* __restrict__ y4,
                                                                   const T* __restrict__ dout, SeParams p,
                                                                   const float* __restrict__ sums /*[N][F][5]*/,
                                                                   T* __restrict__ dy3, T* __restrict__ dy4) {
    const int n = blockIdx.y, F = p.F, cg = F / VEC;
    const long long per = p.V * cg;
    const size_t base = (size_t)n * p.V * F;
    const float invV = 1.f / (float)p.V;
    uint64_t seed, rbase; se_rng(p, seed, rbase);
    const float keep_scale = p.drop_rate > 0.f ? 1.f / (1.f - p.drop_rate) : 1.f;
    // channel-invariant threads (see se_combine_fwd_kernel): 13 per-channel values in registers instead of 26 loads per vector
    const long long i0 = (long long)blockIdx.x * blockDim.x + threadIdx.x, stride = (long long)gridDim.x * blockDim.x;
    const int c0 = (int)(i0 % cg) * VEC;
    float m3[VEC], r3[VEC], g3[VEC], b3[VEC], m4[VEC], r4[VEC], g4[VEC], b4[VEC], gt[VEC], s0[VEC], s1[VEC], s2[VEC], s3[VEC];
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
        const int c = c0 + k; const size_t sc = ((size_t)n * F + c) * 2;
        m3[k] = p.stats3[sc]; r3[k] = p.stats3[sc + 1]; g3[k] = p.gamma3[c]; b3[k] = p.beta3[c];
        se_rho_consts<ID4>(p, sc, c, m4[k], r4[k], g4[k], b4[k]); gt[k] = p.g[c];
        const float* s = sums + ((size_t)n * F + c) * 5;
        s0[k] = s[0] * invV; s1[k] = s[1] * invV; s2[k] = s[2] * invV; s3[k] = s[3] * invV;
        if constexpr (ID4) { s2[k] = 0.f; s3[k] = 0.f; }          // d(residual) = d(rho): no mean terms (there is no norm4)
    }
    for (long long i = i0; i < per; i += stride) {
        float a[VEC], b[VEC], d[VEC];
        VecIO<T, VEC>::ld(y3 + base + i * VEC, a);
        VecIO<T, VEC>::ld(y4 + base + i * VEC, b);
        VecIO<T, VEC>::ld(dout + base + i * VEC, d);
        bool keep[VEC];
        if (MASKED) {
            const unsigned m = p.mask[(base + i * VEC) >> 3];
#pragma unroll
            for (int k = 0; k < VEC; ++k) keep[k] = (m >> k) & 1u;
        } else if (p.drop_rate > 0.f) philox_keep_vec<VEC, VEC % 4 == 0>(seed, rbase, base + i * VEC, p.drop_rate, keep);
        if (p.drop_rate > 0.f) {
#pragma unroll
            for (int k = 0; k < VEC; ++k) d[k] = keep[k] ? d[k] * keep_scale : 0.f;
        }
        if constexpr (DUP) {                     // the second half's gradient (its own dropout draw) over the same (y3, y4)
            const size_t o2 = base + (size_t)p.dupB * p.V * F + i * VEC;
            float d2[VEC];
            VecIO<T, VEC>::ld(dout + o2, d2);
            if (MASKED) {
                const unsigned m = p.mask[o2 >> 3];
#pragma unroll
                for (int k = 0; k < VEC; ++k) keep[k] = (m >> k) & 1u;
            } else if (p.drop_rate > 0.f) philox_keep_vec<VEC, VEC % 4 == 0>(seed, rbase, o2, p.drop_rate, keep);
#pragma unroll
            for (int k = 0; k < VEC; ++k) d[k] += p.drop_rate > 0.f ? (keep[k] ? d2[k] * keep_scale : 0.f) : d2[k];
        }
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
            const float xh3 = (a[k] - m3[k]) * r3[k], xh4 = (b[k] - m4[k]) * r4[k];
            const float x_ = xh3 * g3[k] + b3[k], rho = xh4 * g4[k] + b4[k];
            const float g = gt[k], u = x_ * g * rho;
            const float du = d[k] * lrelu_g(u, 0.1f);
            const float dx_ = du * g * rho, drho = du * g * x_;
            a[k] = g3[k] * r3[k] * (dx_ - s0[k] - xh3 * s1[k]);
            b[k] = g4[k] * r4[k] * (drho - s2[k] - xh4 * s3[k]);
        }
        VecIO<T, VEC>::st(dy3 + base + i * VEC, a);
        VecIO<T, VEC>::st(dy4 + base + i * VEC, b);
    }
}


template <typename T>
static int se_fwd_impl(const void* y3, const void* y4, const SeParams& p, void* out, int N_in, hipStream_t st) {
    constexpr int VW = sizeof(T) == 2 ? 8 : 4;
    const int N = p.dupB ? 2 * N_in : N_in;              // blocks walk the OUTPUT samples (SeParams::dupB: two per input sample)
    if (p.identity4) {                                   // network_blocks.py:63 false branch: its own instantiations (compile-time constants)
        if (p.F % VW == 0)
            hipLaunchKernelGGL((se_combine_fwd_kernel<T, VW, true>), dim3(m1_grid_for_n(p.V * (p.F / VW), p.F / VW, N), N), dim3(256), 0, st, (const T*)y3,
                               (const T*)y4, p, (T*)out);
        else
            hipLaunchKernelGGL((se_combine_fwd_kernel<T, 1, true>), dim3(m1_grid_for_n(p.V * p.F, p.F, N), N), dim3(256), 0, st, (const T*)y3,
                               (const T*)y4, p, (T*)out);
        return m1_check_launch();
    }
    if (p.F % VW == 0)
        hipLaunchKernelGGL((se_combine_fwd_kernel<T, VW>), dim3(m1_grid_for_n(p.V * (p.F / VW), p.F / VW, N), N), dim3(256), 0, st, (const T*)y3,
                           (const T*)y4, p, (T*)out);
    else
        hipLaunchKernelGGL((se_combine_fwd_kernel<T, 1>), dim3(m1_grid_for_n(p.V * p.F, p.F, N), N), dim3(256), 0, st, (const T*)y3,
                           (const T*)y4, p, (T*)out);
    return m1_check_launch();
}

template <typename T>
static int se_bwd_impl(const void* y3, const void* y4, const void* dout, const SeParams& p, void* dy3, void* dy4,
                       float* dgamma3, float* dbeta3, float* dgamma4, float* dbeta4, float* dg, int N, float* ws,
                       hipStream_t st, int acc) {
    constexpr int VW = sizeof(T) == 2 ? 8 : 4;
    const bool masked = VW == 8 && p.mask && p.drop_rate > 0.f && p.F % VW == 0;
    int rc;
    const int nchunks = m1_red_nchunks(p.V, p.F, N);
    float* sums = ws + (size_t)N * nchunks * p.F * 5;
    // parameter gradients ride on the fold: dg is scratch for the gate backward (always overwritten)
    M1ParamOut<5> po{{dbeta3, dgamma3, p.identity4 ? nullptr : dbeta4, p.identity4 ? nullptr : dgamma4, dg}, {acc, acc, acc, acc, 0}};
    if (p.identity4) {
        // the identity-residual block (a rare configuration): the plain variants, the keep bits read from the mask when there is one
        if (masked) { SeBwdF<T, true, true> f{(const T*)y3, (const T*)y4, (const T*)dout, p}; rc = m1_reduce_nc_launch<5>(f, N, p.V, p.F, ws, st); }
        else { SeBwdF<T, false, true> f{(const T*)y3, (const T*)y4, (const T*)dout, p}; rc = m1_reduce_nc_launch<5>(f, N, p.V, p.F, ws, st); }
        if (rc) return rc;
        rc = m1_reduce_finalize_params_launch<5>(ws, N, p.F, nchunks, sums, po, st); if (rc) return rc;
        if (masked)
            hipLaunchKernelGGL((se_combine_bwd_apply_kernel<T, VW, true, 2, true>), dim3(m1_grid_for_n(p.V * (p.F / VW), p.F / VW, N), N), dim3(256), 0, st,
                               (const T*)y3, (const T*)y4, (const T*)dout, p, sums, (T*)dy3, (T*)dy4);
        else if (p.F % VW == 0)
            hipLaunchKernelGGL((se_combine_bwd_apply_kernel<T, VW, false, 2, true>), dim3(m1_grid_for_n(p.V * (p.F / VW), p.F / VW, N), N), dim3(256), 0, st,
                               (const T*)y3, (const T*)y4, (const T*)dout, p, sums, (T*)dy3, (T*)dy4);
        else
            hipLaunchKernelGGL((se_combine_bwd_apply_kernel<T, 1, false, 2, true>), dim3(m1_grid_for_n(p.V * p.F, p.F, N), N), dim3(256), 0, st, (const T*)y3,
                               (const T*)y4, (const T*)dout, p, sums, (T*)dy3, (T*)dy4);
        return m1_check_launch();
    }
    if (p.dupB) {
        // two halves of d(out) over the same (y3, y4) (SeParams::dupB): sums and gradients of the N input samples, both halves added
        if (p.F % VW) return M1_ERR_UNSUPPORTED;
        if (masked) { SeBwdF<T, true, false, true> f{(const T*)y3, (const T*)y4, (const T*)dout, p}; rc = m1_reduce_nc_launch<5>(f, N, p.V, p.F, ws, st); }
        else { SeBwdF<T, false, false, true> f{(const T*)y3, (const T*)y4, (const T*)dout, p}; rc = m1_reduce_nc_launch<5>(f, N, p.V, p.F, ws, st); }
        if (rc) return rc;
        rc = m1_reduce_finalize_params_launch<5>(ws, N, p.F, nchunks, sums, po, st); if (rc) return rc;
        if (masked)
            hipLaunchKernelGGL((se_combine_bwd_apply_kernel<T, VW, true, 2, false, true>), dim3(m1_grid_for_n(p.V * (p.F / VW), p.F / VW, N), N), dim3(256), 0, st,
                               (const T*)y3, (const T*)y4, (const T*)dout, p, sums, (T*)dy3, (T*)dy4);
        else
            hipLaunchKernelGGL((se_combine_bwd_apply_kernel<T, VW, false, 2, false, true>), dim3(m1_grid_for_n(p.V * (p.F / VW), p.F / VW, N), N), dim3(256), 0, st,
                               (const T*)y3, (const T*)y4, (const T*)dout, p, sums, (T*)dy3, (T*)dy4);
        return m1_check_launch();
    }
    if (masked) { SeBwdF<T, true> f{(const T*)y3, (const T*)y4, (const T*)dout, p}; rc = m1_reduce_nc_launch<5>(f, N, p.V, p.F, ws, st); }
    else { SeBwdF<T> f{(const T*)y3, (const T*)y4, (const T*)dout, p}; rc = m1_reduce_nc_launch<5>(f, N, p.V, p.F, ws, st); }
    if (rc) return rc;
    rc = m1_reduce_finalize_params_launch<5>(ws, N, p.F, nchunks, sums, po, st); if (rc) return rc;
    // (the masked kernel takes 164 registers with or without a 3-wave launch bound: 3 waves per SIMD either way, no separate variant)
    if (masked)
        hipLaunchKernelGGL((se_combine_bwd_apply_kernel<T, VW, true>), dim3(m1_grid_for_n(p.V * (p.F / VW), p.F / VW, N), N), dim3(256), 0, st,
                           (const T*)y3, (const T*)y4, (const T*)dout, p, sums, (T*)dy3, (T*)dy4);
    else if (p.F % VW == 0)
        hipLaunchKernelGGL((se_combine_bwd_apply_kernel<T, VW>), dim3(m1_grid_for_n(p.V * (p.F / VW), p.F / VW, N), N), dim3(256), 0, st,
                           (const T*)y3, (const T*)y4, (const T*)dout, p, sums, (T*)dy3, (T*)dy4);
    else
        hipLaunchKernelGGL((se_combine_bwd_apply_kernel<T, 1>), dim3(m1_grid_for_n(p.V * p.F, p.F, N), N), dim3(256), 0, st, (const T*)y3,
                           (const T*)y4, (const T*)dout, p, sums, (T*)dy3, (T*)dy4);
    return m1_check_launch();
}

static int se_combine_fwd_entry(const void* y3, const void* y4, const float* stats3, const float* stats4,
                                const float* gamma3, const float* beta3, const float* gamma4, const float* beta4,
                                const float* g, void* out, int N, long long V, int F, int dtype, float drop_rate,
                                const uint64_t* rng, uint64_t layer_id, unsigned char* keep_mask, void* stream, int dup) {
    if (!y3 || !y4 || !stats3 || !gamma3 || !beta3 || !g || !out || N <= 0) return M1_ERR_BAD_ARG;
    const bool ident = !stats4 && !gamma4 && !beta4;             // all three NULL: identity residual (network_blocks.py:63, C_in == filters)
    if (!ident && (!stats4 || !gamma4 || !beta4)) return M1_ERR_BAD_ARG;
    if (drop_rate > 0.f && !rng) return M1_ERR_BAD_ARG;
    if (drop_rate < 0.f || drop_rate >= 1.f) return M1_ERR_BAD_ARG;
    if (keep_mask && (dtype != M1_BF16 || F % 8)) return M1_ERR_UNSUPPORTED;
    if (dup && ident) return M1_ERR_UNSUPPORTED;
    SeParams p{stats3, stats4, gamma3, beta3, gamma4, beta4, g, V, F, drop_rate, rng, layer_id, keep_mask, ident ? 1 : 0, dup ? N : 0};
    M1ProfScope ps("se_combine_fwd", 0.0, (dup ? 4.0 : 3.0) * N * V * F * (dtype == M1_BF16 ? 2 : 4), (hipStream_t)stream);
    return dtype == M1_BF16 ? se_fwd_impl<bf16_t>(y3, y4, p, out, N, (hipStream_t)stream)
                            : se_fwd_impl<float>(y3, y4, p, out, N, (hipStream_t)stream);
}
extern "C" int m1_se_combine_fwd(const void* y3, const void* y4, const float* stats3, const float* stats4,
                                 const float* gamma3, const float* beta3, const float* gamma4, const float* beta4,
                                 const float* g, void* out, int N, long long V, int F, int dtype, float drop_rate,
                                 const uint64_t* rng, uint64_t layer_id, unsigned char* keep_mask, void* stream) {
    if (m1_debug_skip("se_fwd")) return M1_OK;
    return se_combine_fwd_entry(y3, y4, stats3, stats4, gamma3, beta3, gamma4, beta4, g, out, N, V, F, dtype, drop_rate, rng, layer_id, keep_mask, stream, 0);
}
extern "C" int m1_se_combine_dup_fwd(const void* y3, const void* y4, const float* stats3, const float* stats4,
                                     const float* gamma3, const float* beta3, const float* gamma4, const float* beta4,
                                     const float* g, void* out, int N, long long V, int F, int dtype, float drop_rate,
                                     const uint64_t* rng, uint64_t layer_id, unsigned char* keep_mask, void* stream) {
    if (m1_debug_skip("se_fwd")) return M1_OK;
    return se_combine_fwd_entry(y3, y4, stats3, stats4, gamma3, beta3, gamma4, beta4, g, out, N, V, F, dtype, drop_rate, rng, layer_id, keep_mask, stream, 1);
}

static int se_combine_bwd_entry(const void* y3, const void* y4, const float* stats3, const float* stats4,
                                const float* gamma3, const float* beta3, const float* gamma4, const float* beta4,
                                const float* g, const void* dout, void* dy3, void* dy4, float* dgamma3, float* dbeta3,
                                float* dgamma4, float* dbeta4, float* dg, int N, long long V, int F, int dtype,
                                float drop_rate, const uint64_t* rng, uint64_t layer_id, const unsigned char* keep_mask,
                                float* ws, int accumulate, void* stream, int dup) {
    if (N <= 0 || !y3 || !y4 || !stats3 || !gamma3 || !beta3 || !g || !dout || !dy3 || !dy4 || !dgamma3 || !dbeta3 || !dg || !ws) return M1_ERR_BAD_ARG;
    const bool ident = !stats4 && !gamma4 && !beta4;             // identity residual: dy4 = d(out)/d(y4) directly, dgamma4 / dbeta4 unused
    if (!ident && (!stats4 || !gamma4 || !beta4 || !dgamma4 || !dbeta4)) return M1_ERR_BAD_ARG;
    if (drop_rate > 0.f && !rng && !keep_mask) return M1_ERR_BAD_ARG;
    if (keep_mask && (dtype != M1_BF16 || F % 8)) return M1_ERR_UNSUPPORTED;
    if (dup && ident) return M1_ERR_UNSUPPORTED;
    SeParams p{stats3, stats4, gamma3, beta3, gamma4, beta4, g, V, F, drop_rate, rng, layer_id, const_cast<unsigned char*>(keep_mask), ident ? 1 : 0, dup ? N : 0};
    M1ProfScope ps("se_combine_bwd", 0.0, (dup ? 10.0 : 8.0) * N * V * F * (dtype == M1_BF16 ? 2 : 4), (hipStream_t)stream);
    return dtype == M1_BF16
               ? se_bwd_impl<bf16_t>(y3, y4, dout, p, dy3, dy4, dgamma3, dbeta3, dgamma4, dbeta4, dg, N, ws, (hipStream_t)stream, accumulate)
               : se_bwd_impl<float>(y3, y4, dout, p, dy3, dy4, dgamma3, dbeta3, dgamma4, dbeta4, dg, N, ws, (hipStream_t)stream, accumulate);
}
extern "C" int m1_se_combine_bwd(const void* y3, const void* y4, const float* stats3, const float* stats4,
                                 const float* gamma3, const float* beta3, const float* gamma4, const float* beta4,
                                 const float* g, const void* dout, void* dy3, void* dy4, float* dgamma3, float* dbeta3,
                                 float* dgamma4, float* dbeta4, float* dg, int N, long long V, int F, int dtype,
                                 float drop_rate, const uint64_t* rng, uint64_t layer_id, const unsigned char* keep_mask,
                                 float* ws, int accumulate, void* stream) {
    if (m1_debug_skip("se_bwd")) return M1_OK;
    return se_combine_bwd_entry(y3, y4, stats3, stats4, gamma3, beta3, gamma4, beta4, g, dout, dy3, dy4, dgamma3, dbeta3, dgamma4, dbeta4, dg,
                                N, V, F, dtype, drop_rate, rng, layer_id, keep_mask, ws, accumulate, stream, 0);
}
extern "C" int m1_se_combine_dup_bwd(const void* y3, const void* y4, const float* stats3, const float* stats4,
                                     const float* gamma3, const float* beta3, const float* gamma4, const float* beta4,
                                     const float* g, const void* dout, void* dy3, void* dy4, float* dgamma3, float* dbeta3,
                                     float* dgamma4, float* dbeta4, float* dg, int N, long long V, int F, int dtype,
                                     float drop_rate, const uint64_t* rng, uint64_t layer_id, const unsigned char* keep_mask,
                                     float* ws, int accumulate, void* stream) {
    if (m1_debug_skip("se_bwd")) return M1_OK;
    return se_combine_bwd_entry(y3, y4, stats3, stats4, gamma3, beta3, gamma4, beta4, g, dout, dy3, dy4, dgamma3, dbeta3, dgamma4, dbeta4, dg,
                                N, V, F, dtype, drop_rate, rng, layer_id, keep_mask, ws, accumulate, stream, 1);
}
