// validate.hip -- per-case scoring of a validation batch in one streaming pass (validation.py: validate()).
//   p (B,V,K) fp32 softmax (or the mean of n draws), y (B,V,K) one-hot uint8 / fp32, entropy (B,V) fp32 or null, K <= 4
//   -> one m1_val_record_t (40 doubles) per case: the Focal.FL expression of that sample (losses.py:32-41), the entropy sums, and per
//      class the sums behind the reference's dice_3d (callbacks.py:36-40), the argmax counts behind the hard Dice and the largest p.
// Built as the norm pass of optim.hip is built:
//   val_score_kernel     grid (blocks, B): fp64 per-thread sums and integer counts, wave shuffles, the four wave results through LDS in
//                        a fixed order, one partial row of 40 doubles per (block, case) into the workspace -- no atomics
//   val_finish_kernel    one block per case folds the rows in a fixed order and writes the record (unused slots as zeros)
// The grid and the voxels a thread walks are a function of (B, V, K) alone: pointer alignment only chooses the width of the loads, so
// every bit of a record repeats from run to run and from buffer to buffer.
#include "common.h"

#define VAL_EPS 1e-7f
#define VAL_MAX_K 4
#define VAL_SLOTS 40                     // doubles per record and per partial row
#define VAL_HEAD 8                       // header doubles; class c starts at VAL_HEAD + 8 * c
#define VAL_FOLD 6                       // row lanes of the finish kernel: VAL_FOLD * VAL_SLOTS = 240 of its 256 threads work
// slots of the header / of a class
enum { VH_FOCAL = 0, VH_ENT = 1, VH_ENT_FG = 2, VH_NVOX = 3, VH_NFG = 4 };
enum { VC_SUM_P = 0, VC_SUM_Y = 1, VC_SUM_PY = 2, VC_NPRED = 3, VC_NTRUE = 4, VC_NBOTH = 5, VC_PMAX = 6 };

struct ValP {
    const float* p; const void* y; const float* ent; float alpha[VAL_MAX_K]; float gamma; long long V; int nb;
};

__device__ __forceinline__ float val_pow(float b, float e) { return e == 2.f ? b * b : (e == 1.f ? b : (e == 0.f ? 1.f : powf(b, e))); }
__device__ __forceinline__ bool val_used(int slot, int K) {
    if (slot < VAL_HEAD) return slot <= VH_NFG;
    return (slot - VAL_HEAD) / 8 < K && (slot & 7) <= VC_PMAX;
}

// N consecutive elements as floats; WIDE: one 8- or 16-byte load of fp32 (2 or 4 bytes of uint8) when N is 2 or 4
template <int N, bool WIDE> __device__ __forceinline__ void val_ld(const float* s, float* o) {
    if constexpr (WIDE && N == 4) { const float4 v = *reinterpret_cast<const float4*>(s); o[0] = v.x; o[1] = v.y; o[2] = v.z; o[3] = v.w; }
    else if constexpr (WIDE && N == 2) { const float2 v = *reinterpret_cast<const float2*>(s); o[0] = v.x; o[1] = v.y; }
    else {
#pragma unroll
        for (int i = 0; i < N; ++i) o[i] = s[i];
    }
}
template <int N, bool WIDE> __device__ __forceinline__ void val_ld(const unsigned char* s, float* o) {
    if constexpr (WIDE && N == 4) {
        const unsigned v = *reinterpret_cast<const unsigned*>(s);
        o[0] = (float)(v & 255u); o[1] = (float)((v >> 8) & 255u); o[2] = (float)((v >> 16) & 255u); o[3] = (float)(v >> 24);
    } else if constexpr (WIDE && N == 2) {
        const unsigned v = *reinterpret_cast<const unsigned short*>(s);
        o[0] = (float)(v & 255u); o[1] = (float)(v >> 8);
    } else {
#pragma unroll
        for (int i = 0; i < N; ++i) o[i] = (float)s[i];
    }
}

// VEC voxels per thread and iteration: 2 when K == 2 and V is even (a float4 of p), else 1.  Unit u of case n covers the voxels
// [u * VEC, u * VEC + VEC); block x of a case walks the units x * 256 + t, + nb * 256, ...
template <int K, int VEC, typename TY, bool WIDE, bool ENT>
__global__ void __launch_bounds__(256) val_score_kernel(ValP a, double* __restrict__ partial) {
    constexpr int NQ = 4 + 6 * K;                  // doubles folded by sum: focal, ent, ent_fg, n_fg, then 6 per class
    double focal = 0.0, ent = 0.0, ent_fg = 0.0;
    double sp[K], sy[K], spy[K];
    int n_fg = 0, npred[K], ntrue[K], nboth[K];
    float pmax[K];
#pragma unroll
    for (int c = 0; c < K; ++c) { sp[c] = sy[c] = spy[c] = 0.0; npred[c] = ntrue[c] = nboth[c] = 0; pmax[c] = 0.f; }
    const int n = blockIdx.y;
    const long long U = a.V / VEC, base = (long long)n * a.V;
    const float* __restrict__ pp = a.p + base * K;
    const TY* __restrict__ yp = reinterpret_cast<const TY*>(a.y) + base * K;
    const float* __restrict__ ep = ENT ? a.ent + base : nullptr;
    for (long long u = (long long)blockIdx.x * 256 + threadIdx.x; u < U; u += (long long)a.nb * 256) {
        float pv[VEC * K], yv[VEC * K], ev[VEC];
        val_ld<VEC * K, WIDE>(pp + u * (VEC * K), pv);
        val_ld<VEC * K, WIDE>(yp + u * (VEC * K), yv);
        if (ENT) val_ld<VEC, WIDE>(ep + u * VEC, ev);
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
            const float* p = pv + e * K;
            const float* y = yv + e * K;
            float s = 0.f;
#pragma unroll
            for (int c = 0; c < K; ++c) s += p[c];
            int am = 0, tc = 0;                    // argmax of p and of y, the lowest index among equals (np.argmax)
            float bp = p[0], by = y[0];
#pragma unroll
            for (int c = 1; c < K; ++c) {
                if (p[c] > bp) { bp = p[c]; am = c; }
                if (y[c] > by) { by = y[c]; tc = c; }
            }
            float fl = 0.f;                        // the fp32 evaluation of focal_fwd_kernel (head.hip), one head
#pragma unroll
            for (int c = 0; c < K; ++c) {
                if (y[c] != 0.f) {                 // (a zero label contributes +-0: skipped together with its log)
                    const float q = fminf(fmaxf(p[c] / s, VAL_EPS), 1.f - VAL_EPS);
                    fl += a.alpha[c] * ((y[c] * val_pow(1.f - q, a.gamma)) * (y[c] * -logf(q)));
                }
                sp[c] += (double)p[c];
                sy[c] += (double)y[c];
                spy[c] += (double)p[c] * (double)y[c];
                npred[c] += am == c;
                ntrue[c] += tc == c;
                nboth[c] += (am == c) & (tc == c);
                pmax[c] = fmaxf(pmax[c], p[c]);
            }
            focal += (double)fl;
            n_fg += tc >= 1;
            if (ENT) { ent += (double)ev[e]; if (tc >= 1) ent_fg += (double)ev[e]; }
        }
    }
    // wave shuffles, then the four wave results through LDS in a fixed order; the counts travel as doubles (exact below 2^53)
    __shared__ double red[4][VAL_SLOTS];
    double q[NQ];
    q[0] = focal; q[1] = ent; q[2] = ent_fg; q[3] = (double)n_fg;
#pragma unroll
    for (int c = 0; c < K; ++c) {
        q[4 + 6 * c + 0] = sp[c]; q[4 + 6 * c + 1] = sy[c]; q[4 + 6 * c + 2] = spy[c];
        q[4 + 6 * c + 3] = (double)npred[c]; q[4 + 6 * c + 4] = (double)ntrue[c]; q[4 + 6 * c + 5] = (double)nboth[c];
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {             // (the distance outside: the NQ exchanges of one distance are independent)
#pragma unroll
        for (int i = 0; i < NQ; ++i) q[i] += __shfl_xor(q[i], o, 64);
#pragma unroll
        for (int c = 0; c < K; ++c) pmax[c] = fmaxf(pmax[c], __shfl_xor(pmax[c], o, 64));
    }
    if ((threadIdx.x & 63) == 0) {
        double* r = red[threadIdx.x >> 6];
        r[VH_FOCAL] = q[0]; r[VH_ENT] = q[1]; r[VH_ENT_FG] = q[2]; r[VH_NVOX] = 0.0; r[VH_NFG] = q[3];
#pragma unroll
        for (int c = 0; c < K; ++c) {
#pragma unroll
            for (int j = 0; j < 6; ++j) r[VAL_HEAD + 8 * c + j] = q[4 + 6 * c + j];
            r[VAL_HEAD + 8 * c + VC_PMAX] = (double)pmax[c];
        }
    }
    __syncthreads();
    if (threadIdx.x < VAL_SLOTS) {
        const int j = threadIdx.x;
        double v = 0.0;
        if (val_used(j, K)) {
            if (j >= VAL_HEAD && (j & 7) == VC_PMAX) v = fmax(fmax(red[0][j], red[1][j]), fmax(red[2][j], red[3][j]));
            else v = (red[0][j] + red[1][j]) + (red[2][j] + red[3][j]);
        }
        partial[((size_t)n * a.nb + blockIdx.x) * VAL_SLOTS + j] = v;
    }
}

// one block per case: thread t < 240 owns slot t % 40 and adds the rows t / 40, t / 40 + 6, ... in that order; the six lane sums of a
// slot are folded in a fixed order by the slot's first thread, which writes the record's double
__global__ void __launch_bounds__(256) val_finish_kernel(const double* __restrict__ partial, int nb, int K, long long V,
                                                         double* __restrict__ rec) {
    __shared__ double red[VAL_FOLD][VAL_SLOTS];
    const int n = blockIdx.x, t = threadIdx.x, j = t % VAL_SLOTS, lane = t / VAL_SLOTS;
    const bool is_max = j >= VAL_HEAD && (j & 7) == VC_PMAX;
    if (lane < VAL_FOLD) {
        double v = 0.0;
        if (val_used(j, K)) {
            const double* src = partial + (size_t)n * nb * VAL_SLOTS + j;
            for (int r = lane; r < nb; r += VAL_FOLD) {
                const double x = src[(size_t)r * VAL_SLOTS];
                v = is_max ? fmax(v, x) : v + x;
            }
        }
        red[lane][j] = v;
    }
    __syncthreads();
    if (t < VAL_SLOTS) {
        double v;
        if (is_max) v = fmax(fmax(fmax(red[0][j], red[1][j]), fmax(red[2][j], red[3][j])), fmax(red[4][j], red[5][j]));
        else v = ((red[0][j] + red[1][j]) + (red[2][j] + red[3][j])) + (red[4][j] + red[5][j]);
        if (j == VH_NVOX) v = (double)V;
        rec[(size_t)n * VAL_SLOTS + j] = v;
    }
}

// blocks per case: about four units of VEC voxels per thread, at most 512 rows to fold -- a function of (V, K) alone
static inline int val_vec(long long V, int K) { return (K == 2 && (V & 1) == 0) ? 2 : 1; }
static inline int val_blocks(long long V, int K) {
    const long long b = cdiv_ll(V / val_vec(V, K), 1024);
    return (int)(b > 512 ? 512 : (b < 1 ? 1 : b));
}

extern "C" size_t m1_val_score_ws(int B, long long voxels, int K) {
    if (B <= 0 || voxels <= 0 || K <= 0 || K > VAL_MAX_K) return 0;
    return sizeof(double) * VAL_SLOTS * (size_t)B * (size_t)val_blocks(voxels, K);
}

template <int K, int VEC, typename TY, bool WIDE>
static void val_launch(const ValP& a, bool ent, int B, double* ws, hipStream_t s) {
    if (ent) hipLaunchKernelGGL((val_score_kernel<K, VEC, TY, WIDE, true>), dim3(a.nb, B), dim3(256), 0, s, a, ws);
    else hipLaunchKernelGGL((val_score_kernel<K, VEC, TY, WIDE, false>), dim3(a.nb, B), dim3(256), 0, s, a, ws);
}
template <int K, int VEC, typename TY>
static void val_launch_w(const ValP& a, bool ent, bool wide, int B, double* ws, hipStream_t s) {
    if constexpr (K * VEC == 2 || K * VEC == 4) {
        if (wide) { val_launch<K, VEC, TY, true>(a, ent, B, ws, s); return; }
    }
    val_launch<K, VEC, TY, false>(a, ent, B, ws, s);
}
template <typename TY>
static void val_launch_k(const ValP& a, int K, int vec, bool ent, bool wide, int B, double* ws, hipStream_t s) {
    if (K == 1) val_launch_w<1, 1, TY>(a, ent, wide, B, ws, s);
    else if (K == 2 && vec == 2) val_launch_w<2, 2, TY>(a, ent, wide, B, ws, s);
    else if (K == 2) val_launch_w<2, 1, TY>(a, ent, wide, B, ws, s);
    else if (K == 3) val_launch_w<3, 1, TY>(a, ent, wide, B, ws, s);
    else val_launch_w<4, 1, TY>(a, ent, wide, B, ws, s);
}

extern "C" int m1_val_score(const float* p, const void* y, int y_dtype, const float* entropy, const float* alpha, float gamma, int B,
                            long long voxels, int K, m1_val_record_t* records, void* ws, size_t ws_bytes, void* stream) {
    if (!p || !y || !alpha || !records || !ws || B <= 0 || voxels <= 0 || K <= 0) return M1_ERR_BAD_ARG;
    if (y_dtype != M1_VAL_Y_U8 && y_dtype != M1_VAL_Y_F32) return M1_ERR_BAD_ARG;
    if (((uintptr_t)p & 3) || ((uintptr_t)entropy & 3) || (y_dtype == M1_VAL_Y_F32 && ((uintptr_t)y & 3))) return M1_ERR_BAD_ARG;
    if (((uintptr_t)records | (uintptr_t)ws) & 7) return M1_ERR_BAD_ARG;
    if (K > VAL_MAX_K || B > 65535) return M1_ERR_UNSUPPORTED;
    if (ws_bytes < m1_val_score_ws(B, voxels, K)) return M1_ERR_WORKSPACE;
    if (m1_debug_skip("val_score")) return M1_OK;
    ValP a;
    a.p = p; a.y = y; a.ent = entropy; a.gamma = gamma; a.V = voxels; a.nb = val_blocks(voxels, K);
    for (int c = 0; c < VAL_MAX_K; ++c) a.alpha[c] = c < K ? alpha[c] : 0.f;
    const int vec = val_vec(voxels, K), n = K * vec;                     // elements of p and of y per unit
    const size_t ysz = y_dtype == M1_VAL_Y_U8 ? 1 : 4;
    // wide loads: a unit of p, of y and (two voxels per unit) of the entropy each start on a multiple of their own size.  A case
    // starts voxels * K elements after the one before it, a whole number of units
    const bool wide = (n == 2 || n == 4) && !((uintptr_t)p % (4 * n)) && !((uintptr_t)y % (ysz * n))
        && !(entropy && vec == 2 && ((uintptr_t)entropy & 7));
    hipStream_t s = (hipStream_t)stream;
    const double rows = (double)B * a.nb * VAL_SLOTS * 8.0;
    {
        M1ProfScope ps("val_score", 0.0, (double)B * voxels * (K * (4.0 + ysz) + (entropy ? 4.0 : 0.0)) + rows, s);
        if (y_dtype == M1_VAL_Y_U8) val_launch_k<unsigned char>(a, K, vec, entropy != nullptr, wide, B, (double*)ws, s);
        else val_launch_k<float>(a, K, vec, entropy != nullptr, wide, B, (double*)ws, s);
    }
    {
        M1ProfScope ps("val_finish", 0.0, rows + (double)B * VAL_SLOTS * 8.0, s);
        hipLaunchKernelGGL(val_finish_kernel, dim3(B), dim3(256), 0, s, (const double*)ws, a.nb, K, voxels, (double*)records);
    }
    return m1_check_launch();
}
