// calibrate.hip -- calibration record of a validation batch in one streaming pass (calibration.py: reliability()).
//   p (B,V,K) fp32 or bf16 softmax (or the mean of n draws), label (B,V) uint8 class indices, mask (B,V) uint8 or null,
//   unc (B,V) fp32 or null, M bins, 2 <= K <= 4, 1 <= M <= 64
//   -> one record of 8 + 3 * M * (K + 2) unsigned 64-bit integers per case (layout: include/m1hip.h): the counts and the 2^-32
//      fixed-point sums behind ECE / MCE, the one-vs-rest reliability of every class, the Brier score, the NLL and the
//      uncertainty / error histogram.
// Every accumulator is an integer, so no result depends on the order of the additions: the record equals the numpy restatement
// (calibration.reliability_host) bit for bit, except that the device's fp64 log may differ from numpy's in the last place.
//   cal_zero_kernel      zero-fills the records (a kernel, not a memset node: the call is capturable)
//   cal_score_kernel     grid (blocks, B).  A thread keeps one RUN per histogram in registers -- (bin, count, hits, sum) of the
//                        voxels it saw since the bin last changed -- and adds a run to the block's LDS histogram only when the
//                        bin changes: in a detection map almost every voxel is background at conf ~ 1, and without the runs every
//                        lane of every wave would queue on the same LDS word.  Alternating bins flush on every voxel: two 64-bit
//                        LDS adds per histogram (count and hits share a word).  At the end the block adds its non-zero slots to the
//                        record with 64-bit integer atomics.
// The grid and the voxels a thread walks are a function of (B, V, K, M) and M1_EW_BLOCKS alone; pointer alignment only chooses the
// width of the loads.
#include "common.h"

#define CAL_EPS 1e-7f
#define CAL_MIN_K 2
#define CAL_MAX_K 4
#define CAL_MAX_BINS 64
#define CAL_HEAD 8                       // header slots: n_valid, n_invalid, n_ignored, nll, brier[4]
#define CAL_MAX_VOXELS (1ll << 27)       // 16.2 * 2^27 * 2^32 < 2^64: no fixed-point sum of a case overflows
enum { CH_NVALID = 0, CH_NINVALID = 1, CH_NIGNORED = 2, CH_NLL = 3, CH_BRIER = 4 };
typedef unsigned long long u64;

struct CalP {
    const void* p; const unsigned char* label; const unsigned char* mask; const float* unc;
    float u_scale; long long V; int nb; int M;
};

// floor(v * 2^32) of a non-negative double (a negative one counts as 0)
__device__ __forceinline__ u64 cal_fx(double v) { return v > 0.0 ? (u64)(v * 4294967296.0) : 0ull; }
// min(M - 1, (int)prod) with the product clipped to [0, M] first: a negative value lands in bin 0, anything large in the top bin
__device__ __forceinline__ int cal_bin(float prod, int M) {
    const int b = (int)fminf(fmaxf(prod, 0.f), (float)M);
    return b < M - 1 ? b : M - 1;
}

// one run: the voxels of one histogram since its bin last changed
struct CalRun { int bin; unsigned cnt, hit; u64 sum; };
__device__ __forceinline__ void cal_flush(const CalRun& r, u64* __restrict__ hist, int M, int h) {
    if (r.cnt) {
        u64* w = hist + 2 * (h * M + r.bin);
        atomicAdd(w, (u64)r.cnt | ((u64)r.hit << 32));       // (a block sees fewer than 2^27 voxels: both halves stay below 2^32)
        atomicAdd(w + 1, r.sum);
    }
}
__device__ __forceinline__ void cal_add(CalRun& r, u64* __restrict__ hist, int M, int h, int bin, bool hit, u64 fx) {
    if (bin != r.bin) { cal_flush(r, hist, M, h); r.bin = bin; r.cnt = 0; r.hit = 0; r.sum = 0; }
    r.cnt += 1; r.hit += hit; r.sum += fx;
}

template <int K> struct CalAcc {
    CalRun run[K + 2];                   // 0: top, 1 .. K: cls[c], K + 1: unc
    unsigned n_valid, n_invalid, n_ignored;
    u64 nll, brier[K];
};

template <int K>
__device__ __forceinline__ void cal_voxel(CalAcc<K>& a, u64* __restrict__ hist, int M, const float* p, unsigned y, bool keep,
                                          bool has_unc, float u, float u_scale) {
    if (!keep) return;
    bool nan = has_unc && u != u;
#pragma unroll
    for (int c = 0; c < K; ++c) nan |= p[c] != p[c];
    if (nan) { a.n_invalid += 1; return; }
    if (y >= (unsigned)K) { a.n_ignored += 1; return; }
    a.n_valid += 1;
    int am = 0;                          // the lowest index among equals (np.argmax)
    float conf = p[0], py = p[0];
#pragma unroll
    for (int c = 1; c < K; ++c) {
        if (p[c] > conf) { conf = p[c]; am = c; }
        if (y == (unsigned)c) py = p[c];
    }
    const float fM = (float)M;
    cal_add(a.run[0], hist, M, 0, cal_bin(conf * fM, M), am == (int)y, cal_fx((double)conf));
#pragma unroll
    for (int c = 0; c < K; ++c) {
        const bool pos = y == (unsigned)c;
        cal_add(a.run[1 + c], hist, M, 1 + c, cal_bin(p[c] * fM, M), pos, cal_fx((double)p[c]));
        const double d = (double)p[c] - (pos ? 1.0 : 0.0);
        a.brier[c] += cal_fx(d * d);
    }
    a.nll += cal_fx(-log((double)fmaxf(py, CAL_EPS)));
    if (has_unc) cal_add(a.run[K + 1], hist, M, K + 1, cal_bin(u * u_scale, M), am != (int)y, cal_fx((double)fmaxf(u, 0.f)));
}

// 4 * K consecutive probabilities as floats; WIDE: 16-byte (fp32) / 8-byte (bf16) loads
template <int K, typename T, bool WIDE> __device__ __forceinline__ void cal_ld4(const T* s, float* o) {
    if constexpr (WIDE) {
#pragma unroll
        for (int i = 0; i < K; ++i) VecIO<T, 4>::ld(s + 4 * i, o + 4 * i);
    } else {
#pragma unroll
        for (int i = 0; i < 4 * K; ++i) o[i] = Act<T>::ld(s + i);
    }
}
template <bool WIDE> __device__ __forceinline__ void cal_ld4_u8(const unsigned char* s, unsigned* o) {
    if constexpr (WIDE) {
        const unsigned v = *reinterpret_cast<const unsigned*>(s);
        o[0] = v & 255u; o[1] = (v >> 8) & 255u; o[2] = (v >> 16) & 255u; o[3] = v >> 24;
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) o[i] = s[i];
    }
}

__device__ __forceinline__ u64 cal_wave_sum(u64 v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__global__ void __launch_bounds__(256) cal_zero_kernel(u64* __restrict__ rec, long long n) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) rec[i] = 0ull;
}

// Unit i of a case: i < V / 4 covers the voxels [4 i, 4 i + 4) (the vector body), i >= V / 4 the single voxel 4 (V / 4) + (i - V / 4)
// of the scalar tail.  Block x of a case walks the units x * 256 + t, + nb * 256, ...
template <int K, typename T, bool WIDE>
__global__ void __launch_bounds__(256) cal_score_kernel(CalP q, u64* __restrict__ rec, int slots) {
    __shared__ u64 hist[2 * (CAL_MAX_K + 2) * CAL_MAX_BINS];             // per (histogram, bin): count | hits << 32, sum
    __shared__ u64 head[CAL_HEAD];
    const int M = q.M, nh = (K + 2) * M, n = blockIdx.y;
    for (int i = threadIdx.x; i < 2 * nh; i += 256) hist[i] = 0ull;
    if (threadIdx.x < CAL_HEAD) head[threadIdx.x] = 0ull;
    __syncthreads();
    CalAcc<K> a;
#pragma unroll
    for (int h = 0; h < K + 2; ++h) { a.run[h].bin = 0; a.run[h].cnt = 0; a.run[h].hit = 0; a.run[h].sum = 0; }
    a.n_valid = a.n_invalid = a.n_ignored = 0; a.nll = 0;
#pragma unroll
    for (int c = 0; c < K; ++c) a.brier[c] = 0;
    const long long V4 = q.V >> 2, base = (long long)n * q.V;
    const T* __restrict__ pp = reinterpret_cast<const T*>(q.p) + base * K;
    const unsigned char* __restrict__ lp = q.label + base;
    const unsigned char* __restrict__ mp = q.mask ? q.mask + base : nullptr;
    const float* __restrict__ up = q.unc ? q.unc + base : nullptr;
    const bool has_unc = up != nullptr;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < V4 + (q.V & 3); i += (long long)q.nb * 256) {
        if (i < V4) {
            const long long v = i << 2;
            float pv[4 * K], uv[4] = {0.f, 0.f, 0.f, 0.f};
            unsigned yv[4], mv[4] = {1u, 1u, 1u, 1u};
            cal_ld4<K, T, WIDE>(pp + v * K, pv);
            cal_ld4_u8<WIDE>(lp + v, yv);
            if (mp) cal_ld4_u8<WIDE>(mp + v, mv);
            if (has_unc) {
                if constexpr (WIDE) VecIO<float, 4>::ld(up + v, uv);
                else {
#pragma unroll
                    for (int e = 0; e < 4; ++e) uv[e] = up[v + e];
                }
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) cal_voxel<K>(a, hist, M, pv + e * K, yv[e], mv[e] != 0u, has_unc, uv[e], q.u_scale);
        } else {
            const long long v = (V4 << 2) + (i - V4);
            float pv[K];
#pragma unroll
            for (int c = 0; c < K; ++c) pv[c] = Act<T>::ld(pp + v * K + c);
            cal_voxel<K>(a, hist, M, pv, lp[v], mp ? mp[v] != 0 : true, has_unc, has_unc ? up[v] : 0.f, q.u_scale);
        }
    }
#pragma unroll
    for (int h = 0; h < K + 2; ++h) cal_flush(a.run[h], hist, M, h);
    // header: wave sums, then one LDS add per wave and slot
    u64 hq[4 + K];
    hq[0] = a.n_valid; hq[1] = a.n_invalid; hq[2] = a.n_ignored; hq[3] = a.nll;
#pragma unroll
    for (int c = 0; c < K; ++c) hq[4 + c] = a.brier[c];
#pragma unroll
    for (int j = 0; j < 4 + K; ++j) hq[j] = cal_wave_sum(hq[j]);
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int j = 0; j < 4 + K; ++j)
            if (hq[j]) atomicAdd(&head[j], hq[j]);
    }
    __syncthreads();
    // one integer add per non-zero slot into the record: slot 8 + 3 M h + {0, M, 2 M} + b = count, sum, hits of (h, b)
    u64* __restrict__ r = rec + (size_t)n * slots;
    if (threadIdx.x < CAL_HEAD && head[threadIdx.x]) atomicAdd(r + threadIdx.x, head[threadIdx.x]);
    for (int i = threadIdx.x; i < nh; i += 256) {
        const u64 w = hist[2 * i], s = hist[2 * i + 1];
        const int h = i / M, b = i - h * M;
        u64* d = r + CAL_HEAD + 3 * M * h + b;
        if (w & 0xffffffffull) atomicAdd(d, w & 0xffffffffull);
        if (s) atomicAdd(d + M, s);
        if (w >> 32) atomicAdd(d + 2 * M, w >> 32);
    }
}

// blocks per case: about eight voxels per thread, at most M1_EW_BLOCKS (2048 at the most) -- a function of V and the switch alone
static inline int cal_blocks(long long V, int cap) {
    if (cap < 1) cap = 1;
    if (cap > 2048) cap = 2048;
    const long long b = cdiv_ll((V >> 2) + 3, 512);
    return (int)(b > cap ? cap : b);
}

extern "C" size_t m1_cal_record_slots(int K, int bins) {
    if (K < CAL_MIN_K || K > CAL_MAX_K || bins < 1 || bins > CAL_MAX_BINS) return 0;
    return (size_t)CAL_HEAD + 3 * (size_t)bins * (size_t)(K + 2);
}

template <int K, typename T>
static void cal_launch(const CalP& q, bool wide, int B, u64* rec, int slots, hipStream_t s) {
    if (wide) hipLaunchKernelGGL((cal_score_kernel<K, T, true>), dim3(q.nb, B), dim3(256), 0, s, q, rec, slots);
    else hipLaunchKernelGGL((cal_score_kernel<K, T, false>), dim3(q.nb, B), dim3(256), 0, s, q, rec, slots);
}
template <typename T>
static void cal_launch_k(const CalP& q, int K, bool wide, int B, u64* rec, int slots, hipStream_t s) {
    if (K == 2) cal_launch<2, T>(q, wide, B, rec, slots, s);
    else if (K == 3) cal_launch<3, T>(q, wide, B, rec, slots, s);
    else cal_launch<4, T>(q, wide, B, rec, slots, s);
}

extern "C" int m1_cal_score(const void* p, int p_dtype, const unsigned char* label, const unsigned char* mask, const float* unc,
                            float u_scale, int B, long long voxels, int K, int bins, unsigned long long* records, void* stream) {
    if (!p || !label || !records || B <= 0 || voxels <= 0 || voxels >= CAL_MAX_VOXELS) return M1_ERR_BAD_ARG;
    if (p_dtype != M1_F32 && p_dtype != M1_BF16) return M1_ERR_BAD_ARG;
    const size_t slots = m1_cal_record_slots(K, bins);
    if (!slots) return M1_ERR_BAD_ARG;
    const size_t esz = p_dtype == M1_F32 ? 4 : 2;
    if (((uintptr_t)p & (esz - 1)) || ((uintptr_t)unc & 3) || ((uintptr_t)records & 7)) return M1_ERR_BAD_ARG;
    if (unc && !(u_scale > 0.f && u_scale <= 3.4028234e38f)) return M1_ERR_BAD_ARG;          // (NaN fails the first comparison)
    if (B > 65535) return M1_ERR_UNSUPPORTED;
    if (m1_debug_skip("cal_score")) return M1_OK;
    CalP q;
    q.p = p; q.label = label; q.mask = mask; q.unc = unc; q.u_scale = unc ? u_scale : 0.f; q.V = voxels; q.M = bins;
    q.nb = cal_blocks(voxels, M1_CFG("M1_EW_BLOCKS", 2048));
    // wide loads: a unit of four voxels of p, label, mask and unc starts on a multiple of its own size in every case -- the first
    // case by the pointers, the later ones because a case is a whole number of units long
    const bool wide = !((uintptr_t)p % (4 * esz)) && !((uintptr_t)label & 3) && !((uintptr_t)mask & 3) && !((uintptr_t)unc & 15)
        && (B == 1 || (voxels & 3) == 0);
    hipStream_t s = (hipStream_t)stream;
    const long long n = (long long)B * (long long)slots;
    {
        M1ProfScope ps("cal_zero", 0.0, 8.0 * n, s);
        hipLaunchKernelGGL(cal_zero_kernel, dim3((unsigned)cdiv_ll(n, 256)), dim3(256), 0, s, (u64*)records, n);
    }
    {
        M1ProfScope ps("cal_score", 0.0, (double)B * voxels * (K * (double)esz + 1.0 + (mask ? 1.0 : 0.0) + (unc ? 4.0 : 0.0)) + 8.0 * n, s);
        if (p_dtype == M1_F32) cal_launch_k<float>(q, K, wide, B, (u64*)records, (int)slots, s);
        else cal_launch_k<bf16_t>(q, K, wide, B, (u64*)records, (int)slots, s);
    }
    return m1_check_launch();
}
