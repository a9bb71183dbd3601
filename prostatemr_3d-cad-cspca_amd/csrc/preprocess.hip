// preprocess.hip -- the numerical part of the reference's preprocess.py on the device: whitening with a percentile clip (P:29-39),
// center_crop (P:42-49) and resize_image_with_crop_or_pad (P:74-98), read from the RAW (B, d, h, w, C) fp32 / int16 source through one
// crop / pad index map (m1_crop_pad_t), so that no cropped or padded intermediate volume exists.
//   m1_crop_pad   : the gather alone, one launch.
//   m1_order_stats: exact order statistics of every (b, c) slice's output domain by radix select on the order-preserving key of the
//                   fp32 value, four passes of 8 bits.  Per pass: os_hist_kernel (a block owns one chunk of one slice; one 256-bin LDS
//                   histogram per GROUP of ranks whose prefixes still agree, filled with integer LDS atomics -- a thread first merges
//                   its run of equal bins, which is what keeps the leading digits of clustered data off one LDS address -- and stored
//                   whole, so nothing is zero-filled) and os_scan_kernel (one block per slice folds the blocks' histograms, scans the
//                   256 counts and moves every rank into its bin).  The 2 nq ranks {k, min(k + 1, n - 1)} are selected side by side:
//                   the successor costs no pass of its own and shares its neighbour's histogram until their keys part.
//   m1_whiten     : per-block {count, mean, M2} in fp64 from two sweeps of the block's own chunk, a Chan merge in block order, and
//                   the element pass.
// Compiled without contraction (see augment.hip): the element pass is exactly sub, div.
#include "common.h"

#pragma clang fp contract(off)

#define PP_NT 256
#define PP_MAX_C 8
#define PP_MAX_NQ 4
#define PP_MAXG (2 * PP_MAX_NQ)      // ranks selected side by side: {k, k + 1} per quantile
#define PP_CHUNK 2048                // smallest chunk of a slice one block takes
#define PP_MAX_BLK 64                // blocks per slice at most

struct PPGeom { int s0, s1, s2, d0, d1, d2, t0, t1, t2, mode; float cval; };

__device__ __forceinline__ float pp_ld(const float* p) { return *p; }
__device__ __forceinline__ float pp_ld(const int16_t* p) { return (float)*p; }

// source index of i = o + start on an axis of n voxels; `oob` is raised where M1_PAD_CONSTANT supplies the value.  Always in [0, n).
__device__ __forceinline__ int pp_axis(int i, int n, int mode, bool& oob) {
    if (i >= 0 && i < n) return i;
    int r;
    if (mode == M1_PAD_CONSTANT) { oob = true; return 0; }
    if (mode == M1_PAD_EDGE) {
        r = i < 0 ? 0 : n - 1;
    } else if (mode == M1_PAD_REFLECT) {
        if (n == 1) return 0;
        const int p = 2 * (n - 1);
        r = i % p;
        if (r < 0) r += p;
        if (r >= n) r = p - r;
    } else {
        const int p = 2 * n;
        r = i % p;
        if (r < 0) r += p;
        if (r >= n) r = p - 1 - r;
    }
    return min(max(r, 0), n - 1);
}

// value i of the output domain of slice (b, c), i = (oz * d1 + oy) * d2 + ox
template <typename S>
__device__ __forceinline__ float pp_fetch(const S* __restrict__ src, const PPGeom& g, int C, long long b, int c, int i) {
    const int r = i / g.d2, ox = i - r * g.d2;
    const int oz = r / g.d1, oy = r - oz * g.d1;
    bool oob = false;
    const int sz = pp_axis(oz + g.t0, g.s0, g.mode, oob), sy = pp_axis(oy + g.t1, g.s1, g.mode, oob),
              sx = pp_axis(ox + g.t2, g.s2, g.mode, oob);
    if (oob) return g.cval;
    return pp_ld(src + ((((b * g.s0 + sz) * g.s1 + sy) * (long long)g.s2 + sx) * C + c));
}

__device__ __forceinline__ void pp_ld4(const float* p, float* v) { VecIO<float, 4>::ld(p, v); }
__device__ __forceinline__ void pp_ld4(const int16_t* p, float* v) {
    const uint2 w = *reinterpret_cast<const uint2*>(p);
    v[0] = (float)(int16_t)(w.x & 0xffffu); v[1] = (float)(int16_t)(w.x >> 16);
    v[2] = (float)(int16_t)(w.y & 0xffffu); v[3] = (float)(int16_t)(w.y >> 16);
}

// ---- the element pass: m1_crop_pad (WHITEN = false) and the last launch of m1_whiten ----
// An item is G consecutive elements of one output row (a row = dst[2] * C contiguous elements); G = 4 with VEC.
template <typename S, typename O, bool VEC, bool WHITEN>
__global__ void __launch_bounds__(PP_NT) pp_rows_kernel(const S* __restrict__ src, PPGeom g, int C, long long items, int per_row,
                                                        const float* __restrict__ bounds, const double* __restrict__ stats,
                                                        O* __restrict__ out) {
    constexpr int G = VEC ? 4 : 1;
    for (long long it = (long long)blockIdx.x * PP_NT + threadIdx.x; it < items; it += (long long)gridDim.x * PP_NT) {
        const long long row = it / per_row;
        const int e0 = (int)(it - row * per_row) * G;
        const long long r2 = row / g.d1;
        const int oy = (int)(row - r2 * g.d1);
        const long long b = r2 / g.d0;
        const int oz = (int)(r2 - b * g.d0);
        bool row_oob = false;
        const int sz = pp_axis(oz + g.t0, g.s0, g.mode, row_oob), sy = pp_axis(oy + g.t1, g.s1, g.mode, row_oob);
        const S* rowp = src + ((b * g.s0 + sz) * g.s1 + sy) * (long long)g.s2 * C;
        float v[G];
        bool done = false;
        if constexpr (VEC) {
            // the four elements are contiguous in the source when the voxels of the first and the last lie inside the row
            const int ox0 = e0 / C, ox3 = (e0 + 3) / C;
            if (!row_oob && ox0 + g.t2 >= 0 && ox3 + g.t2 < g.s2) {
                const S* p = rowp + (long long)(ox0 + g.t2) * C + (e0 - ox0 * C);
                if ((((uintptr_t)p) & (4 * sizeof(S) - 1)) == 0) { pp_ld4(p, v); done = true; }
            }
        }
        if (!done) {
#pragma unroll
            for (int k = 0; k < G; ++k) {
                const int e = e0 + k, ox = e / C, c = e - ox * C;
                bool oob = row_oob;
                const int sx = pp_axis(ox + g.t2, g.s2, g.mode, oob);
                v[k] = oob ? g.cval : pp_ld(rowp + (long long)sx * C + c);
            }
        }
        if constexpr (WHITEN) {
#pragma unroll
            for (int k = 0; k < G; ++k) {
                const long long sl = b * C + (e0 + k) % C;
                float y = v[k];
                if (bounds) y = fminf(fmaxf(y, bounds[2 * sl]), bounds[2 * sl + 1]);
                const float mean = (float)stats[2 * sl], sd = (float)stats[2 * sl + 1];
                v[k] = sd > 0.f ? (y - mean) / sd : 0.f;
            }
        }
        O* o = out + row * ((long long)g.d2 * C) + e0;
        if constexpr (VEC) VecIO<O, 4>::st(o, v);
        else Act<O>::st(o, v[0]);
    }
}

// ---- selection ----
struct OsState {                      // per slice, in ws
    unsigned prefix[PP_MAXG];         // key bits fixed so far of rank r (0 below the current digit)
    unsigned krem[PP_MAXG];           // rank r among the elements that share its prefix
    unsigned gprefix[PP_MAXG];        // the distinct prefixes: one histogram each
    int qgroup[PP_MAXG];              // rank r counts in histogram qgroup[r]
    int ngroups;
    int _pad[7];
};
struct OsRanks { int nq; int k[PP_MAX_NQ]; double w[PP_MAX_NQ]; };

__device__ __forceinline__ unsigned os_key(float f) {
    const unsigned u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float os_unkey(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

// grid = slices * nblk; part[((slice * nblk + blk) * maxg + group) * 256 + digit]
template <typename S>
__global__ void __launch_bounds__(PP_NT) os_hist_kernel(const S* __restrict__ src, PPGeom g, int C, int n, int nblk, int chunk,
                                                        int pass, int maxg, const OsState* __restrict__ state,
                                                        unsigned* __restrict__ part) {
    __shared__ unsigned hist[PP_MAXG * 256];
    __shared__ unsigned gp[PP_MAXG];
    const int t = threadIdx.x;
    const int slice = blockIdx.x / nblk, blk = blockIdx.x - slice * nblk;
    const int ng = pass == 0 ? 1 : min(max(state[slice].ngroups, 1), maxg);
    for (int i = t; i < ng * 256; i += PP_NT) hist[i] = 0u;
    if (t < ng) gp[t] = pass == 0 ? 0u : state[slice].gprefix[t];
    __syncthreads();
    const int shift = 24 - 8 * pass;
    const unsigned mask = pass == 0 ? 0u : (0xffffffffu << (shift + 8));
    const long long b = slice / C;
    const int c = slice - (int)b * C;
    const int i0 = (int)min((long long)blk * chunk, (long long)n), i1 = (int)min((long long)i0 + chunk, (long long)n);
    int cur = -1;
    unsigned run = 0u;
    for (int i = i0 + t; i < i1; i += PP_NT) {
        const unsigned key = os_key(pp_fetch(src, g, C, b, c, i));
        const unsigned hi = key & mask;
        int grp = -1;
        for (int k = 0; k < ng; ++k) grp = gp[k] == hi ? k : grp;      // (the prefixes are distinct: at most one matches)
        if (grp < 0) continue;
        const int bin = grp * 256 + (int)((key >> shift) & 255u);
        if (bin == cur) { ++run; continue; }
        if (run) atomicAdd(&hist[cur], run);
        cur = bin; run = 1u;
    }
    if (run) atomicAdd(&hist[cur], run);
    __syncthreads();
    unsigned* dst = part + ((long long)blockIdx.x * maxg) * 256;
    for (int i = t; i < ng * 256; i += PP_NT) dst[i] = hist[i];
}

// one block per slice; thread t owns digit t
__global__ void __launch_bounds__(PP_NT) os_scan_kernel(OsState* __restrict__ state, const unsigned* __restrict__ part, int n, int nblk,
                                                        int pass, int maxg, OsRanks rk, float* __restrict__ pairs,
                                                        float* __restrict__ values) {
    __shared__ unsigned sc[2][PP_NT];
    __shared__ OsState st;
    __shared__ unsigned npre[PP_MAXG], nkrem[PP_MAXG];
    const int t = threadIdx.x, slice = blockIdx.x, nr = 2 * rk.nq;
    if (t == 0) {
        if (pass == 0) {
            for (int r = 0; r < PP_MAXG; ++r) {
                const int k = r < nr ? rk.k[r >> 1] : 0;
                st.prefix[r] = 0u; st.qgroup[r] = 0; st.gprefix[r] = 0u;
                st.krem[r] = (unsigned)((r & 1) ? min(k + 1, n - 1) : k);
            }
            st.ngroups = 1;
        } else {
            st = state[slice];
            st.ngroups = min(max(st.ngroups, 1), maxg);
        }
        for (int r = 0; r < PP_MAXG; ++r) { npre[r] = st.prefix[r]; nkrem[r] = st.krem[r]; }
    }
    __syncthreads();
    const int shift = 24 - 8 * pass;
    for (int gi = 0; gi < st.ngroups; ++gi) {
        unsigned cnt = 0u;
        const unsigned* p = part + (((long long)slice * nblk) * maxg + gi) * 256 + t;
        for (int bk = 0; bk < nblk; ++bk) cnt += p[(long long)bk * maxg * 256];
        // inclusive scan of the 256 counts
        int w = 0;
        sc[0][t] = cnt;
        __syncthreads();
        for (int o = 1; o < PP_NT; o <<= 1) {
            sc[w ^ 1][t] = sc[w][t] + (t >= o ? sc[w][t - o] : 0u);
            w ^= 1;
            __syncthreads();
        }
        const unsigned incl = sc[w][t], excl = incl - cnt;
        for (int r = 0; r < nr; ++r) {
            if (st.qgroup[r] != gi) continue;
            const unsigned k = st.krem[r];
            if (k >= excl && k < incl) { npre[r] = st.prefix[r] | ((unsigned)t << shift); nkrem[r] = k - excl; }
        }
        __syncthreads();
    }
    if (t != 0) return;
    int ng = 0;
    for (int r = 0; r < nr; ++r) {
        st.prefix[r] = npre[r]; st.krem[r] = nkrem[r];
        int f = -1;
        for (int k = 0; k < ng; ++k) f = st.gprefix[k] == npre[r] ? k : f;
        if (f < 0) { f = ng; st.gprefix[ng++] = npre[r]; }
        st.qgroup[r] = f;
    }
    st.ngroups = ng;
    if (pass < 3) { state[slice] = st; return; }
    for (int j = 0; j < rk.nq; ++j) {
        const float a = os_unkey(st.prefix[2 * j]), b = os_unkey(st.prefix[2 * j + 1]);
        const long long o = (long long)slice * rk.nq + j;
        pairs[2 * o] = a;
        pairs[2 * o + 1] = b;
        values[o] = (float)((double)a + ((double)b - (double)a) * rk.w[j]);
    }
}

// ---- whitening statistics ----
// fixed-order block sum: shuffles inside a wave, then the four wave sums in wave order
__device__ __forceinline__ double pp_block_sum(double v, double* sh) {
    v = wave_sum_d(v);
    __syncthreads();                                    // (sh may still be read from the previous call)
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((sh[0] + sh[1]) + sh[2]) + sh[3];
}

// part[(slice * nblk + blk) * 3 + {0, 1, 2}] = {count, mean, M2} of the block's chunk
template <typename S>
__global__ void __launch_bounds__(PP_NT) wh_stats_kernel(const S* __restrict__ src, PPGeom g, int C, int n, int nblk, int chunk,
                                                         const float* __restrict__ bounds, double* __restrict__ part) {
    __shared__ double sh[PP_NT / 64];
    const int t = threadIdx.x;
    const int slice = blockIdx.x / nblk, blk = blockIdx.x - slice * nblk;
    const long long b = slice / C;
    const int c = slice - (int)b * C;
    const bool clip = bounds != nullptr;
    const float lo = clip ? bounds[2 * slice] : 0.f, hi = clip ? bounds[2 * slice + 1] : 0.f;
    const int i0 = (int)min((long long)blk * chunk, (long long)n), i1 = (int)min((long long)i0 + chunk, (long long)n);
    double s = 0.0;
    for (int i = i0 + t; i < i1; i += PP_NT) {
        float y = pp_fetch(src, g, C, b, c, i);
        if (clip) y = fminf(fmaxf(y, lo), hi);
        s += (double)y;
    }
    const double cnt = (double)(i1 - i0);
    const double mean = i1 > i0 ? pp_block_sum(s, sh) / cnt : 0.0;
    double m2 = 0.0;
    for (int i = i0 + t; i < i1; i += PP_NT) {
        float y = pp_fetch(src, g, C, b, c, i);
        if (clip) y = fminf(fmaxf(y, lo), hi);
        const double d = (double)y - mean;
        m2 += d * d;
    }
    m2 = pp_block_sum(m2, sh);
    if (t == 0) {
        double* o = part + ((long long)blockIdx.x) * 3;
        o[0] = cnt; o[1] = mean; o[2] = m2;
    }
}

// one thread per slice: Chan's merge of the blocks' {count, mean, M2} in block order -> stats = {mean, population std}
__global__ void __launch_bounds__(64) wh_fold_kernel(const double* __restrict__ part, int slices, int nblk, double* __restrict__ stats) {
    const int slice = blockIdx.x * 64 + threadIdx.x;
    if (slice >= slices) return;
    double cn = 0.0, mean = 0.0, m2 = 0.0;
    for (int bk = 0; bk < nblk; ++bk) {
        const double* p = part + ((long long)slice * nblk + bk) * 3;
        const double nb = p[0];
        if (!(nb > 0.0)) continue;
        const double delta = p[1] - mean, tot = cn + nb;
        mean = mean + delta * (nb / tot);
        m2 = (m2 + p[2]) + (delta * delta) * (cn * nb / tot);
        cn = tot;
    }
    stats[2 * slice] = mean;
    stats[2 * slice + 1] = cn > 0.0 ? sqrt(m2 / cn) : 0.0;
}

// ---- host ----
static inline bool pp_al(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

struct PPPlan { PPGeom g; int n, nblk, chunk, slices; };

// the checks every entry point shares: M1_OK and the plan, or the status to return
static int pp_plan(const void* src, int src_dtype, const m1_crop_pad_t* g, int B, int C, PPPlan& pl) {
    if (!g || B <= 0 || C <= 0) return M1_ERR_BAD_ARG;
    for (int a = 0; a < 3; ++a)
        if (g->src[a] <= 0 || g->dst[a] <= 0) return M1_ERR_BAD_ARG;
    if (src_dtype != M1_RAW_F32 && src_dtype != M1_RAW_I16) return M1_ERR_UNSUPPORTED;
    if (g->mode < M1_PAD_CONSTANT || g->mode > M1_PAD_SYMMETRIC) return M1_ERR_UNSUPPORTED;
    if (C > PP_MAX_C) return M1_ERR_UNSUPPORTED;
    const long long n = (long long)g->dst[0] * g->dst[1] * g->dst[2];
    if (n >= (1ll << 31)) return M1_ERR_UNSUPPORTED;
    const long long sv = (long long)g->src[0] * g->src[1] * g->src[2];
    if (sv >= (1ll << 31) || (long long)B * C > (1 << 20)) return M1_ERR_UNSUPPORTED;      // (block and element indices stay far inside 63 bits)
    for (int a = 0; a < 3; ++a)
        if (g->start[a] <= -(1 << 30) || g->start[a] >= (1 << 30)) return M1_ERR_BAD_ARG;    // (o + start stays an int)
    if (src && !pp_al(src, src_dtype == M1_RAW_I16 ? 2 : 4)) return M1_ERR_BAD_ARG;
    pl.g = PPGeom{g->src[0], g->src[1], g->src[2], g->dst[0], g->dst[1], g->dst[2], g->start[0], g->start[1], g->start[2], g->mode,
                  g->cval};
    pl.n = (int)n;
    long long nb = cdiv_ll(n, PP_CHUNK);
    if (nb > PP_MAX_BLK) nb = PP_MAX_BLK;
    pl.chunk = (int)cdiv_ll(n, nb);
    pl.nblk = (int)cdiv_ll(n, pl.chunk);
    pl.slices = B * C;
    return M1_OK;
}

static size_t pp_os_state_bytes(const PPPlan& pl) { return (size_t)pl.slices * sizeof(OsState); }
static size_t pp_os_bytes(const PPPlan& pl, int nq) { return pp_os_state_bytes(pl) + (size_t)pl.slices * pl.nblk * (2 * nq) * 256 * sizeof(unsigned); }
static size_t pp_wh_bytes(const PPPlan& pl) { return (size_t)pl.slices * pl.nblk * 3 * sizeof(double); }

extern "C" size_t m1_preprocess_ws_bytes(const m1_crop_pad_t* g, int B, int C, int nq) {
    PPPlan pl;
    if (nq < 0 || nq > PP_MAX_NQ || pp_plan(nullptr, M1_RAW_F32, g, B, C, pl) != M1_OK) return 0;
    const size_t a = nq ? pp_os_bytes(pl, nq) : 0, b = pp_wh_bytes(pl);
    return a > b ? a : b;
}

template <typename S, typename O, bool WHITEN>
static void pp_rows_launch(const void* src, const PPPlan& pl, int B, int C, const float* bounds, const double* stats, void* out,
                           hipStream_t st) {
    const long long rows = (long long)B * pl.g.d0 * pl.g.d1;
    const int rw = pl.g.d2 * C;
    const bool vec = (rw & 3) == 0 && pp_al(out, 4 * sizeof(O));
    const int per_row = vec ? rw / 4 : rw;
    const long long items = rows * per_row;
    const dim3 grid(m1_grid_for(items, 1)), block(PP_NT);
    if (vec) hipLaunchKernelGGL((pp_rows_kernel<S, O, true, WHITEN>), grid, block, 0, st, (const S*)src, pl.g, C, items, per_row, bounds, stats, (O*)out);
    else hipLaunchKernelGGL((pp_rows_kernel<S, O, false, WHITEN>), grid, block, 0, st, (const S*)src, pl.g, C, items, per_row, bounds, stats, (O*)out);
}
template <bool WHITEN>
static void pp_rows_dispatch(const void* src, int src_dtype, const PPPlan& pl, int B, int C, const float* bounds, const double* stats,
                             void* out, int out_dtype, hipStream_t st) {
    if (src_dtype == M1_RAW_I16) {
        if (out_dtype == M1_BF16) pp_rows_launch<int16_t, bf16_t, WHITEN>(src, pl, B, C, bounds, stats, out, st);
        else pp_rows_launch<int16_t, float, WHITEN>(src, pl, B, C, bounds, stats, out, st);
    } else {
        if (out_dtype == M1_BF16) pp_rows_launch<float, bf16_t, WHITEN>(src, pl, B, C, bounds, stats, out, st);
        else pp_rows_launch<float, float, WHITEN>(src, pl, B, C, bounds, stats, out, st);
    }
}

static inline double pp_src_bytes(int src_dtype) { return src_dtype == M1_RAW_I16 ? 2.0 : 4.0; }

extern "C" int m1_crop_pad(const void* src, int src_dtype, const m1_crop_pad_t* g, int B, int C, void* out, int out_dtype,
                           void* stream) {
    if (m1_debug_skip("crop_pad")) return M1_OK;
    if (!src || !out) return M1_ERR_BAD_ARG;
    PPPlan pl;
    if (int rc = pp_plan(src, src_dtype, g, B, C, pl)) return rc;
    if (out_dtype != M1_F32 && out_dtype != M1_BF16) return M1_ERR_UNSUPPORTED;
    if (!pp_al(out, out_dtype == M1_BF16 ? 2 : 4)) return M1_ERR_BAD_ARG;
    hipStream_t st = (hipStream_t)stream;
    const double el = (double)pl.slices * pl.n;
    M1ProfScope ps("crop_pad", 0.0, el * (pp_src_bytes(src_dtype) + (out_dtype == M1_BF16 ? 2.0 : 4.0)), st);
    pp_rows_dispatch<false>(src, src_dtype, pl, B, C, nullptr, nullptr, out, out_dtype, st);
    return m1_check_launch();
}

extern "C" int m1_order_stats(const void* src, int src_dtype, const m1_crop_pad_t* g, int B, int C, const int* ranks,
                              const double* weights, int nq, float* pairs, float* values, void* ws, void* stream) {
    if (m1_debug_skip("order_stats")) return M1_OK;
    if (!src || !ranks || !weights || !pairs || !values || !ws || nq <= 0) return M1_ERR_BAD_ARG;
    PPPlan pl;
    if (int rc = pp_plan(src, src_dtype, g, B, C, pl)) return rc;
    if (nq > PP_MAX_NQ) return M1_ERR_UNSUPPORTED;
    if (!pp_al(pairs, 4) || !pp_al(values, 4) || !pp_al(ws, 8)) return M1_ERR_BAD_ARG;
    OsRanks rk;
    rk.nq = nq;
    for (int j = 0; j < PP_MAX_NQ; ++j) { rk.k[j] = 0; rk.w[j] = 0.0; }
    for (int j = 0; j < nq; ++j) {
        if (ranks[j] < 0 || ranks[j] >= pl.n || !(weights[j] >= 0.0 && weights[j] <= 1.0)) return M1_ERR_BAD_ARG;
        rk.k[j] = ranks[j];
        rk.w[j] = weights[j];
    }
    hipStream_t st = (hipStream_t)stream;
    const int maxg = 2 * nq;
    OsState* state = (OsState*)ws;
    unsigned* part = (unsigned*)((char*)ws + pp_os_state_bytes(pl));
    const double el = (double)pl.slices * pl.n;
    M1ProfScope ps("order_stats", 0.0, 4.0 * el * pp_src_bytes(src_dtype) + 12.0 * pl.slices * nq, st);
    const dim3 hgrid((unsigned)(pl.slices * pl.nblk)), sgrid((unsigned)pl.slices), block(PP_NT);
    for (int pass = 0; pass < 4; ++pass) {
        if (src_dtype == M1_RAW_I16)
            hipLaunchKernelGGL(os_hist_kernel<int16_t>, hgrid, block, 0, st, (const int16_t*)src, pl.g, C, pl.n, pl.nblk, pl.chunk, pass, maxg, state, part);
        else
            hipLaunchKernelGGL(os_hist_kernel<float>, hgrid, block, 0, st, (const float*)src, pl.g, C, pl.n, pl.nblk, pl.chunk, pass, maxg, state, part);
        hipLaunchKernelGGL(os_scan_kernel, sgrid, block, 0, st, state, part, pl.n, pl.nblk, pass, maxg, rk, pairs, values);
    }
    return m1_check_launch();
}

extern "C" int m1_whiten(const void* src, int src_dtype, const m1_crop_pad_t* g, int B, int C, const float* bounds, void* out,
                         int out_dtype, double* stats, void* ws, void* stream) {
    if (m1_debug_skip("whiten")) return M1_OK;
    if (!src || !out || !stats || !ws) return M1_ERR_BAD_ARG;
    PPPlan pl;
    if (int rc = pp_plan(src, src_dtype, g, B, C, pl)) return rc;
    if (out_dtype != M1_F32 && out_dtype != M1_BF16) return M1_ERR_UNSUPPORTED;
    if (!pp_al(out, out_dtype == M1_BF16 ? 2 : 4) || !pp_al(bounds, 4) || !pp_al(stats, 8) || !pp_al(ws, 8)) return M1_ERR_BAD_ARG;
    hipStream_t st = (hipStream_t)stream;
    const double el = (double)pl.slices * pl.n;
    M1ProfScope ps("whiten", 0.0, el * (3.0 * pp_src_bytes(src_dtype) + (out_dtype == M1_BF16 ? 2.0 : 4.0)) + 16.0 * pl.slices, st);
    double* part = (double*)ws;
    const dim3 grid((unsigned)(pl.slices * pl.nblk)), block(PP_NT);
    if (src_dtype == M1_RAW_I16)
        hipLaunchKernelGGL(wh_stats_kernel<int16_t>, grid, block, 0, st, (const int16_t*)src, pl.g, C, pl.n, pl.nblk, pl.chunk, bounds, part);
    else
        hipLaunchKernelGGL(wh_stats_kernel<float>, grid, block, 0, st, (const float*)src, pl.g, C, pl.n, pl.nblk, pl.chunk, bounds, part);
    hipLaunchKernelGGL(wh_fold_kernel, dim3((unsigned)((pl.slices + 63) / 64)), dim3(64), 0, st, part, pl.slices, pl.nblk, stats);
    pp_rows_dispatch<true>(src, src_dtype, pl, B, C, bounds, stats, out, out_dtype, st);
    return m1_check_launch();
}
