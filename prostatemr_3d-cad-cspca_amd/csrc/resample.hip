// resample.hip -- the reference's resample_img (tf2.5/scripts/preprocess.py, P:52-71) on the device: a raw (B, d, h, w, C) fp32 / int16
// volume onto an axis-aligned grid (m1_resample_t: output o of an axis reads the continuous source index (first + o) * step), by a cubic
// B-spline (order 3) or by nearest neighbour (order 0).  The grid of P:52-71 keeps origin and direction and uses the identity transform,
// so the operation is separable.
//   order 3: one pass per axis in the order 2, 1, 0 (the contiguous axis first: the int16 source is read once at 2 bytes per element,
//            and a down-sampled or windowed axis shrinks before the next pass reads it).  A pass prefilters every whole line of its axis
//            (Unser's recursive filter: pole z = sqrt(3) - 2, gain (1 - z)(1 - 1/z) = 6, mirror boundary of period 2(n - 1)) and then
//            emits the window's outputs as 4-tap sums through the mirror map.  fp32 values; the coordinate, its floor and its fraction
//            are fp64.
//     rs_rows_kernel: axis 2.  A line is a contiguous row of w * C elements, channels interleaved.  A block stages a tile of rows into
//            LDS with coalesced loads (16 bytes per lane where the row length and the pointer allow), one thread per (row, channel) runs
//            the two recursions in LDS, then all threads emit the tile's outputs with coalesced stores.  Row pitch = w * C rounded up
//            to C (mod 32): lane (row, c) of the recursion then starts at bank (row * C + c) mod 32 and every step moves all lanes by
//            C banks, so 32 consecutive lanes stay on 32 different banks of the 4-byte LDS reads (the 32-bank, 32-lane-group rule).
//     rs_cols_kernel: axes 1 and 0.  A line is strided by `inner` elements; consecutive threads take consecutive columns, so every
//            global access coalesces without staging.  Lines up to RS_SHORT voxels are copied to LDS (one column per thread, pitch
//            RS_NT: conflict free) and filtered there; longer lines are filtered in place in the workspace volume they are read from.
//            The issue of a dynamic tap index is why the short lines sit in LDS and not in a register array: indexing a register array
//            by floor(x) would send it to scratch.
//            The pass over axis 0 is the last and writes `defval` where any axis is outside (-0.5 <= x < n - 0.5, ITK's IsInsideBuffer).
//   order 0: rs_nearest_kernel, one gather launch: source index floor(x + 0.5) per axis, `defval` outside.
// Causal start: c+[0] = sum_k z^k s[k] over the mirror extension.  Lines of up to RS_HORIZON voxels use the closed form of the periodic
// sum; longer lines truncate it after RS_HORIZON = 24 terms, which drops at most |z|^24 / (1 - |z|) = 2.6e-14 of max|s| -- 2^-21 of the
// 2^-24 unit the fp32 arithmetic works in.  Lines are never split.
// Values at outside voxels of an earlier pass are computed at x = 0: their column only feeds outputs that are outside as well.
// Compiled without contraction, like preprocess.hip: every weight and sum is mul, add in the written order.
#include "common.h"

#pragma clang fp contract(off)

#define RS_NT 256
#define RS_MAX_C 8
#define RS_MAX_LINE M1_RESAMPLE_MAX_LINE
#define RS_LDS_FLOATS 12288          // the row tile of rs_rows_kernel: 48 KiB, three blocks per CU
#define RS_ROWS 64                   // rows per tile at most
#define RS_SHORT 32                  // strided lines up to this length are filtered in LDS (32 * 256 * 4 B = 32 KiB)
#define RS_HORIZON 24                // terms of the truncated causal start
#define RS_UNROLL 8                  // samples a recursion loads ahead of its dependent chain
#define RS_POLE (-0.2679491924311227f)              // sqrt(3) - 2

static_assert((RS_MAX_LINE * RS_MAX_C + 32) <= RS_LDS_FLOATS, "one row at the line limit fits the tile");

struct RSAxis { int n, dn, first, _pad; double step; };
struct RSMask { RSAxis a1, a2; int C; float defval; };

__device__ __forceinline__ float rs_ld(const float* p) { return *p; }
__device__ __forceinline__ float rs_ld(const int16_t* p) { return (float)*p; }
__device__ __forceinline__ void rs_ld4(const float* p, float* v) { VecIO<float, 4>::ld(p, v); }
__device__ __forceinline__ void rs_ld4(const int16_t* p, float* v) {
    const uint2 w = *reinterpret_cast<const uint2*>(p);
    v[0] = (float)(int16_t)(w.x & 0xffffu); v[1] = (float)(int16_t)(w.x >> 16);
    v[2] = (float)(int16_t)(w.y & 0xffffu); v[3] = (float)(int16_t)(w.y >> 16);
}

__device__ __forceinline__ bool rs_inside(const RSAxis& a, int o, double& x) {
    x = (double)(a.first + o) * a.step;
    return x >= -0.5 && x < (double)a.n - 0.5;
}

// mirror map of period 2(n - 1) for j in [-2, n + 1], which is where the taps of an inside coordinate lie; always in [0, n)
__device__ __forceinline__ int rs_mirror(int j, int n) {
    j = j < 0 ? -j : j;
    if (j >= n) j = 2 * (n - 1) - j;
    j = j < 0 ? -j : j;
    return min(max(j, 0), n - 1);
}

// taps and weights of output o; false (and the taps of x = 0) where the coordinate is outside
__device__ __forceinline__ bool rs_coord(const RSAxis& a, int o, int* idx, float* w) {
    double x;
    const bool in = rs_inside(a, o, x);
    if (!in) x = 0.0;
    const double fl = floor(x);
    const float y = (float)(x - fl), z = 1.f - y;
    w[0] = z * z * z / 6.f;
    w[1] = (y * y * (y - 2.f) * 3.f + 4.f) / 6.f;
    w[2] = (z * z * (z - 2.f) * 3.f + 4.f) / 6.f;
    w[3] = y * y * y / 6.f;
    const int i = (int)fl;
#pragma unroll
    for (int k = 0; k < 4; ++k) idx[k] = rs_mirror(i - 1 + k, a.n);
    return in;
}

// the prefilter of one line of n voxels at c[k * s], in place
template <typename I>
__device__ __forceinline__ void rs_prefilter(float* c, I s, int n) {
    if (n < 2) return;
    const float z = RS_POLE, gain = 6.f;
    float acc, zi = z;
    if (n <= RS_HORIZON) {
        float zn = z;                                                   // z^(n - 1)
        for (int k = 2; k < n; ++k) zn *= z;
        acc = c[0] + zn * c[(n - 1) * s];
        for (int i = 1; i < n - 1; ++i) {
            acc += zi * (c[i * s] + zn * c[(n - 1 - i) * s]);
            zi *= z;
        }
        acc = acc / (1.f - zn * zn);
    } else {
        acc = c[0];
        for (int k = 1; k < RS_HORIZON; ++k) {
            acc += zi * c[k * s];
            zi *= z;
        }
    }
    acc *= gain;
    c[0] = acc;
    // both recursions load RS_UNROLL samples ahead of the dependent chain (the line is updated in place, so the compiler cannot move a
    // load across the store before it on its own): one memory latency per RS_UNROLL steps, the same operations in the same order
    float v[RS_UNROLL];
    int k = 1;
    for (; k + RS_UNROLL <= n; k += RS_UNROLL) {
#pragma unroll
        for (int u = 0; u < RS_UNROLL; ++u) v[u] = c[(k + u) * s];
#pragma unroll
        for (int u = 0; u < RS_UNROLL; ++u) {
            acc = gain * v[u] + z * acc;
            c[(k + u) * s] = acc;
        }
    }
    for (; k < n; ++k) {
        acc = gain * c[k * s] + z * acc;
        c[k * s] = acc;
    }
    acc = (z * c[(n - 2) * s] + acc) * (z / (z * z - 1.f));
    c[(n - 1) * s] = acc;
    k = n - 2;
    for (; k >= RS_UNROLL - 1; k -= RS_UNROLL) {
#pragma unroll
        for (int u = 0; u < RS_UNROLL; ++u) v[u] = c[(k - u) * s];
#pragma unroll
        for (int u = 0; u < RS_UNROLL; ++u) {
            acc = z * (acc - v[u]);
            c[(k - u) * s] = acc;
        }
    }
    for (; k >= 0; --k) {
        acc = z * (acc - c[k * s]);
        c[k * s] = acc;
    }
}

template <typename I>
__device__ __forceinline__ float rs_taps(const float* c, I s, const int* idx, const float* w) {
    return ((w[0] * c[idx[0] * s] + w[1] * c[idx[1] * s]) + w[2] * c[idx[2] * s]) + w[3] * c[idx[3] * s];
}

// ---- axis 2: rows of rw = n * C contiguous elements; a block takes R rows ----
template <typename S, bool VEC>
__global__ void __launch_bounds__(RS_NT) rs_rows_kernel(const S* __restrict__ src, float* __restrict__ out, long long rows, int R,
                                                        int C, int pitch, RSAxis a) {
    __shared__ float tile[RS_LDS_FLOATS];
    const int t = threadIdx.x;
    const long long row0 = (long long)blockIdx.x * R;
    const int nr = (int)min((long long)R, rows - row0);
    const int rw = a.n * C;
    const S* sp = src + row0 * rw;
    if constexpr (VEC) {                                                // rw % 4 == 0 and src is aligned to 4 elements
        const int per = rw >> 2;
        for (int it = t; it < nr * per; it += RS_NT) {
            const int r = it / per, k = (it - r * per) << 2;
            float v[4];
            rs_ld4(sp + (long long)it * 4, v);
            float* d = tile + r * pitch + k;
            d[0] = v[0]; d[1] = v[1]; d[2] = v[2]; d[3] = v[3];
        }
    } else {
        for (int e = t; e < nr * rw; e += RS_NT) {
            const int r = e / rw;
            tile[r * pitch + (e - r * rw)] = rs_ld(sp + e);
        }
    }
    __syncthreads();
    for (int wk = t; wk < nr * C; wk += RS_NT) {
        const int r = wk / C;
        rs_prefilter<int>(tile + r * pitch + (wk - r * C), C, a.n);
    }
    __syncthreads();
    const int ow = a.dn * C;
    float* op = out + row0 * ow;
    for (int e = t; e < nr * ow; e += RS_NT) {
        const int r = e / ow, rem = e - r * ow;
        const int o = rem / C, c = rem - o * C;
        int idx[4];
        float w[4];
        rs_coord(a, o, idx, w);
        op[e] = rs_taps<int>(tile + r * pitch + c, C, idx, w);
    }
}

// ---- axes 1 and 0: column `col` = (q, r) of a (Q, n, inner) view; buf is read, and filtered in place unless SHORT ----
template <bool FINAL, typename I>
__device__ __forceinline__ void rs_emit(const float* c, I s, float* o, long long inner, const RSAxis& a, float defval) {
    for (int k = 0; k < a.dn; ++k) {
        int idx[4];
        float w[4];
        const bool in = rs_coord(a, k, idx, w);
        const float v = rs_taps<I>(c, s, idx, w);
        o[k * inner] = (FINAL && !in) ? defval : v;
    }
}

template <bool FINAL, bool SHORT>
__global__ void __launch_bounds__(RS_NT) rs_cols_kernel(float* buf, float* __restrict__ out, long long cols, int inner, RSAxis a,
                                                        RSMask m) {
    __shared__ float lds[SHORT ? RS_SHORT * RS_NT : 1];
    const int t = threadIdx.x;
    const long long col = (long long)blockIdx.x * RS_NT + t;
    if (col >= cols) return;
    const long long q = col / inner, in_l = inner;
    const int r = (int)(col - q * inner);
    float* p = buf + q * a.n * in_l + r;
    float* o = out + q * a.dn * in_l + r;
    if constexpr (FINAL) {
        const int vox = r / m.C, oy = vox / m.a2.dn, ox = vox - oy * m.a2.dn;
        double x;
        if (!(rs_inside(m.a1, oy, x) && rs_inside(m.a2, ox, x))) {
            for (int k = 0; k < a.dn; ++k) o[k * in_l] = m.defval;
            return;
        }
    }
    if constexpr (SHORT) {
        float* c = lds + t;
        for (int k = 0; k < a.n; ++k) c[k * RS_NT] = p[k * in_l];
        rs_prefilter<int>(c, RS_NT, a.n);
        rs_emit<FINAL, int>(c, RS_NT, o, in_l, a, m.defval);
    } else {
        rs_prefilter<long long>(p, in_l, a.n);
        rs_emit<FINAL, long long>(p, in_l, o, in_l, a, m.defval);
    }
}

// ---- order 0 ----
template <typename T>
__global__ void __launch_bounds__(RS_NT) rs_nearest_kernel(const T* __restrict__ src, T* __restrict__ out, long long total, RSAxis a0,
                                                           RSAxis a1, RSAxis a2, int C, T defval) {
    for (long long e = (long long)blockIdx.x * RS_NT + threadIdx.x; e < total; e += (long long)gridDim.x * RS_NT) {
        long long v = e / C;
        const int c = (int)(e - v * C);
        const int ox = (int)(v % a2.dn); v /= a2.dn;
        const int oy = (int)(v % a1.dn); v /= a1.dn;
        const int oz = (int)(v % a0.dn);
        const long long b = v / a0.dn;
        double x0, x1, x2;
        const bool in0 = rs_inside(a0, oz, x0), in1 = rs_inside(a1, oy, x1), in2 = rs_inside(a2, ox, x2);
        T val = defval;
        if (in0 && in1 && in2) {
            const int iz = min(max((int)floor(x0 + 0.5), 0), a0.n - 1), iy = min(max((int)floor(x1 + 0.5), 0), a1.n - 1),
                      ix = min(max((int)floor(x2 + 0.5), 0), a2.n - 1);
            val = src[(((b * a0.n + iz) * a1.n + iy) * (long long)a2.n + ix) * C + c];
        }
        out[e] = val;
    }
}

// ---- host ----
static inline bool rs_al(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }
static inline long long rs_up4(long long v) { return (v + 3) & ~3ll; }

struct RSPlan { RSAxis a[3]; long long n1, n2, nout; };

// the checks both entry points share: M1_OK and the plan, or the status to return
static int rs_plan(const m1_resample_t* g, int B, int C, RSPlan& pl) {
    if (!g || B <= 0 || C <= 0) return M1_ERR_BAD_ARG;
    for (int k = 0; k < 3; ++k) {
        if (g->src[k] <= 0 || g->dst[k] <= 0 || g->first[k] < 0) return M1_ERR_BAD_ARG;
        if (!(g->step[k] > 0.0) || !(g->step[k] <= 1.7e308)) return M1_ERR_BAD_ARG;       // (NaN fails the first, +inf the second)
    }
    if (g->order != 0 && g->order != 3) return M1_ERR_UNSUPPORTED;
    if (C > RS_MAX_C) return M1_ERR_UNSUPPORTED;
    const long long lim = 1ll << 31, bc = (long long)B * C;
    for (int k = 0; k < 3; ++k) {
        if ((long long)g->first[k] + g->dst[k] > (1ll << 30)) return M1_ERR_UNSUPPORTED;   // (first + o stays an int)
        if (g->order == 3 && g->src[k] > RS_MAX_LINE) return M1_ERR_UNSUPPORTED;
        pl.a[k] = RSAxis{g->src[k], g->dst[k], g->first[k], 0, g->step[k]};
    }
    // element counts of the source, the volume after the pass over axis 2, after the pass over axis 1, and the output
    const long long s0 = g->src[0], s1 = g->src[1], s2 = g->src[2], d0 = g->dst[0], d1 = g->dst[1], d2 = g->dst[2];
    if (s0 * s1 * s2 >= lim || d0 * d1 * d2 >= lim || s0 * s1 * d2 >= lim || s0 * d1 * d2 >= lim) return M1_ERR_UNSUPPORTED;
    if (bc * s0 * s1 * s2 >= lim || bc * s0 * s1 * d2 >= lim || bc * s0 * d1 * d2 >= lim || bc * d0 * d1 * d2 >= lim)
        return M1_ERR_UNSUPPORTED;
    pl.n1 = bc * s0 * s1 * d2;
    pl.n2 = bc * s0 * d1 * d2;
    pl.nout = bc * d0 * d1 * d2;
    return M1_OK;
}

extern "C" size_t m1_resample_ws_bytes(const m1_resample_t* g, int B, int C) {
    RSPlan pl;
    if (rs_plan(g, B, C, pl) != M1_OK || g->order != 3) return 0;
    return (size_t)(rs_up4(pl.n1) + pl.n2) * sizeof(float);
}

template <typename S>
static void rs_rows_launch(const void* src, float* out, long long rows, int C, const RSAxis& a, hipStream_t st) {
    const int rw = a.n * C;
    const int pitch = rw + (((C - rw) % 32) + 32) % 32;                 // the smallest pitch >= rw that is C (mod 32)
    int R = RS_LDS_FLOATS / pitch;
    if (R > RS_ROWS) R = RS_ROWS;
    const long long ow = (long long)a.dn * C;                           // (the kernel's element index R * ow stays an int)
    if (R * ow >= (1ll << 31)) R = (int)(((1ll << 31) - 1) / ow);
    const dim3 grid((unsigned)cdiv_ll(rows, R)), block(RS_NT);
    if ((rw & 3) == 0 && rs_al(src, 4 * sizeof(S)))
        hipLaunchKernelGGL((rs_rows_kernel<S, true>), grid, block, 0, st, (const S*)src, out, rows, R, C, pitch, a);
    else
        hipLaunchKernelGGL((rs_rows_kernel<S, false>), grid, block, 0, st, (const S*)src, out, rows, R, C, pitch, a);
}

template <bool FINAL>
static void rs_cols_launch(float* buf, float* out, long long Q, long long inner, const RSAxis& a, const RSMask& m, hipStream_t st) {
    const long long cols = Q * inner;
    const dim3 grid((unsigned)cdiv_ll(cols, RS_NT)), block(RS_NT);
    if (a.n <= RS_SHORT) hipLaunchKernelGGL((rs_cols_kernel<FINAL, true>), grid, block, 0, st, buf, out, cols, (int)inner, a, m);
    else hipLaunchKernelGGL((rs_cols_kernel<FINAL, false>), grid, block, 0, st, buf, out, cols, (int)inner, a, m);
}

extern "C" int m1_resample(const void* src, int src_dtype, const m1_resample_t* g, int B, int C, void* out, int out_dtype, void* ws,
                           void* stream) {
    if (m1_debug_skip("resample")) return M1_OK;
    if (!src || !out) return M1_ERR_BAD_ARG;
    RSPlan pl;
    if (int rc = rs_plan(g, B, C, pl)) return rc;
    if (src_dtype != M1_RAW_F32 && src_dtype != M1_RAW_I16) return M1_ERR_UNSUPPORTED;
    if (out_dtype != (g->order == 3 ? (int)M1_RAW_F32 : src_dtype)) return M1_ERR_UNSUPPORTED;
    if (!rs_al(src, src_dtype == M1_RAW_I16 ? 2 : 4) || !rs_al(out, out_dtype == M1_RAW_I16 ? 2 : 4)) return M1_ERR_BAD_ARG;
    if (g->order == 3 && (!ws || !rs_al(ws, 16))) return M1_ERR_BAD_ARG;
    hipStream_t st = (hipStream_t)stream;
    const double sb = src_dtype == M1_RAW_I16 ? 2.0 : 4.0, nsrc = (double)B * C * g->src[0] * g->src[1] * (double)g->src[2];
    const RSAxis &a0 = pl.a[0], &a1 = pl.a[1], &a2 = pl.a[2];
    if (g->order == 0) {
        M1ProfScope ps("resample_nearest", 0.0, 2.0 * sb * (double)pl.nout, st);
        const dim3 grid(m1_grid_for(pl.nout, 1)), block(RS_NT);
        if (src_dtype == M1_RAW_I16)
            hipLaunchKernelGGL(rs_nearest_kernel<int16_t>, grid, block, 0, st, (const int16_t*)src, (int16_t*)out, pl.nout, a0, a1, a2, C,
                               (int16_t)g->defval);
        else
            hipLaunchKernelGGL(rs_nearest_kernel<float>, grid, block, 0, st, (const float*)src, (float*)out, pl.nout, a0, a1, a2, C,
                               g->defval);
        return m1_check_launch();
    }
    // each pass reads its input once and writes its output once
    M1ProfScope ps("resample", 0.0, sb * nsrc + 8.0 * (double)pl.n1 + 8.0 * (double)pl.n2 + 4.0 * (double)pl.nout, st);
    float* t1 = (float*)ws;
    float* t2 = t1 + rs_up4(pl.n1);
    const RSMask m{a1, a2, C, g->defval};
    const long long rows = (long long)B * a0.n * a1.n;
    if (src_dtype == M1_RAW_I16) rs_rows_launch<int16_t>(src, t1, rows, C, a2, st);
    else rs_rows_launch<float>(src, t1, rows, C, a2, st);
    rs_cols_launch<false>(t1, t2, (long long)B * a0.n, (long long)a2.dn * C, a1, m, st);
    rs_cols_launch<true>(t2, (float*)out, B, (long long)a1.dn * a2.dn * C, a0, m, st);
    return m1_check_launch();
}
