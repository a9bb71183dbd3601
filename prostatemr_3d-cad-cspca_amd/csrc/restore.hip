// restore.hip -- back-projection: a map on the network's grid (B, D, H, W, C) put back on the scan's own grid (B, d, h, w), the exact
// inverse of what preprocess.prepare_scan did (resampling to the network's spacing, then crop / pad to the network's size).
// m1_restore_t describes one axis by {n = dst: the scan's length, ratio = spacing / out_spacing, (first, count): the part of the
// resampled grid the crop kept, lo: the pad voxels in front on the network grid}: scan voxel i sits at the window coordinate
// u = i * ratio - first (fp64), is inside iff -0.5 <= u < count - 0.5 on every axis, and reads the real voxels [lo, lo + count) only --
// every tap is clamped to [0, count - 1] before lo is added, so a pad voxel of the network grid is never read.
//   order 1: taps floor(u), floor(u) + 1, weight y = fp32(u - floor(u)), one axis is a * (1 - y) + b * y, axes in the order 0, 1, 2:
//            preprocess.restore_host(dtype=np.float32) is this arithmetic written down (compiled without contraction).
//   order 0: a gather at floor(u + 0.5); the element type (fp32 / int16 / int32) is kept.
// ONE launch, no workspace.  The kernel is built around its stores (the scan-resolution output is what moves; the source stays in
// cache): a lane produces a run of RST_RUN = 4 consecutive voxels of the contiguous axis, i.e. 4 * nsel consecutive output elements,
// and stores them 4 elements at a time (16 bytes of fp32 / int32, 8 of int16) where the run is whole and starts on a multiple of 4 elements
// of an aligned pointer; the labels of a run are one 4-byte store under the same rule.  Runs at the end of a row and rows that start
// off that boundary (odd w * nsel) go element by element.  Work items (row, run) are dealt to threads in order, so a block of RST_NT
// threads covers at most RST_NT rows: the taps, weights and source offsets of axes 0 and 1 are uniform over a row and are computed
// once per row by the block's first threads into LDS; axis 2's are per lane.  Up to RST_MAX_SEL = 4 selected channels a lane keeps
// its run in registers (NS = nsel at compile time); wider selections (NS = -1) store every value as it is computed, element by element.
// Outputs, either or both, from one pass over the taps: prob = the channels [c0, c0 + nsel) of the restored map; label = the argmax
// over ALL C restored channels on the same values that would be stored (first maximum wins: strict >, channels in rising order).
#include "common.h"

#pragma clang fp contract(off)

#define RST_NT 256
#define RST_RUN 4
#define RST_MAX_SEL M1_RESTORE_MAX_SEL

struct RSTAxis { int n, count, first, lo; double ratio; };
// source element offsets of the rows (z0,y0), (z0,y1), (z1,y0), (z1,y1) of a scan row, and its weights on axes 0 and 1
struct RSTRow { int o[4]; float wz, wy; int inside; };

// taps (lo included) and weight of scan voxel i; false (and the taps of u = 0) where the coordinate is outside
template <int ORDER>
__device__ __forceinline__ bool rst_coord(const RSTAxis& a, int i, int& i0, int& i1, float& y) {
    double u = (double)i * a.ratio - (double)a.first;
    const bool in = u >= -0.5 && u < (double)a.count - 0.5;
    if (!in) u = 0.0;
    if constexpr (ORDER == 0) {
        i0 = i1 = min(max((int)floor(u + 0.5), 0), a.count - 1) + a.lo;
        y = 0.f;
    } else {
        const double fl = floor(u);
        const int f = (int)fl;
        y = (float)(u - fl);
        i0 = min(max(f, 0), a.count - 1) + a.lo;
        i1 = min(max(f + 1, 0), a.count - 1) + a.lo;
    }
    return in;
}

// channel c of one voxel: x0, x1 are the element offsets of axis 2's taps inside a source row
template <typename T, int ORDER>
__device__ __forceinline__ T rst_value(const T* __restrict__ src, const RSTRow& r, int x0, int x1, float wx, int c) {
    if constexpr (ORDER == 0) {
        return src[r.o[0] + x0 + c];
    } else {
        const float* p = src + c;
        const float uz = 1.f - r.wz, uy = 1.f - r.wy, ux = 1.f - wx;
        const float a00 = p[r.o[0] + x0] * uz + p[r.o[2] + x0] * r.wz;          // axis 0 at (y0, x0), (y1, x0), (y0, x1), (y1, x1)
        const float a10 = p[r.o[1] + x0] * uz + p[r.o[3] + x0] * r.wz;
        const float a01 = p[r.o[0] + x1] * uz + p[r.o[2] + x1] * r.wz;
        const float a11 = p[r.o[1] + x1] * uz + p[r.o[3] + x1] * r.wz;
        const float b0 = a00 * uy + a10 * r.wy;                                  // axis 1 at x0, x1
        const float b1 = a01 * uy + a11 * r.wy;
        return b0 * ux + b1 * wx;                                                // axis 2
    }
}

__device__ __forceinline__ void rst_st4(float* p, const float* v) { VecIO<float, 4>::st(p, v); }
__device__ __forceinline__ void rst_st4(int16_t* p, const int16_t* v) {
    uint2 w;
    w.x = (unsigned)(uint16_t)v[0] | ((unsigned)(uint16_t)v[1] << 16);
    w.y = (unsigned)(uint16_t)v[2] | ((unsigned)(uint16_t)v[3] << 16);
    *reinterpret_cast<uint2*>(p) = w;
}
__device__ __forceinline__ void rst_st4(int32_t* p, const int32_t* v) { *reinterpret_cast<int4*>(p) = make_int4(v[0], v[1], v[2], v[3]); }

// NS = the number of selected channels stored to prob (0: no prob output; -1: nsel of them, more than RST_MAX_SEL, by element stores);
// label may be NULL unless NS == 0
template <typename T, int ORDER, int NS>
__global__ void __launch_bounds__(RST_NT) rst_kernel(const T* __restrict__ src, T* __restrict__ prob, uint8_t* __restrict__ label,
                                                     int total, int nruns, int C, int c0, int nsel, RSTAxis a0, RSTAxis a1, RSTAxis a2,
                                                     int D, int H, int W, T defval, int deflabel, int vec_prob, int vec_label) {
    __shared__ RSTRow rowtab[RST_NT];
    const int t = threadIdx.x;
    // (items, rows and output voxels are below 2^31: m1_restore checks; 32-bit divisions)
    const int item0 = (int)blockIdx.x * RST_NT;
    const int row_first = item0 / nruns;
    const int item_last = item0 + min(RST_NT - 1, total - 1 - item0);           // (no sum beyond total - 1: total may be 2^31 - 1)
    const int nrow = item_last / nruns - row_first + 1;                         // <= RST_NT: items are dealt in order, nruns >= 1
    if (t < nrow) {
        const int row = row_first + t;
        const int q = row / a1.n;
        const int y = row - q * a1.n;
        const long long b = q / a0.n;
        const int z = q - (int)b * a0.n;
        int z0, z1, y0, y1;
        RSTRow r;
        const bool inz = rst_coord<ORDER>(a0, z, z0, z1, r.wz), iny = rst_coord<ORDER>(a1, y, y0, y1, r.wy);
        r.inside = inz && iny;
        const long long rw = (long long)W * C, bz = b * D;
        r.o[0] = (int)(((bz + z0) * H + y0) * rw);
        r.o[1] = (int)(((bz + z0) * H + y1) * rw);
        r.o[2] = (int)(((bz + z1) * H + y0) * rw);
        r.o[3] = (int)(((bz + z1) * H + y1) * rw);
        rowtab[t] = r;
    }
    __syncthreads();
    if (t > item_last - item0) return;
    const int item = item0 + t;
    const int row = item / nruns;
    const int xv = (item - row * nruns) * RST_RUN;
    const RSTRow r = rowtab[row - row_first];
    const int nx = min(RST_RUN, a2.n - xv);
    const bool want_label = label != nullptr;
    constexpr int NV = NS > 0 ? NS : 0;
    T vals[RST_RUN * (NV > 0 ? NV : 1)];
    unsigned labs = 0;
    const long long vox = (long long)row * a2.n + xv;
#pragma unroll
    for (int k = 0; k < RST_RUN; ++k) {
        int x0 = 0, x1 = 0, arg = deflabel;
        float wx = 0.f;
        const bool in = k < nx && r.inside && rst_coord<ORDER>(a2, xv + k, x0, x1, wx);
        if (in) {
            const int e0 = x0 * C, e1 = x1 * C;
            T best = defval;
            if constexpr (NS < 0) {
                const long long o = (vox + k) * nsel - c0;
                for (int c = want_label ? 0 : c0; c < (want_label ? C : c0 + nsel); ++c) {
                    const T v = rst_value<T, ORDER>(src, r, e0, e1, wx, c);
                    if (c >= c0 && c < c0 + nsel) prob[o + c] = v;
                    if (c == 0 || v > best) { best = v; arg = c; }
                }
            }
            if (NS >= 0 && want_label)
                for (int c = 0; c < c0; ++c) {
                    const T v = rst_value<T, ORDER>(src, r, e0, e1, wx, c);
                    if (c == 0 || v > best) { best = v; arg = c; }
                }
#pragma unroll
            for (int j = 0; j < NV; ++j) {
                const int c = c0 + j;
                const T v = rst_value<T, ORDER>(src, r, e0, e1, wx, c);
                vals[k * NV + j] = v;
                if (want_label && (c == 0 || v > best)) { best = v; arg = c; }
            }
            if (NS >= 0 && want_label)
                for (int c = c0 + NV; c < C; ++c) {
                    const T v = rst_value<T, ORDER>(src, r, e0, e1, wx, c);
                    if (c == 0 || v > best) { best = v; arg = c; }
                }
        } else {
#pragma unroll
            for (int j = 0; j < NV; ++j) vals[k * NV + j] = defval;
            if constexpr (NS < 0) {
                if (k < nx)
                    for (int j = 0; j < nsel; ++j) prob[(vox + k) * nsel + j] = defval;
            }
        }
        labs |= (unsigned)(arg & 0xff) << (8 * k);
    }
    if constexpr (NS > 0) {
        const long long e = vox * NS;
        if (nx == RST_RUN && vec_prob && (e & 3) == 0) {
#pragma unroll
            for (int j = 0; j < NS; ++j) rst_st4(prob + e + 4 * j, vals + 4 * j);
        } else {
#pragma unroll
            for (int k = 0; k < RST_RUN; ++k)
                if (k < nx) {
#pragma unroll
                    for (int j = 0; j < NS; ++j) prob[e + k * NS + j] = vals[k * NS + j];
                }
        }
    }
    if (want_label) {
        if (nx == RST_RUN && vec_label && (vox & 3) == 0) {
            *reinterpret_cast<unsigned*>(label + vox) = labs;
        } else {
#pragma unroll
            for (int k = 0; k < RST_RUN; ++k)
                if (k < nx) label[vox + k] = (uint8_t)(labs >> (8 * k));
        }
    }
}

// ---- host ----
static inline bool rst_al(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

template <typename T, int ORDER>
static void rst_launch(const void* src, void* prob, void* label, long long rows, int B, int C, int c0, int nsel, const m1_restore_t* g,
                       hipStream_t st) {
    RSTAxis a[3];
    for (int k = 0; k < 3; ++k) a[k] = RSTAxis{g->dst[k], g->count[k], g->first[k], g->lo[k], g->ratio[k]};
    const int nruns = (g->dst[2] + RST_RUN - 1) / RST_RUN;
    const int total = (int)(rows * nruns);                             // (nruns <= dst[2]: below 2^31 like the output's voxels)
    const dim3 grid((unsigned)cdiv_ll(total, RST_NT)), block(RST_NT);
    const int vec_prob = prob && rst_al(prob, 4 * sizeof(T)), vec_label = label && rst_al(label, 4);
    const T defval = (T)g->defval;
#define RST_GO(NS)                                                                                                                  \
    hipLaunchKernelGGL((rst_kernel<T, ORDER, NS>), grid, block, 0, st, (const T*)src, (T*)prob, (uint8_t*)label, total, nruns, C,   \
                       (NS) ? c0 : 0, nsel, a[0], a[1], a[2], g->src[0], g->src[1], g->src[2], defval, g->deflabel, vec_prob, vec_label)
    switch (prob ? nsel : 0) {
        case 0: RST_GO(0); break;
        case 1: RST_GO(1); break;
        case 2: RST_GO(2); break;
        case 3: RST_GO(3); break;
        case 4: RST_GO(4); break;
        default: RST_GO(-1); break;
    }
#undef RST_GO
}

extern "C" int m1_restore(const void* src, int src_dtype, const m1_restore_t* g, int B, int C, int c0, int nsel, void* prob,
                          void* label, void* stream) {
    if (m1_debug_skip("restore")) return M1_OK;
    if (!src || !g || (!prob && !label) || B <= 0 || C < 1) return M1_ERR_BAD_ARG;
    if (g->order != 0 && g->order != 1) return M1_ERR_BAD_ARG;
    if (src_dtype != M1_RAW_F32 && src_dtype != M1_RAW_I16 && src_dtype != M1_RAW_I32) return M1_ERR_UNSUPPORTED;
    if (src_dtype != M1_RAW_F32 && g->order == 1) return M1_ERR_BAD_ARG;
    for (int k = 0; k < 3; ++k) {
        if (g->src[k] <= 0 || g->dst[k] <= 0 || g->first[k] < 0 || g->count[k] <= 0 || g->lo[k] < 0) return M1_ERR_BAD_ARG;
        if ((long long)g->lo[k] + g->count[k] > g->src[k]) return M1_ERR_BAD_ARG;
        if (!(g->ratio[k] > 0.0) || !(g->ratio[k] <= 1.7e308)) return M1_ERR_BAD_ARG;      // (NaN fails the first, +inf the second)
    }
    if (prob && (c0 < 0 || nsel < 1 || (long long)c0 + nsel > C)) return M1_ERR_BAD_ARG;
    if (label && (C > 255 || g->deflabel < 0 || g->deflabel > 255)) return M1_ERR_BAD_ARG;
    const uintptr_t esz = src_dtype == M1_RAW_I16 ? 2 : 4;
    if (!rst_al(src, esz) || (prob && !rst_al(prob, esz))) return M1_ERR_BAD_ARG;
    // the source offsets are ints, the work items and the output voxels long long below 2^31
    const long long lim = 1ll << 31;
    const long long nsrc = (long long)g->src[0] * g->src[1], ndst = (long long)g->dst[0] * g->dst[1];
    if (nsrc >= lim || nsrc * g->src[2] >= lim || nsrc * g->src[2] * C >= lim || nsrc * g->src[2] * C * B >= lim) return M1_ERR_UNSUPPORTED;
    if (ndst >= lim || ndst * g->dst[2] >= lim || ndst * g->dst[2] * B >= lim) return M1_ERR_UNSUPPORTED;
    hipStream_t st = (hipStream_t)stream;
    const long long rows = ndst * B;
    const double nvox = (double)rows * g->dst[2];
    M1ProfScope ps("restore", 0.0, (double)esz * (double)nsrc * g->src[2] * C * B + nvox * ((prob ? (double)esz * nsel : 0.0) + (label ? 1.0 : 0.0)),
                   st);
    if (src_dtype == M1_RAW_I32) rst_launch<int32_t, 0>(src, prob, label, rows, B, C, c0, nsel, g, st);
    else if (src_dtype == M1_RAW_I16) rst_launch<int16_t, 0>(src, prob, label, rows, B, C, c0, nsel, g, st);
    else if (g->order == 0) rst_launch<float, 0>(src, prob, label, rows, B, C, c0, nsel, g, st);
    else rst_launch<float, 1>(src, prob, label, rows, B, C, c0, nsel, g, st);
    return m1_check_launch();
}
