// tile.hip -- sliding-window inference: cut a volume into overlapping tiles of the network's size (m1_tile_gather) and blend per-tile
// maps back onto the volume with a separable weight (m1_tile_blend).  include/m1hip.h states the contract; unets.networks.predict_tiled
// is the public surface, tiling.py the host side (origins, weights, fp64 restatements).
//
// Both are streaming kernels: a few integer divisions per 16 bytes moved, no LDS beyond the 48 origins, no scratch.  The geometry
// (m1_tile_t, 228 bytes) is a kernel argument.  A run-time index into a by-value argument struct would move the whole struct to scratch
// (tools/check_scratch.sh), so the prologue of each block copies the origins to LDS with constant indices and the kernels index that.
//
// m1_tile_blend's arithmetic is fixed by the header (products, sums and one IEEE division per tile, in ascending tile order), so this
// file is compiled without contraction: no product here may be fused into the sum that follows it.
#include "common.h"

#pragma clang fp contract(off)

struct TileOrigins { int o[3][M1_TILE_MAX_AXIS]; };

// origins of `g` -> LDS, axis 2 multiplied by `scale2` (the units of one voxel on that axis); every index into `g` is a constant
__device__ __forceinline__ void tile_stage_origins(const m1_tile_t& g, int scale2, TileOrigins& s) {
    if (threadIdx.x < 3 * M1_TILE_MAX_AXIS) {
        int v = 0;
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int k = 0; k < M1_TILE_MAX_AXIS; ++k)
                if ((int)threadIdx.x == a * M1_TILE_MAX_AXIS + k) v = g.origin[a][k];
        const int a = threadIdx.x / M1_TILE_MAX_AXIS;
        s.o[a][threadIdx.x % M1_TILE_MAX_AXIS] = a == 2 ? v * scale2 : v;
    }
    __syncthreads();
}

// The copy in units of UT (16-byte chunks of a tile's W row, or single elements): unit i of out is unit q of row (s, z, y), s = t * B + b;
// rowu / vrow: the units of a tile's and of the volume's W row, u2: the units of one voxel (0 < u2 only scales the axis-2 origins).
// Every index stays below 2^31: the launcher holds both tensors under 2^31 elements.
template <typename UT>
__global__ void __launch_bounds__(256) tile_gather_kernel(const UT* __restrict__ x, const m1_tile_t g, int B, int rowu, int vrow, int u2,
                                                          long long items, UT* __restrict__ out) {
    __shared__ TileOrigins org;
    tile_stage_origins(g, u2, org);
    const int t0 = g.tile[0], t1 = g.tile[1], n1 = g.n[1], n2 = g.n[2], V0 = g.vol[0], V1 = g.vol[1];
    for (long long ii = (long long)blockIdx.x * 256 + threadIdx.x; ii < items; ii += (long long)gridDim.x * 256) {
        const int i = (int)ii;
        int r = i / rowu;
        const int q = i - r * rowu;
        int p = r / t1;
        const int y = r - p * t1;
        const int s = p / t0, z = p - s * t0;
        const int t = s / B, b = s - t * B;
        const int i01 = t / n2, i2 = t - i01 * n2;
        const int i0 = i01 / n1, i1 = i01 - i0 * n1;
        const int src = ((b * V0 + org.o[0][i0] + z) * V1 + org.o[1][i1] + y) * vrow + org.o[2][i2] + q;
        out[i] = x[src];
    }
}

// One lane owns G consecutive voxels of a W row of `out` and CT of their channels starting at c0 (CT == C unless C > 4: then one
// channel per lane).  G > 1 only when G divides vol[2], tile[2] and every axis-2 origin: the G voxels then share their covering
// tiles and stay inside each of them.  VEC: G * CT is a multiple of 4 floats and every run starts 16-byte aligned.
// The covering tiles are walked twice in ascending t, (i0, i1, i2) nested: first W = sum w, then out = sum (w / W) * v.
template <int CT, int G, bool VEC>
__global__ void __launch_bounds__(256) tile_blend_kernel(const float* __restrict__ tiles, const m1_tile_t g, int B, int C,
                                                         const float* __restrict__ w0, const float* __restrict__ w1,
                                                         const float* __restrict__ w2, long long items, float* __restrict__ out) {
    __shared__ TileOrigins org;
    tile_stage_origins(g, 1, org);
    const int V0 = g.vol[0], V1 = g.vol[1], xg = g.vol[2] / G, t0 = g.tile[0], t1 = g.tile[1], t2 = g.tile[2];
    const int n0 = g.n[0], n1 = g.n[1], n2 = g.n[2], nblk = C / CT;
    constexpr int E = G * CT;
    for (long long ii = (long long)blockIdx.x * 256 + threadIdx.x; ii < items; ii += (long long)gridDim.x * 256) {
        const int i = (int)ii;
        const int vg = i / nblk, c0 = (i - vg * nblk) * CT;
        int r = vg / xg;
        const int x = (vg - r * xg) * G;
        int p = r / V1;
        const int y = r - p * V1;
        const int b = p / V0, z = p - b * V0;
        float W[G];
#pragma unroll
        for (int j = 0; j < G; ++j) W[j] = 0.f;
        for (int i0 = 0; i0 < n0; ++i0) {
            const int d0 = z - org.o[0][i0];
            if ((unsigned)d0 >= (unsigned)t0) continue;
            const float a = w0[d0];
            for (int i1 = 0; i1 < n1; ++i1) {
                const int d1 = y - org.o[1][i1];
                if ((unsigned)d1 >= (unsigned)t1) continue;
                const float ab = a * w1[d1];
                for (int i2 = 0; i2 < n2; ++i2) {
                    const int d2 = x - org.o[2][i2];
                    if ((unsigned)d2 >= (unsigned)t2) continue;
#pragma unroll
                    for (int j = 0; j < G; ++j) W[j] = W[j] + ab * w2[d2 + j];
                }
            }
        }
        float acc[E];
        bool first = true;
        for (int i0 = 0; i0 < n0; ++i0) {
            const int d0 = z - org.o[0][i0];
            if ((unsigned)d0 >= (unsigned)t0) continue;
            const float a = w0[d0];
            for (int i1 = 0; i1 < n1; ++i1) {
                const int d1 = y - org.o[1][i1];
                if ((unsigned)d1 >= (unsigned)t1) continue;
                const float ab = a * w1[d1];
                for (int i2 = 0; i2 < n2; ++i2) {
                    const int d2 = x - org.o[2][i2];
                    if ((unsigned)d2 >= (unsigned)t2) continue;
                    const int t = (i0 * n1 + i1) * n2 + i2;
                    const float* src = tiles + ((((t * B + b) * t0 + d0) * t1 + d1) * t2 + d2) * C + c0;
                    float v[E];
                    if constexpr (VEC) {
#pragma unroll
                        for (int k = 0; k < E / 4; ++k) VecIO<float, 4>::ld(src + 4 * k, v + 4 * k);
                    } else {
#pragma unroll
                        for (int j = 0; j < G; ++j)
#pragma unroll
                            for (int c = 0; c < CT; ++c) v[j * CT + c] = src[j * C + c];
                    }
#pragma unroll
                    for (int j = 0; j < G; ++j) {
                        const float f = (ab * w2[d2 + j]) / W[j];
#pragma unroll
                        for (int c = 0; c < CT; ++c) {
                            const float term = f * v[j * CT + c];
                            acc[j * CT + c] = first ? term : acc[j * CT + c] + term;
                        }
                    }
                    first = false;
                }
            }
        }
        float* dst = out + (((b * V0 + z) * V1 + y) * (xg * G) + x) * C + c0;
        if constexpr (VEC) {
#pragma unroll
            for (int k = 0; k < E / 4; ++k) VecIO<float, 4>::st(dst + 4 * k, acc + 4 * k);
        } else {
#pragma unroll
            for (int j = 0; j < G; ++j)
#pragma unroll
                for (int c = 0; c < CT; ++c) dst[j * C + c] = acc[j * CT + c];
        }
    }
}

static inline bool tile_al(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

// What both entry points refuse about the geometry, in the order the header lists it; *T, *tv, *vv: tiles, voxels of a tile and of the
// volume (doubles: three ints need not fit 63 bits)
static int tile_check(const m1_tile_t* g, int B, int C, double* T, double* tv, double* vv) {
    if (!g || B < 1 || C < 1) return M1_ERR_BAD_ARG;
    *T = *tv = *vv = 1.0;
    for (int a = 0; a < 3; ++a) {
        const int L = g->vol[a], t = g->tile[a], n = g->n[a];
        if (L < 1 || t < 1 || n < 1 || n > M1_TILE_MAX_AXIS) return M1_ERR_BAD_ARG;
        if (g->origin[a][0] != 0) return M1_ERR_BAD_ARG;                              // (the cover starts at 0)
        for (int k = 0; k < n; ++k) {
            const int o = g->origin[a][k];
            if (o < 0 || o > L - t) return M1_ERR_BAD_ARG;                            // (a tile that leaves the volume; L < t)
            if (k && (o <= g->origin[a][k - 1] || o > g->origin[a][k - 1] + t)) return M1_ERR_BAD_ARG;     // (order; a gap)
        }
        if (g->origin[a][n - 1] + t != L) return M1_ERR_BAD_ARG;                      // (the cover ends at L)
        *T *= n; *tv *= t; *vv *= L;
    }
    return M1_OK;
}

// every axis-2 origin, and both W extents, a multiple of m voxels
static bool tile_w_multiple(const m1_tile_t* g, int m) {
    if (g->vol[2] % m || g->tile[2] % m) return false;
    for (int k = 0; k < g->n[2]; ++k)
        if (g->origin[2][k] % m) return false;
    return true;
}

extern "C" int m1_tile_gather(const void* x, int B, int C, int dtype, const m1_tile_t* g, void* out, void* stream) {
    if (m1_debug_skip("tile_gather")) return M1_OK;
    double T, tv, vv;
    if (!x || !out) return M1_ERR_BAD_ARG;
    if (const int rc = tile_check(g, B, C, &T, &tv, &vv)) return rc;
    if (dtype != M1_F32 && dtype != M1_BF16) return M1_ERR_UNSUPPORTED;
    const int es = dtype == M1_BF16 ? 2 : 4;
    if (!tile_al(x, es) || !tile_al(out, es)) return M1_ERR_BAD_ARG;
    const double lim = 2147483648.0;
    if (T * B * tv * C >= lim || vv * B * C >= lim) return M1_ERR_UNSUPPORTED;
    const long long n_out = (long long)(T * B * tv * C);
    hipStream_t st = (hipStream_t)stream;
    M1ProfScope ps("tile_gather", 0.0, 2.0 * (double)n_out * es, st);
    const dim3 block(256);
    // 16-byte chunks: a voxel run of m = 16 / gcd(16, C * es) voxels is a whole number of chunks, so rows and origins must be multiples of m
    int m = 16, vb = C * es;
    { int a = 16, b = vb % 16; while (b) { const int r = a % b; a = b; b = r; } m = 16 / a; }
    if (tile_al(x, 16) && tile_al(out, 16) && tile_w_multiple(g, m)) {
        const int rowu = (int)((long long)g->tile[2] * vb / 16), vrow = (int)((long long)g->vol[2] * vb / 16);
        // (axis-2 origins in chunks: o * vb / 16 = (o / m) * (m * vb / 16))
        m1_tile_t gc = *g;
        for (int k = 0; k < gc.n[2]; ++k) gc.origin[2][k] = (int)((long long)gc.origin[2][k] * vb / 16);
        const long long items = n_out * es / 16;
        hipLaunchKernelGGL(tile_gather_kernel<uint4>, dim3(m1_grid_for(items, 1)), block, 0, st, (const uint4*)x, gc, B, rowu, vrow, 1, items,
                           (uint4*)out);
        return m1_check_launch();
    }
    const int rowu = g->tile[2] * C, vrow = g->vol[2] * C;
    const dim3 grid(m1_grid_for(n_out, 1));
    if (es == 4) hipLaunchKernelGGL(tile_gather_kernel<unsigned>, grid, block, 0, st, (const unsigned*)x, *g, B, rowu, vrow, C, n_out, (unsigned*)out);
    else hipLaunchKernelGGL(tile_gather_kernel<unsigned short>, grid, block, 0, st, (const unsigned short*)x, *g, B, rowu, vrow, C, n_out, (unsigned short*)out);
    return m1_check_launch();
}

template <int CT, int G>
static void tile_blend_launch(bool vec, const float* tiles, const m1_tile_t* g, int B, int C, const float* w, long long items, float* out,
                              hipStream_t st) {
    const float *w0 = w, *w1 = w0 + g->tile[0], *w2 = w1 + g->tile[1];
    const dim3 grid(m1_grid_for(items, 1)), block(256);
    if constexpr ((G * CT) % 4 == 0) {
        if (vec) {
            hipLaunchKernelGGL((tile_blend_kernel<CT, G, true>), grid, block, 0, st, tiles, *g, B, C, w0, w1, w2, items, out);
            return;
        }
    }
    hipLaunchKernelGGL((tile_blend_kernel<CT, 1, false>), grid, block, 0, st, tiles, *g, B, C, w0, w1, w2, items, out);
}

extern "C" int m1_tile_blend(const float* tiles, int B, int C, const m1_tile_t* g, const float* profile, float* out, void* stream) {
    if (m1_debug_skip("tile_blend")) return M1_OK;
    double T, tv, vv;
    if (!tiles || !profile || !out) return M1_ERR_BAD_ARG;
    if (const int rc = tile_check(g, B, C, &T, &tv, &vv)) return rc;
    if (!tile_al(tiles, 4) || !tile_al(profile, 4) || !tile_al(out, 4)) return M1_ERR_BAD_ARG;
    const double lim = 2147483648.0;
    if (T * B * tv * C >= lim || vv * B * C >= lim) return M1_ERR_UNSUPPORTED;
    const long long voxels = (long long)(vv * B);
    hipStream_t st = (hipStream_t)stream;
    M1ProfScope ps("tile_blend", 0.0, (T * B * tv + vv * B) * C * 4.0, st);
    // groups of G voxels = a whole number of 16-byte vectors: 4, 2, 4, 1 voxels for C = 1, 2, 3, 4; wider C: one element per lane
    const int G = C == 1 || C == 3 ? 4 : C == 2 ? 2 : 1;
    const bool vec = C <= 4 && tile_al(tiles, 16) && tile_al(out, 16) && tile_w_multiple(g, G);
    switch (C) {
        case 1: tile_blend_launch<1, 4>(vec, tiles, g, B, C, profile, vec ? voxels / 4 : voxels, out, st); break;
        case 2: tile_blend_launch<2, 2>(vec, tiles, g, B, C, profile, vec ? voxels / 2 : voxels, out, st); break;
        case 3: tile_blend_launch<3, 4>(vec, tiles, g, B, C, profile, vec ? voxels / 4 : voxels, out, st); break;
        case 4: tile_blend_launch<4, 1>(vec, tiles, g, B, C, profile, voxels, out, st); break;
        default: tile_blend_launch<1, 1>(false, tiles, g, B, C, profile, voxels * C, out, st); break;
    }
    return m1_check_launch();
}
