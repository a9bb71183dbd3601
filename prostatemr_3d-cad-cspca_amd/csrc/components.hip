// components.hip -- 3D connected-component labelling and the small kernels lesion extraction and matching are built from
// (detection.py is the public surface; the reference only imports skimage's regionprops and a compute_FROC that was never shipped).
// Volumes are (B, D, H, W), one value per voxel; n = D * H * W; B * n < 2^31 - 1, so that "global linear index + 1" is an int label.
//
//   m1_cc_label: foreground = src > threshold (strict; NaN is background).  Four ideas, six launches, no kernel waits for another
//     workgroup and every loop ends because a successful atomicMin strictly lowers a value:
//     cc_local_kernel    one workgroup per CC_TZ x CC_TY x CC_TX tile: union-find in LDS (atomicMin on LDS words); every foreground voxel
//                        then stores the GLOBAL linear index + 1 of its tile-local root into buffer P (plain stores: the kernel boundary
//                        publishes them).
//     cc_boundary_kernel every foreground voxel looks at those of its 13 "backward" neighbours (the half of the neighbourhood with the
//                        smaller linear index) that lie in ANOTHER tile and unites the two trees in P: find by agent-scope atomic loads,
//                        hook the larger root under the smaller by atomicMin.  Every access to P in this kernel is an agent-scope atomic
//                        (the XCDs' L2s are separate: a plain load may be stale).  A neighbour is addressed by (z, y, x), never by a
//                        linear index +- 1, so nothing crosses a row end, a slice end or a batch entry.
//     cc_flatten_kernel  every voxel follows its chain in P to the root and stores it to a SECOND buffer F (P is only read); the block
//                        also counts the roots (F[v] == v + 1) of its chunk of 1024 voxels.
//     cc_scan_kernel     one block per batch entry: exclusive scan of the chunk totals in chunk order, counts[b] = K_b.
//     cc_rank_kernel     block scan inside the chunk: root number r in raster order writes r + 1 at its own position of P.
//     cc_final_kernel    labels[v] = P[F[v] - 1].
//     The atomicMin root of a component is its smallest linear index, and its rank among the roots of its batch entry is the number
//     scipy.ndimage.label gives the component.  Integer atomics only: results are bitwise identical from run to run.
//   m1_cc_stats / m1_cc_overlap: integer atomics on a table the library zero-fills with a kernel; the value maximum and its position are
//     ONE 64-bit atomicMax on {order-preserving bits of the fp32 value, ~index}: the largest value, ties to the smallest index.
//   m1_cc_peak / m1_cc_select / m1_cc_take: one round of the dynamic extraction for the whole batch, its state in device memory.
#include <limits.h>
#include "common.h"

#define CC_NT 256
#define CC_TZ M1_CC_TILE_Z
#define CC_TY M1_CC_TILE_Y
#define CC_TX M1_CC_TILE_X
#define CC_TILE (CC_TZ * CC_TY * CC_TX)
#define CC_CHUNK 1024                 // voxels of one batch entry a block of the streaming kernels takes
#define CC_PEAK_BLOCKS 64             // partial maxima per batch entry at most

static_assert(CC_TX == 32 && CC_TY == 8 && CC_TZ == 4, "the tile index arithmetic below uses these as shifts");
static_assert(sizeof(m1_cc_row_t) == 64, "the row layout is part of the ABI");
static_assert(CC_CHUNK == 4 * CC_NT, "four voxels per thread");

typedef unsigned long long cc_u64;

__device__ __forceinline__ int cc_ld(int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// order-preserving 32-bit key of an fp32 value (-0.0 was folded into +0.0 by the caller) and its inverse
__device__ __forceinline__ unsigned cc_ord(float v) {
    const unsigned u = __float_as_uint(v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float cc_unord(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }
__device__ __forceinline__ cc_u64 cc_key(float v, unsigned idx) { return ((cc_u64)cc_ord(v + 0.f) << 32) | (cc_u64)(0xffffffffu - idx); }

// is (dz, dy, dx) in {-1, 0} x {-1, 0, 1}^2 a backward neighbour of the `conn`-neighbourhood?
__device__ __forceinline__ bool cc_backward(int dz, int dy, int dx, int conn) {
    if (!(dz < 0 || (dz == 0 && (dy < 0 || (dy == 0 && dx < 0))))) return false;
    return (dz != 0) + (dy != 0) + (dx != 0) <= conn;
}

// ---- (a) tile-local union-find in LDS: L[v] = parent (tile-local index, <= v) or -1 for background ----
__device__ __forceinline__ int cc_find_lds(volatile int* L, int a) {
    for (int p = L[a]; p != a; p = L[a]) a = p;
    return a;
}
__device__ __forceinline__ void cc_union_lds(int* L, int a, int b) {
    for (;;) {
        a = cc_find_lds(L, a);
        b = cc_find_lds(L, b);
        if (a == b) return;
        if (a < b) { const int s = a; a = b; b = s; }
        const int old = atomicMin(&L[a], b);             // a was a root when read: hook it under b
        if (old == a) return;
        a = old;                                        // somebody hooked a first: unite what it points to with b as well
    }
}

template <typename T>
__global__ void __launch_bounds__(CC_NT) cc_local_kernel(const T* __restrict__ src, float thr, const float* __restrict__ thr_dev,
                                                         int conn, int D, int H, int W, int nty, int ntx, int* __restrict__ P) {
    __shared__ int L[CC_TILE];
    const int t = threadIdx.x, b = blockIdx.y;
    int bt = blockIdx.x;
    const int x0 = (bt % ntx) * CC_TX; bt /= ntx;
    const int y0 = (bt % nty) * CC_TY, z0 = (bt / nty) * CC_TZ;
    const float th = thr_dev ? thr_dev[b] : thr;
    const long long base = (long long)b * D * H * W;
    for (int v = t; v < CC_TILE; v += CC_NT) {
        const int x = x0 + (v & 31), y = y0 + ((v >> 5) & 7), z = z0 + (v >> 8);
        bool fg = false;
        if (z < D && y < H && x < W) fg = (float)src[base + ((long long)z * H + y) * W + x] > th;
        L[v] = fg ? v : -1;
    }
    __syncthreads();
    for (int v = t; v < CC_TILE; v += CC_NT) {
        if (L[v] < 0) continue;
        const int lx = v & 31, ly = (v >> 5) & 7, lz = v >> 8;
#pragma unroll
        for (int dz = -1; dz <= 0; ++dz)
#pragma unroll
            for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
                for (int dx = -1; dx <= 1; ++dx) {
                    if (!cc_backward(dz, dy, dx, conn)) continue;
                    const int nz = lz + dz, ny = ly + dy, nx = lx + dx;
                    if (nz < 0 || ny < 0 || ny >= CC_TY || nx < 0 || nx >= CC_TX) continue;
                    const int nb = (nz * CC_TY + ny) * CC_TX + nx;
                    if (((volatile int*)L)[nb] >= 0) cc_union_lds(L, v, nb);
                }
    }
    __syncthreads();
    for (int v = t; v < CC_TILE; v += CC_NT) {
        const int x = x0 + (v & 31), y = y0 + ((v >> 5) & 7), z = z0 + (v >> 8);
        if (z >= D || y >= H || x >= W) continue;
        int lab = 0;
        if (L[v] >= 0) {
            const int r = cc_find_lds(L, v);
            lab = (int)(base + ((long long)(z0 + (r >> 8)) * H + (y0 + ((r >> 5) & 7))) * W + (x0 + (r & 31))) + 1;
        }
        P[base + ((long long)z * H + y) * W + x] = lab;
    }
}

// ---- (b) unions across tile faces, edges and corners: P[i] = label (global index + 1) of the parent of voxel i, 0 = background ----
__device__ __forceinline__ int cc_find_g(int* P, int a) {
    for (int p = cc_ld(P + a - 1); p != a; p = cc_ld(P + a - 1)) a = p;
    return a;
}
__device__ __forceinline__ void cc_union_g(int* P, int a, int b) {
    for (;;) {
        a = cc_find_g(P, a);
        b = cc_find_g(P, b);
        if (a == b) return;
        if (a < b) { const int s = a; a = b; b = s; }
        const int old = atomicMin(P + a - 1, b);
        if (old == a) return;
        a = old;
    }
}

__global__ void __launch_bounds__(CC_NT) cc_boundary_kernel(int* P, int conn, int D, int H, int W) {
    const int b = blockIdx.y;
    const long long n = (long long)D * H * W, base = (long long)b * n;
    for (int k = 0; k < 4; ++k) {
        const long long i = (long long)blockIdx.x * CC_CHUNK + k * CC_NT + threadIdx.x;
        if (i >= n) continue;
        const int x = (int)(i % W), y = (int)((i / W) % H), z = (int)(i / ((long long)W * H));
        // an interior voxel of a tile has no backward neighbour in another tile (dx = +1 is the one offset that looks forward in x)
        if ((z & (CC_TZ - 1)) != 0 && (y & (CC_TY - 1)) != 0 && (y & (CC_TY - 1)) != CC_TY - 1 && (x & (CC_TX - 1)) != 0 &&
            (x & (CC_TX - 1)) != CC_TX - 1)
            continue;
        if (cc_ld(P + base + i) == 0) continue;
#pragma unroll
        for (int dz = -1; dz <= 0; ++dz)
#pragma unroll
            for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
                for (int dx = -1; dx <= 1; ++dx) {
                    if (!cc_backward(dz, dy, dx, conn)) continue;
                    const int nz = z + dz, ny = y + dy, nx = x + dx;
                    if (nz < 0 || ny < 0 || ny >= H || nx < 0 || nx >= W) continue;
                    if ((nz >> 2) == (z >> 2) && (ny >> 3) == (y >> 3) && (nx >> 5) == (x >> 5)) continue;      // the local pass did it
                    const long long j = base + ((long long)nz * H + ny) * W + nx;
                    if (cc_ld(P + j) == 0) continue;
                    cc_union_g(P, (int)(base + i) + 1, (int)j + 1);
                }
    }
}

// sum of one int per thread over the block (every thread gets it); s: CC_NT ints of LDS
__device__ __forceinline__ int cc_excl_scan(int v, int* s, int t, int& total) {
    s[t] = v;
    __syncthreads();
    for (int o = 1; o < CC_NT; o <<= 1) {
        const int x = t >= o ? s[t - o] : 0;
        __syncthreads();
        s[t] += x;
        __syncthreads();
    }
    total = s[CC_NT - 1];
    const int incl = s[t];
    __syncthreads();
    return incl - v;
}

// ---- (c) F[v] = root of v; chunk_roots[b][chunk] = roots in the chunk ----
__global__ void __launch_bounds__(CC_NT) cc_flatten_kernel(const int* __restrict__ P, int* __restrict__ F, int* __restrict__ chunk_roots,
                                                           long long n) {
    __shared__ int s[CC_NT];
    const int t = threadIdx.x, b = blockIdx.y;
    const long long base = (long long)b * n;
    int mine = 0;
    for (int k = 0; k < 4; ++k) {
        const long long i = (long long)blockIdx.x * CC_CHUNK + k * CC_NT + t;
        if (i >= n) continue;
        int a = P[base + i];
        if (a != 0) {
            for (int p = P[a - 1]; p != a; p = P[a - 1]) a = p;
            mine += (a == (int)(base + i) + 1);
        }
        F[base + i] = a;
    }
    int total;
    cc_excl_scan(mine, s, t, total);
    if (t == 0) chunk_roots[(long long)b * gridDim.x + blockIdx.x] = total;
}

// ---- (d) ranks ----
__global__ void __launch_bounds__(CC_NT) cc_scan_kernel(int* __restrict__ chunk_roots, int nchunk, int* __restrict__ counts) {
    __shared__ int s[CC_NT];
    const int t = threadIdx.x;
    int* c = chunk_roots + (long long)blockIdx.x * nchunk;
    int carry = 0;
    for (int c0 = 0; c0 < nchunk; c0 += CC_NT) {
        const bool in = c0 + t < nchunk;
        int total;
        const int ex = cc_excl_scan(in ? c[c0 + t] : 0, s, t, total);
        if (in) c[c0 + t] = carry + ex;
        carry += total;
    }
    if (t == 0) counts[blockIdx.x] = carry;
}

__global__ void __launch_bounds__(CC_NT) cc_rank_kernel(const int* __restrict__ F, const int* __restrict__ chunk_off, int* __restrict__ R,
                                                        long long n) {
    __shared__ int s[CC_NT];
    const int t = threadIdx.x, b = blockIdx.y;
    const long long base = (long long)b * n, i0 = (long long)blockIdx.x * CC_CHUNK + t * 4;
    bool root[4];
    int mine = 0;
    for (int k = 0; k < 4; ++k) {
        root[k] = i0 + k < n && F[base + i0 + k] == (int)(base + i0 + k) + 1;
        mine += root[k];
    }
    int total;
    int r = chunk_off[(long long)b * gridDim.x + blockIdx.x] + cc_excl_scan(mine, s, t, total);
    for (int k = 0; k < 4; ++k)
        if (root[k]) R[base + i0 + k] = ++r;
}

__global__ void __launch_bounds__(CC_NT) cc_final_kernel(const int* __restrict__ F, const int* __restrict__ R, int* __restrict__ labels,
                                                         long long total) {
    for (long long e = (long long)blockIdx.x * CC_NT + threadIdx.x; e < total; e += (long long)gridDim.x * CC_NT) {
        const int f = F[e];
        labels[e] = f ? R[f - 1] : 0;
    }
}

// ---- tables ----
__global__ void __launch_bounds__(CC_NT) cc_fill_kernel(int* __restrict__ p, long long n, int v) {
    for (long long e = (long long)blockIdx.x * CC_NT + threadIdx.x; e < n; e += (long long)gridDim.x * CC_NT) p[e] = v;
}

__global__ void __launch_bounds__(CC_NT) cc_rows_init_kernel(m1_cc_row_t* __restrict__ rows, long long nrows) {
    for (long long e = (long long)blockIdx.x * CC_NT + threadIdx.x; e < nrows; e += (long long)gridDim.x * CC_NT) {
        m1_cc_row_t r;
        r.count = 0; r.vmax = 0.f; r.argmax = 0;
        for (int k = 0; k < 3; ++k) { r.lo[k] = INT_MAX; r.hi[k] = 0; r.sum[k] = 0; }
        rows[e] = r;
    }
}

// while the sums run, `argmax` holds the packed {value, ~index} key
__global__ void __launch_bounds__(CC_NT) cc_stats_kernel(const int* __restrict__ labels, const float* __restrict__ values,
                                                         m1_cc_row_t* rows, int K, int H, int W, long long n) {
    const int b = blockIdx.y;
    const long long base = (long long)b * n;
    for (int k = 0; k < 4; ++k) {
        const long long i = (long long)blockIdx.x * CC_CHUNK + k * CC_NT + threadIdx.x;
        if (i >= n) continue;
        const int l = labels[base + i];
        if (l <= 0 || l > K) continue;
        m1_cc_row_t* r = rows + ((long long)b * K + l - 1);
        const int c[3] = {(int)(i / ((long long)W * H)), (int)((i / W) % H), (int)(i % W)};
        atomicAdd(&r->count, 1);
        for (int a = 0; a < 3; ++a) {
            atomicMin(&r->lo[a], c[a]);
            atomicMax(&r->hi[a], c[a] + 1);
            atomicAdd((cc_u64*)&r->sum[a], (cc_u64)c[a]);
        }
        atomicMax((cc_u64*)&r->argmax, cc_key(values ? values[base + i] : 0.f, (unsigned)i));
    }
}

__global__ void __launch_bounds__(CC_NT) cc_rows_finish_kernel(m1_cc_row_t* __restrict__ rows, long long nrows) {
    for (long long e = (long long)blockIdx.x * CC_NT + threadIdx.x; e < nrows; e += (long long)gridDim.x * CC_NT) {
        m1_cc_row_t* r = rows + e;
        if (r->count == 0) {
            r->lo[0] = r->lo[1] = r->lo[2] = 0;
            continue;
        }
        const cc_u64 key = (cc_u64)r->argmax;
        r->vmax = cc_unord((unsigned)(key >> 32));
        r->argmax = (long long)(0xffffffffu - (unsigned)key);
    }
}

__global__ void __launch_bounds__(CC_NT) cc_overlap_kernel(const int* __restrict__ a, const int* __restrict__ bl, int* table, int Ka, int Kb,
                                                           long long n) {
    __shared__ int s[CC_NT];
    const int t = threadIdx.x, b = blockIdx.y;
    const long long base = (long long)b * n;
    int* tab = table + (long long)b * (Ka + 1) * (Kb + 1);
    int zeros = 0;                                       // most voxels are background in both: one atomic per block for those
    for (int k = 0; k < 4; ++k) {
        const long long i = (long long)blockIdx.x * CC_CHUNK + k * CC_NT + t;
        if (i >= n) continue;
        const int la = a[base + i], lb = bl[base + i];
        if (la < 0 || la > Ka || lb < 0 || lb > Kb) continue;
        if ((la | lb) == 0) ++zeros;
        else atomicAdd(tab + (long long)la * (Kb + 1) + lb, 1);
    }
    int total;
    cc_excl_scan(zeros, s, t, total);
    if (t == 0 && total) atomicAdd(tab, total);
}

// ---- the steps of the dynamic extraction; state word k of sample b is st[k * B + b] ----
__global__ void __launch_bounds__(CC_NT) cc_peak_partial_kernel(const float* __restrict__ w, long long n, cc_u64* __restrict__ part) {
    __shared__ cc_u64 s[CC_NT / 64];
    const int t = threadIdx.x, b = blockIdx.y;
    const float* p = w + (long long)b * n;
    cc_u64 best = 0;
    for (long long i = (long long)blockIdx.x * CC_NT + t; i < n; i += (long long)gridDim.x * CC_NT) {
        const cc_u64 key = cc_key(p[i], (unsigned)i);
        best = key > best ? key : best;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const cc_u64 other = __shfl_xor(best, o, 64);
        best = other > best ? other : best;
    }
    if ((t & 63) == 0) s[t >> 6] = best;
    __syncthreads();
    if (t == 0) {
        for (int k = 1; k < CC_NT / 64; ++k) best = s[k] > best ? s[k] : best;
        part[(long long)b * gridDim.x + blockIdx.x] = best;
    }
}

__global__ void cc_peak_fold_kernel(const cc_u64* __restrict__ part, int nblk, int B, float factor, float min_conf, int reset,
                                    int* __restrict__ st) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    cc_u64 best = 0;
    for (int k = 0; k < nblk; ++k) {
        const cc_u64 v = part[(long long)b * nblk + k];
        best = v > best ? v : best;
    }
    const float peak = cc_unord((unsigned)(best >> 32));
    float* stf = (float*)st;
    stf[M1_CC_ST_PEAK * B + b] = peak;
    st[M1_CC_ST_ARGMAX * B + b] = (int)(0xffffffffu - (unsigned)best);
    stf[M1_CC_ST_THRESHOLD * B + b] = __fdiv_rn(peak, factor);
    st[M1_CC_ST_SEL * B + b] = 0;
    st[M1_CC_ST_COUNT * B + b] = 0;
    if (reset) {
        st[M1_CC_ST_DONE * B + b] = 0;
        st[M1_CC_ST_NCAND * B + b] = 0;
        st[M1_CC_ST_SPARE * B + b] = 0;
    }
    if (!(peak > min_conf)) st[M1_CC_ST_DONE * B + b] = 1;
}

__global__ void cc_select_kernel(const int* __restrict__ labels, long long n, int B, int* __restrict__ st) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    int sel = 0;
    if (!st[M1_CC_ST_DONE * B + b]) {
        const int a = st[M1_CC_ST_ARGMAX * B + b];
        if (a >= 0 && a < n) sel = labels[(long long)b * n + a];
        if (sel <= 0) {                                  // the peak is not above its own threshold: nothing more can be taken
            sel = 0;
            st[M1_CC_ST_DONE * B + b] = 1;
        }
    }
    st[M1_CC_ST_SEL * B + b] = sel;
    st[M1_CC_ST_COUNT * B + b] = 0;
}

__global__ void __launch_bounds__(CC_NT) cc_select_count_kernel(const int* __restrict__ labels, long long n, int B, int* st) {
    __shared__ int s[CC_NT];
    const int t = threadIdx.x, b = blockIdx.y;
    const int sel = st[M1_CC_ST_SEL * B + b];
    if (sel == 0) return;                                // (uniform over the block)
    int mine = 0;
    for (int k = 0; k < 4; ++k) {
        const long long i = (long long)blockIdx.x * CC_CHUNK + k * CC_NT + t;
        if (i < n) mine += labels[(long long)b * n + i] == sel;
    }
    int total;
    cc_excl_scan(mine, s, t, total);
    if (t == 0 && total) atomicAdd(st + M1_CC_ST_COUNT * B + b, total);
}

__global__ void __launch_bounds__(CC_NT) cc_take_kernel(const int* __restrict__ labels, const int* __restrict__ st, const float* w_src,
                                                        float* w, float* __restrict__ det, int* __restrict__ cand, long long n, int B, int nmax,
                                                        int min_voxels, int reset) {
    const int b = blockIdx.y;
    const int sel = st[M1_CC_ST_SEL * B + b], ncand = reset ? 0 : st[M1_CC_ST_NCAND * B + b];
    const bool keep = sel != 0 && st[M1_CC_ST_COUNT * B + b] >= min_voxels && ncand < nmax;
    const float peak = ((const float*)st)[M1_CC_ST_PEAK * B + b];
    if (sel == 0 && !reset) return;
    for (int k = 0; k < 4; ++k) {
        const long long i = (long long)blockIdx.x * CC_CHUNK + k * CC_NT + threadIdx.x;
        if (i >= n) continue;
        const long long e = (long long)b * n + i;
        const bool m = sel != 0 && labels[e] == sel;
        if (reset || (m && keep)) {
            det[e] = (m && keep) ? peak : 0.f;
            cand[e] = (m && keep) ? ncand + 1 : 0;
        }
        if (reset && w_src) w[e] = m ? 0.f : w_src[e];
        else if (m) w[e] = 0.f;
    }
}

__global__ void cc_take_tail_kernel(int* __restrict__ st, float* __restrict__ conf, int B, int nmax, int min_voxels, int reset) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    int ncand = st[M1_CC_ST_NCAND * B + b];
    if (reset) {
        ncand = 0;
        for (int k = 0; k < nmax; ++k) conf[(long long)b * nmax + k] = 0.f;
    }
    if (st[M1_CC_ST_SEL * B + b] != 0 && st[M1_CC_ST_COUNT * B + b] >= min_voxels && ncand < nmax) {
        conf[(long long)b * nmax + ncand] = ((const float*)st)[M1_CC_ST_PEAK * B + b];
        ++ncand;
    }
    st[M1_CC_ST_NCAND * B + b] = ncand;
}

// candidates of a fixed threshold: map[b][l - 1] = candidate number of component l (0 = dropped), conf[b][c - 1] = its maximum
__global__ void cc_relabel_map_kernel(const m1_cc_row_t* __restrict__ rows, int B, int K, int min_voxels, int* __restrict__ map,
                                      float* __restrict__ conf, int* __restrict__ ncand) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    int c = 0;
    for (int k = 0; k < K; ++k) {
        const m1_cc_row_t* r = rows + (long long)b * K + k;
        const bool keep = r->count >= min_voxels && r->count > 0;
        map[(long long)b * K + k] = keep ? c + 1 : 0;
        if (keep) conf[(long long)b * K + c++] = r->vmax;
    }
    for (int k = c; k < K; ++k) conf[(long long)b * K + k] = 0.f;
    ncand[b] = c;
}

__global__ void __launch_bounds__(CC_NT) cc_relabel_kernel(const int* __restrict__ labels, const m1_cc_row_t* __restrict__ rows,
                                                           const int* __restrict__ map, float* __restrict__ det, int* __restrict__ cand,
                                                           long long n, int K) {
    const int b = blockIdx.y;
    for (int k = 0; k < 4; ++k) {
        const long long i = (long long)blockIdx.x * CC_CHUNK + k * CC_NT + threadIdx.x;
        if (i >= n) continue;
        const long long e = (long long)b * n + i;
        const int l = labels[e];
        const int c = (l > 0 && l <= K) ? map[(long long)b * K + l - 1] : 0;
        cand[e] = c;
        det[e] = c ? rows[(long long)b * K + l - 1].vmax : 0.f;
    }
}

// ---- host ----
static inline bool cc_al(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }
static inline long long cc_up4(long long v) { return (v + 3) & ~3ll; }

struct CCPlan { long long n, total; int nchunk; };

// M1_OK and the plan, or the status to return
static int cc_plan(int B, int D, int H, int W, CCPlan& pl) {
    if (B <= 0 || D <= 0 || H <= 0 || W <= 0) return M1_ERR_BAD_ARG;
    pl.n = (long long)D * H * W;
    pl.total = pl.n * B;
    if (B > 65535 || pl.total >= (1ll << 31) - 1) return M1_ERR_UNSUPPORTED;
    pl.nchunk = (int)cdiv_ll(pl.n, CC_CHUNK);
    return M1_OK;
}
static int cc_plan_n(int B, long long n, CCPlan& pl) {
    if (B <= 0 || n <= 0) return M1_ERR_BAD_ARG;
    pl.n = n;
    pl.total = n * B;
    if (B > 65535 || n >= (1ll << 31) - 1 || pl.total >= (1ll << 31) - 1) return M1_ERR_UNSUPPORTED;
    pl.nchunk = (int)cdiv_ll(n, CC_CHUNK);
    return M1_OK;
}

// ws of m1_cc_label: P, F (total ints each, rounded to 16 bytes) and the chunk totals; m1_cc_peak uses the front of it
extern "C" size_t m1_cc_ws_bytes(int B, int D, int H, int W) {
    CCPlan pl;
    if (cc_plan(B, D, H, W, pl) != M1_OK) return 0;
    const long long label = (2 * cc_up4(pl.total) + cc_up4((long long)B * pl.nchunk)) * (long long)sizeof(int);
    const long long peak = (long long)B * CC_PEAK_BLOCKS * (long long)sizeof(cc_u64);
    return (size_t)(label > peak ? label : peak);
}

extern "C" int m1_cc_label(const void* src, int src_dtype, float threshold, const float* threshold_dev, int connectivity, int B, int D,
                           int H, int W, int* labels, int* counts, void* ws, void* stream) {
    if (m1_debug_skip("cc_label")) return M1_OK;
    if (!src || !labels || !counts || !ws) return M1_ERR_BAD_ARG;
    if (connectivity < 1 || connectivity > 3) return M1_ERR_BAD_ARG;
    CCPlan pl;
    if (int rc = cc_plan(B, D, H, W, pl)) return rc;
    if (src_dtype != M1_CC_F32 && src_dtype != M1_CC_U8) return M1_ERR_UNSUPPORTED;
    if (!cc_al(ws, 16) || !cc_al(labels, 4) || !cc_al(counts, 4) || !cc_al(threshold_dev, 4)) return M1_ERR_BAD_ARG;
    if (src_dtype == M1_CC_F32 && !cc_al(src, 4)) return M1_ERR_BAD_ARG;
    hipStream_t st = (hipStream_t)stream;
    M1ProfScope ps("cc_label", 0.0, (src_dtype == M1_CC_F32 ? 4.0 : 1.0) * (double)pl.total + 36.0 * (double)pl.total, st);
    int* P = (int*)ws;
    int* F = P + cc_up4(pl.total);
    int* chunks = F + cc_up4(pl.total);
    const int ntz = (D + CC_TZ - 1) / CC_TZ, nty = (H + CC_TY - 1) / CC_TY, ntx = (W + CC_TX - 1) / CC_TX;
    const long long ntiles = (long long)ntz * nty * ntx;
    if (ntiles >= (1ll << 31)) return M1_ERR_UNSUPPORTED;
    const dim3 block(CC_NT), tiles((unsigned)ntiles, (unsigned)B), chunked((unsigned)pl.nchunk, (unsigned)B);
    if (src_dtype == M1_CC_F32)
        hipLaunchKernelGGL(cc_local_kernel<float>, tiles, block, 0, st, (const float*)src, threshold, threshold_dev, connectivity, D, H, W,
                           nty, ntx, P);
    else
        hipLaunchKernelGGL(cc_local_kernel<uint8_t>, tiles, block, 0, st, (const uint8_t*)src, threshold, threshold_dev, connectivity, D,
                           H, W, nty, ntx, P);
    hipLaunchKernelGGL(cc_boundary_kernel, chunked, block, 0, st, P, connectivity, D, H, W);
    hipLaunchKernelGGL(cc_flatten_kernel, chunked, block, 0, st, (const int*)P, F, chunks, pl.n);
    hipLaunchKernelGGL(cc_scan_kernel, dim3((unsigned)B), block, 0, st, chunks, pl.nchunk, counts);
    hipLaunchKernelGGL(cc_rank_kernel, chunked, block, 0, st, (const int*)F, (const int*)chunks, P, pl.n);
    hipLaunchKernelGGL(cc_final_kernel, dim3(m1_grid_for(pl.total, 1)), block, 0, st, (const int*)F, (const int*)P, labels, pl.total);
    return m1_check_launch();
}

extern "C" int m1_cc_stats(const int* labels, const float* values, int B, int D, int H, int W, int max_components, m1_cc_row_t* rows,
                           void* stream) {
    if (m1_debug_skip("cc_stats")) return M1_OK;
    if (!labels || !rows || max_components <= 0) return M1_ERR_BAD_ARG;
    CCPlan pl;
    if (int rc = cc_plan(B, D, H, W, pl)) return rc;
    if (!cc_al(labels, 4) || !cc_al(values, 4) || !cc_al(rows, 8)) return M1_ERR_BAD_ARG;
    const long long nrows = (long long)B * max_components;
    if (nrows >= (1ll << 31)) return M1_ERR_UNSUPPORTED;
    hipStream_t st = (hipStream_t)stream;
    M1ProfScope ps("cc_stats", 0.0, (values ? 8.0 : 4.0) * (double)pl.total + 128.0 * (double)nrows, st);
    const dim3 block(CC_NT), rgrid(m1_grid_for(nrows, 1));
    hipLaunchKernelGGL(cc_rows_init_kernel, rgrid, block, 0, st, rows, nrows);
    hipLaunchKernelGGL(cc_stats_kernel, dim3((unsigned)pl.nchunk, (unsigned)B), block, 0, st, labels, values, rows, max_components, H, W,
                       pl.n);
    hipLaunchKernelGGL(cc_rows_finish_kernel, rgrid, block, 0, st, rows, nrows);
    return m1_check_launch();
}

extern "C" int m1_cc_overlap(const int* a, const int* b, int B, long long n, int max_a, int max_b, int* table, void* stream) {
    if (m1_debug_skip("cc_overlap")) return M1_OK;
    if (!a || !b || !table || max_a < 0 || max_b < 0) return M1_ERR_BAD_ARG;
    CCPlan pl;
    if (int rc = cc_plan_n(B, n, pl)) return rc;
    if (!cc_al(a, 4) || !cc_al(b, 4) || !cc_al(table, 4)) return M1_ERR_BAD_ARG;
    const long long cells = (long long)B * (max_a + 1ll) * (max_b + 1ll);
    if (cells >= (1ll << 31)) return M1_ERR_UNSUPPORTED;
    hipStream_t st = (hipStream_t)stream;
    M1ProfScope ps("cc_overlap", 0.0, 8.0 * (double)pl.total + 8.0 * (double)cells, st);
    const dim3 block(CC_NT);
    hipLaunchKernelGGL(cc_fill_kernel, dim3(m1_grid_for(cells, 1)), block, 0, st, table, cells, 0);
    hipLaunchKernelGGL(cc_overlap_kernel, dim3((unsigned)pl.nchunk, (unsigned)B), block, 0, st, a, b, table, max_a, max_b, pl.n);
    return m1_check_launch();
}

extern "C" int m1_cc_peak(const float* w, int B, long long n, float factor, float min_confidence, int reset, int* state, void* ws,
                          void* stream) {
    if (m1_debug_skip("cc_peak")) return M1_OK;
    if (!w || !state || !ws) return M1_ERR_BAD_ARG;
    CCPlan pl;
    if (int rc = cc_plan_n(B, n, pl)) return rc;
    if (!(factor > 0.f) || !cc_al(w, 4) || !cc_al(state, 4) || !cc_al(ws, 16)) return M1_ERR_BAD_ARG;
    hipStream_t st = (hipStream_t)stream;
    M1ProfScope ps("cc_peak", 0.0, 4.0 * (double)pl.total, st);
    const int nblk = (int)(cdiv_ll(n, CC_CHUNK) < CC_PEAK_BLOCKS ? cdiv_ll(n, CC_CHUNK) : CC_PEAK_BLOCKS);
    hipLaunchKernelGGL(cc_peak_partial_kernel, dim3((unsigned)nblk, (unsigned)B), dim3(CC_NT), 0, st, w, n, (cc_u64*)ws);
    hipLaunchKernelGGL(cc_peak_fold_kernel, dim3((unsigned)cdiv_ll(B, 64)), dim3(64), 0, st, (const cc_u64*)ws, nblk, B, factor,
                       min_confidence, reset, state);
    return m1_check_launch();
}

extern "C" int m1_cc_select(const int* labels, int B, long long n, int* state, void* stream) {
    if (m1_debug_skip("cc_select")) return M1_OK;
    if (!labels || !state) return M1_ERR_BAD_ARG;
    CCPlan pl;
    if (int rc = cc_plan_n(B, n, pl)) return rc;
    if (!cc_al(labels, 4) || !cc_al(state, 4)) return M1_ERR_BAD_ARG;
    hipStream_t st = (hipStream_t)stream;
    M1ProfScope ps("cc_select", 0.0, 4.0 * (double)pl.total, st);
    hipLaunchKernelGGL(cc_select_kernel, dim3((unsigned)cdiv_ll(B, 64)), dim3(64), 0, st, labels, n, B, state);
    hipLaunchKernelGGL(cc_select_count_kernel, dim3((unsigned)pl.nchunk, (unsigned)B), dim3(CC_NT), 0, st, labels, n, B, state);
    return m1_check_launch();
}

extern "C" int m1_cc_take(const int* labels, int* state, const float* w_src, float* w, float* detection_map, int* candidates, float* confidences, int B,
                          long long n, int max_candidates, int min_voxels, int reset, void* stream) {
    if (m1_debug_skip("cc_take")) return M1_OK;
    if (!labels || !state || !w || !detection_map || !candidates || !confidences || max_candidates <= 0) return M1_ERR_BAD_ARG;
    CCPlan pl;
    if (int rc = cc_plan_n(B, n, pl)) return rc;
    if (!cc_al(labels, 4) || !cc_al(state, 4) || !cc_al(w, 4) || !cc_al(w_src, 4) || !cc_al(detection_map, 4) || !cc_al(candidates, 4) ||
        !cc_al(confidences, 4))
        return M1_ERR_BAD_ARG;
    hipStream_t st = (hipStream_t)stream;
    M1ProfScope ps("cc_take", 0.0, 16.0 * (double)pl.total, st);
    hipLaunchKernelGGL(cc_take_kernel, dim3((unsigned)pl.nchunk, (unsigned)B), dim3(CC_NT), 0, st, labels, (const int*)state, w_src, w,
                       detection_map, candidates, n, B, max_candidates, min_voxels, reset);
    hipLaunchKernelGGL(cc_take_tail_kernel, dim3((unsigned)cdiv_ll(B, 64)), dim3(64), 0, st, state, confidences, B, max_candidates,
                       min_voxels, reset);
    return m1_check_launch();
}

extern "C" int m1_cc_relabel(const int* labels, const m1_cc_row_t* rows, int B, long long n, int max_components, int min_voxels, int* map,
                             float* detection_map, int* candidates, float* confidences, int* ncand, void* stream) {
    if (m1_debug_skip("cc_relabel")) return M1_OK;
    if (!labels || !rows || !map || !detection_map || !candidates || !confidences || !ncand || max_components <= 0) return M1_ERR_BAD_ARG;
    CCPlan pl;
    if (int rc = cc_plan_n(B, n, pl)) return rc;
    if (!cc_al(labels, 4) || !cc_al(rows, 8) || !cc_al(map, 4) || !cc_al(detection_map, 4) || !cc_al(candidates, 4) ||
        !cc_al(confidences, 4) || !cc_al(ncand, 4))
        return M1_ERR_BAD_ARG;
    hipStream_t st = (hipStream_t)stream;
    M1ProfScope ps("cc_relabel", 0.0, 12.0 * (double)pl.total, st);
    hipLaunchKernelGGL(cc_relabel_map_kernel, dim3((unsigned)cdiv_ll(B, 64)), dim3(64), 0, st, rows, B, max_components, min_voxels, map,
                       confidences, ncand);
    hipLaunchKernelGGL(cc_relabel_kernel, dim3((unsigned)pl.nchunk, (unsigned)B), dim3(CC_NT), 0, st, labels, rows, (const int*)map,
                       detection_map, candidates, n, max_components);
    return m1_check_launch();
}
