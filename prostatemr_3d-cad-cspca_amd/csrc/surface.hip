// surface.hip -- surface-distance metrics of integer label maps with anisotropic voxel spacing: Hausdorff, percentile Hausdorff, average
// symmetric surface distance and normalised surface Dice per (batch entry, class) (surface_distance.py is the public surface; the
// reference imports an AnatomySegmentationValidation callback that was never published, so the definitions are pinned against
// scipy.ndimage in the tests).  Volumes are (B, D, H, W), n = D * H * W < 2^31; a slice is one (b, k) pair, S = B * K.
//
//   m1_sd_border  : sd_border_kernel  one launch over all (b, k): a thread reads its voxel and the six face neighbours of BOTH maps once
//                                     (addressed by (z, y, x): nothing crosses a volume face, a batch entry or a class slice; outside the
//                                     volume is background), writes the uint8 border masks of A = (pred == label) and B = (truth ==
//                                     label) and counts {border A, border B, |A|, |B|, |A and B|} by wave ballots into an LDS table;
//                                     the block stores its five counts per class.
//                   sd_count_fold_kernel  one block per (b, k) adds the blocks' counts (integers: exact in any order).
//   m1_sd_distance: exact Euclidean distance to the nearest non-zero voxel of every mask of a stack, three separable passes:
//                   sd_pass_w_kernel  one wave per row: the row as four 64-bit ballot words, the nearest set bit on either side by
//                                     clz / ffs -> |x - y| as uint16 (0xffff: no feature in the row).
//                   sd_pass_kernel    along H, then along D: f_out(x) = min_y ((s * (x - y))^2 + f_in(y)) in fp64 by brute force over
//                                     the line staged in LDS for SD_TC adjacent columns (+inf = no feature on the line); the pass
//                                     along H forms f_in = (s_w * |x - y|)^2 while staging, the pass along D stores (float)sqrt(f).
//   m1_sd_metrics : over the border voxels only, per slice and direction (0: border A against the distance to B, 1: the reverse):
//                   sd_stats_kernel / sd_stats_fold_kernel  count, fp64 sum, maximum and the counts <= tolerance: per-block partials
//                                     (fixed order inside a block: thread-sequential, wave shuffles, the four waves in order) folded in
//                                     block order.
//                   sd_hist_kernel / sd_scan_kernel  x 4: masked radix select on the fp32 bit pattern (non-negative floats order as
//                                     unsigned integers), 8 bits per pass, in the scheme of preprocess.hip: one 256-bin histogram per
//                                     group of ranks whose prefixes still agree; six ranks {k, min(k + 1, n - 1)} for the three
//                                     percentiles (directed 0, directed 1, pooled); the pooled histogram is the sum of the two directed
//                                     ones; the ranks come from the device-side counts in the first scan.  A scan block owns one
//                                     rank of one slice and the state has two copies, read and written in turn.
//                   sd_rows_kernel    the result rows, NaN rules included.
// No kernel waits for another workgroup, nothing synchronises with the host, every buffer that is read was written whole by an
// earlier kernel (no memset / memcpy nodes), and there are no atomics on global memory: results are bit-identical run to run.
// Compiled without contraction: the host restatement forms t * t + f with two roundings.
#include <math.h>
#include "common.h"

#pragma clang fp contract(off)

#define SD_NT 256
#define SD_MAX_K M1_SD_MAX_CLASSES
#define SD_MAX_T M1_SD_MAX_TOLERANCES
#define SD_MAX_LINE M1_SD_MAX_LINE
#define SD_CHUNK 1024                 // voxels of one batch entry a block of the border kernel takes
#define SD_TC 16                      // columns per block of the strided passes: 16 doubles = 128 B per staged row, 32 KB at L = 256
#define SD_CH 64                      // output positions of a line per block
#define SD_NONE 0xffffu               // pass W: no feature in the row
#define SD_MCHUNK 2048                // smallest chunk of a slice one block of the metric kernels takes
#define SD_MAX_BLK 64                 // blocks per slice and direction at most
#define SD_SCAN_Q 4                   // a scan block folds the blocks' histograms in this many interleaved parts
#define SD_UNROLL 4                   // elements a thread of the metric kernels has in flight
#define SD_NR 6                       // ranks selected side by side: {k, k + 1} x {directed 0, directed 1, pooled}

static_assert(SD_MAX_LINE == 4 * 64, "pass W holds a row in four ballot words");
static_assert(SD_CHUNK == 4 * SD_NT, "four voxels per thread");
static_assert(SD_MAX_LINE * SD_TC * sizeof(double) <= 48 * 1024, "the staged lines fit the default dynamic LDS");
static_assert(sizeof(m1_sd_row_t) == 160, "the row layout is part of the ABI");

typedef unsigned long long sd_u64;

struct SdLabels { int v[SD_MAX_K]; };
struct SdTol { float v[SD_MAX_T]; };

// ---- border masks and counts ----
template <typename T>
__device__ __forceinline__ int sd_at(const T* __restrict__ p, bool in, int z, int y, int x, int D, int H, int W, int& ok) {
    ok = in && z >= 0 && z < D && y >= 0 && y < H && x >= 0 && x < W;
    return ok ? (int)p[((long long)z * H + y) * W + x] : 0;
}

// part[((b * K + k) * nchunk + chunk) * 5 + {0..4}] = {border A, border B, |A|, |B|, |A and B|} of the chunk
template <typename T>
__global__ void __launch_bounds__(SD_NT) sd_border_kernel(const T* __restrict__ pred, const T* __restrict__ truth, SdLabels lab, int K,
                                                          int D, int H, int W, uint8_t* __restrict__ borders, int* __restrict__ part) {
    __shared__ int cnt[SD_MAX_K * 5];
    const int t = threadIdx.x, b = blockIdx.y, B = gridDim.y;
    const long long n = (long long)D * H * W;
    const T* p = pred + (long long)b * n;
    const T* q = truth + (long long)b * n;
    if (t < SD_MAX_K * 5) cnt[t] = 0;
    __syncthreads();
    for (int j = 0; j < 4; ++j) {                        // (no lane leaves the loop early: the ballots below are wave-wide)
        const long long i = (long long)blockIdx.x * SD_CHUNK + j * SD_NT + t;
        const bool in = i < n;
        const int x = (int)(i % W), y = (int)((i / W) % H), z = (int)(i / ((long long)W * H));
        int pv[7], qv[7], ok[7];
        const int dz[7] = {0, -1, 1, 0, 0, 0, 0}, dy[7] = {0, 0, 0, -1, 1, 0, 0}, dx[7] = {0, 0, 0, 0, 0, -1, 1};
#pragma unroll
        for (int m = 0; m < 7; ++m) {
            pv[m] = sd_at(p, in, z + dz[m], y + dy[m], x + dx[m], D, H, W, ok[m]);
            qv[m] = sd_at(q, in, z + dz[m], y + dy[m], x + dx[m], D, H, W, ok[m]);
        }
        for (int k = 0; k < K; ++k) {
            const int l = lab.v[k];
            const bool a = in && pv[0] == l, c = in && qv[0] == l;
            bool ia = a, ic = c;                          // interior: all six neighbours inside the volume and in the mask
#pragma unroll
            for (int m = 1; m < 7; ++m) {
                ia = ia && ok[m] && pv[m] == l;
                ic = ic && ok[m] && qv[m] == l;
            }
            const bool ba = a && !ia, bc = c && !ic;
            if (in) {
                borders[((long long)(0 * B + b) * K + k) * n + i] = ba ? 1 : 0;
                borders[((long long)(1 * B + b) * K + k) * n + i] = bc ? 1 : 0;
            }
            const int c0 = __popcll(__ballot(ba)), c1 = __popcll(__ballot(bc)), c2 = __popcll(__ballot(a)), c3 = __popcll(__ballot(c)),
                      c4 = __popcll(__ballot(a && c));
            if ((t & 63) == 0) {
                atomicAdd(&cnt[k * 5 + 0], c0); atomicAdd(&cnt[k * 5 + 1], c1); atomicAdd(&cnt[k * 5 + 2], c2);
                atomicAdd(&cnt[k * 5 + 3], c3); atomicAdd(&cnt[k * 5 + 4], c4);
            }
        }
    }
    __syncthreads();
    if (t < K * 5) part[(((long long)b * K + t / 5) * gridDim.x + blockIdx.x) * 5 + t % 5] = cnt[t];
}

// fixed-order block reduction: shuffles inside a wave, then the four wave results in wave order; sh: SD_NT / 64 values
template <typename V, typename OP>
__device__ __forceinline__ V sd_block_reduce(V v, V* sh, OP op) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = op(v, __shfl_xor(v, o, 64));
    __syncthreads();                                    // (sh may still be read from the previous call)
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    return op(op(op(sh[0], sh[1]), sh[2]), sh[3]);
}
struct SdAdd { template <typename V> __device__ __forceinline__ V operator()(V a, V b) const { return a + b; } };
struct SdMax { __device__ __forceinline__ float operator()(float a, float b) const { return fmaxf(a, b); } };

__global__ void __launch_bounds__(SD_NT) sd_count_fold_kernel(const int* __restrict__ part, int nchunk, long long* __restrict__ counts) {
    __shared__ long long sh[SD_NT / 64];
    const int* p = part + (long long)blockIdx.x * nchunk * 5;
    for (int j = 0; j < 5; ++j) {
        long long c = 0;
        for (int k = threadIdx.x; k < nchunk; k += SD_NT) c += p[(long long)k * 5 + j];
        c = sd_block_reduce(c, sh, SdAdd());
        if (threadIdx.x == 0) counts[(long long)blockIdx.x * 5 + j] = c;
    }
}

// ---- distance transform ----
// pass 1, along W: one wave per row
__global__ void __launch_bounds__(SD_NT) sd_pass_w_kernel(const uint8_t* __restrict__ mask, long long rows, int W,
                                                          unsigned short* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const long long row = (long long)blockIdx.x * (SD_NT / 64) + (threadIdx.x >> 6);
    if (row >= rows) return;                            // (uniform over the wave; the kernel has no barrier)
    const uint8_t* m = mask + row * W;
    sd_u64 bits[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const int x = c * 64 + lane;
        bits[c] = __ballot(x < W && m[x] != 0);
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const int x = c * 64 + lane;
        if (x >= W) continue;
        int left = -1, right = -1;                      // the nearest feature at or below x, at or above x
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const sd_u64 w = q < c ? bits[q] : (q == c ? bits[q] & ((2ull << lane) - 1ull) : 0ull);
            if (w) left = q * 64 + 63 - __clzll((long long)w);
        }
#pragma unroll
        for (int q = 3; q >= 0; --q) {
            const sd_u64 w = q > c ? bits[q] : (q == c ? bits[q] & (~0ull << lane) : 0ull);
            if (w) right = q * 64 + __ffsll((unsigned long long)w) - 1;
        }
        int d = (int)SD_NONE;
        if (left >= 0) d = x - left;
        if (right >= 0) d = min(d, right - x);
        out[row * W + x] = (unsigned short)d;
    }
}

__device__ __forceinline__ double sd_ld(const double* p, double) { return *p; }
__device__ __forceinline__ double sd_ld(const unsigned short* p, double s_prev) {
    const unsigned d = *p;
    if (d == SD_NONE) return INFINITY;
    const double t = s_prev * (double)d;
    return t * t;
}

// passes 2 and 3, along a strided axis: element (o, t, j) at (o * L + t) * inner + j, t the line position.  A block stages the whole
// line for SD_TC adjacent columns j and computes SD_CH output positions of them.  LAST: store (float)sqrt.
template <typename IN, bool LAST>
__global__ void __launch_bounds__(SD_NT) sd_pass_kernel(const IN* __restrict__ in, int L, long long inner, double s_prev, double s,
                                                        double* __restrict__ out, float* __restrict__ dist) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    double* line = (double*)smem;                        // [L][SD_TC]
    const long long ctiles = (inner + SD_TC - 1) / SD_TC;
    const int chunks = (L + SD_CH - 1) / SD_CH;
    long long b = blockIdx.x;
    const long long ct = b % ctiles; b /= ctiles;
    const int ch = (int)(b % chunks);
    const long long o = b / chunks;
    const int col = threadIdx.x & (SD_TC - 1), r0 = threadIdx.x / SD_TC;
    const long long j = ct * SD_TC + col;
    const bool cok = j < inner;
    const IN* src = in + o * L * inner + j;
    for (int t = r0; t < L; t += SD_NT / SD_TC) line[t * SD_TC + col] = cok ? sd_ld(src + (long long)t * inner, s_prev) : (double)INFINITY;
    __syncthreads();
    if (!cok) return;
    const int t1 = min(L, (ch + 1) * SD_CH);
    for (int x = ch * SD_CH + r0; x < t1; x += SD_NT / SD_TC) {
        double best = INFINITY;
        for (int y = 0; y < L; ++y) {
            const double t = s * (double)(x - y);
            best = fmin(best, t * t + line[y * SD_TC + col]);
        }
        const long long idx = (o * L + x) * inner + j;
        if (LAST) dist[idx] = (float)sqrt(best);
        else out[idx] = best;
    }
}

// ---- metrics ----
struct SdPart { double sum; long long cnt; long long le[SD_MAX_T]; float mx; float _pad; };
struct SdSel {                        // per slice, in ws; one copy is read and the other written by every scan (they alternate)
    unsigned prefix[SD_NR];           // key bits fixed so far of rank r (0 below the current digit); r = 2 * selection + {0, 1}
    unsigned krem[SD_NR];             // rank r among the elements that share its prefix
    double w[3];                      // interpolation weight h - floor(h) of each selection
};

// the distinct prefixes of the six ranks in order of first appearance (one histogram each) and the group of every rank; returns their
// number.  The histogram and the scan kernels derive the same grouping from the same state.
__device__ __forceinline__ int sd_groups(const unsigned* prefix, unsigned* gprefix, int* qgroup) {
    int ng = 0;
    for (int r = 0; r < SD_NR; ++r) {
        int f = -1;
        for (int k = 0; k < ng; ++k) f = gprefix[k] == prefix[r] ? k : f;
        if (f < 0) { f = ng; gprefix[ng++] = prefix[r]; }
        qgroup[r] = f;
    }
    return ng;
}

// slice s, direction dir: the border voxels of stack dir against the distances to the border of stack 1 - dir
__device__ __forceinline__ const uint8_t* sd_mask_of(const uint8_t* borders, int S, int s, int dir, long long n) {
    return borders + ((long long)dir * S + s) * n;
}
__device__ __forceinline__ const float* sd_val_of(const float* dist, int S, int s, int dir, long long n) {
    return dist + ((long long)(1 - dir) * S + s) * n;
}

// SD_UNROLL mask bytes and distances of one thread, SD_NT apart, all loads issued before the first use (the distance is loaded whether
// the voxel is a border voxel or not: no load waits for another); past the end of the chunk: not a border voxel
__device__ __forceinline__ void sd_fetch(const uint8_t* __restrict__ m, const float* __restrict__ v, int i, int i1, uint8_t* on, float* d) {
#pragma unroll
    for (int u = 0; u < SD_UNROLL; ++u) {
        const int e = i + u * SD_NT;
        on[u] = e < i1 ? m[e] : (uint8_t)0;
        d[u] = e < i1 ? v[e] : 0.f;
    }
}

// grid (nblk, S, 2); part[(s * 2 + dir) * nblk + blk]
__global__ void __launch_bounds__(SD_NT) sd_stats_kernel(const uint8_t* __restrict__ borders, const float* __restrict__ dist, int n,
                                                         int chunk, SdTol tol, int T, SdPart* __restrict__ part) {
    __shared__ double shd[SD_NT / 64];
    __shared__ long long shl[SD_NT / 64];
    __shared__ float shf[SD_NT / 64];
    const int t = threadIdx.x, s = blockIdx.y, dir = blockIdx.z, S = gridDim.y;
    const uint8_t* m = sd_mask_of(borders, S, s, dir, n);
    const float* v = sd_val_of(dist, S, s, dir, n);
    const int i0 = (int)min((long long)blockIdx.x * chunk, (long long)n), i1 = (int)min((long long)i0 + chunk, (long long)n);
    double sum = 0.0;
    long long cnt = 0, le[SD_MAX_T] = {0, 0, 0, 0};
    float mx = 0.f;
    for (int i = i0 + t; i < i1; i += SD_UNROLL * SD_NT) {
        uint8_t on[SD_UNROLL];
        float d[SD_UNROLL];
        sd_fetch(m, v, i, i1, on, d);
#pragma unroll
        for (int u = 0; u < SD_UNROLL; ++u) {
            if (!on[u]) continue;
            sum += (double)d[u];
            ++cnt;
            mx = fmaxf(mx, d[u]);
#pragma unroll
            for (int k = 0; k < SD_MAX_T; ++k) le[k] += (k < T && d[u] <= tol.v[k]) ? 1 : 0;
        }
    }
    SdPart r;
    r.sum = sd_block_reduce(sum, shd, SdAdd());
    r.cnt = sd_block_reduce(cnt, shl, SdAdd());
#pragma unroll
    for (int k = 0; k < SD_MAX_T; ++k) r.le[k] = sd_block_reduce(le[k], shl, SdAdd());
    r.mx = sd_block_reduce(mx, shf, SdMax());
    r._pad = 0.f;
    if (t == 0) part[((long long)s * 2 + dir) * gridDim.x + blockIdx.x] = r;
}

// one thread per (slice, direction): the blocks' partials in block order into the row
__global__ void __launch_bounds__(64) sd_stats_fold_kernel(const SdPart* __restrict__ part, int S, int nblk, m1_sd_row_t* __restrict__ rows) {
    const int e = blockIdx.x * 64 + threadIdx.x;
    if (e >= 2 * S) return;
    const int s = e >> 1, dir = e & 1;
    SdPart a;
    a.sum = 0.0; a.cnt = 0; a.mx = 0.f;
    for (int k = 0; k < SD_MAX_T; ++k) a.le[k] = 0;
    for (int bk = 0; bk < nblk; ++bk) {
        const SdPart p = part[(long long)e * nblk + bk];
        a.sum += p.sum; a.cnt += p.cnt; a.mx = fmaxf(a.mx, p.mx);
        for (int k = 0; k < SD_MAX_T; ++k) a.le[k] += p.le[k];
    }
    m1_sd_row_t* r = rows + s;
    r->n[dir] = a.cnt;
    r->sum[dir] = a.sum;
    for (int k = 0; k < SD_MAX_T; ++k) r->le[dir][k] = a.le[k];
    if (dir == 0) r->hd_ab = a.mx;
    else r->hd_ba = a.mx;
}

// grid (nblk, S, 2); hist[(((s * 2 + dir) * nblk + blk) * SD_NR + group) * 256 + digit]; `state`: what the previous scan wrote
__global__ void __launch_bounds__(SD_NT) sd_hist_kernel(const uint8_t* __restrict__ borders, const float* __restrict__ dist, int n,
                                                        int chunk, int pass, const SdSel* __restrict__ state, unsigned* __restrict__ hist) {
    __shared__ unsigned h[SD_NR * 256];
    __shared__ unsigned gp[SD_NR];
    __shared__ int ngs;
    const int t = threadIdx.x, s = blockIdx.y, dir = blockIdx.z, S = gridDim.y;
    if (t == 0) {
        if (pass == 0) {
            gp[0] = 0u;
            ngs = 1;
        } else {
            unsigned pre[SD_NR], g[SD_NR];
            int qg[SD_NR];
            for (int r = 0; r < SD_NR; ++r) pre[r] = state[s].prefix[r];
            ngs = sd_groups(pre, g, qg);
            for (int k = 0; k < ngs; ++k) gp[k] = g[k];
        }
    }
    __syncthreads();
    const int ng = ngs;
    for (int i = t; i < ng * 256; i += SD_NT) h[i] = 0u;
    __syncthreads();
    const int shift = 24 - 8 * pass;
    const unsigned keep = pass == 0 ? 0u : (0xffffffffu << (shift + 8));
    const uint8_t* m = sd_mask_of(borders, S, s, dir, n);
    const float* v = sd_val_of(dist, S, s, dir, n);
    const int i0 = (int)min((long long)blockIdx.x * chunk, (long long)n), i1 = (int)min((long long)i0 + chunk, (long long)n);
    for (int i = i0 + t; i < i1; i += SD_UNROLL * SD_NT) {
        uint8_t on[SD_UNROLL];
        float d[SD_UNROLL];
        sd_fetch(m, v, i, i1, on, d);
#pragma unroll
        for (int u = 0; u < SD_UNROLL; ++u) {
            if (!on[u]) continue;
            const unsigned key = __float_as_uint(d[u]);
            const unsigned hi = key & keep;
            int grp = -1;
            for (int k = 0; k < ng; ++k) grp = gp[k] == hi ? k : grp;  // (the prefixes are distinct: at most one matches)
            if (grp >= 0) atomicAdd(&h[grp * 256 + (int)((key >> shift) & 255u)], 1u);
        }
    }
    __syncthreads();
    unsigned* dst = hist + ((((long long)s * 2 + dir) * gridDim.x + blockIdx.x) * SD_NR) * 256;
    for (int i = t; i < ng * 256; i += SD_NT) dst[i] = h[i];
}

// grid (S, SD_NR): one block per slice and rank, SD_SCAN_Q * 256 threads; thread (t, qd) adds digit t of every SD_SCAN_Q-th block's
// histogram, the quarters meet in LDS, the 256 counts are scanned and the rank moves into its bin.  Reads `in` (not at pass 0, where
// the ranks come from the counts in `rows`), writes rank r of `out`: no block reads what another block of the launch writes.
__global__ void __launch_bounds__(SD_NT * SD_SCAN_Q) sd_scan_kernel(const SdSel* __restrict__ in, SdSel* __restrict__ out,
                                                                    const unsigned* __restrict__ hist, int nblk, int pass, double q,
                                                                    const m1_sd_row_t* __restrict__ rows) {
    __shared__ unsigned fold[SD_SCAN_Q][SD_NT];
    __shared__ unsigned sc[2][SD_NT];
    __shared__ unsigned pre_s, krem_s, npre_s, nkrem_s;
    __shared__ int gi_s;
    __shared__ double w_s;
    const int t = threadIdx.x & (SD_NT - 1), qd = threadIdx.x / SD_NT, s = blockIdx.x, r = blockIdx.y, sel = r >> 1;
    if (threadIdx.x == 0) {
        if (pass == 0) {
            const long long n0 = rows[s].n[0], n1 = rows[s].n[1];
            const long long ns = sel == 0 ? n0 : (sel == 1 ? n1 : n0 + n1);
            long long lo = 0, up = 0;
            double w = 0.0;
            if (ns > 0) {
                const double h = ((double)(ns - 1) * q) / 100.0;
                lo = (long long)floor(h);
                lo = lo < 0 ? 0 : (lo > ns - 1 ? ns - 1 : lo);
                up = lo + 1 < ns ? lo + 1 : ns - 1;
                w = h - (double)lo;
            }
            pre_s = 0u; krem_s = (unsigned)((r & 1) ? up : lo); gi_s = 0; w_s = w;
        } else {
            unsigned pre[SD_NR], g[SD_NR];
            int qg[SD_NR];
            for (int k = 0; k < SD_NR; ++k) pre[k] = in[s].prefix[k];
            sd_groups(pre, g, qg);
            pre_s = pre[r]; krem_s = in[s].krem[r]; gi_s = qg[r]; w_s = in[s].w[sel];
        }
        npre_s = pre_s; nkrem_s = krem_s;
    }
    __syncthreads();
    const long long stride = (long long)SD_NR * 256;
    unsigned a0 = 0u, a1 = 0u, a2 = 0u, a3 = 0u;
    for (int dir = 0; dir < 2; ++dir) {
        if (sel != 2 && sel != dir) continue;            // the pooled histogram is the sum of the two directed ones
        const unsigned* p = hist + ((((long long)s * 2 + dir) * nblk) * SD_NR + gi_s) * 256 + t;
        int bk = qd;
        for (; bk + 3 * SD_SCAN_Q < nblk; bk += 4 * SD_SCAN_Q) {
            a0 += p[bk * stride]; a1 += p[(bk + SD_SCAN_Q) * stride];
            a2 += p[(bk + 2 * SD_SCAN_Q) * stride]; a3 += p[(bk + 3 * SD_SCAN_Q) * stride];
        }
        for (; bk < nblk; bk += SD_SCAN_Q) a0 += p[bk * stride];
    }
    fold[qd][t] = (a0 + a1) + (a2 + a3);
    __syncthreads();
    unsigned cnt = 0u;
#pragma unroll
    for (int k = 0; k < SD_SCAN_Q; ++k) cnt += fold[k][t];
    int w = 0;                                          // inclusive scan of the 256 counts (every quarter keeps the barriers)
    if (qd == 0) sc[0][t] = cnt;
    __syncthreads();
    for (int o = 1; o < SD_NT; o <<= 1) {
        if (qd == 0) sc[w ^ 1][t] = sc[w][t] + (t >= o ? sc[w][t - o] : 0u);
        w ^= 1;
        __syncthreads();
    }
    const unsigned incl = sc[w][t], excl = incl - cnt, k = krem_s;
    if (qd == 0 && k >= excl && k < incl) { npre_s = pre_s | ((unsigned)t << (24 - 8 * pass)); nkrem_s = k - excl; }
    __syncthreads();
    if (threadIdx.x != 0) return;
    out[s].prefix[r] = npre_s;
    out[s].krem[r] = nkrem_s;
    if ((r & 1) == 0) out[s].w[sel] = w_s;
}

// one thread per slice; counts (S, 5) may be NULL
__global__ void __launch_bounds__(64) sd_rows_kernel(const SdSel* __restrict__ state, const long long* __restrict__ counts, int S, int T,
                                                     m1_sd_row_t* __restrict__ rows) {
    const int s = blockIdx.x * 64 + threadIdx.x;
    if (s >= S) return;
    m1_sd_row_t* r = rows + s;
    const long long n0 = r->n[0], n1 = r->n[1];
    const float nan = __uint_as_float(0x7fc00000u);
    float pct[3];
    for (int sel = 0; sel < 3; ++sel) {
        const double a = (double)__uint_as_float(state[s].prefix[2 * sel]), b = (double)__uint_as_float(state[s].prefix[2 * sel + 1]);
        pct[sel] = (float)(a + state[s].w[sel] * (b - a));
    }
    if (n0 > 0 && n1 > 0) {
        const double m0 = r->sum[0] / (double)n0, m1 = r->sum[1] / (double)n1;
        r->hd = fmaxf(r->hd_ab, r->hd_ba);
        r->mean_ab = (float)m0; r->mean_ba = (float)m1;
        r->assd = (float)((m0 + m1) / 2.0);
        r->hdq_ab = pct[0]; r->hdq_ba = pct[1]; r->hdq = pct[2];
    } else {
        r->hd = r->hd_ab = r->hd_ba = r->assd = r->mean_ab = r->mean_ba = r->hdq = r->hdq_ab = r->hdq_ba = nan;
    }
    for (int k = 0; k < SD_MAX_T; ++k) {
        float v = nan;
        if (k < T) {
            if (n0 > 0 && n1 > 0) v = (float)((double)(r->le[0][k] + r->le[1][k]) / (double)(n0 + n1));
            else if (n0 == 0 && n1 == 0) v = 1.f;        // both surfaces empty: they agree
        }
        r->nsd[k] = v;
    }
    float dice = nan;
    if (counts) {
        const long long vp = counts[(long long)s * 5 + 2], vt = counts[(long long)s * 5 + 3], vb = counts[(long long)s * 5 + 4];
        if (vp + vt > 0) dice = (float)(2.0 * (double)vb / (double)(vp + vt));
    }
    r->dice = dice;
    r->_pad[0] = r->_pad[1] = 0.f;
}

// ---- host ----
static inline bool sd_al(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }
static inline size_t sd_up16(size_t v) { return (v + 15) & ~(size_t)15; }

struct SdPlan { long long n; int nchunk, nblk, chunk; };

// M1_OK and the plan for N stacked volumes, or the status to return
static int sd_plan(int N, int D, int H, int W, SdPlan& pl) {
    if (N <= 0 || D <= 0 || H <= 0 || W <= 0) return M1_ERR_BAD_ARG;
    pl.n = (long long)D * H * W;
    if (N > 65535 || pl.n >= (1ll << 31) - 1 || pl.n * N >= (1ll << 40)) return M1_ERR_UNSUPPORTED;
    pl.nchunk = (int)cdiv_ll(pl.n, SD_CHUNK);
    long long nb = cdiv_ll(pl.n, SD_MCHUNK);
    if (nb > SD_MAX_BLK) nb = SD_MAX_BLK;
    pl.chunk = (int)cdiv_ll(pl.n, nb);
    pl.nblk = (int)cdiv_ll(pl.n, pl.chunk);
    return M1_OK;
}

static size_t sd_metric_part_bytes(const SdPlan& pl, int S) { return sd_up16((size_t)S * 2 * pl.nblk * sizeof(SdPart)); }
static size_t sd_metric_state_bytes(int S) { return sd_up16((size_t)2 * S * sizeof(SdSel)); }
static size_t sd_metric_hist_bytes(const SdPlan& pl, int S) { return (size_t)S * 2 * pl.nblk * SD_NR * 256 * sizeof(unsigned); }

extern "C" size_t m1_sd_ws_bytes(int stage, int B, int K, int D, int H, int W) {
    SdPlan pl;
    if (stage == M1_SD_STAGE_DISTANCE) {
        if (sd_plan(B, D, H, W, pl) != M1_OK || D > SD_MAX_LINE || H > SD_MAX_LINE || W > SD_MAX_LINE) return 0;
        return sd_up16((size_t)B * pl.n * sizeof(unsigned short)) + (size_t)B * pl.n * sizeof(double);
    }
    if (K < 1 || K > SD_MAX_K || sd_plan(B, D, H, W, pl) != M1_OK || (long long)B * K * 2 > 65535) return 0;
    if (stage == M1_SD_STAGE_BORDER) return (size_t)B * K * pl.nchunk * 5 * sizeof(int);
    if (stage == M1_SD_STAGE_METRICS) return sd_metric_part_bytes(pl, B * K) + sd_metric_state_bytes(B * K) + sd_metric_hist_bytes(pl, B * K);
    return 0;
}

extern "C" int m1_sd_border(const void* pred, const void* truth, int dtype, const int* labels, int K, int B, int D, int H, int W,
                            uint8_t* borders, long long* counts, void* ws, void* stream) {
    if (m1_debug_skip("sd_border")) return M1_OK;
    if (!pred || !truth || !labels || !borders || !counts || !ws) return M1_ERR_BAD_ARG;
    if (K < 1 || K > SD_MAX_K) return M1_ERR_BAD_ARG;
    SdPlan pl;
    if (int rc = sd_plan(B, D, H, W, pl)) return rc;
    if (dtype != M1_SD_U8 && dtype != M1_SD_I32) return M1_ERR_UNSUPPORTED;
    if ((long long)B * K * 2 > 65535) return M1_ERR_UNSUPPORTED;
    const uintptr_t al = dtype == M1_SD_I32 ? 4 : 1;
    if (!sd_al(pred, al) || !sd_al(truth, al) || !sd_al(counts, 8) || !sd_al(ws, 4)) return M1_ERR_BAD_ARG;
    SdLabels lab;
    for (int k = 0; k < SD_MAX_K; ++k) lab.v[k] = k < K ? labels[k] : 0;
    hipStream_t st = (hipStream_t)stream;
    const double vox = (double)B * (double)pl.n;
    M1ProfScope ps("sd_border", 0.0, vox * (2.0 * (double)al + 2.0 * K), st);
    int* part = (int*)ws;
    const dim3 grid((unsigned)pl.nchunk, (unsigned)B), block(SD_NT);
    if (dtype == M1_SD_U8)
        hipLaunchKernelGGL(sd_border_kernel<uint8_t>, grid, block, 0, st, (const uint8_t*)pred, (const uint8_t*)truth, lab, K, D, H, W,
                           borders, part);
    else
        hipLaunchKernelGGL(sd_border_kernel<int>, grid, block, 0, st, (const int*)pred, (const int*)truth, lab, K, D, H, W, borders, part);
    hipLaunchKernelGGL(sd_count_fold_kernel, dim3((unsigned)(B * K)), block, 0, st, (const int*)part, pl.nchunk, counts);
    return m1_check_launch();
}

extern "C" int m1_sd_distance(const uint8_t* mask, int N, int D, int H, int W, const double* spacing, float* dist, void* ws,
                              void* stream) {
    if (m1_debug_skip("sd_distance")) return M1_OK;
    if (!mask || !spacing || !dist || !ws) return M1_ERR_BAD_ARG;
    for (int a = 0; a < 3; ++a)
        if (!(spacing[a] > 0.0) || !isfinite(spacing[a])) return M1_ERR_BAD_ARG;
    SdPlan pl;
    if (int rc = sd_plan(N, D, H, W, pl)) return rc;
    if (D > SD_MAX_LINE || H > SD_MAX_LINE || W > SD_MAX_LINE) return M1_ERR_UNSUPPORTED;
    if (!sd_al(dist, 4) || !sd_al(ws, 16)) return M1_ERR_BAD_ARG;
    const long long rows = (long long)N * D * H, in_d = (long long)H * W;
    const long long gw = cdiv_ll(rows, SD_NT / 64);
    const long long gh = (long long)N * D * cdiv_ll(H, SD_CH) * cdiv_ll(W, SD_TC);
    const long long gd = (long long)N * cdiv_ll(D, SD_CH) * cdiv_ll(in_d, SD_TC);
    if (gw > 0x7fffffffLL || gh > 0x7fffffffLL || gd > 0x7fffffffLL) return M1_ERR_UNSUPPORTED;
    hipStream_t st = (hipStream_t)stream;
    const double vox = (double)N * (double)pl.n;
    M1ProfScope ps("sd_distance", vox * 4.0 * ((double)H + (double)D), vox * (1.0 + 2.0 + 2.0 + 8.0 + 8.0 + 4.0), st);
    unsigned short* a = (unsigned short*)ws;
    double* b = (double*)((char*)ws + sd_up16((size_t)N * pl.n * sizeof(unsigned short)));
    const dim3 block(SD_NT);
    hipLaunchKernelGGL(sd_pass_w_kernel, dim3((unsigned)gw), block, 0, st, mask, rows, W, a);
    // along H: outer (n, d), inner w;  along D: outer n, inner (h, w)
    hipLaunchKernelGGL((sd_pass_kernel<unsigned short, false>), dim3((unsigned)gh), block, (size_t)H * SD_TC * sizeof(double), st,
                       (const unsigned short*)a, H, (long long)W, spacing[2], spacing[1], b, (float*)nullptr);
    hipLaunchKernelGGL((sd_pass_kernel<double, true>), dim3((unsigned)gd), block, (size_t)D * SD_TC * sizeof(double), st,
                       (const double*)b, D, in_d, 0.0, spacing[0], (double*)nullptr, dist);
    return m1_check_launch();
}

extern "C" int m1_sd_metrics(const uint8_t* borders, const float* dist, const long long* counts, int B, int K, int D, int H, int W,
                             double percentile, const float* tolerances, int T, m1_sd_row_t* rows, void* ws, void* stream) {
    if (m1_debug_skip("sd_metrics")) return M1_OK;
    if (!borders || !dist || !rows || !ws) return M1_ERR_BAD_ARG;
    if (K < 1 || K > SD_MAX_K || T < 0 || T > SD_MAX_T || (T > 0 && !tolerances)) return M1_ERR_BAD_ARG;
    if (!(percentile >= 0.0 && percentile <= 100.0)) return M1_ERR_BAD_ARG;
    SdPlan pl;
    if (int rc = sd_plan(B, D, H, W, pl)) return rc;
    const int S = B * K;
    if ((long long)S * 2 > 65535) return M1_ERR_UNSUPPORTED;
    if (!sd_al(dist, 4) || !sd_al(counts, 8) || !sd_al(rows, 8) || !sd_al(ws, 16)) return M1_ERR_BAD_ARG;
    SdTol tol;
    for (int k = 0; k < SD_MAX_T; ++k) {
        tol.v[k] = k < T ? tolerances[k] : 0.f;
        if (tol.v[k] != tol.v[k]) return M1_ERR_BAD_ARG;
    }
    hipStream_t st = (hipStream_t)stream;
    M1ProfScope ps("sd_metrics", 0.0, 5.0 * 2.0 * (double)S * (double)pl.n, st);
    SdPart* part = (SdPart*)ws;
    SdSel* state = (SdSel*)((char*)ws + sd_metric_part_bytes(pl, S));
    unsigned* hist = (unsigned*)((char*)state + sd_metric_state_bytes(S));
    const dim3 grid((unsigned)pl.nblk, (unsigned)S, 2u), block(SD_NT), small((unsigned)cdiv_ll(2 * S, 64)), b64(64);
    hipLaunchKernelGGL(sd_stats_kernel, grid, block, 0, st, borders, dist, (int)pl.n, pl.chunk, tol, T, part);
    hipLaunchKernelGGL(sd_stats_fold_kernel, small, b64, 0, st, (const SdPart*)part, S, pl.nblk, rows);
    for (int pass = 0; pass < 4; ++pass) {               // scan `pass` writes copy (pass & 1) of the state, the next pass reads it
        const SdSel* prev = state + (size_t)((pass + 1) & 1) * S;
        hipLaunchKernelGGL(sd_hist_kernel, grid, block, 0, st, borders, dist, (int)pl.n, pl.chunk, pass, prev, hist);
        hipLaunchKernelGGL(sd_scan_kernel, dim3((unsigned)S, SD_NR), dim3(SD_NT * SD_SCAN_Q), 0, st, prev, state + (size_t)(pass & 1) * S,
                           (const unsigned*)hist, pl.nblk, pass, percentile, (const m1_sd_row_t*)rows);
    }
    hipLaunchKernelGGL(sd_rows_kernel, small, b64, 0, st, (const SdSel*)(state + S), counts, S, T, rows);
    return m1_check_launch();
}
