// wgrad_fold.hip -- the fold every weight-gradient kernel (wgrad_*.hip) ends in, and the process-wide queue of deferred work.
//
// * Every voxel split of a weight-gradient launch stores its partial tile into its own copy of the member's gradient block
//   (wgrad_fold.h: m1_wg_copies); tf_finish_* add the copies into dw / db in a fixed order -- no floating-point atomics.
// * Under m1_wgrad_defer the folds, and the bias column sums of the transposed convs (kernels in norm.hip), are queued and run in a
//   few batched launches by m1_wgrad_fold_pending: ONE queue, one mutex, one switch (the autograd engine calls the weight
//   gradients from its own thread).
#include "common.h"
#include "wgrad_fold.h"
#include <mutex>
#include <vector>

// R[idx(i)] += sum over the copies of Rx[copy][idx(i)] for the NT x CA x CB block of one concat member (+ its bias sums).
// A block owns EL consecutive elements; its 256/EL lane rows stride the copies, fold through LDS, and ONE lane adds the
// total into R -- fixed order, no atomics: the weight gradient of these layers is run-to-run deterministic.
struct TfFin { float* Rx; long long stride; int ncopies; float* R; int NT, CA, CB; long long RT, RSA; int a_off, b_off;
               float* bsum; long long rx_bias; int nb; int EL; int bias_serial; };
// (bodies take the block index / block count of THEIR fold, so that one launch can serve many folds: tf_finish_batch_kernel)
__device__ __forceinline__ void tf_fold_generic(const TfFin& f, unsigned vb, float* red) {
    const long long n = (long long)f.NT * f.CA * f.CB;
    const int e = threadIdx.x % f.EL, y = threadIdx.x / f.EL, YL = 256 / f.EL;
    const long long i = (long long)vb * f.EL + e;
    const long long idx = i;                              // the copies are compact: [tap][a][b] of this member, then CB bias sums
    float* dst = nullptr;
    if (i < n) {
        const int b = (int)(i % f.CB); const long long q = i / f.CB; const int a = (int)(q % f.CA), t = (int)(q / f.CA);
        dst = f.R + (long long)t * f.RT + (long long)(a + f.a_off) * f.RSA + b + f.b_off;
    } else if (i < n + f.nb) { dst = f.bsum + (i - n) + f.b_off; }
    float s = 0.f;
    if (dst) {
#pragma unroll 8
        for (int c = y; c < f.ncopies; c += YL) s += f.Rx[(long long)c * f.stride + idx];
    }
    red[threadIdx.x] = s;
    __syncthreads();
    if (y == 0 && dst) {
        for (int q = 1; q < YL; ++q) s += red[q * f.EL + e];
        *dst += s;
    }
}
__global__ void __launch_bounds__(256) tf_finish_kernel(TfFin f) {
    __shared__ float red[256];
    tf_fold_generic(f, blockIdx.x, red);
}

// Few copies of a large block (deep layers: 2..16 voxel splits of a multi-MB weight block): one thread folds 4 consecutive
// elements over all copies with 16-byte loads -- bandwidth-bound, where the kernel above (built for hundreds of copies of a
// small block) spends its time in 55k nearly empty blocks.  Same fixed order of additions.
__device__ __forceinline__ void tf_fold_vec(const TfFin& f, unsigned vb, unsigned nblk) {
    const long long n = (long long)f.NT * f.CA * f.CB, n4 = n >> 2;
    for (long long q = (long long)vb * 256 + threadIdx.x; q < n4; q += (long long)nblk * 256) {
        const long long i = q << 2;
        float4 s = *reinterpret_cast<const float4*>(f.Rx + i);
        for (int c = 1; c < f.ncopies; ++c) {
            const float4 v = *reinterpret_cast<const float4*>(f.Rx + (long long)c * f.stride + i);
            s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
        }
        const int b = (int)(i % f.CB); const long long r = i / f.CB; const int a = (int)(r % f.CA), t = (int)(r / f.CA);
        float* dst = f.R + (long long)t * f.RT + (long long)(a + f.a_off) * f.RSA + b + f.b_off;
        dst[0] += s.x; dst[1] += s.y; dst[2] += s.z; dst[3] += s.w;
    }
    if (vb == 0)
        for (int j = threadIdx.x; j < f.nb; j += 256) {
            float s = 0.f;
            for (int c = 0; c < f.ncopies; ++c) s += f.Rx[(long long)c * f.stride + n + j];
            f.bsum[j + f.b_off] += s;
        }
}
__global__ void __launch_bounds__(256) tf_finish_vec_kernel(TfFin f) { tf_fold_vec(f, blockIdx.x, gridDim.x); }

// Many copies (tens to hundreds of voxel splits): a block owns 256 consecutive elements, its 4 waves take every 4th copy with
// 16-byte loads (1 KB contiguous per wave and copy), fold through LDS in wave order, one store.  Fixed order, coalesced.
__device__ __forceinline__ void tf_fold_wide(const TfFin& f, unsigned vb, float4 (*red)[64]) {
    const long long n = (long long)f.NT * f.CA * f.CB;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const long long i = ((long long)vb * 64 + lane) << 2;
    float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
    if (i < n) {
#pragma unroll 4
        for (int c = w; c < f.ncopies; c += 4) {
            const float4 v = *reinterpret_cast<const float4*>(f.Rx + (long long)c * f.stride + i);
            s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
        }
    }
    red[w][lane] = s;
    __syncthreads();
    if (w == 0 && i < n) {
#pragma unroll
        for (int q = 1; q < 4; ++q) { const float4 v = red[q][lane]; s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w; }
        const int b = (int)(i % f.CB); const long long r = i / f.CB; const int a = (int)(r % f.CA), t = (int)(r / f.CA);
        float* dst = f.R + (long long)t * f.RT + (long long)(a + f.a_off) * f.RSA + b + f.b_off;
        dst[0] += s.x; dst[1] += s.y; dst[2] += s.z; dst[3] += s.w;
    }
    // bias sums (block 0 of the fold): the copies are spread over the lane rows -- 256 / nbp rows stride the copies with four loads in
    // flight, then fold through LDS in row order.  (Round 6: one thread per bias element used to walk ALL copies, 512 dependent loads
    // of a single block -- the tail of a batched launch of thousands of blocks, 100-160 us.)
    if (vb == 0 && f.bias_serial) {                        // (M1_TF_BIAS_SERIAL=1: the round-5 form, for A/B)
        for (int j = threadIdx.x; j < f.nb; j += 256) {
            float sb = 0.f;
            for (int c = 0; c < f.ncopies; ++c) sb += f.Rx[(long long)c * f.stride + n + j];
            f.bsum[j + f.b_off] += sb;
        }
    } else if (vb == 0 && f.nb > 0) {
        __syncthreads();                                   // (red is reused)
        float* const rb = reinterpret_cast<float*>(red);   // 256 floats
        int nbp = 1; while (nbp < f.nb && nbp < 256) nbp <<= 1;
        const int rows = 256 / nbp, j = threadIdx.x % nbp, r0 = threadIdx.x / nbp;
        for (int j0 = 0; j0 < f.nb; j0 += nbp) {
            float sb = 0.f;
            if (j0 + j < f.nb) {
#pragma unroll 4
                for (int c = r0; c < f.ncopies; c += rows) sb += f.Rx[(long long)c * f.stride + n + j0 + j];
            }
            rb[threadIdx.x] = sb;
            __syncthreads();
            if (r0 == 0 && j0 + j < f.nb) {
                for (int q = 1; q < rows; ++q) sb += rb[q * nbp + j];
                f.bsum[j0 + j + f.b_off] += sb;
            }
            __syncthreads();
        }
    }
}
__global__ void __launch_bounds__(256) tf_finish_wide_kernel(TfFin f) {
    __shared__ float4 red[4][64];
    tf_fold_wide(f, blockIdx.x, red);
}

// Many folds in one launch (m1_wgrad_defer / m1_wgrad_fold_pending): a fold of one conv member is 5-10 us of a few dozen blocks;
// ~130 of them per C3 step, each alone on its stream, were 4 % of the step.  The jobs travel by value in the kernel arguments.
#define TF_FOLD_MAX 24
struct TfFoldBatch { int n; int pref[TF_FOLD_MAX + 1]; int mode[TF_FOLD_MAX]; TfFin f[TF_FOLD_MAX]; };
static_assert(sizeof(TfFoldBatch) <= 3800, "fold batch must fit the kernel argument segment");
__global__ void __launch_bounds__(256) tf_finish_batch_kernel(TfFoldBatch B) {
    __shared__ float4 red[4][64];
    int j = 0;
    while (j + 1 < B.n && (int)blockIdx.x >= B.pref[j + 1]) ++j;
    const unsigned vb = blockIdx.x - B.pref[j], nblk = B.pref[j + 1] - B.pref[j];
    const TfFin& f = B.f[j];
    if (B.mode[j] == 1) tf_fold_vec(f, vb, nblk);
    else if (B.mode[j] == 2) tf_fold_wide(f, vb, red);
    else tf_fold_generic(f, vb, reinterpret_cast<float*>(red));
}

// ---- the deferred queue: folds and column sums, run by m1_wgrad_fold_pending -------------------------------------------------------
struct TfPending { TfFin f; int mode; int blocks; };
static std::mutex g_mu;
static int g_defer = 0;
static std::vector<TfPending> g_folds;
static std::vector<ColSumJob> g_sums[2];                // [bf16, fp32]
static void drop_locked() { g_folds.clear(); g_sums[0].clear(); g_sums[1].clear(); }
// fold batches of at most TF_FOLD_MAX jobs in queue order, then the bf16 column sums, then the fp32 ones; a failed launch clears
// what was queued
static int launch_locked(hipStream_t st) {
    int rc = M1_OK;
    for (size_t i = 0; i < g_folds.size() && rc == M1_OK;) {
        TfFoldBatch B{}; B.pref[0] = 0;
        while (i < g_folds.size() && B.n < TF_FOLD_MAX) {
            const TfPending& q = g_folds[i++];
            B.f[B.n] = q.f; B.mode[B.n] = q.mode; B.pref[B.n + 1] = B.pref[B.n] + q.blocks; ++B.n;
        }
        m1_note_plan("foldbatch:n=%d blocks=%d", B.n, B.pref[B.n]);
        hipLaunchKernelGGL(tf_finish_batch_kernel, dim3((unsigned)B.pref[B.n]), dim3(256), 0, st, B);
        rc = m1_check_launch();
    }
    for (int t = 0; t < 2; ++t)
        for (size_t i = 0; i < g_sums[t].size() && rc == M1_OK; i += CS_MAX) {
            const size_t n = g_sums[t].size() - i;
            rc = m1_colsum_launch_batch(&g_sums[t][i], (int)(n < CS_MAX ? n : CS_MAX), t == 0 ? M1_BF16 : M1_F32, st);
        }
    drop_locked();
    return rc;
}
int m1_fold_defer_set(int on) { std::lock_guard<std::mutex> lk(g_mu); const int was = g_defer; g_defer = on ? 1 : 0; return was; }
extern "C" int m1_wgrad_defer(int on) { m1_fold_defer_set(on); return M1_OK; }
extern "C" int m1_wgrad_fold_drop(void) { std::lock_guard<std::mutex> lk(g_mu); drop_locked(); return M1_OK; }
extern "C" int m1_wgrad_fold_pending(void* stream) {
    if (m1_debug_skip("fold")) return m1_wgrad_fold_drop();
    std::lock_guard<std::mutex> lk(g_mu);
    return launch_locked((hipStream_t)stream);
}

// true: queued (nothing launched); false: the caller runs the reduction now (deferral off, shape outside the batched kernel, or a
// second gradient into the same db while one is queued -- two read-modify-writes of db must not share a launch)
bool m1_colsum_defer(const void* x, int N, long long V, int C, int dtype, float* out, float* ws, int accumulate) {
    ColSumJob job;
    if (!M1_CFG("M1_BIAS_DEFER", 1) || !m1_colsum_job(x, N, V, C, dtype, out, ws, accumulate, &job)) return false;
    std::lock_guard<std::mutex> lk(g_mu);
    if (!g_defer) return false;
    for (const std::vector<ColSumJob>& v : g_sums)
        for (const ColSumJob& q : v) if (q.out == out) return false;
    g_sums[dtype == M1_BF16 ? 0 : 1].push_back(job);
    return true;
}

int m1_wg_rx_finish(float* rx, long long stride, int ncopies, const WgradSpec& g, long long nw, hipStream_t st) {
    TfFin f{rx, stride, ncopies, g.R, g.kd * g.kh * g.kw, g.CA, g.CB, g.RT, g.RSA, g.a_off, g.b_off, g.bsum, nw, g.bsum ? g.CB : 0, 32,
            M1_CFG("M1_TF_BIAS_SERIAL", 0)};
    const long long n = (long long)f.NT * f.CA * f.CB + f.nb;
    int mode = 0; long long blocks;
    if (ncopies <= 16 && f.CB % 4 == 0 && n >= (1 << 16)) {
        mode = 1; blocks = (n / 4 + 255) / 256; if (blocks > 4096) blocks = 4096;
    } else if (f.CB % 4 == 0 && n - f.nb >= (1 << 15)) {            // (n - nb) / 256 >= 128 blocks
        mode = 2; blocks = (n - f.nb + 255) / 256;
    } else {
        while (f.EL > 4 && n / f.EL < 128) f.EL >>= 1;           // small blocks of R: more lane rows per element, more blocks
        blocks = (n + f.EL - 1) / f.EL;
    }
    const char* const mname = mode == 1 ? "vec" : (mode == 2 ? "wide" : "generic");
    {
        std::lock_guard<std::mutex> lk(g_mu);
        if (g_defer) {
            // Two folds into the same block of R (a parameter used by two passes) must not share a launch (both read-modify-write
            // R).  The queue may hold folds whose partial copies were written on OTHER streams (SE shortcut / gate branches,
            // weight-gradient streams) that `st` is not ordered behind, so it is NOT flushed here: this fold runs now, on its own
            // stream, right behind the kernel that wrote its copies; the queued one follows at m1_wgrad_fold_pending, which the
            // caller issues on a stream that has joined every stream used since (ops.join_side_streams).
            bool dup = false;
            for (const TfPending& q : g_folds)
                if (q.f.R == f.R && q.f.a_off == f.a_off && q.f.b_off == f.b_off) { dup = true; break; }
            if (!dup) {
                g_folds.push_back(TfPending{f, mode, (int)blocks});
                m1_note_plan("fold:%s copies=%d n=%lld nb=%d el=%d queued", mname, ncopies, n, f.nb, f.EL);
                return M1_OK;
            }
        }
    }
    m1_note_plan("fold:%s copies=%d n=%lld nb=%d el=%d now", mname, ncopies, n, f.nb, f.EL);
    if (mode == 1) hipLaunchKernelGGL(tf_finish_vec_kernel, dim3((unsigned)blocks), dim3(256), 0, st, f);
    else if (mode == 2) hipLaunchKernelGGL(tf_finish_wide_kernel, dim3((unsigned)blocks), dim3(256), 0, st, f);
    else hipLaunchKernelGGL(tf_finish_kernel, dim3((unsigned)blocks), dim3(256), 0, st, f);
    return m1_check_launch();
}

int m1_wg_fold_members(float* rx, long long rx_mem, long long stride, int ncopies, const WgradSpec& g, long long nw, int nmem,
                       const int* a_offs, hipStream_t st) {
    for (int m = 0; m < nmem; ++m) {
        WgradSpec gm = g;
        if (nmem > 1) gm.a_off = a_offs[m];
        if (m) gm.bsum = nullptr;
        const int rc = m1_wg_rx_finish(rx + (long long)m * rx_mem, stride, ncopies, gm, nw, st); if (rc) return rc;
    }
    return M1_OK;
}
