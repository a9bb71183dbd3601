// mc.hip -- Monte-Carlo inference: mean and predictive entropy of n softmax draws of the detection head (the reference's
// --UNET_PROBA_ITER, train_model.py:72, with scipy.stats.entropy) without a per-draw probability tensor.
//   m1_mc_accum : one forward pass over R replicas of the batch -> sum_p (+)= sum_r softmax(logits_r)        (fp32, (B,V,nc))
//   m1_mc_finish: mean = sum_p / n, entropy = -sum_c mean_c ln(mean_c)
//   m1_mc_accum_u / m1_mc_finish_u: the same pass and the same finish with two more accumulators, sum_h (+)= sum_r H(p_r) and
//   sum_pp (+)= sum_r p_r^2, from the probabilities already in registers -> expected entropy (aleatoric), mutual information
//   (epistemic, entropy - expected entropy) and the per-class population variance.
//   m1_mc_accum_v: either pass over replicas that are mirrored views (test-time augmentation, see the block further down).
// There is one accumulate item, mc_accum_item<T, NC, G, U, V>, and one finish item, mc_finish_item<NC, G, U>: U adds the two extra
// sums, V reads a replica's group at mirrored coordinates, and every entry point above is an instantiation of them.
// Both stream: a thread owns G consecutive voxels (G*nc elements = nc 16-byte vectors of logits) through every replica, so the
// replica sum lives in registers and nothing is exchanged between threads (no atomics, no LDS).  The voxels behind the last whole
// group, and everything when a pointer or the replica stride is not 16-byte aligned, take the same code with G = 1.
// The softmax is head.hip's, operation for operation (max, expf(x - max), sum in class order, 1 / sum, product): a single draw
// equals m1_softmax_heads_fwd bit for bit.  The file is compiled without contraction (see augment.hip for why the __f*_rn
// intrinsics do not give that): each probability is rounded before it is added, which is what the tests' restatement counts.
#include "common.h"

#pragma clang fp contract(off)

template <int NC>
__device__ __forceinline__ void mc_softmax(float* v) {
    float m = -3.4e38f;
#pragma unroll
    for (int c = 0; c < NC; ++c) m = fmaxf(m, v[c]);
    float s = 0.f;
#pragma unroll
    for (int c = 0; c < NC; ++c) { v[c] = expf(v[c] - m); s += v[c]; }
    const float inv = 1.f / s;
#pragma unroll
    for (int c = 0; c < NC; ++c) v[c] = v[c] * inv;
}

// E consecutive floats: float4 accesses when the caller's group is a whole number of them (G > 1), element accesses otherwise
template <int E, bool VEC>
__device__ __forceinline__ void mc_ld(const float* p, float* o) {
    if constexpr (VEC) {
#pragma unroll
        for (int q = 0; q < E / 4; ++q) VecIO<float, 4>::ld(p + 4 * q, o + 4 * q);
    } else {
#pragma unroll
        for (int k = 0; k < E; ++k) o[k] = p[k];
    }
}
template <int E, bool VEC>
__device__ __forceinline__ void mc_st(float* p, const float* o) {
    if constexpr (VEC) {
#pragma unroll
        for (int q = 0; q < E / 4; ++q) VecIO<float, 4>::st(p + 4 * q, o + 4 * q);
    } else {
#pragma unroll
        for (int k = 0; k < E; ++k) p[k] = o[k];
    }
}

// Which terms -p ln(p) an entropy takes.  U = false is m1_mc_finish's form, p > 0: a term with p == 0 contributes exactly 0 (no
// 0 * -inf), and so does a NaN.  The *_u entry points take every p that is not <= 0: the same terms for every number, in the same
// order, and a NaN stays a NaN in the maps instead of reading as "certain".
template <bool U>
__device__ __forceinline__ bool mc_term(float p) { return U ? !(p <= 0.f) : (p > 0.f); }

// H(p) = -sum_c p_c ln(p_c) of one draw of one voxel, in mc_finish_item's operation order
template <int NC>
__device__ __forceinline__ float mc_draw_entropy(const float* p) {
    float a = 0.f;
#pragma unroll
    for (int c = 0; c < NC; ++c)
        if (mc_term<true>(p[c])) a = a - p[c] * logf(p[c]);
    return a;
}

// The G voxels from voxel v0 on, through every replica (rstride elements apart).  U: also sum_h (one value per voxel) and sum_pp
// (laid out as sum_p), every sum in the same association: replicas in replica order, then old + acc.
// V: the voxels are those of a (B, D, H, W) grid and replica r is a view mirrored by bits [3r, 3r + 3) of `flips` (bit 0: W, bit 1:
// H, bit 2: D), so its group is read at (b, d', h', w'), x' = extent - 1 - x where the bit is set.  That is all V changes: where
// replica r's group is read.  The callers keep a group inside one W row (G divides W), where it is one contiguous run; with a W
// mirror the run starts at W - G - w and its voxels are reversed in registers, the classes of a voxel staying in order.
template <typename T, int NC, int G, bool U, bool V>
__device__ __forceinline__ void mc_accum_item(const T* lg, long long rstride, int R, long long v0, float* sum_p, int accumulate,
                                              float* samples, float* sum_h, float* sum_pp, unsigned long long flips = 0, int D = 0,
                                              int H = 0, int W = 0) {
    constexpr int E = G * NC, LV = sizeof(T) == 2 ? 8 : 4;
    constexpr bool VEC = G > 1;
    const long long e0 = v0 * NC;
    long long b = 0;
    int d = 0, h = 0, w = 0;
    if constexpr (V) {                                                          // (v0 = ((b * D + d) * H + h) * W + w)
        const long long row = v0 / W, bd = row / H;
        w = (int)(v0 - row * W), h = (int)(row - bd * H);
        b = bd / D;
        d = (int)(bd - b * D);
    }
    float old[E], acc[E];
    float oldq[U ? E : 1], accq[U ? E : 1], oldh[U ? G : 1], acch[U ? G : 1];
    if (accumulate) mc_ld<E, VEC>(sum_p + e0, old);
    if constexpr (U) {
        if (accumulate) {
            mc_ld<E, VEC>(sum_pp + e0, oldq);
            mc_ld<G, VEC>(sum_h + v0, oldh);
        }
    }
    for (int r = 0; r < R; ++r) {
        unsigned m = 0;
        long long src = e0;                                                     // (where the group starts inside replica r)
        if constexpr (V) {
            m = (unsigned)(flips >> (3 * r)) & 7u;
            const int ds = (m & 4u) ? D - 1 - d : d, hs = (m & 2u) ? H - 1 - h : h, ws = (m & 1u) ? W - G - w : w;
            src = (((b * D + ds) * H + hs) * W + ws) * NC;
        }
        float v[E];
        const T* p = lg + (long long)r * rstride + src;
        if constexpr (VEC) {
#pragma unroll
            for (int q = 0; q < E / LV; ++q) VecIO<T, LV>::ld(p + q * LV, v + q * LV);
            if (m & 1u) {                                                       // (the run was read backwards: voxel g <-> G - 1 - g)
#pragma unroll
                for (int g = 0; g < G / 2; ++g) {
#pragma unroll
                    for (int c = 0; c < NC; ++c) {
                        const float t = v[g * NC + c];
                        v[g * NC + c] = v[(G - 1 - g) * NC + c];
                        v[(G - 1 - g) * NC + c] = t;
                    }
                }
            }
        } else {
#pragma unroll
            for (int k = 0; k < E; ++k) v[k] = Act<T>::ld(p + k);
        }
#pragma unroll
        for (int g = 0; g < G; ++g) mc_softmax<NC>(v + g * NC);
        if (samples) mc_st<E, VEC>(samples + (long long)r * rstride + e0, v);
        if (r == 0) {
#pragma unroll
            for (int k = 0; k < E; ++k) acc[k] = v[k];
        } else {
#pragma unroll
            for (int k = 0; k < E; ++k) acc[k] = acc[k] + v[k];
        }
        if constexpr (U) {
            float hh[G];
#pragma unroll
            for (int g = 0; g < G; ++g) hh[g] = mc_draw_entropy<NC>(v + g * NC);
#pragma unroll
            for (int k = 0; k < E; ++k) v[k] = v[k] * v[k];                  // (a rounded product: the file is not contracted)
            if (r == 0) {
#pragma unroll
                for (int k = 0; k < E; ++k) accq[k] = v[k];
#pragma unroll
                for (int g = 0; g < G; ++g) acch[g] = hh[g];
            } else {
#pragma unroll
                for (int k = 0; k < E; ++k) accq[k] = accq[k] + v[k];
#pragma unroll
                for (int g = 0; g < G; ++g) acch[g] = acch[g] + hh[g];
            }
        }
    }
    if (accumulate) {
#pragma unroll
        for (int k = 0; k < E; ++k) acc[k] = old[k] + acc[k];
    }
    mc_st<E, VEC>(sum_p + e0, acc);
    if constexpr (U) {
        if (accumulate) {
#pragma unroll
            for (int k = 0; k < E; ++k) accq[k] = oldq[k] + accq[k];
#pragma unroll
            for (int g = 0; g < G; ++g) acch[g] = oldh[g] + acch[g];
        }
        mc_st<E, VEC>(sum_pp + e0, accq);
        mc_st<G, VEC>(sum_h + v0, acch);
    }
}

// items [0, ngroups): whole groups of G voxels; items [ngroups, ngroups + ntail): the single voxels behind them.  M = B * V.
// (sum_h and sum_pp are null without U)
template <typename T, int NC, bool U>
__global__ void __launch_bounds__(256) mc_accum_kernel(const T* __restrict__ lg, int R, long long M, long long ngroups,
                                                       float* __restrict__ sum_p, float* __restrict__ sum_h,
                                                       float* __restrict__ sum_pp, int accumulate, float* __restrict__ samples) {
    constexpr int G = sizeof(T) == 2 ? 8 : 4;
    const long long items = ngroups + (M - ngroups * G), rstride = M * NC;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < items; i += (long long)gridDim.x * 256) {
        if (i < ngroups) mc_accum_item<T, NC, G, U, false>(lg, rstride, R, i * G, sum_p, accumulate, samples, sum_h, sum_pp);
        else mc_accum_item<T, NC, 1, U, false>(lg, rstride, R, ngroups * G + (i - ngroups), sum_p, accumulate, samples, sum_h, sum_pp);
    }
}

template <int NC, int G, bool U>
__device__ __forceinline__ void mc_finish_item(const float* sum_p, float n, long long v0, float* mean, float* entropy,
                                               const float* sum_h, const float* sum_pp, float* expected, float* mutual,
                                               float* variance) {
    constexpr int E = G * NC;
    constexpr bool VEC = G > 1;
    float m[E], h[G];
    float q[U ? E : 1], eh[U ? G : 1], mi[U ? G : 1];
    mc_ld<E, VEC>(sum_p + v0 * NC, m);
    if constexpr (U) {                                  // (everything is read before anything is written: the outputs may alias)
        mc_ld<E, VEC>(sum_pp + v0 * NC, q);
        mc_ld<G, VEC>(sum_h + v0, eh);
    }
#pragma unroll
    for (int g = 0; g < G; ++g) {
        float a = 0.f;
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            const float mc = m[g * NC + c] / n;
            m[g * NC + c] = mc;
            if (mc_term<U>(mc)) a = a - mc * logf(mc);  // (mean_c == 0: the term is exactly 0, no 0 * -inf)
        }
        h[g] = a;
    }
    if constexpr (U) {
#pragma unroll
        for (int g = 0; g < G; ++g) {
            eh[g] = eh[g] / n;
            const float d = h[g] - eh[g];
            mi[g] = d < 0.f ? 0.f : d;                  // (not fmaxf: a NaN stays a NaN)
        }
#pragma unroll
        for (int k = 0; k < E; ++k) {
            const float d = q[k] / n - m[k] * m[k];     // (population variance; both terms rounded, so n == 1 gives p*p - p*p = +0)
            q[k] = d < 0.f ? 0.f : d;
        }
    }
    mc_st<E, VEC>(mean + v0 * NC, m);
    mc_st<G, VEC>(entropy + v0, h);
    if constexpr (U) {
        mc_st<G, VEC>(expected + v0, eh);
        mc_st<G, VEC>(mutual + v0, mi);
        mc_st<E, VEC>(variance + v0 * NC, q);
    }
}

// (mean / expected / variance may alias sum_p / sum_h / sum_pp: a thread reads its own elements before it writes them, so none of
// the six is __restrict__; entropy and mutual alias nothing.  Without U only sum_p, mean and entropy are given.)
template <int NC, bool U>
__global__ void __launch_bounds__(256) mc_finish_kernel(const float* sum_p, const float* sum_h, const float* sum_pp, float n,
                                                        long long M, long long ngroups, float* mean, float* __restrict__ entropy,
                                                        float* expected, float* __restrict__ mutual, float* variance) {
    constexpr int G = 4;
    const long long items = ngroups + (M - ngroups * G);
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < items; i += (long long)gridDim.x * 256) {
        if (i < ngroups) mc_finish_item<NC, G, U>(sum_p, n, i * G, mean, entropy, sum_h, sum_pp, expected, mutual, variance);
        else mc_finish_item<NC, 1, U>(sum_p, n, ngroups * G + (i - ngroups), mean, entropy, sum_h, sum_pp, expected, mutual, variance);
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// Test-time augmentation by mirroring: a view is a replica whose logits are read at mirrored coordinates.
//   m1_mc_accum_v: m1_mc_accum / m1_mc_accum_u over (B, D, H, W) with one 3-bit mirror mask per replica (bit 0: W, bit 1: H, bit 2:
//   D; replica r owns bits [3r, 3r + 3) of `flips`, passed by value: no device table, no memcpy node).  Output voxel (b, d, h, w)
//   takes replica r's voxel (b, d', h', w').  It is mc_accum_item with V = true: the same softmax, entropy and square per voxel, the
//   same association, so the sums and the samples are those of the unmirrored entry points on logits un-mirrored beforehand, bit
//   for bit.
//   m1_tta_views: the stacked input of such a pass, replica r = x mirrored by mask r, one launch.
// A group of G voxels is read as one contiguous run only inside one W row, so the vector path needs W % G == 0 on top of the
// alignment the unmirrored launch asks for, and every other shape runs the item with G = 1.  One G per launch, not groups and a
// tail in one kernel: the G = 1 launch then keeps the few registers of the scalar item.
// ---------------------------------------------------------------------------------------------------------------------------------
// M = B * D * H * W voxels in items of G: G divides W (the launcher's vector condition), so it divides M and no item leaves its row
template <typename T, int NC, int G, bool U>
__global__ void __launch_bounds__(256) mc_accum_v_kernel(const T* __restrict__ lg, int R, unsigned long long flips, long long M, int D,
                                                         int H, int W, float* __restrict__ sum_p, float* __restrict__ sum_h,
                                                         float* __restrict__ sum_pp, int accumulate, float* __restrict__ samples) {
    const long long items = M / G, rstride = M * NC;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < items; i += (long long)gridDim.x * 256)
        mc_accum_item<T, NC, G, U, true>(lg, rstride, R, i * G, sum_p, accumulate, samples, sum_h, sum_pp, flips, D, H, W);
}

static inline bool mc_al(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

// The two launch shapes of one pass; `vec`: groups of G voxels may be read and written as 16-byte vectors
template <typename T, int NC, bool U>
static void mc_accum_launch(const T* lg, int R, long long M, float* sum_p, float* sum_h, float* sum_pp, int acc, float* samples, bool vec,
                            hipStream_t st) {
    constexpr int G = sizeof(T) == 2 ? 8 : 4;
    const long long ngroups = vec ? M / G : 0, items = ngroups + (M - ngroups * G);
    const dim3 grid(m1_grid_for(items, 1)), block(256);
    hipLaunchKernelGGL((mc_accum_kernel<T, NC, U>), grid, block, 0, st, lg, R, M, ngroups, sum_p, sum_h, sum_pp, acc, samples);
}

template <typename T, int NC, bool U>
static void mc_accum_v_launch(const T* lg, int R, unsigned long long flips, long long M, int D, int H, int W, float* sum_p, float* sum_h,
                              float* sum_pp, int acc, float* samples, bool vec, hipStream_t st) {
    constexpr int G = sizeof(T) == 2 ? 8 : 4;
    const dim3 grid(m1_grid_for(vec ? M / G : M, 1)), block(256);
    if (vec) hipLaunchKernelGGL((mc_accum_v_kernel<T, NC, G, U>), grid, block, 0, st, lg, R, flips, M, D, H, W, sum_p, sum_h, sum_pp, acc, samples);
    else hipLaunchKernelGGL((mc_accum_v_kernel<T, NC, 1, U>), grid, block, 0, st, lg, R, flips, M, D, H, W, sum_p, sum_h, sum_pp, acc, samples);
}

// W > 0: the mirrored shape over (D, H, W); W == 0: the plain one.  The vector path: every pointer that is given 16-byte aligned, and
// the replica stride a multiple of 16 bytes when there is more than one replica; mirrored, also whole groups in a W row.
template <typename T, int NC, bool U>
static int mc_accum_launch_nc(const void* logits, int R, unsigned long long flips, long long M, int D, int H, int W, float* sum_p,
                              float* sum_h, float* sum_pp, int accumulate, float* samples, hipStream_t st) {
    constexpr int G = sizeof(T) == 2 ? 8 : 4;
    const bool vec = mc_al(logits, 16) && mc_al(sum_p, 16) && mc_al(sum_h, 16) && mc_al(sum_pp, 16) && mc_al(samples, 16) &&
                     (R == 1 || (M * NC * (long long)sizeof(T)) % 16 == 0);
    const int acc = accumulate != 0;
    if (W > 0) mc_accum_v_launch<T, NC, U>((const T*)logits, R, flips, M, D, H, W, sum_p, sum_h, sum_pp, acc, samples, vec && W % G == 0, st);
    else mc_accum_launch<T, NC, U>((const T*)logits, R, M, sum_p, sum_h, sum_pp, acc, samples, vec, st);
    return m1_check_launch();
}

// the runtime nc as the template parameter NC (the check holds it to 2..4)
template <typename T, bool U>
static int mc_accum_dispatch(int nc, const void* logits, int R, unsigned long long flips, long long M, int D, int H, int W, float* sum_p,
                             float* sum_h, float* sum_pp, int accumulate, float* samples, hipStream_t st) {
    switch (nc) {
        case 2: return mc_accum_launch_nc<T, 2, U>(logits, R, flips, M, D, H, W, sum_p, sum_h, sum_pp, accumulate, samples, st);
        case 3: return mc_accum_launch_nc<T, 3, U>(logits, R, flips, M, D, H, W, sum_p, sum_h, sum_pp, accumulate, samples, st);
        default: return mc_accum_launch_nc<T, 4, U>(logits, R, flips, M, D, H, W, sum_p, sum_h, sum_pp, accumulate, samples, st);
    }
}

// R in 1..16 and no bit of `flips` at or above 3R: M1_OK, else the status both mirror entry points answer
static int mc_views_check(int R, unsigned long long flips) {
    if (R <= 0) return M1_ERR_BAD_ARG;
    if (R > 16) return M1_ERR_UNSUPPORTED;
    if (flips >> (3 * R)) return M1_ERR_BAD_ARG;
    return M1_OK;
}

// What the three accumulate entry points refuse, in the order they refuse it.  `vox`: the voxels of one sample, a double because
// D * H * W of three ints need not fit 63 bits; `views`: the replicas are mirrored views, R and `flips` answer to mc_views_check.
// sum_h and sum_pp come together or not at all.
static int mc_accum_check(const void* logits, int R, int B, double vox, int nc, int dtype, bool views, unsigned long long flips,
                          const float* sum_p, const float* sum_h, const float* sum_pp, const float* samples) {
    if (!logits || !sum_p || (sum_h == nullptr) != (sum_pp == nullptr) || R <= 0 || B <= 0 || !(vox > 0) ||
        (dtype != M1_F32 && dtype != M1_BF16))
        return M1_ERR_BAD_ARG;
    if (const int rc = views ? mc_views_check(R, flips) : M1_OK) return rc;
    if (nc < 2 || nc > 4) return M1_ERR_UNSUPPORTED;
    if (!mc_al(logits, dtype == M1_BF16 ? 2 : 4) || !mc_al(sum_p, 4) || !mc_al(sum_h, 4) || !mc_al(sum_pp, 4) || !mc_al(samples, 4))
        return M1_ERR_BAD_ARG;
    if ((double)B * vox > (double)((1ll << 40) / R)) return M1_ERR_BAD_ARG;         // (element offsets stay far inside 63 bits)
    return M1_OK;
}

// One pass behind every m1_mc_accum*: the check, the profile scope `scope` and the launch.  D = H = W = 0 without views.
static int mc_accum_run(const char* scope, const void* logits, int R, int B, double vox, int D, int H, int W, int nc, int dtype,
                        unsigned long long flips, float* sum_p, float* sum_h, float* sum_pp, int accumulate, float* samples, void* stream) {
    if (const int rc = mc_accum_check(logits, R, B, vox, nc, dtype, W > 0, flips, sum_p, sum_h, sum_pp, samples)) return rc;
    const long long M = (long long)((double)B * vox);                                // (exact: the check holds it under 2^40)
    const bool u = sum_h != nullptr;
    const double el = (double)M * nc;
    hipStream_t st = (hipStream_t)stream;
    M1ProfScope ps(scope, 0.0, el * R * (dtype == M1_BF16 ? 2 : 4) + (u ? 2.0 * el + (double)M : el) * 4 * (accumulate ? 2 : 1) +
                   (samples ? el * R * 4 : 0.0), st);
    if (dtype == M1_BF16)
        return u ? mc_accum_dispatch<bf16_t, true>(nc, logits, R, flips, M, D, H, W, sum_p, sum_h, sum_pp, accumulate, samples, st)
                 : mc_accum_dispatch<bf16_t, false>(nc, logits, R, flips, M, D, H, W, sum_p, sum_h, sum_pp, accumulate, samples, st);
    return u ? mc_accum_dispatch<float, true>(nc, logits, R, flips, M, D, H, W, sum_p, sum_h, sum_pp, accumulate, samples, st)
             : mc_accum_dispatch<float, false>(nc, logits, R, flips, M, D, H, W, sum_p, sum_h, sum_pp, accumulate, samples, st);
}

extern "C" int m1_mc_accum(const void* logits, int R, int B, long long V, int nc, int dtype, float* sum_p, int accumulate,
                           float* samples_out, void* stream) {
    if (m1_debug_skip("mc_accum")) return M1_OK;
    return mc_accum_run("mc_accum", logits, R, B, (double)V, 0, 0, 0, nc, dtype, 0ull, sum_p, nullptr, nullptr, accumulate, samples_out,
                        stream);
}

extern "C" int m1_mc_accum_u(const void* logits, int R, int B, long long V, int nc, int dtype, float* sum_p, float* sum_h, float* sum_pp,
                             int accumulate, float* samples_out, void* stream) {
    if (m1_debug_skip("mc_accum")) return M1_OK;
    if (!sum_h || !sum_pp) return M1_ERR_BAD_ARG;
    return mc_accum_run("mc_accum_u", logits, R, B, (double)V, 0, 0, 0, nc, dtype, 0ull, sum_p, sum_h, sum_pp, accumulate, samples_out,
                        stream);
}

extern "C" int m1_mc_accum_v(const void* logits, int R, int B, int D, int H, int W, int nc, int dtype, unsigned long long flips,
                             float* sum_p, float* sum_h, float* sum_pp, int accumulate, float* samples_out, void* stream) {
    if (m1_debug_skip("mc_accum")) return M1_OK;
    if (D <= 0 || H <= 0 || W <= 0) return M1_ERR_BAD_ARG;
    return mc_accum_run("mc_accum_v", logits, R, B, (double)D * H * W, D, H, W, nc, dtype, flips, sum_p, sum_h, sum_pp, accumulate,
                        samples_out, stream);
}

// Both finishes: U = false takes sum_p, mean and entropy alone and leaves the other five pointers null
template <bool U>
static int mc_finish_run(const char* scope, const float* sum_p, const float* sum_h, const float* sum_pp, int n_draws, int B, long long V,
                         int nc, float* mean, float* entropy, float* expected, float* mutual, float* variance, void* stream) {
    if (m1_debug_skip("mc_finish")) return M1_OK;
    const void* ptrs[8] = {sum_p, mean, entropy, sum_h, sum_pp, expected, mutual, variance};
    constexpr int np = U ? 8 : 3;
    for (int i = 0; i < np; ++i)
        if (!ptrs[i]) return M1_ERR_BAD_ARG;
    if (n_draws <= 0 || B <= 0 || V <= 0) return M1_ERR_BAD_ARG;
    if (nc < 2 || nc > 4) return M1_ERR_UNSUPPORTED;
    bool vec = true;
    for (int i = 0; i < np; ++i) {
        if (!mc_al(ptrs[i], 4)) return M1_ERR_BAD_ARG;
        vec = vec && mc_al(ptrs[i], 16);
    }
    const long long M = (long long)B * V;
    if (M > (1ll << 40)) return M1_ERR_BAD_ARG;
    const long long ngroups = vec ? M / 4 : 0, items = ngroups + (M - ngroups * 4);
    const dim3 grid(m1_grid_for(items, 1)), block(256);
    hipStream_t st = (hipStream_t)stream;
    M1ProfScope ps(scope, 0.0, (double)M * ((2.0 * nc + 1.0) + (U ? 2.0 * nc + 3.0 : 0.0)) * 4, st);    // (U: read the sums, write five maps)
    const float n = (float)n_draws;
    switch (nc) {
        case 2: hipLaunchKernelGGL((mc_finish_kernel<2, U>), grid, block, 0, st, sum_p, sum_h, sum_pp, n, M, ngroups, mean, entropy, expected, mutual, variance); break;
        case 3: hipLaunchKernelGGL((mc_finish_kernel<3, U>), grid, block, 0, st, sum_p, sum_h, sum_pp, n, M, ngroups, mean, entropy, expected, mutual, variance); break;
        default: hipLaunchKernelGGL((mc_finish_kernel<4, U>), grid, block, 0, st, sum_p, sum_h, sum_pp, n, M, ngroups, mean, entropy, expected, mutual, variance); break;
    }
    return m1_check_launch();
}

extern "C" int m1_mc_finish(const float* sum_p, int n_draws, int B, long long V, int nc, float* mean, float* entropy, void* stream) {
    return mc_finish_run<false>("mc_finish", sum_p, nullptr, nullptr, n_draws, B, V, nc, mean, entropy, nullptr, nullptr, nullptr, stream);
}

extern "C" int m1_mc_finish_u(const float* sum_p, const float* sum_h, const float* sum_pp, int n_draws, int B, long long V, int nc,
                              float* mean, float* entropy, float* expected_entropy, float* mutual_info, float* variance, void* stream) {
    return mc_finish_run<true>("mc_finish_u", sum_p, sum_h, sum_pp, n_draws, B, V, nc, mean, entropy, expected_entropy, mutual_info,
                               variance, stream);
}

// The copy in 16-byte chunks of a W row (W * C elements, a whole number of chunks; ET = the element as an unsigned integer): a thread
// reads one chunk of x once and, per replica, stores it whole to the same place of the (D-, H-) mirrored row, or with a W mirror
// scatters its K elements to (W - 1 - w) * C + c -- a wave's stores still cover one contiguous run of the row, backwards.
template <typename ET>
__global__ void __launch_bounds__(256) tta_views_row_kernel(const uint4* __restrict__ x, long long rows, int D, int H, int W, int C,
                                                            int cpr, int R, unsigned long long flips, ET* __restrict__ out) {
    constexpr int K = 16 / (int)sizeof(ET);
    const long long items = rows * cpr, rowlen = (long long)W * C;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < items; i += (long long)gridDim.x * 256) {
        const long long row = i / cpr, bd = row / H, b = bd / D;
        const int q = (int)(i - row * cpr), h = (int)(row - bd * H), d = (int)(bd - b * D);
        union { uint4 v; ET e[K]; } u;
        u.v = x[i];
        const int e0 = q * K, w0 = e0 / C, c0 = e0 - w0 * C;
        for (int r = 0; r < R; ++r) {
            const unsigned m = (unsigned)(flips >> (3 * r)) & 7u;
            const int dd = (m & 4u) ? D - 1 - d : d, hd = (m & 2u) ? H - 1 - h : h;
            ET* dst = out + ((long long)r * rows + (b * D + dd) * H + hd) * rowlen;
            if (!(m & 1u)) {
                *reinterpret_cast<uint4*>(dst + e0) = u.v;
            } else {
                int w = w0, c = c0;
#pragma unroll
                for (int j = 0; j < K; ++j) {
                    dst[(W - 1 - w) * C + c] = u.e[j];
                    if (++c == C) { c = 0; ++w; }
                }
            }
        }
    }
}

// Every other shape or alignment: one unit (4 or 2 bytes) of one voxel of x to its place in every replica, n units per voxel.
template <typename UT>
__global__ void __launch_bounds__(256) tta_views_kernel(const UT* __restrict__ x, long long M, int D, int H, int W, int n, int R,
                                                        unsigned long long flips, UT* __restrict__ out) {
    const long long items = M * n;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < items; i += (long long)gridDim.x * 256) {
        const long long v0 = i / n, row = v0 / W, bd = row / H, b = bd / D;
        const int u = (int)(i - v0 * n), w = (int)(v0 - row * W), h = (int)(row - bd * H), d = (int)(bd - b * D);
        const UT val = x[i];
        for (int r = 0; r < R; ++r) {
            const unsigned m = (unsigned)(flips >> (3 * r)) & 7u;
            const int dd = (m & 4u) ? D - 1 - d : d, hd = (m & 2u) ? H - 1 - h : h, wd = (m & 1u) ? W - 1 - w : w;
            out[((long long)r * M + ((b * D + dd) * H + hd) * W + wd) * n + u] = val;
        }
    }
}

extern "C" int m1_tta_views(const void* x, int B, int D, int H, int W, int C, int dtype, int R, unsigned long long flips, void* out,
                            void* stream) {
    if (m1_debug_skip("tta_views")) return M1_OK;
    if (!x || !out || B <= 0 || D <= 0 || H <= 0 || W <= 0 || C <= 0 || (dtype != M1_F32 && dtype != M1_BF16)) return M1_ERR_BAD_ARG;
    if (const int rc = mc_views_check(R, flips)) return rc;
    const int es = dtype == M1_BF16 ? 2 : 4;
    if (!mc_al(x, es) || !mc_al(out, es)) return M1_ERR_BAD_ARG;
    if ((double)B * D * H * W * C > (double)((1ll << 40) / R)) return M1_ERR_BAD_ARG;
    const long long M = (long long)B * D * H * W, vb = (long long)C * es, rb = vb * W;      // (voxels; bytes per voxel, per W row)
    hipStream_t st = (hipStream_t)stream;
    M1ProfScope ps("tta_views", 0.0, (double)M * vb * (1.0 + R), st);
    const dim3 block(256);
    if (rb % 16 == 0 && rb < (1ll << 31) && mc_al(x, 16) && mc_al(out, 16)) {
        const long long rows = M / W;
        const int cpr = (int)(rb / 16);
        const dim3 grid(m1_grid_for(rows * cpr, 1));
        if (es == 4) hipLaunchKernelGGL(tta_views_row_kernel<unsigned>, grid, block, 0, st, (const uint4*)x, rows, D, H, W, C, cpr, R, flips, (unsigned*)out);
        else hipLaunchKernelGGL(tta_views_row_kernel<unsigned short>, grid, block, 0, st, (const uint4*)x, rows, D, H, W, C, cpr, R, flips, (unsigned short*)out);
        return m1_check_launch();
    }
    const int ub = (vb % 4 == 0 && mc_al(x, 4) && mc_al(out, 4)) ? 4 : 2;
    const int n = (int)(vb / ub);
    const dim3 grid(m1_grid_for(M * n, 1));
    if (ub == 4) hipLaunchKernelGGL(tta_views_kernel<unsigned>, grid, block, 0, st, (const unsigned*)x, M, D, H, W, n, R, flips, (unsigned*)out);
    else hipLaunchKernelGGL(tta_views_kernel<unsigned short>, grid, block, 0, st, (const unsigned short*)x, M, D, H, W, n, R, flips, (unsigned short*)out);
    return m1_check_launch();
}
