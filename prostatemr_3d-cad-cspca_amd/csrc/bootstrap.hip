// bootstrap.hip -- case-level bootstrap replicates of AUROC, AP, the FROC sensitivities and per-case means (bootstrap.py: replicates()).
//   The scores never change between replicates, only the case multiplicities do: the host sorts once (bootstrap.pack) and a replicate
//   is one draw, two weighted prefix scans and a few integer comparisons.
//   table (include/m1hip.h: m1_bootstrap_table_t): the cases in ascending score order (label, group end, lesions), the events --
//   candidates and matched lesions with confidence > 0 -- in descending confidence order (case, is TP, group end), values (V, N) fp64
//   -> out (n_boot, 2 + R + V) fp64: auroc, ap, sens@rate[0..R), mean of values[0..V); NaN where a replicate cannot define one.
// One workgroup of 256 threads per replicate (bs_kernel):
//   1. the multiplicities w[N] (u32) live in LDS: zeroed, then N draws of Philox4x32-10 added with LDS integer atomics (any order gives
//      the same integers), or the caller's row of weights copied in.  Everything after reads w from LDS.
//   2. cases, in chunks of 1024 (four consecutive cases per thread): block-wide inclusive scans of the weighted positives and negatives
//      with carries between the chunks.  At a group end (the last case of a run of equal scores)
//          2U += pos_g * (2 * neg_below + neg_g) = (P_end - P_prev_end) * (N_prev_end + N_end),
//      where the counts at the PREVIOUS group end are an exclusive max-scan of (group end ? count : 0) -- the counts are monotone -- so
//      nothing looks behind across threads or chunks.  auroc = 2U / (2 * P_w * N_w), one fp64 division of two integers.
//   3. events, the same pass over the weighted TP and FP counts.  At a group end k (a threshold of detection.froc):
//          sens@x  = the TP count at the last group end with (double)fp / (double)sum_w <= x (an integer max), / lesions
//          ap     += (tp_k / L - tp_prev / L) * (tp_k / (tp_k + fp_k)) where tp_k > tp_prev
//      -- the fp64 expressions of detection.froc / validation.sens_at / detection.average_precision, term by term.
//   4. means: sum of w_i * x_i over the cases whose x_i is not NaN / their weight.
// The AP sum and the value sums are fp64 folds in a fixed order: per thread (ascending index), per wave (xor butterfly), per block (the
// four waves in order).  No floating-point atomics, no global workspace, no memset / memcpy node, no host read: capturable, and a row is
// a pure function of (table, seed, replicate index) -- bit-identical over runs, grids (n_boot) and pointer alignments (narrow loads only).
// Ranges: w_i <= 65535 (weights) or <= N <= 16384 (draws), so sum_w < 2^30 and 2 * P_w * N_w < 2^61; a chunk's scans stay below 2^26
// and travel as two 32-bit halves of one word, the carries are 64-bit.
#include "common.h"

#define BS_THREADS 256
#define BS_PER 4                             // consecutive items per thread and chunk
#define BS_CHUNK (BS_THREADS * BS_PER)       // items per pass: M1_BOOTSTRAP_CHUNK
#define BS_WAVES (BS_THREADS / M1_WAVE)
static_assert(BS_CHUNK == M1_BOOTSTRAP_CHUNK, "include/m1hip.h names the chunk");
typedef unsigned long long u64;

struct BsP {
    m1_bootstrap_table_t t;
    const int* weights;
    double* out;
    double rates[M1_BOOTSTRAP_MAX_RATES];
    u64 key;
    int R, S;
};

__device__ __forceinline__ u64 bs_max(u64 a, u64 b) { return a > b ? a : b; }

// inclusive scans over the 64 lanes of a wave
__device__ __forceinline__ u64 bs_wave_scan_add(u64 v) {
    const int lane = threadIdx.x & (M1_WAVE - 1);
#pragma unroll
    for (int o = 1; o < M1_WAVE; o <<= 1) {
        const u64 u = __shfl_up(v, o, M1_WAVE);
        if (lane >= o) v += u;
    }
    return v;
}
__device__ __forceinline__ u64 bs_wave_scan_max(u64 v) {
    const int lane = threadIdx.x & (M1_WAVE - 1);
#pragma unroll
    for (int o = 1; o < M1_WAVE; o <<= 1) {
        const u64 u = __shfl_up(v, o, M1_WAVE);
        if (lane >= o) v = bs_max(v, u);
    }
    return v;
}
// exclusive scans over the block; sm: BS_WAVES slots nobody else touches until the next barrier.  total = the fold of all 256 values.
__device__ __forceinline__ u64 bs_block_scan_add(u64 v, u64* sm, u64& total) {
    const int lane = threadIdx.x & (M1_WAVE - 1), wv = threadIdx.x >> 6;
    const u64 inc = bs_wave_scan_add(v);
    if (lane == M1_WAVE - 1) sm[wv] = inc;
    __syncthreads();
    u64 base = 0, tot = 0;
#pragma unroll
    for (int k = 0; k < BS_WAVES; ++k) {
        const u64 s = sm[k];
        if (k < wv) base += s;
        tot += s;
    }
    total = tot;
    return base + inc - v;
}
__device__ __forceinline__ u64 bs_block_scan_max(u64 v, u64* sm, u64& total) {
    const int lane = threadIdx.x & (M1_WAVE - 1), wv = threadIdx.x >> 6;
    const u64 inc = bs_wave_scan_max(v);
    if (lane == M1_WAVE - 1) sm[wv] = inc;
    __syncthreads();
    u64 base = 0, tot = 0;
#pragma unroll
    for (int k = 0; k < BS_WAVES; ++k) {
        const u64 s = sm[k];
        if (k < wv) base = bs_max(base, s);
        tot = bs_max(tot, s);
    }
    total = tot;
    const u64 before = __shfl_up(inc, 1, M1_WAVE);                        // the inclusive scan of the lane in front = this lane's exclusive
    return lane ? bs_max(base, before) : base;
}
__device__ __forceinline__ u64 bs_wave_sum(u64 v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, M1_WAVE);
    return v;
}
__device__ __forceinline__ u64 bs_wave_max(u64 v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = bs_max(v, __shfl_xor(v, o, M1_WAVE));
    return v;
}

// One chunked pass over `n` items in order.  Item i adds (a, b) -- the weight of its case in the first or the second count -- and may
// end a group; at_end(a_end, b_end, a_prev, b_prev) runs at every group end, in item order inside a thread, with the inclusive counts
// there and the counts at the group end before it (0, 0 in front of the first).  Returns the totals through (ta, tb).
template <typename Item, typename AtEnd>
__device__ __forceinline__ void bs_pass(int n, u64* sm, Item item, AtEnd at_end, u64& ta, u64& tb) {
    u64 ca = 0, cb = 0;                      // the counts in front of this chunk
    u64 ea = 0, eb = 0;                      // the counts at the last group end in front of this chunk
    for (int base = 0; base < n; base += BS_CHUNK) {
        const int i0 = base + (int)threadIdx.x * BS_PER;
        unsigned a[BS_PER], b[BS_PER];
        bool end[BS_PER];
        u64 mine = 0;
#pragma unroll
        for (int e = 0; e < BS_PER; ++e) {
            a[e] = 0u; b[e] = 0u; end[e] = false;
            if (i0 + e < n) item(i0 + e, a[e], b[e], end[e]);
            mine += (u64)a[e] | ((u64)b[e] << 32);
        }
        u64 tot;
        const u64 ex = bs_block_scan_add(mine, sm, tot);
        const u64 pa = ca + (ex & 0xffffffffull), pb = cb + (ex >> 32);
        u64 ra = pa, rb = pb, ga = 0, gb = 0;                              // this thread's last group end (0: none; the counts are monotone)
#pragma unroll
        for (int e = 0; e < BS_PER; ++e) {
            ra += a[e]; rb += b[e];
            if (end[e]) { ga = ra; gb = rb; }
        }
        u64 ma, mb;
        u64 qa = bs_max(bs_block_scan_max(ga, sm + BS_WAVES, ma), ea);
        u64 qb = bs_max(bs_block_scan_max(gb, sm + 2 * BS_WAVES, mb), eb);
        ra = pa; rb = pb;
#pragma unroll
        for (int e = 0; e < BS_PER; ++e) {
            ra += a[e]; rb += b[e];
            if (end[e]) { at_end(ra, rb, qa, qb); qa = ra; qb = rb; }
        }
        ca += tot & 0xffffffffull; cb += tot >> 32;
        ea = bs_max(ea, ma); eb = bs_max(eb, mb);
        __syncthreads();                                                  // (sm is written again by the next chunk, or by the caller)
    }
    ta = ca; tb = cb;
}

__global__ void __launch_bounds__(BS_THREADS) bs_kernel(BsP q) {
    extern __shared__ unsigned bs_w[];                                    // N multiplicities
    __shared__ u64 sm[3 * BS_WAVES];
    __shared__ u64 red_u[BS_WAVES][2 + M1_BOOTSTRAP_MAX_RATES];
    __shared__ double red_d[BS_WAVES][1 + M1_BOOTSTRAP_MAX_VALUES];
    __shared__ u64 red_c[BS_WAVES][M1_BOOTSTRAP_MAX_VALUES];
    const int t = threadIdx.x, lane = t & (M1_WAVE - 1), wv = t >> 6;
    const int N = q.t.N, M = q.t.M, V = q.t.V, R = q.R;
    const unsigned rep = blockIdx.x;

    // ---- 1. the multiplicities ----
    if (q.weights) {
        const int* __restrict__ row = q.weights + (size_t)rep * (size_t)N;
        for (int i = t; i < N; i += BS_THREADS) {
            const int v = row[i];
            bs_w[i] = v < 0 ? 0u : (v > 65535 ? 65535u : (unsigned)v);
        }
    } else {
        for (int i = t; i < N; i += BS_THREADS) bs_w[i] = 0u;
        __syncthreads();
        const bool strat = q.t.P >= 0;                                    // (P < 0: every draw over all N cases)
        const unsigned P = strat ? (unsigned)q.t.P : 0u, uN = (unsigned)N;
        for (int c = t; c < ((N + 3) >> 2); c += BS_THREADS) {
            const uint4 r = philox4x32_10(q.key, ((u64)rep << 12) + (u64)c);
            const unsigned word[4] = {r.x, r.y, r.z, r.w};
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const unsigned j = 4u * (unsigned)c + k;
                if (j < uN) {
                    unsigned idx;
                    if (!strat) idx = (unsigned)(((u64)word[k] * uN) >> 32);
                    else if (j < P) idx = (unsigned)(((u64)word[k] * P) >> 32);
                    else idx = P + (unsigned)(((u64)word[k] * (uN - P)) >> 32);
                    if (q.t.draw_perm) idx = (unsigned)q.t.draw_perm[idx];
                    if (idx < uN) atomicAdd(&bs_w[idx], 1u);             // (a permutation entry outside the table is dropped, not followed)
                }
            }
        }
    }
    __syncthreads();

    // ---- 2. cases: AUROC, sum_w and the weighted lesion count ----
    u64 twoU = 0, lw = 0, Pw, Nw;
    bs_pass(N, sm,
            [&](int i, unsigned& a, unsigned& b, bool& end) {
                const unsigned w = bs_w[i];
                if (q.t.case_label[i]) a = w; else b = w;
                end = q.t.case_group_end[i] != 0;
                const int les = q.t.case_lesions[i];
                lw += (u64)w * (u64)(les > 0 ? les : 0);
            },
            [&](u64 pe, u64 ne, u64 pp, u64 np) { twoU += (pe - pp) * (np + ne); }, Pw, Nw);
    twoU = bs_wave_sum(twoU);
    lw = bs_wave_sum(lw);
    if (lane == 0) { red_u[wv][0] = twoU; red_u[wv][1] = lw; }
    __syncthreads();
    twoU = (red_u[0][0] + red_u[1][0]) + (red_u[2][0] + red_u[3][0]);
    const u64 Lw = (red_u[0][1] + red_u[1][1]) + (red_u[2][1] + red_u[3][1]);
    const u64 Sw = Pw + Nw;
    __syncthreads();

    // ---- 3. events: the sensitivities and AP ----
    const double dL = (double)Lw, dS = (double)Sw;
    double ap = 0.0;
    u64 best[M1_BOOTSTRAP_MAX_RATES];
#pragma unroll
    for (int r = 0; r < M1_BOOTSTRAP_MAX_RATES; ++r) best[r] = 0;
    u64 tpw, fpw;
    bs_pass(M, sm,
            [&](int i, unsigned& a, unsigned& b, bool& end) {
                const unsigned c = (unsigned)q.t.ev_case[i];
                const unsigned w = c < (unsigned)N ? bs_w[c] : 0u;
                if (q.t.ev_tp[i]) a = w; else b = w;
                end = q.t.ev_group_end[i] != 0;
            },
            [&](u64 tp, u64 fp, u64 tp_prev, u64) {
                if (tp > tp_prev) ap += ((double)tp / dL - (double)tp_prev / dL) * ((double)tp / (double)(tp + fp));
                const double fpc = (double)fp / dS;
#pragma unroll
                for (int r = 0; r < M1_BOOTSTRAP_MAX_RATES; ++r)
                    if (r < R && fpc <= q.rates[r]) best[r] = tp;          // (monotone: the last one that passes is the largest)
            }, tpw, fpw);
    ap = wave_sum_d(ap);
#pragma unroll
    for (int r = 0; r < M1_BOOTSTRAP_MAX_RATES; ++r) best[r] = bs_wave_max(best[r]);
    if (lane == 0) {
        red_d[wv][0] = ap;
#pragma unroll
        for (int r = 0; r < M1_BOOTSTRAP_MAX_RATES; ++r) red_u[wv][2 + r] = best[r];
    }

    // ---- 4. the means ----
    for (int v = 0; v < V; ++v) {
        const double* __restrict__ col = q.t.values + (size_t)v * (size_t)N;
        double s = 0.0;
        u64 c = 0;
        for (int i = t; i < N; i += BS_THREADS) {
            const unsigned w = bs_w[i];
            const double x = col[i];
            if (w && x == x) { s += (double)w * x; c += w; }
        }
        s = wave_sum_d(s);
        c = bs_wave_sum(c);
        if (lane == 0) { red_d[wv][1 + v] = s; red_c[wv][v] = c; }
    }
    __syncthreads();

    double* __restrict__ o = q.out + (size_t)rep * (size_t)q.S;
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    if (t == 0) {
        o[0] = (Pw && Nw) ? (double)twoU / (double)(2ull * Pw * Nw) : nan;
        o[1] = Lw ? (red_d[0][0] + red_d[1][0]) + (red_d[2][0] + red_d[3][0]) : nan;
    }
    if (t < R) {
        const u64 b = bs_max(bs_max(red_u[0][2 + t], red_u[1][2 + t]), bs_max(red_u[2][2 + t], red_u[3][2 + t]));
        o[2 + t] = Lw ? (double)b / dL : nan;
    }
    if (t < V) {
        const u64 c = (red_c[0][t] + red_c[1][t]) + (red_c[2][t] + red_c[3][t]);
        const double s = (red_d[0][1 + t] + red_d[1][1 + t]) + (red_d[2][1 + t] + red_d[3][1 + t]);
        o[2 + R + t] = c ? s / (double)c : nan;
    }
}

extern "C" int m1_bootstrap_metrics(const m1_bootstrap_table_t* table, int n_boot, uint64_t seed, const int* weights,
                                    const double* fp_rates, int n_rates, double* out, void* stream) {
    if (!table || !out || n_boot < 1) return M1_ERR_BAD_ARG;
    const m1_bootstrap_table_t& t = *table;
    if (t.N < 1 || t.M < 0 || t.V < 0 || t.V > M1_BOOTSTRAP_MAX_VALUES || n_rates < 0 || n_rates > M1_BOOTSTRAP_MAX_RATES)
        return M1_ERR_BAD_ARG;
    if (!t.case_label || !t.case_group_end || !t.case_lesions || (n_rates && !fp_rates) || (t.V && !t.values)) return M1_ERR_BAD_ARG;
    if (t.M && (!t.ev_case || !t.ev_tp || !t.ev_group_end)) return M1_ERR_BAD_ARG;
    if (t.P > t.N) return M1_ERR_BAD_ARG;
    if ((((uintptr_t)t.case_lesions | (uintptr_t)t.ev_case | (uintptr_t)t.draw_perm | (uintptr_t)weights) & 3)
        || (((uintptr_t)t.values | (uintptr_t)out) & 7)) return M1_ERR_BAD_ARG;
    if (n_boot > M1_BOOTSTRAP_MAX_BOOT || t.N > M1_BOOTSTRAP_MAX_CASES) return M1_ERR_UNSUPPORTED;
    if (m1_debug_skip("bootstrap_metrics")) return M1_OK;
    BsP q;
    q.t = t; q.weights = weights; q.out = out; q.R = n_rates; q.S = 2 + n_rates + t.V;
    if (!t.M) { q.t.ev_case = nullptr; q.t.ev_tp = nullptr; q.t.ev_group_end = nullptr; }
    if (!t.V) q.t.values = nullptr;
    for (int r = 0; r < M1_BOOTSTRAP_MAX_RATES; ++r) q.rates[r] = r < n_rates ? fp_rates[r] : 0.0;
    q.key = seed + (uint64_t)M1_STREAM_BOOTSTRAP * 0x9E3779B97F4A7C15ull;
    const int lds = (int)sizeof(unsigned) * t.N;
    // (more than the default dynamic limit only near the cap; the opt-in is asked for the cap, once per process)
    if (lds > 32 * 1024 && m1_allow_dynamic_lds((const void*)bs_kernel, (int)sizeof(unsigned) * M1_BOOTSTRAP_MAX_CASES) != M1_OK)
        return M1_ERR_LAUNCH;
    hipStream_t s = (hipStream_t)stream;
    const double per = 6.0 * t.N + 6.0 * t.M + 8.0 * t.N * t.V + (weights || t.draw_perm ? 4.0 * t.N : 0.0) + 8.0 * q.S;
    M1ProfScope ps("bootstrap_metrics", 0.0, per * n_boot, s);
    hipLaunchKernelGGL(bs_kernel, dim3((unsigned)n_boot), dim3(BS_THREADS), (size_t)lds, s, q);
    return m1_check_launch();
}
