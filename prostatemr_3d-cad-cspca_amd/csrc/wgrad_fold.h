// wgrad_fold.h -- what the weight-gradient launchers (wgrad_*.hip) share on the host: the plan of the per-split partial copies, the
// K-tile geometry, the fold of the copies and the process-wide queue of deferred folds (wgrad_fold.hip).
#pragma once
#include "gather.h"

// ---- partial copies -------------------------------------------------------------------------------------------------------------
// Every voxel split stores its tile into its own compact copy of ONE concat member's block, [tap][CA][CB] floats with the bias
// sums behind it, inside the spec's rx region (dispatch.hip: wgrad_rx_bytes sizes it with the same two definitions).
#define M1_WG_MAX_COPIES 512
static inline long long m1_wg_copy_floats(long long taps, long long CA, long long CB, long long nbias) { return taps * CA * CB + nbias; }

// What differs between the launchers, as data: one initialiser next to each kernel.
enum WgShort { WG_SHORT_ERROR,        // a region that holds no copy: M1_ERR_WORKSPACE, nothing launched (the ladder's next rung)
               WG_SHORT_FALLBACK };   // a region that holds fewer than two: no copies (Rx = nullptr), the launcher runs one split or atomics
struct WgCopyRule {
    int min_ktiles;          // K-tiles a copy must be worth (0: the launcher bounds its splits itself)
    int max_copies;          // ceiling on the copies (0: none)
    long long max_bytes;     // ceiling on the bytes of all copies (0: none)
    WgShort on_short;
};
struct WgCopies { long long stride, rx_bias, nsplit; float* Rx; int rc; long long fit; };     // fit: copies the region holds (plan log)
// `want` splits of `ntiles` K-tiles under rule `r`; use_rx = false: the split count for a launch without copies
static inline WgCopies m1_wg_copies(const WgradSpec& g, int taps, long long want, long long ntiles, const WgCopyRule& r, bool use_rx = true) {
    WgCopies c{};
    c.rx_bias = (long long)taps * g.CA * g.CB;
    c.stride = m1_wg_copy_floats(taps, g.CA, g.CB, g.CB);
    c.rc = M1_OK;
    long long n = want;
    if (r.min_ktiles && n > ntiles / r.min_ktiles) n = ntiles / r.min_ktiles;
    if (r.max_copies && n > r.max_copies) n = r.max_copies;
    if (r.max_bytes && n * c.stride * 4 > r.max_bytes) n = r.max_bytes / (c.stride * 4);
    const long long fit = g.rx ? g.rx_floats / c.stride : 0;
    c.fit = fit;
    if (r.on_short == WG_SHORT_ERROR) {
        if (fit < 1) { c.rc = M1_ERR_WORKSPACE; return c; }
        if (n > fit) n = fit;                                  // as many copies as the caller's scratch holds
        // no split left: the launcher with a byte ceiling (tf) declines, the others run one split (only reachable for tf, whose
        // single copy can exceed its ceiling: the others' planners guarantee min_ktiles K-tiles.  Looks like drift; kept.)
        if (n < 1) { if (r.max_bytes) { c.rc = M1_ERR_UNSUPPORTED; return c; } n = 1; }
        c.Rx = g.rx;
    } else {
        if (n < 1) n = 1;
        if (use_rx && n >= 2 && fit >= 2) { if (n > fit) n = fit; c.Rx = g.rx; }
    }
    c.nsplit = n;
    return c;
}

// ---- K-tile geometry ------------------------------------------------------------------------------------------------------------
// A K-tile is TH rows x KWs columns of one (n, d) slice of B: at most `kt` voxel slots.  Columns: the largest of 32 / 16 / 8 that
// divides the row, else the kernel's own answer `other` (tap: the whole row; tf, t3s: gated to multiples of 8 before).
static inline int m1_wg_kws(int BW, int other) { return BW % 32 == 0 ? 32 : (BW % 16 == 0 ? 16 : (BW % 8 == 0 ? 8 : other)); }
struct WgKTiles { int KWs, TH, tiles_w, tiles_h; long long ntiles; };
// fills those five fields of a kernel's parameter struct (or of a WgKTiles); false: fewer than min_tiles K-tiles, or too many for
// the kernels' 32-bit tile counters
template <typename P>
static inline bool m1_wg_ktiles(const WgradSpec& g, int kt, int kws, long long min_tiles, P& p) {
    p.KWs = kws; p.TH = kt / kws;
    p.tiles_w = g.BW / kws; p.tiles_h = (g.BH + p.TH - 1) / p.TH;
    const long long nt = (long long)g.N * g.BD * p.tiles_h * p.tiles_w;
    p.ntiles = (decltype(p.ntiles))nt;
    return nt < (1ll << 30) && nt >= min_tiles;
}
// both operands addressable with 32-bit voxel indices (tap, tf: DMA offsets relative to a tile origin, 2^20 voxels of slack)
// the launcher's line of the plan log (m1_debug_plans), noted next to its m1_note_kernel once the plan is final
static inline void m1_wg_note_plan(const char* name, long long tiles, long long want, long long splits, const WgCopies& c, bool rx, int stages,
                                   unsigned gx, unsigned gy, unsigned gz) {
    m1_note_plan("wg:%s tiles=%lld want=%lld splits=%lld fit=%lld rx=%d stages=%d grid=%u,%u,%u", name, tiles, want, splits, c.fit, (int)rx,
                 stages, gx, gy, gz);
}
static inline bool m1_wg_vox32(const WgradSpec& g) {
    const long long lim = (1ll << 31) - (1 << 20);
    return (long long)g.N * g.AD * g.AH * g.AW < lim && (long long)g.N * g.BD * g.BH * g.BW < lim;
}

// ---- the fold and its queue (wgrad_fold.hip) --------------------------------------------------------------------------------------
// Adds `ncopies` copies of stride `stride` floats into g.R / g.bsum in a fixed order (bias sums at offset nw inside a copy); under
// m1_wgrad_defer the fold is queued for m1_wgrad_fold_pending instead.
int m1_wg_rx_finish(float* rx, long long stride, int ncopies, const WgradSpec& g, long long nw, hipStream_t st);
// one fold per concat member of a multi-member launch: member m's copies at rx + m * rx_mem, its block of R at a_offs[m] (nmem = 1:
// g's own a_off); the bias sums ride on member 0
int m1_wg_fold_members(float* rx, long long rx_mem, long long stride, int ncopies, const WgradSpec& g, long long nw, int nmem,
                       const int* a_offs, hipStream_t st);
int m1_fold_defer_set(int on);                  // the switch of m1_wgrad_defer; returns the previous setting
// Bias gradient of a transposed conv, out[c] (+)= sum_{n,v} x[n,v,c], queued with the folds.  true: queued, nothing launched (x and
// ws stay alive until m1_wgrad_fold_pending / _drop); false: the caller reduces now
bool m1_colsum_defer(const void* x, int N, long long V, int C, int dtype, float* out, float* ws, int accumulate);

// the column-sum kernels behind that queue (norm.hip)
#define CS_MAX 24
struct ColSumJob { const void* x; long long V; int C, N, chunkV, nchunks; float* partial; float* out; int acc; };
bool m1_colsum_job(const void* x, int N, long long V, int C, int dtype, float* out, float* ws, int accumulate, ColSumJob* job);   // false: shape outside the batched kernel
int m1_colsum_launch_batch(const ColSumJob* jobs, int n, int dtype, hipStream_t st);       // n <= CS_MAX jobs of one dtype: reduce + finalize
