// dispatch.hip -- the public conv entry points.  Each builds the logical problems (gather.h) of its role and runs them on the
// matrix-core kernels, whatever the channel counts (unaligned members are zero-padded to whole 16-byte K segments inside the
// kernel); the generic direct kernels take what those kernels decline and are the m1_set_force_direct reference path.
//   plan_gather    where every sub-problem of a forward / data gradient keeps its panel in `ws`, and when the data gradient is fused
//   wgrad_ws       the regions of a weight gradient's `ws`
//   WG_LADDER      the order in which the weight-gradient kernels are tried
#include "common.h"
#include "wgrad_fold.h"
#include "reduce.h"
#include <stdio.h>
#include <stdlib.h>

static inline bool desc_ok(const m1_conv_desc_t* d) {
    if (!(d && d->N > 0 && d->D > 0 && d->H > 0 && d->W > 0 && d->Cin > 0 && d->Cout > 0 && d->kd > 0 && d->kh > 0 &&
          d->kw > 0 && d->sd > 0 && d->sh > 0 && d->sw > 0 && d->nsrc >= 1 && d->nsrc <= M1_MAX_SRC)) return false;
    if (d->dtype != M1_F32 && d->dtype != M1_BF16) return false;
    int c = 0;
    for (int i = 0; i < d->nsrc; ++i) { if (!d->src[i].ptr || d->src[i].C <= 0) return false; c += d->src[i].C; }
    return c == d->Cin;
}
static inline double esz(int dt) { return dt == M1_BF16 ? 2.0 : 4.0; }
static inline void same_pad(int in, int k, int s, int* out, int* pb) {
    int o = (in + s - 1) / s;
    int tot = (o - 1) * s + k - in; if (tot < 0) tot = 0;
    *out = o; *pb = tot / 2;
}
static inline int convT_pb(int k, int s) { return (k - s > 0 ? k - s : 0) / 2; }

struct Geo { int OD, OH, OW, pd, ph, pw; };
static inline Geo conv_geo(const m1_conv_desc_t* d) {
    Geo g; same_pad(d->D, d->kd, d->sd, &g.OD, &g.pd); same_pad(d->H, d->kh, d->sh, &g.OH, &g.ph); same_pad(d->W, d->kw, d->sw, &g.OW, &g.pw);
    return g;
}
static inline Geo convT_geo(const m1_conv_desc_t* d) {
    Geo g; g.OD = d->D * d->sd; g.OH = d->H * d->sh; g.OW = d->W * d->sw;
    g.pd = convT_pb(d->kd, d->sd); g.ph = convT_pb(d->kh, d->sh); g.pw = convT_pb(d->kw, d->sw);
    return g;
}
// algorithmic work: flops = 2*MAC; bytes = every logical input read once + output written once
static inline double conv_macs(const m1_conv_desc_t* d, bool T) {
    Geo g = T ? convT_geo(d) : conv_geo(d);
    const double taps = (double)d->kd * d->kh * d->kw;
    const double vox = T ? (double)d->D * d->H * d->W : (double)g.OD * g.OH * g.OW;
    return (double)d->N * vox * taps * d->Cin * d->Cout;
}
static inline double conv_bytes(const m1_conv_desc_t* d, bool T) {
    Geo g = T ? convT_geo(d) : conv_geo(d);
    return ((double)d->N * d->D * d->H * d->W * d->Cin + (double)d->N * g.OD * g.OH * g.OW * d->Cout) * esz(d->dtype);
}

// M1_PROF_DETAIL=1: the profiler hooks (prof.hip) key conv records by geometry, not only by entry point
struct ProfName { char s[48]; };
static ProfName prof_name(const char* fam, const m1_conv_desc_t* d) {
    int detail = M1_CFG("M1_PROF_DETAIL", 0);
    ProfName n; 
    if (!detail) { snprintf(n.s, sizeof(n.s), "%s", fam); return n; }
    snprintf(n.s, sizeof(n.s), "%s %dx%dx%d c%d>%d k%d%d%d s%d%d%d m%d", fam, d->D, d->H, d->W, d->Cin, d->Cout, d->kd, d->kh, d->kw,
             d->sd, d->sh, d->sw, d->nsrc);
    return n;
}

extern "C" const char* m1_status_name(int s) {
    switch (s) {
        case M1_OK: return "M1_OK";
        case M1_ERR_BAD_ARG: return "M1_ERR_BAD_ARG";
        case M1_ERR_UNSUPPORTED: return "M1_ERR_UNSUPPORTED";
        case M1_ERR_LAUNCH: return "M1_ERR_LAUNCH";
        case M1_ERR_WORKSPACE: return "M1_ERR_WORKSPACE";
        default: return "M1_ERR_UNKNOWN";
    }
}
extern "C" int m1_abi_version(void) { return 1; }

static int g_force_direct = 0;
extern "C" int m1_set_force_direct(int on) { g_force_direct = on; return M1_OK; }

static inline size_t align256(size_t v) { return (v + 255) / 256 * 256; }
static inline unsigned char* at(void* ws, size_t off) { return ws ? (unsigned char*)ws + off : nullptr; }

// matrix-core kernel if not forced direct and supported, else the direct kernel (which needs no workspace)
static bool use_mfma(const GatherSpec& g) { return !g_force_direct && m1_mfma_supported(g); }
static size_t gather_ws_bytes(const GatherSpec& g) { return use_mfma(g) ? align256(m1_mfma_ws_bytes(g)) : 0; }
static int run_gather(const GatherSpec& g, void* ws, int ws_packed, hipStream_t st) {
    if (!use_mfma(g)) return m1_direct_gather(g, st);
    return ws ? m1_mfma_gather(g, ws, ws_packed, st) : M1_ERR_WORKSPACE;
}

// ---- spec builders -------------------------------------------------------------------------------------------
// forward-type problems: the concat `d->src` is the CONTRACTION axis, `out` has all Cout channels
static GatherSpec fwd_spec(const m1_conv_desc_t* d, bool T, const float* w, const float* bias, void* y) {
    GatherSpec g{}; Geo q = T ? convT_geo(d) : conv_geo(d);
    g.nsrc = d->nsrc;
    for (int i = 0; i < d->nsrc; ++i) { g.src[i] = d->src[i].ptr; g.srcC[i] = d->src[i].C; }
    g.ID = d->D; g.IH = d->H; g.IW = d->W; g.out = y; g.OC = d->Cout; g.OD = q.OD; g.OH = q.OH; g.OW = q.OW; g.N = d->N;
    g.w = w; g.bias = bias; g.kd = d->kd; g.kh = d->kh; g.kw = d->kw; g.sd = d->sd; g.sh = d->sh; g.sw = d->sw;
    g.pd = q.pd; g.ph = q.ph; g.pw = q.pw; g.dtype = d->dtype;
    if (!T) { g.mode = 0; g.wST = (long long)d->Cin * d->Cout; g.wSC = d->Cout; g.wSO = 1; }     // w[tap][ci][co]
    else    { g.mode = 1; g.wST = (long long)d->Cout * d->Cin; g.wSC = 1; g.wSO = d->Cin; }      // w[tap][co][ci]
    return g;
}
// data-gradient problems: dy (Cout channels) is the contraction axis, one spec per concat member
static GatherSpec dgrad_spec(const m1_conv_desc_t* d, bool T, const float* w, const void* dy, void* dx, int member, int ch_off) {
    GatherSpec g{}; Geo q = T ? convT_geo(d) : conv_geo(d);
    g.nsrc = 1; g.src[0] = dy; g.srcC[0] = d->Cout;
    g.ID = q.OD; g.IH = q.OH; g.IW = q.OW; g.out = dx; g.OC = d->src[member].C; g.OD = d->D; g.OH = d->H; g.OW = d->W; g.N = d->N;
    g.w = w; g.bias = nullptr; g.oc_off = ch_off; g.kd = d->kd; g.kh = d->kh; g.kw = d->kw; g.sd = d->sd; g.sh = d->sh; g.sw = d->sw;
    g.pd = q.pd; g.ph = q.ph; g.pw = q.pw; g.dtype = d->dtype;
    if (!T) { g.mode = 1; g.wST = (long long)d->Cin * d->Cout; g.wSC = 1; g.wSO = d->Cout; }     // out = ci, contraction = co
    else    { g.mode = 0; g.wST = (long long)d->Cout * d->Cin; g.wSC = d->Cin; g.wSO = 1; }
    return g;
}

// the data gradient of ALL concat members as one problem: Cin output columns spread over the members' gradient tensors
// (GatherSpec::outs).  One launch instead of one per member: dY is gathered once per tile instead of once per member, 32-channel
// members stop running on 32-column tiles (the loader-bound shape), and a 5-member dense-skip concat costs 1 launch, not 5.
static GatherSpec dgrad_fused_spec(const m1_conv_desc_t* d, bool T, const float* w, const void* dy, void* const* dx, const int* accumulate) {
    GatherSpec g = dgrad_spec(d, T, w, dy, nullptr, 0, 0);
    g.OC = d->Cin; g.oc_off = 0; g.out = nullptr; g.accumulate = 0;
    g.nout = d->nsrc;
    for (int i = 0; i < d->nsrc; ++i) {
        g.outs[i] = dx ? dx[i] : nullptr; g.outC[i] = d->src[i].C; g.outAcc[i] = (accumulate && accumulate[i]) ? 1 : 0;
    }
    return g;
}
static bool dgrad_fused(const m1_conv_desc_t* d, bool T) {
    int en = M1_CFG("M1_DGRAD_FUSED", 1);
    if (!en || d->nsrc < 2) return false;
    const int seg = d->dtype == M1_BF16 ? 8 : 4;
    for (int i = 0; i < d->nsrc; ++i) if (d->src[i].C % seg) return false;
    // the wide, shallow layers (res0/res1: <= 64 dY channels, stride 1, >= 32,768 voxels) run on the halo-tile kernel, whose blocks
    // own one 32-column weight slice each: per-member launches are faster there (192->32 at res0: 0.76 vs 1.13 ms per step fused)
    const long long vox = (long long)d->N * d->D * d->H * d->W;
    int hf = M1_CFG("M1_DGRAD_FUSED_HALO", 0);
    if (!hf && d->dtype == M1_BF16 && d->Cout <= 64 && d->sd == 1 && d->sh == 1 && d->sw == 1 && vox >= 32768 && d->kd * d->kh * d->kw > 1) return false;
    return use_mfma(dgrad_fused_spec(d, T, nullptr, nullptr, nullptr, nullptr));
}

// ---- the plan of a forward / data gradient: its sub-problems and their places in the workspace ------------------------------
// One sub-problem of a forward (concat members [first, first + count) at channel ch_off of the contraction) or of a data gradient
// (the gradient of those members), and where its panel lives in `ws`.
struct GatherItem { int first, count, ch_off; size_t off, bytes; };
struct GatherPlan { bool T, fused; int n; GatherItem item[M1_MAX_SRC]; size_t stats_off, total; };
static void add_item(GatherPlan* p, int first, int count, int ch_off) { p->item[p->n++] = GatherItem{first, count, ch_off, 0, 0}; }
// A concat of wide members plus a tiny one that is not a whole 16-byte segment per voxel (the latent z of 1..3 channels in front of
// the feature map: networks.py:652-653, dec_hi = Conv3DTranspose([z, f])): as ONE problem the odd member takes the whole contraction
// off the LDS-DMA loader (515 -> 256 at res4: 144 us against 69 us for 512 -> 256).  Split: the run of 64-byte-aligned members is one
// conv that writes y (+ bias) on the fast path, the odd members follow as tiny convs that add into y.  Forward and transposed forward.
static bool odd_split(const m1_conv_desc_t* d, GatherPlan* p) {
    int en = M1_CFG("M1_ODD_SPLIT", 1);
    if (!en || g_force_direct || d->nsrc < 2) return false;
    const int seg = d->dtype == M1_BF16 ? 8 : 4, chunk = 4 * seg;
    int a0 = -1, a1 = -1, nodd = 0, call = 0;
    for (int i = 0; i < d->nsrc; ++i) {
        const int c = d->src[i].C;
        if (c % chunk == 0) { if (a0 < 0) a0 = i; a1 = i; call += c; }
        else if (c < seg) ++nodd;
        else return false;
    }
    if (!nodd || a0 < 0 || call < 64) return false;
    for (int i = a0; i <= a1; ++i) if (d->src[i].C % chunk) return false;        // the aligned members must be one run
    int off = 0, offs[M1_MAX_SRC];
    for (int i = 0; i < d->nsrc; ++i) { offs[i] = off; off += d->src[i].C; }
    p->n = 0;
    add_item(p, a0, a1 - a0 + 1, offs[a0]);
    if (a0 > 0) add_item(p, 0, a0, 0);
    if (a1 + 1 < d->nsrc) add_item(p, a1 + 1, d->nsrc - a1 - 1, offs[a1 + 1]);
    return true;
}
// Forward of a wide concat as one halo-tile launch per member group.  The halo-tile kernel (conv_halo.hip) stages an input tile
// once for all taps but holds at most 64 contraction channels; the dense-skip concats of the full model (160 channels at res0, 256
// at res1: networks.py:604-623) fell back to the per-tap gather (160->32 at res0: 470 us, bound by 9x re-reads from L2).  Split the
// members into groups of 8/16/32/64 channels: the first group writes y (+ bias), the others add into it in their epilogue, the last
// one also emits the InstanceNorm statistics of the sum.  Each group is an ordinary conv over its members with a channel offset
// into the weights (own panel, own job).
static bool fwd_groups(const m1_conv_desc_t* d, GatherPlan* p) {
    if (odd_split(d, p)) return true;
    const bool T = p->T;
    int en = M1_CFG("M1_HALO_GROUPS", 1);
    if (!en || T || g_force_direct || d->dtype != M1_BF16 || d->nsrc < 2 || d->Cin <= 64) return false;
    if (d->kd * d->kh * d->kw < 2) return false;
    Geo q = conv_geo(d);
    if (q.OW % 8 || (long long)d->N * q.OD * q.OH * q.OW < 32768) return false;
    auto ok = [](int c) { return c == 8 || c == 16 || c == 32 || c == 64; };
    p->n = 0; int cur = 0, off = 0;
    for (int i = 0; i < d->nsrc; ++i) {
        const int c = d->src[i].C;
        if (!ok(c)) return false;
        if (p->n > 0 && ok(cur + c) && cur + c <= 64) { p->item[p->n - 1].count++; cur += c; }
        else { add_item(p, i, 1, off); cur = c; }
        off += c;
    }
    return p->n >= 2;
}
// item k of a forward plan: the first writes y (+ bias), the others add into it (an ungrouped forward is its only item)
static GatherSpec fwd_item_spec(const m1_conv_desc_t* d, const GatherPlan& p, int k, const float* w, const float* bias, void* y) {
    const GatherItem& it = p.item[k];
    GatherSpec g = fwd_spec(d, p.T, w, k == 0 ? bias : nullptr, y);
    g.nsrc = it.count;
    for (int i = 0; i < g.nsrc; ++i) { g.src[i] = d->src[it.first + i].ptr; g.srcC[i] = d->src[it.first + i].C; }
    g.cc_off = it.ch_off;
    g.accumulate = k > 0 ? 1 : 0;
    return g;
}
// item k of a data-gradient plan: all members as one problem (fused) or member it.first alone
static GatherSpec dgrad_item_spec(const m1_conv_desc_t* d, const GatherPlan& p, int k, const float* w, const void* dy, void* const* dx,
                                  const int* accumulate) {
    if (p.fused) return dgrad_fused_spec(d, p.T, w, dy, dx, accumulate);
    const int i = p.item[k].first;
    GatherSpec g = dgrad_spec(d, p.T, w, dy, dx ? dx[i] : nullptr, i, p.item[k].ch_off);
    g.accumulate = accumulate && accumulate[i] ? 1 : 0;
    return g;
}
// THE layout of a forward (role 0) / data-gradient (role 1) workspace: the panels of the sub-problems back to back, in the order they
// run; behind them the statistics rows of a forward; 256 spare bytes.  A sub-problem the direct kernels take has no panel (0 bytes).
static GatherPlan plan_gather(const m1_conv_desc_t* d, bool T, int role) {
    GatherPlan p{}; p.T = T;
    if (role == 0) {
        if (!fwd_groups(d, &p)) { p.n = 0; add_item(&p, 0, d->nsrc, 0); }
    } else if (dgrad_fused(d, T)) {
        p.fused = true; add_item(&p, 0, d->nsrc, 0);
    } else {
        for (int i = 0, off = 0; i < d->nsrc; ++i) { add_item(&p, i, 1, off); off += d->src[i].C; }
    }
    size_t off = 0;
    for (int k = 0; k < p.n; ++k) {
        p.item[k].off = off;
        p.item[k].bytes = gather_ws_bytes(role == 0 ? fwd_item_spec(d, p, k, nullptr, nullptr, nullptr)
                                                    : dgrad_item_spec(d, p, k, nullptr, nullptr, nullptr, nullptr));
        off += p.item[k].bytes;
    }
    p.stats_off = off;
    if (role == 0) {
        const Geo q = T ? convT_geo(d) : conv_geo(d);
        off += align256(m1_stats_ws_floats(d->N, (long long)q.OD * q.OH * q.OW, d->Cout) * sizeof(float));
    }
    p.total = off + 256;
    return p;
}

// ---- stem weight gradient (Cin < 8: the image channels, networks.py:472) -----------------------------------------------
// 3 (or 2) input channels are 6 (4) bytes per voxel: no 16-byte segments for the LDS-DMA loaders, so this layer used to run
// on the generic per-tap kernel, re-reading dY once per tap (157 us at batch 2 = the slowest weight gradient of the step for
// 0.2 % of its flops).  Instead: X -> X8 (zero-padded to 8 channels, one 16-byte segment per voxel) in the workspace, the
// tap-fused kernel on (X8, dY) into a scratch gradient with 8 input rows per tap, and a fold of its first Cin rows.
static bool stem_wanted(const m1_conv_desc_t* d, bool T) {
    int en = M1_CFG("M1_STEM_TF", 1);
    // (fp32: the same with 4 channels = one 16-byte segment per voxel, on the fp32 tap-fused kernel)
    return en && !T && !g_force_direct && d->nsrc == 1 && d->src[0].C < (d->dtype == M1_BF16 ? 8 : 4) && d->Cin == d->src[0].C;
}
// Zero fill as a KERNEL.  hipMemsetAsync on a capturing stream becomes a memset node of the step's hipGraph, and on this ROCm release
// a replayed graph does not keep a memset node ordered between the kernel nodes around it (round 5: from the third replay on, the
// padded-stem weight gradient -- zero r8, accumulate into it, read it -- differed from run to run, in order on ONE stream; eager
// launches never; tools/probes/graph_memset_probe.py).  M1_MEMSET_KERNEL=0 restores the memset (the reproducer of that finding).
__global__ void __launch_bounds__(256) m1_zero_kernel(unsigned* __restrict__ head, int nhead, uint4* __restrict__ p, long long n16,
                                                      unsigned* __restrict__ tail, int ntail) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n16; i += (long long)gridDim.x * 256) p[i] = make_uint4(0, 0, 0, 0);
    if (blockIdx.x == 0 && (int)threadIdx.x < nhead) head[threadIdx.x] = 0u;
    if (blockIdx.x == 0 && (int)threadIdx.x < ntail) tail[threadIdx.x] = 0u;
}
// Any 4-byte aligned buffer of a multiple of 4 bytes (dw / db at an odd float offset of a caller's flat gradient buffer): up to three
// dwords in front of the first 16-byte boundary, the 16-byte body, up to three dwords behind it -- always a kernel, never a memset
// node (round-5 advisor: the old fallback to hipMemsetAsync for unaligned pointers brought the replay defect back without an error).
// M1_MEMSET_KERNEL=0 restores the memset = the reproducer of that defect.
static int m1_zero_async(void* p, size_t bytes, hipStream_t st) {
    if (!bytes) return M1_OK;
    if (!M1_CFG("M1_MEMSET_KERNEL", 1)) return hipMemsetAsync(p, 0, bytes, st) == hipSuccess ? M1_OK : M1_ERR_LAUNCH;
    if (((uintptr_t)p & 3) || (bytes & 3)) return M1_ERR_BAD_ARG;
    size_t ndw = bytes >> 2;
    int nhead = (int)(((16 - ((uintptr_t)p & 15)) & 15) >> 2);
    if ((size_t)nhead > ndw) nhead = (int)ndw;
    unsigned* head = (unsigned*)p;
    unsigned char* body = (unsigned char*)p + 4 * (size_t)nhead;
    const long long n16 = (long long)((ndw - nhead) >> 2);
    const int ntail = (int)((ndw - nhead) & 3);
    long long g = (n16 + 255) / 256; if (g > 2048) g = 2048; if (g < 1) g = 1;
    hipLaunchKernelGGL(m1_zero_kernel, dim3((unsigned)g), dim3(256), 0, st, head, nhead, (uint4*)body, n16, (unsigned*)(body + (n16 << 4)), ntail);
    return m1_check_launch();
}
__global__ void __launch_bounds__(256) stem_pad8_kernel(const unsigned short* __restrict__ x, uint4* __restrict__ x8, long long nvox, int C) {
    for (long long v = (long long)blockIdx.x * 256 + threadIdx.x; v < nvox; v += (long long)gridDim.x * 256) {
        unsigned short e[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        for (int c = 0; c < C; ++c) e[c] = x[v * C + c];
        uint4 o;
        o.x = e[0] | ((unsigned)e[1] << 16); o.y = e[2] | ((unsigned)e[3] << 16);
        o.z = e[4] | ((unsigned)e[5] << 16); o.w = e[6] | ((unsigned)e[7] << 16);
        x8[v] = o;
    }
}
__global__ void __launch_bounds__(256) stem_pad4f_kernel(const float* __restrict__ x, float4* __restrict__ x4, long long nvox, int C) {
    for (long long v = (long long)blockIdx.x * 256 + threadIdx.x; v < nvox; v += (long long)gridDim.x * 256) {
        float e[4] = {0.f, 0.f, 0.f, 0.f};
        for (int c = 0; c < C; ++c) e[c] = x[v * C + c];
        x4[v] = make_float4(e[0], e[1], e[2], e[3]);
    }
}
// dw[t][ci][co] += r8[t][ci][co], ci < Cin   (dw was zeroed above when accumulate == 0); CP = padded channels of r8 (8 / 4)
__global__ void __launch_bounds__(256) stem_fold_kernel(const float* __restrict__ r8, float* __restrict__ dw, int taps, int Cin, int Cout, int CP) {
    const int n = taps * Cin * Cout;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
        const int co = i % Cout, ci = (i / Cout) % Cin, t = i / (Cout * Cin);
        dw[i] += r8[((size_t)t * CP + ci) * Cout + co];
    }
}

// Scratch for the per-split partial copies of a weight gradient (+ bias sums): compact copies of ONE concat member's block
// ([tap][C_member][Cout] + Cout floats), up to M1_WG_MAX_COPIES of them, at most 64 MB.  It lives in the caller's wgrad workspace -- one region
// per call, so weight gradients that run concurrently on different streams never share it (the library keeps no device memory
// of its own).  All weight-gradient kernels fold copies in a fixed order instead of using floating-point atomics.
static size_t wgrad_rx_bytes(const m1_conv_desc_t* d) {
    const size_t taps = (size_t)d->kd * d->kh * d->kw;
    size_t cmax = 8;                                           // (the padded stem runs as an 8-channel member)
    for (int i = 0; i < d->nsrc; ++i) if ((size_t)d->src[i].C > cmax) cmax = d->src[i].C;
    const size_t other = cmax > (size_t)d->Cout ? cmax : (size_t)d->Cout;      // (transposed conv: the roles of the two sides swap)
    const size_t stride = (size_t)m1_wg_copy_floats(taps, cmax, d->Cout, other);
    size_t b = M1_WG_MAX_COPIES * stride * sizeof(float);
    const long long cap = (long long)M1_CFG("M1_WG_RX_MB", 64) << 20;
    if (b > (size_t)cap) b = (size_t)cap;
    if (b < 2 * stride * sizeof(float)) b = 2 * stride * sizeof(float);
    return align256(b);
}
// THE layout of a weight-gradient workspace (byte offsets): the reduction scratch of the bias gradient, the stem's padded input x8
// and scratch gradient r8 (stem_wanted only), then one partial-copy region of rx_floats per concat member: with deferred folds
// (m1_wgrad_defer) the copies of member i must survive the kernels of member i+1.
struct WgradWs { size_t reduce_bytes, x8, r8, rx, total; long long rx_floats; };
static WgradWs wgrad_ws(const m1_conv_desc_t* d, bool T) {
    const Geo q = T ? convT_geo(d) : conv_geo(d);
    WgradWs w{};
    w.reduce_bytes = align256(m1_reduce_ws_floats(d->N, (long long)q.OD * q.OH * q.OW, d->Cout, 1) * sizeof(float)) + 256;
    w.x8 = w.r8 = w.rx = w.reduce_bytes;
    if (stem_wanted(d, T)) {                             // x8: 16 bytes per voxel; r8: 8 input rows per tap (fp32 uses 4 of them)
        w.r8 = w.x8 + align256((size_t)d->N * d->D * d->H * d->W * 16);
        w.rx = w.r8 + align256((size_t)d->kd * d->kh * d->kw * 8 * d->Cout * sizeof(float));
    }
    const size_t rx_bytes = wgrad_rx_bytes(d);
    w.rx_floats = (long long)(rx_bytes / sizeof(float));
    w.total = w.rx + rx_bytes * (size_t)d->nsrc;
    return w;
}

// ---- workspace query ---------------------------------------------------------------------------------------------
extern "C" size_t m1_conv_ws_bytes(const m1_conv_desc_t* d, int transposed, int role) {
    if (!desc_ok(d)) return 0;
    return role == 0 || role == 1 ? plan_gather(d, transposed != 0, role).total : wgrad_ws(d, transposed != 0).total;
}

// ---- packed-weight panel records ----------------------------------------------------------------------------------
// Device addresses of the pack-job records inside `ws`: one per matrix-core panel of the role's plan.  A record is filled by the
// first (lazy) pack of its panel; m1_pack_batch re-runs filled records.
extern "C" int m1_conv_pack_jobs(const m1_conv_desc_t* d, int transposed, int role, void* ws, void** jobs_out) {
    if (!desc_ok(d) || !ws || !jobs_out || (role != 0 && role != 1)) return 0;
    const GatherPlan p = plan_gather(d, transposed != 0, role);
    int n = 0;
    for (int k = 0; k < p.n; ++k) if (p.item[k].bytes) jobs_out[n++] = at(ws, p.item[k].off);
    return n;
}
extern "C" int m1_pack_batch(const void* const* jobs_dev, const int* block_prefix_dev, int njobs, int total_blocks, void* stream) {
    if (m1_debug_skip("pack")) return M1_OK;
    if (njobs < 0 || (njobs > 0 && !jobs_dev) || (block_prefix_dev && total_blocks < njobs)) return M1_ERR_BAD_ARG;
    M1ProfScope ps("pack_batch", 0.0, 0.0, (hipStream_t)stream);
    return m1_pack_batch_internal(jobs_dev, block_prefix_dev, njobs, total_blocks, (hipStream_t)stream);
}

// ---- Conv3D ------------------------------------------------------------------------------------------------------
// the items of the forward plan in order; the last one also emits the InstanceNorm statistics of the finished y
static int fwd_common(const m1_conv_desc_t* d, bool T, const float* w, const float* bias, void* y, float* stats, void* ws, int ws_packed,
                      hipStream_t st) {
    if (stats && !ws) return M1_ERR_WORKSPACE;
    const GatherPlan p = plan_gather(d, T, 0);
    // without a workspace there are no groups: the whole concat as one problem (the direct kernels take it, or M1_ERR_WORKSPACE)
    if (!ws && p.n > 1) return run_gather(fwd_spec(d, T, w, bias, y), nullptr, ws_packed, st);
    for (int k = 0; k < p.n; ++k) {
        GatherSpec g = fwd_item_spec(d, p, k, w, bias, y);
        const bool emit = stats && k == p.n - 1;
        if (emit) { g.stats_out = stats; g.stats_eps = 1e-3f; g.stats_ws = reinterpret_cast<float*>(at(ws, p.stats_off)); }   // tfa InstanceNormalization epsilon
        int rc = run_gather(g, at(ws, p.item[k].off), ws_packed, st); if (rc) return rc;
        // direct path: conv, then the stand-alone reduction.  (Known gap, kept as it was: a GROUPED forward that the matrix-core
        // kernels decline -- more than 27 taps -- runs its groups on the direct kernels and writes no statistics.)
        if (emit && p.n == 1 && !use_mfma(g))
            return m1_stats_internal(y, d->N, (long long)g.OD * g.OH * g.OW, d->Cout, d->dtype, 1e-3f, stats, g.stats_ws, st);
    }
    return M1_OK;
}
extern "C" int m1_conv3d_fwd(const m1_conv_desc_t* d, const float* w, const float* bias, void* y, float* stats, void* ws,
                             int ws_packed, void* stream) {
    if (m1_debug_skip("conv_fwd")) return M1_OK;
    if (!desc_ok(d) || !w || !y) return M1_ERR_BAD_ARG;
    M1ProfScope ps(prof_name("conv3d_fwd", d).s, 2.0 * conv_macs(d, false), conv_bytes(d, false), (hipStream_t)stream);
    return fwd_common(d, false, w, bias, y, stats, ws, ws_packed, (hipStream_t)stream);
}
// ---- conv1 || conv4 of an SE block (network_blocks.py:53,64: same input, same kernel size and strides) as ONE problem --------
// Forward: one conv with C1 + C4 output columns, written to two tensors ([y1 | y4]) with their own bias vectors and InstanceNorm
// statistics: the im2col operand is gathered once, and the C1 = F/4 columns that alone would run on a loader-bound 32-column
// tile ride on the 128-column tiles of their big twin.  Data gradient: one contraction over the virtual concat [dy1 | dy4] with a
// panel packed from both weight tensors (no read-modify-write of dx by a second launch).  d->Cout = C1 + C4.
static bool pair_ok(const m1_conv_desc_t* d, int C1) {
    if (!desc_ok(d) || g_force_direct) return false;     // (desc_ok: d may be null)
    const int seg = d->dtype == M1_BF16 ? 8 : 4;
    if (C1 <= 0 || C1 >= d->Cout || C1 % seg || (d->Cout - C1) % seg) return false;
    for (int i = 0; i < d->nsrc; ++i) if (d->src[i].C % seg) return false;
    return true;
}
// The pair's problems live in the workspace of the plain conv with C1 + C4 outputs (the caller sizes `ws` from d): one item of that
// conv's plan, with the second weight tensor added.  false: not as a pair (the shape runs as a grouped forward / a data gradient
// per member, or the matrix-core kernel does not take it).  The pointers may be null (m1_conv3d_pair_supported).
static bool pair_fwd_spec(const m1_conv_desc_t* d, int C1, const float* w1, const float* b1, const float* w4, const float* b4, void* y1,
                          void* y4, float* stats1, float* stats4, void* ws, GatherSpec* out) {
    const GatherPlan p = plan_gather(d, false, 0);
    if (p.n != 1) return false;
    const int C4 = d->Cout - C1;
    GatherSpec g = fwd_item_spec(d, p, 0, w1, b1, nullptr);
    g.wST = (long long)d->Cin * C1; g.wSC = C1; g.wSO = 1;
    g.w2 = w4; g.w2ST = (long long)d->Cin * C4; g.w2SC = C4; g.w2SO = 1; g.oc_split = C1; g.bias2 = b4;
    g.nout = 2; g.outs[0] = y1; g.outC[0] = C1; g.outAcc[0] = 0; g.outs[1] = y4; g.outC[1] = C4; g.outAcc[1] = 0;
    if (stats1) { g.stats_out = stats1; g.stats_out2 = stats4; g.stats_eps = 1e-3f; g.stats_ws = reinterpret_cast<float*>(at(ws, p.stats_off)); }
    *out = g;
    return m1_mfma_supported(g) && gather_ws_bytes(g) == p.item[0].bytes;      // (the statistics rows start behind the pair's panel)
}
static bool pair_dgrad_spec(const m1_conv_desc_t* d, int C1, const float* w1, const float* w4, const void* dy1, const void* dy4,
                            void* const* dx, const int* accumulate, GatherSpec* out) {
    const GatherPlan p = plan_gather(d, false, 1);
    if (p.n != 1) return false;
    const int C4 = d->Cout - C1;
    GatherSpec g = dgrad_item_spec(d, p, 0, w1, dy1, dx, accumulate);
    g.nsrc = 2; g.src[0] = dy1; g.srcC[0] = C1; g.src[1] = dy4; g.srcC[1] = C4;
    g.wST = (long long)d->Cin * C1; g.wSC = 1; g.wSO = C1;
    g.w2 = w4; g.w2ST = (long long)d->Cin * C4; g.w2SC = 1; g.w2SO = C4; g.c_split = C1;
    *out = g;
    // The pair's panel must FIT the plan's (nothing of a data-gradient workspace lies behind it).  Equal it need not be: the plan
    // sizes for dy as one tensor of C1 + C4 channels, and conv_t3's 32-channel rule may hold for that sum but not for C1 and C4
    // (48 + 144): the plan then also sizes for a kernel that the pair does not take.
    return m1_mfma_supported(g) && gather_ws_bytes(g) <= p.item[0].bytes;
}
extern "C" int m1_conv3d_pair_fwd(const m1_conv_desc_t* d, const float* w1, const float* b1, const float* w4, const float* b4, int C1,
                                  void* y1, void* y4, float* stats1, float* stats4, void* ws, int ws_packed, void* stream) {
    if (m1_debug_skip("conv_fwd")) return M1_OK;
    if (!d || !w1 || !w4 || !y1 || !y4 || !ws || (stats1 == nullptr) != (stats4 == nullptr)) return M1_ERR_BAD_ARG;
    GatherSpec g;
    if (!pair_ok(d, C1) || !pair_fwd_spec(d, C1, w1, b1, w4, b4, y1, y4, stats1, stats4, ws, &g)) return M1_ERR_UNSUPPORTED;
    M1ProfScope ps(prof_name("conv3d_fwd", d).s, 2.0 * conv_macs(d, false), conv_bytes(d, false), (hipStream_t)stream);
    return m1_mfma_gather(g, ws, ws_packed, (hipStream_t)stream);
}
extern "C" int m1_conv3d_pair_dgrad(const m1_conv_desc_t* d, const float* w1, const float* w4, int C1, const void* dy1, const void* dy4,
                                    void* const* dx, const int* accumulate, void* ws, int ws_packed, void* stream) {
    if (m1_debug_skip("conv_dgrad")) return M1_OK;
    if (!d || !w1 || !w4 || !dy1 || !dy4 || !dx || !ws) return M1_ERR_BAD_ARG;
    if (!pair_ok(d, C1)) return M1_ERR_UNSUPPORTED;
    M1ProfScope ps(prof_name("conv3d_dgrad", d).s, 2.0 * conv_macs(d, false), conv_bytes(d, false), (hipStream_t)stream);
    if (d->nsrc == 1 && !dx[0]) return M1_OK;             // (a single unwanted gradient is answered before the shape is judged)
    GatherSpec g;
    if (!pair_dgrad_spec(d, C1, w1, w4, dy1, dy4, dx, accumulate, &g)) return M1_ERR_UNSUPPORTED;
    bool any = false;
    for (int i = 0; i < d->nsrc; ++i) any |= dx[i] != nullptr;
    return any ? m1_mfma_gather(g, ws, ws_packed, (hipStream_t)stream) : M1_OK;
}

// 1 when BOTH m1_conv3d_pair_fwd and m1_conv3d_pair_dgrad take this shape (neither would return M1_ERR_UNSUPPORTED): the caller
// decides between the pair and the two single convs BEFORE it builds its autograd graph (a refusal in the middle of a backward pass
// has no fallback).  The same gates as the two entry points: pair_ok and their spec builders.
extern "C" int m1_conv3d_pair_supported(const m1_conv_desc_t* d, int C1) {
    GatherSpec g;
    return pair_ok(d, C1) && pair_fwd_spec(d, C1, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, &g) &&
           pair_dgrad_spec(d, C1, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, &g);
}

extern "C" int m1_convT3d_fwd(const m1_conv_desc_t* d, const float* w, const float* bias, void* y, void* ws, int ws_packed,
                              void* stream) {
    if (m1_debug_skip("conv_fwd")) return M1_OK;
    if (!desc_ok(d) || !w || !y) return M1_ERR_BAD_ARG;
    M1ProfScope ps(prof_name("convT3d_fwd", d).s, 2.0 * conv_macs(d, true), conv_bytes(d, true), (hipStream_t)stream);
    return fwd_common(d, true, w, bias, y, nullptr, ws, ws_packed, (hipStream_t)stream);
}
// the items of the data-gradient plan whose members' gradients are wanted, each on its own panel of ws (cacheable)
static int dgrad_common(const m1_conv_desc_t* d, bool T, const float* w, const void* dy, void* const* dx, const int* accumulate,
                        void* ws, int ws_packed, hipStream_t st) {
    const GatherPlan p = plan_gather(d, T, 1);
    for (int k = 0; k < p.n; ++k) {
        const GatherItem& it = p.item[k];
        bool any = false;
        for (int i = it.first; i < it.first + it.count; ++i) any |= dx[i] != nullptr;
        if (!any) continue;
        int rc = run_gather(dgrad_item_spec(d, p, k, w, dy, dx, accumulate), at(ws, it.off), ws_packed, st); if (rc) return rc;
    }
    return M1_OK;
}
extern "C" int m1_conv3d_dgrad(const m1_conv_desc_t* d, const float* w, const void* dy, void* const* dx, const int* accumulate,
                               void* ws, int ws_packed, void* stream) {
    if (m1_debug_skip("conv_dgrad")) return M1_OK;
    if (!desc_ok(d) || !w || !dy || !dx) return M1_ERR_BAD_ARG;
    M1ProfScope ps(prof_name("conv3d_dgrad", d).s, 2.0 * conv_macs(d, false), conv_bytes(d, false), (hipStream_t)stream);
    return dgrad_common(d, false, w, dy, dx, accumulate, ws, ws_packed, (hipStream_t)stream);
}
// Data gradient of a single-input Conv3D whose input is a = lrelu(IN(x)) (conv2 / conv3 of an SE block, network_blocks.py:54-59):
// the kernel that writes d(a) also emits the per-tile sums the InstanceNorm backward needs ({sum dy, sum dy*xh} per sample and
// channel) into `partial` [N][*nparts][Cin][2].  *nparts = 0: the kernel that took the shape has no such epilogue -- d(a) is
// complete, the caller runs m1_instnorm_bwd instead of m1_instnorm_bwd_partials.
// rows per sample the partial buffer of m1_conv3d_dgrad_inbwd must hold (`partial` = N * rows * Cin * 2 floats): the most any kernel
// behind it writes -- one row per epilogue tile (>= 64 voxels each) or one per chunk of the split-K finish reduction
extern "C" int m1_conv3d_dgrad_inbwd_rows(const m1_conv_desc_t* d) {
    if (!desc_ok(d)) return 0;
    const long long V = (long long)d->D * d->H * d->W;
    const long long tiles = m1_stats_rows_cap(V), chunks = m1_red_nchunks(V, d->Cin, d->N);     // (>= one row per 64 voxels)
    const long long r = tiles > chunks ? tiles : chunks;
    return r > 0x3fffffff ? 0x3fffffff : (int)r;
}
extern "C" int m1_conv3d_dgrad_inbwd(const m1_conv_desc_t* d, const float* w, const void* dy, void* da, const void* x, const float* stats,
                                     const float* gamma, const float* beta, float slope, float* partial, int partial_rows, int* nparts,
                                     void* ws, int ws_packed, void* stream) {
    if (!desc_ok(d) || !w || !dy || !da || !x || !stats || !gamma || !beta || !partial || !nparts || d->nsrc != 1 || partial_rows < 0) return M1_ERR_BAD_ARG;
    M1ProfScope ps(prof_name("conv3d_dgrad", d).s, 2.0 * conv_macs(d, false), conv_bytes(d, false), (hipStream_t)stream);
    *nparts = 0;
    if (g_force_direct) { void* dxs[1] = {da}; int acc0[1] = {0}; return dgrad_common(d, false, w, dy, dxs, acc0, ws, ws_packed, (hipStream_t)stream); }
    GatherSpec g = dgrad_spec(d, false, w, dy, da, 0, 0);      // (one member: the only item of its plan, panel at offset 0)
    g.ib_x = x; g.ib_stats = stats; g.ib_gamma = gamma; g.ib_beta = beta; g.ib_slope = slope; g.ib_partial = partial; g.ib_nparts = nparts; g.ib_cap = partial_rows;
    return run_gather(g, ws, ws_packed, (hipStream_t)stream);
}
extern "C" int m1_convT3d_dgrad(const m1_conv_desc_t* d, const float* w, const void* dy, void* const* dx, const int* accumulate,
                                void* ws, int ws_packed, void* stream) {
    if (m1_debug_skip("conv_dgrad")) return M1_OK;
    if (!desc_ok(d) || !w || !dy || !dx) return M1_ERR_BAD_ARG;
    M1ProfScope ps(prof_name("convT3d_dgrad", d).s, 2.0 * conv_macs(d, true), conv_bytes(d, true), (hipStream_t)stream);
    return dgrad_common(d, true, w, dy, dx, accumulate, ws, ws_packed, (hipStream_t)stream);
}

// ---- weight gradients ------------------------------------------------------------------------------------------
// The weight gradient of concat member i, whose channels start at `off` of the concat, inside the whole gradient dw; db: the bias
// gradient rides along (Conv3D only); rx: this member's partial-copy region.  The padded stem is member 0 of a copy of the
// descriptor whose only member is the padded input.
static WgradSpec wgrad_spec(const m1_conv_desc_t* d, bool T, const Geo& q, int i, int off, const void* dy, float* dw, float* db, float* rx,
                            long long rx_floats) {
    WgradSpec g{};
    g.N = d->N; g.R = dw; g.kd = d->kd; g.kh = d->kh; g.kw = d->kw; g.sd = d->sd; g.sh = d->sh; g.sw = d->sw;
    g.pd = q.pd; g.ph = q.ph; g.pw = q.pw; g.dtype = d->dtype;
    g.rx = rx; g.rx_floats = rx_floats;
    if (!T) {   // dw[tap][ci][co] = sum X[v*s+tap-p][ci] * dY[v][co]
        g.A = d->src[i].ptr; g.CA = d->src[i].C; g.AD = d->D; g.AH = d->H; g.AW = d->W;
        g.B = dy; g.CB = d->Cout; g.BD = q.OD; g.BH = q.OH; g.BW = q.OW;
        g.RT = (long long)d->Cin * d->Cout; g.RSA = d->Cout; g.a_off = off; g.b_off = 0;
        if (db) { g.bsum = db; g.bsum_tap = (q.pd * d->kh + q.ph) * d->kw + q.pw; }
    } else {    // dw[tap][co][ci] = sum dOut[i*s+tap-pb][co] * In[i][ci]
        g.A = dy; g.CA = d->Cout; g.AD = q.OD; g.AH = q.OH; g.AW = q.OW;
        g.B = d->src[i].ptr; g.CB = d->src[i].C; g.BD = d->D; g.BH = d->H; g.BW = d->W;
        g.RT = (long long)d->Cout * d->Cin; g.RSA = d->Cin; g.a_off = 0; g.b_off = off;
    }
    return g;
}
static bool tf_wanted(const WgradSpec& g) {
    int maxc = M1_CFG("M1_TF_MAXC", 128);
    // 32x32 channel tiles re-read dY once per 32 input channels and X once per 32 output channels: a win while the OUTPUT side
    // is narrow (conv1 of an SE block: F/4 <= 32 channels -- 512->32 at res2: 1.70 -> 1.08 ms per step), a loss beyond (512->128: 2x slower)
    if (g.CA > 64 && g.CB > 32) return false;
    return g.CA <= maxc && g.CB <= maxc && m1_tf_wgrad_supported(g);
}
// What a rung of the ladder sees besides the member's spec.  run: the members from this one on that have its channel count (a
// transposed conv has its members on the dY-less side: always 1), with their tensors and channel offsets for the kernels that
// take such a run in ONE launch.
struct WgCall {
    bool T; int run; const void* Am[M1_MAX_SRC]; int aoffs[M1_MAX_SRC];
    long long nw; int nbias; long long rx_floats; hipStream_t st;
    const char** took;         // for M1_WG_LOG: the rung's name, unless the rung names the kernel it chose
};
static int equal_run(const m1_conv_desc_t* d, int i) {
    int n = 1;
    while (i + n < d->nsrc && d->src[i + n].C == d->src[i].C) ++n;
    return n;
}
// THE order in which the weight-gradient kernels are tried for a member (wgrad_common walks it).  A rung whose gate holds runs; it
// may still decline (M1_ERR_UNSUPPORTED / M1_ERR_WORKSPACE: nothing launched), then the next one is asked.  whole_run: the rung
// consumes c.run members, else one.  m1_set_force_direct leaves only the rungs marked `forced`.
struct WgRung {
    const char* name; bool whole_run, forced;
    bool (*gate)(const WgradSpec& g, const WgCall& c);
    int (*run)(const WgradSpec& g, const WgCall& c);
};
static const WgRung WG_LADDER[] = {
    // >= 64 channels on both sides: the 64x64-tile tap-fused kernel on 32x32x16 MFMAs, one launch for a run of equal-width
    // members (dY staged once per kd slice for all of them, wgrad_t3.hip)
    {"t3", true, false, [](const WgradSpec& g, const WgCall&) { return g.rx && m1_t3_wgrad_supported(g); },
     [](const WgradSpec& g, const WgCall& c) { return m1_t3_wgrad(g, c.nw, c.nbias, c.st, c.run, c.Am, c.aoffs, c.rx_floats); }},
    {"pwf", false, false, [](const WgradSpec& g, const WgCall& c) { return g.rx && g.dtype == M1_F32 && !c.T && m1_pwf_wgrad_supported(g); },
     [](const WgradSpec& g, const WgCall& c) { return m1_pwf_wgrad(g, c.nw, c.nbias, c.st); }},
    // fp32 layers the 64x64-tile kernel does not take (few channels on a side): the 32x32-tile tap-fused fp32 kernel
    {"t3s", false, false, [](const WgradSpec& g, const WgCall&) { return g.rx && g.dtype == M1_F32 && m1_t3s_wgrad_supported(g); },
     [](const WgradSpec& g, const WgCall& c) { return m1_t3s_wgrad(g, c.nw, c.nbias, c.st); }},
    // a run of members with the same channel count on the tap-fused kernel: ONE launch (blockIdx.z = member)
    {"tf-multi", true, false,
     [](const WgradSpec& g, const WgCall& c) { int multi = M1_CFG("M1_TF_MULTI", 1); return multi && !c.T && g.rx && tf_wanted(g) && c.run > 1; },
     [](const WgradSpec& g, const WgCall& c) { return m1_tf_wgrad_multi(g, c.nw, c.nbias, c.st, c.run, c.Am, c.aoffs, c.rx_floats); }},
    {"tf", false, false, [](const WgradSpec& g, const WgCall&) { return tf_wanted(g); },
     [](const WgradSpec& g, const WgCall& c) { return m1_tf_wgrad(g, c.nw, c.nbias, c.st); }},
    // the terminal choice: whatever it answers is the member's result
    {"terminal", false, true, [](const WgradSpec&, const WgCall&) { return true; },
     [](const WgradSpec& g, const WgCall& c) {
         if (g_force_direct == 2 && m1_skinny_wgrad_supported(g)) { *c.took = "skinny"; return m1_skinny_wgrad(g, c.st); }   // test hook for that kernel
         if (!g_force_direct && m1_tap_wgrad_supported(g)) { *c.took = "tap"; return m1_tap_wgrad(g, c.nw, c.nbias, c.st); }
         if (!g_force_direct && m1_mfma_wgrad_supported(g)) { *c.took = "mfma"; return m1_mfma_wgrad_ex(g, c.nw, c.nbias, c.st); }
         *c.took = "direct"; return m1_direct_wgrad(g, c.st);
     }},
};
static int wgrad_common(const m1_conv_desc_t* d, bool T, const void* dy, float* dw, float* db, void* ws, hipStream_t st,
                        int accumulate) {
    Geo q = T ? convT_geo(d) : conv_geo(d);
    const size_t nw = (size_t)d->kd * d->kh * d->kw * d->Cin * d->Cout;
    if (!accumulate && m1_zero_async(dw, nw * sizeof(float), st) != M1_OK) return M1_ERR_LAUNCH;
    // Conv3D bias gradient rides on the matrix-core wgrad of the first concat member (all-ones fragment); the
    // transposed conv (its dOut is the SHIFTED operand) and the direct path keep the separate column-sum pass
    const bool fuse_db = db && !T && !g_force_direct;
    if (fuse_db && !accumulate && m1_zero_async(db, (size_t)d->Cout * sizeof(float), st) != M1_OK) return M1_ERR_LAUNCH;
    const int nbias = fuse_db ? d->Cout : 0;
    const WgradWs L = wgrad_ws(d, T);
    float* const rx = reinterpret_cast<float*>(at(ws, L.rx));        // partial-copy scratch: the tail of the caller's workspace
    const long long rx_floats = ws ? L.rx_floats : 0;
    if (stem_wanted(d, T) && ws) {
        const bool f32 = d->dtype == M1_F32;
        const int CP = f32 ? 4 : 8;                       // padded channels: one 16-byte segment per voxel
        uint4* x8 = reinterpret_cast<uint4*>(at(ws, L.x8));
        float* r8 = reinterpret_cast<float*>(at(ws, L.r8));
        m1_conv_desc_t dp = *d; dp.Cin = CP; dp.src[0].ptr = x8; dp.src[0].C = CP;       // the padded member, its gradient in r8
        const WgradSpec g = wgrad_spec(&dp, false, q, 0, 0, dy, r8, fuse_db ? db : nullptr, rx, rx_floats);
        if (f32 ? m1_t3s_wgrad_supported(g) : m1_tf_wgrad_supported(g)) {
            const int taps = d->kd * d->kh * d->kw, Cin = d->Cin;
            const long long nvox = (long long)d->N * d->D * d->H * d->W;
            const size_t nw8 = (size_t)taps * CP * d->Cout;
            if (m1_zero_async(r8, nw8 * sizeof(float), st) != M1_OK) return M1_ERR_LAUNCH;
            long long pb = (nvox + 255) / 256; if (pb > 8192) pb = 8192;
            if (f32) hipLaunchKernelGGL(stem_pad4f_kernel, dim3((unsigned)pb), dim3(256), 0, st, (const float*)d->src[0].ptr, reinterpret_cast<float4*>(x8), nvox, Cin);
            else hipLaunchKernelGGL(stem_pad8_kernel, dim3((unsigned)pb), dim3(256), 0, st, (const unsigned short*)d->src[0].ptr, x8, nvox, Cin);
            const int was = m1_fold_defer_set(0);      // (stem_fold_kernel below reads the folded 8-channel gradient)
            int rc = f32 ? m1_t3s_wgrad(g, (long long)nw8, nbias, st) : m1_tf_wgrad(g, (long long)nw8, nbias, st);
            m1_fold_defer_set(was);
            if (rc == M1_OK) {
                m1_note_plan("stem:cp=%d", CP);
                hipLaunchKernelGGL(stem_fold_kernel, dim3((taps * Cin * d->Cout + 255) / 256), dim3(256), 0, st, r8, dw, taps, Cin, d->Cout, CP);
                return m1_check_launch();
            }
            if (rc != M1_ERR_UNSUPPORTED && rc != M1_ERR_WORKSPACE) return rc;      // declined: nothing launched, take the generic path
        }
    }
    const int wlog = M1_CFG("M1_WG_LOG", 0);
    for (int i = 0, off = 0; i < d->nsrc;) {
        WgCall c{};
        c.T = T; c.nw = (long long)nw; c.nbias = nbias; c.rx_floats = rx_floats; c.st = st;
        c.run = T ? 1 : equal_run(d, i);
        for (int m = 0, o = off; m < c.run; ++m) { c.Am[m] = d->src[i + m].ptr; c.aoffs[m] = o; o += d->src[i + m].C; }
        const WgradSpec g = wgrad_spec(d, T, q, i, off, dy, dw, fuse_db && i == 0 ? db : nullptr, rx ? rx + (long long)i * rx_floats : nullptr,
                                       rx_floats);
        int rc = M1_ERR_UNSUPPORTED, used = 1;
        for (const WgRung& r : WG_LADDER) {
            if ((g_force_direct && !r.forced) || !r.gate(g, c)) continue;
            const char* took = r.name; c.took = &took;
            rc = r.run(g, c); used = r.whole_run ? c.run : 1;
            if (wlog) fprintf(stderr, "wgrad %s N%d B %dx%dx%d CA %d x%d CB %d k%d%d%d s%d%d%d -> %s rc %d\n", T ? "convT" : "conv", g.N, g.BD,
                              g.BH, g.BW, g.CA, used, g.CB, g.kd, g.kh, g.kw, g.sd, g.sh, g.sw, took, rc);
            if (rc != M1_ERR_UNSUPPORTED && rc != M1_ERR_WORKSPACE) break;      // taken or a hard error; else declined: the next rung
            m1_note_plan("decline:%s rc=%d", r.name, rc);
        }
        if (rc) return rc;
        for (int m = 0; m < used; ++m) off += d->src[i++].C;
    }
    if (db && !fuse_db) {
        if (!ws) return M1_ERR_WORKSPACE;
        const long long Vd = (long long)q.OD * q.OH * q.OW;
        if (!g_force_direct && m1_colsum_defer(dy, d->N, Vd, d->Cout, d->dtype, db, (float*)ws, accumulate)) return M1_OK;
        return m1_colsum_internal(dy, d->N, Vd, d->Cout, d->dtype, db, (float*)ws, st, accumulate);
    }
    return M1_OK;
}
extern "C" int m1_conv3d_wgrad(const m1_conv_desc_t* d, const void* dy, float* dw, float* db, void* ws, int accumulate,
                               void* stream) {
    if (m1_debug_skip("conv_wgrad")) return M1_OK;
    if (!desc_ok(d) || !dy || !dw) return M1_ERR_BAD_ARG;
    M1ProfScope ps(prof_name("conv3d_wgrad", d).s, 2.0 * conv_macs(d, false), conv_bytes(d, false), (hipStream_t)stream);
    return wgrad_common(d, false, dy, dw, db, ws, (hipStream_t)stream, accumulate);
}
extern "C" int m1_convT3d_wgrad(const m1_conv_desc_t* d, const void* dy, float* dw, float* db, void* ws, int accumulate,
                                void* stream) {
    if (m1_debug_skip("conv_wgrad")) return M1_OK;
    if (!desc_ok(d) || !dy || !dw) return M1_ERR_BAD_ARG;
    M1ProfScope ps(prof_name("convT3d_wgrad", d).s, 2.0 * conv_macs(d, true), conv_bytes(d, true), (hipStream_t)stream);
    return wgrad_common(d, true, dy, dw, db, ws, (hipStream_t)stream, accumulate);
}
