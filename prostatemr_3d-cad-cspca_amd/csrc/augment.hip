// augment.hip -- train-time augmentations of tf2.5/scripts/model/augmentations.py (A:36-326, augment_tensors) on device tensors.
//
// Per sample, every op 2-D over (H, W) with one parameter record (m1_aug_params_t, include/m1hip.h) for all slices and channels:
//   zoom (A:139-152)   tf.image.resize bilinear (TF2: half-pixel centres, no antialias) to (scale, scale), crop at the bottom-right corner
//   flip (A:156-163)   mirror along W
//   rotate (A:219-236) SYMMETRIC pad by rot_pad, tfa.image.rotate bilinear (output -> input projective map, fill 0), central crop
//   translate (A:167-181) / channel shift (A:185-215)   SYMMETRIC pad top / left, crop at (pad_bottom, pad_right): an index map
//   gamma (A:275-310), poor scan (A:240-271), noise (A:314-326) on the first nimg channels
// aug_geom_kernel evaluates the five geometric stages lazily, from the output voxel back to the source: the index maps compose, the
// rotation reads four taps of the zoomed slice, each of which is four taps of the source.  Every stage's fp32 value is formed before
// the next stage uses it, in the operation order of the TF kernels, so the result is what materialising each stage would give.  A stage
// that did not fire contributes no arithmetic at all (index-only stages and un-fired samples are bit-exact copies).
// No contraction: hipcc fuses a * b + c into an fma by default, and a last-bit difference in a coordinate flips a floor.  The
// __fmul_rn / __fadd_rn intrinsics do not prevent that (this ROCm's __clang_hip_math.h defines them as plain * and +, compiled with
// contraction allowed), so the whole file is compiled under `#pragma clang fp contract(off)` and every operation whose rounding is
// part of the contract with the tests' restatement goes through this file's own rn_mul / rn_add / rn_sub / rn_div (one IEEE
// operation each): aug_geom_kernel holds no v_fma / v_fmac apart from the expansion of the IEEE division.
// The gamma stage needs min / max / mean / std of the whole geometric result per (sample, channel): the geometric kernel leaves
// per-block fp64 partials, a fold kernel adds them in a fixed order; aug_gstats_kernel does the same for the powered values
// (A:306-307); aug_intensity_kernel then applies gamma + poor scan + noise in one pass.
#include "common.h"

#pragma clang fp contract(off)
__device__ __forceinline__ float rn_mul(float a, float b) { return a * b; }
__device__ __forceinline__ float rn_add(float a, float b) { return a + b; }
__device__ __forceinline__ float rn_sub(float a, float b) { return a - b; }
__device__ __forceinline__ float rn_div(float a, float b) { return a / b; }

#define AUG_MAXC 8
#define AUG_MAXI 4                // image channels (3 MRI sequences for 'lesion', 1 for 'zonal')
#define AUG_BPS_MAX 256           // blocks per sample of the voxel kernels (also the number of partial rows per sample)
#define AUG_GOLDEN 0x9E3779B97F4A7C15ull
#define AUG_GEOM_BITS (M1_AUG_ZOOM | M1_AUG_FLIP | M1_AUG_ROTATE | M1_AUG_TRANSLATE | M1_AUG_CSHIFT)

struct AugDims { int D, H, W, C, nimg, nc, stages, bps; };

__device__ __forceinline__ int aug_clamp(int i, int n) { return min(max(i, 0), n - 1); }
// index of tf.pad(mode='SYMMETRIC') position i of an axis of n (clamped: a table entry out of range cannot leave the slice)
__device__ __forceinline__ int aug_sym(int i, int n) {
    if (i < 0) i = -1 - i;
    else if (i >= n) i = 2 * n - 1 - i;
    return aug_clamp(i, n);
}
// a + (b - a) * t, as tf.image.resize's bilinear kernel forms it
__device__ __forceinline__ float aug_lerp(float a, float b, float t) { return rn_add(a, rn_mul(rn_sub(b, a), t)); }

struct AugTap { int lo, hi; float t; };
// TF2 bilinear resize, output index i: in = (i + 0.5) * scale - 0.5, lower = max(floor(in), 0), upper = min(ceil(in), n - 1)
__device__ __forceinline__ AugTap aug_resize_tap(int i, float sf, int n_in) {
    const float in = rn_sub(rn_mul(rn_add((float)i, 0.5f), sf), 0.5f);
    const float f = floorf(in);
    AugTap r;
    r.lo = aug_clamp((int)f, n_in);
    r.hi = aug_clamp((int)ceilf(in), n_in);
    r.t = rn_sub(in, f);
    return r;
}
// TF2 nearest resize, output index i: min(floor((i + 0.5) * scale), n - 1)
__device__ __forceinline__ int aug_nearest(int i, float sf, int n_in) {
    return aug_clamp((int)floorf(rn_mul(rn_add((float)i, 0.5f), sf)), n_in);
}

// per-sample geometry, decoded once per thread
struct AugGeo {
    bool zoom, flip, rot, trans, cshift;
    int H, W, zoff_y, zoff_x, pad, dy, dx, cdy, cdx, csc;
    float zsf, t[6];
};
__device__ __forceinline__ AugGeo aug_decode(const m1_aug_params_t& p, const AugDims& g) {
    const unsigned f = (p.fired & M1_AUG_MASTER) ? (p.fired & (unsigned)g.stages) : 0u;
    AugGeo q;
    q.H = g.H; q.W = g.W;
    q.zoom = f & M1_AUG_ZOOM; q.flip = f & M1_AUG_FLIP; q.rot = f & M1_AUG_ROTATE; q.trans = f & M1_AUG_TRANSLATE;
    q.cshift = f & M1_AUG_CSHIFT;
    const int sc = max(p.scale, 1);
    q.zoff_y = sc - g.H; q.zoff_x = sc - g.W;                 // crop_to_bounding_box(scale - H, scale - W, H, W)
    q.zsf = rn_div((float)g.H, (float)sc);                           // A:143 resizes both axes to `scale` from shape[1] == shape[2]
    q.pad = max(p.rot_pad, 0);
#pragma unroll
    for (int i = 0; i < 6; ++i) q.t[i] = p.rot[i];
    q.dy = p.tr[1] - p.tr[0]; q.dx = p.tr[2] - p.tr[3];       // padded row r holds source row r - pad_top; the crop starts at pad_bottom
    q.cdy = p.cs[1] - p.cs[0]; q.cdx = p.cs[2] - p.cs[3];
    q.csc = p.cs_channel;
    return q;
}

// zoomed + flipped slice at (y, x): channels [c0, c1) of `s` (one (H, W, Cn) slice)
__device__ __forceinline__ void aug_zf(const float* __restrict__ s, int Cn, int c0, int c1, const AugGeo& q, int y, int x, float* o) {
    if (q.flip) x = q.W - 1 - x;
    if (!q.zoom) {
        const float* p = s + ((long long)y * q.W + x) * Cn;
#pragma unroll
        for (int c = 0; c < AUG_MAXC; ++c) if (c >= c0 && c < c1) o[c] = p[c];
        return;
    }
    const AugTap ty = aug_resize_tap(y + q.zoff_y, q.zsf, q.H), tx = aug_resize_tap(x + q.zoff_x, q.zsf, q.W);
    const float* tl = s + ((long long)ty.lo * q.W + tx.lo) * Cn;
    const float* tr = s + ((long long)ty.lo * q.W + tx.hi) * Cn;
    const float* bl = s + ((long long)ty.hi * q.W + tx.lo) * Cn;
    const float* br = s + ((long long)ty.hi * q.W + tx.hi) * Cn;
#pragma unroll
    for (int c = 0; c < AUG_MAXC; ++c)
        if (c >= c0 && c < c1) {
            const float top = aug_lerp(tl[c], tr[c], tx.t), bot = aug_lerp(bl[c], br[c], tx.t);
            o[c] = aug_lerp(top, bot, ty.t);
        }
}
// one tap of the rotation: position (yy, xx) (already floor values, as floats) of the SYMMETRIC-padded slice, 0 outside it
__device__ __forceinline__ void aug_padded(const float* __restrict__ s, int Cn, int c0, int c1, const AugGeo& q, float yy, float xx,
                                           float* o) {
    const int Hp = q.H + 2 * q.pad, Wp = q.W + 2 * q.pad;
    if (!(yy >= 0.f && yy < (float)Hp && xx >= 0.f && xx < (float)Wp)) {
#pragma unroll
        for (int c = 0; c < AUG_MAXC; ++c) o[c] = 0.f;
        return;
    }
    aug_zf(s, Cn, c0, c1, q, aug_sym((int)yy - q.pad, q.H), aug_sym((int)xx - q.pad, q.W), o);
}
// the slice after zoom, flip and rotate at (y, x)
__device__ __forceinline__ void aug_zfr(const float* __restrict__ s, int Cn, int c0, int c1, const AugGeo& q, int y, int x, float* o) {
    if (!q.rot) { aug_zf(s, Cn, c0, c1, q, y, x, o); return; }
    // tfa.image.rotate -> ImageProjectiveTransform, bilinear, fill 0; output position in the padded slice; central_crop starts at pad
    const float X = (float)(x + q.pad), Y = (float)(y + q.pad);
    const float ix = rn_add(rn_add(rn_mul(q.t[0], X), rn_mul(q.t[1], Y)), q.t[2]);
    const float iy = rn_add(rn_add(rn_mul(q.t[3], X), rn_mul(q.t[4], Y)), q.t[5]);
    const float xf = floorf(ix), yf = floorf(iy), xc = rn_add(xf, 1.f), yc = rn_add(yf, 1.f);
    const float wx0 = rn_sub(xc, ix), wx1 = rn_sub(ix, xf), wy0 = rn_sub(yc, iy), wy1 = rn_sub(iy, yf);
    float a[AUG_MAXC], b[AUG_MAXC], lo[AUG_MAXC];
    aug_padded(s, Cn, c0, c1, q, yf, xf, a);
    aug_padded(s, Cn, c0, c1, q, yf, xc, b);
#pragma unroll
    for (int c = 0; c < AUG_MAXC; ++c) if (c >= c0 && c < c1) lo[c] = rn_add(rn_mul(wx0, a[c]), rn_mul(wx1, b[c]));
    aug_padded(s, Cn, c0, c1, q, yc, xf, a);
    aug_padded(s, Cn, c0, c1, q, yc, xc, b);
#pragma unroll
    for (int c = 0; c < AUG_MAXC; ++c)
        if (c >= c0 && c < c1) {
            const float hi = rn_add(rn_mul(wx0, a[c]), rn_mul(wx1, b[c]));
            o[c] = rn_add(rn_mul(wy0, lo[c]), rn_mul(wy1, hi));
        }
}
// ... and after translate
__device__ __forceinline__ void aug_zfrt(const float* __restrict__ s, int Cn, int c0, int c1, const AugGeo& q, int y, int x, float* o) {
    if (q.trans) { y = aug_sym(y + q.dy, q.H); x = aug_sym(x + q.dx, q.W); }
    aug_zfr(s, Cn, c0, c1, q, y, x, o);
}

// workspace (doubles): fin [N][AUG_MAXI][8] = {min, max, mean, std, mean of powered, std of powered, -, -},
//                      part [N][bps][AUG_MAXI][4] = {min, max, sum, sum of squares} of one block
__device__ __forceinline__ double* aug_fin(void* ws, int n, int c) { return (double*)ws + ((long long)n * AUG_MAXI + c) * 8; }
__device__ __forceinline__ double* aug_part(void* ws, int N, int bps, int n, int b, int c) {
    return (double*)ws + (long long)N * AUG_MAXI * 8 + (((long long)n * bps + b) * AUG_MAXI + c) * 4;
}

// block-wide {min, max, sum, sum of squares} of up to AUG_MAXI channels into this block's partial row (fixed order)
__device__ __forceinline__ void aug_block_stats(const double* mn, const double* mx, const double* s1, const double* s2, int nimg,
                                                double* row) {
    __shared__ double red[4][AUG_MAXI][4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int c = 0; c < AUG_MAXI; ++c) {
        double a = mn[c], b = mx[c];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) { a = fmin(a, __shfl_xor(a, o, 64)); b = fmax(b, __shfl_xor(b, o, 64)); }
        const double u = wave_sum_d(s1[c]), v = wave_sum_d(s2[c]);
        if (lane == 0) { red[wave][c][0] = a; red[wave][c][1] = b; red[wave][c][2] = u; red[wave][c][3] = v; }
    }
    __syncthreads();
    if ((int)threadIdx.x < nimg) {
        const int c = threadIdx.x;
        row[c * 4 + 0] = fmin(fmin(red[0][c][0], red[1][c][0]), fmin(red[2][c][0], red[3][c][0]));
        row[c * 4 + 1] = fmax(fmax(red[0][c][1], red[1][c][1]), fmax(red[2][c][1], red[3][c][1]));
        row[c * 4 + 2] = (red[0][c][2] + red[1][c][2]) + (red[2][c][2] + red[3][c][2]);
        row[c * 4 + 3] = (red[0][c][3] + red[1][c][3]) + (red[2][c][3] + red[3][c][3]);
    }
}

__global__ void __launch_bounds__(256) aug_geom_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                       const m1_aug_params_t* __restrict__ table, float* __restrict__ gx,
                                                       float* __restrict__ gy, AugDims g, int N, void* ws) {
    const int n = blockIdx.y;
    const AugGeo q = aug_decode(table[n], g);
    const long long HW = (long long)g.H * g.W, DHW = HW * g.D;
    double mn[AUG_MAXI], mx[AUG_MAXI], s1[AUG_MAXI], s2[AUG_MAXI];
#pragma unroll
    for (int c = 0; c < AUG_MAXI; ++c) { mn[c] = 1e300; mx[c] = -1e300; s1[c] = 0.0; s2[c] = 0.0; }
    for (long long v = (long long)blockIdx.x * 256 + threadIdx.x; v < DHW; v += (long long)gridDim.x * 256) {
        const long long d = v / HW;
        const int r = (int)(v - d * HW), yy = r / g.W, xx = r - yy * g.W;
        const long long slice = (long long)n * g.D + d;
        float o[AUG_MAXC];
        const float* s = x + slice * HW * g.C;
        aug_zfrt(s, g.C, 0, g.C, q, yy, xx, o);
        if (q.cshift && q.csc >= 0 && q.csc < g.C) {              // A:185-215: one channel, translated once more with its own pads
            float t[AUG_MAXC];
            aug_zfrt(s, g.C, q.csc, q.csc + 1, q, aug_sym(yy + q.cdy, g.H), aug_sym(xx + q.cdx, g.W), t);
#pragma unroll
            for (int c = 0; c < AUG_MAXC; ++c) if (c == q.csc) o[c] = t[c];
        }
        float* dst = gx + (slice * HW + r) * g.C;
#pragma unroll
        for (int c = 0; c < AUG_MAXC; ++c) if (c < g.C) dst[c] = o[c];
#pragma unroll
        for (int c = 0; c < AUG_MAXI; ++c)
            if (c < g.nimg) {
                const double e = (double)o[c];
                mn[c] = fmin(mn[c], e); mx[c] = fmax(mx[c], e); s1[c] += e; s2[c] += e * e;
            }
        if (y) {
            aug_zfrt(y + slice * HW * g.nc, g.nc, 0, g.nc, q, yy, xx, o);
            float* ld = gy + (slice * HW + r) * g.nc;
#pragma unroll
            for (int c = 0; c < AUG_MAXC; ++c) if (c < g.nc) ld[c] = o[c];
        }
    }
    if (g.stages & M1_AUG_GAMMA) aug_block_stats(mn, mx, s1, s2, g.nimg, aug_part(ws, N, g.bps, n, blockIdx.x, 0));
}

// one wave per (sample, image channel): fold the partial rows in a fixed order.  second == 0: min, max, mean, std of the geometric
// result; second != 0: mean and std of the powered values
__global__ void __launch_bounds__(64) aug_fold_kernel(void* ws, int N, int bps, int nimg, double count, int second) {
    const int n = blockIdx.x / nimg, c = blockIdx.x - n * nimg, lane = threadIdx.x;
    double a = 1e300, b = -1e300, u = 0.0, v = 0.0;
    for (int i = lane; i < bps; i += 64) {
        const double* p = aug_part(ws, N, bps, n, i, c);
        a = fmin(a, p[0]); b = fmax(b, p[1]); u += p[2]; v += p[3];
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { a = fmin(a, __shfl_xor(a, o, 64)); b = fmax(b, __shfl_xor(b, o, 64)); }
    u = wave_sum_d(u); v = wave_sum_d(v);
    if (lane == 0) {
        double* f = aug_fin(ws, n, c);
        const double mean = u / count, var = fmax(v / count - mean * mean, 0.0);
        if (!second) { f[0] = a; f[1] = b; f[2] = mean; f[3] = sqrt(var); }
        else { f[4] = mean; f[5] = sqrt(var); }
    }
}

// per-(sample, channel) constants of the gamma stage (A:298-310), fp32 as the reference's tensors are
struct AugGam { bool on; float lo, rnge, den, mn, sd, m2, den2, gamma; };
__device__ __forceinline__ AugGam aug_gam(const m1_aug_params_t& p, int stages, void* ws, int n, int c) {
    AugGam k;
    k.on = (p.fired & M1_AUG_MASTER) && (p.fired & (unsigned)stages & M1_AUG_GAMMA) && ((p.gamma_ch >> c) & 1u);
    if (!k.on) return k;
    const double* f = aug_fin(ws, n, c);
    k.lo = (float)f[0];
    k.rnge = rn_sub((float)f[1], k.lo);
    k.den = rn_add(k.rnge, 1e-8f);
    k.mn = (float)f[2]; k.sd = (float)f[3]; k.m2 = (float)f[4]; k.den2 = rn_add((float)f[5], 1e-8f);
    k.gamma = p.gamma;
    return k;
}
// ((x - min) / (max - min + 1e-8)) ^ gamma * (max - min) + min   (A:302-304)
__device__ __forceinline__ float aug_pow(const AugGam& k, float v) {
    const float t = rn_div(rn_sub(v, k.lo), k.den);
    return rn_add(rn_mul(powf(t, k.gamma), k.rnge), k.lo);
}
// ... re-standardised to the original mean and std (A:306-308)
__device__ __forceinline__ float aug_gamma(const AugGam& k, float v) {
    if (!k.on) return v;
    return rn_add(rn_mul(rn_div(rn_sub(aug_pow(k, v), k.m2), k.den2), k.sd), k.mn);
}

__global__ void __launch_bounds__(256) aug_gstats_kernel(const float* __restrict__ gx, const m1_aug_params_t* __restrict__ table,
                                                         AugDims g, int N, void* ws) {
    const int n = blockIdx.y;
    const m1_aug_params_t p = table[n];
    AugGam k[AUG_MAXI];
#pragma unroll
    for (int c = 0; c < AUG_MAXI; ++c) { k[c].on = false; if (c < g.nimg) k[c] = aug_gam(p, g.stages, ws, n, c); }
    const long long DHW = (long long)g.D * g.H * g.W;
    double mn[AUG_MAXI], mx[AUG_MAXI], s1[AUG_MAXI], s2[AUG_MAXI];
#pragma unroll
    for (int c = 0; c < AUG_MAXI; ++c) { mn[c] = 0.0; mx[c] = 0.0; s1[c] = 0.0; s2[c] = 0.0; }
    for (long long v = (long long)blockIdx.x * 256 + threadIdx.x; v < DHW; v += (long long)gridDim.x * 256) {
        const float* s = gx + ((long long)n * DHW + v) * g.C;
#pragma unroll
        for (int c = 0; c < AUG_MAXI; ++c)
            if (c < g.nimg && k[c].on) { const double e = (double)aug_pow(k[c], s[c]); s1[c] += e; s2[c] += e * e; }
    }
    aug_block_stats(mn, mx, s1, s2, g.nimg, aug_part(ws, N, g.bps, n, blockIdx.x, 0));
}

struct AugNoise { const uint64_t* rng; uint64_t stream_id; };

__global__ void __launch_bounds__(256) aug_intensity_kernel(const float* __restrict__ gx, const m1_aug_params_t* __restrict__ table,
                                                            AugNoise nz, float* __restrict__ out, AugDims g, int h2, void* ws) {
    const int n = blockIdx.y;
    const m1_aug_params_t p = table[n];
    const unsigned f = (p.fired & M1_AUG_MASTER) ? (p.fired & (unsigned)g.stages) : 0u;
    AugGam k[AUG_MAXI];
#pragma unroll
    for (int c = 0; c < AUG_MAXI; ++c) { k[c].on = false; if (c < g.nimg) k[c] = aug_gam(p, g.stages, ws, n, c); }
    const bool poor = f & M1_AUG_POOR, noise = (f & M1_AUG_NOISE) && nz.rng;
    const float up_sf = rn_div((float)h2, (float)g.H), down_sf = rn_div((float)g.H, (float)h2);      // A:267-268
    uint64_t seed = 0, base = 0;
    if (noise) { seed = nz.rng[0] + nz.stream_id * AUG_GOLDEN; base = nz.rng[1] << 36; }
    const long long HW = (long long)g.H * g.W, DHW = HW * g.D;
    for (long long v = (long long)blockIdx.x * 256 + threadIdx.x; v < DHW; v += (long long)gridDim.x * 256) {
        const long long d = v / HW;
        const int r = (int)(v - d * HW), yy = r / g.W, xx = r - yy * g.W;
        const float* s = gx + ((long long)n * g.D + d) * HW * g.C;
        float o[AUG_MAXC];
#pragma unroll
        for (int c = 0; c < AUG_MAXC; ++c) if (c < g.C) o[c] = s[(long long)r * g.C + c];
        float z[AUG_MAXI] = {0.f, 0.f, 0.f, 0.f};
        if (noise) {
            const uint4 w = philox4x32_10(seed, base + (uint64_t)((long long)n * DHW + v));
            const float u1 = ((float)(w.x >> 8) + 0.5f) * (1.0f / 16777216.0f), u2 = (float)(w.y >> 8) * (1.0f / 16777216.0f);
            const float r1 = sqrtf(-2.f * logf(u1));
            z[0] = r1 * cosf(6.28318530718f * u2);
            if (g.nimg > 1) {
                const float u3 = ((float)(w.z >> 8) + 0.5f) * (1.0f / 16777216.0f), u4 = (float)(w.w >> 8) * (1.0f / 16777216.0f);
                const float r2 = sqrtf(-2.f * logf(u3));
                z[1] = r1 * sinf(6.28318530718f * u2); z[2] = r2 * cosf(6.28318530718f * u4); z[3] = r2 * sinf(6.28318530718f * u4);
            }
        }
        AugTap ty, tx;
        if (poor) {
            ty = aug_resize_tap(aug_nearest(yy, up_sf, h2), down_sf, g.H);
            tx = aug_resize_tap(aug_nearest(xx, up_sf, h2), down_sf, g.W);
        }
#pragma unroll
        for (int c = 0; c < AUG_MAXI; ++c) {
            if (c >= g.nimg) continue;
            float e;
            if (poor && ((p.poor_ch >> c) & 1u)) {
                const float tl = aug_gamma(k[c], s[((long long)ty.lo * g.W + tx.lo) * g.C + c]);
                const float tr = aug_gamma(k[c], s[((long long)ty.lo * g.W + tx.hi) * g.C + c]);
                const float bl = aug_gamma(k[c], s[((long long)ty.hi * g.W + tx.lo) * g.C + c]);
                const float br = aug_gamma(k[c], s[((long long)ty.hi * g.W + tx.hi) * g.C + c]);
                e = aug_lerp(aug_lerp(tl, tr, tx.t), aug_lerp(bl, br, tx.t), ty.t);
            } else {
                e = aug_gamma(k[c], o[c]);
            }
            if (noise) e = rn_add(e, rn_mul(p.noise_std, z[c]));
            o[c] = e;
        }
        float* dst = out + ((long long)n * DHW + v) * g.C;
#pragma unroll
        for (int c = 0; c < AUG_MAXC; ++c) if (c < g.C) dst[c] = o[c];
    }
}

// ---- the table, drawn on the device ------------------------------------------------------------------------------------------
struct AugHyper {
    float prob, tx_prob, rot_deg, noise, g0, g1;
    int zoom_on, zoom_hi, flip_on, rot_on, tr_on, tr_hi_h, tr_hi_w, cs_on, cs_hi_h, cs_hi_w, gamma_on, poor_on, noise_on;
    int H, W, nimg, pad;
};

__global__ void __launch_bounds__(64) aug_draw_kernel(m1_aug_params_t* __restrict__ table, int N, const uint64_t* __restrict__ rng,
                                                      uint64_t stream_id, AugHyper h) {
    const int n = blockIdx.x * 64 + threadIdx.x;
    if (n >= N) return;
    const uint64_t seed = rng[0] + stream_id * AUG_GOLDEN, base = (rng[1] << 36) + (uint64_t)n * 64;
    unsigned k = 0;
    auto word = [&]() -> uint32_t { return philox4x32_10(seed, base + k++).x; };
    auto uni = [&]() -> float { return (float)(word() >> 9) * (1.0f / 8388608.0f); };             // 23 bits, as TF's Uint32ToFloat
    auto between = [&](int lo, int hi) -> int { return lo + (int)(word() % (uint32_t)(hi - lo)); };
    auto ufl = [&](float lo, float hi) -> float { return rn_add(rn_mul(uni(), rn_sub(hi, lo)), lo); };
    m1_aug_params_t r;
    r.fired = 0; r.gamma_ch = 0; r.poor_ch = 0; r.scale = h.H; r.rot_pad = h.pad;
    r.rot[0] = 1.f; r.rot[1] = 0.f; r.rot[2] = 0.f; r.rot[3] = 0.f; r.rot[4] = 1.f; r.rot[5] = 0.f;
    for (int i = 0; i < 4; ++i) { r.tr[i] = 0; r.cs[i] = 0; }
    r.cs_channel = 0; r.gamma = 1.f; r.noise_std = 0.f; r.angle_deg = 0.f; r._pad = 0;
    if (uni() > rn_sub(1.f, h.prob)) {                                            // A:51
        r.fired |= M1_AUG_MASTER;
        if (h.zoom_on) {                                                             // A:58-62
            if (uni() > h.tx_prob) r.fired |= M1_AUG_ZOOM;
            r.scale = between(h.H, h.zoom_hi);
        }
        if (h.flip_on && uni() > 0.5f) r.fired |= M1_AUG_FLIP;                       // A:65-67
        if (h.rot_on) {                                                              // A:70-73, 232; tfa angles_to_projective_transforms
            if (uni() > h.tx_prob) r.fired |= M1_AUG_ROTATE;
            r.angle_deg = ufl(-h.rot_deg, h.rot_deg);
            const float rad = rn_div(rn_mul(r.angle_deg, 3.14159265358979323846f), 180.f);
            const float c = cosf(rad), s = sinf(rad);
            const float w1 = (float)(h.W + 2 * h.pad - 1), h1 = (float)(h.H + 2 * h.pad - 1);
            r.rot[0] = c; r.rot[1] = -s; r.rot[2] = (w1 - (c * w1 - s * h1)) / 2.f;
            r.rot[3] = s; r.rot[4] = c;  r.rot[5] = (h1 - (s * w1 + c * h1)) / 2.f;
        }
        if (h.tr_on) {                                                               // A:76-83
            if (uni() > h.tx_prob) r.fired |= M1_AUG_TRANSLATE;
            r.tr[0] = between(0, h.tr_hi_h); r.tr[1] = between(0, h.tr_hi_h);
            r.tr[2] = between(0, h.tr_hi_w); r.tr[3] = between(0, h.tr_hi_w);
        }
        if (h.cs_on) {                                                               // A:85-94, 189
            const bool on = uni() > h.tx_prob;
            r.cs[0] = between(0, h.cs_hi_h); r.cs[1] = between(0, h.cs_hi_h);
            r.cs[2] = between(0, h.cs_hi_w); r.cs[3] = between(0, h.cs_hi_w);
            if (on) { r.fired |= M1_AUG_CSHIFT; r.cs_channel = between(0, 3); }
        }
        if (h.gamma_on) {                                                            // A:97-100, 299
            const bool on = uni() > h.tx_prob;
            r.gamma = ufl(h.g0, h.g1);
            if (on) {
                r.fired |= M1_AUG_GAMMA;
                for (int c = 0; c < h.nimg; ++c) if (uni() > 0.5f) r.gamma_ch |= 1u << c;
            }
        }
        if (h.poor_on && uni() > h.tx_prob) {                                        // A:103-105, 265
            r.fired |= M1_AUG_POOR;
            for (int c = 0; c < h.nimg; ++c) if (uni() > 0.5f) r.poor_ch |= 1u << c;
        }
        if (h.noise_on) {                                                            // A:108-111
            if (uni() > h.tx_prob) r.fired |= M1_AUG_NOISE;
            r.noise_std = ufl(0.f, h.noise);
        }
    }
    table[n] = r;
}

// ---- host side -----------------------------------------------------------------------------------------------------------------
static inline int aug_bps(long long DHW) { long long b = cdiv_ll(DHW, 256); return (int)(b > AUG_BPS_MAX ? AUG_BPS_MAX : (b < 1 ? 1 : b)); }
// A:222-223
static inline int aug_rot_pad(int H, int W) {
    const double diag = sqrt((double)H * H + (double)W * W);
    return (int)ceil((diag - (double)(H < W ? H : W)) / 2.0);
}
// tf.math.ceil of a float32 tensor made from the Python product (A:61, 78-81, 89-92)
static inline int aug_ceil_f32(double v) { return (int)ceilf((float)v); }

static int aug_check(int N, int D, int H, int W, int C, int nimg, int stages, int dtype) {
    if (N <= 0 || D <= 0 || H <= 0 || W <= 0 || C <= 0 || nimg <= 0 || nimg > C || stages < 0) return M1_ERR_BAD_ARG;
    if (dtype != M1_F32 && dtype != M1_BF16) return M1_ERR_BAD_ARG;
    if (dtype != M1_F32 || C > AUG_MAXC || nimg > AUG_MAXI || N > 65535) return M1_ERR_UNSUPPORTED;
    if ((stages & (M1_AUG_ZOOM | M1_AUG_ROTATE | M1_AUG_POOR)) && H != W) return M1_ERR_UNSUPPORTED;
    if ((stages & M1_AUG_POOR) && (int)((double)H * 0.75) < 1) return M1_ERR_UNSUPPORTED;
    if (stages & M1_AUG_ROTATE) {
        // tf.image.central_crop(x, H / Hp) (A:233-234): start = int((Hp - Hp * fraction) / 2) in double, size = Hp - 2 * start
        const int pad = aug_rot_pad(H, W), Hp = H + 2 * pad;
        const double frac = (double)H / (double)Hp;
        const int start = (int)(((double)Hp - (double)Hp * frac) / 2.0);
        if (Hp - 2 * start != H || start != pad || pad > H) return M1_ERR_UNSUPPORTED;
    }
    return M1_OK;
}

extern "C" size_t m1_aug_ws_bytes(int N, int D, int H, int W, int nimg) {
    if (N <= 0 || D <= 0 || H <= 0 || W <= 0 || nimg <= 0 || nimg > AUG_MAXI) return 0;
    const int bps = aug_bps((long long)D * H * W);
    return sizeof(double) * ((size_t)N * AUG_MAXI * 8 + (size_t)N * bps * AUG_MAXI * 4);
}

extern "C" int m1_aug_draw(m1_aug_params_t* table, int N, const uint64_t* rng, uint64_t stream_id, double prob, double tx_prob,
                           double translate_factor, double rotation_degree, int axial_hflip, double zoom_factor,
                           double gauss_noise_stddev, double chan_shift_factor, int sim_poor_scan, double gamma_lo, double gamma_hi,
                           int H, int W, int nimg, int lesion, void* stream) {
    if (!table || !rng || N <= 0 || H <= 0 || W <= 0 || nimg <= 0 || nimg > AUG_MAXI) return M1_ERR_BAD_ARG;
    AugHyper h;
    h.prob = (float)prob; h.tx_prob = (float)tx_prob; h.rot_deg = (float)rotation_degree; h.noise = (float)gauss_noise_stddev;
    h.g0 = (float)gamma_lo; h.g1 = (float)gamma_hi;
    h.zoom_on = zoom_factor != 0.0; h.zoom_hi = aug_ceil_f32((double)H * zoom_factor);
    h.flip_on = axial_hflip != 0; h.rot_on = rotation_degree != 0.0;
    h.tr_on = translate_factor != 0.0;
    h.tr_hi_h = aug_ceil_f32((double)H * translate_factor); h.tr_hi_w = aug_ceil_f32((double)W * translate_factor);
    h.cs_on = lesion && chan_shift_factor != 0.0;
    h.cs_hi_h = aug_ceil_f32((double)H * chan_shift_factor); h.cs_hi_w = aug_ceil_f32((double)W * chan_shift_factor);
    h.gamma_on = (gamma_lo + gamma_hi) != 0.0; h.poor_on = sim_poor_scan != 0; h.noise_on = gauss_noise_stddev != 0.0;
    h.H = H; h.W = W; h.nimg = nimg; h.pad = aug_rot_pad(H, W);
    if (h.zoom_on && h.zoom_hi <= H) return M1_ERR_BAD_ARG;
    if (h.tr_on && (h.tr_hi_h < 1 || h.tr_hi_w < 1 || h.tr_hi_h > H || h.tr_hi_w > W)) return M1_ERR_BAD_ARG;
    if (h.cs_on && (h.cs_hi_h < 1 || h.cs_hi_w < 1 || h.cs_hi_h > H || h.cs_hi_w > W || nimg < 3)) return M1_ERR_BAD_ARG;
    if ((h.zoom_on || h.rot_on || h.poor_on) && H != W) return M1_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(aug_draw_kernel, dim3((unsigned)cdiv_ll(N, 64)), dim3(64), 0, (hipStream_t)stream, table, N, rng, stream_id, h);
    return m1_check_launch();
}

static AugDims aug_dims(int D, int H, int W, int C, int nimg, int nc, int stages) {
    AugDims g; g.D = D; g.H = H; g.W = W; g.C = C; g.nimg = nimg; g.nc = nc; g.stages = stages; g.bps = aug_bps((long long)D * H * W);
    return g;
}

extern "C" int m1_aug_geom(const float* x, const float* y, const m1_aug_params_t* table, float* gx, float* gy, int N, int D, int H,
                           int W, int C, int nimg, int nc, int stages, int dtype, void* ws, void* stream) {
    if (!x || !table || !gx || (y && (!gy || nc <= 0)) || x == gx || (y && y == gy)) return M1_ERR_BAD_ARG;
    const int rc = aug_check(N, D, H, W, C, nimg, stages, dtype);
    if (rc != M1_OK) return rc;
    if (y && nc > AUG_MAXC) return M1_ERR_UNSUPPORTED;
    if ((stages & M1_AUG_GAMMA) && (!ws || ((uintptr_t)ws & 7))) return M1_ERR_BAD_ARG;
    const AugDims g = aug_dims(D, H, W, C, nimg, y ? nc : 0, stages);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(aug_geom_kernel, dim3(g.bps, N), dim3(256), 0, st, x, y, table, gx, gy, g, N, ws);
    if (stages & M1_AUG_GAMMA)
        hipLaunchKernelGGL(aug_fold_kernel, dim3(N * nimg), dim3(64), 0, st, ws, N, g.bps, nimg, (double)D * H * W, 0);
    return m1_check_launch();
}

extern "C" int m1_aug_gamma_stats(const float* gx, const m1_aug_params_t* table, int N, int D, int H, int W, int C, int nimg,
                                  int stages, int dtype, void* ws, void* stream) {
    if (!gx || !table || !ws || ((uintptr_t)ws & 7)) return M1_ERR_BAD_ARG;
    const int rc = aug_check(N, D, H, W, C, nimg, stages, dtype);
    if (rc != M1_OK) return rc;
    if (!(stages & M1_AUG_GAMMA)) return M1_OK;
    const AugDims g = aug_dims(D, H, W, C, nimg, 0, stages);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(aug_gstats_kernel, dim3(g.bps, N), dim3(256), 0, st, gx, table, g, N, ws);
    hipLaunchKernelGGL(aug_fold_kernel, dim3(N * nimg), dim3(64), 0, st, ws, N, g.bps, nimg, (double)D * H * W, 1);
    return m1_check_launch();
}

extern "C" int m1_aug_intensity(const float* gx, const m1_aug_params_t* table, const uint64_t* rng, uint64_t stream_id, float* out,
                                int N, int D, int H, int W, int C, int nimg, int stages, int dtype, void* ws, void* stream) {
    if (!gx || !table || !out || gx == out || ((stages & M1_AUG_NOISE) && !rng)) return M1_ERR_BAD_ARG;
    const int rc = aug_check(N, D, H, W, C, nimg, stages, dtype);
    if (rc != M1_OK) return rc;
    if ((stages & M1_AUG_GAMMA) && (!ws || ((uintptr_t)ws & 7))) return M1_ERR_BAD_ARG;
    if ((long long)N * D * H * W >= (1ll << 36)) return M1_ERR_UNSUPPORTED;      // the noise counter keeps the step above bit 36
    const AugDims g = aug_dims(D, H, W, C, nimg, 0, stages);
    const int h2 = (stages & M1_AUG_POOR) ? (int)((double)H * 0.75) : H;
    hipLaunchKernelGGL(aug_intensity_kernel, dim3(g.bps, N), dim3(256), 0, (hipStream_t)stream, gx, table, AugNoise{rng, stream_id},
                       out, g, h2, ws);
    return m1_check_launch();
}
