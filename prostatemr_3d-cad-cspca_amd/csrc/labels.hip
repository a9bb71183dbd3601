// labels.hip -- label preparation of the reference's data generator (data_generators.py:51-72,92-97) on the device.
//   m1_contour_smooth_u8: contour_smoothening, i.e. the 8-bit fixed-point Gaussian blur of every axial slice of a uint8 mask, as the
//                         integer rule of DESIGN.md ("label feed"): S = sum_dy sum_dx w[dy] w[dx] m(r(y+dy), r(x+dx)), r = reflect-101,
//                         out = (S + 32768) >> 16.  The seven taps are DATA (a table the host computes, data_generators.gaussian_taps_u8).
//   m1_label_prepare    : the fused feed -- binarise the raw annotation per class, smooth every class mask, one-hot, and write the
//                         network input (image channels + the posterior's label channels), the `detection` target and the zero `KL`
//                         target in ONE launch (no memset / memcpy: the zero fills are stores of this kernel).
// One block of 256 threads owns one LT x LT tile of one slice.  The tile with its halo is staged in LDS as bytes with the reflection
// applied on the way in (32-bit loads where a word lies inside the row and is aligned, byte loads on the borders); the row pass leaves
// 16-bit sums in LDS (255 * 256 fits), the column pass reads them as 8-byte vectors and keeps S in 32 bits (255 * 65536 fits).  No
// float appears before the one-hot values are converted for the fp32 outputs.
#include "common.h"

#define LT 32                      // tile edge (hip/ops.py LABEL_TILE states the same number for the tests)
#define LR 3                       // halo = radius of the 7 taps
#define LROWS (LT + 2 * LR)        // 38 staged rows
#define LMW 10                     // staged row = 10 words = 40 bytes: global columns x0 - 4 .. x0 + 35 (word-aligned where the row is)
#define LNT 256

struct LabelTaps { int w[2 * LR + 1]; };

enum { BIN_RAW = 0, BIN_LESION = 1, BIN_TZ = 2, BIN_PZ = 3 };

__device__ __forceinline__ int reflect101(int i, int n) {
    if (n == 1) return 0;
    const int p = 2 * (n - 1);
    i %= p;
    if (i < 0) i += p;
    return i < n ? i : p - i;
}

__device__ __forceinline__ unsigned bin_byte(unsigned v, int bin) {
    return bin == BIN_RAW ? v : bin == BIN_LESION ? (v >= 2u) : bin == BIN_TZ ? (v == 1u) : (v == 2u);
}
__device__ __forceinline__ unsigned bin_word(unsigned v, int bin) {
    return bin_byte(v & 255u, bin) | (bin_byte((v >> 8) & 255u, bin) << 8) | (bin_byte((v >> 16) & 255u, bin) << 16) |
           (bin_byte(v >> 24, bin) << 24);
}

// The smoothed values of the tile at (y0, x0) of one H x W slice: thread t returns the four of row t / 8, columns 4 (t % 8) .. + 3,
// packed little-endian in one word (values outside the slice are computed from reflected data and are not to be stored).
// Ends with the LDS free for the next call only after the caller's next __syncthreads.
__device__ __forceinline__ unsigned smooth_tile(const uint8_t* __restrict__ pl, int H, int W, int y0, int x0, int bin,
                                                const LabelTaps& tp, unsigned* m_w, unsigned short* hs) {
    const int t = threadIdx.x;
    const bool rows_aligned = (W & 3) == 0 && (((uintptr_t)pl) & 3) == 0;
    // stage: LROWS x LMW words, byte (r, j) = m(reflect(y0 - 3 + r), reflect(x0 - 4 + j))
    for (int i = t; i < LROWS * LMW; i += LNT) {
        const int r = i / LMW, k = i - r * LMW;
        const int gy = reflect101(y0 - LR + r, H), c = x0 - 4 + 4 * k;
        const uint8_t* row = pl + (long long)gy * W;
        unsigned v;
        if (rows_aligned && c >= 0 && c + 3 < W) {
            v = *reinterpret_cast<const unsigned*>(row + c);
        } else {
            v = (unsigned)row[reflect101(c, W)] | ((unsigned)row[reflect101(c + 1, W)] << 8) |
                ((unsigned)row[reflect101(c + 2, W)] << 16) | ((unsigned)row[reflect101(c + 3, W)] << 24);
        }
        m_w[i] = bin_word(v, bin);
    }
    __syncthreads();
    // row pass: item (r, q) -> hs[r][4q .. 4q + 3]; output column lx reads staged bytes lx + 1 .. lx + 7
    for (int i = t; i < LROWS * (LT / 4); i += LNT) {
        const int r = i / (LT / 4), q = i - r * (LT / 4);
        const unsigned a = m_w[r * LMW + q], b = m_w[r * LMW + q + 1], c = m_w[r * LMW + q + 2];
        unsigned by[12];
#pragma unroll
        for (int j = 0; j < 4; ++j) { by[j] = (a >> (8 * j)) & 255u; by[4 + j] = (b >> (8 * j)) & 255u; by[8 + j] = (c >> (8 * j)) & 255u; }
        unsigned s[4];
#pragma unroll
        for (int o = 0; o < 4; ++o) {
            unsigned acc = 0;
#pragma unroll
            for (int d = 0; d < 2 * LR + 1; ++d) acc += (unsigned)tp.w[d] * by[o + 1 + d];
            s[o] = acc;
        }
        uint2 pk;
        pk.x = s[0] | (s[1] << 16);
        pk.y = s[2] | (s[3] << 16);
        *reinterpret_cast<uint2*>(hs + r * LT + 4 * q) = pk;
    }
    __syncthreads();
    // column pass
    const int ly = t >> 3, q = t & 7;
    unsigned S[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int d = 0; d < 2 * LR + 1; ++d) {
        const uint2 pk = *reinterpret_cast<const uint2*>(hs + (ly + d) * LT + 4 * q);
        const unsigned w = (unsigned)tp.w[d];
        S[0] += w * (pk.x & 0xffffu); S[1] += w * (pk.x >> 16);
        S[2] += w * (pk.y & 0xffffu); S[3] += w * (pk.y >> 16);
    }
    return ((S[0] + 32768u) >> 16) | (((S[1] + 32768u) >> 16) << 8) | (((S[2] + 32768u) >> 16) << 16) | (((S[3] + 32768u) >> 16) << 24);
}

__device__ __forceinline__ void tile_of_block(long long blk, int tx_n, int ty_n, long long& plane, int& y0, int& x0) {
    const long long per = (long long)tx_n * ty_n;
    plane = blk / per;
    const int rem = (int)(blk - plane * per);
    const int ty = rem / tx_n;
    y0 = ty * LT;
    x0 = (rem - ty * tx_n) * LT;
}

__global__ void __launch_bounds__(LNT) contour_smooth_kernel(const uint8_t* __restrict__ in, uint8_t* __restrict__ out, int H, int W,
                                                             int tx_n, int ty_n, LabelTaps tp) {
    __shared__ unsigned m_w[LROWS * LMW];
    __shared__ __attribute__((aligned(8))) unsigned short hs[LROWS * LT];
    long long plane; int y0, x0;
    tile_of_block(blockIdx.x, tx_n, ty_n, plane, y0, x0);
    const long long base = plane * (long long)H * W;
    const unsigned v = smooth_tile(in + base, H, W, y0, x0, BIN_RAW, tp, m_w, hs);
    const int y = y0 + (threadIdx.x >> 3), x = x0 + 4 * (threadIdx.x & 7);
    if (y >= H || x >= W) return;
    uint8_t* o = out + base + (long long)y * W + x;
    if (x + 3 < W && (((uintptr_t)o) & 3) == 0) {
        *reinterpret_cast<unsigned*>(o) = v;
    } else {
        for (int j = 0; j < 4 && x + j < W; ++j) o[j] = (uint8_t)(v >> (8 * j));
    }
}

// NCH floats per voxel over the tile's rows: element (ly, lx, c) = f(ly, lx, c).  Every tile row is one contiguous run of tw * NCH
// floats; with `vec` (rows 16-byte aligned and a multiple of 4 floats long) a thread writes four of them as one float4.
template <int NCH, typename F>
__device__ __forceinline__ void emit_rows(float* __restrict__ dst, long long vox0, int W, int th, int tw, bool vec, F f) {
    if (vec) {
        constexpr int SEG = LT * NCH / 4;
        for (int i = threadIdx.x; i < LT * SEG; i += LNT) {
            const int ly = i / SEG, k = i - ly * SEG;
            if (ly >= th || 4 * k >= tw * NCH) continue;
            float o[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) { const int j = 4 * k + q; o[q] = f(ly, j / NCH, j % NCH); }
            VecIO<float, 4>::st(dst + (vox0 + (long long)ly * W) * NCH + 4 * k, o);
        }
    } else {
        constexpr int SEG = LT * NCH;
        for (int i = threadIdx.x; i < LT * SEG; i += LNT) {
            const int ly = i / SEG, j = i - ly * SEG;
            if (ly >= th || j >= tw * NCH) continue;
            dst[(vox0 + (long long)ly * W) * NCH + j] = f(ly, j / NCH, j % NCH);
        }
    }
}

// NC classes, COUT channels of the network input = keep image channels + npost posterior channels (npost = 0 or NC - 1)
template <int NC, int COUT>
__global__ void __launch_bounds__(LNT) label_prepare_kernel(const uint8_t* __restrict__ ann, const float* __restrict__ image,
                                                            float* __restrict__ xo, float* __restrict__ det, float* __restrict__ kl,
                                                            int H, int W, int C, int npost, int post_live, int tx_n, int ty_n, bool vec,
                                                            LabelTaps tp) {
    __shared__ unsigned m_w[LROWS * LMW];
    __shared__ __attribute__((aligned(8))) unsigned short hs[LROWS * LT];
    __shared__ unsigned cls_w[(NC - 1) * LT * (LT / 4)];
    const uint8_t* cls = reinterpret_cast<const uint8_t*>(cls_w);
    long long plane; int y0, x0;
    tile_of_block(blockIdx.x, tx_n, ty_n, plane, y0, x0);
    const long long base = plane * (long long)H * W;
    if (ann) {
#pragma unroll
        for (int k = 0; k < NC - 1; ++k) {         // (class k + 1 may stage while class k's column pass reads hs: other arrays)
            cls_w[k * LT * (LT / 4) + threadIdx.x] = smooth_tile(ann + base, H, W, y0, x0, NC == 2 ? BIN_LESION : BIN_TZ + k, tp, m_w, hs);
        }
    } else {
#pragma unroll
        for (int k = 0; k < NC - 1; ++k) cls_w[k * LT * (LT / 4) + threadIdx.x] = 0u;
    }
    __syncthreads();
    const int th = min(LT, H - y0), tw = min(LT, W - x0);
    const long long vox0 = base + (long long)y0 * W + x0;
    // one-hot in 8-bit arithmetic: background = 1 - tz - pz (mod 256), as the reference's uint8 arrays compute it
    auto onehot = [&](int ly, int lx, int c) -> float {
        if (c > 0) return (float)cls[(c - 1) * LT * LT + ly * LT + lx];
        unsigned bg = 1u;
#pragma unroll
        for (int k = 0; k < NC - 1; ++k) bg -= cls[k * LT * LT + ly * LT + lx];
        return (float)(bg & 255u);
    };
    emit_rows<NC>(det, vox0, W, th, tw, vec, onehot);
    if (kl) emit_rows<NC>(kl, vox0, W, th, tw, vec, [](int, int, int) -> float { return 0.f; });
    const int keep = COUT - npost;
    emit_rows<COUT>(xo, vox0, W, th, tw, vec, [&](int ly, int lx, int c) -> float {
        if (c < keep) return image[(vox0 + (long long)ly * W + lx) * C + c];
        return post_live ? (float)cls[(c - keep) * LT * LT + ly * LT + lx] : 0.f;
    });
}

static int label_taps(const int* taps, LabelTaps& tp) {
    if (!taps) return M1_ERR_BAD_ARG;
    int sum = 0;
    for (int d = 0; d < 2 * LR + 1; ++d) {
        if (taps[d] < 0 || taps[d] > 256) return M1_ERR_BAD_ARG;
        tp.w[d] = taps[d];
        sum += taps[d];
    }
    return sum == 256 ? M1_OK : M1_ERR_BAD_ARG;         // (the 16- and 32-bit sums of the kernel are sized for weights that sum to 256)
}

static inline bool label_blocks(long long planes, int H, int W, int& tx_n, int& ty_n, long long& blocks) {
    tx_n = (W + LT - 1) / LT;
    ty_n = (H + LT - 1) / LT;
    blocks = planes * tx_n * ty_n;
    return blocks <= 0x7fffffffll && planes * (long long)H * W <= (1ll << 40);
}

extern "C" int m1_contour_smooth_u8(const uint8_t* in, uint8_t* out, uint8_t* scratch, long long planes, int H, int W, const int* taps,
                                    int iterations, void* stream) {
    if (m1_debug_skip("contour_smooth")) return M1_OK;
    if (!in || !out || in == out || planes <= 0 || H <= 0 || W <= 0 || iterations <= 0) return M1_ERR_BAD_ARG;
    if (iterations > 1 && (!scratch || scratch == in || scratch == out)) return M1_ERR_BAD_ARG;
    LabelTaps tp;
    if (int rc = label_taps(taps, tp)) return rc;
    int tx_n, ty_n; long long blocks;
    if (!label_blocks(planes, H, W, tx_n, ty_n, blocks)) return M1_ERR_UNSUPPORTED;
    hipStream_t st = (hipStream_t)stream;
    M1ProfScope ps("contour_smooth", 0.0, 2.0 * (double)planes * H * W * iterations, st);
    const uint8_t* src = in;
    for (int it = 0; it < iterations; ++it) {
        uint8_t* dst = ((iterations - 1 - it) & 1) ? scratch : out;      // ping-pong so that the last pass lands in `out`
        hipLaunchKernelGGL(contour_smooth_kernel, dim3((unsigned)blocks), dim3(LNT), 0, st, src, dst, H, W, tx_n, ty_n, tp);
        src = dst;
    }
    return m1_check_launch();
}

extern "C" int m1_label_prepare(const uint8_t* ann, const float* image, float* x_out, float* detection, float* kl, int B, int D, int H,
                                int W, int C, int objective, int mode, int probabilistic, const int* taps, void* stream) {
    if (m1_debug_skip("label_prepare")) return M1_OK;
    if (!image || !x_out || !detection || B <= 0 || D <= 0 || H <= 0 || W <= 0 || C <= 0) return M1_ERR_BAD_ARG;
    if (objective != M1_LABEL_LESION && objective != M1_LABEL_ZONAL) return M1_ERR_UNSUPPORTED;
    if (mode != M1_FEED_TRAIN && mode != M1_FEED_VALID && mode != M1_FEED_TEST) return M1_ERR_UNSUPPORTED;
    if (mode == M1_FEED_TEST) ann = nullptr;                             // (the reference reads no annotation there: zeros)
    else if (!ann) return M1_ERR_BAD_ARG;
    if ((probabilistic != 0) != (kl != nullptr)) return M1_ERR_BAD_ARG;
    if ((((uintptr_t)image) | ((uintptr_t)x_out) | ((uintptr_t)detection) | ((uintptr_t)kl)) & 3) return M1_ERR_BAD_ARG;
    LabelTaps tp;
    if (int rc = label_taps(taps, tp)) return rc;
    const int nc = objective == M1_LABEL_LESION ? 2 : 3;
    const int keep = objective == M1_LABEL_LESION ? C : 1;               // zonal: image[..., :1]
    const int npost = probabilistic ? nc - 1 : 0, cout = keep + npost;
    if (keep > 4 || C > 64) return M1_ERR_UNSUPPORTED;
    int tx_n, ty_n; long long blocks;
    const long long planes = (long long)B * D;
    if (!label_blocks(planes, H, W, tx_n, ty_n, blocks)) return M1_ERR_UNSUPPORTED;
    const bool vec = (W & 3) == 0 && ((((uintptr_t)x_out) | ((uintptr_t)detection) | ((uintptr_t)kl)) & 15) == 0;
    const int post_live = mode == M1_FEED_TRAIN;
    hipStream_t st = (hipStream_t)stream;
    const double vox = (double)planes * H * W;
    M1ProfScope ps("label_prepare", 0.0, vox * ((ann ? nc - 1 : 0) + 4.0 * (keep + cout + nc * (probabilistic ? 2 : 1))), st);
    const dim3 grid((unsigned)blocks), block(LNT);
#define LP_LAUNCH(NC_, CO_) hipLaunchKernelGGL((label_prepare_kernel<NC_, CO_>), grid, block, 0, st, ann, image, x_out, detection, kl, \
                                               H, W, C, npost, post_live, tx_n, ty_n, vec, tp)
    if (nc == 2) {
        switch (cout) {
            case 1: LP_LAUNCH(2, 1); break;
            case 2: LP_LAUNCH(2, 2); break;
            case 3: LP_LAUNCH(2, 3); break;
            case 4: LP_LAUNCH(2, 4); break;
            default: LP_LAUNCH(2, 5); break;
        }
    } else {
        if (cout == 1) LP_LAUNCH(3, 1); else LP_LAUNCH(3, 3);
    }
#undef LP_LAUNCH
    return m1_check_launch();
}
