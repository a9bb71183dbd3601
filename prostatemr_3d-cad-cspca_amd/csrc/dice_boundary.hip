// dice_boundary.hip -- Soft Dice + Boundary (surface) loss of losses.py:66-130 (SoftDicePlusBoundarySurface) on the GPU.
//
// Signed distance map (L:83-99): for every sample n and foreground class c >= 1, pos = (y_true[...,c] != 0) and
//   phi = edt(~pos) * ~pos - (edt(pos) - 1) * pos          (scipy.ndimage.distance_transform_edt, unit spacing)
// computed as an EXACT squared Euclidean distance transform in three separable passes (W, then H, then D):
//   f_out(x) = min_y ((x - y)^2 + f_in(y))                  (int32; DT_INF = "no feature voxel on this line", saturating)
// Both transforms run in the same passes: .x = squared distance to the nearest foreground voxel, .y = to the nearest background
// voxel.  Each output is a brute-force minimum over the line staged in LDS (every line is <= DT_MAX_LINE long); the three passes
// take 85 us at (2,20,160,160,2) (profiles/dice_boundary_loss.txt), the bulk of the loss's cost.  The last pass takes the sqrt in fp64, applies the sign and writes
// phi (N,D,H,W,nc-1) fp32.  A class with no foreground voxel gives phi = 0 (L:95); one with no background voxel (the class fills
// the sample, where scipy's transform is degenerate) also gives phi = 0 -- this package's one deviation.
//
// Loss, per head h over all n, voxels v and classes c >= 1 (K.flatten: one ratio over the whole batch):
//   q_c = clip(p_c / sum_k p_k, eps, 1-eps);  I_h = sum y_c q_c;  Dn_h = sum (y_c + q_c);  B_h = sum q_c phi_c
//   loss = mean_h [ w0 (1 - 2 I_h / (Dn_h + smooth)) + w1 B_h ]
// forward: fp64 per-block partials of (I, Dn, B) for every head, folded in a fixed order by one block, which also keeps I_h and
// Dn_h in the workspace; backward: one element-wise pass reading them and dloss from device memory (no host sync).
#include "common.h"

#define DB_MAX_HEADS 4
#define DB_MAX_NC 8
#define DT_MAX_LINE 256           // longest D, H or W the LDS tiling holds
#define DT_INF 0x3fffffff         // (x-y)^2 + DT_INF > DT_INF, and DT_INF + 3 * 255^2 < 2^31: min() saturates without overflow
#define DT_TC 32                  // columns per block of the strided passes (32 x int2 = 256 B per staged row)
#define DB_EPS 1e-7f

template <typename TY> __device__ __forceinline__ float db_ld_y(const void* y, long long i);
template <> __device__ __forceinline__ float db_ld_y<float>(const void* y, long long i) { return ((const float*)y)[i]; }
template <> __device__ __forceinline__ float db_ld_y<unsigned short>(const void* y, long long i) {
    return __uint_as_float((unsigned)((const unsigned short*)y)[i] << 16);
}

__device__ __forceinline__ int2 dt_min_line(const int2* __restrict__ line, int stride, int L, int x) {
    int2 b = make_int2(DT_INF, DT_INF);
    for (int y = 0; y < L; ++y) {
        const int2 f = line[y * stride];
        const int dd = __mul24(x - y, x - y);                 // |x - y| < 256: the full-rate 24-bit multiply
        b.x = min(b.x, f.x + dd);
        b.y = min(b.y, f.y + dd);
    }
    return b;
}

// pass 1, along W: one wave per (n,d,h) row.  Reads the row's nc labels (contiguous), stages the 0 / DT_INF seeds of both
// transforms for the nc-1 foreground classes in LDS and writes (N,D,H,W,nc-1) int2.
template <typename TY>
__global__ void __launch_bounds__(256) dt_pass_w_kernel(const void* __restrict__ y, long long rows, int W, int nc,
                                                        int2* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int cp = nc - 1, wave = threadIdx.x >> 6, lane = threadIdx.x & 63, n_el = W * cp;
    int2* s = (int2*)smem + wave * n_el;
    const long long row = (long long)blockIdx.x * 4 + wave;
    const bool ok = row < rows;
    for (int i = lane; ok && i < n_el; i += 64) {
        const int w = i / cp, c = i - w * cp;
        const bool fg = db_ld_y<TY>(y, (row * W + w) * nc + 1 + c) != 0.f;
        s[i] = fg ? make_int2(0, DT_INF) : make_int2(DT_INF, 0);
    }
    __syncthreads();
    for (int i = lane; ok && i < n_el; i += 64) {
        const int w = i / cp, c = i - w * cp;
        out[row * n_el + i] = dt_min_line(s + c, cp, W, w);
    }
}

// passes 2 and 3, along a strided axis: element (o, t, j) at (o * L + t) * inner + j, t the line position.  A block stages the
// whole line for DT_TC adjacent columns j (coalesced 256-B rows) and computes DT_CH output positions of them.  LAST: write phi.
#define DT_CH 32
template <bool LAST>
__global__ void __launch_bounds__(256) dt_pass_strided_kernel(const int2* __restrict__ in, long long outer, int L, long long inner,
                                                              int2* __restrict__ out, float* __restrict__ phi) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    int2* s = (int2*)smem;                                      // [L][DT_TC]
    const long long ctiles = (inner + DT_TC - 1) / DT_TC;
    const int chunks = (L + DT_CH - 1) / DT_CH;
    long long b = blockIdx.x;
    const long long ct = b % ctiles; b /= ctiles;
    const int ch = (int)(b % chunks);
    const long long o = b / chunks;
    const int col = threadIdx.x & (DT_TC - 1), r0 = threadIdx.x / DT_TC;
    const long long j = ct * DT_TC + col;
    const bool cok = j < inner;
    const int2* src = in + o * L * inner + j;
    for (int t = r0; t < L; t += 256 / DT_TC) s[t * DT_TC + col] = cok ? src[(long long)t * inner] : make_int2(DT_INF, DT_INF);
    __syncthreads();
    if (!cok) return;
    const int t1 = min(L, (ch + 1) * DT_CH);
    for (int x = ch * DT_CH + r0; x < t1; x += 256 / DT_TC) {
        const int2 d = dt_min_line(s + col, DT_TC, L, x);
        const long long idx = (o * L + x) * inner + j;
        if (!LAST) {
            out[idx] = d;
        } else {
            float v;
            if (d.x == 0) v = d.y >= DT_INF ? 0.f : (float)(1.0 - sqrt((double)d.y));   // inside: -(edt(pos) - 1)
            else v = d.x >= DT_INF ? 0.f : (float)sqrt((double)d.x);                      // outside: edt(~pos)
            phi[idx] = v;
        }
    }
}

static inline long long db_grid(long long n, long long cap) { long long b = (n + 255) / 256; return b > cap ? cap : (b < 1 ? 1 : b); }

extern "C" size_t m1_dist_map_ws_bytes(int N, int D, int H, int W, int nc) {
    if (N <= 0 || D <= 0 || H <= 0 || W <= 0 || nc < 2) return 0;
    return (size_t)2 * N * D * H * W * (nc - 1) * sizeof(int2);
}

extern "C" int m1_dist_map(const void* y_true, int y_dtype, int N, int D, int H, int W, int nc, void* ws, float* out, void* stream) {
    if (!y_true || !ws || !out || N <= 0 || D <= 0 || H <= 0 || W <= 0 || nc < 2) return M1_ERR_BAD_ARG;
    if (nc > DB_MAX_NC || D > DT_MAX_LINE || H > DT_MAX_LINE || W > DT_MAX_LINE || (y_dtype != M1_F32 && y_dtype != M1_BF16))
        return M1_ERR_UNSUPPORTED;
    hipStream_t st = (hipStream_t)stream;
    const int cp = nc - 1;
    const long long vox = (long long)N * D * H * W * cp;
    int2* a = (int2*)ws;
    int2* b = a + vox;
    const long long rows = (long long)N * D * H;
    const size_t lds_w = (size_t)4 * W * cp * sizeof(int2);
    // along H: outer (n,d), inner (w,c);  along D: outer n, inner (h,w,c)
    const long long in_h = (long long)W * cp, in_d = (long long)H * W * cp;
    const long long gh = (long long)N * D * ((H + DT_CH - 1) / DT_CH) * ((in_h + DT_TC - 1) / DT_TC);
    const long long gd = (long long)N * ((D + DT_CH - 1) / DT_CH) * ((in_d + DT_TC - 1) / DT_TC);
    if (gh > 0x7fffffffLL || gd > 0x7fffffffLL || (rows + 3) / 4 > 0x7fffffffLL) return M1_ERR_UNSUPPORTED;
    if (y_dtype == M1_F32)
        hipLaunchKernelGGL(dt_pass_w_kernel<float>, dim3((unsigned)((rows + 3) / 4)), dim3(256), lds_w, st, y_true, rows, W, nc, a);
    else
        hipLaunchKernelGGL(dt_pass_w_kernel<unsigned short>, dim3((unsigned)((rows + 3) / 4)), dim3(256), lds_w, st, y_true, rows, W,
                           nc, a);
    hipLaunchKernelGGL(dt_pass_strided_kernel<false>, dim3((unsigned)gh), dim3(256), (size_t)H * DT_TC * sizeof(int2), st, a,
                       (long long)N * D, H, in_h, b, (float*)nullptr);
    hipLaunchKernelGGL(dt_pass_strided_kernel<true>, dim3((unsigned)gd), dim3(256), (size_t)D * DT_TC * sizeof(int2), st, b,
                       (long long)N, D, in_d, (int2*)nullptr, out);
    return m1_check_launch();
}

// ---------------------------------------------------------------------------------------------------------------------------
struct DiceBdP {
    const float* probs; const void* y; const float* phi;
    long long NV; int nheads, nc;
    float w0, w1, smooth;
};

// workspace (doubles): [0, nheads) I_h, [nheads, 2 nheads) Dn_h, then the partials [(q * nheads + h) * blocks + block], q = I, Dn, B
static inline int db_blocks(long long NV) { long long b = (NV + 255) / 256; return (int)(b > 2048 ? 2048 : (b < 1 ? 1 : b)); }

template <typename TY>
__global__ void __launch_bounds__(256) dice_bd_fwd_kernel(DiceBdP p, double* __restrict__ part) {
    double acc[3][DB_MAX_HEADS];
    for (int q = 0; q < 3; ++q)
        for (int h = 0; h < DB_MAX_HEADS; ++h) acc[q][h] = 0.0;
    const int cp = p.nc - 1;
    for (long long v = (long long)blockIdx.x * 256 + threadIdx.x; v < p.NV; v += (long long)gridDim.x * 256) {
        float y[DB_MAX_NC], f[DB_MAX_NC];
        for (int c = 1; c < p.nc; ++c) { y[c] = db_ld_y<TY>(p.y, v * p.nc + c); f[c] = p.phi[v * cp + c - 1]; }
        const float* pp = p.probs + v * (p.nheads * p.nc);
        for (int h = 0; h < DB_MAX_HEADS; ++h) {
            if (h >= p.nheads) break;
            float s = 0.f;
            for (int c = 0; c < p.nc; ++c) s += pp[h * p.nc + c];
            float i_ = 0.f, d_ = 0.f, b_ = 0.f;
            for (int c = 1; c < p.nc; ++c) {
                const float q = fminf(fmaxf(pp[h * p.nc + c] / s, DB_EPS), 1.f - DB_EPS);
                i_ += y[c] * q; d_ += y[c] + q; b_ += q * f[c];
            }
            acc[0][h] += i_; acc[1][h] += d_; acc[2][h] += b_;
        }
    }
    __shared__ double red[3][DB_MAX_HEADS][4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int q = 0; q < 3; ++q)
        for (int h = 0; h < DB_MAX_HEADS; ++h) {
            if (h >= p.nheads) break;
            const double a = wave_sum_d(acc[q][h]);
            if (lane == 0) red[q][h][wave] = a;
        }
    __syncthreads();
    if (threadIdx.x < 3 * p.nheads) {
        const int q = threadIdx.x / p.nheads, h = threadIdx.x - q * p.nheads;
        part[2 * p.nheads + (long long)threadIdx.x * gridDim.x + blockIdx.x] = (red[q][h][0] + red[q][h][1]) + (red[q][h][2] + red[q][h][3]);
    }
}

// one block: fold the partials of every (q, h) in a fixed order (all rows in one sweep: one round of loads, not one per row);
// loss and the kept I_h, Dn_h
__global__ void __launch_bounds__(256) dice_bd_finish_kernel(double* __restrict__ ws, int nheads, int blocks, float w0, float w1,
                                                             float smooth, float* __restrict__ loss) {
    __shared__ double red[3 * DB_MAX_HEADS][4];
    const double* part = ws + 2 * nheads;
    const int R = 3 * nheads, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double a[3 * DB_MAX_HEADS];
#pragma unroll
    for (int r = 0; r < 3 * DB_MAX_HEADS; ++r) a[r] = 0.0;
    for (int i = threadIdx.x; i < blocks; i += 256) {
#pragma unroll
        for (int r = 0; r < 3 * DB_MAX_HEADS; ++r)
            if (r < R) a[r] += part[(long long)r * blocks + i];
    }
#pragma unroll
    for (int r = 0; r < 3 * DB_MAX_HEADS; ++r)
        if (r < R) { const double v = wave_sum_d(a[r]); if (lane == 0) red[r][wave] = v; }
    __syncthreads();
    if (threadIdx.x == 0) {
        double l = 0.0;
        for (int h = 0; h < nheads; ++h) {
            double t[3];
            for (int q = 0; q < 3; ++q) { const int r = q * nheads + h; t[q] = (red[r][0] + red[r][1]) + (red[r][2] + red[r][3]); }
            ws[h] = t[0]; ws[nheads + h] = t[1];
            l += (double)w0 * (1.0 - 2.0 * t[0] / (t[1] + (double)smooth)) + (double)w1 * t[2];
        }
        loss[0] = (float)(l / nheads);
    }
}

// dp_k = (g_k - sum_c g_c p_c / S) / S,  g_c = dloss/nheads * (a_h y_c + b_h + w1 phi_c) inside the clip range (c >= 1), g_0 = 0,
// a_h = -2 w0 / (Dn_h + smooth),  b_h = 2 w0 I_h / (Dn_h + smooth)^2
template <typename TY>
__global__ void __launch_bounds__(256) dice_bd_bwd_kernel(DiceBdP p, const double* __restrict__ ws, const float* __restrict__ go,
                                                          float* __restrict__ dprobs) {
    const float sc = go[0] / (float)p.nheads;
    float ah[DB_MAX_HEADS], bh[DB_MAX_HEADS];
    for (int h = 0; h < DB_MAX_HEADS; ++h) {
        if (h >= p.nheads) { ah[h] = bh[h] = 0.f; continue; }
        const double den = ws[p.nheads + h] + (double)p.smooth;
        ah[h] = (float)(-2.0 * p.w0 / den);
        bh[h] = (float)(2.0 * p.w0 * ws[h] / (den * den));
    }
    const int cp = p.nc - 1;
    for (long long v = (long long)blockIdx.x * 256 + threadIdx.x; v < p.NV; v += (long long)gridDim.x * 256) {
        float y[DB_MAX_NC], f[DB_MAX_NC];
        for (int c = 1; c < p.nc; ++c) { y[c] = db_ld_y<TY>(p.y, v * p.nc + c); f[c] = p.phi[v * cp + c - 1]; }
        const float* pp = p.probs + v * (p.nheads * p.nc);
        float* dp = dprobs + v * (p.nheads * p.nc);
        for (int h = 0; h < DB_MAX_HEADS; ++h) {
            if (h >= p.nheads) break;
            float s = 0.f, pc[DB_MAX_NC], g[DB_MAX_NC], gp = 0.f;
            for (int c = 0; c < p.nc; ++c) { pc[c] = pp[h * p.nc + c]; s += pc[c]; }
            const float inv = 1.f / s;
            g[0] = 0.f;
            for (int c = 1; c < p.nc; ++c) {
                const float r = pc[c] / s;
                g[c] = (r >= DB_EPS && r <= 1.f - DB_EPS) ? ah[h] * y[c] + bh[h] + p.w1 * f[c] : 0.f;
                gp += g[c] * pc[c];
            }
            for (int c = 0; c < p.nc; ++c) dp[h * p.nc + c] = sc * (g[c] - gp * inv) * inv;
        }
    }
}

static int dice_bd_fill(DiceBdP& p, const float* probs, const void* y, int y_dtype, const float* phi, long long NV, int nheads,
                        int nc, float w0, float w1, float smooth) {
    if (!probs || !y || !phi || NV <= 0 || nc < 2 || nheads <= 0) return M1_ERR_BAD_ARG;
    if (nheads > DB_MAX_HEADS || nc > DB_MAX_NC || (y_dtype != M1_F32 && y_dtype != M1_BF16)) return M1_ERR_UNSUPPORTED;
    p.probs = probs; p.y = y; p.phi = phi; p.NV = NV; p.nheads = nheads; p.nc = nc; p.w0 = w0; p.w1 = w1; p.smooth = smooth;
    return M1_OK;
}

extern "C" size_t m1_dice_bd_ws_floats(long long NV, int nheads) {
    if (NV <= 0 || nheads <= 0 || nheads > DB_MAX_HEADS) return 0;
    return (size_t)2 * (2 * nheads + (size_t)3 * nheads * db_blocks(NV));
}

extern "C" int m1_dice_bd_fwd(const float* probs, const void* y_true, int y_dtype, const float* phi, long long NV, int nheads, int nc,
                              float w0, float w1, float smooth, float* ws, float* loss, void* stream) {
    DiceBdP p; int rc = dice_bd_fill(p, probs, y_true, y_dtype, phi, NV, nheads, nc, w0, w1, smooth);
    if (rc != M1_OK) return rc;
    if (!ws || !loss || ((uintptr_t)ws & 7)) return M1_ERR_BAD_ARG;
    const int blocks = db_blocks(NV);
    hipStream_t st = (hipStream_t)stream;
    if (y_dtype == M1_F32) hipLaunchKernelGGL(dice_bd_fwd_kernel<float>, dim3(blocks), dim3(256), 0, st, p, (double*)ws);
    else hipLaunchKernelGGL(dice_bd_fwd_kernel<unsigned short>, dim3(blocks), dim3(256), 0, st, p, (double*)ws);
    hipLaunchKernelGGL(dice_bd_finish_kernel, dim3(1), dim3(256), 0, st, (double*)ws, nheads, blocks, w0, w1, smooth, loss);
    return m1_check_launch();
}

extern "C" int m1_dice_bd_bwd(const float* probs, const void* y_true, int y_dtype, const float* phi, long long NV, int nheads, int nc,
                              float w0, float w1, float smooth, const float* ws, const float* dloss, float* dprobs, void* stream) {
    DiceBdP p; int rc = dice_bd_fill(p, probs, y_true, y_dtype, phi, NV, nheads, nc, w0, w1, smooth);
    if (rc != M1_OK) return rc;
    if (!ws || !dloss || !dprobs || ((uintptr_t)ws & 7)) return M1_ERR_BAD_ARG;
    const long long blocks = db_grid(NV, 4096);
    hipStream_t st = (hipStream_t)stream;
    if (y_dtype == M1_F32)
        hipLaunchKernelGGL(dice_bd_bwd_kernel<float>, dim3((unsigned)blocks), dim3(256), 0, st, p, (const double*)ws, dloss, dprobs);
    else
        hipLaunchKernelGGL(dice_bd_bwd_kernel<unsigned short>, dim3((unsigned)blocks), dim3(256), 0, st, p, (const double*)ws, dloss,
                           dprobs);
    return m1_check_launch();
}
