// wgrad_tf.hip -- tap-fused weight gradients (bf16) for the wide, shallow layers (res0..res2: many voxels, <= 32
// channels per tile), where the per-tap kernel of wgrad_mfma.hip re-reads both operands once per tap.
//
//   R[tap][a][b] += sum_{n,v} A[n, v*s + tap - p][a] * B[n, v][b]            all taps of a (1,3,3)/(3,3,3) kernel at once
//
// * One block owns a 32(a) x 32(b) channel tile and walks K-tiles of 64 or 128 output voxels (2 or 4 k-steps of 32: rows x
//   KWs columns, KWs = 32/16/8 dividing the row length; 128 for the (1,3,3) kernels, see tf_plan).  Per K-tile it stages, by LDS-DMA (global_load_lds_dwordx4,
//   no staging registers), the 64 B rows and the A rows of the tile INCLUDING the tap halo -- every A voxel is loaded
//   once for all taps -- in their natural voxel-major layout.
// * The MFMA wants K(=voxel)-contiguous fragments: ds_read_b64_tr_b16 (gfx950 transpose read) takes a
//   [4 voxels][16 channels] block per 16-lane group and hands lane i channel i of the 4 voxels, so a tap is just a
//   different ROW offset into the same A tile (no register transposes, no unaligned LDS reads).
//   Probe of the instruction's lane mapping: tools/probes/tr_b16_probe.hip.
// * wave w accumulates the 16x16 tile (w>>1, w&1) of every tap: NT x 4 accumulator registers; the B fragment of a
//   k-step is read once and reused by all taps.  With 32 channels on both sides (KPARTS == 1) the M32 body runs instead: one
//   wave per 32x32 tile of its own taps on v_mfma_f32_32x32x16_bf16 (see there).
// * K-tiles are dealt round-robin to the blocks of a channel tile; every block stores its partial tile into its own copy of the
//   member's gradient block and a fold (wgrad_fold.hip: tf_finish_*, queued and run in batches) adds the copies in a fixed
//   order -- no floating-point atomics.  The equal-width members of a concat share one launch (blockIdx.z = member).
#include "common.h"
#include "wgrad_fold.h"
#include "cdna4.h"
#include <stdlib.h>

#define TF_MAX_NKS 4        // k-steps (of 32 voxels) per K-tile: 2, or 4 for the <= 16-channel layers (see tf_plan)
#define TF_MAX_AIT 10       // LDS-DMA pieces per thread for the A tile

struct TfP {
    const bf16_t* A; const bf16_t* B; float* R; float* bsum;
    int CA, CB, AD, AH, AW, BD, BH, BW, N;
    long long RT, RSA; int a_off, b_off;
    int sd, sh, sw, pd, ph, pw;
    int KWs, TH;             // k-step = (32/KWs) rows x KWs columns; K-tile = TH = nks*(32/KWs) rows x KWs columns
    int AHt, AWt;            // A tile extent per kd slice (rows, columns) incl. halo
    int spra, sprb;          // 16-byte slots per LDS row = min(C, 32)/8
    int a_slots, b_slots;    // slots of the A / B tile (a_slots rounded up to whole waves)
    int a_bytes, b_bytes;    // LDS bytes per buffer (with slack for the 32-byte fragment reads of short rows)
    int tiles_w, tiles_h; long long ntiles;
    int bTiles, nsplit;
    int stages;              // LDS pipeline depth (tiles staged ahead of the MFMAs + 1)
    float* Rx; long long rx_stride;      // per-XCD private copies of R (+ bias sums behind it): see the epilogue
    long long rx_bias;       // offset of the bias sums inside one copy
    int nks;                 // k-steps per K-tile (template TF_NKS of the kernel)
    // several concat members of one conv in ONE launch (same geometry and channel count, blockIdx.z = member): a per-member launch
    // of ~256 blocks leaves one block per CU; member m reads Am[m] and stores into the copies at Rx + m * rx_mem
    int nmem; const bf16_t* Am[M1_MAX_SRC]; long long rx_mem;
};

#define TF_MAX_STAGES 8

// M32 (KPARTS == 1 only, M1_TF_MFMA32): the 32x32x16 body -- one wave computes the whole 32 x 32 tile of ITS taps (see below);
// staging, K-tiles, pipeline and the partial-copy layout are the same code.
template <int KD, int KH, int KW, int KPARTS, int TF_NKS, bool M32 = false>
__global__ void __launch_bounds__(256, M32 ? 2 : 1) wgrad_tf_kernel(TfP p) {
#if defined(__HIP_DEVICE_COMPILE__)      // (buffer-resource builtins do not exist in the host pass)
    constexpr int NT = KD * KH * KW, NG = KD * KH;           // taps; tap groups (the KW taps of one (kd,kh) share a row offset)
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    // waves -> (16x16 output tile, tap part): with <= 16 channels on a side there are only 2 or 1 tiles and the waves that
    // share a tile split the taps between them (tap t belongs to part t % kparts)
    constexpr int kparts = KPARTS, ntile = 4 / KPARTS;       // host: ntile = (CA > 16 ? 2 : 1) * (CB > 16 ? 2 : 1)
    const int ntb = p.CB > 16 ? 2 : 1;
    const int tile_id = wave % ntile, part = wave / ntile;
    const int ta = tile_id / ntb, tb = tile_id % ntb;
    const int a0 = (blockIdx.x / p.bTiles) * 32, b0 = (blockIdx.x % p.bTiles) * 32;
    const int mem = p.nmem > 1 ? (int)blockIdx.z : 0;
    const bf16_t* Abase = p.A;
    if (p.nmem > 1) {         // (a chain of uniform selects: a dynamic index would move the whole argument struct to scratch memory)
        Abase = p.Am[0];
#pragma unroll
        for (int m = 1; m < M1_MAX_SRC; ++m) if (mem == m) Abase = p.Am[m];
    }
    const int PA = p.spra * 16, PB = p.sprb * 16;            // LDS row pitch (bytes)
    const int stage_bytes = p.a_bytes + p.b_bytes;           // [A tile][B tile] per stage

    // ---- per-lane description of its LDS-DMA pieces (the same for every K-tile).  Every wave issues nait + 1 pieces
    //      per stage (tiles padded to whole 256-slot rounds, padding fetches the zero page): static vmcnt arithmetic ----
    // (buffer loads: tile origin in the resource base, constant 32-bit lane offsets, 2^31 = out of range -> zeros)
    constexpr unsigned OOB = 0x80000000u;
    unsigned a_vo[TF_MAX_AIT]; int a_pk[TF_MAX_AIT];
    const int nait = p.a_slots >> 8;
#pragma unroll
    for (int it = 0; it < TF_MAX_AIT; ++it) {
        const int q = it * 256 + tid;
        const int row = q / p.spra, slp = q - row * p.spra;
        const int dd = row / (p.AHt * p.AWt); const int r2 = row - dd * (p.AHt * p.AWt);
        const int hh = r2 / p.AWt, ww = r2 - hh * p.AWt;
        // 64-byte rows: the two 32-byte halves of a row swap when bit 3 of the tile column is set -- lane groups 0/1 of a
        // transpose read sit 8 columns apart and would otherwise hit the same banks
        const int sl = p.spra == 4 ? (slp ^ (((ww >> 3) & 1) << 1)) : slp;
        a_pk[it] = dd | (hh << 8) | (ww << 16);
        a_vo[it] = (row < KD * p.AHt * p.AWt) ? (unsigned)((((dd * p.AH + hh) * p.AW + ww) * p.CA + a0 + sl * 8) * 2) : OOB;
    }
    constexpr int NBIT = (TF_NKS * 32 * 4 + 255) / 256;      // LDS-DMA pieces per thread for the B tile (max)
    const int nbit = (p.b_slots + 255) >> 8;
    unsigned b_vo[NBIT]; int b_th[NBIT];
#pragma unroll
    for (int it = 0; it < NBIT; ++it) {
        const int q = it * 256 + tid;
        const int row = q / p.sprb, slp = q - row * p.sprb;
        const int th = row / p.KWs, tw = row - th * p.KWs;
        const int sl = p.sprb == 4 ? (slp ^ (((tw >> 3) & 1) << 1)) : slp;
        b_th[it] = th;
        b_vo[it] = q < p.b_slots ? (unsigned)(((th * p.BW + tw) * p.CB + b0 + sl * 8) * 2) : OOB;
    }

    // tile counter of the NEXT tile to issue, decoded incrementally (no divisions in the loop)
    int q_kt = blockIdx.y, q_tw, q_th, q_bd, q_n;
    { int r = q_kt; q_tw = r % p.tiles_w; r /= p.tiles_w; q_th = r % p.tiles_h; r /= p.tiles_h; q_bd = r % p.BD; q_n = r / p.BD; }
    int s_tw, s_th, s_bd, s_n;
    { int r = p.nsplit; s_tw = r % p.tiles_w; r /= p.tiles_w; s_th = r % p.tiles_h; r /= p.tiles_h; s_bd = r % p.BD; s_n = r / p.BD; }
    auto issue = [&](int st) {
        const bool live = q_kt < (int)p.ntiles;
        const int twi = q_tw, thi = q_th, bd = q_bd, n = q_n;
        q_kt += p.nsplit;
        q_tw += s_tw; int c = q_tw >= p.tiles_w; q_tw -= c ? p.tiles_w : 0;
        q_th += s_th + c; c = q_th >= p.tiles_h; q_th -= c ? p.tiles_h : 0;
        q_bd += s_bd + c; c = q_bd >= p.BD; q_bd -= c ? p.BD : 0;
        q_n += s_n + c;
        const int ad0 = bd * p.sd - p.pd, ah0 = thi * p.TH * p.sh - p.ph, aw0 = twi * p.KWs * p.sw - p.pw;
        const long long lin0 = (((long long)n * p.AD + ad0) * p.AH + ah0) * p.AW + aw0;
        const int bh0 = thi * p.TH;
        const long long blin0 = (((long long)n * p.BD + bd) * p.BH + bh0) * p.BW + twi * p.KWs;
        unsigned char* As = smem + st * stage_bytes;
        unsigned char* Bs = As + p.a_bytes;
        const __amdgpu_buffer_rsrc_t ra = __builtin_amdgcn_make_buffer_rsrc((void*)(Abase + lin0 * p.CA), 0, live ? 0x7fffffff : 0, 0x00020000);
        const __amdgpu_buffer_rsrc_t rb = __builtin_amdgcn_make_buffer_rsrc((void*)(p.B + blin0 * p.CB), 0, live ? 0x7fffffff : 0, 0x00020000);
        const bool a_inner = ad0 >= 0 && ad0 + KD - 1 < p.AD && ah0 >= 0 && ah0 + p.AHt - 1 < p.AH && aw0 >= 0 && aw0 + p.AWt - 1 < p.AW;
        if (a_inner) {                                     // uniform: no per-lane work
#pragma unroll
            for (int it = 0; it < TF_MAX_AIT; ++it)
                if (it < nait) __builtin_amdgcn_raw_ptr_buffer_load_lds(ra, (lptr_t)(As + (it * 256 + wave * 64) * 16), 16, a_vo[it], 0, 0, 0);
        } else {
#pragma unroll
            for (int it = 0; it < TF_MAX_AIT; ++it) {
                if (it < nait) {
                    const int pk = a_pk[it];
                    const int dd = pk & 0xff, hh = (pk >> 8) & 0xff, ww = (pk >> 16) & 0xff;
                    const bool ok = (unsigned)(ad0 + dd) < (unsigned)p.AD && (unsigned)(ah0 + hh) < (unsigned)p.AH && (unsigned)(aw0 + ww) < (unsigned)p.AW;
                    __builtin_amdgcn_raw_ptr_buffer_load_lds(ra, (lptr_t)(As + (it * 256 + wave * 64) * 16), 16, ok ? a_vo[it] : OOB, 0, 0, 0);
                }
            }
        }
        const bool b_inner = bh0 + p.TH <= p.BH;
#pragma unroll
        for (int it = 0; it < NBIT; ++it)
            if (it < nbit)
                __builtin_amdgcn_raw_ptr_buffer_load_lds(rb, (lptr_t)(Bs + (it * 256 + wave * 64) * 16), 16,
                                                         (b_inner || bh0 + b_th[it] < p.BH) ? b_vo[it] : OOB, 0, 0, 0);
    };

    if constexpr (M32) {
    // ---- v_mfma_f32_32x32x16_bf16, waves split by TAP (both sides 32 channels: 64-byte rows).  Wave w owns the taps t = w + 4 j
    //      (9 taps: 3/2/2/2, 27: 7/7/7/6) and accumulates their whole 32 x 32 tile: the dY fragment of a 16-voxel k-step is read once
    //      per wave, an X fragment by exactly one wave -- 52 / 124 transpose reads per 32 voxels and block where the 16x16x32 body
    //      below issues 80 / 224.  Operand layout as in wgrad_t3.hip: lane l supplies channel l & 31, k = 8 (l >> 5) ..; lane
    //      (g2 = l >> 4, i = l & 15) points at voxel 16 ks + 8 (g2 >> 1) + 4 h + (i >> 2), 16-channel half g2 & 1, 8-byte piece
    //      i & 3.  Lanes 0-31 (one LDS cycle) read both halves of 4 rows: with stride 1 four consecutive 64-byte rows = all 64
    //      banks once, whatever the half swap of the staging does (both halves of a row are read) -- the DMA side stays as it is.
    const unsigned lds0 = (unsigned)(unsigned long long)(lptr_t)smem;
    const int S = p.stages;
    const int npiece = nait + nbit;                            // LDS-DMA pieces per wave per stage
    const long long kt0 = blockIdx.y, step = p.nsplit;
    static_assert(KPARTS == 1 && KW == 3, "the tap split assumes 32 x 32 tiles and t % KW == (w + j) % KW");
    constexpr int NK = 2 * TF_NKS, NTW = (NT + 3) / 4;         // k-steps of 16 voxels per K-tile; taps per wave (the last may be missing)
    const int g2 = lane >> 4, i = lane & 15, kg = g2 >> 1, ch = g2 & 1;
    // byte addresses inside stage 0 of k-step 0, tap row (kd,kh) = (0,0); a_ad[h][r]: kw = (wave + r) % KW.  K-step ks lies 16 ks voxel
    // slots on: whole rows and multiples of 16 columns (KWs = 8 / 16 / 32), which leave the half swap (bit 3 of the column) alone --
    // a wave-uniform offset, (ks >> 1) * ko2 + (ks & 1) * ko1 for X and 16 ks rows for dY
    unsigned a_ad[2][KW], b_ad[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int kk = 8 * kg + 4 * h + (i >> 2);
        const int th = kk / p.KWs, tw = kk - th * p.KWs;
#pragma unroll
        for (int r = 0; r < KW; ++r) {
            const int ww = tw * p.sw + (wave + r) % KW;
            a_ad[h][r] = lds0 + ((th * p.sh) * p.AWt + ww) * PA + (ch ^ ((ww >> 3) & 1)) * 32 + (i & 3) * 8;
        }
        b_ad[h] = lds0 + p.a_bytes + kk * PB + (ch ^ ((tw >> 3) & 1)) * 32 + (i & 3) * 8;
    }
    const unsigned ko1 = (unsigned)(((16 / p.KWs) * p.sh * p.AWt + (16 % p.KWs) * p.sw) * PA);
    const unsigned ko2 = (unsigned)(((32 / p.KWs) * p.sh * p.AWt + (32 % p.KWs) * p.sw) * PA);
    unsigned ro[NTW];                                          // (wave-uniform) byte offset of the tap row (kd,kh) of tap j
#pragma unroll
    for (int j = 0; j < NTW; ++j) {
        const int tg = (wave + 4 * j) / KW;
        ro[j] = (unsigned)(((tg / KH) * p.AHt + tg % KH) * p.AWt * PA);
    }
    const bool last_ok = wave + 4 * (NTW - 1) < NT;            // this wave has NTW taps (else NTW - 1)

    f32x16_t acc[NTW];
#pragma unroll
    for (int j = 0; j < NTW; ++j)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[j][e] = 0.f;
    const bool do_bsum = p.bsum != nullptr && a0 == 0 && wave == 3 && mem == 0;      // (wave 3 has the fewest taps)
    // bias sums as the 16x16x32 body takes them, a ones operand in front of the dY fragment (every row of the tile = the column sums): the
    // MFMA adds its k values in order, so two K = 16 steps leave the bits one K = 32 step leaves -- the same holds for the taps
    f32x16_t accb;
#pragma unroll
    for (int e = 0; e < 16; ++e) accb[e] = 0.f;
    const bf16x8_t ones = __builtin_bit_cast(bf16x8_t, make_uint4(0x3F803F80u, 0x3F803F80u, 0x3F803F80u, 0x3F803F80u));

    // the K-tile at stage offset sb for a wave with N taps, as a flat list of ITEMS of two transpose reads each: per k-step the dY
    // fragment, then the X fragments of the N taps (one MFMA each).  Reads run D items ahead of the MFMAs through a ring of D + 1
    // fragment slots; LDS reads return in order, so item m has landed once at most 2 * (items issued after m) reads are in flight.
    auto tile = [&](unsigned sb, auto n_c) {
        constexpr int N = decltype(n_c)::value, NI = NK * (N + 1);
        constexpr int D = N + 1 < 6 ? N + 1 : 6, RS = D + 1;   // (D <= N + 1: the dY fragment of k-step u lives until u + 2 is read)
        u32x2_t bl[2], bh[2], al[RS], ah[RS];
        auto rd = [&](auto m_c) {
            constexpr int m = decltype(m_c)::value, u = m / (N + 1), j = m % (N + 1) - 1;
            if constexpr (j < 0) {
                const unsigned so = sb + (unsigned)(u * 16) * PB;
                bl[u & 1] = m1_tr_read_asm(b_ad[0] + so); bh[u & 1] = m1_tr_read_asm(b_ad[1] + so);
            } else {
                constexpr int sl = (u * N + j) % RS;
                const unsigned so = sb + ro[j] + (u >> 1) * ko2 + (u & 1) * ko1;
                al[sl] = m1_tr_read_asm(a_ad[0][j % KW] + so); ah[sl] = m1_tr_read_asm(a_ad[1][j % KW] + so);
            }
        };
        m1_static_for<0, D>(rd);
        bf16x8_t bfr;
        m1_static_for<0, NI>([&](auto m_c) {
            constexpr int m = decltype(m_c)::value, u = m / (N + 1), j = m % (N + 1) - 1;
            if constexpr (m + D < NI) rd(std::integral_constant<int, m + D>{});
            constexpr int after = NI - 1 - m < D ? NI - 1 - m : D;
            if constexpr (j < 0) {
                m1_lds_wait_n<2 * after>(bl[u & 1], bh[u & 1]);
                bfr = m1_frag8(bl[u & 1], bh[u & 1]);
                if (do_bsum) accb = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ones, bfr, accb, 0, 0, 0);
            } else {
                constexpr int sl = (u * N + j) % RS;
                m1_lds_wait_n<2 * after>(al[sl], ah[sl]);
                acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(m1_frag8(al[sl], ah[sl]), bfr, acc[j], 0, 0, 0);
            }
            __builtin_amdgcn_sched_barrier(0);
        });
    };

    // the S-deep pipeline of the 16x16x32 body below around `tile(stage byte offset)`
    auto run_tiles = [&](auto&& tile_fn) {
        for (int s = 0; s < S - 1; ++s) issue(s);
        int st = 0;
        for (long long kt = kt0; kt < p.ntiles; kt += step) {
            m1_wait_vm<48>(npiece * (S - 2));         // this wave's pieces of tile kt have landed ...
            __builtin_amdgcn_s_barrier();                      // ... and everybody's; everybody is also done with tile kt - step
            int stn = st + S - 1; if (stn >= S) stn -= S;
            issue(stn);                                        // refill the buffer tile kt - step was read from
            tile_fn((unsigned)(st * stage_bytes));
            if (++st == S) st = 0;
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");       // the padding stages of the tail
    };
    // (one K loop per tap count: a choice inside the loop makes the accumulators change registers where the two paths meet)
    if (last_ok) run_tiles([&](unsigned sb) { tile(sb, std::integral_constant<int, NTW>{}); });
    else run_tiles([&](unsigned sb) { tile(sb, std::integral_constant<int, NTW - 1>{}); });

    // ---- D[a][b] of a 32x32 tile: lane holds b = lane & 31, a = (e & 3) + 8 (e >> 2) + 4 (lane >> 5); same copy layout as below ----
    float* Rx = p.Rx + (long long)mem * p.rx_mem + (long long)blockIdx.y * p.rx_stride;
    const int b = b0 + (lane & 31);
    if (do_bsum && lane < 32 && b < p.CB) Rx[p.rx_bias + b] = accb[0];
#pragma unroll
    for (int j = 0; j < NTW; ++j) {
        const int t = wave + 4 * j;
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int a = a0 + (e & 3) + 8 * (e >> 2) + 4 * (lane >> 5);
            if (t < NT && a < p.CA && b < p.CB) Rx[((long long)t * p.CA + a) * p.CB + b] = acc[j][e];
        }
    }
    } else {
    // ---- fragment read addresses: lane (g = lane>>4, i = lane&15) supplies voxel 8g + 4h + (i>>2), 8-byte piece i&3 ----
    const int g = lane >> 4, i = lane & 15;
    const unsigned lds0 = (unsigned)(unsigned long long)(lptr_t)smem;
    unsigned a_ad[TF_NKS][2][KW], b_ad[TF_NKS][2];            // byte addresses inside stage 0 for tap row (kd,kh) = (0,0)
#pragma unroll
    for (int ks = 0; ks < TF_NKS; ++ks)
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int kk = ks * 32 + 8 * g + 4 * h + (i >> 2);
            const int th = kk / p.KWs, tw = kk - th * p.KWs;
#pragma unroll
            for (int kw = 0; kw < KW; ++kw) {
                const int ww = tw * p.sw + kw;
                const int half = p.spra == 4 ? (ta ^ ((ww >> 3) & 1)) : ta;
                a_ad[ks][h][kw] = lds0 + ((th * p.sh) * p.AWt + ww) * PA + half * 32 + (i & 3) * 8;
            }
            const int halfb = p.sprb == 4 ? (tb ^ ((tw >> 3) & 1)) : tb;
            b_ad[ks][h] = lds0 + p.a_bytes + kk * PB + halfb * 32 + (i & 3) * 8;
        }
    const int grp_pitch = p.AWt * PA;                          // bytes between tap rows kh and kh+1 (kd: x AHt)

    f32x4_t acc[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[t] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
    const bool do_bsum = p.bsum != nullptr && a0 == 0 && ta == 0 && part == 0 && mem == 0;
    f32x4_t accb = (f32x4_t){0.f, 0.f, 0.f, 0.f};
    const bf16x8_t ones = __builtin_bit_cast(bf16x8_t, make_uint4(0x3F803F80u, 0x3F803F80u, 0x3F803F80u, 0x3F803F80u));

    // ---- S-deep pipeline: while tile j is on the MFMAs, tiles j+1 .. j+S-1 are in flight ----
    const int S = p.stages;
    const int npiece = nait + nbit;                            // LDS-DMA pieces per wave per stage
    const long long kt0 = blockIdx.y, step = p.nsplit;
    for (int s = 0; s < S - 1; ++s) issue(s);
    int st = 0;
    for (long long kt = kt0; kt < p.ntiles; kt += step) {
        m1_wait_vm<48>(npiece * (S - 2));             // this wave's pieces of tile kt have landed ...
        __builtin_amdgcn_s_barrier();                          // ... and everybody's; everybody is also done with tile kt - step
        int stn = st + S - 1; if (stn >= S) stn -= S;
        issue(stn);                                            // refill the buffer tile kt - step was read from
        const unsigned sb = (unsigned)(st * stage_bytes);
        // fragment reads run one unit (= the KH*KW taps of one kd slice for one k-step) ahead of the MFMAs
        constexpr int NU = TF_NKS * KD, CH = KH * KW;
        u32x2_t bl[2], bh[2], al[2][CH], ah[2][CH];
        auto rd_unit = [&](int u, int set) {
            const int ks = u / KD, kd = u % KD;
            if (kd == 0) { bl[ks & 1] = m1_tr_read_asm(b_ad[ks][0] + sb); bh[ks & 1] = m1_tr_read_asm(b_ad[ks][1] + sb); }
#pragma unroll
            for (int kh = 0; kh < KH; ++kh) {
                const unsigned ro = sb + (unsigned)((kd * p.AHt + kh) * grp_pitch);
#pragma unroll
                for (int kw = 0; kw < KW; ++kw) {
                    if (((kd * CH + kh * KW + kw) % kparts) == part) {
                        al[set][kh * KW + kw] = m1_tr_read_asm(a_ad[ks][0][kw] + ro);
                        ah[set][kh * KW + kw] = m1_tr_read_asm(a_ad[ks][1][kw] + ro);
                    }
                }
            }
        };
        rd_unit(0, 0);
#pragma unroll
        for (int u = 0; u < NU; ++u) {
            const int ks = u / KD, kd = u % KD, set = u & 1;
            if (kd == 0) m1_lds_wait(bl[ks & 1], bh[ks & 1]);
#pragma unroll
            for (int c = 0; c < CH; ++c) m1_lds_wait(al[set][c], ah[set][c]);
            if (u + 1 < NU) rd_unit(u + 1, set ^ 1);
            __builtin_amdgcn_sched_barrier(0);
            const bf16x8_t bfr = m1_frag8(bl[ks & 1], bh[ks & 1]);
            if (do_bsum && kd == 0) accb = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ones, bfr, accb, 0, 0, 0);
#pragma unroll
            for (int c = 0; c < CH; ++c)
                if (((kd * CH + c) % kparts) == part)
                    acc[kd * CH + c] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(m1_frag8(al[set][c], ah[set][c]), bfr, acc[kd * CH + c], 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
        }
        if (++st == S) st = 0;
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");           // the padding stages of the tail

    // ---- D[a][b]: lane holds a = 4*(lane>>4) + r, b = lane&15 ----
    // Float atomics are executed at the memory side on this multi-XCD part (~7 G requests/s in total, measured), which
    // would cost more than the whole K loop.  Every block instead STORES its partial tile into its own copy of R
    // (copy = K-split index); tf_finish_kernel adds the copies.
    float* Rx = p.Rx + (long long)mem * p.rx_mem + (long long)blockIdx.y * p.rx_stride;
    const int b = b0 + tb * 16 + i;
    if (do_bsum && g == 0 && b < p.CB) Rx[p.rx_bias + b] = accb[0];
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int a = a0 + ta * 16 + g * 4 + r;
            if ((t % kparts) == part && a < p.CA && b < p.CB) Rx[((long long)t * p.CA + a) * p.CB + b] = acc[t][r];
        }
    }
#endif
}


static inline bool tf_chan_ok(int c) { return c == 8 || c == 16 || (c >= 32 && c % 32 == 0); }

// fills the launch geometry; false = shape outside this kernel (the per-tap kernel of wgrad_mfma.hip takes it)
static bool tf_plan(const WgradSpec& g, TfP& p) {
    if (g.dtype != M1_BF16) return false;
    const bool k133 = g.kd == 1 && g.kh == 3 && g.kw == 3, k333 = g.kd == 3 && g.kh == 3 && g.kw == 3;
    if (!k133 && !k333) return false;
    if (!tf_chan_ok(g.CA) || !tf_chan_ok(g.CB)) return false;
    if (g.BW % 8) return false;
    if (!m1_wg_vox32(g)) return false;
    p = TfP{};
    p.A = (const bf16_t*)g.A; p.B = (const bf16_t*)g.B; p.R = g.R; p.bsum = g.bsum;
    p.CA = g.CA; p.CB = g.CB; p.AD = g.AD; p.AH = g.AH; p.AW = g.AW; p.BD = g.BD; p.BH = g.BH; p.BW = g.BW; p.N = g.N;
    p.RT = g.RT; p.RSA = g.RSA; p.a_off = g.a_off; p.b_off = g.b_off;
    p.sd = g.sd; p.sh = g.sh; p.sw = g.sw; p.pd = g.pd; p.ph = g.ph; p.pw = g.pw;
    // K-tile: 128 voxels (4 k-steps per barrier and DMA round trip) for the (1,3,3) kernels and wherever both sides have <= 16
    // channels; 64 for the other (3,3,3) layers, whose 3-slice input tiles would leave one block per CU.  With the members of a
    // concat in one launch (enough blocks per CU) the larger tile pays: 64 -> 32 at (2,20,160,160) 146 -> 112 us, 320 -> 64 at
    // (2,20,80,80) 358 -> 294 us, -1.2 % per C3 step.  M1_TF_NKS4: 2 (default), 1 = only the <= 16-channel layers, 0 = always 64.
    int n4 = M1_CFG("M1_TF_NKS4", 2);
    const int nks = ((n4 && g.CA <= 16 && g.CB <= 16) || (n4 == 2 && g.kd == 1)) ? 4 : 2;
    p.nks = nks;
    if (!m1_wg_ktiles(g, nks * 32, m1_wg_kws(g.BW, 8), 0, p)) return false;
    p.AHt = (p.TH - 1) * g.sh + g.kh; p.AWt = (p.KWs - 1) * g.sw + g.kw;
    p.spra = (g.CA < 32 ? g.CA : 32) / 8; p.sprb = (g.CB < 32 ? g.CB : 32) / 8;
    const int a_rows = g.kd * p.AHt * p.AWt;
    p.a_slots = (a_rows * p.spra + 255) / 256 * 256; p.b_slots = nks * 32 * p.sprb;
    if (p.a_slots > TF_MAX_AIT * 256 || p.AHt > 255 || p.AWt > 255) return false;
    p.a_bytes = p.a_slots * 16; p.b_bytes = (p.b_slots + 255) / 256 * 256 * 16 + 64;      // (+64: slack for the 32-byte fragment reads of short rows)
    // as many stages as fit ~76 KB (two blocks per CU), at least 3, bounded by the vmcnt range
    const int sb = p.a_bytes + p.b_bytes, npiece = p.a_slots / 256 + (p.b_slots + 255) / 256;
    int S = (76 * 1024) / sb;
    if (S < 3) S = 3;
    if (S > TF_MAX_STAGES) S = TF_MAX_STAGES;
    while (S > 3 && npiece * (S - 2) > 48) --S;
    { int fs = M1_CFG("M1_TF_STAGES", 0); if (fs >= 3) S = fs; }
    p.stages = S;
    return npiece * (S - 2) <= 48 && (size_t)S * sb <= 160 * 1024;
}
// 64x64 variant: both sides multiples of 64 channels
bool m1_tf_wgrad_supported(const WgradSpec& g) { TfP p; return tf_plan(g, p); }

// copies: any K-tile is worth one, no ceiling on their number, 96 MB in all.  (Looks like drift, kept: the rx region is at most
// 64 MB (M1_WG_RX_MB) and sized for 512 copies, so neither absence nor ceiling binds by default; and where the others would run
// one split this launcher declines.)
static const WgCopyRule TF_COPIES = {1, 0, 96ll << 20, WG_SHORT_ERROR};
static int tf_wgrad_launch(const WgradSpec& g, long long nw, int nb, hipStream_t st, int nmem, const void* const* Am, const int* a_offs, long long rx_mem);
// `nmem` members of one Conv3D concat at once: member m = (Am[m], a_off a_offs[m]), all with g.CA channels; copies of member m
// live at g.rx + m * rx_mem (rx_mem >= g.rx_floats of one member)
int m1_tf_wgrad_multi(const WgradSpec& g, long long nw, int nb, hipStream_t st, int nmem, const void* const* Am, const int* a_offs, long long rx_mem) {
    return tf_wgrad_launch(g, nw, nb, st, nmem, Am, a_offs, rx_mem);
}
// nw / nb: floats of the whole weight / bias gradient that g.R / g.bsum point into
int m1_tf_wgrad(const WgradSpec& g, long long nw, int nb, hipStream_t st) { return tf_wgrad_launch(g, nw, nb, st, 1, nullptr, nullptr, 0); }
static int tf_wgrad_launch(const WgradSpec& g, long long nw, int nb, hipStream_t st, int nmem, const void* const* Am, const int* a_offs, long long rx_mem) {
    TfP p;
    if (!tf_plan(g, p)) return M1_ERR_UNSUPPORTED;
    const int TS = 32;
    const int aTiles = (g.CA + TS - 1) / TS; p.bTiles = (g.CB + TS - 1) / TS;
    const int ctiles = aTiles * p.bTiles;
    // blocks per launch (M1_TF_SPLIT, 0 = by size): 256 (one per CU) up to ~24k K-tiles, 512 beyond -- isolated, the 64 -> 32 layer
    // at (20,160,160) runs 102 -> 67 us with 512, but every block adds a partial copy to fold and in the captured step other
    // kernels fill the idle SIMDs: C3 (4 volumes per launch) -2 % with 512, C2 (2 volumes) +1 %
    int tgt_env = M1_CFG("M1_TF_SPLIT", 0);
    const int tgt = tgt_env > 0 ? tgt_env : (p.ntiles >= 24576 ? 512 : 256);
    const long long want = (tgt + ctiles - 1) / ctiles;                                                        // (rounded UP)
    const WgCopies c = m1_wg_copies(g, g.kd * g.kh * g.kw, want, p.ntiles, TF_COPIES);
    if (c.rc) return c.rc;
    const long long nsplit = c.nsplit;
    p.nsplit = (int)nsplit;
    p.Rx = c.Rx; p.rx_stride = c.stride; p.rx_bias = c.rx_bias;
    const size_t smem = (size_t)p.stages * (p.a_bytes + p.b_bytes);
    dim3 grid(ctiles, (unsigned)nsplit, 1);
    p.nmem = 1; p.rx_mem = 0;
    if (nmem > 1) {
        if (nmem > M1_MAX_SRC) return M1_ERR_UNSUPPORTED;
        p.nmem = nmem; p.rx_mem = rx_mem; grid.z = (unsigned)nmem;
        for (int m = 0; m < nmem; ++m) p.Am[m] = (const bf16_t*)Am[m];
    }
    const int kparts = 4 / ((g.CA > 16 ? 2 : 1) * (g.CB > 16 ? 2 : 1));
    void (*kern)(TfP) = nullptr;
#define TF_PICK(KD_, KP_) if ((g.kd == KD_) && kparts == KP_ && p.nks == 2) kern = wgrad_tf_kernel<KD_, 3, 3, KP_, 2>;
    TF_PICK(1, 1) TF_PICK(1, 2) TF_PICK(1, 4) TF_PICK(3, 1) TF_PICK(3, 2) TF_PICK(3, 4)
#undef TF_PICK
    if (p.nks == 4 && kparts == 4) kern = g.kd == 1 ? wgrad_tf_kernel<1, 3, 3, 4, 4> : (g.kd == 3 ? wgrad_tf_kernel<3, 3, 3, 4, 4> : nullptr);
    if (p.nks == 4 && g.kd == 1 && kparts == 1) kern = wgrad_tf_kernel<1, 3, 3, 1, 4>;
    if (p.nks == 4 && g.kd == 1 && kparts == 2) kern = wgrad_tf_kernel<1, 3, 3, 2, 4>;
    // 32 channels on both sides: the 32x32x16 body with the waves split by tap (same plan, grid, stages and copies).  M1_TF_MFMA32: 0 = the
    // 16x16x32 body everywhere
    if (kparts == 1 && kern && M1_CFG("M1_TF_MFMA32", 1)) {
        if (g.kd == 3) kern = wgrad_tf_kernel<3, 3, 3, 1, 2, true>;
        else kern = p.nks == 4 ? wgrad_tf_kernel<1, 3, 3, 1, 4, true> : wgrad_tf_kernel<1, 3, 3, 1, 2, true>;
    }
    if (!kern) return M1_ERR_UNSUPPORTED;
    if (m1_allow_dynamic_lds((const void*)kern, 160 * 1024) != M1_OK) return M1_ERR_LAUNCH;
    m1_note_kernel("wgrad_tf");
    m1_wg_note_plan("wgrad_tf", p.ntiles, want, nsplit, c, true, p.stages, grid.x, grid.y, grid.z);
    hipLaunchKernelGGL(kern, grid, dim3(256), smem, st, p);
    int rc = m1_check_launch(); if (rc) return rc;
    return m1_wg_fold_members(p.Rx, rx_mem, c.stride, (int)nsplit, g, c.rx_bias, nmem < 1 ? 1 : nmem, a_offs, st);
}
