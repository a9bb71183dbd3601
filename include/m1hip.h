/* m1hip.h -- C ABI of the MI355X-native M1 hot path (libm1hip.so, gfx950 only).
 *
 * The reference (DIAGNijmegen/prostateMR_3D-CAD-csPCa, tf2.5/) owns NO native code: every op below is,
 * in the reference, a call into a TensorFlow / TF-Addons / TF-Probability layer.  Each entry point
 * cites the reference call site(s) whose arithmetic it replaces, relative to
 * tf2.5/scripts/model/unets/  (N: = networks.py, B: = network_blocks.py).
 *
 * Conventions
 *   - plain pointers and sizes only; the caller (PyTorch, or any host) owns every buffer, including
 *     workspaces; no device allocation, no hidden synchronisation; every launch goes to the caller's
 *     hipStream_t (graph-capturable: no memset / memcpy nodes, zero fills are kernels).
 *   - process-global host state the library DOES keep (all of it behind mutexes, none of it device memory):
 *     the tuning-switch table (m1_config_*), the ONE queue of deferred weight-gradient folds and transposed-conv bias
 *     sums between m1_wgrad_defer(1) and m1_wgrad_fold_pending / _drop (the queued jobs point into caller-owned
 *     workspaces and, for the bias sums, into d(out); the caller keeps both alive until then), the test hook m1_set_force_direct, the opt-in profiler (m1_prof_*) and the opt-in
 *     kernel-choice log (m1_debug_kernels).  One thread drives the library at a time per process.
 *   - results are bit-reproducible run to run in the default configuration: every reduction across blocks goes
 *     through per-split partials folded in a fixed order.  Floating-point atomics remain compiled in behind
 *     switches only (M1_WG_DET=0, m1_set_force_direct: the generic fp32 reference kernels of conv_direct.hip).
 *   - activations are NDHWC, C-contiguous; `dtype` selects their storage type
 *     (M1_F32 / M1_BF16); parameters, statistics, reductions and gradients of parameters are fp32.
 *   - every function returns 0 on success or a negative m1_status.
 *   - `void* stream` is a hipStream_t.
 */
#ifndef M1HIP_H
#define M1HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum m1_dtype { M1_F32 = 0, M1_BF16 = 1 };

enum m1_status {
    M1_OK = 0,
    M1_ERR_BAD_ARG = -1,
    M1_ERR_UNSUPPORTED = -2,
    M1_ERR_LAUNCH = -3,
    M1_ERR_WORKSPACE = -4
};

#define M1_MAX_SRC 6

/* One member of a virtual channel-concat (tf.concat(axis=-1), N:596,604,606,613,615,621,623,653,677,
 * 701,725).  The concat is never materialised: kernels walk the list. */
typedef struct {
    const void* ptr; /* (N, D, H, W, C) */
    int C;
    int _pad;
} m1_src_t;

/* Geometry of one Conv3D(padding='same') or Conv3DTranspose(padding='same').
 * For Conv3D:           (D,H,W) = input extent,  output = ceil(in/s)       
 * For Conv3DTranspose:  (D,H,W) = input extent,  output = in*s              */
typedef struct {
    int N, D, H, W;
    int Cin, Cout;
    int kd, kh, kw;
    int sd, sh, sw;
    int dtype;
    int nsrc;                 /* number of concat members forming the Cin axis */
    m1_src_t src[M1_MAX_SRC]; /* sum of C == Cin */
} m1_conv_desc_t;

const char* m1_status_name(int status);
int m1_abi_version(void);

/* ---- Conv3D(padding='same') + bias : B:37,39,41,43,100-103 ; N:472,526,529-531,534-537 ; B:275 ----
 * w: Keras layout (kd,kh,kw,Cin,Cout) fp32; bias (Cout) fp32 or NULL; y: (N,OD,OH,OW,Cout). */
/* ws: caller-owned scratch of m1_conv_ws_bytes(d, transposed, role) bytes, 256-byte aligned (packed bf16/fp32
 * weight panels for the matrix-core kernels; bias-gradient partials for wgrad). role: 0 fwd, 1 dgrad, 2 wgrad. */
size_t m1_conv_ws_bytes(const m1_conv_desc_t* d, int transposed, int role);
/* Packed-panel refresh (no reference counterpart: the panels are this library's own copy of the Keras kernels,
 * train_model.py:231's optimizer step changes them once per step).  The first pack of a panel (ws_packed == 0) leaves
 * a job record in front of it inside ws; ws must therefore be ZERO-FILLED when it is first handed over.
 * m1_conv_pack_jobs writes the device addresses of the records of (d, transposed, role in {0,1}) into jobs_out
 * (room for M1_MAX_SRC entries) and returns their number; m1_pack_batch re-packs, in one launch, every filled record
 * of the device array jobs_dev[njobs] from the current weight values (records never filled are skipped).
 * block_prefix_dev (optional, device, njobs + 1 ints, prefix[0] = 0, prefix[njobs] = total_blocks): blocks of 256 threads per
 * job, sized by the caller in proportion to each job's weight count (>= 1 each); NULL = 48 blocks for every job. */
int m1_conv_pack_jobs(const m1_conv_desc_t* d, int transposed, int role, void* ws, void** jobs_out);
int m1_pack_batch(const void* const* jobs_dev, const int* block_prefix_dev, int njobs, int total_blocks, void* stream);
/* ws_packed != 0: ws still holds the weight panels a previous call with the SAME descriptor geometry, role and
 * (unchanged) weights left there -- the pack pass is skipped (the prior / posterior cores run twice per step). */
/* stats (optional, (N,Cout,2) fp32): {mean, rstd} (eps 1e-3, biased variance) of y per (n, channel) for the
 * InstanceNormalization that follows (B:54-60, N:575) -- accumulated from the stored (rounded) outputs in the
 * conv's own epilogue, so the statistics cost no extra pass over y. */
int m1_conv3d_fwd(const m1_conv_desc_t* d, const float* w, const float* bias, void* y, float* stats, void* ws,
                  int ws_packed, void* stream);
/* dx[i]: gradient buffer of concat member i (same shape/dtype as src[i]) or NULL to skip it.
 * accumulate (NULL = all 0): accumulate[i] != 0 -> dx[i] += instead of dx[i] = : a tensor read by several layers
 * (an SE block's input feeds conv1 and conv4, B:53,64; an encoder output also feeds its attention gate, N:584-590)
 * gets its gradient summed by the kernels' own epilogues, in call order, instead of by separate add passes. */
int m1_conv3d_dgrad(const m1_conv_desc_t* d, const float* w, const void* dy, void* const* dx, const int* accumulate,
                    void* ws, int ws_packed, void* stream);
/* 1 when both pair entry points below accept this shape (they return M1_ERR_UNSUPPORTED otherwise): ask before building a graph. */
int m1_conv3d_pair_supported(const m1_conv_desc_t* d, int C1);
/* Data gradient of a single-input Conv3D whose input is a = lrelu(IN(x)) -- conv2 / conv3 of an SEResNetBottleNeck (B:54-59): `da`
 * = d(a), and the kernel that writes it also emits the two sums the InstanceNorm backward needs (dbeta = sum dy,
 * dgamma = sum dy*xh, dy = da*lrelu'(gamma*xh+beta)) per tile into partial [N][*nparts][Cin][2] -- no separate reduction pass over
 * (x, da).  partial: N * partial_rows * Cin * 2 + N * Cin * 2 + 64 floats with partial_rows = m1_conv3d_dgrad_inbwd_rows(d) (a kernel
 * that would write more rows than the caller states leaves *nparts = 0).  *nparts = 0 on return: the kernel that took this shape has no such
 * epilogue; da is complete, finish with m1_instnorm_bwd; otherwise with m1_instnorm_bwd_partials. */
int m1_conv3d_dgrad_inbwd_rows(const m1_conv_desc_t* d);
int m1_conv3d_dgrad_inbwd(const m1_conv_desc_t* d, const float* w, const void* dy, void* da, const void* x, const float* stats,
                          const float* gamma, const float* beta, float slope, float* partial, int partial_rows, int* nparts,
                          void* ws, int ws_packed, void* stream);
/* conv1 || conv4 of an SEResNetBottleNeck as ONE problem (B:53 and B:64 apply Conv3D(F/4, k, s) and Conv3D(F, k, s) to the same
 * input): d->Cout = C1 + C4; w1 (kd,kh,kw,Cin,C1), w4 (kd,kh,kw,Cin,C4) stay separate Keras tensors.  Forward writes y1 (…,C1) and
 * y4 (…,C4) and, optionally, both (N,C,2) statistics tensors; the data gradient contracts over the virtual concat [dy1 | dy4].
 * ws: m1_conv_ws_bytes(d, 0, role) of the SAME descriptor (roles 0 / 1), same zero-fill and ws_packed contract as m1_conv3d_fwd /
 * m1_conv3d_dgrad.  M1_ERR_UNSUPPORTED (nothing launched): take the two single convs instead (channel counts that are not
 * multiples of one 16-byte segment, the halo-tile member-group regime, m1_set_force_direct). */
int m1_conv3d_pair_fwd(const m1_conv_desc_t* d, const float* w1, const float* b1, const float* w4, const float* b4, int C1,
                       void* y1, void* y4, float* stats1, float* stats4, void* ws, int ws_packed, void* stream);
int m1_conv3d_pair_dgrad(const m1_conv_desc_t* d, const float* w1, const float* w4, int C1, const void* dy1, const void* dy4,
                         void* const* dx, const int* accumulate, void* ws, int ws_packed, void* stream);
/* dw (kd,kh,kw,Cin,Cout) and db (Cout): accumulate == 0 -> overwritten (zeroed inside first);
 * accumulate != 0 -> added to what is there (the caller's flat gradient buffer, zeroed once per step: a weight
 * shared by several passes -- prior / posterior cores run twice per step -- sums without any extra copy). The
 * same flag has the same meaning on every other parameter-gradient output of this ABI. */
int m1_conv3d_wgrad(const m1_conv_desc_t* d, const void* dy, float* dw, float* db, void* ws, int accumulate,
                    void* stream);
/* test hook: 1 = route every conv through the generic direct kernels (no matrix cores). */
int m1_set_force_direct(int on);
/* Tuning switches ("M1_..." names): one table for the whole library.  A switch's value is its built-in default, or the
 * environment variable of the same name as the process started, or the last m1_config_set; m1_config_unset drops the override.
 * A change takes effect at the next launch that consults the switch (there are no per-call-site caches).  m1_config_get returns
 * M1_ERR_UNSUPPORTED for a switch nothing has consulted or set yet. */
int m1_config_set(const char* name, int value);
int m1_config_unset(const char* name);
int m1_config_get(const char* name, int* value);
/* debug probe (tools/dbg/stress_lds.py): `blocks` workgroups fill 31 KB of static LDS with a pattern and re-read it `spins` times; *bad
 * (device, unsigned) counts the words that changed.  Launched next to another kernel it shows whether that kernel writes LDS outside
 * its own allocation. */
int m1_debug_lds_canary(unsigned* bad, int blocks, int spins, void* stream);
/* debug probes (csrc/debug.hip; hip/ops.py M1_DEBUG_TRACE / M1_DEBUG_POISON=2; never launched unless a debug switch asks):
 * m1_debug_checksum: *slot (device) = a deterministic 64-bit checksum of the nbytes at p (4-byte aligned), ONE single-block kernel --
 * capturable into a hipGraph, so the outputs of every op of a replayed step can be compared between two processes.
 * m1_debug_scribble: `blocks` workgroups (0 = 512) that each take a whole CU (160 KB of LDS, four waves with 256 VGPRs + 256 AGPRs)
 * and leave the NaN pattern 0x7FC07FC0 in every LDS word and every vector register; `spins` ~microseconds each block stays resident
 * (so that all CUs are covered).  A kernel that reads LDS or a register it never wrote then yields NaN instead of a value that
 * depends on its predecessor on that CU. */
int m1_debug_checksum(const void* p, long long nbytes, unsigned long long* slot, void* stream);
/* Kernel-choice log: which kernel the dispatch put behind the conv-like launches since the log was last cleared, as a comma-separated
 * list ("conv_t3:bn160:ks2,wgrad_t3:kws16:big1,conv_mfma:128x128:w8:ks1", ...; valid until the next call).  mode 1 / 0: return the
 * log, clear it and switch logging on / off; mode < 0: return it only.  Off by default.  The op tests of the special kernels assert
 * on it: a shape the special kernel declines would otherwise compare the generic kernel with itself and stay green. */
const char* m1_debug_kernels(int mode);
/* Plan log: what stands behind the weight-gradient kernel names of the log above, as a ';'-separated list with the same `mode` argument
 * (off by default, nothing recorded while off, valid until the next call):
 *   wg:<kernel name> tiles=<K-tiles; voxels for wgrad_mfma> want=<splits asked of the copy planner> splits=<launched>
 *      fit=<copies the region holds> rx=<0|1: partial copies + fold> stages=<S or 0> grid=<x,y,z>      every weight-gradient launcher
 *   fold:<generic|vec|wide> copies=<n> n=<floats> nb=<bias floats> el=<EL> <queued|now>                 every fold of partial copies
 *   foldbatch:n=<jobs> blocks=<total>                                                                   every batched fold launch
 *   decline:<rung> rc=<code>      a rung of the weight-gradient ladder whose gate held returned M1_ERR_UNSUPPORTED / M1_ERR_WORKSPACE
 *   stem:cp=<4|8>                 the padded stem path ran */
const char* m1_debug_plans(int mode);
int m1_debug_scribble(int blocks, int spins, void* stream);

/* ---- Conv3DTranspose(padding='same') + bias : N:496-499,505-507,513-514,520,546-553 ----
 * w: Keras layout (kd,kh,kw,Cout,Cin) fp32; y: (N, D*sd, H*sh, W*sw, Cout). */
int m1_convT3d_fwd(const m1_conv_desc_t* d, const float* w, const float* bias, void* y, void* ws, int ws_packed,
                   void* stream);
int m1_convT3d_dgrad(const m1_conv_desc_t* d, const float* w, const void* dy, void* const* dx, const int* accumulate,
                     void* ws, int ws_packed, void* stream);
int m1_convT3d_wgrad(const m1_conv_desc_t* d, const void* dy, float* dw, float* db, void* ws, int accumulate,
                     void* stream);

/* ---- tfa.layers.InstanceNormalization (eps 1e-3) [+ LeakyReLU(slope)] : B:38,40,42,44,54-60,104,128;
 *      N:473,575-576.  x,y: (N,V,C).  stats: (N,C,2) fp32 = {mean, rstd}.
 *      ws: fp32 workspace of m1_reduce_ws_floats(N,V,C,nsums) floats. ---- */
size_t m1_reduce_ws_floats(int N, long long V, int C, int nsums);
int m1_instnorm_stats(const void* x, int N, long long V, int C, int dtype, float eps, float* stats, float* ws,
                      void* stream);
int m1_instnorm_apply(const void* x, const float* stats, const float* gamma, const float* beta, float slope,
                      void* y, int N, long long V, int C, int dtype, void* stream);
/* dy = grad wrt the (activated) output; writes dx (grad wrt raw x); dgamma, dbeta (C): see `accumulate`. */
int m1_instnorm_bwd(const void* x, const float* stats, const float* gamma, const float* beta, float slope,
                    const void* dy, void* dx, float* dgamma, float* dbeta, int N, long long V, int C, int dtype,
                    float* ws, int accumulate, void* stream);

/* the same from the partial sums of m1_conv3d_dgrad_inbwd: partial [N][nparts][C][2]; sums: (N,C,2) floats of scratch */
int m1_instnorm_bwd_partials(const void* x, const float* stats, const float* gamma, const float* beta, float slope,
                             const void* dy, void* dx, float* dgamma, float* dbeta, int N, long long V, int C, int dtype,
                             const float* partial, int nparts, float* sums, int accumulate, void* stream);

/* ---- SE gate + multiplicative residual combine : B:68-78 ----
 * gate: g = sigmoid(W7 . lrelu(W6 . beta3 + b6) + b7)  (GAP(IN3(.)) == beta3 exactly).
 * W6: (F,Fr) W7: (Fr,F) Keras (1,1,1,Cin,Cout) layout.  hidden: (Fr) pre-activation, saved for bwd. */
int m1_se_gate_fwd(const float* beta3, const float* W6, const float* b6, const float* W7, const float* b7,
                   int F, int Fr, float* hidden, float* g, void* stream);
/* dg: the F + Fr float scratch written by m1_se_combine_bwd (contents are consumed and overwritten). */
int m1_se_gate_bwd(const float* beta3, const float* W6, const float* W7, const float* hidden, const float* g,
                   const float* dg, int F, int Fr, float* dbeta3_add, float* dW6, float* db6, float* dW7,
                   float* db7, int accumulate, void* stream);
#define M1_SE_GATE_BATCH 16
/* All gates of a core pass in one launch (they depend on parameters only): same arguments as m1_se_gate_fwd per job. */
typedef struct {
    const float* beta3; const float* W6; const float* b6; const float* W7; const float* b7;
    float* hidden; float* g;
    int F, Fr;
} m1_se_gate_fwd_job_t;
int m1_se_gate_fwd_batch(const m1_se_gate_fwd_job_t* jobs /* host array */, int njobs, void* stream);
/* The gate backward yields parameter gradients only (nothing on the data-gradient chain waits for it): a caller may
 * collect the jobs of a whole backward pass and run them in two launches.  Same arguments as m1_se_gate_bwd.  Jobs
 * that name the same destination buffers (one SE block evaluated by several passes of the cores) must have
 * accumulate = 1; they are applied one after the other in array order, so the sums are run-to-run identical. */
typedef struct {
    const float* beta3; const float* W6; const float* W7; const float* hidden; const float* g;
    float* dg;                 /* the F + Fr scratch of m1_se_combine_bwd (must stay alive until the batch has run) */
    float* dbeta3_add; float* dW6; float* db6; float* dW7; float* db7;
    int F, Fr, accumulate, _pad;
} m1_se_gate_job_t;
int m1_se_gate_bwd_batch(const m1_se_gate_job_t* jobs /* host array */, int njobs, void* stream);
/* out = dropout( lrelu( IN3(y3) * g * IN4(y4) ) ); y3,y4 raw conv outputs (N,V,F); stats3/4 (N,F,2).
 * Dropout state is DEVICE resident so a captured graph can be replayed: rng[0] = seed, rng[1] = step
 * counter (advanced by m1_step_advance); layer_id separates the streams of different layers. The mask is
 * a pure function of (rng, layer_id, element index): backward can regenerate it.  keep_mask (optional, bf16 and
 * F % 8 == 0 only, N*V*F/8 bytes): the forward also stores the keep bits (bit idx & 7 of byte idx >> 3) and a backward
 * given the same buffer reads them instead of re-running Philox (the backward passes are instruction bound:
 * 10 Philox rounds per 4 elements were ~45 % of their instructions).
 * stats4 == gamma4 == beta4 == NULL: the identity residual of B:63 (C_in == filters: no conv4 / norm4) -- y4 is then the block's
 * INPUT tensor (N,V,F) and out = dropout( lrelu( IN3(y3) * g * y4 ) ). */
int m1_se_combine_fwd(const void* y3, const void* y4, const float* stats3, const float* stats4,
                      const float* gamma3, const float* beta3, const float* gamma4, const float* beta4,
                      const float* g, void* out, int N, long long V, int F, int dtype, float drop_rate,
                      const uint64_t* rng, uint64_t layer_id, unsigned char* keep_mask, void* stream);
/* writes dy3, dy4 (grads wrt the RAW conv outputs, i.e. through both InstanceNorms); dgamma3,dbeta3,dgamma4,
 * dbeta4 (F each) per `accumulate`; dg is scratch for m1_se_gate_bwd, F + Fr floats, first F always overwritten.
 * ws: m1_reduce_ws_floats(N,V,F,5).  Identity residual (stats4 == gamma4 == beta4 == NULL): dy4 is the gradient wrt the block input
 * through the residual factor (no normalisation to go back through), dgamma4 / dbeta4 are not touched (may be NULL). */
int m1_se_combine_bwd(const void* y3, const void* y4, const float* stats3, const float* stats4,
                      const float* gamma3, const float* beta3, const float* gamma4, const float* beta4,
                      const float* g, const void* dout, void* dy3, void* dy4, float* dgamma3, float* dbeta3,
                      float* dgamma4, float* dbeta4, float* dg, int N, long long V, int F, int dtype,
                      float drop_rate, const uint64_t* rng, uint64_t layer_id, const unsigned char* keep_mask,
                      float* ws, int accumulate, void* stream);

/* The same for TWO stacked passes of a core that share everything in front of their first dropout draw (round 6).  A training step
 * evaluates each core twice on the same input (N:348-349 posterior, N:351-352 prior; here stacked along the batch axis): with
 * Monte-Carlo dropout the two passes differ from the first SE block's dropout on (N:579-582) -- the stem and that block's convolutions
 * and norms are the same computation twice.  y3 / y4 / stats3 / stats4 hold N samples; out (and keep_mask) hold 2N: output sample n
 * reads input sample n % N and draws its own keep mask (the dropout stream is indexed by the OUTPUT element, exactly as if the inputs
 * had been duplicated).  Backward: dout holds 2N samples; dy3 / dy4 (N samples) and the parameter sums take the SUM of the two halves'
 * gradients (lrelu' and both factors are common to the halves).  Not for the identity residual. */
int m1_se_combine_dup_fwd(const void* y3, const void* y4, const float* stats3, const float* stats4,
                          const float* gamma3, const float* beta3, const float* gamma4, const float* beta4,
                          const float* g, void* out, int N, long long V, int F, int dtype, float drop_rate,
                          const uint64_t* rng, uint64_t layer_id, unsigned char* keep_mask, void* stream);
int m1_se_combine_dup_bwd(const void* y3, const void* y4, const float* stats3, const float* stats4,
                          const float* gamma3, const float* beta3, const float* gamma4, const float* beta4,
                          const float* g, const void* dout, void* dy3, void* dy4, float* dgamma3, float* dbeta3,
                          float* dgamma4, float* dbeta4, float* dg, int N, long long V, int F, int dtype,
                          float drop_rate, const uint64_t* rng, uint64_t layer_id, const unsigned char* keep_mask,
                          float* ws, int accumulate, void* stream);

/* ---- grid attention gate pieces : B:113-124 ----
 * theta: (N, Dt,Ht,Wt, C) ; phi: (N, Dp,Hp,Wp, C) nearest-upsampled by (Dt/Dp,...) ;
 * sigma[n,v] = sigmoid( sum_c lrelu(theta+phi_up)[c]*wpsi[c] + bpsi ) : (N,Dt,Ht,Wt) stored as dtype */
int m1_gate_sigma_fwd(const void* theta, const void* phi, const float* wpsi, const float* bpsi, void* sigma,
                      int N, int Dt, int Ht, int Wt, int Dp, int Hp, int Wp, int C, int dtype, void* stream);
/* dtheta (like theta) is written; dphi (like phi) = window-sum of dtheta; dwpsi (C), dbpsi (1) overwritten.
 * ws: m1_reduce_ws_floats(N, Dt*Ht*Wt, C, 2) floats */
int m1_gate_sigma_bwd(const void* theta, const void* phi, const float* wpsi, const void* sigma,
                      const void* dsigma, void* dtheta, void* dphi, float* dwpsi, float* dbpsi, int N, int Dt,
                      int Ht, int Wt, int Dp, int Hp, int Wp, int C, int dtype, float* ws, int accumulate,
                      void* stream);
/* y = sigma_up * x : x (N,D,H,W,C), sigma (N,D/ss0,H/ss1,W/ss2) */
int m1_mul_sigma_fwd(const void* x, const void* sigma, void* y, int N, int D, int H, int W, int C, int s0,
                     int s1, int s2, int dtype, void* stream);
/* Both of the above as ONE launch (B:113-124): sigma (N,Dt,Ht,Wt) is written AND y = sigma_up * x with the stored (rounded) sigma;
 * x, y (N,D,H,W,Cx), Ci = channels of theta / phi, (Dt,Ht,Wt) = (D/s0, H/s1, W/s2).  M1_ERR_UNSUPPORTED (nothing launched) for channel
 * counts that are no multiple of a 16-byte vector or a mismatching sigma grid: take the two calls. */
int m1_gate_sigma_mul_fwd(const void* theta, const void* phi, const float* wpsi, const float* bpsi, void* sigma, const void* x,
                          void* y, int N, int Dt, int Ht, int Wt, int Dp, int Hp, int Wp, int Ci, int D, int H, int W, int Cx,
                          int s0, int s1, int s2, int dtype, void* stream);
/* accumulate_dx != 0: dx += sigma_up * dy (x also feeds other layers, see m1_conv3d_dgrad); dsigma is always overwritten */
int m1_mul_sigma_bwd(const void* x, const void* sigma, const void* dy, void* dx, void* dsigma, int N, int D,
                     int H, int W, int C, int s0, int s1, int s2, int dtype, int accumulate_dx, void* stream);

/* ---- latent head : N:640-647 (x4 levels) and KL N:373-385 ----
 * ml: (N,V,2L) = [mu | logsigma]; z = mu + exp(clip(logsigma,+-0.1))*eps  (mode 0) or mu (mode 1);
 * mode 2: N even, two passes stacked along the batch axis -- samples [0, N/2) as mode 0 with eps of N/2 samples (N:348),
 * samples [N/2, N) as mode 1 (N:349). */
int m1_latent_sample_fwd(const void* ml, const void* eps, void* z, int N, long long V, int L, int mode,
                         int dtype, void* stream);
int m1_latent_sample_bwd(const void* ml, const void* eps, const void* dz, void* dml, int N, long long V, int L,
                         int mode, int dtype, void* stream);
/* The same with the N(0,1) draws made INSIDE the kernel (no draw tensor, no generator launch in the step): element i of the sampling
 * pass takes Box-Muller of Philox4x32-10(seed = rng[0] + stream_id * golden, counter = (rng[1] << 36) + i), rng = the device-resident
 * {seed, step} pair of the dropout stream (m1_step_advance moves it).  The backward regenerates the same draws from the same state:
 * call it before the step counter advances.  stream_id: distinct per latent head. */
int m1_latent_sample_rng_fwd(const void* ml, const uint64_t* rng, uint64_t stream_id, void* z, int N, long long V, int L, int mode,
                             int dtype, void* stream);
int m1_latent_sample_rng_bwd(const void* ml, const uint64_t* rng, uint64_t stream_id, const void* dz, void* dml, int N, long long V,
                             int L, int mode, int dtype, void* stream);
/* kl[0] = mean_n sum_v KL(q||p) (fp32, overwritten). */
int m1_kl_fwd(const void* ml_q, const void* ml_p, float* kl, int N, long long V, int L, int dtype, void* stream);
/* dml_q, dml_p = dkl[0] * dKL/d(ml_*)  */
int m1_kl_bwd(const void* ml_q, const void* ml_p, const float* dkl, void* dml_q, void* dml_p, int N,
              long long V, int L, int dtype, void* stream);
/* the same when the KL term reads only the first N of Nall samples of ml_q / ml_p (the sampling half of two stacked passes, N:348,351):
 * dml_q / dml_p are (Nall, V, 2L); the gradient of the samples >= N is written as zeros by the kernel */
int m1_kl_bwd_first(const void* ml_q, const void* ml_p, const float* dkl, void* dml_q, void* dml_p, int N, long long V,
                    int L, int Nall, int dtype, void* stream);

/* ---- output heads : softmax(logits) (N:754, N:388-390) with deep-supervision heads upsampled by
 *      nearest repeat (N:739-741,751).  logits_h: (N, D/u0, H/u1, W/u2, nc) per head;
 *      probs: (N,D,H,W,nheads*nc) fp32. ---- */
typedef struct {
    const void* logits;
    void* dlogits;
    int u0, u1, u2;
    int _pad;
} m1_head_t;
int m1_softmax_heads_fwd(const m1_head_t* heads, int nheads, float* probs, int N, int D, int H, int W, int nc,
                         int dtype, void* stream);
int m1_softmax_heads_bwd(const m1_head_t* heads, int nheads, const float* probs, const float* dprobs, int N,
                         int D, int H, int W, int nc, int dtype, void* stream);

/* ---- Monte-Carlo inference : train_model.py:72 (--UNET_PROBA_ITER), scipy.stats.entropy ----
 * The mean and the predictive entropy of n softmax draws without a per-draw probability tensor (csrc/mc.hip).
 * m1_mc_accum: logits (R*B, V, nc) bf16 / fp32 = the raw head output of ONE forward pass over R replicas of the caller's B samples,
 * replica-major (sample r*B + b is replica r of sample b).  Per (b, v) and replica: the max-subtracted fp32 softmax over nc in the
 * operation order of m1_softmax_heads_fwd (one draw equals that kernel's output bit for bit); the R vectors are summed in replica
 * order; accumulate == 0: sum_p (B, V, nc) fp32 = that sum (this is how the accumulator is initialised: no zero fill exists or is
 * needed), accumulate != 0: sum_p += that sum.  samples_out (optional, (R*B, V, nc) fp32): the per-draw probabilities.
 * nc in 2..4 (M1_ERR_UNSUPPORTED otherwise).  Pointers must be aligned to their element type; 16-byte accesses are used when every
 * pointer is 16-byte aligned and (R == 1 or B*V*nc elements of logits are a multiple of 16 bytes), element accesses otherwise.
 * m1_mc_finish: mean (B, V, nc) = sum_p / n_draws (IEEE division: n_draws == 1 returns the draw unchanged; mean may alias sum_p);
 * entropy (B, V) = -sum_c mean_c * ln(mean_c) in nats, a term with mean_c == 0 contributing exactly 0.
 * No atomics, no memset / memcpy nodes; results are bit-identical run to run. */
int m1_mc_accum(const void* logits, int R, int B, long long V, int nc, int dtype, float* sum_p, int accumulate, float* samples_out,
                void* stream);
int m1_mc_finish(const float* sum_p, int n_draws, int B, long long V, int nc, float* mean, float* entropy, void* stream);

/* ---- Uncertainty maps of the same draws (csrc/mc.hip): total entropy split into what the draws disagree on and what they agree on ----
 * Per voxel, N draws p_1..p_N, nats:  expected_entropy = (1/N) sum_r H(p_r), H(p) = -sum_c p_c ln p_c (aleatoric);
 * mutual_info = entropy - expected_entropy (epistemic, BALD);  variance_c = (1/N) sum_r p_r,c^2 - mean_c^2 (population variance).
 * m1_mc_accum_u: m1_mc_accum's pass with two more fp32 accumulators, sum_h (B, V) (+)= sum_r H(p_r) and sum_pp (B, V, nc) (+)=
 * sum_r p_r^2, from the probabilities already in registers (no second read of the logits, no LDS, no atomics).  All three sums
 * associate alike: the R replicas of a pass in replica order, then old + that.  accumulate == 0 writes all three (no zero fill).
 * sum_p and samples_out are m1_mc_accum's, bit for bit.  16-byte accesses need every pointer 16-byte aligned (and the replica
 * stride, as above); element accesses otherwise, with the same bits.
 * m1_mc_finish_u: mean and entropy as m1_mc_finish (bit for bit for every input without a NaN); expected_entropy (B, V) = sum_h /
 * n_draws; mutual_info (B, V) and variance (B, V, nc) as defined, values below 0 (rounding) written as +0.  mean may alias sum_p,
 * expected_entropy sum_h and variance sum_pp: a thread reads its own elements before it writes them.  n_draws == 1 gives
 * expected_entropy == entropy bit for bit and mutual_info == variance == +0 (p*p and mean*mean are rounded products, never fused).
 * NaN: a voxel whose softmax is NaN in any draw (a NaN or infinite logit) has NaN in all five maps (the clamp is x < 0 ? 0 : x, and the entropies take every term
 * that is not <= 0); m1_mc_finish, whose terms are those > 0, writes entropy 0 for such a voxel.  No other voxel is affected.
 * Arguments are checked as for m1_mc_accum / m1_mc_finish. */
int m1_mc_accum_u(const void* logits, int R, int B, long long V, int nc, int dtype, float* sum_p, float* sum_h, float* sum_pp,
                  int accumulate, float* samples_out, void* stream);
int m1_mc_finish_u(const float* sum_p, const float* sum_h, const float* sum_pp, int n_draws, int B, long long V, int nc, float* mean,
                   float* entropy, float* expected_entropy, float* mutual_info, float* variance, void* stream);

/* ---- Test-time augmentation by mirroring (csrc/mc.hip): a mirrored view is one more draw, un-mirrored while it is summed ----
 * A view is a 3-bit mask: bit 0 mirrors W, bit 1 mirrors H, bit 2 mirrors D.  The masks of the R <= 16 replicas of a pass travel by
 * value in `flips`, replica r in bits [3r, 3r + 3): no device table, no memcpy node, so the calls can be captured.
 * m1_mc_accum_v: logits (R*B, D, H, W, nc) bf16 / fp32, replica-major; the accumulators as for m1_mc_accum[_u] with V = D*H*W.  Output
 * voxel (b, d, h, w) takes replica r's voxel (b, d', h', w'), x' = extent - 1 - x where the bit of x is set in mask r.  sum_h ==
 * sum_pp == NULL: m1_mc_accum; both given: m1_mc_accum_u; exactly one: M1_ERR_BAD_ARG.  samples_out (R, B, D, H, W, nc) receives the
 * UN-mirrored per-draw probabilities.  The result equals m1_mc_accum[_u] on logits un-mirrored beforehand, bit for bit, in every
 * accumulator and in the samples; with flips == 0 it equals that entry point on the same arguments.  16-byte accesses need W to be
 * a multiple of the group (4 voxels fp32, 8 bf16) besides the alignment m1_mc_accum asks for; element accesses otherwise, same bits.
 * R > 16: M1_ERR_UNSUPPORTED; a bit of flips at or above 3R: M1_ERR_BAD_ARG; everything else as m1_mc_accum.
 * m1_tta_views: out (R*B, D, H, W, C), replica r = x (B, D, H, W, C) mirrored by mask r; a copy, bf16 / fp32, any C >= 1. */
int m1_mc_accum_v(const void* logits, int R, int B, int D, int H, int W, int nc, int dtype, unsigned long long flips, float* sum_p,
                  float* sum_h, float* sum_pp, int accumulate, float* samples_out, void* stream);
int m1_tta_views(const void* x, int B, int D, int H, int W, int C, int dtype, int R, unsigned long long flips, void* out, void* stream);

/* ---- Sliding-window inference (csrc/tile.hip; unets.networks.predict_tiled is the public surface, tiling.py the host side) ----
 * A volume (B, vol[0], vol[1], vol[2], C) larger than the network's grid is cut into T = n[0] * n[1] * n[2] overlapping tiles of the
 * network's size, tile t = (i0 * n[1] + i1) * n[2] + i2 at (origin[0][i0], origin[1][i1], origin[2][i2]).  The geometry travels by
 * value into the kernels: no device table, no memcpy node, so the calls can be captured.  Per axis a: origin[a][0 .. n[a]) strictly
 * ascending, 0 <= origin and origin + tile[a] <= vol[a] (a tile never leaves the volume: there is no padding here), and the tiles
 * together cover [0, vol[a]): origin[a][0] == 0, no gap between neighbours, the last tile ends at vol[a].
 * m1_tile_gather: x (B, vol..., C) fp32 / bf16, any C >= 1 -> out (T*B, tile..., C) of the same type, tile-major: sample t * B + b is
 * tile t of batch entry b.  A copy, one launch.  16-byte accesses when both pointers are 16-byte aligned and vol[2], tile[2] and
 * every origin[2][] are multiples of m = 16 / gcd(16, C * element size) voxels; element accesses otherwise, same bits.
 * m1_tile_blend: tiles (T*B, tile..., C) fp32 in that order (the MC accumulators, or any per-voxel map; C = 1 for sum_h), profile =
 * the device rows w0[tile[0]], w1[tile[1]], w2[tile[2]] one after the other, fp32, all > 0 (the caller's promise: the kernel cannot
 * refuse them before it runs) -> out (B, vol..., C) fp32.  One lane owns output voxels and reads every tile that covers them: no
 * atomics, no workspace, no zero fill, no memset node; one launch; bit-identical from run to run and for every grid.  Per voxel, the
 * covering tiles i in ascending t: w_i = (w0 * w1) * w2 at the voxel's position inside tile i, W = sum_i w_i, out_c = sum_i
 * (w_i / W) * v_i,c, each sum in that order starting from its first term, every operation a separate fp32 rounding, IEEE division.
 * A voxel that one tile covers receives that tile's value bit for bit.  16-byte accesses when C <= 4, both tensors are 16-byte
 * aligned and vol[2], tile[2] and every origin[2][] are multiples of G = 4, 2, 4, 1 voxels for C = 1, 2, 3, 4; element accesses
 * otherwise, same bits.
 * NULL pointers, B, C or an extent < 1, n[a] outside 1..M1_TILE_MAX_AXIS, origins that break the rules above, a pointer not aligned
 * to its element: M1_ERR_BAD_ARG.  A dtype outside the enum, T * B * tile voxels * C or B * vol voxels * C >= 2^31:
 * M1_ERR_UNSUPPORTED.  Both before any launch. */
#define M1_TILE_MAX_AXIS 16
typedef struct { int vol[3]; int tile[3]; int n[3]; int origin[3][M1_TILE_MAX_AXIS]; } m1_tile_t;
int m1_tile_gather(const void* x, int B, int C, int dtype, const m1_tile_t* g, void* out, void* stream);
int m1_tile_blend(const float* tiles, int B, int C, const m1_tile_t* g, const float* profile, float* out, void* stream);

/* ---- Focal loss on the softmax heads : losses.py:32-49 (FL: renormalise, clip [1e-7, 1-1e-7], -y log p, * y (1-p)^gamma,
 * * alpha, sum over D,H,W,C, mean over the batch; loss(): mean over the y_pred.shape[-1] / nc heads) ----
 * probs (N,V,nheads*nc) fp32 as written by m1_softmax_heads_fwd; y_true (N,V,nc) fp32 or bf16; alpha: nc HOST floats.
 * fwd: ws of m1_focal_ws_floats floats (per-block partials, folded in a fixed order); loss: 1 device float.
 * bwd: dprobs = dloss[0] * dLoss/dprobs (dloss: 1 device float, e.g. autograd's incoming gradient). */
size_t m1_focal_ws_floats(int N, long long V, int nheads);
int m1_focal_fwd(const float* probs, const void* y_true, int y_dtype, const float* alpha, float gamma, int N, long long V,
                 int nheads, int nc, float* ws, float* loss, void* stream);
int m1_focal_bwd(const float* probs, const void* y_true, int y_dtype, const float* alpha, float gamma, int N, long long V,
                 int nheads, int nc, const float* dloss, float* dprobs, void* stream);

/* ---- Soft Dice + Boundary (surface) loss on the softmax heads : losses.py:66-130 (SoftDicePlusBoundarySurface) ----
 * Distance map (calc_dist_map, L:83-92): y_true (N,D,H,W,nc) fp32 or bf16 one-hot, nc >= 2; for each sample and class c >= 1,
 * pos = (y_true[...,c] != 0): phi = edt(~pos) on ~pos, 1 - edt(pos) on pos (exact Euclidean distance, unit spacing); phi = 0 for
 * a class with no foreground voxel in the sample (L:90) and for one with no background voxel (where scipy is degenerate).
 * out: phi (N,D,H,W,nc-1) fp32.  ws: m1_dist_map_ws_bytes bytes.  D, H, W <= 256, nc <= 8 (M1_ERR_UNSUPPORTED otherwise).
 * Loss (DB + loss, L:94-130): probs (NV, nheads*nc) fp32 as written by m1_softmax_heads_fwd, y_true (NV,nc), phi (NV,nc-1);
 *   per head: q = clip(p / sum p, 1e-7, 1-1e-7), I = sum y q, Dn = sum (y + q), B = sum q phi over every voxel and class >= 1
 *   of the whole batch; loss = mean_h [w0 (1 - 2 I / (Dn + smooth)) + w1 B].
 * fwd: ws of m1_dice_bd_ws_floats floats, 8-byte aligned (fp64 per-block partials folded in a fixed order; I and Dn stay there
 * for the backward); loss: 1 device float.  bwd: the same ws after fwd; dprobs = dloss[0] * dLoss/dprobs. */
size_t m1_dist_map_ws_bytes(int N, int D, int H, int W, int nc);
int m1_dist_map(const void* y_true, int y_dtype, int N, int D, int H, int W, int nc, void* ws, float* out, void* stream);
size_t m1_dice_bd_ws_floats(long long NV, int nheads);
int m1_dice_bd_fwd(const float* probs, const void* y_true, int y_dtype, const float* phi, long long NV, int nheads, int nc,
                   float w0, float w1, float smooth, float* ws, float* loss, void* stream);
int m1_dice_bd_bwd(const float* probs, const void* y_true, int y_dtype, const float* phi, long long NV, int nheads, int nc,
                   float w0, float w1, float smooth, const float* ws, const float* dloss, float* dprobs, void* stream);

/* ---- Train-time augmentations : tf2.5/scripts/model/augmentations.py (A:) 36-326, augment_tensors and its helpers ----
 * x (N,D,H,W,C) fp32 image whose first nimg channels are MRI sequences (3 lesion / 1 zonal; the rest are the label channels of a
 * probabilistic input), y (N,D,H,W,nc) fp32 label or NULL.  Every op is 2-D over (H,W) with one set of parameters per sample.
 * Everything random reaches the resampling / intensity kernels through ONE plain-data record per sample, m1_aug_params_t: filled
 * on the device by m1_aug_draw, or by the caller (tests inject tables).  The kernels never call cos / sin: the six coefficients of
 * the rotation's projective transform (tfa.image.rotate: [cos, -sin, x_off, sin, cos, y_off], output -> input, about the centre of
 * the SYMMETRIC-padded slice) are table entries.  Sampling coordinates are fp32 in a fixed operation order without contraction:
 * (i + 0.5f) * ((float)in / (float)out) - 0.5f for tf.image.resize (TF2 half-pixel centres, no antialias),
 * floor((i + 0.5f) * ((float)in / (float)out)) for the TF2 nearest resize, (t0 * x + t1 * y) + t2 for the rotation.
 * `stages`: the M1_AUG_* bits of the stages the hyper-parameters enable (a table bit outside it is ignored); M1_AUG_ZOOM,
 * M1_AUG_ROTATE or M1_AUG_POOR on a non-square slice -> M1_ERR_UNSUPPORTED (A:60-61,143-148 and A:267-268 use shape[1] for both
 * axes; A:233-234 crops both axes by the fraction of the first).  dtype: M1_F32 only (M1_BF16 -> M1_ERR_UNSUPPORTED, anything else
 * M1_ERR_BAD_ARG).  C, nc <= 8, nimg <= min(C, 4).  Out-of-range table entries cannot fault: every source index is clamped.
 * Results are bit-identical run to run (fp64 per-block partials folded in a fixed order, no atomics); every launch goes to
 * `stream`, nothing synchronises, nothing is a memset / memcpy node. */
enum m1_aug_stage {
    M1_AUG_MASTER = 1, M1_AUG_ZOOM = 2, M1_AUG_FLIP = 4, M1_AUG_ROTATE = 8, M1_AUG_TRANSLATE = 16, M1_AUG_CSHIFT = 32,
    M1_AUG_GAMMA = 64, M1_AUG_POOR = 128, M1_AUG_NOISE = 256
};
typedef struct {
    uint32_t fired;        /* M1_AUG_* bits: the master coin (A:51) and the stage coins (A:59,66,71,77,88,98,104,109) that came up */
    uint32_t gamma_ch;     /* bit c: the per-channel coin of A:299 for image channel c */
    uint32_t poor_ch;      /* bit c: the per-channel coin of A:265 */
    int32_t scale;         /* A:60-61: side of the resized slice, in [H, ceil(H * zoom_factor)) */
    int32_t rot_pad;       /* A:223: ceil((diagonal - min(H, W)) / 2), also the start of the central crop (A:233-234) */
    float rot[6];          /* t0..t5: source x = (t0 * X + t1 * Y) + t2, source y = (t3 * X + t4 * Y) + t5, in the padded slice */
    int32_t tr[4];         /* A:78-81: pad_top, pad_bottom, pad_right, pad_left */
    int32_t cs[4];         /* A:89-92: the same for the channel shift */
    int32_t cs_channel;    /* A:189 */
    float gamma;           /* A:99 */
    float noise_std;       /* A:110 */
    float angle_deg;       /* A:72, informational: the kernels read rot[] */
    int32_t _pad;
} m1_aug_params_t;
/* One thread per sample fills table[n] in the draw order of A:51-111 (a stage that is disabled, or whose coin the master coin
 * precedes and did not fire, draws nothing).  Draw k of sample n: Philox4x32-10(seed = rng[0] + stream_id * golden,
 * counter = (rng[1] << 36) + n * 64 + k), rng = a device-resident {seed, step} pair (m1_step_advance moves it).  Uniform floats
 * are (word >> 9) * 2^-23 (23 bits, as TensorFlow's: lo + u * (hi - lo) then stays below hi), integers in [lo, hi) are
 * lo + word % (hi - lo).  Hyper-parameters as in A:39-48, as doubles (what Python hands to TF: the integer bounds are
 * ceil((float)(H * factor)), A:61,78-81,89-92); lesion != 0 for train_obj == 'lesion'.  An empty or oversized integer interval
 * (ceil(H * zoom_factor) <= H, a pad bound < 1 or > H) is M1_ERR_BAD_ARG; zoom, rotation or poor scan enabled on a non-square
 * slice M1_ERR_UNSUPPORTED. */
int m1_aug_draw(m1_aug_params_t* table, int N, const uint64_t* rng, uint64_t stream_id, double prob, double tx_prob,
                double translate_factor, double rotation_degree, int axial_hflip, double zoom_factor, double gauss_noise_stddev,
                double chan_shift_factor, int sim_poor_scan, double gamma_lo, double gamma_hi, int H, int W, int nimg, int lesion,
                void* stream);
/* ws of every call below: m1_aug_ws_bytes bytes, 8-byte aligned, the same buffer through the three calls of one batch. */
size_t m1_aug_ws_bytes(int N, int D, int H, int W, int nimg);
/* zoom -> flip -> rotate -> translate -> channel shift of x into gx and zoom -> flip -> rotate -> translate of y into gy (same
 * coins and parameters, A:114-120), ONE gather launch evaluated from the output voxel back to the source (at most 16 source reads
 * per element; the stages' fp32 results are formed one after the other exactly as if each stage had been materialised).  A sample
 * whose master coin did not fire is copied.  With M1_AUG_GAMMA in `stages` the launch also leaves min / max / sum / sum of squares
 * of every image channel of gx in ws (per-block fp64 partials + one fold launch). */
int m1_aug_geom(const float* x, const float* y, const m1_aug_params_t* table, float* gx, float* gy, int N, int D, int H, int W,
                int C, int nimg, int nc, int stages, int dtype, void* ws, void* stream);
/* A:306-307: mean and population std of the gamma-powered channels of gx (after m1_aug_geom with M1_AUG_GAMMA). */
int m1_aug_gamma_stats(const float* gx, const m1_aug_params_t* table, int N, int D, int H, int W, int C, int nimg, int stages,
                       int dtype, void* ws, void* stream);
/* gamma curve + re-standardisation (A:298-310), poor scan (A:264-271: the nearest pick of a bilinear tap of the gamma-corrected
 * volume, four reads) and additive noise (A:314-326) in one pass, one write of `out`.  Noise of voxel v: Box-Muller of
 * Philox4x32-10(seed = rng[0] + stream_id * golden, counter = (rng[1] << 36) + v), up to four draws per voxel, one per image
 * channel; rng may be NULL when M1_AUG_NOISE is not in `stages`.  N*D*H*W >= 2^36 voxels: M1_ERR_UNSUPPORTED (the step sits above
 * bit 36 of the counter). */
int m1_aug_intensity(const float* gx, const m1_aug_params_t* table, const uint64_t* rng, uint64_t stream_id, float* out, int N,
                     int D, int H, int W, int C, int nimg, int stages, int dtype, void* ws, void* stream);

/* ---- label preparation of the data generator : data_generators.py:51-72,92-97 (labels.hip) ----
 * contour_smoothening as an integer rule (DESIGN.md "label feed"; restated from OpenCV's 8-bit bit-exact Gaussian, not pinned against
 * cv2): per H x W slice S(y,x) = sum_dy sum_dx taps[dy+3] * taps[dx+3] * m(r(y+dy,H), r(x+dx,W)), r = reflect-101 repeated until the
 * index is in range (0 when the extent is 1), out = (S + 32768) >> 16.  taps: 7 HOST integers >= 0 that sum to 256
 * (data_generators.gaussian_taps_u8(7, 4.0) = 31 36 40 42 40 36 31), else M1_ERR_BAD_ARG.
 * m1_contour_smooth_u8: in / out / scratch hold planes * H * W bytes; `iterations` repeats the pass (scratch is needed, and may be
 * NULL otherwise, for iterations > 1); the three buffers are distinct. */
int m1_contour_smooth_u8(const uint8_t* in, uint8_t* out, uint8_t* scratch, long long planes, int H, int W, const int* taps,
                         int iterations, void* stream);
enum m1_label_objective { M1_LABEL_LESION = 0, M1_LABEL_ZONAL = 1 };
enum m1_feed_mode { M1_FEED_TRAIN = 0, M1_FEED_VALID = 1, M1_FEED_TEST = 2 };
/* The generator's sample from the raw arrays, one launch, no memset / memcpy nodes.  ann (B,D,H,W) uint8: the raw annotation (grades
 * for M1_LABEL_LESION: >= 2 -> 1; zones for M1_LABEL_ZONAL: == 1 -> TZ, == 2 -> PZ, each binarised on its own), ignored and
 * allowed to be NULL for M1_FEED_TEST (all background).  Every class mask is smoothed (one iteration), then
 *   detection (B,D,H,W,nc) fp32 = {1 - sum of the foreground masks in 8-bit arithmetic (mod 256), masks...}, nc = 2 / 3;
 *   kl        (B,D,H,W,nc) fp32 = 0, required when probabilistic != 0 and NULL otherwise;
 *   x_out     (B,D,H,W,keep [+ nc - 1]) fp32 = the first `keep` channels of image (B,D,H,W,C) -- keep = C for lesion (at most 4),
 *             1 for zonal -- followed, when probabilistic, by detection[..., 1:] for M1_FEED_TRAIN and zeros otherwise.
 * An objective or mode outside the enums, or more kept channels than 4: M1_ERR_UNSUPPORTED. */
int m1_label_prepare(const uint8_t* ann, const float* image, float* x_out, float* detection, float* kl, int B, int D, int H, int W,
                     int C, int objective, int mode, int probabilistic, const int* taps, void* stream);

/* ---- scan preprocessing : tf2.5/scripts/preprocess.py (P:) 29-39 whitening, 42-49 center_crop, 74-98 resize_image_with_crop_or_pad
 *      (csrc/preprocess.hip; resample_img, P:52-71, is the next section: a restatement pinned against scipy, not against ITK) ----
 * Every entry point reads a raw source (B, d, h, w, C), channel-last, `src_dtype` M1_RAW_F32 or M1_RAW_I16 (the scans' native type;
 * the load converts, every int16 is exact in fp32), through ONE index map, so that no cropped or padded intermediate volume exists.
 * m1_crop_pad_t: src = (d, h, w), dst = the output extent, output voxel o of an axis reads source index o + start (start < 0 where the
 * axis is padded in front).  An index outside [0, n) goes through `mode`: M1_PAD_CONSTANT -> the value cval, M1_PAD_EDGE -> the nearest
 * voxel, M1_PAD_REFLECT -> period 2(n - 1) without repeating the edge (index 0 when n == 1), M1_PAD_SYMMETRIC -> period 2n with the edge
 * repeated: np.pad's modes, its iterated reflection for pads wider than the axis included.  Every source index is clamped after the
 * map: a wrong table cannot fault.  The axes are independent, which is what P:98 computes (it pads the cropped volume).
 * The "output domain" of a (b, c) slice is its n = dst[0] * dst[1] * dst[2] output values, pad values included: all statistics are
 * taken over it, which is what the reference gets when it whitens after cropping.  Non-finite input is outside the contract (the
 * reference's own result for it is an accident of `image * 0.`): the selection orders NaNs by their bit patterns and the whitened
 * output is then NaN.
 * Common rules: B, C and every extent > 0 and pointers aligned to their element type, else M1_ERR_BAD_ARG; n >= 2^31, C > 8, nq > 4,
 * a mode or dtype outside the enums: M1_ERR_UNSUPPORTED; both before any launch.  ws: m1_preprocess_ws_bytes bytes, 8-byte aligned
 * (one buffer serves m1_order_stats and then m1_whiten of one batch); its contents need no initialisation.  No atomics on global
 * memory, no memset / memcpy nodes, no host synchronisation; results are bit-identical run to run. */
enum m1_raw_dtype { M1_RAW_F32 = 0, M1_RAW_I16 = 1, M1_RAW_I32 = 2 };       /* (M1_RAW_I32: m1_restore with order 0 only) */
enum m1_pad_mode { M1_PAD_CONSTANT = 0, M1_PAD_EDGE = 1, M1_PAD_REFLECT = 2, M1_PAD_SYMMETRIC = 3 };
typedef struct { int src[3]; int dst[3]; int start[3]; int mode; float cval; } m1_crop_pad_t;
/* pure host; nq = 0 sizes the buffer for m1_whiten alone.  0 for arguments the entry points would reject. */
size_t m1_preprocess_ws_bytes(const m1_crop_pad_t* g, int B, int C, int nq);
/* The gather alone: out (B, dst[0], dst[1], dst[2], C) fp32 or bf16 (out_dtype M1_F32 / M1_BF16) = the mapped source values.
 * 16-byte stores when dst[2] * C is a multiple of 4 and out is aligned to 4 elements (vector loads for the runs that are contiguous
 * and aligned in the source), element accesses otherwise. */
int m1_crop_pad(const void* src, int src_dtype, const m1_crop_pad_t* g, int B, int C, void* out, int out_dtype, void* stream);
/* Exact order statistics of every (b, c) slice's output domain.  Quantile j is given as ranks[j] in [0, n) and weights[j] in [0, 1]
 * (HOST arrays of nq entries; numpy's linear rule in fp64: virtual = q / 100 * (n - 1), rank = floor, weight = fraction).  With a[]
 * the sorted slice: pairs (B, C, nq, 2) fp32 = {a[rank], a[min(rank + 1, n - 1)]}, bit-exact (-0.0 and +0.0 are ordered by their
 * sign bits); values (B, C, nq) fp32 = a[rank] + (a[rank + 1] - a[rank]) * weight evaluated in fp64 and rounded once.
 * Method: radix select on the order-preserving 32-bit key of the fp32 value, four passes of 8 bits; the 2 nq ranks advance in the same
 * passes and share a histogram while their prefixes agree.  Per pass one launch of per-block LDS histograms (integer LDS atomics:
 * counts do not depend on order) and one launch that folds the blocks' histograms in ws and advances the prefixes: 8 launches. */
int m1_order_stats(const void* src, int src_dtype, const m1_crop_pad_t* g, int B, int C, const int* ranks, const double* weights,
                   int nq, float* pairs, float* values, void* ws, void* stream);
/* Whitening (P:29-39) of every (b, c) slice's output domain: y = min(max(x, lo), hi) with {lo, hi} = bounds[b][c] when bounds
 * ((B, C, 2) fp32, DEVICE: the `values` of m1_order_stats for the quantiles {100 - p, p}) is not NULL -- lo > hi yields hi everywhere,
 * as np.clip does; mean and population standard deviation (ddof = 0) of y in fp64 (per-block {count, mean, M2} from two sweeps of
 * the block's own chunk, merged in block order by Chan's rule: no sum of raw squares); stats (B, C, 2) fp64 = {mean, std}; then
 * out (B, dst[0], dst[1], dst[2], C) fp32 or bf16 = (y - (float)mean) / (float)std in fp32 with IEEE division when (float)std > 0,
 * +0.0 otherwise; the bf16 store is the round-to-nearest-even of that fp32 value (m1_cast's).  3 launches. */
int m1_whiten(const void* src, int src_dtype, const m1_crop_pad_t* g, int B, int C, const float* bounds, void* out, int out_dtype,
              double* stats, void* ws, void* stream);

/* ---- resampling to a target spacing : P:52-71 resample_img (csrc/resample.hip) ----
 * The reference resamples with SimpleITK's ResampleImageFilter on a grid that keeps origin and direction and uses the identity
 * transform: the grid is axis-aligned and the operation separable.  m1_resample_t: src = (d, h, w), dst = the number of outputs per
 * axis, output o of an axis reads the continuous source index x = (first + o) * step (fp64; step = out_spacing / spacing, first > 0
 * where only a window of the resampled axis is wanted).  A voxel is inside when -0.5 <= x < n - 0.5 on every axis (ITK's
 * IsInsideBuffer) and receives `defval` otherwise.
 *   order 3: cubic B-spline.  One pass per axis in the order 2, 1, 0; a pass prefilters every whole line of its axis (pole sqrt(3) - 2,
 *            gain 6, mirror boundary of period 2(n - 1); a line of one voxel is left as it is) and emits 4-tap sums at floor(x) - 1 ..
 *            floor(x) + 2 through the mirror map.  fp32 values, fp64 coordinates.  The causal start of a line longer than 24 voxels is
 *            the mirror sum truncated after 24 terms (at most 2.6e-14 of max|src| is dropped); shorter lines use its closed form.
 *            This is the algorithm of Unser / Thevenaz that ITK's BSplineDecompositionImageFilter and scipy.ndimage descend from; the
 *            tests pin it against scipy.ndimage (spline_filter + map_coordinates, mode 'mirror').  Parity with ITK itself is NOT
 *            pinned: SimpleITK is not available where this is built.  src fp32 / int16 -> out fp32 (out_dtype M1_RAW_F32).
 *            ws: m1_resample_ws_bytes = 4 * (roundup4(B*C*src[0]*src[1]*dst[2]) + B*C*src[0]*dst[1]*dst[2]) bytes, 16-byte aligned: the
 *            volumes after the passes over axis 2 and axis 1; its contents need no initialisation.  3 launches.
 *   order 0: nearest neighbour, source index floor(x + 0.5) (ITK's round half up).  One gather launch; out_dtype = src_dtype, defval
 *            is converted to it; ws is not used (m1_resample_ws_bytes is 0, ws may be NULL).
 * NULL or misaligned pointers, B, C or an extent <= 0, first < 0, a step that is not finite and positive: M1_ERR_BAD_ARG.  A dtype or
 * order outside the above, C > 8, any volume (source, intermediate, output; times B*C) of 2^31 elements or more, first + dst > 2^30,
 * and for order 3 a source axis longer than M1_RESAMPLE_MAX_LINE: M1_ERR_UNSUPPORTED.  Both before any launch.  No atomics on global
 * memory, no memset / memcpy nodes, no host synchronisation; everything runs on `stream`; results are bit-identical run to run, and
 * an output does not depend on which window it is computed in. */
#define M1_RESAMPLE_MAX_LINE 1024
typedef struct { int src[3]; int dst[3]; int first[3]; int order; double step[3]; float defval; int _pad; } m1_resample_t;
/* pure host.  0 for arguments m1_resample would reject, and for order 0. */
size_t m1_resample_ws_bytes(const m1_resample_t* g, int B, int C);
int m1_resample(const void* src, int src_dtype, const m1_resample_t* g, int B, int C, void* out, int out_dtype, void* ws, void* stream);

/* ---- back-projection onto the scan's own grid (csrc/restore.hip; preprocess.restore is the public surface) ----
 * The inverse of the geometry of preprocess.prepare_scan (resampling to the network's spacing, then crop / pad to the network's
 * size): a map (B, src[0], src[1], src[2], C) on the network's grid is put back on the scan's grid (B, dst[0], dst[1], dst[2]).  The
 * reference ships no such step; it fixes the forward geometry (P:52-71, P:74-98), of which this is the exact inverse.
 * m1_restore_t per axis: dst = the scan's length, ratio = spacing / out_spacing (the reciprocal of m1_resample_t's step), (first,
 * count) = the part of the resampled grid the crop kept, lo = the pad voxels in front on the network grid: the real voxels of the
 * network axis are [lo, lo + count).  Scan voxel i sits at the window coordinate u = i * ratio - first (fp64, product then
 * difference) and is inside when -0.5 <= u < count - 0.5 on every axis; outside voxels receive defval (deflabel in the label
 * output) and read nothing.
 *   order 1: taps floor(u) and floor(u) + 1, each clamped to [0, count - 1] and then offset by lo, weight y = fp32(u - floor(u)), one
 *            axis is a * (1 - y) + b * y in fp32, axes applied in the order 0, 1, 2.  src fp32 -> prob fp32.
 *   order 0: the voxel at floor(u + 0.5), clamped the same way.  src fp32 / int16 / int32 (M1_RAW_I32) -> prob of the same type (defval,
 *            a float, is converted to it: exact up to 2^24 in magnitude).
 * A pad voxel of the network grid is never read.  Outputs, either or both, from one pass over the taps: prob (B, dst..., nsel) = the
 * channels [c0, c0 + nsel) of the restored map (c0 and nsel are not read when prob is NULL); label (B, dst...) uint8 = the argmax
 * over ALL C restored channels, taken on the values that would be stored (strict >, channels in rising order: the first maximum
 * wins).  One launch, no workspace.  A lane stores runs of 4 consecutive voxels: 16-byte stores (8 for int16; 4 for the labels) where
 * the run is whole and starts at a multiple of 4 elements of an aligned pointer, element stores otherwise, and always for nsel >
 * M1_RESTORE_MAX_SEL (the widest selection a lane keeps in registers).
 * NULL src or g, both outputs NULL, B or C < 1, a channel range outside [0, C), C > 255 or a deflabel outside [0, 255] with a label
 * output, an extent or count < 1, first or lo < 0, lo + count > src, a ratio that is not finite and positive, an order other than
 * 0 / 1, an integer type with order 1, a pointer not aligned to its element: M1_ERR_BAD_ARG.  A dtype outside the enum, a source
 * (times B * C) or an output (times B) of 2^31 voxels or more: M1_ERR_UNSUPPORTED.  Both before any
 * launch.  No atomics, no memset / memcpy nodes, no host synchronisation; results are bit-identical run to run. */
#define M1_RESTORE_MAX_SEL 4
typedef struct { int src[3]; int dst[3]; int first[3]; int count[3]; int lo[3]; int order; double ratio[3]; float defval; int deflabel; } m1_restore_t;
int m1_restore(const void* src, int src_dtype, const m1_restore_t* g, int B, int C, int c0, int nsel, void* prob, void* label,
               void* stream);

/* ---- connected components, lesion candidates and matching : train_model.py's `regionprops` import, callbacks.py's `compute_FROC`
 *      (csrc/components.hip; detection.py is the public surface.  The reference ships neither function: the numbering is pinned
 *      against scipy.ndimage.label, the extraction and matching rules are this project's own) ----
 * Volumes are (B, D, H, W) with one value per voxel, n = D * H * W.  Common rules: NULL or misaligned pointers, B or an extent <= 0,
 * connectivity outside 1..3, max_components / max_candidates <= 0, max_a / max_b < 0: M1_ERR_BAD_ARG; B > 65535, B * n >= 2^31 - 1, a table of 2^31 cells or more, a dtype outside the
 * enum: M1_ERR_UNSUPPORTED; both before any launch.  Only integer atomics (min, max, add) touch global memory: results are bit-identical
 * run to run.  No kernel waits for another workgroup; zero fills are kernels (no memset / memcpy nodes); nothing synchronises.
 * m1_cc_label: foreground = src > threshold (strict; fp32 or uint8 source, the uint8 converted to fp32; NaN is background), the
 *   threshold being threshold_dev[b] (DEVICE, B floats) when threshold_dev is not NULL and `threshold` otherwise.  connectivity 1 / 2 / 3
 *   = the 6- / 18- / 26-neighbourhood (scipy.ndimage.generate_binary_structure(3, c)); no neighbour across a row end, a slice end or a
 *   batch entry.  labels (B, D, H, W) int32: 0 = background, components 1..K_b numbered per batch entry in raster order of each
 *   component's first voxel (scipy.ndimage.label's numbering); counts (B) int32 = K_b.  There is no cap on K_b.
 *   ws: m1_cc_ws_bytes(B, D, H, W) bytes, 16-byte aligned, contents need no initialisation.  6 launches: union-find in LDS per
 *   M1_CC_TILE_Z x _Y x _X tile, atomicMin unions across tile borders, flatten into a second buffer, ranks of the roots by a block scan
 *   plus a fixed-order fold of the block totals.
 * m1_cc_stats: rows (B, max_components) of m1_cc_row_t, row l - 1 of a batch entry for its label l <= max_components (larger labels get
 *   no row; rows above K_b are all zero).  values (fp32, same shape) may be NULL: vmax is then 0 and argmax the component's first voxel.
 *   argmax: linear index inside the batch entry of the largest value (-0.0 counts as +0.0), ties to the smallest index; lo / hi: bounding
 *   box per axis (z, y, x), hi exclusive as scipy.ndimage.find_objects; sum: coordinate sums (centroid = sum / count).  3 launches.
 * m1_cc_overlap: table (B, max_a + 1, max_b + 1) int32, table[b][i][j] = voxels with a == i and b == j (row / column 0: background); a
 *   voxel whose label is negative or above its cap is counted nowhere.  2 launches.
 * One round of the dynamic extraction (detection.extract_lesion_candidates), for every batch entry at once, its state in DEVICE memory:
 *   state = 8 * B 4-byte words, word k of sample b at state[k * B + b], k = enum m1_cc_state.
 *   m1_cc_peak: PEAK / ARGMAX = the maximum of w (B, n) fp32 and its index (ties to the smallest), THRESHOLD = PEAK / factor (fp32, IEEE
 *     division), SEL = COUNT = 0; reset != 0 first clears DONE and NCAND; then DONE = 1 where not PEAK > min_confidence.  Per-block
 *     partial maxima in ws (the front of a m1_cc_ws_bytes buffer) folded in block order.  2 launches.
 *   m1_cc_select: SEL = labels[b][ARGMAX] and COUNT = its voxels; 0 / 0 for a sample that is DONE; a SEL of 0 (the peak is background
 *     under its own threshold) sets DONE.  2 launches.
 *   m1_cc_take: where labels == SEL != 0: w = 0 always, and when COUNT >= min_voxels and NCAND < max_candidates: detection_map = PEAK,
 *     candidates = NCAND + 1; then confidences[b][NCAND] = PEAK and NCAND += 1.  reset != 0: every other element of detection_map
 *     (B, n) fp32, candidates (B, n) int32 and confidences (B, max_candidates) fp32 is written as 0 and NCAND starts at 0 -- the first
 *     round initialises the outputs; with w_src (B, n) not NULL it also initialises w = w_src outside the taken component (the
 *     round's peak and labels were then computed from w_src: no copy of the probability map is made beforehand).  2 launches.
 * m1_cc_relabel: the candidates of a FIXED threshold from the rows of m1_cc_stats: components with count >= min_voxels keep their order
 *   and become candidates 1..ncand[b]; map (B, max_components) int32 = candidate number of each row or 0, confidences
 *   (B, max_components) fp32 = vmax per candidate then zeros, candidates / detection_map (B, n) = the number / vmax on the kept
 *   components' voxels and 0 elsewhere.  2 launches. */
#define M1_CC_TILE_Z 4
#define M1_CC_TILE_Y 8
#define M1_CC_TILE_X 32
enum m1_cc_dtype { M1_CC_F32 = 0, M1_CC_U8 = 1 };
enum m1_cc_state {
    M1_CC_ST_PEAK = 0, M1_CC_ST_ARGMAX = 1, M1_CC_ST_THRESHOLD = 2, M1_CC_ST_SEL = 3, M1_CC_ST_COUNT = 4, M1_CC_ST_DONE = 5,
    M1_CC_ST_NCAND = 6, M1_CC_ST_SPARE = 7
};
typedef struct {
    int32_t count;
    float vmax;
    int64_t argmax;
    int32_t lo[3];
    int32_t hi[3];
    int64_t sum[3];
} m1_cc_row_t; /* 64 bytes */
/* pure host.  0 for arguments m1_cc_label would reject. */
size_t m1_cc_ws_bytes(int B, int D, int H, int W);
int m1_cc_label(const void* src, int src_dtype, float threshold, const float* threshold_dev, int connectivity, int B, int D, int H, int W,
                int* labels, int* counts, void* ws, void* stream);
int m1_cc_stats(const int* labels, const float* values, int B, int D, int H, int W, int max_components, m1_cc_row_t* rows, void* stream);
int m1_cc_overlap(const int* a, const int* b, int B, long long n, int max_a, int max_b, int* table, void* stream);
int m1_cc_peak(const float* w, int B, long long n, float factor, float min_confidence, int reset, int* state, void* ws, void* stream);
int m1_cc_select(const int* labels, int B, long long n, int* state, void* stream);
int m1_cc_take(const int* labels, int* state, const float* w_src, float* w, float* detection_map, int* candidates, float* confidences, int B, long long n,
               int max_candidates, int min_voxels, int reset, void* stream);
int m1_cc_relabel(const int* labels, const m1_cc_row_t* rows, int B, long long n, int max_components, int min_voxels, int* map,
                  float* detection_map, int* candidates, float* confidences, int* ncand, void* stream);

/* ---- surface-distance metrics of label maps with voxel spacing : train_model.py's `AnatomySegmentationValidation` import
 *      (csrc/surface.hip; surface_distance.py is the public surface.  The reference never shipped the callback: the definitions are
 *      pinned against scipy.ndimage binary_erosion / distance_transform_edt and numpy's linear percentile) ----
 * Label maps are (B, D, H, W) uint8 or int32, n = D * H * W.  For class k of batch entry b (slice s = b * K + k): A = (pred == labels[k]),
 * B = (truth == labels[k]); border(M) = the voxels of M with at least one of their six face neighbours outside M, outside the volume
 * counting as background.  Common rules: NULL or misaligned pointers, B or an extent <= 0, K outside 1..M1_SD_MAX_CLASSES, a spacing
 * that is not finite and positive, T outside 0..M1_SD_MAX_TOLERANCES, a NaN tolerance, a percentile outside [0, 100]: M1_ERR_BAD_ARG;
 * an axis longer than M1_SD_MAX_LINE (m1_sd_distance only), a dtype outside the enum, n >= 2^31 - 1, more than 65535 stacked volumes:
 * M1_ERR_UNSUPPORTED; both before any launch.  No atomics on global memory, no memset / memcpy nodes, no host synchronisation, no
 * kernel waits for another workgroup; sums are folded in a fixed order: results are bit-identical run to run.
 * m1_sd_border: borders (2, B, K, D, H, W) uint8 = border(A) then border(B) as 0 / 1; counts (B, K, 5) int64 = {|border(A)|, |border(B)|,
 *   |A|, |B|, |A and B|}.  `labels`: K ints in HOST memory.  ws: m1_sd_ws_bytes(M1_SD_STAGE_BORDER, ...) bytes, 4-byte aligned.  2 launches.
 * m1_sd_distance: dist (N, D, H, W) fp32 = the distance of every voxel to the nearest non-zero voxel of its own volume of `mask`
 *   (N, D, H, W) uint8: the exact minimum of sqrt(sum_i (spacing[i] * delta_i)^2), spacing = 3 doubles in HOST memory in array-axis order
 *   (D, H, W), formed in fp64 and rounded once to fp32; +inf where the volume has no non-zero voxel.  Three separable passes, along W, H,
 *   D.  ws: m1_sd_ws_bytes(M1_SD_STAGE_DISTANCE, N, 1, D, H, W) bytes, 16-byte aligned.  3 launches.
 * m1_sd_metrics: borders as m1_sd_border writes them, dist (2, B, K, D, H, W) fp32 = m1_sd_distance of those 2 * B * K volumes (not NaN,
 *   not negative).  Direction 0 is the set d_AB = {dist[1][s][x] : borders[0][s][x] != 0}, direction 1 the set d_BA with the roles
 *   swapped.  rows (B, K) of m1_sd_row_t: n / sum / le[t] = size, fp64 sum and number of elements <= tolerances[t] of each directed set;
 *   hd_ab / hd_ba = the directed maxima, hd their maximum; mean_ab / mean_ba = sum / n, assd = (mean_ab + mean_ba) / 2; hdq_ab / hdq_ba /
 *   hdq = the `percentile`-th percentile of d_AB, of d_BA and of the pooled multiset, by numpy's linear rule: h = (n - 1) * percentile /
 *   100, lo = floor(h), a[lo] + (h - lo) * (a[min(lo + 1, n - 1)] - a[lo]) in fp64, rounded once to fp32; nsd[t] = (le_ab[t] + le_ba[t])
 *   / (n_ab + n_ba).  A set that is empty makes every distance result of the row NaN; nsd is then NaN too, except that two empty sets
 *   give 1; nsd[t] for t >= T is NaN.  dice = 2 |A and B| / (|A| + |B|) from `counts` (the table of m1_sd_border; NaN when both are
 *   empty or counts is NULL).  `tolerances`: T floats in HOST memory.  ws: m1_sd_ws_bytes(M1_SD_STAGE_METRICS, ...) bytes, 16-byte
 *   aligned.  11 launches: partial statistics and their fold, four rounds of histogram and scan of an 8-bit radix select on the fp32
 *   bit pattern, the rows. */
#define M1_SD_MAX_CLASSES 8
#define M1_SD_MAX_TOLERANCES 4
#define M1_SD_MAX_LINE 256
enum m1_sd_dtype { M1_SD_U8 = 0, M1_SD_I32 = 1 };
enum m1_sd_stage { M1_SD_STAGE_BORDER = 0, M1_SD_STAGE_DISTANCE = 1, M1_SD_STAGE_METRICS = 2 };
typedef struct {
    int64_t n[2];
    int64_t le[2][4];
    double sum[2];
    float hd, hd_ab, hd_ba;
    float assd, mean_ab, mean_ba;
    float hdq, hdq_ab, hdq_ba;
    float dice;
    float nsd[4];
    float _pad[2];
} m1_sd_row_t; /* 160 bytes */
/* pure host.  0 for arguments the stage's entry point would reject.  M1_SD_STAGE_DISTANCE: B = the number of stacked volumes, K unused. */
size_t m1_sd_ws_bytes(int stage, int B, int K, int D, int H, int W);
int m1_sd_border(const void* pred, const void* truth, int dtype, const int* labels, int K, int B, int D, int H, int W, uint8_t* borders,
                 long long* counts, void* ws, void* stream);
int m1_sd_distance(const uint8_t* mask, int N, int D, int H, int W, const double* spacing, float* dist, void* ws, void* stream);
int m1_sd_metrics(const uint8_t* borders, const float* dist, const long long* counts, int B, int K, int D, int H, int W, double percentile,
                  const float* tolerances, int T, m1_sd_row_t* rows, void* ws, void* stream);

/* ---- MonteCarloDropout / Dropout : B:142-143 ; N:462-463 (Philox4x32-10, mask regenerated in bwd) ---- */
int m1_dropout(const void* x, void* y, long long n, float rate, const uint64_t* rng, uint64_t layer_id, int dtype,
               void* stream);

/* ---- dtype conversion of activations (fp32 <-> bf16) ---- */
int m1_cast(const void* x, int src_dtype, void* y, int dst_dtype, long long n, void* stream);

/* ---- Keras Adam(amsgrad=True) + L2 regulariser gradient : train_model.py:120 ; N:456-460 ----
 * p,g,m,v,vhat: flat fp32 of n elements; g += 2*lambda*p first (lambda per contiguous range:
 * [0,n_kernel) -> l2_kernel, [n_kernel,n_kernel+n_bias) -> l2_bias, rest -> 0); grad_scale multiplies g
 * (1/world_size after a sum all-reduce). lr_dev[0] = learning rate and step_dev[0] = 1-based step, both in
 * device memory (graph replay). All five buffers 16-byte aligned. */
int m1_adam_amsgrad(float* p, const float* g, float* m, float* v, float* vhat, long long n, long long n_kernel,
                    long long n_bias, float l2_kernel, float l2_bias, float grad_scale, const float* lr_dev,
                    float beta1, float beta2, float eps, const int* step_dev, void* stream);
/* step_dev[0] += 1 (may be NULL); rng_dev[1] += 1 (may be NULL). */
int m1_step_advance(int* step_dev, uint64_t* rng_dev, void* stream);

/* ---- Guarded step: tf.keras' clipvalue / global_clipnorm and a skip of non-finite gradients, decided on the device ----
 * All of it works on the regularised gradient gr = g*grad_scale + 2*lambda*p of m1_adam_amsgrad (same ranges, same fp32 evaluation):
 * Keras clips what the optimiser receives.  clipvalue clamps every gr to [-clipvalue, clipvalue] first (NaN stays NaN, +-Inf is
 * clamped); the global norm is taken over the clamped values.  0 switches clipvalue / global_clipnorm off; negative, NaN and Inf
 * are M1_ERR_BAD_ARG.  The 16-byte record (device memory, 16-byte aligned, zero before its first use) carries the decision from
 * m1_grad_norm to m1_adam_amsgrad_ctl and m1_step_advance_ctl inside one captured step. */
typedef struct {
    float norm;        /* (float)sqrt(sum of clamp(gr)^2), the sum in fp64: Inf / NaN when a gradient is */
    float coef;        /* global_clipnorm / norm when global_clipnorm > 0 and norm > global_clipnorm, otherwise exactly 1;
                        * NaN when the sum is not finite, global_clipnorm > 0 and the guard is off (as tf.clip_by_global_norm) */
    int32_t apply;     /* 0: skip_nonfinite is on and the sum is not finite -- the update and the step advance do nothing */
    int32_t skipped;   /* number of launches of m1_grad_norm on this record that set apply = 0 */
} m1_step_ctl_t;
/* Bytes of `ws` for n elements (pure host call; 8-byte aligned workspace, no initialisation needed). */
size_t m1_grad_norm_ws(long long n);
/* Two launches: per-block fp64 partial sums into ws (grid = f(n, M1_EW_BLOCKS) <= 2048 blocks; no atomics: the same input gives the
 * same bits), then one block that folds them in a fixed order and writes *ctl.  p is read only when l2_kernel or l2_bias is
 * non-zero (it must still be a valid 16-byte aligned pointer).  g, p 16-byte aligned. */
int m1_grad_norm(const float* g, const float* p, long long n, long long n_kernel, long long n_bias, float l2_kernel,
                 float l2_bias, float grad_scale, float clipvalue, float global_clipnorm, int skip_nonfinite, void* ws,
                 size_t ws_bytes, m1_step_ctl_t* ctl, void* stream);
/* m1_adam_amsgrad on clamp(gr, clipvalue) * ctl->coef; nothing is read or written when ctl->apply == 0.  With clipvalue == 0 and
 * coef == 1 the result equals m1_adam_amsgrad's bit for bit. */
int m1_adam_amsgrad_ctl(float* p, const float* g, float* m, float* v, float* vhat, long long n, long long n_kernel,
                        long long n_bias, float l2_kernel, float l2_bias, float grad_scale, const float* lr_dev,
                        float beta1, float beta2, float eps, const int* step_dev, float clipvalue,
                        const m1_step_ctl_t* ctl, void* stream);
/* step_dev[0] += ctl->apply. */
int m1_step_advance_ctl(int* step_dev, const m1_step_ctl_t* ctl, void* stream);

/* ---- Per-case scoring of a validation batch : callbacks.py:17-40 (dice_3d), losses.py:32-41 (Focal.FL) ----
 * One streaming pass (csrc/validate.hip) over p (B, voxels, K) fp32 -- the softmax, or the mean of n draws --, y (B, voxels, K) one-hot
 * (y_dtype: enum m1_val_dtype) and entropy (B, voxels) fp32 or NULL leaves one record of 40 doubles per case:
 *   focal          sum over voxels and classes of alpha_c * y * (1 - q)^gamma * (y * -log q), q = clip(p_c / sum_k p_k, 1e-7, 1 - 1e-7)
 *                  evaluated in fp32 as m1_focal_fwd evaluates it, summed in fp64: the mean over the batch is Focal.FL(y, p)
 *   entropy_sum, entropy_fg_sum   over all voxels / over voxels whose true class (the argmax of y) is 1 or higher; 0 without entropy
 *   n_voxels, n_fg                voxels of the case / of them with a true class of 1 or higher
 *   cls[c].sum_p, sum_y, sum_py   fp64 sums of p_c, y_c and p_c * y_c: dice_3d = (2 sum_py + 1e-7) / (sum_p + sum_y + 1e-7)
 *   cls[c].n_pred, n_true, n_both voxels whose argmax of p / of y / of both is c (the lowest index among equals, as np.argmax)
 *   cls[c].p_max                  the largest p_c of the case (0 when every p_c is negative or NaN)
 * Counts are whole numbers stored as doubles; unused slots, and the classes >= K, are 0.
 * Two launches: per (block, case) one partial row of 40 doubles into ws, then one block per case that folds the rows in a fixed
 * order.  No atomics, no memset / memcpy nodes; the grid is a function of (B, voxels, K) alone and pointer alignment only widens the
 * loads, so a record repeats bit for bit.  alpha: K HOST floats.  ws: m1_val_score_ws bytes (pure host call), 8-byte aligned, no
 * initialisation needed.  NULL p / y / alpha / records / ws, a pointer not aligned to its element (records, ws: 8 bytes), a y_dtype
 * outside the enum, B, K or voxels <= 0: M1_ERR_BAD_ARG; K > 4 or B > 65535: M1_ERR_UNSUPPORTED; ws_bytes too small:
 * M1_ERR_WORKSPACE; all before any launch. */
enum m1_val_dtype { M1_VAL_Y_F32 = 0, M1_VAL_Y_U8 = 1 };
typedef struct {
    double focal, entropy_sum, entropy_fg_sum, n_voxels, n_fg, _head[3];
    struct { double sum_p, sum_y, sum_py, n_pred, n_true, n_both, p_max, _pad; } cls[4];
} m1_val_record_t; /* 320 bytes */
size_t m1_val_score_ws(int B, long long voxels, int K);
int m1_val_score(const float* p, const void* y, int y_dtype, const float* entropy, const float* alpha, float gamma, int B,
                 long long voxels, int K, m1_val_record_t* records, void* ws, size_t ws_bytes, void* stream);

/* ---- Calibration record of a validation batch (no reference counterpart; calibration.py: ECE, MCE, Brier, NLL, referral) ----
 * One streaming pass (csrc/calibrate.hip) over p (B, voxels, K) fp32 or bf16 (p_dtype: enum m1_dtype) -- the softmax, or the mean of
 * n draws --, label (B, voxels) uint8 class indices, mask (B, voxels) uint8 or NULL (0 skips the voxel, uncounted) and unc
 * (B, voxels) fp32 or NULL (entropy, mutual information, ...) leaves one record of m1_cal_record_slots(K, bins) = 8 + 3 * bins * (K + 2)
 * unsigned 64-bit integers per case.  2 <= K <= 4, 1 <= bins = M <= 64, voxels < 2^27.
 * Per voxel, am = argmax of p (the lowest index among equals, as np.argmax), conf = p[am], y = label:
 *   a voxel with a NaN p[c], or a NaN unc, counts in n_invalid and nowhere else; otherwise one with y >= K (an ignore label) counts
 *   in n_ignored and nowhere else; the rest count in n_valid and in everything below.
 *   fx(v)  = floor(max(v, 0) as a double * 2^32): sums of real quantities are 2^-32 fixed point (exact for an fp32 v >= 2^-9)
 *   bin(v) = min(M - 1, (int)clip(v * (float)M, 0, M)), the product one fp32 multiply
 * Slots:
 *   [0] n_valid  [1] n_invalid  [2] n_ignored
 *   [3] nll            += fx(-log((double)max(p[y], 1e-7f))), the log in fp64, p as given (no renormalisation)
 *   [4 + c] brier[c]   += fx(d * d), d = (double)p[c] - (y == c); c < 4, zero for c >= K
 *   then K + 2 histograms of 3 * M slots each, histogram h at 8 + 3 * M * h: count[M], sum[M], hits[M]
 *   h = 0         top:    at bin(conf)      count += 1, sum += fx(conf),      hits += (am == y)
 *   h = 1 + c     cls[c]: at bin(p[c])      count += 1, sum += fx(p[c]),      hits += (y == c)
 *   h = K + 1     unc:    at bin of u       count += 1, sum += fx(max(u, 0)), hits += (am != y); all zero without unc.
 *                 Its bin is min(M - 1, (int)clip(u * u_scale, 0, M)), u_scale = (float)(M / u_max) computed by the caller.
 * p and unc are expected finite (p a probability, u <= 16.2): nothing then overflows.  Every accumulator is an integer, so the
 * record does not depend on the order of the additions and repeats bit for bit; only nll depends on the device's fp64 log.
 * Two launches: a kernel zero-fills the records (no memset node), then the scoring kernel (grid = f(B, voxels, M1_EW_BLOCKS)) adds
 * per-block LDS histograms into them with 64-bit integer atomics.  No host read, no float atomics; pointer alignment only chooses
 * the width of the loads.  NULL p / label / records, a pointer not aligned to its element (records: 8 bytes), a p_dtype outside the
 * enum, B or voxels <= 0, voxels >= 2^27, K or bins out of range, unc with a u_scale that is not positive and finite:
 * M1_ERR_BAD_ARG; B > 65535: M1_ERR_UNSUPPORTED; all before any launch.  m1_cal_record_slots is a pure host call, 0 when K or
 * bins is out of range. */
size_t m1_cal_record_slots(int K, int bins);
int m1_cal_score(const void* p, int p_dtype, const unsigned char* label, const unsigned char* mask, const float* unc, float u_scale,
                 int B, long long voxels, int K, int bins, unsigned long long* records, void* stream);

/* ---- Case-level bootstrap replicates (no reference counterpart; bootstrap.py: AUROC, AP, FROC sensitivities, per-case means) ----
 * The table is sorted once on the host (bootstrap.pack); csrc/bootstrap.hip computes one replicate per workgroup of 256 threads from
 * the case multiplicities w[N], which it keeps in LDS (N <= M1_BOOTSTRAP_MAX_CASES = 16384: 64 KiB).
 *   cases, in ASCENDING score order: case_label[N] (uint8, non-zero: a positive case), case_group_end[N] (uint8, 1 on the last case of
 *     a run of equal scores), case_lesions[N] (int32, the case's annotated lesions, missed ones included: the recall denominator)
 *   events -- unmatched candidates and matched lesions with confidence > 0 -- in DESCENDING confidence order: ev_case[M] (int32, index
 *     into the case order above), ev_tp[M] (uint8, non-zero: a matched lesion), ev_group_end[M] (uint8).  M = 0 is legal.
 *   values (V, N) fp64 or NULL with V = 0: row v holds one scalar per case (case order above), NaN = the case has none.  V <= 16.
 *   draw_perm[N] (int32) or NULL (identity): the case index, in the order above, behind every index a draw picks.  bootstrap.pack
 *     maps the caller's ORIGINAL case order here, so that two tables of the same cases get the same resamples whatever their scores;
 *     for the stratified draw (P >= 0) the P positive cases come first.  An entry outside [0, N) drops the draw.
 * The draw (without `weights`): Philox4x32-10 under the key seed + M1_STREAM_BOOTSTRAP * 0x9E3779B97F4A7C15 (mod 2^64; the other
 * consumers' ids -- dropout layers 1, 2, ..., the augmentation table 0xA06D + 2 * rank and noise 0xA06E + 2 * rank, the latent heads
 * 0x4C415400 + 8 * core + level -- are given by their callers).  Draw j < N of replicate b reads word j & 3 of counter
 * (b << 12) + (j >> 2) and picks draw_perm[(word * N) >> 32]; stratified (P >= 0): j < P picks draw_perm[(word * P) >> 32], j >= P
 * picks draw_perm[P + ((word * (N - P)) >> 32)].  w[i] = how often case i was picked: a pure function of (seed, b).
 * `weights` (n_boot, N) int32 or NULL: row b REPLACES the draw (case order above; values are clamped to [0, 65535]).
 * Row b of out (n_boot, 2 + n_rates + V) fp64, with P_w / N_w / S_w = the weight of the positive / negative / all cases and
 * L_w = sum of w * case_lesions:
 *   [0] auroc = 2U / (2 * P_w * N_w), 2U = sum over the groups of equal scores of pos_g * (2 * neg_below + neg_g), all weighted 64-bit
 *       integers, one fp64 division: Mann-Whitney with ties counting half.  NaN unless P_w > 0 and N_w > 0.
 *   [1] ap = sum over the event groups k, in order, with tp_k > tp_{k-1} of ((double)tp_k / L_w - (double)tp_{k-1} / L_w)
 *       * ((double)tp_k / (double)(tp_k + fp_k)); tp_k, fp_k = weighted counts down to the group's end.  NaN when L_w = 0.
 *   [2 + r] sens@fp_rates[r] = tp_k / L_w at the last group end with (double)fp_k / (double)S_w <= fp_rates[r]; 0 without one;
 *       NaN when L_w = 0.
 *   [2 + n_rates + v] = sum of (double)w_i * values[v][i] over the cases with w_i > 0 and a value that is not NaN, divided by their
 *       weight; NaN without one.
 * The integers do not depend on any order; the AP sum and the value sums are fp64 folds in a fixed order (thread, wave, block): a row
 * repeats bit for bit over runs, n_boot (row b of a longer call is row b of a shorter one) and pointer alignments.  One launch, no
 * global workspace, no memset / memcpy node, no host read; fp_rates: HOST doubles, passed by value.
 * NULL table / out / a required array, N < 1, M < 0, n_boot < 1, n_rates outside 0..8, V outside 0..16, P > N,
 * a pointer not aligned to its element: M1_ERR_BAD_ARG; n_boot > 2^20 or N > 16384: M1_ERR_UNSUPPORTED; all before any launch. */
#define M1_STREAM_BOOTSTRAP 0x424F4F54ull        /* "BOOT" */
#define M1_BOOTSTRAP_MAX_CASES 16384
#define M1_BOOTSTRAP_MAX_BOOT (1 << 20)
#define M1_BOOTSTRAP_MAX_RATES 8
#define M1_BOOTSTRAP_MAX_VALUES 16
#define M1_BOOTSTRAP_CHUNK 1024                  /* cases / events per block-wide scan */
typedef struct {
    const unsigned char* case_label; const unsigned char* case_group_end; const int* case_lesions;
    const int* ev_case; const unsigned char* ev_tp; const unsigned char* ev_group_end;
    const double* values; const int* draw_perm;
    int N, M, V, P;                              /* P < 0: the draw is not stratified */
} m1_bootstrap_table_t;
int m1_bootstrap_metrics(const m1_bootstrap_table_t* table, int n_boot, uint64_t seed, const int* weights, const double* fp_rates,
                         int n_rates, double* out, void* stream);

/* Deferred folds of the weight-gradient partial copies (no reference counterpart; the reference's tf.GradientTape sums weight
 * gradients inside each op).  m1_conv3d_wgrad / m1_convT3d_wgrad split the voxels over blocks, every block stores its partial
 * tile into a copy inside `ws`, and a fold kernel adds the copies into dw / db in a fixed order.  After m1_wgrad_defer(1) the
 * weight-gradient entry points QUEUE that fold instead of launching it (process-wide, host side); m1_wgrad_fold_pending runs
 * everything queued in a few batched launches on `stream` -- the caller orders `stream` behind the weight-gradient launches and
 * keeps alive until then every `ws` and, for m1_convT3d_wgrad with a db, also d(out): the bias gradient of a transposed conv is
 * a column sum of d(out), queued with the folds and READ at m1_wgrad_fold_pending.  dw / db are incomplete before.
 * m1_wgrad_fold_drop forgets the queue (gradients discarded).  The same parameter twice inside one window: a second fold into
 * a block of dw that already has one queued is NOT queued and does not run the queue -- it is launched at once on its own call's
 * stream (the queue may hold work of streams that call is not ordered behind) and the queued one still runs at
 * m1_wgrad_fold_pending; a second column sum into a db that has one queued is computed at once, in place, likewise. */
int m1_wgrad_defer(int on);
int m1_wgrad_fold_pending(void* stream);
int m1_wgrad_fold_drop(void);

/* ---- opt-in per-kernel-family timing with hipEvents on the launch stream (bench.py roofline) ---- */
int m1_prof_enable(int on);
int m1_prof_reset(void);
/* after a stream sync: fills up to max_n records; returns count. */
typedef struct {
    char name[48];
    double total_ms;
    double flops; /* algorithmic flops summed over launches */
    double bytes; /* algorithmic bytes summed over launches */
    long long launches;
} m1_prof_rec_t;
int m1_prof_read(m1_prof_rec_t* out, int max_n);

#ifdef __cplusplus
}
#endif
#endif /* M1HIP_H */
