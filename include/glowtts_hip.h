/*
 * glowtts_hip.h — C-ABI of the MI355X-native (gfx950) Glow-TTS training hot path.
 *
 * Drop-in boundary: every entry point takes plain device pointers + sizes and a HIP
 * stream (passed as void* so this header needs no HIP include), is asynchronous on
 * that stream, allocates nothing, keeps no global state and never throws.
 * Return value: 0 = ok, negative = error (GT_E_*).  The caller (a PyTorch-ROCm
 * shim, see glow-tts_amd/_lib.py, or any other host) owns all memory.
 *
 * Each function names the reference interface it replaces (paths are relative to the
 * reference repository arkiven4/glow-tts).
 */
#ifndef GLOWTTS_HIP_H
#define GLOWTTS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* error codes */
#define GT_OK            0
#define GT_E_INVAL      -1   /* bad argument (null pointer, negative size, ...)        */
#define GT_E_UNSUPPORTED -2  /* shape outside what the kernel supports (see function)  */
#define GT_E_ALIGN      -3   /* pointer / stride alignment requirement violated        */
#define GT_E_LAUNCH     -4   /* hipLaunchKernel reported an error                      */

/* element types for outputs whose dtype follows the caller's tensor */
#define GT_DT_F32  0
#define GT_DT_I32  1
#define GT_DT_F16  2
#define GT_DT_BF16 3
#define GT_DT_U8   4

/* bits set in *status by gt_mas_f32 */
#define GT_MAS_ST_TX_GT_TY   1  /* some utterance had t_x > t_y (reference: silent OOB read,
                                   monotonic_align/core.pyx:34 with boundscheck off)          */
#define GT_MAS_ST_BAD_LEN    2  /* some utterance had t_x/t_y < 0 or beyond T_x/T_y           */

/* library identification: returns a static string "glowtts_hip <version> gfx950". */
const char* gt_version(void);

/* ------------------------------------------------------------------------------------
 * Monotonic Alignment Search.
 * Replaces: monotonic_align/core.pyx:38-45  maximum_path_c(paths, values, t_xs, t_ys)
 *           (+ :9-35 maximum_path_each) and the host wrapper
 *           monotonic_align/__init__.py:6-21 maximum_path(value, mask).
 *
 *   logp        [B, T_x, T_y] fp32 log-likelihood lattice, last dim contiguous,
 *               element (b,x,y) at logp[b*stride_b + x*stride_x + y].  NOT modified
 *               (the reference mutates its private copy).
 *   mask        optional (may be NULL) fp32 tensor with the same strides; when given the
 *               kernel uses logp*mask exactly like __init__.py:11.
 *   t_x, t_y    [B] int32 valid lengths per utterance (__init__.py:18-19).
 *   path        optional (may be NULL) [B, T_x, T_y] contiguous output of element type
 *               path_dtype (GT_DT_*): 1 on the alignment path, 0 elsewhere — every element
 *               is written (by a second, chip-wide kernel on the same stream).
 *   durations   optional [B, T_x] fp32: row sums of path (models.py:1085 `w`).
 *   frame2token optional [B, T_y] int32: for each frame y < t_y the row x with
 *               path[b,x,y]==1, else -1 (lets the prior expansion models.py:1118-1119
 *               be a gather instead of a matmul with a one-hot matrix).
 *   workspace   device scratch of at least gt_mas_workspace_bytes(B,T_x,T_y) bytes, 4-byte
 *               aligned; after the call it holds int32 [B, T_x+1] row start columns (row x of
 *               utterance b is aligned to frames [ws[b][x], ws[b][x+1]) ).
 *   status      optional device int32, OR-ed with GT_MAS_ST_* bits.  Utterances with
 *               invalid lengths get an all-zero path.
 *
 * Limits: T_x <= 512, and gt_mas_lds_bytes(T_x,T_y) <= 160 KiB, else GT_E_UNSUPPORTED (gt_mas_long_f32 takes those).
 * Bit-exact with the reference for every t_x <= t_y (IEEE fp32, same tie-breaks).
 */
int gt_mas_f32(const float* logp, const float* mask,
               const int32_t* t_x, const int32_t* t_y,
               void* path, int path_dtype,
               float* durations, int32_t* frame2token,
               int B, int T_x, int T_y, int64_t stride_b, int64_t stride_x,
               void* workspace, size_t workspace_bytes,
               int32_t* status, void* stream);

/* Scratch bytes gt_mas_f32 needs for a batch (host helper). */
size_t gt_mas_workspace_bytes(int B, int T_x, int T_y);

/* LDS bytes one workgroup of gt_mas_f32 needs for a [T_x, T_y] lattice (host helper). */
size_t gt_mas_lds_bytes(int T_x, int T_y);

/* Monotonic Alignment Search for the lattices gt_mas_f32 refuses (T_x > 512, or gt_mas_lds_bytes > 160 KiB).  Arguments,
 * outputs, status bits and error codes are gt_mas_f32's, word for word: the logp*mask form, any stride_b / stride_x, path in the
 * five GT_DT_* types with every element written by the same chip-wide kernel, durations, frame2token (-1 past t_y), an all-zero
 * path for invalid or empty utterances; asynchronous on `stream`, no allocation, no host synchronisation.  Bit-exact with the
 * reference for every t_x <= t_y, and with gt_mas_f32 wherever both accept the lattice (gt_mas_f32 is the faster one there:
 * callers dispatch to it first).
 *
 * The rows are walked in bands of 512 by one workgroup per utterance; the direction bits (T_x*T_y/8 bytes) and the band
 * boundaries live in the workspace, nothing in LDS grows with T_x*T_y.
 *   workspace   at least gt_mas_long_workspace_bytes(B,T_x,T_y) bytes, 4-byte aligned.  Its head is the same int32
 *               [B, T_x+1] row start columns gt_mas_f32 leaves; the rest is scratch.
 * Limits (checked on the host, GT_E_UNSUPPORTED): T_x <= GT_MAS_LONG_MAX_TX (row starts in LDS), T_y <= GT_MAS_LONG_MAX_TY,
 * B <= GT_MAS_LONG_MAX_B (grid of the path kernel). */
#define GT_MAS_LONG_MAX_TX 4096
#define GT_MAS_LONG_MAX_TY 32768
#define GT_MAS_LONG_MAX_B  65535
int gt_mas_long_f32(const float* logp, const float* mask,
                    const int32_t* t_x, const int32_t* t_y,
                    void* path, int path_dtype,
                    float* durations, int32_t* frame2token,
                    int B, int T_x, int T_y, int64_t stride_b, int64_t stride_x,
                    void* workspace, size_t workspace_bytes,
                    int32_t* status, void* stream);

/* Scratch bytes gt_mas_long_f32 needs for a batch (host helper): row starts + two band-boundary rows per utterance +
 * B * ceil(T_x/64)*64 * ceil(T_y/32) direction words.  0 for an empty batch. */
size_t gt_mas_long_workspace_bytes(int B, int T_x, int T_y);

/* Lengths from a [B,T_x,T_y] fp32 mask the way monotonic_align/__init__.py:18-19 does:
 * t_x[b] = sum_x mask[b,x,0], t_y[b] = sum_y mask[b,0,y] (truncated to int32). */
int gt_mas_lengths_from_mask_f32(const float* mask, int32_t* t_x, int32_t* t_y,
                                 int B, int T_x, int T_y, int64_t stride_b, int64_t stride_x,
                                 void* stream);

/* ------------------------------------------------------------------------------------
 * "Rows" activation layout used by every kernel below: [R, C] channels-last (C contiguous),
 * uniform: R = B * Tp, utterance b owns rows [b*Tp, (b+1)*Tp), Tp = T + 2*HALO (HALO = 2); ragged: every entry point
 * that takes Tp also takes `row0` (device int32 [B+1], NULL = uniform): utterance b owns rows [row0[b], row0[b+1]) =
 * its own frames + 2*HALO (the last utterance also owns the rows that round R up), so frames past an utterance's
 * length cost no work, and Tp is only an upper bound on the rows of one utterance (grid sizing).  Frame t of
 * utterance b is row base(b) + HALO + t; halo rows and rows past the utterance length are zero
 * (rowmask[R] is 1 on valid frames, 0 elsewhere).  bf16 tensors are raw uint16 bit patterns.
 */
#define GT_HALO 2

/* 1-D convolution (odd k <= 5, dilation 1) as implicit GEMM on bf16 MFMA, fp32 accumulate.
 * Replaces the conv1d calls of modules.py:152,165 / attentions.py:144,172,232-238,365-371 /
 * modules.py:97 / models.py:710 and, with dgrad-packed weights, their data gradients.
 *   Y[m,n] = epi( sum_tap sum_ci X[m + tap - k/2, ci] * W[tap][n][ci] + bias[n] + cond[u(m)][n] )
 *   cond (may be NULL): [B, ldc] fp32 with u(m) = utterance of row m when B > 0 (WN.cond_layer(g), modules.py:148-156);
 *        [R, ldc] fp32 with u(m) = m when B == 0 (per-frame conditioning: WNP.cond_layer1(pitch), modules.py:316-334).
 *   epi: optional relu, optional dropout (drop_p, counter-based on (m,n)), optional + addend[m,n],
 *        optional * rowmask[m]; output bf16 or fp32.
 *   gate == 1 (WaveNet gate, commons.py:61-68; N = 2*half, packed with the gate interleave):
 *     pre = drop(acc + bias) + cond;  T = tanh(pre[:half]), S = sigmoid(pre[half:]),
 *     Y[m, :half] = T*S (bf16), T and S are saved to gate_t / gate_s ([R, ldts] bf16; ldts%8, ldy%8 == 0).
 *     This epilogue has no relu, addend or rowmask: any of them returns GT_E_INVAL.
 *   gate == 2 (backward of that gate fused behind a data-gradient GEMM): d = acc + addend is d(T*S);
 *     gate_t / gate_s are the SAVED T / S (read-only); Y is [R, 2N] bf16: Y[m, n] = d*S*(1-T^2), Y[m, N+n] =
 *     d*T*S*(1-S), both times the forward's dropout mask (drop_p / drop_seed as given to the forward call).
 *   gate == 3 (backward of y = dropout(relu(.)), attentions.py:368-370 / modules.py:97-99, fused behind a data-gradient
 *     GEMM): gate_t is the SAVED y ([R, ldts] bf16, read-only; gate_s unused); Y[m, n] = (acc + addend) / (1 - drop_p)
 *     where y[m, n] != 0, else 0 (bf16; N%8, ldts%8, ldy%8 == 0).  No mask is drawn: drop_p only gives the scale.
 *   Wp: weights packed by gt_pack_conv_weights ([taps][Np][Kp] bf16, zero padded).
 * Dropout masks are a counter-based hash of (seed, row, col), replayed by the backward kernels.
 * seed_dev (here and in every entry point that takes it; may be NULL) is a device uint32 XOR-ed into the
 * host seed at kernel start: a captured HIP graph then draws fresh masks on every replay by bumping that word.
 * tile: 0 = the library's choice from (R, Np, gate); tests force a variant with GT_TILE_64x64 … GT_TILE_256x64
 * (rows x packed channels per workgroup; a variant the shape does not allow returns GT_E_INVAL).
 * End rows: the kernels CLAMP the row index m + tap - k/2 into [0, R-1] instead of reading zeros outside [0, R).  The two agree
 *   because the first and last k/2 rows of X are zero — halo rows of the first and last utterance in the rows layout (k/2 <= GT_HALO).
 *   That is a precondition of every call with k > 1; with other rows there, only Y's first and last k/2 rows differ from the
 *   zero-padded sum (tests/test_conv_gemm_fp64_gpu.py pins the clamp).
 * Alignment (GT_E_ALIGN otherwise): X, Wp, Y, bias, cond, gate_t, gate_s and a fp32 addend 16 B, a bf16 addend 8 B, rowmask 4 B;
 *   N%4, Cin%8, ldx%8, ldy%4, ldadd%4, ldc%4, Kp%64 == 0. */
#define GT_TILE_AUTO 0
#define GT_TILE_64x64 1
#define GT_TILE_64x128 2
#define GT_TILE_128x64 3
#define GT_TILE_128x128 4
#define GT_TILE_256x64 5
#define GT_TILE_64x64_TAPS 6   /* 64 x 64, all taps of a K slice per pipeline stage (short, deep convs; no gate) */
int gt_conv_gemm_bf16(const void* X, int ldx, const void* Wp, const float* bias,
                      const float* cond, int ldc, const float* rowmask,
                      void* Y, int ldy, int out_f32, const void* addend, int ldadd,
                      void* gate_t, void* gate_s, int ldts,
                      int R, int N, int Cin, int taps, int Tp, int Np, int Kp,
                      int relu, int gate, float drop_p, uint32_t drop_seed, const uint32_t* seed_dev,
                      const int32_t* row0, int B, int tile, void* stream);

/* Weight preparation for gt_conv_gemm_bf16: w = g*v/||v|| when g != NULL (torch weight_norm,
 * dim 0: modules.py:127,132,141, attentions.py:103) else w = v; v is [Cout, Cin, taps] fp32.
 * Writes bf16 pack_fwd [taps][Np_fwd][Kp_fwd] and/or pack_dgrad [taps][Np_dgrad][Kp_dgrad]
 * (roles swapped, taps flipped) and inv_norm[Cout] = 1/||v|| (optional; pack pointers may both be NULL when only
 * the norms are wanted).  Padding entries are not touched: zero the buffers once.
 * `gate` is a bit set: 1 = WaveNet-gate row interleave of the forward image ([32 tanh | 32 sigmoid] per 64 rows),
 * 2 = forward image in MFMA-fragment order [tap][n/32][k/16][lane = n%32 + 32*((k%16)/8)][k%8] (one 1-KB MFMA A-fragment per (n/32, k/16): the fused WaveNet-layer kernels),
 * 4 = the same for the data-gradient image (Np, Kp multiples of 32 / 16 then),
 * 16 = the gate interleave at MFMA-block granularity, [16 tanh | 16 sigmoid] per 32 packed rows (instead of 1): every 32-column
 *     accumulator block then holds both halves of its 16 gate channels in the same lanes (gt_wn_layer_fwd's in-register gate),
 * 8 = bf16x3 ("split") images for a near-fp32 product out of three bf16 MFMA passes: the reduction axis is K-concatenated
 *     as [w_hi ; w_lo ; w_hi] (Kp >= 3*Cin resp. 3*Cout; w_hi = bf16(w), w_lo = bf16(w - w_hi)) and meets activations laid
 *     out as [x_hi | x_hi | x_lo] (gt_rows_split3): x_hi w_hi + x_hi w_lo + x_lo w_hi.  The stochastic predictors' 1x1 convs
 *     use it (their spline flows amplify bf16 rounding of the conditioning chaotically); not with 1, 2, 4;
 *     only through the one-row-per-workgroup packing (group8 == 0). */
int gt_pack_conv_weights(const float* v, const float* g, void* pack_fwd, void* pack_dgrad,
                         float* inv_norm, int Cout, int Cin, int taps,
                         int Np_fwd, int Kp_fwd, int Np_dgrad, int Kp_dgrad, int gate, void* stream);

/* The same for every conv of a model in ONE launch: `descs_device` is a device array of n_convs
 * descriptors sorted by row_start (row_start = prefix sum of Cout), total_rows = sum of Cout.  group8 != 0: every conv has
 * Cout % 8 == 0, Cin % 8 == 0 and Cin*taps <= 2304 — 8 output channels per workgroup, both images written with 16-byte
 * stores (else one workgroup per output channel). */
typedef struct gt_pack_desc {
  const float* v; const float* g; void* pack_fwd; void* pack_dgrad; float* inv_norm;
  int32_t Cout, Cin, taps, Np_fwd, Kp_fwd, Np_dgrad, Kp_dgrad, gate, row_start, pad_;
} gt_pack_desc;
/* group8: 0 one workgroup per output channel; 1 eight output channels per workgroup (every conv: Cout % 8 == 0, Cin % 8 == 0,
 * Cin * taps <= 2304); 2 the same for tables whose every conv has Cin * taps <= 1024 (less LDS and fewer registers per workgroup). */
int gt_pack_conv_weights_multi(const void* descs_device, int n_convs, int total_rows, int group8, void* stream);

/* Weight gradient of the rows-layout convolution: partial sums over S row slabs into
 * workspace [S][taps][Cout][Cin] fp32 (S from gt_conv_wgrad_workspace_bytes), bf16 MFMA with
 * transposing LDS reads.  dW[tap][co][ci] = sum_m dY[m,co] * X[m + tap - k/2, ci].
 * (ATen conv backward-weight in the reference, reached through autograd.) */
size_t gt_conv_wgrad_workspace_bytes(int R, int Cin, int Cout, int taps, int* slabs_out);
/* input channels one workgroup tile of the weight-gradient kernel spans at this tap count (64 at k = 3 and 5, 192 at k = 1): the ci0
 * granularity of gt_wgrad_tile below; 0 for an unsupported tap count. */
int gt_conv_wgrad_ci_tile(int taps);
int gt_conv_wgrad_bf16(const void* X, int ldx, const void* dY, int ldy, int R, int Cin, int Cout,
                       int taps, void* workspace, size_t workspace_bytes, void* stream);

/* Reduce the wgrad workspace and map it onto the parameter gradient(s) in the parameter's own
 * [Cout, Cin, taps] layout: plain conv (g == NULL): dv (+)= dW; weight-normed conv
 * (torch weight_norm dim 0): dg = <dW,v>/||v||, dv = g/||v|| (dW - v <dW,v>/||v||^2).
 * dbias (optional) receives the bias gradient: the wgrad kernel also leaves the column sums of dY
 * per slab in the workspace (summed from the MFMA A fragments it reads anyway). */
int gt_weightnorm_bwd(const void* workspace, int R, const float* v, const float* g, const float* inv_norm,
                      float* dv, float* dg, float* dbias, int Cout, int Cin, int taps, int accumulate, void* stream);

/* Batched forms: the weight gradients of a whole network in one launch per tap count, after the
 * data-gradient chain has run (every job's X and dY rows stay resident in HBM until then), and ONE
 * weight-norm backward over all of them.  Tables live in device memory.
 *   job:  dY column c is output channel co_begin + c (co_count columns) of a conv with Cout channels whose
 *         partials are part[S][taps][Cout][Cin] (+ part_bias[S][Cout], may be NULL); slab_rows % 64 == 0.
 *   tile: one workgroup = 128 dY columns from co0 x gt_conv_wgrad_ci_tile(taps) input channels from ci0 x all taps x rows of `slab`;
 *         tiles are ordered taps 5, then 3, then 1.
 *   wnb job: as gt_weightnorm_bwd, rows [row_start, row_start + Cout) of the launch. */
typedef struct gt_wgrad_job {
  const void* X; const void* dY; float* part; float* part_bias;
  int32_t ldx, ldy, R, Cin, Cout, co_begin, co_count, slab_rows;
} gt_wgrad_job;
typedef struct gt_wgrad_tile { int32_t job, co0, ci0, slab; } gt_wgrad_tile;
typedef struct gt_wnb_job {
  const float* part; const float* part_bias; const float* v; const float* g; const float* inv_norm;
  float* dv; float* dg; float* dbias;
  int32_t S, Cout, Cin, taps, row_start, accumulate, pad0_, pad1_;
} gt_wnb_job;
int gt_conv_wgrad_batched(const void* jobs_device, const void* tiles_device, int n_tiles5, int n_tiles3,
                          int n_tiles1, void* stream);
int gt_weightnorm_bwd_batched(const void* jobs_device, int n_jobs, int total_rows, int max_row_elems, void* stream);

/* Paired form of the batched weight gradient for taps 5 and 3: one 512-thread workgroup computes two 128 x 64 tiles of one (job, slab)
 * from one staged copy of the operand rows they share.  Jobs are gt_wgrad_job as above; partials are bit-identical to
 * gt_conv_wgrad_batched over the same tiles.
 *   pair, kind 0: tiles (co0, ci0) and (co0, ci0 + 64) share the dY rows; with ci0 + 64 >= Cin it is the single tile (co0, ci0).
 *   pair, kind 1: tiles (co0, ci0) and (co0 + 128, ci0) share the X rows; with co0 + 128 >= co_count it is the single tile (co0, ci0).
 *   pairs are ordered taps 5, then 3; every tile of a job's grid must be covered exactly once. */
typedef struct gt_wgrad_pair { int32_t job, co0, ci0, slab, kind, pad0_, pad1_, pad2_; } gt_wgrad_pair;
int gt_conv_wgrad_paired(const void* jobs_device, const void* pairs_device, int n_pairs5, int n_pairs3, void* stream);

/* out[n] += sum_m Y[m,n]  (bias gradients); Y bf16 (is_f32 == 0) or fp32 rows. */
int gt_colsum(const void* Y, int ldy, int is_f32, float* out, int R, int N, void* stream);

/* commons.squeeze / unsqueeze (commons.py:339-364) fused with the [B,C,T] <-> rows layout change.
 * len_sq[b] = valid squeezed frames; Tp = Ty/2 + 2*GT_HALO; C <= 80.  Each is the other's backward. */
int gt_squeeze_rows_f32(const float* y, float* rows, const int32_t* len_sq, int B, int C, int Ty, int Tp,
                        const int32_t* row0, void* stream);
int gt_unsqueeze_rows_f32(const float* rows, float* y, const int32_t* len_sq, int B, int C, int Ty, int Tp,
                          const int32_t* row0, void* stream);

/* ActNorm data-dependent initialisation (ActNorm.initialize, modules.py:607-619) on the rows layout: from the rows x
 * [R, C] fp32 the layer is about to see (rows outside an utterance are zero) and the valid frame counts len[B]:
 *   m = sum x / sum len, v = sum x^2 / sum len - m^2, logs = -0.5 log(max(v, 1e-6)), bias = -m * exp(logs).
 * workspace: 2*C doubles (cleared here).  One-off (first batch of a run with ddi=true, configs/base.json:13). */
int gt_actnorm_ddi(const float* x, const int32_t* len, int B, int R, int C, double* workspace, float* logs, float* bias,
                   void* stream);

/* ActNorm (modules.py:584-599) + InvConvNear (modules.py:635-665) fused, rows layout fp32 [R,C]:
 *   y = (W_4x4 applied per group {2g,2g+1,C/2+2g,C/2+2g+1} to (bias + exp(logs)*x)) * mask
 *   logdet[b] += (sum(logs) + (C/4)*logdet(W)) * len[b]          (when logdet != NULL)
 * gt_flow_scalars precomputes scal[18] = {sum logs, logdet W, W^-T}.  y0_bf16 (optional) receives
 * a bf16 copy of the first C/2 channels (the coupling's start-conv input). */
int gt_flow_scalars(const float* logs, int C, const float* W, float* scal, void* stream);
/* the same for n (ActNorm, InvConvNear) pairs in one launch: logs_ptrs / w_ptrs are DEVICE arrays of n device pointers,
 * scal is [n][18] */
int gt_flow_scalars_multi(const void* logs_ptrs, const void* w_ptrs, int C, float* scal, int n, void* stream);
int gt_actnorm_invconv_fwd(const float* x, float* y, void* y0_bf16, int ld0, const float* logs, const float* bias,
                           const float* W, const float* scal, const float* rowmask, const int32_t* len,
                           float* logdet, int B, int R, int C, void* stream);
/* dlogs/dbias/dW are ACCUMULATED into (zero them first). */
int gt_actnorm_invconv_bwd(const float* x, const float* dy, float* dx, const float* logs, const float* bias,
                           const float* W, const float* scal, const float* rowmask, const int32_t* len,
                           const float* dlogdet, float* dlogs, float* dbias, float* dW, int B, int R, int C, void* stream);

/* Affine coupling (attentions.py:174-186): out = [m|logs] fp32 rows from the `end` conv.
 *   z = [x0 | (m + exp(logs)*x1)*mask],  logdet[b] += sum(logs*mask). */
int gt_coupling_fwd(const float* out, const float* x, float* z, const float* rowmask, float* logdet,
                    int B, int R, int C, int Tp, const int32_t* row0, int sigmoid_scale, void* stream);
int gt_coupling_bwd(const float* out, const float* x, const float* dz, const float* dlogdet, const float* rowmask,
                    float* dx, void* dout_bf16, int B, int R, int C, int Tp, const int32_t* row0, int sigmoid_scale,
                    void* stream);

/* WaveNet gate backward (commons.py:61-68): dpre [R,2*half] bf16 from d(acts), saved T and S;
 * dpre carries the replayed dropout mask, dpre_cond (optional) does not. */
int gt_gate_bwd(const void* dacts, int ldd, const void* T, const void* S, int ldts, void* dpre, int ldp, void* dpre_cond,
                int R, int half, float drop_p, uint32_t drop_seed, const uint32_t* seed_dev, void* stream);

/* backward of y = rowmask * dropout(relu(c)) given the saved y: dc = (y != 0) ? d/(1-p) : 0 (bf16 rows). */
int gt_relu_drop_bwd(const void* d, int ldd, const void* y, int ldy, void* dc, int ldc, int R, int n, float drop_p, void* stream);

/* small row helpers */
int gt_rows_add_bf16(float* dx, int ldx, const void* add, int lda, int R, int n, void* stream);
int gt_rows_f32_to_bf16(const float* in, int ldi, void* out, int ldo, const float* rowmask, int R, int n, void* stream);

/* Channel LayerNorm of the text encoder / predictors on rows (modules.py:26-44, eps 1e-4), with the
 * surrounding elementwise work fused (attentions.py:79-84, modules.py:95-102, models.py:598-607):
 *   s = a (fp32, optional) + dropout_in(y (bf16, optional));  n = LN(s)*gamma + beta;
 *   o = dropout_out(relu?(n)) * rowmask;  out_f32 / out_bf16 (either optional).  C <= 256.
 * Dropout masks are counter-based (seed) and replayed by the backward. dgamma/dbeta ACCUMULATE.
 * gt_layernorm_bwd: relu bit 0 = the forward's relu flag; bit 1 (value 2) = y is itself a ReLU's output (conv -> relu -> norm,
 * models.py:591-598): dy is zeroed where y == 0, so the ReLU's backward needs no launch of its own. */
int gt_layernorm_fwd(const float* a, const void* y, int ldy, const float* gamma, const float* beta, const float* rowmask,
                     float* out_f32, void* out_bf16, int ldo, float* mean, float* rstd, int R, int C, float eps,
                     float p_in, uint32_t seed_in, float p_out, uint32_t seed_out, int relu, const uint32_t* seed_dev, void* stream);
int gt_layernorm_bwd(const float* a, const void* y, int ldy, const float* gamma, const float* beta, const float* rowmask,
                     const float* mean, const float* rstd, int R, int C, float eps,
                     float p_in, uint32_t seed_in, float p_out, uint32_t seed_out, int relu, const uint32_t* seed_dev,
                     const float* dout_f32, const void* dout_bf16, int lddo,
                     float* da, void* dy, int lddy, float* dgamma, float* dbeta, void* stream);
/* The same backward without atomics: one row per wave, the dgamma | dbeta sums of workgroup w go to row w of partials
 * [gt_layernorm_bwd_partial_rows(R)][2 C]; gt_param_partials_reduce then ADDS the column sums of up to GT_PARTIALS_MAX such
 * buffers [n_rows][Ca + Cb] to their destinations dst_a[Ca] / dst_b[Cb] in one launch (at the end of a module's backward). */
int gt_layernorm_bwd_partial_rows(int R);
int gt_layernorm_bwd_partials(const float* a, const void* y, int ldy, const float* gamma, const float* beta, const float* rowmask,
                              const float* mean, const float* rstd, int R, int C, float eps,
                              float p_in, uint32_t seed_in, float p_out, uint32_t seed_out, int relu, const uint32_t* seed_dev,
                              const float* dout_f32, const void* dout_bf16, int lddo,
                              float* da, void* dy, int lddy, float* partials, void* stream);
#define GT_PARTIALS_MAX 32
typedef struct gt_partials_job { const float* partials; float* dst_a; float* dst_b; int32_t n_rows, Ca, Cb, pad_; } gt_partials_job;
typedef struct gt_partials_args { gt_partials_job job[GT_PARTIALS_MAX]; int32_t n_jobs; } gt_partials_args;
int gt_param_partials_reduce(const gt_partials_args* args, void* stream);

/* Relative-position multi-head self-attention (attentions.py:241-336) in its banded form:
 *   score[i,j] = (q_i.k_j + [|j-i|<=win] q_i.Ek[j-i+win]) / sqrt(D), masked keys/queries -> -1e4,
 *   out_i = sum_j dropout(softmax)[i,j] v_j + sum_{|j-i|<=win} dropout(softmax)[i,j] Ev[j-i+win].
 * q,k,v,out: bf16 rows [B*Tp, H*D]; Ek,Ev: [2*win+1, D] fp32 shared by heads; P: [B,H,T,T] fp32
 * (softmax before dropout, kept for the backward); workspace: gt_attn_bwd_workspace_bytes(B,T,H) bytes of
 * scratch, 16-byte aligned; dEk/dEv ACCUMULATE.  D = 96, win = 4: T <= 384 runs on bf16 MFMA (gt_attn_mfma_shape) and
 * 505 < T <= GT_ATTN_LONG_MAX_T on key-tiled bf16 MFMA kernels whose LDS and registers do not grow with T (gt_attn_long_shape);
 * the rest runs on the generic kernels, which hold an utterance-head in LDS: at D = 96, win = 4 the forward to T = 597, the
 * backward to T = 505 — GT_E_UNSUPPORTED past what fits, and for every T > GT_ATTN_LONG_MAX_T before anything is launched.
 * P and the workspace are each 4 B H T^2 bytes (4.3 GB at B = 32, H = 2, T = 4096); gt_attn_fwd_stats / gt_attn_bwd_stats below
 * train the key-tiled shapes with O(B H T) bytes instead.
 * gt_attn_fwd with P == NULL — a forward nobody differentiates (synthesis) — is taken when, and only when, gt_attn_long_shape(T, D,
 * win) holds: the key-tiled kernel then stores no P and writes the same `out`, bit for bit (strides / operand alignment that kernel
 * does not take: GT_E_ALIGN).  At every other shape a NULL P is GT_E_INVAL (T > GT_ATTN_LONG_MAX_T: GT_E_UNSUPPORTED comes first).
 * gt_attn_bwd always needs the P its forward stored.
 *   workspace   device scratch of at least gt_attn_bwd_workspace_bytes(B,T,H) bytes, 16-byte aligned; after gt_attn_bwd it
 *               holds what the call's second pass read (dS = P (dP - sum_j dP P) / sqrt(D), zero where masked):
 *               on the MFMA kernels (both families) bf16 dS^T [B,H,T(key j),TI(query i)], TI = ceil(T/32)*32, followed by dropout(P)^T in
 *               the same shape with the rows of queries i >= lens[b] zero, columns i >= T of both zero;
 *               on the generic kernels fp32 dS [B,H,T(query i),T(key j)].
 * Query rows i >= lens[b] contribute nothing to dk, dv, dEk and dEv (and get dq = 0) whatever dout holds there. */
int gt_attn_fwd(const void* q, const void* k, const void* v, int ld, const float* Ek, const float* Ev,
                const int32_t* lens, void* out, int ldo, float* P, int B, int T, int Tp, const int32_t* row0, int H, int D, int win,
                float drop_p, uint32_t drop_seed, const uint32_t* seed_dev, void* stream);
size_t gt_attn_bwd_workspace_bytes(int B, int T, int H);
/* 1 if gt_attn_fwd / gt_attn_bwd run a (T, D, win) shape on the T <= 384 MFMA kernels, 0 if not (the dispatchers' own test;
 * operands laid out as the rows layout leaves them) */
int gt_attn_mfma_shape(int T, int D, int win);
/* 1 if they run it on the key-tiled MFMA kernels: D == 96, win == 4, 505 < T <= GT_ATTN_LONG_MAX_T (the token limit of
 * gt_mas_long_f32).  Both directions switch at the same T, so a backward differentiates what its forward computed. */
#define GT_ATTN_LONG_MAX_T 4096
int gt_attn_long_shape(int T, int D, int win);
int gt_attn_bwd(const void* q, const void* k, const void* v, int ld, const float* Ek, const float* Ev,
                const int32_t* lens, const void* dout, int lddo, const float* P, void* workspace, size_t workspace_bytes,
                void* dq, void* dk, void* dv, int lddq, float* dEk, float* dEv,
                int B, int T, int Tp, const int32_t* row0, int H, int D, int win, float drop_p, uint32_t drop_seed,
                const uint32_t* seed_dev, void* stream);

/* The same attention at the key-tiled shapes without anything of size T^2 (opt-in; gt_attn_fwd / gt_attn_bwd are unchanged).
 * gt_attn_fwd_stats writes the `out` of gt_attn_fwd bit for bit, stores no P, and leaves two floats per query row:
 *   stats       [B, H, T, 2] fp32, 8-byte aligned, gt_attn_stats_bytes(B,T,H) = 8 B H T bytes: for query i of (b, h)
 *               stats[..., 0] = mx, the maximum over the keys of the masked, scaled scores, and stats[..., 1] = rden = 1 / sum_j
 *               exp(s[i,j] - mx), so that P[i,j] = exp(s[i,j] - mx) * rden is the forward's own P.  Every i < T is written, padded
 *               queries (i >= lens[b]) included.
 * gt_attn_bwd_stats recomputes P tile by tile from q, k, Ek and stats in both of its kernels; dq equals gt_attn_bwd's bit for bit on
 * the same operands, dk / dv / dEk / dEv round as gt_attn_bwd's do (bf16 dS and P' feed their MFMAs) and differ from them in fp32
 * summation order only.  dEk/dEv ACCUMULATE; query rows i >= lens[b] contribute nothing and get dq = 0; one writer per row as above.
 *   workspace   device scratch of at least gt_attn_bwd_stats_workspace_bytes(B,T,H) = 80 B H T bytes, 16-byte aligned; after the
 *               call it holds one record of 20 floats per query row, [B, H, T, 20]: [0] Dsum_i = sum_j dP P, [1..9] q_i . Ek[r],
 *               [10..18] dO_i . Ev[r] (Ek / Ev rounded to bf16, r = j - i + win), [19] zero.
 * Asynchronous, no allocation, no global state.  Refused before any launch, in this order: a NULL pointer (stats and workspace
 * included) or a non-positive B, T, H: GT_E_INVAL; T > GT_ATTN_LONG_MAX_T or any shape at which gt_attn_long_shape(T, D, win) is 0 (there
 * is no other kernel behind these entries), or drop_p >= 1: GT_E_UNSUPPORTED; workspace_bytes too small: GT_E_INVAL; strides or
 * operand alignment the kernels do not take (ld, lddo multiples of 8, ldo, lddq of 4; q, k, v, dout, workspace 16-byte aligned,
 * stats 8-byte): GT_E_ALIGN. */
size_t gt_attn_stats_bytes(int B, int T, int H);
size_t gt_attn_bwd_stats_workspace_bytes(int B, int T, int H);
int gt_attn_fwd_stats(const void* q, const void* k, const void* v, int ld, const float* Ek, const float* Ev,
                      const int32_t* lens, void* out, int ldo, float* stats, int B, int T, int Tp, const int32_t* row0, int H, int D, int win,
                      float drop_p, uint32_t drop_seed, const uint32_t* seed_dev, void* stream);
int gt_attn_bwd_stats(const void* q, const void* k, const void* v, int ld, const float* Ek, const float* Ev,
                      const int32_t* lens, const void* dout, int lddo, const float* stats, void* workspace, size_t workspace_bytes,
                      void* dq, void* dk, void* dv, int lddq, float* dEk, float* dEv,
                      int B, int T, int Tp, const int32_t* row0, int H, int D, int win, float drop_p, uint32_t drop_seed,
                      const uint32_t* seed_dev, void* stream);

/* Embedding * scale into rows (models.py:693): fp32 and/or bf16 output, zero halo / padded rows.  emb [n_vocab, C];
 * the rows have stride ld >= C (ld > C: the language embedding of models.py:698-699 fills channels [C, ld) — written by
 * gt_rows_add_cond on that column window); the backward ACCUMULATES into demb. */
int gt_embedding_fwd(const int64_t* ids, const float* emb, const int32_t* lens, float* out_f32, void* out_bf16,
                     int B, int T, int Tp, const int32_t* row0, int R, int C, int ld, float scale, void* stream);
int gt_embedding_bwd(const int64_t* ids, const float* dx, const int32_t* lens, float* demb,
                     int B, int T, int Tp, const int32_t* row0, int R, int C, int ld, float scale, void* stream);

/* Ragged rows layout (see GT_HALO above): from the row offsets row0[B+1] and the lengths, fill the per-row tables the
 * host side keeps next to them — rowbatch[m] (utterance of row m, int64), rowframe[m] (m - row0[b] - GT_HALO) and
 * rowmask[m] (1 on valid frames), rowutt[m] (optional int32 twin of rowbatch) — in one launch (a replayed HIP graph's contexts
 * are refreshed per batch). */
int gt_rows_ctx_fill(const int32_t* row0, const int32_t* lens, int64_t* rowbatch, int32_t* rowframe, float* rowmask, int32_t* rowutt,
                     int B, int R, void* stream);

/* Everything a replayed training step takes from its batch, in ONE launch (train.Trainer's graph replay; the reference's loop does
 * `x.cuda(rank, non_blocking=True)` per tensor, train_ms_emo_lang_pitch.py:286-300): up to GT_STEP_MAX_COPIES padded copies — rows of
 * src_words 4-byte words into rows of dst_words >= src_words words, the tail of every row zeroed — and up to GT_STEP_MAX_CTX ragged row
 * contexts: geo_src = row0[B+1] | lengths[B] as int32 (device or PINNED HOST memory: read directly by the kernel), copied to geo_dst
 * and expanded into gt_rows_ctx_fill's tables.  blk0 is filled in by the call. */
#define GT_STEP_MAX_COPIES 10
#define GT_STEP_MAX_CTX 3
#define GT_STEP_MAX_B 1024
typedef struct gt_step_copy { const void* src; void* dst; int32_t rows, src_words, dst_words, blk0; } gt_step_copy;
typedef struct gt_step_ctx {
  const int32_t* geo_src; int32_t* geo_dst; int64_t* rowbatch; int32_t* rowframe; float* rowmask; int32_t* rowutt;
  int32_t B, R, blk0, pad_;
} gt_step_ctx;
typedef struct gt_step_inputs_args {
  gt_step_copy copy[GT_STEP_MAX_COPIES]; gt_step_ctx ctx[GT_STEP_MAX_CTX]; int32_t n_copy, n_ctx;
} gt_step_inputs_args;
int gt_step_inputs(const gt_step_inputs_args* args, void* stream);
/* The head of a training step: up to GT_ZERO_MAX regions zeroed (16-byte aligned, sizes multiples of 16) and *seed_word += seed_inc
 * (optional), one launch. */
#define GT_ZERO_MAX 4
typedef struct gt_step_zero_args { void* ptr[GT_ZERO_MAX]; uint64_t bytes[GT_ZERO_MAX]; uint32_t* seed_word; uint32_t seed_inc; int32_t n; } gt_step_zero_args;
int gt_step_zero(const gt_step_zero_args* args, void* stream);

/* out[m,:] = (x[m,:] + cond[utterance(m),:]) * rowmask[m]: a per-utterance vector added to every valid row — the
 * speaker conditioning the reference broadcasts over time in attentions.py:66-67 (Encoder.cond_g, before layer index 2)
 * and models.py:587-589 (DurationPredictor.cond).  Source fp32 `x` (wins) or bf16 `xb`; cond [B,C] fp32; fp32 and/or
 * bf16 output (either may be NULL, in place allowed); halo / padded rows are written as zero.  The gradient of cond is
 * the per-utterance row sum of the output gradient (gt_rows_utt_sum). */
int gt_rows_add_cond(const float* x, int ldx, const void* xb, int ldxb, const float* cond, const float* rowmask,
                     float* out, int ldo, void* outb, int ldob, int B, int R, int C, int Tp, const int32_t* row0, void* stream);

/* out[b, :C] (+)= sum over the rows m of utterance b of y[m, :C] * rowmask[m] (rowmask NULL = 1): the gradient of a
 * per-utterance vector broadcast over time — gt_rows_add_cond's cond, and the speaker conditioning g_l that WN adds
 * inside the gate (modules.py:148-156).  y bf16 (is_f32 == 0) or fp32 rows; out [B, ldo] fp32; accumulate != 0 adds to
 * out.  No atomics: one workgroup per (utterance, 64 channels). */
int gt_rows_utt_sum(const void* y, int ldy, int is_f32, const float* rowmask, float* out, int ldo, int accumulate,
                    int B, int R, int C, int Tp, const int32_t* row0, void* stream);

/* log-likelihood lattice (models.py:1076-1082) on exact-fp32 MFMA: x_m, x_logs (NULL = 0): [B,C,Tx],
 * z: [B,C,Ty] -> logp [B,Tx,Ty] fp32. */
int gt_logp_f32(const float* x_m, const float* x_logs, const float* z, float* logp, int B, int C, int Tx, int Ty, void* stream);

/* Prior expansion models.py:1118-1119 as a gather by frame2token (from gt_mas_f32; -1 = padded frame) and its backward as
 * the segment sums over the frames of every token (deterministic: fixed summation order; Tx <= 16384, past 512 tokens with one
 * wave per workgroup and Tx floats of dynamic LDS; GT_E_UNSUPPORTED beyond). */
int gt_prior_expand(const float* x_m, const int32_t* frame2token, float* z_m, int B, int C, int Tx, int Ty, void* stream);
int gt_prior_expand_bwd(const float* dz_m, const int32_t* frame2token, float* dx_m, int B, int C, int Tx, int Ty, void* stream);

/* mle_loss pieces (commons.py:28-33): gt_mle_sums leaves GT_MLE_PARTS partial pairs (sum(logs), sum(exp(-2 logs)(z-m)^2)) in acc2 — one per
 * workgroup, plain stores, summed by gt_mle_finish; n == 0 is not refused: the launch leaves GT_MLE_PARTS zero pairs (z, m may then
 * be NULL), so gt_mle_finish gives -sum(logdet) / denom + 0.5 log(2 pi);
 * backward: dz = g e^{-2 logs}(z-m), dm = -dz, dlogs = g (1 - e^{-2 logs}(z-m)^2), g = *gscale (/ *gdenom when gdenom != NULL:
 * the loss's denominator stays on the device); dlogdet (optional, [B]) receives -g. */
#define GT_MLE_PARTS 2048      /* acc2 holds this many (sum logs, sum exp(-2 logs)(z-m)^2) partial pairs: 2 * GT_MLE_PARTS floats, all written */
int gt_mle_sums(const float* z, const float* m, const float* logs, float* acc2, size_t n, void* stream);
int gt_mle_bwd(const float* z, const float* m, const float* logs, const float* gscale, float* dz, float* dm, float* dlogs,
               size_t n, const float* gdenom, float* dlogdet, int B, void* stream);
/* commons.sequence_mask as floats: mask[b, t] = t < lengths[b] (lengths int32 or int64), [B, T] in one launch. */
/* dev (bench.py --marks): one lane writes the device wall clock (100 MHz) to *slot — a time mark at this point of `stream`, valid
 * inside a replayed HIP graph, where the profiler's serialisation would hide which branch is the critical one. */
int gt_mark(unsigned long long* slot, void* stream);
int gt_length_mask(const void* lengths, int is_int64, float* mask, int B, int T, void* stream);

/* mle_loss's scalar tail (commons.py:31-33) in one launch: out2[0] = (acc2[0] + 0.5 acc2[1] - sum logdet) / denom + 0.5 log(2 pi),
 * out2[1] = denom = C * sum(mask) (acc2 from gt_mle_sums; mask: the n_mask floats of z_mask [B, 1, T]). */
int gt_mle_finish(const float* acc2, const float* logdet, const float* mask, int n_mask, int B, int C, float* out2, void* stream);
/* Duration loss of the deterministic predictor (models.py:1089-1092): l_length[b] = sum_t (logw[b,t] - log(w[b,t] + 1e-8) * mask)^2
 * / sum(mask), logw / w fp32 [B, Tx] (w = MAS durations), mask from x_lengths; backward: dlogw = g[b] * 2 (logw - logw_) / sum(mask). */
int gt_duration_loss_fwd(const float* logw, const float* w, const int32_t* x_lengths, int B, int Tx, float* l_length, void* stream);
int gt_duration_loss_bwd(const float* logw, const float* w, const int32_t* x_lengths, const float* g, int B, int Tx, float* dlogw, void* stream);

/* The alignment -> loss chain of a training step in three launches; every output is bit-identical to the chain of entries above
 * (gt_prior_expand, gt_mle_sums, gt_mle_finish, gt_duration_loss_fwd; gt_mle_bwd, gt_prior_expand_bwd, gt_duration_loss_bwd).
 * gt_align_loss_fwd: z [B,C,Ty], x_m (x_logs, NULL = mean_only) [B,C,Tx], frame2token [B,Ty] (-1 = padded frame) -> z_m (z_logs with
 *   x_logs) [B,C,Ty] and the GT_MLE_PARTS partial pairs in acc2; with logw and w ([B,Tx]; both or neither) and x_lengths also
 *   l_length [B].  GT_E_ALIGN: Ty % 4 != 0, or z / z_m / z_logs / frame2token off a 16-byte boundary; GT_E_UNSUPPORTED: Tx > 512 or
 *   B C Ty >= 2^31; nothing is written then (the callers go on with the unfused entries).
 * gt_align_loss_finish: out4[0] = mle loss, out4[1] = its denominator (both as gt_mle_finish), out4[2] = sum_b l_length[b] in the
 *   order ATen's sum gives a contiguous fp32 vector of B < 128 elements (l_length NULL: 0), out4[3] = out4[0] + out4[2].
 * gt_align_loss_bwd: with g = *gscale / *gdenom: dz = g e^{-2 z_logs}(z - z_m), dx_m = segment sums of -dz, dx_logs (with z_logs) =
 *   segment sums of g (1 - e^{-2 z_logs}(z - z_m)^2), dlogdet[b] = -g, and with logw / w: dlogw = *gscale * 2 (logw - logw_) /
 *   sum(mask).  One launch; Tx <= 512 (GT_E_UNSUPPORTED past it). */
int gt_align_loss_fwd(const float* z, const float* x_m, const float* x_logs, const int32_t* frame2token, const float* logw, const float* w,
                      const int32_t* x_lengths, float* z_m, float* z_logs, float* acc2, float* l_length, int B, int C, int Tx, int Ty,
                      void* stream);
int gt_align_loss_finish(const float* acc2, const float* logdet, const float* mask, int n_mask, const float* l_length, int B, int C,
                         float* out4, void* stream);
int gt_align_loss_bwd(const float* z, const float* z_m, const float* z_logs, const int32_t* frame2token, const float* logw, const float* w,
                      const int32_t* x_lengths, const float* gscale, const float* gdenom, float* dz, float* dx_m, float* dx_logs,
                      float* dlogdet, float* dlogw, int B, int C, int Tx, int Ty, void* stream);

/* [B, C, T] <-> rows at the public boundary (fp32 or bf16 on either side: *_f32 = 1 / 0), one launch each:
 *   gt_rows_from_bct: rows[m, c] = x[b, c, t] for the frame rows of utterance b (row base(b) + HALO + t, 0 <= t < T), 0 elsewhere;
 *   gt_bct_from_rows: x[b, c, t] = rows[base(b) + HALO + t, c] for t < lengths[b], 0 beyond.  row0 == NULL: uniform layout. */
int gt_rows_from_bct(const void* x, int x_f32, void* rows, int rows_f32, const int32_t* row0, int B, int C, int T, int Tp, int R, void* stream);
int gt_bct_from_rows(const void* rows, int rows_f32, void* x, int x_f32, const int32_t* lengths, const int32_t* row0,
                     int B, int C, int T, int Tp, int R, void* stream);

/* Reverse (inference) direction of the flows — models.py:765-785 with reverse=True.
 *   gt_actnorm_invconv_rev: x = ((W^-1 y) * mask - bias) * exp(-logs) * mask  (InvConvNear^-1 then ActNorm^-1,
 *     modules.py:647-652,592-594); scal from gt_flow_scalars (holds W^-T); x0_bf16 (optional) = bf16(x[:, :C/2]).
 *   gt_coupling_rev: x = [z0 | (z1 - m) * exp(-logs) * mask] with [m | logs] = out (attentions.py:178-180). */
int gt_actnorm_invconv_rev(const float* y, float* x, void* x0_bf16, int ld0, const float* logs, const float* bias,
                           const float* scal, const float* rowmask, int R, int C, void* stream);
int gt_coupling_rev(const float* out, const float* z, float* x, const float* rowmask, int R, int C,
                    int sigmoid_scale, void* stream);

/* AdamW over flat fp32 buffers (parameters, gradients, both moments are slices of four buffers of n floats,
 * n % 4 == 0, 16-B aligned) — replaces torch.optim.AdamW.step + commons.clip_grad_value_(params, None)
 * (train_ms_emo_lang_pitch.py:311-312, commons.py:320-336).  hyper (device) = {lr, beta1, beta2, eps,
 * weight_decay, step} with step >= 1 already counting this update; *gnorm_sq (optional, device, caller zeroes
 * it) += sum g^2. */
int gt_adamw_flat(float* p, const float* g, float* m, float* v, size_t n, const float* hyper,
                  float* gnorm_sq, void* stream);

/* ---- A whole WaveNet (all gated layers of modules.WN.forward, modules.py:144-171, without the final skip sum) as ONE kernel
 * (csrc/wn_stack.hip): a workgroup recomputes the 2-row halo every k = 5 layer needs instead of exchanging it — 64 rows computed
 * per layer, gt_wn_stack_rows_per_workgroup(n_layers) = 64 - 4 (n_layers - 1) rows owned and stored.  Same arithmetic, dropout
 * hash and outputs as n_layers calls of gt_wn_layer_fwd (bit-identical).  H = 192, taps = 5, n_layers <= 4; weight images as
 * for gt_wn_layer_fwd; cond: [B, >= 2H n] per utterance (B > 0, row0 / Tp as elsewhere) or [R, >= 2H n] per row (B == 0),
 * layer i reads columns [2H i, 2H (i+1)); dropout seed of layer i is drop_seed + i (^ *seed_dev). */
typedef struct gt_wn_stack_fwd_args {
  const void* x0;                               /* bf16 [R, H]: the WaveNet's input (masked) */
  const void* w_in[4]; const float* b_in[4];    /* in_layer images (flags 2 | 4 | 16) and biases [2H] */
  const void* w_res[4]; const float* b_res[4];  /* residual 1x1 images and biases [H] of layers 0 .. n_layers-2 */
  const float* cond; int ldc; const int32_t* row0; int B; int Tp;
  const float* rowmask;
  void* acts; int ldacts;                       /* out: bf16 [R, >= n_layers * H], layer i in columns [H i, H (i+1)) */
  void* gate_t[4]; void* gate_s[4];             /* out: bf16 [R, H] per layer (saved tanh / sigmoid halves) */
  void* x_out[4];                               /* out: x_out[i] = input of layer i+1, bf16 [R, H], i < n_layers-1 */
  /* gate_t / gate_s / x_out are what a BACKWARD reads.  All of them NULL (every layer): the kernel stores acts only — the
   * synthesis direction, where they are 2/3 of the launch's writes; acts is bit-identical either way.  Needs drop_p == 0 and no
   * affine conditioning (aff_*) (GT_E_UNSUPPORTED otherwise); a mix of NULL and non-NULL among them is GT_E_INVAL. */
  int R, H, taps, n_layers;
  float drop_p; uint32_t drop_seed; const uint32_t* seed_dev;
  unsigned long long* stamps; int stamp_slot; const int32_t* stamp_base;   /* as gt_wn_layer_fwd */
  /* optional, instead of cond: AFFINE per-frame conditioning of modules.WNP (modules.py:316-343, 353-362) formed in the kernel:
   * cond[m, 2H i + c] = aff_b[off + c] + aff_sig[m, par] * aff_w[off + c] with O = H n_layers, par = (2H i) / O, off = (2H i) % O
   * (n_layers even) — aff_w / aff_b: fp32 [O] (cond_layer1's weight-normed weight and bias), aff_sig: fp32 [R, 2] = the contour
   * at frames 2 m and 2 m + 1 of squeezed row m */
  const float* aff_w; const float* aff_b; const float* aff_sig;
} gt_wn_stack_fwd_args;
/* gradient of the affine conditioning's parameters from the d pre rows of the WaveNet's layers (dpre_c of gt_wn_stack_bwd, or dpre
 * where no dropout is applied): dw[off_i + c] += sum_m dpre_i[m, c] aff_sig[m, par_i], db[off_i + c] += sum_m dpre_i[m, c]
 * (par_i, off_i as above; fp32 [H n_layers] accumulators the caller zeroes; dpre_i: bf16 [R, lddp >= 2H]) */
int gt_cond_affine_grads(const void* dpre0, const void* dpre1, const void* dpre2, const void* dpre3, int lddp, const float* sig,
                         float* dw, float* db, int R, int H, int n_layers, void* stream);
int gt_wn_stack_rows_per_workgroup(int n_layers);
/* 32-row (1) or 64-row (2) blocks per tile that gt_wn_stack_fwd (fwd = 1) / gt_wn_stack_bwd (fwd = 0) choose for R rows */
int gt_wn_stack_row_blocks(int R, int n_layers, int fwd);
int gt_wn_stack_fwd(const gt_wn_stack_fwd_args* args, void* stream);
/* gt_wn_stack_bwd: the data-gradient chain of the same WaveNet in one launch (what n_layers - 1 calls of gt_wn_layer_bwd, the
 * bottom call without a second stage and gt_gate_bwd for the top layer compute; bit-identical):
 *   d pre_{n-1} = gate backward of via_skip[:, H (n-1) ..] (the top layer has no residual output);
 *   for j = n-1 .. 0:  dx[j] = (conv_k5^T(d pre_j; w_in_d[j]) + dx[j+1]) * rowmask;
 *                      j > 0:  d acts_{j-1} = dx[j] @ W_res_{j-1} (w_res_d[j-1]) + via_skip[:, H (j-1) ..];  d pre_{j-1} = gate backward.
 * dx[0] is the gradient at the WaveNet's input; dpre_c[i] (optional) = d pre_i before the dropout mask (gradient of the cond
 * term).  via_skip: bf16 [R, >= n H]; dpre / dpre_c: bf16 [R, 2H]; dx: bf16 [R, H]. */
typedef struct gt_wn_stack_bwd_args {
  const void* via_skip; int ldvs;
  const void* gate_t[4]; const void* gate_s[4];
  const void* w_in_d[4];                        /* data-gradient images of the in_layers (flag 4) */
  const void* w_res_d[4];                       /* data-gradient images of the residual 1x1s, layers 0 .. n_layers-2 */
  const float* rowmask;
  void* dpre[4]; void* dpre_c[4]; void* dx[4];
  int R, H, taps, n_layers;
  float drop_p; uint32_t drop_seed; const uint32_t* seed_dev;
} gt_wn_stack_bwd_args;
int gt_wn_stack_bwd(const gt_wn_stack_bwd_args* args, void* stream);

/* ---- Everything between two WaveNets of the flow decoder as ONE kernel (csrc/wn_boundary.hip): all of it is row-local.
 * Shapes: C = 160 flow channels (n_sqz * 80 mels), H = 192, n_layers = 4 (every reference config); 64 rows per workgroup.
 * Weight images: gt_pack_conv_weights(_multi) in MFMA-fragment order (flags 2 | 4), ks_* = padded K / 16 of each image.
 *
 * gt_wn_boundary_fwd — [tail of block b] when acts != NULL:
 *     wn_out = (acts @ Wskipcat^T + b_skip) * mask       modules.py:168-171 (K-concatenated skip GEMM, bf16 out, kept for wgrad)
 *     [m | logs] = wn_out @ Wend^T + b_end               attentions.py:162-165
 *     z = [y0 | (m + exp(logs) * y1) * mask], logdet[utt] += sum logs * mask      attentions.py:171-184; logs_raw [R, C/2] kept
 *   [head of block b+1] when y_next != NULL (input: the z tile, or x_in [R, C] when there is no tail):
 *     y_next = InvConvNear(ActNorm(z)) * mask, logdet[b] += (sum an_logs + C/4 * logdet W) * len[b]    modules.py:584-599, 635-665
 *     y0_bf16 = bf16(y_next[:, :C/2]);  h_next = (y0 @ Wstart^T + b_start) * mask                      attentions.py:147
 * gt_wn_boundary_bwd — [head of block b+1] when dh != NULL:
 *     d y = [dx_in[:, :C/2] + dh @ Wstart | dx_in[:, C/2:]];  ActNorm / InvConvNear backward against x (their input):
 *     d_an_logs, d_an_bias, d_w_ic accumulated with atomics (+ the log-det terms), d x -> the tile (or dx_out without a tail)
 *   [tail of block b] when dout != NULL (input: that tile, or dz_in [R, C] when there is no head):
 *     dx_out = [d z0 | d z1 * exp(logs) * mask];  dout = bf16 [d m | d logs] (kept for wgrad)
 *     dwn_out = (dout @ Wend) * mask (bf16, kept for wgrad);  via_skip [R, n_layers * H] = dwn_out @ Wskipcat
 * A NULL pointer selects the variant; everything is fp32 rows [R, C] unless said otherwise; rowutt int32 [R]. */
typedef struct gt_boundary_fwd_args {
  /* tail */
  const void* acts; int ldacts;                 /* bf16 [R, >= n_layers*H] gated activations of the block's WN */
  const void* w_skip; const float* b_skip;      /* forward image of the skip-cat GEMM [H, n_layers*H]; bias = sum of skip biases */
  const void* w_end; const float* b_end; int ks_end;
  const float* y;                               /* [R, C]: this block's ActNorm+InvConv output (y0 | y1) */
  void* wn_out;                                 /* out: bf16 [R, H] */
  float* logs_raw;                              /* out: [R, C/2] fp32 (before sigmoid_scale) */
  float* z;                                     /* out: [R, C] */
  float* logdet; const int32_t* rowutt; int sigmoid_scale;
  /* head */
  const float* x_in;                            /* head-only variant: the flow state [R, C] */
  const float* an_logs; const float* an_bias; const float* w_ic; const float* scal; const int32_t* len; int B;
  float* y_next; void* y0_bf16;                 /* out: [R, C] fp32, bf16 [R, C/2] */
  const void* w_start; const float* b_start; int ks_start;
  void* h_next;                                 /* out: bf16 [R, H] */
  const float* rowmask; int R, H, C, n_layers;
  /* optional: commons.squeeze / unsqueeze (commons.py:339-364) folded into the first / last launch of the pass —
   * y_bct (head-only variant, instead of x_in): the decoder's input [B, C/2, T] fp32 (z, if given, then receives the squeezed rows); z_bct (tail-only variant, instead of z): its
   * output [B, C/2, T] fp32, pre-zeroed by the caller; rowbatch (int64) / rowframe (int32): gt_rows_ctx_fill's tables; len as above */
  const float* y_bct; float* z_bct; int T; const int64_t* rowbatch; const int32_t* rowframe;
  /* optional: up to 16 buffers (16-byte aligned, pf_bytes[i] % 16 == 0, pf_ptr[i] == NULL ends the list) that 64 EXTRA workgroups of
   * the launch read once, on CUs the 64-row tiles leave idle — the weight images of the WaveNet launch that follows on the chain,
   * which would otherwise take their first touch (HBM) inside it */
  const void* pf_ptr[16]; uint32_t pf_bytes[16];
} gt_boundary_fwd_args;
typedef struct gt_boundary_bwd_args {
  /* head */
  const void* dh;                               /* bf16 [R, H]: masked gradient at the WN's input */
  const void* w_start_d; int ks_start_d;
  const float* dx_in;                           /* [R, C]: [d z0 | d y1] of this block (dx_out of the previous launch) */
  const float* x;                               /* [R, C]: input of this block's ActNorm */
  const float* an_logs; const float* an_bias; const float* w_ic; const float* scal; const int32_t* len; int B;
  float* d_an_logs; float* d_an_bias; float* d_w_ic;   /* accumulators [C], [C], [16] */
  /* tail */
  const float* dz_in;                           /* tail-only variant: gradient of the decoder's output rows [R, C] */
  const float* logs_raw; const float* y;        /* saved by the forward: [R, C/2], [R, C] */
  const float* dlogdet; const int32_t* rowutt; int sigmoid_scale;
  float* dx_out;                                /* out: [R, C] */
  void* dout;                                   /* out: bf16 [R, C] */
  const void* w_end_d; int ks_end_d;
  void* dwn_out;                                /* out: bf16 [R, H] */
  const void* w_skip_d; int ks_skip_d;
  void* via_skip; int ldvs;                     /* out: bf16 [R, >= n_layers*H] */
  const float* rowmask; int R, H, C, n_layers;
  /* optional, as in the forward: dz_bct (tail-only variant, instead of dz_in) and dx_bct (head-only variant, instead of dx_out;
   * pre-zeroed) are [B, C/2, T] fp32 */
  const float* dz_bct; float* dx_bct; int T; const int64_t* rowbatch; const int32_t* rowframe;
  /* optional (head): one row of gt_boundary_param_partials() floats per workgroup of the launch (ceil(R / 64) rows) — the
   * workgroup's sums for d_an_logs | d_an_bias | d_w_ic are STORED there instead of added to the three accumulators with atomics
   * (152 workgroups on the same 336 addresses serialise at L2: ~10 us of a 33 us launch); gt_boundary_param_reduce adds the rows up */
  float* pg_partial;
  const void* pf_ptr[16]; uint32_t pf_bytes[16];  /* optional prefetch list, as in the forward */
} gt_boundary_bwd_args;
int gt_wn_boundary_fwd(const gt_boundary_fwd_args* args, void* stream);
int gt_wn_boundary_bwd(const gt_boundary_bwd_args* args, void* stream);
/* floats per workgroup row of pg_partial, and the reduction over rows for n_blocks launches at once: partials
 * [n_blocks][n_wg][gt_boundary_param_partials()], dst = DEVICE array of 3 * n_blocks pointers {d_an_logs, d_an_bias, d_w_ic} per block;
 * every destination element gets += the sum over the block's n_wg rows (modules.py:584-599, 635-665 parameter gradients) */
int gt_boundary_param_partials(void);
/* gt_wn_boundary_rev — the same for the REVERSE (synthesis) direction, models.py:765-785 with reverse=True: everything between the
 * WaveNet of block b and the WaveNet of block b-1 as one launch.  No log-det, nothing kept for a backward: wn_out, [m | logs] and
 * x0 stay in LDS; HBM receives the fp32 flow state x and the bf16 rows h_next only.
 *   [tail of block b] when acts != NULL (acts = gt_wn_stack_fwd's gated activations of block b's last WaveNet):
 *     wn_out = bf16((acts @ Wskipcat^T + b_skip) * mask)                         modules.py:168-171
 *     [m | logs] = wn_out @ Wend^T + b_end;  sigmoid_scale: logs = log(1e-6 + sigmoid(logs + 2))      attentions.py:162-165, 172-173
 *     u = [z0 | (z1 - m) * exp(-logs) * mask]                                    attentions.py:178-180 (as gt_coupling_rev)
 *     x = ((W^-1 u) * mask - an_bias) * exp(-an_logs) * mask                     modules.py:647-652, 592-594 (as gt_actnorm_invconv_rev;
 *                                                                                scal = the block's gt_flow_scalars, holds W^-T)
 *   [head of block b-1] when h_next != NULL (input: the x tile, or x_in / z_bct when there is no tail):
 *     x0 = bf16(x[:, :C/2]);  h_next = bf16((x0 @ Wstart^T + b_start) * mask)    attentions.py:147
 * A pass over n blocks is n + 1 launches: head-only (block n-1's start conv), n - 1 with both halves, tail-only (block 0).
 * Same contract as the forward: plain device pointers, asynchronous on the stream, no allocation, rows of either layout.
 * GT_E_INVAL on a NULL required pointer or a shape other than H = 192, C = 160, n_layers = 4; GT_E_ALIGN on a pointer that is
 * not 16-byte aligned.  Rows whose rowmask is 0 come out as zero in x and h_next. */
typedef struct gt_boundary_rev_args {
  /* tail */
  const void* acts; int ldacts;                 /* bf16 [R, >= n_layers*H] gated activations of block b's (last) WaveNet */
  const void* w_skip; const float* b_skip;      /* fragment-ordered forward image of the skip-cat GEMM; bias = sum of skip biases */
  const void* w_end; const float* b_end; int ks_end;
  const float* z;                               /* [R, C]: the flow state at block b's output (x of the previous launch) */
  int sigmoid_scale;
  const float* an_logs; const float* an_bias;   /* block b's ActNorm parameters [C] */
  const float* scal;                            /* block b's flow scalars [18] (gt_flow_scalars): scal[2 ..] = W^-T */
  float* x;                                     /* out: [R, C] the flow state at block b's input (optional with x_bct) */
  /* head */
  const float* x_in;                            /* head-only variant: the flow state [R, C] */
  const void* w_start; const float* b_start; int ks_start;   /* block b-1's start conv */
  void* h_next;                                 /* out: bf16 [R, H] */
  const float* rowmask; int R, H, C, n_layers;
  /* optional: commons.squeeze / unsqueeze folded into the first / last launch of the pass (T even) — z_bct (head-only variant,
   * instead of x_in): the decoder's input [B, C/2, T] fp32, x then receives the squeezed rows; x_bct (tail-only variant, instead
   * of or besides x): its output [B, C/2, T] fp32, pre-zeroed by the caller; rowbatch (int64) / rowframe (int32): gt_rows_ctx_fill's
   * tables; len: int32 [B] squeezed lengths */
  const float* z_bct; float* x_bct; int T; const int64_t* rowbatch; const int32_t* rowframe; const int32_t* len;
  const void* pf_ptr[16]; uint32_t pf_bytes[16];  /* optional prefetch list (the next WaveNet's weight images), as in the forward */
} gt_boundary_rev_args;
int gt_wn_boundary_rev(const gt_boundary_rev_args* args, void* stream);
int gt_boundary_rev_args_size(void);            /* sizeof(gt_boundary_rev_args): lets a binding check its mirror of the struct */
int gt_boundary_param_reduce(const float* partials, int n_wg, int n_blocks, float* const* dst, void* stream);

/* ---- One WaveNet layer as ONE kernel (modules.WN.forward, one loop iteration, modules.py:151-170; csrc/wn_layer.hip).
 * H = 192 hidden channels, k = 5, dilation 1; a workgroup owns 64 rows and all channels, so the 1x1 residual conv runs on the
 * gated tile the k=5 conv just produced (and, in the backward, the gate backward on the tile the data gradient just produced).
 * Weights are images of gt_pack_conv_weights in MFMA-FRAGMENT order (flags 2 / 4) with Np == N, Kp == K exactly; the in_layer's
 * forward image also carries the block-granular gate interleave (flag 16).  A wave loads its own fragments L2 -> registers.
 *
 * gt_wn_layer_fwd:  x_in = drop(conv_k5(x) + bias_in) + cond;  T = tanh(x_in[:H]), S = sigmoid(x_in[H:]), acts = T*S
 *                   (acts / T / S bf16 rows out, as gt_conv_gemm_bf16 gate == 1 writes them; same dropout hash);
 *                   w_res_frag != NULL:  x_next = (x + acts @ W_res^T + bias_res) * rowmask     (rows [0,H) of res_skip_i)
 * gt_wn_layer_bwd:  dX = (conv_k5^T(dpre_next) + resid) * rowmask  -> dx [R, H]   (data gradient of the NEXT layer's in_layer,
 *                   resid = gradient arriving at that layer's output through the residual path, NULL for the top layer);
 *                   w_res_dgrad_frag != NULL:  d acts = dX @ W_res + via_skip;  dpre = gate backward of (T, S) with the forward's
 *                   dropout replayed, [R, 2H] = [d tanh-half | d sigmoid-half];  dpre_c (optional): the same before the dropout
 *                   mask (the gradient of the conditioning term, which is added after the dropout).  NULL: dx only (bottom layer).
 * stamps (optional, bench.py): device uint64 pairs [2*slot] = min start / [2*slot+1] = max end of the launch in
 * wall_clock64() ticks (100 MHz) — the kernel's duration inside a replayed HIP graph; init to ~0 / 0;
 * slot = stamp_slot + *stamp_base (stamp_base: optional device int32 the step bumps, so every replay fills fresh slots). */
int gt_wn_layer_fwd(const void* x, int ldx, const void* w_in_frag, const float* bias_in,
                    const float* cond, int ldc, const int32_t* row0, int B, int Tp, const float* rowmask,
                    void* acts, int ldacts, void* gate_t, void* gate_s, int ldts,
                    const void* w_res_frag, const float* bias_res, void* x_next, int ldxn,
                    int R, int H, int taps, float drop_p, uint32_t drop_seed, const uint32_t* seed_dev,
                    unsigned long long* stamps, int stamp_slot, const int32_t* stamp_base, void* stream);
int gt_wn_layer_bwd(const void* dpre_next, int lddn, const void* w_in_dgrad_frag, const void* resid, int ldres,
                    const float* rowmask, void* dx, int lddx, const void* w_res_dgrad_frag,
                    const void* via_skip, int ldvs, const void* gate_t, const void* gate_s, int ldts,
                    void* dpre, void* dpre_c, int lddp, int R, int H, int taps, float drop_p, uint32_t drop_seed,
                    const uint32_t* seed_dev, unsigned long long* stamps, int stamp_slot, const int32_t* stamp_base, void* stream);

/* ---- Stochastic duration / pitch / energy predictors (models.py:217-481, modules.py:683-819,
 * transforms.py:12-202) on the rows layout.  C = 192 (filter_channels = in_channels, models.py:223).  `utt` is the
 * int32 utterance index of every row ([R]); rows with rowmask == 0 are zero on input and on output.  Gradient outputs
 * named d<param> ACCUMULATE (atomics); `acc` / `gacc` are per-utterance [B] accumulators of the negative log-likelihood
 * and their incoming gradient.
 *
 * DilatedDepthSeparableConv layer i (modules.py:726-734), dilation = kernel_size^i, kernel_size = 3:
 *   gt_dds_sep_fwd:  a1 = gelu(LayerNorm2(dwconv_d(x) + b))                -> bf16x3 rows [R, 3C], operand of the split 1x1 GEMM
 *   gt_dds_out_fwd:  out = (x + dropout(gelu(LayerNorm2(h2)))) * mask       h2 = 1x1 conv output incl. bias (fp32 rows)
 *   gt_dds_out_bwd:  dy -> d h2 (bf16x3 rows [R, 3C]), d gamma2 / d beta2
 *   gt_dds_sep_bwd:  d a1 (fp32, from the 1x1 data-gradient GEMM) -> d h1, d gamma1 / d beta1   (h1 recomputed from x)
 *   gt_dds_dw_bwd:   dx = (dy + dwconv_d^T(d h1)) * mask, d w [C,3], d b [C] */
/* bf16x3 operand layout for a split GEMM (gt_pack_conv_weights flag 8): out[m] = [hi | hi | lo] of in[m, :C]
 * (in fp32: hi = bf16(x), lo = bf16(x - hi); in bf16: lo = 0), out bf16 [R, ldo >= 3C], rows masked by rowmask if given.
 * gt_dds_sep_fwd's a1 and gt_dds_out_bwd's d h2 are written in this layout directly (lda / row pitch 3C). */
int gt_rows_split3(const void* in, int ldi, int is_f32, void* out, int ldo, const float* rowmask, int R, int C, void* stream);
int gt_dds_sep_fwd(const float* x, int ldx, const float* w, const float* b, const float* gamma, const float* beta,
                   const int32_t* utt, const float* rowmask, void* a1_bf16, int lda, int R, int C, int dilation, float eps, void* stream);
int gt_dds_out_fwd(const float* h2, const float* x, int ldx, const float* gamma, const float* beta, const float* rowmask,
                   float* out, void* out_bf16, int R, int C, float eps, float drop_p, uint32_t seed, const uint32_t* seed_dev, void* stream);
/* The three backward kernels accumulate their parameter gradients with one atomic per address and workgroup — or, with `partials`
 * (then the gradient pointers may be NULL), store the workgroup's sums to row w of partials [gt_dds_bwd_partial_rows(R)][W], W = 2 C
 * (gamma | beta) for out / sep, 4 C (dw[C][3] | db[C]) for dw; gt_param_partials_reduce adds the column sums later.
 * gt_dds_bwd_partial_rows(R) = ceil(R / 8) (one row per workgroup of 8 rows), 0 for R <= 0.
 *
 * Refusals of gt_rows_split3 and the five gt_dds_* entries (tests/test_dds_ops_cabi.py), all before any launch.  GT_E_INVAL first:
 * a required pointer NULL (optional: rowmask of gt_rows_split3, out_bf16, seed_dev, and dgamma / dbeta / dw / db when `partials` is
 * given; without `partials` both gradient pointers of a backward are required), R <= 0, dilation <= 0 (sep_fwd, sep_bwd, dw_bwd),
 * lda < 3 C (sep_fwd), ldo < 3 C or C <= 0 (gt_rows_split3), drop_p outside [0, 1) (out_fwd, out_bwd).  Then GT_E_UNSUPPORTED for
 * C != 192 (the gt_dds_* entries; gt_rows_split3 takes any C > 0).  ldx and ldi are not checked: a row of x / in starts every ldx /
 * ldi elements and only its first C are read. */
int gt_dds_bwd_partial_rows(int R);
int gt_dds_out_bwd(const float* h2, const float* dy, const float* gamma, const float* beta, const float* rowmask,
                   void* dh2_bf16, float* dgamma, float* dbeta, float* partials, int R, int C, float eps, float drop_p, uint32_t seed,
                   const uint32_t* seed_dev, void* stream);
int gt_dds_sep_bwd(const float* x, int ldx, const float* w, const float* b, const float* gamma, const float* beta,
                   const int32_t* utt, const float* rowmask, const float* da1, float* dh1, float* dgamma, float* dbeta,
                   float* partials, int R, int C, int dilation, float eps, void* stream);
int gt_dds_dw_bwd(const float* x, int ldx, const float* dh1, const float* dy, const float* w, const int32_t* utt,
                  const float* rowmask, float* dx, float* dw, float* db, float* partials, int R, int C, int dilation, void* stream);

/* The same layer as ONE launch per direction (csrc/dds_layer.hip): a workgroup owns gt_dds_layer_tile_rows() (64)
 * consecutive rows, keeps a1 / d h2 in LDS as a bf16 hi / lo pair and runs the split 1x1 product on the MFMA units itself.  Same
 * arithmetic as the five kernels above (fp32 row work, bf16x3 product with fp32 accumulation, the same dropout hash of
 * (seed ^ *seed_dev, row, channel)); only the summation order of the 1x1 product differs.  Each direction pairs with the other path's.
 *   gt_dds_layer_fwd:  x -> a1 (bf16x3 rows [R, lda >= 3C] = [hi | hi | lo], saved), h2 (fp32 [R, C], saved, = gt_conv_gemm_bf16's
 *                      output incl. bias), out = (x + dropout(gelu(LayerNorm2(h2)))) * mask (fp32 [R, C]) and, unless NULL,
 *                      out_split3 = gt_rows_split3(out) (bf16x3 rows [R, ldo3 >= 3C]).  Masked rows: a1 = out = 0, h2 = b1x1.
 *                      w1x1_split: the forward image of gt_pack_conv_weights flag 8 (row-major [>= C][Kp], Kp >= 3C).
 *   gt_dds_layer_bwd:  dy -> d h2 (its bf16 hi part, rows [R, lddh >= C]: the operand of the deferred weight / bias gradient),
 *                      d h1 (fp32 [R, C]: gt_dds_dw_bwd's input), d gamma2 / d beta2 / d gamma1 / d beta1.  h1 is recomputed from x.
 *                      w1x1_dgrad_split: the data-gradient image of flag 8 ([>= C][Kp], Kp >= 3C).
 *                      Parameter gradients: one atomic per address and workgroup, or with `partials` (then the four gradient
 *                      pointers may be NULL) plain stores into partials [gt_dds_layer_partial_rows(R)][2C]: with
 *                      n = gt_dds_layer_partial_rows(R) / 2 workgroups, row w < n is workgroup w's [d gamma2 | d beta2] and row
 *                      n + w its [d gamma1 | d beta1] — two buffers of the form gt_param_partials_reduce takes, back to back.
 *   gt_dds_dw_bwd follows gt_dds_layer_bwd unchanged (dx[m] needs d h1[m +- d] across tiles).
 * Refusals, before any launch and in this order: a NULL required pointer GT_E_INVAL; C != 192, dilation not a power of 3
 * (1, 3, 9, ...; <= 0 included) or R <= 0 GT_E_UNSUPPORTED; drop_p outside [0, 1) GT_E_INVAL; ldx < C, lda < 3C, ldo3 < 3C with
 * out_split3, lddh < C, Kp < 3C, Kp % 8 != 0 or an image that is not 16-byte aligned GT_E_ALIGN.
 * gt_dds_layer_partial_rows(R) = 2 ceil(R / 64), 0 for R <= 0. */
int gt_dds_layer_tile_rows(void);
int gt_dds_layer_partial_rows(int R);
int gt_dds_layer_fwd(const float* x, int ldx, const float* w_sep, const float* b_sep, const float* gamma1, const float* beta1,
                     const void* w1x1_split, int Kp, const float* b1x1, const float* gamma2, const float* beta2,
                     const int32_t* utt, const float* rowmask, void* a1_bf16, int lda, float* h2, float* out,
                     void* out_split3, int ldo3, int R, int C, int dilation, float eps, float drop_p, uint32_t seed,
                     const uint32_t* seed_dev, void* stream);
int gt_dds_layer_bwd(const float* x, int ldx, const float* w_sep, const float* b_sep, const float* gamma1, const float* beta1,
                     const void* w1x1_dgrad_split, int Kp, const float* gamma2, const float* beta2,
                     const int32_t* utt, const float* rowmask, const float* h2, const float* dy, void* dh2_bf16, int lddh,
                     float* dh1, float* dgamma2, float* dbeta2, float* dgamma1, float* dbeta1, float* partials,
                     int R, int C, int dilation, float eps, float drop_p, uint32_t seed, const uint32_t* seed_dev, void* stream);

/* ConvFlow (modules.py:792-819), in_channels = 2, on z rows [R, 2]:
 *   gt_convflow_pre_fwd:    x0 = (w_pre * z[:,0] + b_pre + g1 (+ g2)) * mask          (pre + DDSConv's `x = x + g`)
 *   gt_convflow_pre_bwd:    dx0 -> d w_pre, d b_pre, dz[:,0] += sum_c dx0 w_pre, dg += dx0      (dz / dg may be NULL)
 *   gt_convflow_spline_fwd: params = (Wp h + bp) * mask ([R,32], 29 used); z_out = [z0, RQS(z1)] * mask, channels swapped when
 *                           flip (the torch.flip after every ConvFlow, models.py:317-318); acc[utt] += sign * log|det|
 *   gt_convflow_spline_bwd: dz_out, gacc -> dh, d Wp [29,C], d bp [29], dz_in
 *   gt_convflow_spline_inv: synthesis direction (transforms.py:152-180): z_out = [z0, RQS^-1(z1)] * mask
 * The spline is transforms.piecewise_rational_quadratic_transform with 10 bins, linear tails, tail_bound 5. */
int gt_convflow_pre_fwd(const float* z, int ldz, const float* w_pre, const float* b_pre, const float* g1, const float* g2,
                        const float* rowmask, float* out, int R, int C, void* stream);
int gt_convflow_pre_bwd(const float* dx0, const float* z, int ldz, const float* w_pre, const float* rowmask,
                        float* dw_pre, float* db_pre, float* dz, int lddz, float* dg, int R, int C, void* stream);
int gt_convflow_spline_fwd(const float* h, const float* Wp, const float* bp, const float* z_in, const float* rowmask,
                           const int32_t* utt, float* z_out, float* params, float* acc, float sign, int flip, int R, int C, void* stream);
/* partials (optional; then dWp / dbp may be NULL): row w of [gt_convflow_spline_partial_rows(R)][gt_convflow_spline_partial_width()]
 * receives workgroup w's d Wp [29][C] | d bp [29] sums instead of atomics (gt_param_partials_reduce adds them up). */
int gt_convflow_spline_partial_rows(int R);
int gt_convflow_spline_partial_width(void);
int gt_convflow_spline_bwd(const float* h, const float* Wp, const float* params, const float* z_in, const float* dz_out,
                           const float* gacc, const float* rowmask, const int32_t* utt, float* dh, float* dWp, float* dbp,
                           float* partials, float* dz_in, float sign, int flip, int R, int C, void* stream);
int gt_convflow_spline_inv(const float* h, const float* Wp, const float* bp, const float* z_in, const float* rowmask,
                           float* z_out, int R, int C, void* stream);

/* ElementwiseAffine (modules.py:750-756) on [R,2]: y = (x * exp(log_scale) + translation) * mask (reverse: the inverse),
 * acc[utt] += sign * (log_scale_0 + log_scale_1) per valid row (acc may be NULL). */
int gt_ea_fwd(const float* x, const float* log_scale, const float* translation, const float* rowmask, const int32_t* utt,
              float* y, float* acc, float sign, int reverse, int R, void* stream);
int gt_ea_bwd(const float* x, const float* log_scale, const float* dy, const float* gacc, const float* rowmask, const int32_t* utt,
              float* dx, float* dlog_scale, float* dtranslation, float sign, int R, void* stream);

/* StochasticDurationPredictor between its posterior flows and its flows (models.py:299-311): z_q = [z_u, z_v], durations w [R],
 * noise e_q [R,2] -> z = [log(max(w - sigmoid(z_u), 1e-5)), z_v];  acc[utt] += -0.5 (2 log 2pi + |e_q|^2)
 * - (logsigmoid(z_u) + logsigmoid(-z_u)) + z[:,0].   gt_nll_gauss_*: acc[utt] += 0.5 (2 log 2pi + |z|^2) (models.py:321, 395, 469). */
int gt_sdp_mid_fwd(const float* z_q, const float* w, const float* e_q, const float* rowmask, const int32_t* utt, float* z, float* acc,
                   int R, void* stream);
int gt_sdp_mid_bwd(const float* z_q, const float* w, const float* dz, const float* gacc, const float* rowmask, const int32_t* utt,
                   float* dz_q, int R, void* stream);
int gt_nll_gauss_fwd(const float* z, const float* rowmask, const int32_t* utt, float* acc, int R, void* stream);
int gt_nll_gauss_bwd(const float* z, const float* gacc, const float* rowmask, const int32_t* utt, float* dz, int R, void* stream);

/* x_feature = x @ attn (models.py:1094) for the hard MAS path: frame row m of utterance b takes the token row
 * frame2token[b, t] (bf16 rows, C % 8 == 0); *_x describe the text-side rows, *_f the frame-rate rows.  Rows with rowmask_f == 0
 * are written as zeros and read neither frame2token nor x_rows.  The kernel moves 16 bytes per thread:
 *   GT_E_INVAL  a NULL x_rows / frame2token / utt_f / rowmask_f / out, R_f <= 0, C <= 0, C % 8 != 0, ldx % 8 != 0, ldx < C;
 *   GT_E_ALIGN  x_rows or out not 16-byte aligned. */
int gt_rows_gather_tokens(const void* x_rows, int ldx, const int32_t* frame2token, int Ty, const int32_t* row0_x, int Tp_x,
                          const int32_t* utt_f, const int32_t* row0_f, int Tp_f, const float* rowmask_f, void* out, int R_f, int C,
                          void* stream);

/* ---- Device front end of synthesis (FlowGenerator.infer with set_synthesis_front; csrc/synth_front.hip).
 * Vector stores only, no atomics, one writer per output element: deterministic.
 *
 * The Gaussian generator (csrc/common.h randn_key / randn_pair; all arithmetic mod 2^32, hash_u32 = the dropout hash):
 *   key(seed, stream, b) = hash_u32(hash_u32(seed) + b * 0x9E3779B1 + stream * 0x85EBCA6B)
 *   h1 = hash_u32(key + s * 0x9E3779B1 + c * 0x85EBCA6B),  h2 = hash_u32(h1 + 0x632BE5AB)
 *   u1 = ((h1 >> 9) + 0.5) * 2^-23,  u2 likewise from h2;  r = sqrt(-2 ln u1),  e0 = r cos(2 pi u2),  e1 = r sin(2 pi u2)
 * stream: 0 prior, 1 duration predictor, 2 pitch predictor, 3 energy predictor.
 *
 * gt_synth_lengths: dur [B, Tx] fp32 = ceil(w), integer valued (tokens i >= x_len[b] count as 0, a duration is clamped to
 *   [0, 2^20]) -> cum [B, Tx] int32 inclusive scan, y_len [B] int32 = max(sum, 1) (models.py:1189), and optionally
 *   logw [B, Tx] = log(1e-8 + dur) * (i < x_len[b]) (models.py:1199).  Tx <= 512, else GT_E_UNSUPPORTED.  B == 0 returns 0.
 *
 * gt_synth_prior: models.py:1196-1201 + commons.squeeze.  Frame t of utterance b belongs to the first token i < x_len[b] with
 *   cum[b, i] > t (commons.generate_path, zero-duration tokens included), to none when t >= sum(dur) or t >= y_len[b];
 *   z[b, c, t] = x_m[b, c, i] + exp(x_logs[b, c, i]) * e * noise_scale,  e = e0 (t even) / e1 (t odd) of (seed, stream 0, b, s = t / 2, c)
 *   rows [R, 2 C] fp32: rows[r, j * C + c] = z[b, c, 2 s + j] for the row r of squeezed frame s < y_len[b] / 2 (an odd trailing
 *   frame is dropped); EVERY one of the R rows is written, halo / padding / rounding rows as zeros.  row0 (int32 [B + 1]) = the
 *   ragged layout's row offsets, NULL = uniform rows (R == B * Tp); Tp as in RowsCtx (>= the rows of the largest utterance).
 *   Optional outputs (NULL-able), over all Ty frames, zero where no token owns the frame: z_m / z_logs [B, C, Ty] (z_logs = 0 when
 *   x_logs == NULL, the mean_only form), frame2token [B, Ty] int32 (-1 where no token owns the frame), attn [B, Tx, Ty] fp32.
 *   NULL args / required pointer: GT_E_INVAL;  R == 0 or B == 0: 0;  Tx > 512 or C > 80: GT_E_UNSUPPORTED;  fp32 pointers not
 *   16-byte aligned: GT_E_ALIGN.
 *
 * gt_randn_rows: out [R, ncol] fp32 = scale * (e0 | e1 by the parity of col) of (seed, stream, b = 0, s = row, c = col / 2).
 *
 * Texts of 513 .. GT_SYNTH_LONG_MAX_TX tokens: gt_synth_lengths_long / gt_synth_prior_long (and gt_synth_prior_long_call below) keep
 *   the contracts of gt_synth_lengths / gt_synth_prior / gt_synth_prior_call — outputs, masks, one writer per element, refusal codes —
 *   for every 1 <= Tx <= GT_SYNTH_LONG_MAX_TX (= GT_ATTN_LONG_MAX_T); Tx > GT_SYNTH_LONG_MAX_TX: GT_E_UNSUPPORTED before any launch.
 *   On Tx <= 512 they write what the short entries write, bit for bit, the noise included, with ONE difference: gt_synth_lengths_long
 *   clamps a token's duration to [0, 2^18] (4096 tokens then sum to at most 2^30, inside int32) where gt_synth_lengths clamps to
 *   [0, 2^20].  The short entries keep refusing Tx > 512. */
#define GT_SYNTH_LONG_MAX_TX 4096
typedef struct gt_synth_prior_args {
  const float* x_m; const float* x_logs;        /* [B, C, Tx] fp32; x_logs NULL = mean_only */
  const int32_t* cum;                           /* [B, Tx] gt_synth_lengths' scan */
  const int32_t* x_len; const int32_t* y_len;   /* [B] */
  const int32_t* row0; int Tp, R;               /* rows layout of the squeezed mel axis */
  float* rows;                                  /* out: [R, 2 C] */
  float* z_m; float* z_logs;                    /* optional out: [B, C, Ty] */
  int32_t* frame2token;                         /* optional out: [B, Ty] */
  float* attn;                                  /* optional out: [B, Tx, Ty] */
  int B, C, Tx, Ty;
  uint32_t seed; float noise_scale;
} gt_synth_prior_args;
int gt_synth_lengths(const float* dur, const int32_t* x_len, int32_t* cum, int32_t* y_len, float* logw, int B, int Tx, void* stream);
int gt_synth_prior(const gt_synth_prior_args* args, void* stream);
int gt_synth_lengths_long(const float* dur, const int32_t* x_len, int32_t* cum, int32_t* y_len, float* logw, int B, int Tx, void* stream);
int gt_synth_prior_long(const gt_synth_prior_args* args, void* stream);
int gt_synth_prior_args_size(void);             /* sizeof(gt_synth_prior_args) */
int gt_randn_rows(float* out, int R, int ncol, uint32_t seed, uint32_t stream_id, float scale, void* stream);

/* ---- Synthesis as one captured graph (FlowGenerator.compile_synthesis, glow-tts_amd/synthesis.py): nothing of a call
 * is baked into the launch sequence — the row geometry of the mel axis is built on the device from the predicted lengths, the call's
 * scalars are read from device memory, every size is a capacity.  Vector stores only, no atomics, one writer per element.
 *
 * gt_synth_geometry: y_len [B] int32 (gt_synth_lengths' output) + the capacities Ty_cap (frames, even) and R_cap (rows of the
 *   squeezed axis) -> everything a ragged rows context of the squeezed mel axis holds, in ONE launch: exactly
 *   RowsCtx.row_starts(lengths [v / 2], T = Ty_cap / 2) with starts[B] = R_cap, followed by gt_rows_ctx_fill:
 *     len_sq[b] = min(y_len[b], Ty_cap) / 2,   row0[0] = 0,   row0[b + 1] = row0[b] + len_sq[b] + 2 GT_HALO,   row0[B] = R_cap
 *     rowbatch [R_cap] int64 / rowframe / rowmask / rowutt (optional) as gt_rows_ctx_fill writes them: the rows behind the last
 *     utterance's frames belong to the last utterance and are masked.  y_len_eff [B] = the frame count gt_synth_prior[_call] must
 *     be given as y_len (min(y_len[b], Ty_cap); 2 len_sq[b] where the rows were cut).
 *   status (one int32): bit 0 = some y_len[b] > Ty_cap; bit 1 = the rows of the (frame-clipped) lengths do not fit R_cap.  With
 *   bit 1 the kernel stays inside its buffers: utterances are laid out in order, each keeps its two halos, and len_sq[b] is cut to
 *   what fits in front of the halos of the utterances behind it (possibly 0): row0[b] = min(unclipped row0[b], R_cap - 2 GT_HALO
 *   (B - b)).  row0 stays monotone, row0[b + 1] <= R_cap, len_sq[b] + 2 GT_HALO <= row0[b + 1] - row0[b], all R_cap table entries
 *   are written.  A non-zero status is a handled outcome: the caller discards the call's output (or takes the clipped one).
 *   B < 0, R_cap < 0, Ty_cap < 0 or odd: GT_E_INVAL;  B == 0 or R_cap == 0: 0;  B > GT_STEP_MAX_B or Ty_cap > 2^20:
 *   GT_E_UNSUPPORTED;  a NULL pointer other than rowutt, or R_cap < 2 GT_HALO B (no room for the halos): GT_E_INVAL;  int32 /
 *   fp32 pointers not 4-byte, rowbatch not 8-byte aligned: GT_E_ALIGN.
 *
 * gt_synth_call: the scalars of ONE synthesis call, in DEVICE memory (uploaded per call; a captured graph reads them at replay).
 * gt_synth_prior_call / gt_randn_rows_call: gt_synth_prior / gt_randn_rows — the same kernel code, bit-identical outputs — with
 *   seed and the scale taken from *call (args->seed / args->noise_scale are ignored; which_scale: 0 = noise_scale, 1 =
 *   noise_scale_w, anything else GT_E_INVAL).  length_scale is read by the host-side plumbing between the duration predictor and
 *   gt_synth_lengths.  call == NULL: GT_E_INVAL (behind the R == 0 / B == 0 returns);  not 4-byte aligned: GT_E_ALIGN. */
typedef struct gt_synth_call { uint32_t seed; float noise_scale; float noise_scale_w; float length_scale; } gt_synth_call;
int gt_synth_call_size(void);                   /* sizeof(gt_synth_call) */
int gt_synth_geometry(const int32_t* y_len, int B, int Ty_cap, int R_cap, int32_t* row0, int32_t* len_sq, int32_t* y_len_eff,
                      int64_t* rowbatch, int32_t* rowframe, float* rowmask, int32_t* rowutt, int32_t* status, void* stream);
int gt_synth_prior_call(const gt_synth_prior_args* args, const gt_synth_call* call, void* stream);
int gt_synth_prior_long_call(const gt_synth_prior_args* args, const gt_synth_call* call, void* stream);
int gt_randn_rows_call(float* out, int R, int ncol, const gt_synth_call* call, uint32_t stream_id, int which_scale, void* stream);

/* ---- Full-model synthesis: stochastic duration / pitch / energy predictors (csrc/synth_prosody.hip, csrc/synth_front.hip; DESIGN
 * 4.14).  Vector stores only, no atomics, one writer per element.
 *
 * gt_randn_keyed: the predictors' noise keyed by (utterance, token or frame) instead of by row index, so a draw does not depend on
 *   the rows layout.  Row r of out [R, ncol] fp32 belongs to utterance b and frame t = r - row0[b] - GT_HALO of the rows layout given
 *   as row0 (int32 [B + 1]; NULL = uniform rows, R == B * Tp) and Tp, as gt_synth_prior takes it:
 *     out[r, col] = scale * (e0 | e1 by the parity of col) of (seed, stream_id, b, s = t, c = col / 2)   for 0 <= t < lengths[b]
 *   and 0 on every other row (halo, padding, rounding): EVERY one of the R rows is written, the `* rowmask` is folded in.
 *   R < 0, B < 0, ncol <= 0: GT_E_INVAL;  R == 0: 0;  out / lengths NULL, B == 0, uniform rows with R != B * Tp: GT_E_INVAL;
 *   pointers not 4-byte aligned: GT_E_ALIGN;  R * ceil(ncol / 2) > 2^31 - 1: GT_E_UNSUPPORTED.
 * gt_synth_call_ext: gt_synth_call followed by the four scalars of the pitch / energy predictors, in DEVICE memory.  Its first 16
 *   bytes ARE a gt_synth_call: gt_synth_prior_call / gt_randn_rows_call take the same pointer.
 * gt_randn_keyed_call: gt_randn_keyed — the same kernel code, bit-identical output — with seed and the scale from *call
 *   (which_scale: 0 = noise_scale, 1 = noise_scale_w, 2 = f0_noise_scale, 3 = energy_noise_scale; anything else GT_E_INVAL;
 *   call == NULL: GT_E_INVAL behind the R == 0 return; not 4-byte aligned: GT_E_ALIGN).
 *
 * gt_synth_frame_geometry: the ragged rows context of the UN-squeezed mel axis (the frame rate the pitch / energy predictors run at)
 *   at capacity Rf_cap, from gt_synth_geometry's y_len_eff (<= Ty_cap): exactly RowsCtx.row_starts(y_len_eff, T = Ty_cap) with
 *   starts[B] = Rf_cap, followed by gt_rows_ctx_fill:  len_f[b] = min(y_len_eff[b], Ty_cap),  row0_f[b + 1] = row0_f[b] + len_f[b] +
 *   2 GT_HALO,  row0_f[B] = Rf_cap,  rowbatch / rowframe / rowmask / rowutt (optional) [Rf_cap].  Launched BEHIND gt_synth_geometry on
 *   the same stream: when the frame rows do not fit Rf_cap one thread ORs bit 2 (value 4) into *status, and gt_synth_geometry's
 *   overflow rule holds on whole frames — every utterance keeps its halos, len_f[b] is cut to what fits in front of the halos of
 *   the utterances behind it, row0_f[b] = min(unclipped row0_f[b], Rf_cap - 2 GT_HALO (B - b)), row0_f is monotone, all Rf_cap table
 *   entries are written.  Argument checks as gt_synth_geometry (Ty_cap may be odd); Rf_cap < 2 GT_HALO B: GT_E_INVAL.
 *
 * gt_synth_contours: the predictors' outputs on the frame-rate rows (pitch_rows / energy_rows [Rf] fp32, either may be NULL) ->
 *   pitch / energy [B, Ty] fp32 = rows[row of frame t] * scale for t < len_f[b], 0 behind it (the return tuple's contours), and
 *   psig / esig [R, 2] fp32 = the squeezed contour rows the reverse decoder's prosody WaveNets read: sig[r, j] = contour[b, 2 s + j]
 *   for the row r of squeezed frame s < min(len_sq[b], Ty / 2), 0 on every other row; all R rows are written.  One launch for what
 *   was from_rows -> * scale -> reshape -> gt_squeeze_rows_f32 per contour, bit-identical to it.  Both rows layouts are given as
 *   (row0, Tp) with row0 == NULL = uniform.  An output whose pointer is NULL is not written; an output whose input is NULL is zero.
 *   B == 0: 0;  len_f / len_sq NULL, a uniform layout whose B * Tp differs from its row count: GT_E_INVAL;  pointers not 4-byte
 *   (psig / esig: 8-byte) aligned: GT_E_ALIGN.  gt_synth_contours_call: the same kernel code with pitch_scale / energy_scale from *call. */
typedef struct gt_synth_call_ext { gt_synth_call base; float f0_noise_scale; float energy_noise_scale; float pitch_scale; float energy_scale; } gt_synth_call_ext;
int gt_synth_call_ext_size(void);               /* sizeof(gt_synth_call_ext) = 32 */
int gt_randn_keyed(float* out, const int32_t* row0, int Tp, const int32_t* lengths, int B, int R, int ncol, uint32_t seed,
                   uint32_t stream_id, float scale, void* stream);
int gt_randn_keyed_call(float* out, const int32_t* row0, int Tp, const int32_t* lengths, int B, int R, int ncol,
                        const gt_synth_call_ext* call, uint32_t stream_id, int which_scale, void* stream);
int gt_synth_frame_geometry(const int32_t* y_len_eff, int B, int Ty_cap, int Rf_cap, int32_t* row0_f, int32_t* len_f, int64_t* rowbatch,
                            int32_t* rowframe, float* rowmask, int32_t* rowutt, int32_t* status, void* stream);
int gt_synth_contours(const float* pitch_rows, const float* energy_rows, const int32_t* row0_f, int Tp_f, const int32_t* len_f, int Rf,
                      const int32_t* row0, int Tp, const int32_t* len_sq, int R, float* psig, float* esig, float* pitch, float* energy,
                      int B, int Ty, float pitch_scale, float energy_scale, void* stream);
int gt_synth_contours_call(const float* pitch_rows, const float* energy_rows, const int32_t* row0_f, int Tp_f, const int32_t* len_f,
                           int Rf, const int32_t* row0, int Tp, const int32_t* len_sq, int R, float* psig, float* esig, float* pitch,
                           float* energy, int B, int Ty, const gt_synth_call_ext* call, void* stream);

/* ---- device mel front end (csrc/mel_front.hip): waveforms -> log-mel, energy, magnitudes in one kernel ----------
 * The reference's TacotronSTFT.mel_spectrogram (commons.py:298-317, stft.py:78-101 CUDA branch) applied to every utterance of a
 * padded batch on its own, in exact fp32 (v_mfma_f32_32x32x2_f32).  Utterance b has F_b = 1 + wav_len[b] / 256 frames; frame f covers
 * samples 256 f - 512 .. 256 f + 511, indices outside [0, wav_len[b]) reflected about the utterance's own ends (edge not repeated);
 *   mag = sqrt(re^2 + im^2) [513 bins],  energy = ||mag||_2,  mel = logf(max(mel_basis mag, clip)),
 * and every output position f >= F_b is written as 0: all of mel [B, n_mel, F_max], energy [B, F_max] and mag [B, 513, F_max] (mag
 * may be NULL: not stored, the other two bit-identical) is defined.  No atomics; the summation order of an element depends on its
 * frame index alone, not on B, F_max or the row: a batch row is bit-identical to the utterance computed alone.
 *   wav      [B rows, pitch ld_wav elements] fp32 in [-1, 1], or int16 when is_i16 != 0 (scaled by 1/32768 in the kernel).
 *   wav_len  device int32 [B]; clamped to ld_wav.  wav_len <= 512 (no reflect padding exists) gives an unspecified result, but the
 *            reflected index is clamped: nothing outside the utterance's wav_len samples is read.  wav_len <= 0: all zeros.
 *   packed   gt_mel_pack_bytes() bytes written ONCE by gt_mel_pack from the reference's own buffers: basis = STFT.forward_basis
 *            (fp32 [2 * 513, 1024]: 513 real rows, then 513 imaginary rows, windowed) and mel_basis (fp32 [n_mel, 513]); the same
 *            n_mel goes to both calls.  The image folds every frame about its centre (K = 512), so the window must be symmetric
 *            about sample 512 with w[0] = 0 — the periodic Hann window of every reference config.
 * Supported: n_fft = win = 1024, hop = 256, n_mel <= GT_MEL_MAX_N_MEL; anything else GT_E_UNSUPPORTED before a launch.  NULL wav /
 * wav_len / packed / mel / energy, B outside [1, GT_MEL_MAX_B], F_max outside [1, GT_MEL_MAX_FRAMES], ld_wav <= 0, n_mel <= 0:
 * GT_E_INVAL.  Pointers not 16-byte (wav_len: 4-byte) aligned, ld_wav no multiple of 4: GT_E_ALIGN.
 * gt_mel_tile_frames: frames per workgroup (a tile past an utterance's end costs a zero fill). */
#define GT_MEL_MAX_N_MEL 128
#define GT_MEL_MAX_B 65535
#define GT_MEL_MAX_FRAMES 1048576
size_t gt_mel_pack_bytes(void);
int gt_mel_tile_frames(void);
int gt_mel_pack(const float* basis, const float* mel_basis, int n_fft, int n_mel, void* packed, void* stream);
int gt_mel_spectrogram(const void* wav, int is_i16, int ld_wav, const int32_t* wav_len, int B, int F_max,
                       const void* packed, int n_fft, int hop, int win, int n_mel, float clip,
                       float* mel, float* energy, float* mag, void* stream);

/* ---- device pitch front end (csrc/yin_front.hip): waveforms -> the YIN f0 contour in one kernel -----------------
 * The reference's yin.compute_yin (yin.py:70-119) as get_f0 calls it, applied to every utterance of a padded batch on its own, in
 * fp32 with direct differences.  Utterance b with L = wav_len[b] samples (clamped to ld_wav) has n_b = ceil((L - w_len) / hop)
 * analysis frames for L > w_len, else 0; frame i is samples hop i .. hop i + w_len - 1 (not centred, not reflected), and nothing at
 * or beyond index L is read.  Per frame
 *   d[t] = sum_{j = 0}^{w_len - 1 - t} (x[j] - x[j + t])^2  (t < tau_max),   c[0] = 1,  c[t] = d[t] t / sum_{1..t} d,
 *   p    = the first t in [tau_min, tau_max) with c[t] < thresh, then forward while t + 1 < tau_max and c[t + 1] < c[t]; 0 if none,
 * and at position lead + i of the [B, F_max] outputs
 *   f0 = sr / p (0 when p = 0),   harm = c[p] (min c when p = 0),   argmin_f0 = sr / argmin c if argmin c > tau_min, else 0.
 * Every other position (the first `lead`, everything from lead + n_b on) is written as 0; lead = 2 is get_f0's padding.  harm and
 * argmin_f0 may be NULL: not stored, f0 bit-identical.
 * ONE departure from the reference: a lag whose running sum of d is 0 (digital silence) gets c = 1 where the reference divides
 * 0 / 0 into NaN, so a silent frame is f0 = 0, argmin_f0 = 0, harm = 1.
 * Asynchronous, no allocation, no atomics, capturable in a graph; the summation order of an output depends on its (hop, lag) alone,
 * not on B, F_max or the tile: a batch row is bit-identical to the utterance computed alone.
 *   wav      [B rows, pitch ld_wav elements] fp32 in [-1, 1], or int16 when is_i16 != 0 (scaled by 1/32768 in the kernel).
 *   wav_len  device int32 [B].
 * Refusals, before any launch and in this order: NULL wav / wav_len / f0, B outside [1, GT_MEL_MAX_B], F_max outside
 * [1, GT_MEL_MAX_FRAMES], ld_wav <= 0, lead < 0, w_len <= 0, hop <= 0, tau_min < 1, tau_max <= tau_min, sr not > 0: GT_E_INVAL;
 * w_len != 1024, hop != 256 or tau_max > GT_YIN_MAX_TAU: GT_E_UNSUPPORTED; wav, f0, harm, argmin_f0 not 16-byte (wav_len: 4-byte)
 * aligned, ld_wav no multiple of 4: GT_E_ALIGN.
 * gt_yin_tile_frames: frames per workgroup (a tile past an utterance's end costs a zero fill). */
#define GT_YIN_MAX_TAU 512
int gt_yin_tile_frames(void);
int gt_yin_f0(const void* wav, int is_i16, int ld_wav, const int32_t* wav_len, int B, int F_max,
              int w_len, int hop, int tau_min, int tau_max, float sr, float thresh, int lead,
              float* f0, float* harm, float* argmin_f0, void* stream);

/* ---- device waveform back end (csrc/griffin_lim.hip): inverse STFT and the two halves of Griffin-Lim ------------
 * The reference's STFT.inverse (stft.py:121-148 CUDA branch) and griffin_lim (audio_processing.py:59-75) applied to every utterance
 * of a ragged batch on its own, in exact fp32 (v_mfma_f32_32x32x2_f32), n_fft = win = 1024, hop = 256, periodic Hann window.
 * Utterance b has F_b = n_frames[b] frames (clamped to F_max; F_b < 2: no sample, every output of the row is 0) and
 * L_b = 256 (F_b - 1) samples.  One Griffin-Lim run is gt_gl_polar, gt_istft, then n_iters x (gt_gl_project, gt_istft).
 *   spec     the complex spectrum Y of the batch, gt_gl_spec_bytes(B, F_max) bytes, in the fragment order gt_istft reads: per
 *            utterance [Fp / 32 frame groups][64 bin groups][64 lanes][re 4 | im 4] fp32 with lane = 32 (bin & 1) + (frame & 31),
 *            word = (bin & 7) >> 1, bin group = bin >> 3 for bins 0..511, then Re of bin 512 [Fp]; Fp = F_max rounded up to
 *            gt_gl_tile_frames().  Im of bins 0 and 512 is not kept (its inverse basis row is zero).  Both writers define all of
 *            it: zeros from frame F_b on.
 *   gt_gl_pack     once, from the reference's STFT.inverse_basis (fp32 [2 * 513, 1024]: pinv(4 fourier_basis).T times the window;
 *            it must be even (cos rows) / odd (sin rows) about sample 512 with column 0 zero, and row 0 the window / 4096 — the
 *            squared-window envelope is taken from it): gt_gl_pack_bytes() bytes.
 *   gt_gl_polar    spec = (mag cos(phase), mag sin(phase)), mag and phase fp32 [B, 513, F_max]: STFT.inverse's first line.
 *   gt_gl_project  the analysis half: frames of wav row b ([B rows, pitch ld_wav] fp32, L_b samples) reflected about the utterance's
 *            own ends as gt_mel_spectrogram takes them (F_b additionally clamped to 1 + ld_wav / 256; a reflected index is clamped
 *            into [0, L_b): nothing else is read), X = the folded DFT with the basis image of gt_mel_pack (mel_packed), and
 *            spec = mag X / |X| — the unit phasor instead of the reference's atan2 / cos / sin, the ONE departure from its
 *            arithmetic (the same mathematics); |X|^2 == 0 in fp32 gives (mag, 0), as atan2(0, 0) = 0 does.
 *   gt_istft       the synthesis half: per frame x = inverse_basis^T Y, overlap-added (4 frames per sample, ascending frame order),
 *            divided by the squared-window envelope (the sum of w^2 over the frames that really cover the sample, fp32, same order)
 *            where it exceeds FLT_MIN, times 1024 / 256, the 512 samples at both ends trimmed: wav row b ([B rows, pitch ld_wav])
 *            gets L_b samples and zeros behind them up to column 256 (F_max - 1); columns from there on are not written.
 * Asynchronous, no allocation, no atomics, capturable in a graph; the summation order of an element depends on its index within
 * its utterance alone, not on B, F_max or the tile: a batch row is bit-identical to the utterance computed alone.
 * Refusals, before any launch and in this order: a NULL pointer, B outside [1, GT_MEL_MAX_B], F_max outside
 * [1, GT_MEL_MAX_FRAMES], ld_wav <= 0, gt_istft's ld_wav < 256 (F_max - 1): GT_E_INVAL; n_fft != 1024, hop != 256 or
 * win != 1024: GT_E_UNSUPPORTED; a pointer not 16-byte (n_frames: 4-byte) aligned, ld_wav no multiple of 4: GT_E_ALIGN.
 * gt_gl_spec_bytes is 0 for a (B, F_max) the calls refuse.  gt_gl_tile_frames: frames per workgroup of gt_gl_project and gt_istft;
 * gt_gl_tile_hops: the output hops a gt_istft workgroup completes (its frames less a 3-frame halo). */
size_t gt_gl_pack_bytes(void);
int gt_gl_tile_frames(void);
int gt_gl_tile_hops(void);
size_t gt_gl_spec_bytes(int B, int F_max);
int gt_gl_pack(const float* inverse_basis, int n_fft, void* packed, void* stream);
int gt_gl_polar(const float* mag, const float* phase, const int32_t* n_frames, int B, int F_max, int n_fft, int hop, int win,
                float* spec, void* stream);
int gt_gl_project(const float* wav, int ld_wav, const float* mag, const int32_t* n_frames, int B, int F_max, const void* mel_packed,
                  int n_fft, int hop, int win, float* spec, void* stream);
int gt_istft(const float* spec, const int32_t* n_frames, int B, int F_max, const void* gl_packed, int n_fft, int hop, int win,
             float* wav, int ld_wav, void* stream);

/* ---- mel inversion in front of the loop (csrc/gl_mel.hip) ----------------------------------------------------------
 * gt_gl_from_mel: ragged log-mel -> linear magnitudes and the loop's initial spectrum in ONE launch; gt_istft follows it directly.
 *   mel      fp32 log-mel, element (b, k, f) at mel[b * stride_b + k * stride_c + f] (frames contiguous; strides in elements, each
 *            >= F_max).  Utterance b has F_b = min(max(n_frames[b], 0), F_max) frames; nothing at a frame >= F_b is read.
 *   mag      out [B, 513, F_max]: mag[b][j][f] = max(sum_k mel_pinv[j][k] expf(mel[b][k][f]), 0) for f < F_b, exactly 0 behind —
 *            ONE fp32 fmaf chain over k ascending per element (accurate expf): its bits depend on the utterance's data, j and f alone.
 *   spec     out, gt_gl_spec_bytes(B, F_max) bytes in the order described above, ALL of it defined (zeros from frame F_b on):
 *            mag (cos phi, sin phi) with phi = pi t, t = 2 u - 1, u = ((h >> 9) + 0.5) 2^-23,
 *            h = hash(key(seed, 4, b) + f * 0x9E3779B1 + j * 0x85EBCA6B) — the counter generator of the synthesis front end
 *            (gt_randn_keyed) on stream id 4; (sin, cos) = sincospif(t).  The phase is a function of (seed, b, f, j) alone.  Im of
 *            bin 0 is stored as gt_gl_polar stores it; Im of bin 512 is not kept.
 *   seed     by value, or (seed_dev != NULL) *seed_dev read on the device: a captured graph replays with the call's seed.
 * Asynchronous, no allocation, no atomics, capturable in a graph.
 * Refusals, before any launch and in this order: a NULL pointer other than seed_dev, B outside [1, GT_MEL_MAX_B], F_max outside
 * [1, GT_MEL_MAX_FRAMES], n_mel outside [1, GT_MEL_MAX_N_MEL], a stride below F_max (non-positive included): GT_E_INVAL; mag, spec or
 * mel_pinv not 16-byte, mel, n_frames or seed_dev not 4-byte aligned: GT_E_ALIGN. */
int gt_gl_from_mel(const float* mel, int64_t stride_b, int64_t stride_c, const int32_t* n_frames, int B, int F_max, int n_mel,
                   const float* mel_pinv, uint32_t seed, const uint32_t* seed_dev, float* mag, float* spec, void* stream);

/* ---- device sample-rate conversion (csrc/resample.hip): a rational-rate polyphase resampler for ragged batches ----
 * The definition of scipy.signal.resample_poly(x, up, down) with its default window ('kaiser', 5.0) and zero padding, applied to every
 * utterance of a padded batch on its own, in exact fp32.  (up, down) is reduced; half = 10 max(up, down); the prototype filter h has
 * 2 half + 1 taps (firwin(2 half + 1, 1 / max(up, down), window=('kaiser', 5.0)) * up); taps = ceil((2 half + 1) / up).  Utterance b
 * with L = wav_len[b] samples (clamped to [0, min(ld_wav, GT_RESAMPLE_MAX_LEN)]) has n_b = ceil(L up / down) outputs, and with
 * q = n down + half, p = q mod up, k0 = q div up
 *   out[b][n] = sum_{j = 0}^{taps - 1} bank[p][j] x[k0 - j],   x[k] = 0 outside [0, L)   (nothing at or beyond index L is read)
 * as ONE fmaf chain over j ascending.  Row b of out holds min(n_b, ld_out) samples and zeros behind them up to ld_out: every element
 * of [B, ld_out] is written.
 *   wav      [B rows, pitch ld_wav elements] fp32, or int16 when is_i16 != 0 (scaled by 1/32768 in the kernel).
 *   wav_len  device int32 [B].
 *   bank     fp32 [up, taps], bank[p][j] = h[p + j up] and 0 past the end of h: built on the host in float64 and rounded once.
 *   out_len  optional device int32 [B]: min(n_b, ld_out) — the wav_len of a gt_mel_spectrogram / gt_yin_f0 call that follows, with
 *            no host synchronisation.
 * Asynchronous, no allocation, no atomics, capturable in a graph; the summation order of an output depends on (n, up, down) alone,
 * not on B, ld_out, the tile or the row: a batch row is bit-identical to the utterance computed alone, an int16 input to its fp32
 * image.  n down + half is formed in 64 bits.
 * Supported: every reduced (up, down) whose bank (rows at the odd pitch taps | 1) plus the input span of one tile of
 * gt_resample_tile_out() outputs, (up - 1 + (tile - 1) down) div up + taps samples, fit 64 KB of LDS — each rounded up to 16 bytes;
 * gt_resample_lds_bytes(up, down) is that sum, gt_resample_taps(up, down) the taps per phase, both 0 for a pair that is refused (not
 * reduced, non-positive, or too large).
 * Refusals, before any launch and in this order: NULL wav / wav_len / bank / out, B outside [1, GT_MEL_MAX_B], ld_wav, ld_out, up,
 * down or taps <= 0: GT_E_INVAL; taps != ceil((20 max(up, down) + 1) / up): GT_E_INVAL; a pair gt_resample_taps refuses, or
 * ld_out > GT_RESAMPLE_MAX_OUT: GT_E_UNSUPPORTED; wav, bank, out not 16-byte (wav_len, out_len: 4-byte) aligned, ld_wav or ld_out no
 * multiple of 4: GT_E_ALIGN. */
#define GT_RESAMPLE_MAX_LEN 268435456
#define GT_RESAMPLE_MAX_OUT 1073741824
int gt_resample_tile_out(void);
int gt_resample_taps(int up, int down);
size_t gt_resample_lds_bytes(int up, int down);
int gt_resample(const void* wav, int is_i16, int ld_wav, const int32_t* wav_len, int B, const float* bank, int up, int down,
                int taps, float* out, int ld_out, int32_t* out_len, void* stream);

/* ---- HiFi-GAN generator (csrc/hifigan.hip): one dilated-convolution MFMA kernel for every layer --------------------
 * gt_voc_conv: a dilated 1-D convolution of a ragged batch on dense channels-last activations, bf16 operands, fp32 accumulation,
 * every utterance zero-padded at its own ends:
 *   Y[b, t, n] = epi( sum_{j < taps} sum_{ci < Cin} bf16( lrelu( X[b, t + (j - taps / 2) dil, ci] ) ) W[j][n][ci] )      t < len_b
 *   len_b = min(max(n_frames[b], 0) len_mul, L_cap).  A tap outside [0, len_b) contributes 0 and is never read (whatever lies there);
 *   Y at positions [len_b, L_cap) is written as 0; nothing beyond L_cap is touched.  The host never reads n_frames.
 *   X        fp32 (x_bf16 == 0) or bf16 [B, L_cap, Cin], element (b, t, c) at X[b x_stride_b + t Cin + c]; or, x_mel != 0 (fp32 only),
 *            the channel-major log-mel of the decoder, element (b, c, t) at X[b x_stride_b + c x_stride_c + t] (gt_gl_from_mel's form).
 *   lrelu    v < 0 ? v slope : v in fp32 (slope = 1: none), then round-to-nearest-even to bf16: that value is the MFMA operand.
 *   W        bf16 image in MFMA-fragment order, [taps][Np / 32][Kp / 16][64 lanes][8]: lane 32 h + r, element e holds
 *            W[j][32 nt + r][16 ks + 8 h + e], zeros for n >= N and ci >= Cin; Np = N rounded up to 32, Kp = Cin rounded up to
 *            gt_voc_k_chunk(Cin) (64 where 64 divides Cin, else 32).  Packed once per weight version by the caller.
 *   epi(s)   (s + bias[n] + res[b, t, n] + acc[b, t, n]) scale, then tanh when tanh_out != 0 (the kernels' fast tanh); res and acc
 *            are optional fp32 with Y's geometry.  Y is fp32 or bf16 (y_bf16), element (b, t, n) at Y[b y_stride_b + t ldy + n].
 *            Y may alias res and / or acc (each element is read and written by the same lane); Y may not alias X.
 * Asynchronous, no allocation, no atomics, capturable in a graph; the grid is sized by L_cap.  The summation order of an element
 * depends on (t, n, Cin, taps) alone: a batch row is bit-identical to the utterance computed alone, in a buffer of any capacity.
 * A workgroup owns gt_voc_tile_positions() positions and stages them plus (taps - 1) dil halo rows of one Cin chunk in
 * gt_voc_lds_bytes(Cin, taps, dil) bytes of LDS = (tile + (taps - 1) dil) (2 chunk + 16), at most 64 KB (0 for a shape that is refused).
 * Refusals, before any launch and in this order: args or X / W / bias / Y / n_frames NULL; B, L_cap, Cin, N, dil or len_mul <= 0; taps
 * <= 0 or even; ldy < N, y_stride_b < L_cap ldy; x_stride_b < L_cap Cin (x_mel: x_stride_b or x_stride_c < L_cap, or x_bf16 set);
 * Y == X: GT_E_INVAL.  taps > GT_VOC_MAX_TAPS, Cin no multiple of 16, B > 65535, B L_cap max(Cin, N) >= 2^31, a halo past the LDS
 * bound: GT_E_UNSUPPORTED.  W not 16-byte, bias / n_frames / Y / res / acc not 4-byte aligned, X not 16-byte aligned or x_stride_b no
 * multiple of 8 (x_mel: X not 4-byte aligned): GT_E_ALIGN. */
#define GT_VOC_MAX_TAPS 11
typedef struct gt_voc_conv_args {
  const void* X; int64_t x_stride_b; int64_t x_stride_c;
  const void* W; const float* bias; const float* res; const float* acc;
  void* Y; int64_t y_stride_b; int ldy;
  int len_mul; const int32_t* n_frames;
  int B; int L_cap; int Cin; int N; int taps; int dil;
  int x_bf16; int x_mel; int y_bf16; int tanh_out;
  float slope; float scale;
} gt_voc_conv_args;
int gt_voc_conv(const gt_voc_conv_args* args, void* stream);
int gt_voc_conv_args_size(void);                /* sizeof(gt_voc_conv_args): lets a binding check its mirror of the struct */
int gt_voc_tile_positions(void);
int gt_voc_k_chunk(int Cin);
size_t gt_voc_lds_bytes(int Cin, int taps, int dil);

/* ---- BigVGAN's anti-aliased snake activation (csrc/voc_snake.hip): one memory-bound kernel in front of gt_voc_conv ------
 * gt_voc_snake: Activation1d (2x up-sampling FIR -> snake -> 2x down-sampling FIR, per channel) of a ragged batch on dense channels-last
 * activations, fp32 in, bf16 out (the x_bf16 operand of the next gt_voc_conv), every utterance on its own [0, len_b):
 *   u[2q]   = 2 sum_{j < 6} fu[11 - 2j] x[cl(q - 3 + j)]      u[2q + 1] = 2 sum_{j < 6} fu[10 - 2j] x[cl(q - 2 + j)]      cl(i) = min(max(i, 0), len_b - 1)
 *   v[i]    = u[i] + ib[c] sin^2(a[c] u[i])
 *   Y[b, t, c] = bf16( sum_{k < 12} fd[k] v[min(max(2t + k - 5, 0), 2 len_b - 1)] )                                        t < len_b
 *   len_b = min(max(n_frames[b], 0) len_mul, L_cap).  x is replicated at the utterance's ends and so is v: v's INDEX is clamped, v is
 *   not evaluated outside [0, 2 len_b).  Nothing at or behind len_b is read (whatever lies there); Y at positions [len_b, L_cap) is
 *   written as bf16 zero; nothing beyond L_cap is touched.  The host never reads n_frames.
 *   X        fp32 [B, L_cap, C], element (b, t, c) at X[b x_stride_b + t C + c].
 *   Y        bf16 [B, L_cap, C], element (b, t, c) at Y[b y_stride_b + t C + c]; Y may not alias X.
 *   P        fp32 parameter block of 2 C + 24 values: [C] a = alpha', [C] ib = 1 / (beta' + 1e-9), [12] fu (the up-sampling filter),
 *            [12] fd (the down-sampling filter).  Built by the caller (exp of log-scale parameters, the reciprocal): the kernel evaluates
 *            no exp and no division.
 * Arithmetic is fp32: fmaf chains with j ascending for u and k ascending for y, sin by the device library's sinf, one rounding to
 * nearest even to bf16.  The order depends on (t, c) alone: a batch row is bit-identical to the utterance computed alone, in a buffer
 * of any capacity.  Asynchronous, no allocation, no atomics, no LDS, capturable in a graph; the grid is sized by L_cap: a workgroup
 * owns gt_voc_snake_tile_positions() positions x 32 channels, a thread a strip of 16 positions of two channels.
 * Refusals, before any launch and in this order: args or X / Y / P / n_frames NULL; B, L_cap, C or len_mul <= 0; x_stride_b or
 * y_stride_b < L_cap C; Y == X: GT_E_INVAL.  C no multiple of 16, B > 65535, B L_cap C >= 2^31: GT_E_UNSUPPORTED.  X not 16-byte, Y not
 * 8-byte, P or n_frames not 4-byte aligned, x_stride_b or y_stride_b no multiple of 8: GT_E_ALIGN. */
typedef struct gt_voc_snake_args {
  const float* X; int64_t x_stride_b;
  const float* P;
  void* Y; int64_t y_stride_b;
  int len_mul; const int32_t* n_frames;
  int B; int L_cap; int C;
} gt_voc_snake_args;
int gt_voc_snake(const gt_voc_snake_args* args, void* stream);
int gt_voc_snake_args_size(void);               /* sizeof(gt_voc_snake_args): lets a binding check its mirror of the struct */
int gt_voc_snake_tile_positions(void);

/* ---- Vocos vocoder (csrc/vocos.hip): the frame-rate ConvNeXt backbone's kernels and the iSTFT head's nonlinearity ----
 * One run of L blocks is gt_voc_conv (embedding, taps 7, x_mel), gt_vocos_norm, L x (gt_vocos_norm, gt_vocos_mlp), gt_vocos_norm,
 * gt_voc_conv (head Linear, taps 1, N = 1026), gt_vocos_polar, gt_istft: 6 + 2 L launches.
 * Shared by the three: activations are dense channels-last; len_b = min(max(n_frames[b], 0), L_cap), the host never reads n_frames;
 * nothing at or behind len_b is read (whatever lies there); outputs at [len_b, L_cap) are written as zero and nothing beyond L_cap is
 * touched; asynchronous, no allocation, no atomics, capturable in a graph, the grid sized by L_cap; the summation order of an element
 * depends on its position within its utterance and the shape alone: a batch row is bit-identical to the utterance computed alone, in
 * a buffer of any capacity.
 *
 * gt_vocos_norm: depthwise k = 7 convolution (optional) + LayerNorm over the C channels of every position:
 *   h[b, t, c] = bd[c] + sum_{j < 7} wd[c][j] X[b, t + j - 3, c]   one fp32 fmaf chain, j ascending; a tap outside [0, len_b) contributes
 *                0 and is not read.  wd == NULL (then bd == NULL too): h = X.
 *   Y = (h - mean) rstd g[c] + be[c], mean = sum h / C, rstd = rsqrtf(sum (h - mean)^2 / C + eps), fp32.
 *   X fp32 [B, L_cap, C] (b at x_stride_b elements); Y fp32 or bf16 (y_bf16, round to nearest even) at y_stride_b; wd fp32 [C][7].
 *   Y may be X only with wd == NULL and fp32 out.  One wave per row, a lane owns the C / 64 channels lane + 64 j;
 *   gt_vocos_norm_tile_positions() positions per workgroup.
 * Refusals, before any launch and in this order: args or X / g / be / Y / n_frames NULL; exactly one of wd / bd NULL; B, L_cap or C <= 0;
 * eps negative or NaN; x_stride_b or y_stride_b < L_cap C; Y == X with wd != NULL or y_bf16: GT_E_INVAL.  C no multiple of 64 or > 512,
 * B > 65535, B L_cap C >= 2^31: GT_E_UNSUPPORTED.  A pointer not 4-byte (a bf16 Y: 2-byte) aligned: GT_E_ALIGN. */
typedef struct gt_vocos_norm_args {
  const float* X; int64_t x_stride_b;
  const float* wd; const float* bd; const float* g; const float* be;
  void* Y; int64_t y_stride_b;
  const int32_t* n_frames;
  int B; int L_cap; int C; int y_bf16;
  float eps;
} gt_vocos_norm_args;
int gt_vocos_norm(const gt_vocos_norm_args* args, void* stream);
int gt_vocos_norm_args_size(void);              /* sizeof(gt_vocos_norm_args) */
int gt_vocos_norm_tile_positions(void);

/* gt_vocos_mlp: a ConvNeXt block's pointwise MLP with its residual; the hidden activation u stays on the chip:
 *   u[b, t, h] = bf16( gelu( b1[h] + sum_c A[b, t, c] W1[h][c] ) )       gelu(x) = 0.5 x (1 + erff(x / sqrt 2)) in fp32
 *   Y[b, t, n] = (b2[n] + sum_h u[b, t, h] W2[n][h]) + R[b, t, n]          fp32 MFMA accumulation, c and h ascending in 16-deep steps
 *   A        bf16 [B, L_cap, C] (gt_vocos_norm's output), b at a_stride_b elements.
 *   W1, W2   bf16 images of [H, C, 1] and [C, H, 1] in gt_voc_conv's fragment order (taps = 1); the caller folds the layer scale into
 *            W2 and b2.  b1 fp32 [H], b2 fp32 [C].
 *   R, Y     fp32 [B, L_cap, C] at r_stride_b / y_stride_b; Y may be R (an element is read and written by the same lane).
 *   U        optional (tests): bf16 [B, L_cap, H] at u_stride_b, receives u at positions < len_b (nothing else of it is written);
 *            Y is bit-identical with and without it.
 * A workgroup owns gt_vocos_tile_positions() positions, keeps their A tile in LDS and walks H in chunks of gt_vocos_hidden_chunk()
 * units through a double buffer: gt_vocos_mlp_lds_bytes(C) = tile (2 C + 16) + 2 tile (2 chunk + 16) bytes (0 for a C that is refused).
 * Refusals, before any launch and in this order: args or A / W1 / b1 / W2 / b2 / R / Y / n_frames NULL; B, L_cap, C or H <= 0; a_stride_b,
 * r_stride_b or y_stride_b < L_cap C; U with u_stride_b < L_cap H; Y == A, U == Y, R or A: GT_E_INVAL.  C not 128, 256 or 512, H no
 * multiple of the hidden chunk or > 2048, B > 65535, B L_cap max(C, H) >= 2^31: GT_E_UNSUPPORTED.  A, W1 or W2 not 16-byte aligned,
 * a_stride_b no multiple of 8, b1 / b2 / R / Y / n_frames not 4-byte, U not 8-byte aligned or u_stride_b no multiple of 4: GT_E_ALIGN. */
typedef struct gt_vocos_mlp_args {
  const void* A; int64_t a_stride_b;
  const void* W1; const float* b1; const void* W2; const float* b2;
  const float* R; int64_t r_stride_b;
  float* Y; int64_t y_stride_b;
  void* U; int64_t u_stride_b;
  const int32_t* n_frames;
  int B; int L_cap; int C; int H;
} gt_vocos_mlp_args;
int gt_vocos_mlp(const gt_vocos_mlp_args* args, void* stream);
int gt_vocos_mlp_args_size(void);               /* sizeof(gt_vocos_mlp_args) */
int gt_vocos_tile_positions(void);
int gt_vocos_hidden_chunk(void);
size_t gt_vocos_mlp_lds_bytes(int C);

/* gt_vocos_polar: the iSTFT head's nonlinearity into the spectrum workspace gt_istft reads (gt_gl_spec_bytes(B, F_max) bytes, the
 * fragment order described with gt_gl_polar):
 *   m = fminf(expf(O[b, f, k]), 100),  (re, im)[k] = m (cosf, sinf)(O[b, f, 513 + k]),  k < 513, f < F_b
 *   O fp32 [B, F_max, 1026] (b at o_stride_b elements): 513 log-magnitudes, then 513 phases (unbounded: the accurate library functions).
 *   F_b = min(n_frames[b], F_max), 0 below 2 frames (gt_istft's rule).  ALL of spec is defined: zeros from frame F_b on, the padded
 *   frames included.  Im of bin 0 is stored as gt_gl_polar stores it; Im of bin 512 is not kept.
 * Refusals, before any launch and in this order: args or O / n_frames / spec NULL, B outside [1, GT_MEL_MAX_B], F_max outside
 * [1, GT_MEL_MAX_FRAMES], o_stride_b < 1026 F_max: GT_E_INVAL; n_fft != 1024: GT_E_UNSUPPORTED; O or n_frames not 4-byte, spec not
 * 16-byte aligned: GT_E_ALIGN. */
typedef struct gt_vocos_polar_args {
  const float* O; int64_t o_stride_b;
  const int32_t* n_frames;
  float* spec;
  int B; int F_max; int n_fft;
} gt_vocos_polar_args;
int gt_vocos_polar(const gt_vocos_polar_args* args, void* stream);
int gt_vocos_polar_args_size(void);             /* sizeof(gt_vocos_polar_args) */

/* ---- objective synthesis metrics (csrc/dtw.hip): mel cepstra, dynamic time warping, F0 statistics along the path ----
 * gt_mel_cepstrum: the cepstrum of every frame of a ragged log-mel batch,
 *   out[b][f][k] = sum_{n < N} dct[k][n] mel[b][n][f]      k < K, f < len[b]      (ONE mul + add chain over n ascending, no fma)
 * and 0 for k in [K, 16) and for f in [len[b], F_max): every element of [B, F_max, 16] is written, no frame at or beyond len[b] is read.
 *   mel      fp32 [B, N, ld], the decoder's channel-major layout (TacotronSTFT's natural log).
 *   len      device int32 [B], clamped to [0, F_max].
 *   dct      fp32 [K, N]: rows 1..K of the orthonormal DCT-II, dct[k - 1][n] = sqrt(2 / N) cos(pi k (n + 1/2) / N), built on the host in
 *            float64 and rounded once (c0 is dropped: a gain in the log domain costs nothing).
 *   out      fp32 [B, F_max, 16]: rows of 64 bytes, the form gt_dtw_f32 takes.
 * Refusals, before any launch and in this order: NULL mel / len / dct / out, B outside [1, GT_MEL_MAX_B], N, K or F_max <= 0,
 * F_max > GT_MEL_MAX_FRAMES, ld < F_max: GT_E_INVAL; N > GT_MEL_MAX_N_MEL or K > 16: GT_E_UNSUPPORTED; out not 16-byte, mel, len or dct
 * not 4-byte aligned: GT_E_ALIGN.
 *
 * gt_dtw_f32: dynamic time warping of a[b] (a_len[b] rows) against b[b] (b_len[b] rows), every utterance on its own:
 *   d(i, j) = alpha sqrt(sum_{k < 16} (a[i][k] - b[j][k])^2)      (differences, products and a sum over k ascending, correctly rounded sqrt)
 *   D(0, 0) = d(0, 0),  D(i, j) = d(i, j) + min(D(i-1, j-1), D(i-1, j), D(i, j-1)), a missing predecessor +infinity; on equal values the
 *   first of that order wins.  cost[b] = D(a_len - 1, b_len - 1), the DP's own last cell; the path runs from (0, 0) to that cell,
 *   max(a_len, b_len) <= path_len[b] <= a_len + b_len - 1.
 *   a, b     fp32 [B, Fa_max, 16] / [B, Fb_max, 16] (feature vectors shorter than 16 padded with zeros).
 *   a_len, b_len  device int32 [B].  A length of 0 on either side: cost 0, path_len 0.  A length below 0 or above its capacity is
 *            treated as 0 and sets GT_DTW_ST_BAD_LEN in *status (optional device int32, OR-ed).
 *   path     int32 [B, ld_path, 2]: (i, j) forward from (0, 0), -1 from path_len[b] to ld_path; ld_path >= Fa_max + Fb_max - 1.
 *   workspace  gt_dtw_workspace_bytes(B, Fa_max, Fb_max) = 4 (B Fa_max nq + B round64(Fa_max + Fb_max)) bytes rounded up to 256, with
 *            nq = ceil(Fb_max / 16) rounded up to 4: two direction bits per cell (the fp32 lattice is never stored) and the path in walk
 *            order.  Needs no initialisation.
 * Two launches: the DP, one workgroup of min(ceil(Fa_max / 64), 16) waves per utterance with gt_dtw_lds_bytes(Fa_max, Fb_max) bytes of
 * dynamic LDS, and the walk back along the direction bits, one workgroup of four waves per utterance.  The DP's LDS: a ring of
 * 512 bytes per wave, 4 Fb_max bytes (rounded up to 16) where Fa_max > 1024, and the image of b's features, 64 Fb_max bytes, where all
 * of it fits 160 KB (else b is read from global memory: the same arithmetic).  Both helpers return 0 for a shape that is refused.
 * Asynchronous, no allocation, no host synchronisation, capturable in a graph; every element of cost, path_len and path
 * is written; no value depends on B, the capacities or the schedule: a batch row is bit-identical to the utterance alone.
 * Refusals, before any launch and in this order: NULL a / b / a_len / b_len / cost / path_len / path / workspace, B outside
 * [1, GT_MEL_MAX_B], Fa_max or Fb_max <= 0, ld_path < Fa_max + Fb_max - 1, workspace_bytes below gt_dtw_workspace_bytes: GT_E_INVAL;
 * Fa_max or Fb_max > GT_DTW_MAX_F: GT_E_UNSUPPORTED; a, b, path or workspace not 16-byte, a_len, b_len, cost, path_len or status not
 * 4-byte aligned: GT_E_ALIGN.
 *
 * gt_dtw_f0_stats: over the path_len[b] (clamped to [0, ld_path]) steps (i, j) of path[b], with x = f0_a[b][i], y = f0_b[b][j] in Hz and
 * 0 = unvoiced (gt_yin_f0's form): counts[b] = {n_vv: both voiced; n_vu: exactly one voiced; n_gross: both voiced and
 * |x - y| > 0.2 y (compared in fp64)}, sums[b] = {sum (x - y)^2, sum (1200 log2(x / y))^2} over the both-voiced steps, the cents
 * term formed in fp64 and rounded once.  One workgroup per utterance, per-thread sums at a stride of 256 steps and one fixed tree: no
 * atomics, a batch row is the utterance alone.  A step outside [0, ld_a) x [0, ld_b) is skipped.
 * Refusals, before any launch and in this order: a NULL pointer, B outside [1, GT_MEL_MAX_B], ld_path, ld_a or ld_b <= 0: GT_E_INVAL;
 * path not 8-byte, any other pointer not 4-byte aligned: GT_E_ALIGN. */
#define GT_DTW_MAX_F 4096
#define GT_DTW_ST_BAD_LEN 1
size_t gt_dtw_lds_bytes(int Fa_max, int Fb_max);
size_t gt_dtw_workspace_bytes(int B, int Fa_max, int Fb_max);
int gt_mel_cepstrum(const float* mel, int ld, const int32_t* len, const float* dct, int B, int N, int K, int F_max, float* out,
                    void* stream);
int gt_dtw_f32(const float* a, const float* b, const int32_t* a_len, const int32_t* b_len, int B, int Fa_max, int Fb_max, float alpha,
               float* cost, int32_t* path_len, int32_t* path, int ld_path, void* workspace, size_t workspace_bytes, int32_t* status,
               void* stream);
int gt_dtw_f0_stats(const int32_t* path, int ld_path, const int32_t* path_len, const float* f0_a, int ld_a, const float* f0_b, int ld_b,
                    int B, int32_t* counts, float* sums, void* stream);

/* ---- WaveGlow vocoder (csrc/waveglow.hip): the reverse flow's two kernels next to gt_voc_conv --------------------------
 * One run of n_flows WaveNets of n layers is gt_voc_conv (the upsampling transposed convolution as a 7-tap convolution at frame rate,
 * x_mel, N = 20480 = spect [B, 32 F, 640] bf16), gt_wg_boundary (first form), per flow n x (gt_wg_gate, gt_voc_conv res_skip, taps 1, Y
 * aliasing acc on the state) and one gt_wg_boundary: 1 + n_flows 2 n + n_flows + 1 launches.  Positions are GROUPS of 8 samples:
 * len_b = min(max(n_frames[b], 0) len_mul, L_cap) with len_mul = 32; nothing at or behind len_b is read, the host never reads n_frames.
 *
 * gt_wg_gate: one WaveNet layer's dilated in_layer + its slice of the conditioning layer + the gate, as ONE implicit GEMM:
 *   acts[b, t, m] = b_in[m] + b_cond[m] + sum_{j < taps} sum_{c < C} bf16( X[b, t + (j - taps / 2) dil, c] ) W_in[j][m][c]
 *                                       + sum_{c < Cs} S[b, t, c] W_cond[m][c]                                  m < 2C, t < len_b
 *   G[b, t, n]    = bf16( tanhf_(acts[b, t, n]) * sigmoidf_(acts[b, t, n + C]) )                                  n < C    (csrc/common.h)
 *   A tap outside [0, len_b) contributes 0 and is never read; G at positions [len_b, L_cap) is written as bf16 zero.
 *   X        fp32 residual stream, element (b, t, c) at X[b x_stride_b + t ldx + c] (ldx = 2C on the x | skip state); rounded to
 *            nearest even to bf16 when staged: that value is the MFMA operand.
 *   S        bf16 spect, element (b, t, c) at S[b s_stride_b + t Cs + c]; no halo.
 *   W_in     bf16 image of [2C', C, taps] in gt_voc_conv's fragment order, W_cond of [2C', Cs, 1], where the 2C output rows are
 *            INTERLEAVED in groups of 32: packed row 64 q + r is channel 32 q + r, packed row 64 q + 32 + r is channel C + 32 q + r
 *            (q < C / 32, r < 32).  A lane then holds acts[n] and acts[n + C] of the same positions: the gate needs no LDS round trip.
 *   b_in, b_cond  fp32 [2C] in the natural channel order.
 *   G        bf16 [B, L_cap, C], element (b, t, n) at G[b g_stride_b + t C + n]; G may not alias X or S.
 * A workgroup of four waves owns gt_wg_tile_positions() positions x 128 gate channels (a wave: all positions x 32 channels = two
 * 32-column accumulator tiles), stages 64-channel chunks of X with (taps - 1) dil halo rows, then of S, in
 * gt_wg_gate_lds_bytes(C, taps, dil) = (tile + (taps - 1) dil) 144 bytes of LDS, at most 64 KB (0 for a shape that is refused).
 * Asynchronous, no allocation, no atomics, capturable in a graph; the grid is sized by L_cap.  fp32 accumulation in the MFMA over
 * (X chunk, tap, k-step) then (S chunk, k-step) ascending: the summation order depends on (t, n, C, taps) alone — a batch row is
 * bit-identical to the utterance computed alone, in a buffer of any capacity.
 * Refusals, before any launch and in this order: args or X / S / W_in / W_cond / b_in / b_cond / G / n_frames NULL; B, L_cap, C, Cs, dil
 * or len_mul <= 0; taps <= 0 or even; ldx < C, x_stride_b < L_cap ldx, s_stride_b < L_cap Cs, g_stride_b < L_cap C; G == X or G == S:
 * GT_E_INVAL.  taps > GT_VOC_MAX_TAPS, C or Cs no multiple of 64, B > 65535, B L_cap max(ldx, Cs) >= 2^31, a halo past the LDS bound:
 * GT_E_UNSUPPORTED.  X, S, W_in or W_cond not 16-byte, b_in / b_cond / G / n_frames not 4-byte aligned, ldx or x_stride_b no multiple
 * of 4, s_stride_b no multiple of 8: GT_E_ALIGN. */
typedef struct gt_wg_gate_args {
  const float* X; int64_t x_stride_b; int ldx;
  int Cs; const void* S; int64_t s_stride_b;
  const void* W_in; const void* W_cond; const float* b_in; const float* b_cond;
  void* G; int64_t g_stride_b;
  int len_mul; const int32_t* n_frames;
  int B; int L_cap; int C; int taps; int dil;
} gt_wg_gate_args;
int gt_wg_gate(const gt_wg_gate_args* args, void* stream);
int gt_wg_gate_args_size(void);                 /* sizeof(gt_wg_gate_args): lets a binding check its mirror of the struct */
int gt_wg_tile_positions(void);
size_t gt_wg_gate_lds_bytes(int C, int taps, int dil);

/* gt_wg_boundary: everything between two WaveNets of the reverse flow, per group position t < len_b, in fp32 on the vector ALU.  The
 * audio lives in 8 SLOTS per position, A[b a_stride_b + 8 t + s]: the c current channels are slots [8 - c, 8) (slot s is channel s of
 * the latent Z, so an early output is prepended by widening the window downwards), and with c = 8 the buffer IS the waveform,
 * wav[b, 8 t + s].  With c_in channels before and c_out after (lo = 8 - c_in, h = c_in / 2, lo' = 8 - c_out, h' = c_out / 2), in order:
 *   1. end     e[r] = b_end[r] + sum_{c < C} skip[b, t, c] w_end[c][r],  r = s - 4 (the shift of slot s) and s (its log-scale) for the
 *              coupled slots s in [lo + h, 8) (never below 4): per lane an fmaf chain over c = lane, lane + 64, ... ascending, then
 *              the xor butterfly of the wave (offsets 32, 16, ..., 1), then the bias.  skip[b, t, c] = state[b st_stride_b + t ld + C + c].
 *   2. couple  a[s] = (a[s] - e[s - 4]) expf(-e[s])   for s in [lo + h, 8)   (the device library's expf)
 *   3. 1x1     a'[s] = sum_{k = lo}^{7} w_inv[s][k] a[k]   for s in [lo, 8): ONE fmaf chain over k ascending from 0 (w_inv is the
 *              8 x 8 image of the c_in x c_in inverse, zero outside its block; slots below lo enter as 0)
 *   4. concat  a'[2p], a'[2p + 1] = sigma (e0, e1) of randn_pair(randn_key(seed, 5, b), t, p) for the new slots [lo', lo)
 *              (csrc/common.h; stream id 5); seed by value, or (seed_dev != NULL) *seed_dev read on the device.
 *   5. start   x[b, t, n] = b_start[n] + sum_{s = lo'}^{lo' + h' - 1} w_start[n][s] a'[s],  n < C: ONE fmaf chain over s ascending from
 *              the bias, written to state[b st_stride_b + t ld + n]; skip[b, t, :] is cleared to 0 in the same pass.
 *   A[b, t, 0..8) is written whole (slots below lo' as 0).
 * Forms: w_end == NULL (with b_end, w_inv NULL and c_in = 0) is the FIRST form: steps 1-3 are skipped, the c_out slots are drawn.
 * w_start == NULL (with b_start NULL, c_out = 8) is the LAST form: step 5 is skipped, the state is not touched, and A at positions
 * [len_b, L_cap) is written as 0 — the samples, zero behind the utterance.  In the other forms nothing at or behind len_b is written.
 *   w_end    fp32 [C][8], b_end fp32 [8] (columns of uncoupled slots are not used); w_inv fp32 [8][8]; w_start fp32 [C][8], b_start [C].
 * A wave owns 8 consecutive positions, a workgroup of four waves 32; no LDS.  Asynchronous, no allocation, no atomics, capturable in a
 * graph; the grid is sized by L_cap; every order above depends on (t, C) alone: a batch row is bit-identical to the utterance alone.
 * Refusals, before any launch and in this order: args or state / A / n_frames NULL; B, L_cap, C or len_mul <= 0; ld < 2C,
 * st_stride_b < L_cap ld, a_stride_b < 8 L_cap; c_in or c_out odd or outside [0, 8], c_out < 2, c_out < c_in; w_end, b_end and w_inv
 * not all NULL or all set, or set with c_in == 0, or NULL with c_in > 0; w_start and b_start not both NULL or both set, or NULL with
 * c_out != 8; sigma negative or NaN: GT_E_INVAL.  C no multiple of 64 or > GT_WG_MAX_C, B > 65535, B L_cap ld >= 2^31:
 * GT_E_UNSUPPORTED.  A, w_end, w_inv or w_start not 16-byte, any other pointer not 4-byte aligned, ld, st_stride_b or a_stride_b no
 * multiple of 4: GT_E_ALIGN. */
#define GT_WG_MAX_C 512
#define GT_WG_NOISE_STREAM 5
typedef struct gt_wg_boundary_args {
  float* state; int64_t st_stride_b; int ld;
  int C; float* A; int64_t a_stride_b;
  const float* w_end; const float* b_end; const float* w_inv; const float* w_start; const float* b_start;
  const int32_t* n_frames; const uint32_t* seed_dev;
  uint32_t seed; float sigma;
  int len_mul; int B; int L_cap; int c_in; int c_out;
} gt_wg_boundary_args;
int gt_wg_boundary(const gt_wg_boundary_args* args, void* stream);
int gt_wg_boundary_args_size(void);             /* sizeof(gt_wg_boundary_args) */

/* ---- spectral-subtraction denoiser behind the vocoders (csrc/denoise.hip) -----------------------------------------
 * NVIDIA's WaveGlow `Denoiser` (denoiser.py, mode "zeros") is STFT.inverse(clamp(|X| - strength bias_spec, min = 0), angle X) with
 * X = STFT(audio), n_fft = win = 1024, hop = 256, and bias_spec [513] frame 0 of |STFT| of the network's output for a zero mel at
 * sigma = 0.  gt_denoise_spec is its analysis half with the subtraction as the epilogue; gt_istft (above) is the other half.
 *   wav      in, [B rows, pitch ld_wav] fp32: row b holds what a vocoder wrote for n_b = min(n_frames[b], F_max) mel frames,
 *            L_b = 256 max(n_b - lost, 0) samples (lost = the vocoder's min_frames - 1: 0 or 1; L_b additionally clamped to
 *            256 (ld_wav / 256)).  Frames are reflected about the utterance's own ends as gt_gl_project takes them; nothing at or
 *            behind L_b is read.
 *   frames_out  out, int32 [B]: Fa_b = L_b / 256 + 1 analysis frames, 0 where L_b == 0 — the n_frames of the gt_istft call that
 *            follows, at the capacity Fa_max = F_max - lost + 1 (its row of 256 (Fa_max - 1) = 256 (F_max - lost) samples).
 *   spec     out, gt_gl_spec_bytes(B, Fa_max) bytes in the fragment order described with gt_gl_polar, ALL of it defined (zeros from
 *            frame Fa_b on): Y = X max(|X| - c_k, 0) / |X| with c_k = strength[0] * bias[k] (one fp32 product), X the folded DFT
 *            with the basis image of gt_mel_pack (mel_packed); |X|^2 == 0 in fp32 gives (max(-c_k, 0), 0), as atan2(0, 0) = 0 does.
 *            Bin 512 is real: y = sign(x) max(|x| - c_512, 0).  The unit phasor replaces the reference's atan2 / cos / sin (the same
 *            mathematics).
 *   bias     fp32 [513]; strength: ONE fp32 word, both read on the device — a captured graph replays with the value the word holds.
 * Asynchronous, no allocation, no atomics, capturable in a graph; the grid is sized by Fa_max; the summation order of an element
 * depends on its index within its utterance alone: a batch row is bit-identical to the utterance computed alone.
 * Refusals, before any launch and in this order: args or a pointer NULL, lost outside {0, 1}, ld_wav <= 0, B outside
 * [1, GT_MEL_MAX_B], F_max or F_max - lost + 1 outside [1, GT_MEL_MAX_FRAMES]: GT_E_INVAL; n_fft != 1024, hop != 256 or win != 1024:
 * GT_E_UNSUPPORTED; wav, mel_packed or spec not 16-byte, bias, strength, n_frames or frames_out not 4-byte aligned, ld_wav no
 * multiple of 4: GT_E_ALIGN. */
typedef struct gt_denoise_spec_args {
  const float* wav; const float* bias; const float* strength;
  const int32_t* n_frames; const void* mel_packed;
  float* spec; int32_t* frames_out;
  int ld_wav; int lost; int B; int F_max; int n_fft; int hop; int win;
} gt_denoise_spec_args;
int gt_denoise_spec(const gt_denoise_spec_args* args, void* stream);
int gt_denoise_spec_args_size(void);            /* sizeof(gt_denoise_spec_args) */

/* ---- ITU-R BS.1770-4 integrated loudness and normalisation behind the vocoders (csrc/loudness.hip) ------------------
 * Mono.  z = the K-weighting cascade (two biquads, zero initial state) of x; Ns = fs / 10, Nb = 4 Ns; an utterance of N >= Nb samples
 * has J = N / Ns - 3 blocks of mean square z_j over samples [j Ns, j Ns + Nb), one of N < Nb has ONE block over all its samples (the
 * recommendation is silent below 400 ms), N = 0 none; l_j = -0.691 + 10 log10 z_j; A = {l_j > -70}, Gamma = l(mean_A z) - 10,
 * R = {j in A: l_j > Gamma}, L = l(mean_R z), -inf where A is empty.  peak = max |x| (the sample peak);
 * g = 10^((target - L) / 20), lowered to ceiling / peak where g peak > ceiling, 1 where L = -inf.
 *   wav      [B rows, pitch ld elements] fp32, or (is_i16) int16 scaled by 1 / 32768.  Row b holds N_b = min(hop max(n_frames[b] -
 *            lost, 0), L_cap) samples (a vocoder's row: hop and lost = min_frames - 1 are its own; stand-alone callers pass hop = 1,
 *            lost = 0 and sample counts).  Nothing at or behind N_b is read.
 *   params   GT_LOUD_PARAMS doubles read on the device: [0..4] the shelf's b0 b1 b2 a1 a2, [5..9] the high-pass's, [10..25] M, the
 *            4 x 4 row-major transition of the cascade's state (s1, s2 of the shelf, s1, s2 of the high-pass, transposed direct form
 *            II) over gt_loudness_chunk(fs) samples, [26..41] M^16, [42] the target in LUFS, [43] the peak ceiling, linear,
 *            [44..59] M^256.  A captured graph replays with the values the words hold.
 *   stats    out, fp32 [B][GT_LOUD_STATS]: L, peak, g, J, |A|, |R|, Gamma (-inf where A is empty), N_b.
 *   ws       gt_loudness_ws_bytes(B, L_cap, fs) bytes, 16-byte aligned: chunk states (double [B][Kc][4], Kc = ceil(L_cap / Lc)), chunk
 *            sums of z^2 (double [B][Kc]), segment sums (double [B][L_cap / Ns + 1]), chunk peaks (float [B][Kc]), in this order.
 * gt_loudness_measure: four launches (chunk end states from zero; the state scan; chunk sums from the true start states; blocks,
 * gates and gain), the recurrence, every sum and the gating in double.  gt_loudness_apply: one launch, fp32 rows only: y = g x for
 * the N_b samples and 0 from there to L_cap, g = stats[b][2]; written over wav, or (out != NULL) to out [B rows, pitch ld_out] with
 * wav only read.  params and ws are not looked at by gt_loudness_apply.
 * gt_loudness_chunk(fs): the chunk length Lc, the largest divisor of fs / 10 in [16, 50]; 0 for a rate the kernels do not take
 * (fs outside [8000, 192000], no multiple of 10, or no such divisor).  16000, 22050, 24000, 44100, 48000 give 50, 49, 50, 49, 50.
 * gt_loudness_ws_bytes: 0 outside what the kernels take (such a rate, B outside [1, GT_MEL_MAX_B], L_cap <= 0, 4 B Kc >= 2^31).
 * Asynchronous, no allocation, no atomics, capturable in a graph; grids are sized by B and L_cap; the order of every sum depends on
 * the index within the utterance alone: a batch row, stats and samples, is bit-identical to the utterance computed alone.
 * Refusals, before any launch and in this order: args, wav, n_frames or stats NULL, (measure) params or ws NULL, B outside
 * [1, GT_MEL_MAX_B], L_cap <= 0, ld < L_cap, hop <= 0, lost < 0, (apply, out != NULL) ld_out < L_cap, (measure) ws_bytes below
 * gt_loudness_ws_bytes: GT_E_INVAL; a rate or a capacity the kernels do not take, (apply) is_i16: GT_E_UNSUPPORTED; wav not aligned
 * to its element, n_frames, stats or out not 4-byte, (measure) params not 8-byte or ws not 16-byte aligned: GT_E_ALIGN. */
#define GT_LOUD_STATS 8
#define GT_LOUD_PARAMS 64
typedef struct gt_loudness_args {
  void* wav; const int32_t* n_frames; const double* params;
  float* stats; void* ws; float* out;
  int64_t ws_bytes;
  int ld; int ld_out; int is_i16; int hop; int lost; int B; int L_cap; int fs;
} gt_loudness_args;
int gt_loudness_measure(const gt_loudness_args* args, void* stream);
int gt_loudness_apply(const gt_loudness_args* args, void* stream);
int gt_loudness_args_size(void);                /* sizeof(gt_loudness_args) */
int gt_loudness_chunk(int fs);
size_t gt_loudness_ws_bytes(int B, int L_cap, int fs);

#ifdef __cplusplus
}
#endif
#endif /* GLOWTTS_HIP_H */
