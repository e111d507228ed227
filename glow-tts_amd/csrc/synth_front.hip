// Device front end of synthesis (FlowGenerator.infer with set_synthesis_front): durations -> lengths, the encoder's
// prior + a seed -> the sampled, squeezed latent in the rows layout the reverse decoder reads, and the counter-hash Gaussian draws
// of the stochastic predictors.  Plain C++: vector stores only, no atomics, every output element has exactly one writer, so the
// results are deterministic by construction.  Memory-bound; no MFMA.
#include "common.h"
#include "../../include/glowtts_hip.h"
#include "internal.h"

#define HALO GT_HALO

#define SF_TX_MAX 512        // tokens per utterance (gt_prior_expand's and gt_mas_f32's limit)
#define SF_C_MAX 80          // mel channels
#define SF_ROWS 32           // squeezed rows of one workgroup's tile ...
#define SF_FRAMES 64         // ... = frames of it
#define SF_LD (SF_FRAMES + 1)   // LDS pitch of a channel's frames: the row phase reads one channel per lane, 65 words apart
#define SF_DUR_MAX 1048576.f // a token's duration is clamped here: 512 tokens stay inside int32
#define SF_LONG_TX_MAX GT_SYNTH_LONG_MAX_TX   // tokens per utterance of the *_long entries (gt_attn_fwd's and gt_mas_long_f32's limit)
#define SF_LONG_DUR_MAX 262144.f              // ... and their clamp: 4096 tokens of 2^18 frames sum to 2^30
#define SF_LONG_TOK (SF_LONG_TX_MAX / 256)    // tokens per thread of gt_synth_lengths_long_kernel

// One wave per utterance: lane l owns tokens [8 l, 8 l + 8); inclusive scan over the wave with shuffles.
__global__ __launch_bounds__(64) void gt_synth_lengths_kernel(const float* __restrict__ dur, const int32_t* __restrict__ x_len,
                                                              int32_t* __restrict__ cum, int32_t* __restrict__ y_len,
                                                              float* __restrict__ logw, int Tx)
{
  const int b = blockIdx.x, lane = threadIdx.x;
  const int n = min(max(x_len[b], 0), Tx);
  const size_t base = (size_t)b * Tx;
  int d[8];
  int own = 0;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const int i = lane * 8 + k;
    d[k] = (i < n) ? (int)fminf(fmaxf(dur[base + i], 0.f), SF_DUR_MAX) : 0;     // fmaxf drops a NaN
    own += d[k];
  }
  int incl = own;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int v = __shfl_up(incl, o);
    if (lane >= o) incl += v;
  }
  int run = incl - own;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const int i = lane * 8 + k;
    run += d[k];
    if (i < Tx) {
      cum[base + i] = run;
      if (logw) logw[base + i] = logf(1e-8f + (float)d[k]) * (i < n ? 1.f : 0.f);
    }
  }
  if (lane == 63) y_len[b] = max(incl, 1);
}

// 513 .. 4096 tokens (gt_synth_lengths_long; it takes every 1 <= Tx <= 4096): one workgroup per utterance, thread t owns tokens
// [16 t, 16 t + 16); the scan of a wave as above, the totals of the four waves through LDS (as gt_synth_geometry_kernel does).
// Integer sums: the same cum / y_len in whatever order they are added.
__global__ __launch_bounds__(256) void gt_synth_lengths_long_kernel(const float* __restrict__ dur, const int32_t* __restrict__ x_len,
                                                                    int32_t* __restrict__ cum, int32_t* __restrict__ y_len,
                                                                    float* __restrict__ logw, int Tx)
{
  __shared__ int32_t wsum_s[4];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int n = min(max(x_len[b], 0), Tx);
  const size_t base = (size_t)b * Tx;
  int d[SF_LONG_TOK];
  int own = 0;
#pragma unroll
  for (int k = 0; k < SF_LONG_TOK; ++k) {
    const int i = tid * SF_LONG_TOK + k;
    d[k] = (i < n) ? (int)fminf(fmaxf(dur[base + i], 0.f), SF_LONG_DUR_MAX) : 0;     // fmaxf drops a NaN
    own += d[k];
  }
  int incl = own;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int v = __shfl_up(incl, o);
    if (lane >= o) incl += v;
  }
  if (lane == 63) wsum_s[w] = incl;
  __syncthreads();
  int run = incl - own;
  for (int j = 0; j < w; ++j) run += wsum_s[j];
#pragma unroll
  for (int k = 0; k < SF_LONG_TOK; ++k) {
    const int i = tid * SF_LONG_TOK + k;
    run += d[k];
    if (i < Tx) {
      cum[base + i] = run;
      if (logw) logw[base + i] = logf(1e-8f + (float)d[k]) * (i < n ? 1.f : 0.f);
    }
  }
  if (tid == 255) y_len[b] = max(run, 1);
}

// A workgroup owns utterance blockIdx.y and row offsets [32 k, 32 k + 32) of it = squeezed frames s in [32 k - 2, 32 k + 30) =
// frames t in [64 k - 4, 64 k + 60): the halo rows in front belong to tile 0, the halo / padding / rounding rows behind to the
// tiles they fall into, so every row has one writer.  The tokens a tile touches are a contiguous range of the utterance: their
// means / log-deviations go through LDS frame by frame (a wave reads one channel along Tx, one workgroup-wide phase later a
// wave writes rows along the channels).
// CALL: seed / noise_scale come from the gt_synth_call block in device memory (a captured graph replays with the scalars of
// every call) instead of the by-value arguments; the only difference between those two instantiations.
// LONG (Tx <= SF_LONG_TX_MAX, the *_long entries): the utterance's scan is the one Tx-sized thing here; the 64 binary searches of a
// tile read it where gt_synth_lengths_long left it (16 KiB at most, L2-hot) instead of every tile copying the whole row into LDS.
template <bool CALL, bool LONG>
__global__ __launch_bounds__(256) void gt_synth_prior_kernel(gt_synth_prior_args a, const gt_synth_call* __restrict__ call)
{
  __shared__ float m_s[SF_C_MAX * SF_LD];
  __shared__ float l_s[SF_C_MAX * SF_LD];
  __shared__ int32_t cum_s[LONG ? 1 : SF_TX_MAX];
  __shared__ int32_t tok_s[SF_FRAMES];
  const int b = blockIdx.y, k = blockIdx.x, tid = threadIdx.x;
  const int C = a.C, Tx = a.Tx, Ty = a.Ty;
  const int n = min(max(a.x_len[b], 0), Tx);
  const int ylen = a.y_len[b];
  // a tile behind the utterance's rows AND behind the optional outputs' frames has nothing to write (a capacity-sized grid)
  if (k * SF_ROWS >= gt_row_count(a.row0, b, a.Tp) && k * SF_FRAMES - 2 * HALO >= Ty) return;
  const int32_t* __restrict__ cum_b = a.cum + (size_t)b * Tx;
  if (!LONG) {
    for (int i = tid; i < n; i += 256) cum_s[i] = cum_b[i];
    __syncthreads();
  }
  const int32_t* cum_r = LONG ? cum_b : cum_s;          // entries [0, n) are read
  const int t0 = k * SF_FRAMES - 2 * HALO;
  if (tid < SF_FRAMES) {
    const int t = t0 + tid;
    int tok = -1;                                       // commons.generate_path: the first token whose cumulative duration passes t
    if (t >= 0 && t < ylen && n > 0 && t < cum_r[n - 1]) {
      int lo = 0, hi = n - 1;
      while (lo < hi) { const int mid = (lo + hi) >> 1; if (cum_r[mid] > t) hi = mid; else lo = mid + 1; }
      tok = lo;
    }
    tok_s[tid] = tok;
    if (a.frame2token && t >= 0 && t < Ty) a.frame2token[(size_t)b * Ty + t] = tok;
  }
  __syncthreads();
  for (int idx = tid; idx < C * SF_FRAMES; idx += 256) {
    const int c = idx >> 6, f = idx & 63, t = t0 + f;
    const int tok = tok_s[f];
    const size_t src = ((size_t)b * C + c) * Tx + (tok >= 0 ? tok : 0);
    const float m = tok >= 0 ? a.x_m[src] : 0.f;
    const float l = (tok >= 0 && a.x_logs) ? a.x_logs[src] : 0.f;
    m_s[c * SF_LD + f] = m;
    l_s[c * SF_LD + f] = l;
    if (t >= 0 && t < Ty) {
      if (a.z_m) a.z_m[((size_t)b * C + c) * Ty + t] = m;
      if (a.z_logs) a.z_logs[((size_t)b * C + c) * Ty + t] = l;
    }
  }
  if (a.attn) {
    for (int idx = tid; idx < Tx * SF_FRAMES; idx += 256) {
      const int i = idx >> 6, f = idx & 63, t = t0 + f;
      if (t >= 0 && t < Ty) a.attn[((size_t)b * Tx + i) * Ty + t] = tok_s[f] == i ? 1.f : 0.f;
    }
  }
  __syncthreads();
  const int base = gt_row_base(a.row0, b, a.Tp), nrow = gt_row_count(a.row0, b, a.Tp);
  const int len_sq = ylen / 2;                          // commons.squeeze drops an odd trailing frame
  const uint32_t key = randn_key(CALL ? call->seed : a.seed, 0u, (uint32_t)b);
  const float ns = CALL ? call->noise_scale : a.noise_scale;
  const int ldr = 2 * C;
  for (int idx = tid; idx < SF_ROWS * C; idx += 256) {
    const int j = idx / C, c = idx - j * C;
    const int off = k * SF_ROWS + j, r = base + off;
    if (off >= nrow || r >= a.R) continue;
    const int s = off - HALO;
    float v0 = 0.f, v1 = 0.f;
    if (s >= 0 && s < len_sq) {
      v0 = m_s[c * SF_LD + 2 * j];
      v1 = m_s[c * SF_LD + 2 * j + 1];
      if (ns != 0.f) {
        float e0, e1;
        randn_pair(key, (uint32_t)s, (uint32_t)c, e0, e1);
        v0 += expf(l_s[c * SF_LD + 2 * j]) * e0 * ns;
        v1 += expf(l_s[c * SF_LD + 2 * j + 1]) * e1 * ns;
      }
    }
    a.rows[(size_t)r * ldr + c] = v0;
    a.rows[(size_t)r * ldr + C + c] = v1;
  }
}

template <bool CALL>
__global__ __launch_bounds__(256) void gt_randn_rows_kernel(float* __restrict__ out, int R, int ncol, uint32_t seed, uint32_t stream_id,
                                                            float scale, const gt_synth_call* __restrict__ call, int which_scale)
{
  if (CALL) { seed = call->seed; scale = which_scale == 0 ? call->noise_scale : call->noise_scale_w; }
  const int np = (ncol + 1) >> 1;
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= R * np) return;
  const int row = idx / np, p = idx - row * np;
  float e0, e1;
  randn_pair(randn_key(seed, stream_id, 0u), (uint32_t)row, (uint32_t)p, e0, e1);
  out[(size_t)row * ncol + 2 * p] = e0 * scale;
  if (2 * p + 1 < ncol) out[(size_t)row * ncol + 2 * p + 1] = e1 * scale;
}

// The ragged rows layout of the squeezed mel axis from the predicted lengths, on the device: what
// RowsCtx.row_starts + gt_rows_ctx_fill give for lengths [min(y_len, Ty_cap) / 2], with starts[B] = R_cap.  Every workgroup redoes
// the <= 1024-element scan in LDS (4 lengths per thread, shuffles inside a wave, 4 wave totals through LDS) and fills its own 256
// rows by binary search: no grid-wide ordering, one writer per element.  Rows that do not fit (status bit 1): the clipped offsets
// have the closed form row0[b] = min(P[b], R_cap - 2 HALO (B - b)) of the unclipped offsets P — utterances in order, each keeps its
// two halos and as many frames as still fit in front of the halos of those behind it — so nothing is sequential.
// DIV = 2: the squeezed axis (gt_synth_geometry).  DIV = 1: the frame-rate axis of the stochastic pitch / energy predictors
// (gt_synth_frame_geometry) — the same scan, closed form and tables on whole frames; it runs behind the DIV = 2 launch in
// stream order, takes that launch's y_len_eff as its lengths, writes no y_len_eff of its own and ORs bit 2 into the status word.
template <int DIV>
__global__ __launch_bounds__(256) void gt_synth_geometry_kernel(const int32_t* __restrict__ y_len, int B, int Ty_cap, int R_cap,
                                                                int32_t* __restrict__ row0, int32_t* __restrict__ len_sq,
                                                                int32_t* __restrict__ y_len_eff, int64_t* __restrict__ rowbatch,
                                                                int32_t* __restrict__ rowframe, float* __restrict__ rowmask,
                                                                int32_t* __restrict__ rowutt, int32_t* __restrict__ status)
{
  __shared__ int32_t r0_s[GT_STEP_MAX_B];
  __shared__ int32_t len_s[GT_STEP_MAX_B];
  __shared__ int32_t wsum_s[4];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  int yl[4], l[4];
  int own = 0, over = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int i = tid * 4 + k;
    yl[k] = i < B ? max(y_len[i], 0) : 0;
    over |= yl[k] > Ty_cap;
    yl[k] = min(yl[k], Ty_cap);
    l[k] = DIV == 2 ? yl[k] >> 1 : yl[k];
    own += i < B ? l[k] + 2 * HALO : 0;
  }
  int incl = own;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int v = __shfl_up(incl, o);
    if (lane >= o) incl += v;
  }
  if (lane == 63) wsum_s[w] = incl;
  over = __syncthreads_or(over);
  int P = incl - own;                                    // unclipped offset of this thread's first utterance
  for (int j = 0; j < w; ++j) P += wsum_s[j];
  const int total = wsum_s[0] + wsum_s[1] + wsum_s[2] + wsum_s[3];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int i = tid * 4 + k;
    if (i < B) {
      const int start = min(P, R_cap - 2 * HALO * (B - i));
      P += l[k] + 2 * HALO;
      const int le = min(P, R_cap - 2 * HALO * (B - i - 1)) - start - 2 * HALO;      // frames that fit: <= l[k], >= 0
      r0_s[i] = start;
      len_s[i] = le;
      if (blockIdx.x == 0) {
        row0[i] = start;
        len_sq[i] = le;
        if (DIV == 2) y_len_eff[i] = le == l[k] ? yl[k] : 2 * le;      // an odd trailing frame stays (the prior's optional outputs hold it)
        if (i == B - 1) row0[B] = R_cap;                  // the last utterance owns the spare rows, masked
      }
    }
  }
  if (blockIdx.x == 0 && tid == 0) {
    if (DIV == 2) *status = (over ? 1 : 0) | (total > R_cap ? 2 : 0);
    else if (total > R_cap) *status |= 4;        // one thread, behind the squeezed geometry's store in stream order
  }
  __syncthreads();
  const int m = blockIdx.x * 256 + tid;
  if (m >= R_cap) return;
  int lo = 0, hi = B - 1;
  while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (r0_s[mid] <= m) lo = mid; else hi = mid - 1; }
  const int t = m - r0_s[lo] - HALO;
  rowbatch[m] = lo;
  if (rowutt) rowutt[m] = lo;
  rowframe[m] = t;
  rowmask[m] = (t >= 0 && t < len_s[lo]) ? 1.f : 0.f;
}

extern "C" int gt_synth_lengths(const float* dur, const int32_t* x_len, int32_t* cum, int32_t* y_len, float* logw, int B, int Tx,
                                void* stream)
{
  if (B < 0 || Tx <= 0) return GT_E_INVAL;
  if (B == 0) return 0;
  if (!dur || !x_len || !cum || !y_len) return GT_E_INVAL;
  if (Tx > SF_TX_MAX) return GT_E_UNSUPPORTED;
  hipLaunchKernelGGL(gt_synth_lengths_kernel, dim3(B), dim3(64), 0, GT_ST(stream), dur, x_len, cum, y_len, logw, Tx);
  GT_RET();
}

extern "C" int gt_synth_lengths_long(const float* dur, const int32_t* x_len, int32_t* cum, int32_t* y_len, float* logw, int B, int Tx,
                                     void* stream)
{
  if (B < 0 || Tx <= 0) return GT_E_INVAL;
  if (B == 0) return 0;
  if (!dur || !x_len || !cum || !y_len) return GT_E_INVAL;
  if (Tx > SF_LONG_TX_MAX) return GT_E_UNSUPPORTED;
  hipLaunchKernelGGL(gt_synth_lengths_long_kernel, dim3(B), dim3(256), 0, GT_ST(stream), dur, x_len, cum, y_len, logw, Tx);
  GT_RET();
}

extern "C" int gt_synth_prior_args_size(void) { return (int)sizeof(gt_synth_prior_args); }
extern "C" int gt_synth_call_size(void) { return (int)sizeof(gt_synth_call); }

extern "C" int gt_synth_geometry(const int32_t* y_len, int B, int Ty_cap, int R_cap, int32_t* row0, int32_t* len_sq, int32_t* y_len_eff,
                                 int64_t* rowbatch, int32_t* rowframe, float* rowmask, int32_t* rowutt, int32_t* status, void* stream)
{
  if (B < 0 || R_cap < 0 || Ty_cap < 0 || (Ty_cap & 1)) return GT_E_INVAL;
  if (B == 0 || R_cap == 0) return 0;
  if (B > GT_STEP_MAX_B || Ty_cap > (1 << 20)) return GT_E_UNSUPPORTED;   // 1024 utterances of 2^19 + 4 rows stay inside int32
  if (!y_len || !row0 || !len_sq || !y_len_eff || !rowbatch || !rowframe || !rowmask || !status) return GT_E_INVAL;
  if ((long long)R_cap < 2LL * HALO * B) return GT_E_INVAL;               // every utterance keeps its two halos
  if (((uintptr_t)y_len | (uintptr_t)row0 | (uintptr_t)len_sq | (uintptr_t)y_len_eff | (uintptr_t)rowframe | (uintptr_t)rowmask |
       (uintptr_t)rowutt | (uintptr_t)status) & 3) return GT_E_ALIGN;
  if ((uintptr_t)rowbatch & 7) return GT_E_ALIGN;
  hipLaunchKernelGGL(gt_synth_geometry_kernel<2>, dim3((R_cap + 255) / 256), dim3(256), 0, GT_ST(stream), y_len, B, Ty_cap, R_cap, row0,
                     len_sq, y_len_eff, rowbatch, rowframe, rowmask, rowutt, status);
  GT_RET();
}

extern "C" int gt_synth_frame_geometry(const int32_t* y_len_eff, int B, int Ty_cap, int Rf_cap, int32_t* row0_f, int32_t* len_f,
                                       int64_t* rowbatch, int32_t* rowframe, float* rowmask, int32_t* rowutt, int32_t* status, void* stream)
{
  if (B < 0 || Rf_cap < 0 || Ty_cap < 0) return GT_E_INVAL;
  if (B == 0 || Rf_cap == 0) return 0;
  if (B > GT_STEP_MAX_B || Ty_cap > (1 << 20)) return GT_E_UNSUPPORTED;   // 1024 utterances of 2^20 + 4 rows stay inside int32
  if (!y_len_eff || !row0_f || !len_f || !rowbatch || !rowframe || !rowmask || !status) return GT_E_INVAL;
  if ((long long)Rf_cap < 2LL * HALO * B) return GT_E_INVAL;              // every utterance keeps its two halos
  if (((uintptr_t)y_len_eff | (uintptr_t)row0_f | (uintptr_t)len_f | (uintptr_t)rowframe | (uintptr_t)rowmask | (uintptr_t)rowutt |
       (uintptr_t)status) & 3) return GT_E_ALIGN;
  if ((uintptr_t)rowbatch & 7) return GT_E_ALIGN;
  hipLaunchKernelGGL(gt_synth_geometry_kernel<1>, dim3((Rf_cap + 255) / 256), dim3(256), 0, GT_ST(stream), y_len_eff, B, Ty_cap, Rf_cap,
                     row0_f, len_f, (int32_t*)nullptr, rowbatch, rowframe, rowmask, rowutt, status);
  GT_RET();
}

static int synth_prior_launch(const gt_synth_prior_args* args, const gt_synth_call* call, bool from_call, bool long_form, void* stream)
{
  if (!args) return GT_E_INVAL;
  const gt_synth_prior_args& a = *args;
  if (a.R < 0 || a.B < 0) return GT_E_INVAL;
  if (a.R == 0 || a.B == 0) return 0;
  if (a.C <= 0 || a.Tx <= 0 || a.Ty <= 0 || a.Tp <= 2 * HALO) return GT_E_INVAL;
  if (a.Tx > (long_form ? SF_LONG_TX_MAX : SF_TX_MAX) || a.C > SF_C_MAX || a.B > 65535) return GT_E_UNSUPPORTED;
  if (!a.x_m || !a.cum || !a.x_len || !a.y_len || !a.rows || (from_call && !call)) return GT_E_INVAL;
  if (!a.row0 && (long long)a.B * a.Tp != a.R) return GT_E_INVAL;             // uniform rows: utterance b owns [b Tp, (b + 1) Tp)
  if (!al16(a.x_m) || !al16(a.x_logs) || !al16(a.rows) || !al16(a.z_m) || !al16(a.z_logs) || !al16(a.attn)) return GT_E_ALIGN;
  if (((uintptr_t)a.cum | (uintptr_t)a.x_len | (uintptr_t)a.y_len | (uintptr_t)a.row0 | (uintptr_t)a.frame2token | (uintptr_t)call) & 3)
    return GT_E_ALIGN;
  // row tiles over the largest utterance (Tp bounds it in the ragged layout), and frame tiles over all Ty frames of the optional outputs
  const int gx = max((a.Tp + SF_ROWS - 1) / SF_ROWS, (a.Ty + 2 * HALO + SF_FRAMES - 1) / SF_FRAMES);
  auto kernel = long_form ? (from_call ? gt_synth_prior_kernel<true, true> : gt_synth_prior_kernel<false, true>)
                          : (from_call ? gt_synth_prior_kernel<true, false> : gt_synth_prior_kernel<false, false>);
  hipLaunchKernelGGL(kernel, dim3(gx, a.B), dim3(256), 0, GT_ST(stream), a, call);
  GT_RET();
}

extern "C" int gt_synth_prior(const gt_synth_prior_args* args, void* stream) { return synth_prior_launch(args, nullptr, false, false, stream); }

extern "C" int gt_synth_prior_call(const gt_synth_prior_args* args, const gt_synth_call* call, void* stream)
{
  return synth_prior_launch(args, call, true, false, stream);
}

extern "C" int gt_synth_prior_long(const gt_synth_prior_args* args, void* stream)
{
  return synth_prior_launch(args, nullptr, false, true, stream);
}

extern "C" int gt_synth_prior_long_call(const gt_synth_prior_args* args, const gt_synth_call* call, void* stream)
{
  return synth_prior_launch(args, call, true, true, stream);
}

static int randn_rows_launch(float* out, int R, int ncol, uint32_t seed, uint32_t stream_id, float scale, const gt_synth_call* call,
                             bool from_call, int which_scale, void* stream)
{
  if (R < 0 || ncol <= 0 || (from_call && (which_scale < 0 || which_scale > 1))) return GT_E_INVAL;
  if (R == 0) return 0;
  if (!out || (from_call && !call)) return GT_E_INVAL;
  if ((uintptr_t)call & 3) return GT_E_ALIGN;
  if ((uintptr_t)out & 3) return GT_E_ALIGN;
  const long long n = (long long)R * ((ncol + 1) / 2);
  if (n > 0x7fffffffLL) return GT_E_UNSUPPORTED;
  const dim3 grid((unsigned)((n + 255) / 256));
  if (from_call)
    hipLaunchKernelGGL(gt_randn_rows_kernel<true>, grid, dim3(256), 0, GT_ST(stream), out, R, ncol, seed, stream_id, scale, call, which_scale);
  else
    hipLaunchKernelGGL(gt_randn_rows_kernel<false>, grid, dim3(256), 0, GT_ST(stream), out, R, ncol, seed, stream_id, scale, call, which_scale);
  GT_RET();
}

extern "C" int gt_randn_rows(float* out, int R, int ncol, uint32_t seed, uint32_t stream_id, float scale, void* stream)
{
  return randn_rows_launch(out, R, ncol, seed, stream_id, scale, nullptr, false, 0, stream);
}

extern "C" int gt_randn_rows_call(float* out, int R, int ncol, const gt_synth_call* call, uint32_t stream_id, int which_scale, void* stream)
{
  return randn_rows_launch(out, R, ncol, 0u, stream_id, 0.f, call, true, which_scale, stream);
}
