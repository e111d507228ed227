// Device front end of synthesis (FlowGenerator.infer with set_synthesis_front): durations -> lengths, the encoder's
// prior + a seed -> the sampled, squeezed latent in the rows layout the reverse decoder reads, and the counter-hash Gaussian draws
// of the stochastic predictors.  Plain C++: vector stores only, no atomics, every output element has exactly one writer, so the
// results are deterministic by construction.  Memory-bound; no MFMA.
#include "common.h"
#include "../../include/glowtts_hip.h"
#include "internal.h"

#define HALO GT_HALO
#define GT_ST(s) static_cast<hipStream_t>(s)
#define GT_RET() return gt_launch_status(__func__)

#define SF_TX_MAX 512        // tokens per utterance (gt_prior_expand's and gt_mas_f32's limit)
#define SF_C_MAX 80          // mel channels
#define SF_ROWS 32           // squeezed rows of one workgroup's tile ...
#define SF_FRAMES 64         // ... = frames of it
#define SF_LD (SF_FRAMES + 1)   // LDS pitch of a channel's frames: the row phase reads one channel per lane, 65 words apart
#define SF_DUR_MAX 1048576.f // a token's duration is clamped here: 512 tokens stay inside int32

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

// A workgroup owns utterance blockIdx.y and row offsets [32 k, 32 k + 32) of it = squeezed frames s in [32 k - 2, 32 k + 30) =
// frames t in [64 k - 4, 64 k + 60): the halo rows in front belong to tile 0, the halo / padding / rounding rows behind to the
// tiles they fall into, so every row has one writer.  The tokens a tile touches are a contiguous range of the utterance: their
// means / log-deviations go through LDS frame by frame (a wave reads one channel along Tx, one workgroup-wide phase later a
// wave writes rows along the channels).
__global__ __launch_bounds__(256) void gt_synth_prior_kernel(gt_synth_prior_args a)
{
  __shared__ float m_s[SF_C_MAX * SF_LD];
  __shared__ float l_s[SF_C_MAX * SF_LD];
  __shared__ int32_t cum_s[SF_TX_MAX];
  __shared__ int32_t tok_s[SF_FRAMES];
  const int b = blockIdx.y, k = blockIdx.x, tid = threadIdx.x;
  const int C = a.C, Tx = a.Tx, Ty = a.Ty;
  const int n = min(max(a.x_len[b], 0), Tx);
  const int ylen = a.y_len[b];
  for (int i = tid; i < n; i += 256) cum_s[i] = a.cum[(size_t)b * Tx + i];
  __syncthreads();
  const int t0 = k * SF_FRAMES - 2 * HALO;
  if (tid < SF_FRAMES) {
    const int t = t0 + tid;
    int tok = -1;                                       // commons.generate_path: the first token whose cumulative duration passes t
    if (t >= 0 && t < ylen && n > 0 && t < cum_s[n - 1]) {
      int lo = 0, hi = n - 1;
      while (lo < hi) { const int mid = (lo + hi) >> 1; if (cum_s[mid] > t) hi = mid; else lo = mid + 1; }
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
  const uint32_t key = randn_key(a.seed, 0u, (uint32_t)b);
  const float ns = a.noise_scale;
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

__global__ __launch_bounds__(256) void gt_randn_rows_kernel(float* __restrict__ out, int R, int ncol, uint32_t seed, uint32_t stream_id,
                                                            float scale)
{
  const int np = (ncol + 1) >> 1;
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= R * np) return;
  const int row = idx / np, p = idx - row * np;
  float e0, e1;
  randn_pair(randn_key(seed, stream_id, 0u), (uint32_t)row, (uint32_t)p, e0, e1);
  out[(size_t)row * ncol + 2 * p] = e0 * scale;
  if (2 * p + 1 < ncol) out[(size_t)row * ncol + 2 * p + 1] = e1 * scale;
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

extern "C" int gt_synth_prior_args_size(void) { return (int)sizeof(gt_synth_prior_args); }

extern "C" int gt_synth_prior(const gt_synth_prior_args* args, void* stream)
{
  if (!args) return GT_E_INVAL;
  const gt_synth_prior_args& a = *args;
  if (a.R < 0 || a.B < 0) return GT_E_INVAL;
  if (a.R == 0 || a.B == 0) return 0;
  if (a.C <= 0 || a.Tx <= 0 || a.Ty <= 0 || a.Tp <= 2 * HALO) return GT_E_INVAL;
  if (a.Tx > SF_TX_MAX || a.C > SF_C_MAX || a.B > 65535) return GT_E_UNSUPPORTED;
  if (!a.x_m || !a.cum || !a.x_len || !a.y_len || !a.rows) return GT_E_INVAL;
  if (!a.row0 && (long long)a.B * a.Tp != a.R) return GT_E_INVAL;             // uniform rows: utterance b owns [b Tp, (b + 1) Tp)
  if (!al16(a.x_m) || !al16(a.x_logs) || !al16(a.rows) || !al16(a.z_m) || !al16(a.z_logs) || !al16(a.attn)) return GT_E_ALIGN;
  if (((uintptr_t)a.cum | (uintptr_t)a.x_len | (uintptr_t)a.y_len | (uintptr_t)a.row0 | (uintptr_t)a.frame2token) & 3) return GT_E_ALIGN;
  // row tiles over the largest utterance (Tp bounds it in the ragged layout), and frame tiles over all Ty frames of the optional outputs
  const int gx = max((a.Tp + SF_ROWS - 1) / SF_ROWS, (a.Ty + 2 * HALO + SF_FRAMES - 1) / SF_FRAMES);
  hipLaunchKernelGGL(gt_synth_prior_kernel, dim3(gx, a.B), dim3(256), 0, GT_ST(stream), a);
  GT_RET();
}

extern "C" int gt_randn_rows(float* out, int R, int ncol, uint32_t seed, uint32_t stream_id, float scale, void* stream)
{
  if (R < 0 || ncol <= 0) return GT_E_INVAL;
  if (R == 0) return 0;
  if (!out) return GT_E_INVAL;
  if ((uintptr_t)out & 3) return GT_E_ALIGN;
  const long long n = (long long)R * ((ncol + 1) / 2);
  if (n > 0x7fffffffLL) return GT_E_UNSUPPORTED;
  hipLaunchKernelGGL(gt_randn_rows_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, GT_ST(stream), out, R, ncol, seed, stream_id,
                     scale);
  GT_RET();
}
