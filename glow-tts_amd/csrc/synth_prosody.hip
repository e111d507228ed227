// Full-model synthesis (stochastic duration / pitch / energy predictors): the predictors' Gaussian draws keyed by
// (utterance, token or frame) instead of by row index — a draw no longer depends on how the batch is laid out, so a graph captured at
// capacity sizes, the eager call and the overflow fallback all see the same noise — and the predicted contours written straight into
// the rows the reverse decoder reads.  Plain C++: vector stores only, no atomics, every output element has exactly one writer.
// Memory-bound; no MFMA.
#include "common.h"
#include "../../include/glowtts_hip.h"
#include "internal.h"

#define HALO GT_HALO

// One thread per (row, column pair).  The row's utterance comes from a binary search over row0 (uniform rows: a division).
// CALL: seed / scale come from the gt_synth_call_ext block in device memory; the only difference between the two instantiations.
template <bool CALL>
__global__ __launch_bounds__(256) void gt_randn_keyed_kernel(float* __restrict__ out, const int32_t* __restrict__ row0, int Tp,
                                                             const int32_t* __restrict__ lengths, int B, int R, int ncol, uint32_t seed,
                                                             uint32_t stream_id, float scale, const gt_synth_call_ext* __restrict__ call,
                                                             int which_scale)
{
  if (CALL) {
    seed = call->base.seed;
    scale = which_scale == 0 ? call->base.noise_scale
          : which_scale == 1 ? call->base.noise_scale_w
          : which_scale == 2 ? call->f0_noise_scale : call->energy_noise_scale;
  }
  const int np = (ncol + 1) >> 1;
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= R * np) return;
  const int row = idx / np, p = idx - row * np;
  const int b = min(gt_row_batch(row0, B, row, Tp), B - 1);
  const int t = row - gt_row_base(row0, b, Tp) - HALO;
  float v0 = 0.f, v1 = 0.f;
  if (t >= 0 && t < lengths[b] && t < gt_row_count(row0, b, Tp) - 2 * HALO) {      // not a halo / padding / rounding row
    float e0, e1;
    randn_pair(randn_key(seed, stream_id, (uint32_t)b), (uint32_t)t, (uint32_t)p, e0, e1);
    v0 = e0 * scale;
    v1 = e1 * scale;
  }
  out[(size_t)row * ncol + 2 * p] = v0;
  if (2 * p + 1 < ncol) out[(size_t)row * ncol + 2 * p + 1] = v1;
}

struct contours_args {
  const float* pitch_rows; const float* energy_rows;       // [Rf] predictor outputs on the frame-rate rows, either NULL
  const int32_t* row0_f; int Tp_f; const int32_t* len_f; int Rf;
  const int32_t* row0; int Tp; const int32_t* len_sq; int R;
  float* psig; float* esig;                                // [R, 2]
  float* pitch; float* energy;                             // [B, Ty]
  int B, Ty;
  float pitch_scale, energy_scale;
};

// Thread i writes squeezed row i of psig / esig (both parities: one 8-byte store each) and element i of pitch / energy [B, Ty]:
// contour[b, t] = rows[row of frame t] * scale for t < len_f[b], 0 behind it — what from_rows -> * scale gives — and
// sig[r, j] = contour[b, 2 s + j] for the row r of squeezed frame s < len_sq[b] (gt_squeeze_rows_f32 with one channel).
template <bool CALL>
__global__ __launch_bounds__(256) void gt_synth_contours_kernel(contours_args a, const gt_synth_call_ext* __restrict__ call)
{
  const float ps = CALL ? call->pitch_scale : a.pitch_scale;
  const float es = CALL ? call->energy_scale : a.energy_scale;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < a.R) {
    const int b = min(gt_row_batch(a.row0, a.B, i, a.Tp), a.B - 1);
    const int s = i - gt_row_base(a.row0, b, a.Tp) - HALO;
    const int nf = min(a.len_f[b], a.Ty), T2 = a.Ty >> 1;
    const int src = gt_row_base(a.row0_f, b, a.Tp_f) + HALO + 2 * s;
    const bool in0 = s >= 0 && s < a.len_sq[b] && s < T2;
    const bool ok0 = in0 && 2 * s < nf && src < a.Rf, ok1 = in0 && 2 * s + 1 < nf && src + 1 < a.Rf;
    if (a.psig) {
      float2 v;
      v.x = (ok0 && a.pitch_rows) ? a.pitch_rows[src] * ps : 0.f;
      v.y = (ok1 && a.pitch_rows) ? a.pitch_rows[src + 1] * ps : 0.f;
      *reinterpret_cast<float2*>(a.psig + 2 * (size_t)i) = v;
    }
    if (a.esig) {
      float2 v;
      v.x = (ok0 && a.energy_rows) ? a.energy_rows[src] * es : 0.f;
      v.y = (ok1 && a.energy_rows) ? a.energy_rows[src + 1] * es : 0.f;
      *reinterpret_cast<float2*>(a.esig + 2 * (size_t)i) = v;
    }
  }
  if (i < a.B * a.Ty) {
    const int b = i / a.Ty, t = i - b * a.Ty;
    const int src = gt_row_base(a.row0_f, b, a.Tp_f) + HALO + t;
    const bool ok = t < a.len_f[b] && src < a.Rf;
    if (a.pitch) a.pitch[i] = (ok && a.pitch_rows) ? a.pitch_rows[src] * ps : 0.f;
    if (a.energy) a.energy[i] = (ok && a.energy_rows) ? a.energy_rows[src] * es : 0.f;
  }
}

extern "C" int gt_synth_call_ext_size(void) { return (int)sizeof(gt_synth_call_ext); }

static int randn_keyed_launch(float* out, const int32_t* row0, int Tp, const int32_t* lengths, int B, int R, int ncol, uint32_t seed,
                              uint32_t stream_id, float scale, const gt_synth_call_ext* call, bool from_call, int which_scale, void* stream)
{
  if (R < 0 || B < 0 || ncol <= 0 || (from_call && (which_scale < 0 || which_scale > 3))) return GT_E_INVAL;
  if (R == 0) return 0;
  if (!out || !lengths || B == 0 || (from_call && !call)) return GT_E_INVAL;
  if (!row0 && (Tp < 2 * HALO || (long long)B * Tp != R)) return GT_E_INVAL;     // uniform rows: utterance b owns [b Tp, (b + 1) Tp)
  if (((uintptr_t)call | (uintptr_t)out | (uintptr_t)row0 | (uintptr_t)lengths) & 3) return GT_E_ALIGN;
  const long long n = (long long)R * ((ncol + 1) / 2);
  if (n > 0x7fffffffLL) return GT_E_UNSUPPORTED;
  const dim3 grid((unsigned)((n + 255) / 256));
  if (from_call)
    hipLaunchKernelGGL(gt_randn_keyed_kernel<true>, grid, dim3(256), 0, GT_ST(stream), out, row0, Tp, lengths, B, R, ncol, seed, stream_id,
                       scale, call, which_scale);
  else
    hipLaunchKernelGGL(gt_randn_keyed_kernel<false>, grid, dim3(256), 0, GT_ST(stream), out, row0, Tp, lengths, B, R, ncol, seed, stream_id,
                       scale, call, which_scale);
  GT_RET();
}

extern "C" int gt_randn_keyed(float* out, const int32_t* row0, int Tp, const int32_t* lengths, int B, int R, int ncol, uint32_t seed,
                              uint32_t stream_id, float scale, void* stream)
{
  return randn_keyed_launch(out, row0, Tp, lengths, B, R, ncol, seed, stream_id, scale, nullptr, false, 0, stream);
}

extern "C" int gt_randn_keyed_call(float* out, const int32_t* row0, int Tp, const int32_t* lengths, int B, int R, int ncol,
                                   const gt_synth_call_ext* call, uint32_t stream_id, int which_scale, void* stream)
{
  return randn_keyed_launch(out, row0, Tp, lengths, B, R, ncol, 0u, stream_id, 0.f, call, true, which_scale, stream);
}

static int contours_launch(const contours_args& a, const gt_synth_call_ext* call, bool from_call, void* stream)
{
  if (a.R < 0 || a.Rf < 0 || a.B < 0 || a.Ty < 0) return GT_E_INVAL;
  if (a.B == 0 || (a.R == 0 && a.Ty == 0)) return 0;
  if (!a.len_f || !a.len_sq || (from_call && !call)) return GT_E_INVAL;
  if ((a.pitch_rows || a.energy_rows) && a.Rf == 0) return GT_E_INVAL;
  if (!a.row0_f && (a.Tp_f < 2 * HALO || (long long)a.B * a.Tp_f != a.Rf)) return GT_E_INVAL;
  if (!a.row0 && (a.Tp < 2 * HALO || (long long)a.B * a.Tp != a.R)) return GT_E_INVAL;
  if (((uintptr_t)a.pitch_rows | (uintptr_t)a.energy_rows | (uintptr_t)a.row0_f | (uintptr_t)a.len_f | (uintptr_t)a.row0 |
       (uintptr_t)a.len_sq | (uintptr_t)a.pitch | (uintptr_t)a.energy | (uintptr_t)call) & 3) return GT_E_ALIGN;
  if (((uintptr_t)a.psig | (uintptr_t)a.esig) & 7) return GT_E_ALIGN;            // a row's two parities are one 8-byte store
  const long long n = max((long long)a.R, (long long)a.B * a.Ty);
  if (n > 0x7fffffffLL) return GT_E_UNSUPPORTED;
  if (n == 0) return 0;
  const dim3 grid((unsigned)((n + 255) / 256));
  if (from_call) hipLaunchKernelGGL(gt_synth_contours_kernel<true>, grid, dim3(256), 0, GT_ST(stream), a, call);
  else hipLaunchKernelGGL(gt_synth_contours_kernel<false>, grid, dim3(256), 0, GT_ST(stream), a, call);
  GT_RET();
}

extern "C" int gt_synth_contours(const float* pitch_rows, const float* energy_rows, const int32_t* row0_f, int Tp_f, const int32_t* len_f,
                                 int Rf, const int32_t* row0, int Tp, const int32_t* len_sq, int R, float* psig, float* esig, float* pitch,
                                 float* energy, int B, int Ty, float pitch_scale, float energy_scale, void* stream)
{
  const contours_args a = {pitch_rows, energy_rows, row0_f, Tp_f, len_f, Rf, row0, Tp, len_sq, R, psig, esig, pitch, energy, B, Ty,
                           pitch_scale, energy_scale};
  return contours_launch(a, nullptr, false, stream);
}

extern "C" int gt_synth_contours_call(const float* pitch_rows, const float* energy_rows, const int32_t* row0_f, int Tp_f,
                                      const int32_t* len_f, int Rf, const int32_t* row0, int Tp, const int32_t* len_sq, int R, float* psig,
                                      float* esig, float* pitch, float* energy, int B, int Ty, const gt_synth_call_ext* call, void* stream)
{
  const contours_args a = {pitch_rows, energy_rows, row0_f, Tp_f, len_f, Rf, row0, Tp, len_sq, R, psig, esig, pitch, energy, B, Ty, 0.f, 0.f};
  return contours_launch(a, call, true, stream);
}
