// BigVGAN's anti-aliased periodic activation on the device: ONE stand-alone, memory-bound kernel — 2x up-sampling FIR,
// snake, 2x down-sampling FIR per channel — from the fp32 residual stream to the bf16 operand the next gt_voc_conv reads (x_bf16).
//
//   definition  on each utterance's own [0, len), len = min(max(n_frames[b], 0) len_mul, L_cap), with cl(i) = min(max(i, 0), len - 1):
//                 u[2q]   = 2 sum_{j < 6} fu[11 - 2j] x[cl(q - 3 + j)]          u[2q + 1] = 2 sum_{j < 6} fu[10 - 2j] x[cl(q - 2 + j)]
//                 v[i]    = u[i] + ib sin^2(a u[i])                              a = alpha', ib = 1 / (beta' + 1e-9): P's, per channel
//                 y[t]    = sum_{k < 12} fd[k] v[min(max(2t + k - 5, 0), 2 len - 1)]
//               TWO clamps: x is replicated at the utterance's ends (cl), and so is v — its INDEX is clamped into [0, 2 len - 1]; v is
//               never evaluated at an index outside that range from a clamped x.  Outputs at [len, L_cap) are written as bf16 zero.
//   pairs       v[2m - 1] and v[2m] read the same six inputs x[cl(m - 3 .. m + 2)]: a thread walks m upwards, slides that window by one
//               load per step and forms the pair (vo, ve); pair m feeds the six outputs t = m + 2 .. m - 3 as their taps k = 0, 1 ..
//               10, 11, so each y[t] is one fmaf chain in k ascending held in a register while its twelve v arrive, and every v is
//               computed once per strip.  At the ends: pair 0 is (v[0], v[0]), pair len is (v[2 len - 1], v[2 len - 1]), a pair below 0 /
//               above len repeats that one.
//   shape       lanes along channels, two channels per thread (one 8-byte load, one 4-byte store per position: sixteen lanes cover a
//               128-byte line); a thread owns a strip of S = 16 consecutive positions of its two channels and re-reads the 5-position
//               halo on either side (26 loads for 16 outputs, the halo out of L2 / L1).  A workgroup is 16 strips x 16 channel groups
//               (8 at C = 16): TM = 256 positions x 32 channels.  Two loads ahead of their use are in flight per thread; 93 registers
//               (four sinf in flight), five waves per SIMD — four channels per thread took 169.  No LDS, no barrier.
//   order       fp32 fmaf chains: j ascending for u, k ascending for y, one rounding to bf16 (nearest even) at the end; fixed by (t, c)
//               alone — a batch row is bit-identical to the utterance computed alone, in a buffer of any capacity.
//   sine        the device library's sinf (<= 2 ulp over the whole range): the hardware sine takes revolutions, and the reduction
//               a u / 2 pi in fp32 costs an absolute 2^-24 |a u| / 2 pi revolutions on top of its own error, at |a u| in the hundreds
//               more than everything else in the bound together.  No exp, no division.
//   bounds      every load is at a clamped position in [0, len) and a channel < C; every store at a position < L_cap and a channel < C;
//               all offsets are size_t.
#include "common.h"
#include "internal.h"
#include "../../include/glowtts_hip.h"

namespace {

constexpr int S = 16;                                    // positions per strip
constexpr int STRIPS = 16;                               // strips per workgroup
constexpr int TM = S * STRIPS;                           // positions per workgroup
constexpr int V = 2;                                     // channels per thread
constexpr int CB = 32;                                   // channels per workgroup: 16 groups of V

struct xv { float e[V]; };
__device__ __forceinline__ xv ldv(const float* p) { xv r; const float2 q = *reinterpret_cast<const float2*>(p); r.e[0] = q.x; r.e[1] = q.y; return r; }

__device__ __forceinline__ float snake(float u, float a, float ib)
{
  const float s = sinf(a * u);
  return fmaf(ib, s * s, u);
}

__global__ __launch_bounds__(256) void gt_voc_snake_kernel(const gt_voc_snake_args a)
{
  const int G = blockDim.x / STRIPS;                      // channel groups of this launch: min(C, CB) / V
  const int cg = threadIdx.x % G, strip = threadIdx.x / G;
  const int c = blockIdx.y * CB + cg * V, b = blockIdx.z;
  const int t0 = blockIdx.x * TM + strip * S;
  if (c >= a.C || t0 >= a.L_cap) return;
  int nf = a.n_frames[b];
  nf = nf > 0 ? nf : 0;
  const long long len64 = (long long)nf * a.len_mul;
  const int len = len64 < a.L_cap ? (int)len64 : a.L_cap;
  const size_t C = (size_t)a.C;
  bf16_t* __restrict__ y = static_cast<bf16_t*>(a.Y) + (size_t)b * (size_t)a.y_stride_b + c;
  const int t_end = t0 + S < a.L_cap ? t0 + S : a.L_cap;

  if (t0 >= len) {                                        // behind the utterance: zeros, nothing is read
    for (int t = t0; t < t_end; ++t) *reinterpret_cast<uint32_t*>(y + (size_t)t * C) = 0u;
    return;
  }
  const float* __restrict__ x = a.X + (size_t)b * (size_t)a.x_stride_b + c;
  const float* __restrict__ P = a.P;
  float al[V], ib[V];
#pragma unroll
  for (int i = 0; i < V; ++i) { al[i] = P[c + i]; ib[i] = P[C + c + i]; }
  float fo[6], fe[6], fd[12];                             // uniform: scalar registers
#pragma unroll
  for (int j = 0; j < 6; ++j) { fo[j] = 2.f * P[2 * C + 10 - 2 * j]; fe[j] = 2.f * P[2 * C + 11 - 2 * j]; }
#pragma unroll
  for (int k = 0; k < 12; ++k) fd[k] = P[2 * C + 12 + k];

  const int last = len - 1;
  auto cl = [last](int i) { return i < 0 ? 0 : (i > last ? last : i); };
  auto xat = [&](int i) { return ldv(x + (size_t)cl(i) * C); };
  // (vo, ve) of the window w = x[cl(m - 3 .. m + 2)], j ascending
  auto pair = [&](const xv (&w)[6], float (&vo)[V], float (&ve)[V]) {
    float uo[V], ue[V];
#pragma unroll
    for (int j = 0; j < 6; ++j) {
      const float* wj = w[j].e;
#pragma unroll
      for (int i = 0; i < V; ++i) {
        uo[i] = j ? fmaf(fo[j], wj[i], uo[i]) : fo[0] * wj[i];
        ue[i] = j ? fmaf(fe[j], wj[i], ue[i]) : fe[0] * wj[i];
      }
    }
#pragma unroll
    for (int i = 0; i < V; ++i) { vo[i] = snake(uo[i], al[i], ib[i]); ve[i] = snake(ue[i], al[i], ib[i]); }
  };

  xv w[6];
  float vo[V], ve[V];
  float v0[V] = {};
  if (t0 == 0) {                                          // the utterance's first strip: pairs -2 and -1 repeat v[0]
#pragma unroll
    for (int j = 0; j < 6; ++j) w[j] = xat(j - 3);
    pair(w, vo, v0);
  }
  int m = t0 - 2;
#pragma unroll
  for (int j = 0; j < 6; ++j) w[j] = xat(m - 3 + j);
  xv p0 = xat(m + 3), p1 = xat(m + 4);                // the next two window entries, in flight
  float acc[6][V];
#pragma unroll
  for (int d = 0; d < 6; ++d)
#pragma unroll
    for (int i = 0; i < V; ++i) acc[d][i] = 0.f;

#pragma unroll 1
  for (int it = 0; it < S + 5; ++it, ++m) {
    const xv p2 = xat(m + 5);
    if (m <= len) {                                       // above len: the pair of len stays
      pair(w, vo, ve);
      if (m <= 0) {
#pragma unroll
        for (int i = 0; i < V; ++i) { ve[i] = m < 0 ? v0[i] : ve[i]; vo[i] = ve[i]; }
      }
      if (m == len) {
#pragma unroll
        for (int i = 0; i < V; ++i) ve[i] = vo[i];
      }
    }
    // pair m holds taps 2d, 2d + 1 of output t = m + 2 - d
#pragma unroll
    for (int d = 0; d < 6; ++d)
#pragma unroll
      for (int i = 0; i < V; ++i) acc[d][i] = fmaf(fd[2 * d + 1], ve[i], fmaf(fd[2 * d], vo[i], acc[d][i]));
    const int t = m - 3;                                  // complete
    if (t >= t0 && t < t_end) {
      const bool in = t < len;
      *reinterpret_cast<uint32_t*>(y + (size_t)t * C) = in ? pack2bf(acc[5][0], acc[5][1]) : 0u;
    }
#pragma unroll
    for (int d = 5; d > 0; --d)
#pragma unroll
      for (int i = 0; i < V; ++i) acc[d][i] = acc[d - 1][i];
#pragma unroll
    for (int i = 0; i < V; ++i) acc[0][i] = 0.f;
#pragma unroll
    for (int j = 0; j < 5; ++j) w[j] = w[j + 1];
    w[5] = p0; p0 = p1; p1 = p2;
  }
}

}  // namespace

extern "C" int gt_voc_snake_tile_positions(void) { return TM; }
extern "C" int gt_voc_snake_args_size(void) { return (int)sizeof(gt_voc_snake_args); }

extern "C" int gt_voc_snake(const gt_voc_snake_args* args, void* stream)
{
  if (!args) return GT_E_INVAL;
  const gt_voc_snake_args& a = *args;
  if (!a.X || !a.Y || !a.P || !a.n_frames) return GT_E_INVAL;
  if (a.B <= 0 || a.L_cap <= 0 || a.C <= 0 || a.len_mul <= 0) return GT_E_INVAL;
  if (a.x_stride_b < (long long)a.L_cap * a.C || a.y_stride_b < (long long)a.L_cap * a.C) return GT_E_INVAL;
  if (a.Y == (const void*)a.X) return GT_E_INVAL;
  if (a.C % 16 || a.B > 65535) return GT_E_UNSUPPORTED;
  if ((long long)a.B * a.L_cap * a.C >= (1ll << 31)) return GT_E_UNSUPPORTED;
  if (!al16(a.X) || ((uintptr_t)a.Y & 7) || ((uintptr_t)a.P & 3) || ((uintptr_t)a.n_frames & 3)) return GT_E_ALIGN;
  if ((a.x_stride_b & 7) || (a.y_stride_b & 7)) return GT_E_ALIGN;
  const int G = (a.C < CB ? a.C : CB) / V;
  const dim3 grid((a.L_cap + TM - 1) / TM, (a.C + CB - 1) / CB, a.B);
  hipLaunchKernelGGL(gt_voc_snake_kernel, grid, dim3(G * STRIPS), 0, static_cast<hipStream_t>(stream), a);
  return gt_launch_status("gt_voc_snake");
}
