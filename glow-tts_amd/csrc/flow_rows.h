// The row-local maths of a flow block: ActNorm + InvConvNear on a (row, channel group), the affine coupling on an element, the
// parameter-gradient fold and the log-det bookkeeping, for the five-launch kernels (flow_ops.hip) and the fused between-WaveNet kernels
// (wn_boundary.hip).  Who forms exp(logs) (per item there, per thread here), where the operands come from and which rows a thread walks
// stay with the caller: every leaf takes the precomputed values, in the expression shape and operation order its callers had.
// Two texts exist a second time, in gt_wn_boundary_bwd_kernel, each with its reason there: actnorm_invconv_bwd and unsq_scatter_group.
#pragma once
#include "common.h"

namespace fr {

// channel group g -> its four members {2g, 2g+1, half+2g, half+2g+1}
__device__ __forceinline__ void group_channels(int g, int half, int (&ch)[4]) { ch[0] = 2 * g; ch[1] = 2 * g + 1; ch[2] = half + 2 * g; ch[3] = half + 2 * g + 1; }

// ---- affine coupling (attentions.py:171-186) on one element; lg = the log-scale after sigmoid_scale (ONE test for an item's N elements)
template <int N>
__device__ __forceinline__ void coupling_lg(float (&lg)[N], int sigmoid_scale)
{
  if (sigmoid_scale) {
#pragma unroll
    for (int j = 0; j < N; ++j) lg[j] = __logf(1e-6f + sigmoidf_(lg[j] + 2.0f));
  }
}
__device__ __forceinline__ float coupling_lg(float raw, int sigmoid_scale) { float lg[1] = {raw}; coupling_lg(lg, sigmoid_scale); return lg[0]; }
__device__ __forceinline__ float coupling_lg(float raw, int sigmoid_scale, float& dl_draw)   // one element, also d lg / d raw
{
  float lg = raw;
  dl_draw = 1.0f;
  if (sigmoid_scale) { const float sg = sigmoidf_(raw + 2.0f); lg = __logf(1e-6f + sg); dl_draw = sg * (1.0f - sg) / (1e-6f + sg); }
  return lg;
}
__device__ __forceinline__ float coupling_fwd(float m, float lg, float y1, float rm) { return (m + __expf(lg) * y1) * rm; }
__device__ __forceinline__ float coupling_inv(float m, float lg, float z1, float rm) { return (z1 - m) * __expf(-lg) * rm; }
// dz1 and dld (= d logdet of the row's utterance) already carry the row mask; d m = dz1
__device__ __forceinline__ void coupling_bwd(float dz1, float lg, float dl_draw, float y1, float dld, float& dx1, float& dlg)
{
  const float e = __expf(lg);
  dx1 = dz1 * e;
  dlg = (dz1 * e * y1 + dld) * dl_draw;
}

// ---- ActNorm + InvConvNear (modules.py:584-599, 635-665) on one (row, group): xv = the group's four members, el = exp(logs), bs = bias
// of those channels, W the 4x4 weight row major (a register array or the global pointer)
template <class Wt>
__device__ __forceinline__ void actnorm_invconv_fwd(const float (&xv)[4], const float (&el)[4], const float (&bs)[4], const Wt& W, float rm, float (&o)[4])
{
  const float a0 = bs[0] + el[0] * xv[0], a1 = bs[1] + el[1] * xv[1], a2 = bs[2] + el[2] * xv[2], a3 = bs[3] + el[3] * xv[3];
#pragma unroll
  for (int q = 0; q < 4; ++q) o[q] = (W[q * 4] * a0 + W[q * 4 + 1] * a1 + W[q * 4 + 2] * a2 + W[q * 4 + 3] * a3) * rm;
}
// inverse: x = ((W^-1 u) mask - bias) exp(-logs) mask;  Wi = scal + 2 (W^-T row major: W^-1[k][j] = Wi[4 j + k]), eli = exp(-logs).
// FROM_ZERO: the four products are added to a sum that starts at 0 (gt_actnorm_invconv_rev: each contracts into an FMA) instead of to
// one another (gt_wn_boundary_rev: the first stays a product); the two kernels have always differed in that rounding, and keep it
template <bool FROM_ZERO, class Wt>
__device__ __forceinline__ void actnorm_invconv_inv(const float (&uv)[4], const float (&eli)[4], const float (&bs)[4], const Wt& Wi, float rm, float (&o)[4])
{
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    float a = 0.f;
    if (FROM_ZERO) {
#pragma unroll
      for (int j = 0; j < 4; ++j) a += Wi[4 * j + q] * uv[j];
    } else a = Wi[q] * uv[0] + Wi[4 + q] * uv[1] + Wi[8 + q] * uv[2] + Wi[12 + q] * uv[3];
    o[q] = a * rm;
  }
#pragma unroll
  for (int q = 0; q < 4; ++q) o[q] = (o[q] - bs[q]) * eli[q] * rm;
}
// backward: dym = d y (masked); d x -> dxv, the row's terms added to accW (d W), accL (d logs), accB (d bias)
template <class Wt>
__device__ __forceinline__ void actnorm_invconv_bwd(const float (&xv)[4], const float (&dym)[4], const float (&el)[4], const float (&bs)[4], const Wt& W,
                                                    float (&accW)[16], float (&accL)[4], float (&accB)[4], float (&dxv)[4])
{
  float av[4], d_a[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) av[k] = bs[k] + el[k] * xv[k];
#pragma unroll
  for (int i = 0; i < 4; ++i) d_a[i] = W[i] * dym[0] + W[4 + i] * dym[1] + W[8 + i] * dym[2] + W[12 + i] * dym[3];
#pragma unroll
  for (int o = 0; o < 4; ++o)
#pragma unroll
    for (int i = 0; i < 4; ++i) accW[o * 4 + i] += dym[o] * av[i];
#pragma unroll
  for (int k = 0; k < 4; ++k) { accB[k] += d_a[k]; accL[k] += d_a[k] * xv[k] * el[k]; dxv[k] = d_a[k] * el[k]; }
}

// ---- parameter-gradient fold of a 256-thread workgroup: wave = row phase ph, lane = group g.  sL, sB [4][64][4], sW [4][16] in LDS.
// Same-address float atomics serialise at L2: the four row phases are folded first, so every channel sees ONE add per workgroup.
__device__ __forceinline__ void param_fold(float* sL, float* sB, float* sW, int ph, int g, const float (&accL)[4], const float (&accB)[4], float (&accW)[16])
{
#pragma unroll
  for (int k = 0; k < 4; ++k) { sL[(ph * 64 + g) * 4 + k] = accL[k]; sB[(ph * 64 + g) * 4 + k] = accB[k]; }
#pragma unroll
  for (int i = 0; i < 16; ++i) accW[i] = wave_sum(accW[i]);
  if (g == 0) {
#pragma unroll
    for (int i = 0; i < 16; i += 4) *reinterpret_cast<float4*>(sW + ph * 16 + i) = make_float4(accW[i], accW[i + 1], accW[i + 2], accW[i + 3]);   // sW: 16-byte aligned
  }
}
__device__ __forceinline__ float fold4(const float* s, int g, int k) { return s[g * 4 + k] + s[(64 + g) * 4 + k] + s[(128 + g) * 4 + k] + s[(192 + g) * 4 + k]; }
__device__ __forceinline__ float fold4W(const float* sW, int i) { return sW[i] + sW[16 + i] + sW[32 + i] + sW[48 + i]; }
// after the barrier behind param_fold: one atomic per channel and workgroup
__device__ __forceinline__ void param_fold_atomics(float* dlogs, float* dbias, float* dW, const float* sL, const float* sB,
                                                   const float* sW, int ph, int g, int G, int half)
{
  if (ph == 0 && g < G) {
    int ch[4];
    group_channels(g, half, ch);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      atomicAdd(dlogs + ch[k], fold4(sL, g, k));
      atomicAdd(dbias + ch[k], fold4(sB, g, k));
    }
  }
  if (threadIdx.x < 16) atomicAdd(dW + threadIdx.x, fold4W(sW, threadIdx.x));
}

// ---- log-det bookkeeping of an ActNorm + InvConvNear pair: logdet[b] += (sum logs + G logdet W) len_b; scal = {sum logs, logdet W, W^-T}.
// Backward, by a whole 256-thread workgroup (one barrier inside; sred: 4 floats of LDS): s = sum_b dlogdet[b] len_b, d logs += s, d W += G s W^-T
__device__ __forceinline__ float pair_logdet_per_frame(const float* scal, int G) { return scal[0] + (float)G * scal[1]; }
__device__ __forceinline__ float dlogdet_len_sum(const float* dlogdet, const int32_t* len, int B, float* sred)
{
  float sv = 0.f;
  for (int b = threadIdx.x; b < B; b += 256) sv += dlogdet[b] * (float)len[b];
  sv = wave_sum(sv);
  if ((threadIdx.x & 63) == 0) sred[threadIdx.x >> 6] = sv;
  __syncthreads();
  return sred[0] + sred[1] + sred[2] + sred[3];
}
__device__ __forceinline__ void pair_logdet_bwd_atomics(float* dlogs, float* dW, const float* scal, float sv, int C)
{
  for (int c = threadIdx.x; c < C; c += 256) atomicAdd(dlogs + c, sv);
  if (threadIdx.x < 16) atomicAdd(dW + threadIdx.x, (float)(C >> 2) * sv * scal[2 + threadIdx.x]);
}

// ---- commons.squeeze / unsqueeze (commons.py:339-364, n_sqz = 2) folded into the first / last kernels of a pass: squeezed frame t of
// utterance b, channel p * half + c  <->  y[b, c, 2 t + p] of the [B, half, T] tensor at the decoder's public boundary
__device__ __forceinline__ float4 sq_gather4(const float* __restrict__ y, int b, int t, int c, int T, int half)
{
  const int p = c >= half, cc = c - half * p;
  const float* src = y + ((size_t)b * half + cc) * T + 2 * t + p;
  return make_float4(src[0], src[(size_t)T], src[2 * (size_t)T], src[3 * (size_t)T]);
}
__device__ __forceinline__ void sq_scatter4(float* __restrict__ y, int b, int t, int c, int T, int half, const float4& v)
{
  const int p = c >= half, cc = c - half * p;
  float* dst = y + ((size_t)b * half + cc) * T + 2 * t + p;
  dst[0] = v.x; dst[(size_t)T] = v.y; dst[2 * (size_t)T] = v.z; dst[3 * (size_t)T] = v.w;
}
// a group's four members: channels 2g, 2g+1 at frames 2t (members 0, 1) and 2t + 1 (members 2, 3)
__device__ __forceinline__ void unsq_scatter_group(float* y, int b, int t, int g, int T, int half, const float (&o)[4])
{
  float* d0 = y + ((size_t)b * half + 2 * g) * T + 2 * t;
  d0[0] = o[0]; d0[(size_t)T] = o[1]; d0[1] = o[2]; d0[(size_t)T + 1] = o[3];
}

}  // namespace fr
