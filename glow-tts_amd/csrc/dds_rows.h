// Row arithmetic of a DilatedDepthSeparableConv layer (modules.py:718-735) shared by the per-op kernels of predictor_ops.hip and the
// fused layer kernels of dds_layer.hip: "one wave walks rows, a lane owns C/64 channels" at C = 192.
#pragma once
#include "common.h"

namespace gtdds {

constexpr int PC = 192;                       // channels of every predictor network (filter_channels = in_channels, models.py:223)
constexpr int NC = PC / 64;                   // channels per lane

// parameter-gradient partial of this lane, the four waves' values folded in LDS first (same-address float atomics serialise at L2,
// ~25-50 ns each; with one per wave they were most of these kernels); the workgroup's sum goes to its row of a partials buffer (plain
// store: gt_param_partials_reduce adds the column sums of all rows to the parameter gradients in one launch per module backward) if
// there is one, else to dst with one atomic
__device__ __forceinline__ void wg_fold_out(float* __restrict__ dst, float* __restrict__ part, float v, float* sm, int lane, int wave)
{
  sm[wave * 64 + lane] = v;
  __syncthreads();
  if (wave == 0) {
    const float s = sm[lane] + sm[64 + lane] + sm[128 + lane] + sm[192 + lane];
    if (part) *part = s;
    else if (s != 0.f) atomicAdd(dst, s);
  }
  __syncthreads();
}

__device__ __forceinline__ float gelu_f(float x) { return 0.5f * x * (1.0f + erff(x * 0.70710678118654752f)); }
__device__ __forceinline__ float gelu_grad(float x)
{
  return 0.5f * (1.0f + erff(x * 0.70710678118654752f)) + x * 0.3989422804014327f * __expf(-0.5f * x * x);
}
__device__ __forceinline__ void ld3(const float* p, int lane, float (&v)[NC])
{
#pragma unroll
  for (int j = 0; j < NC; ++j) v[j] = p[lane + 64 * j];
}
// bf16x3 operand of a split GEMM (gt_pack_conv_weights flag 8): row = [hi | hi | lo], each PC wide
__device__ __forceinline__ void split3_store(bf16_t* row, int c, float v)
{
  const bf16_t hi = f2bf(v);
  row[c] = hi; row[PC + c] = hi; row[2 * PC + c] = f2bf(v - bf2f(hi));
}
// (mean, rstd) of one row held as NC values per lane
__device__ __forceinline__ void ln_stats(const float (&v)[NC], float eps, float& mean, float& rstd)
{
  float s = 0.f;
#pragma unroll
  for (int j = 0; j < NC; ++j) s += v[j];
  mean = wave_sum(s) * (1.0f / PC);
  float q = 0.f;
#pragma unroll
  for (int j = 0; j < NC; ++j) { const float d = v[j] - mean; q += d * d; }
  rstd = rsqrtf(wave_sum(q) * (1.0f / PC) + eps);
}
// LayerNorm backward for one row: du (gradient at the affine output) -> gradient at the LayerNorm input
__device__ __forceinline__ void ln_bwd_row(const float (&du)[NC], const float (&xhat)[NC], const float (&gamma)[NC], float rstd, float (&dx)[NC])
{
  float s1 = 0.f, s2 = 0.f, dxh[NC];
#pragma unroll
  for (int j = 0; j < NC; ++j) { dxh[j] = du[j] * gamma[j]; s1 += dxh[j]; s2 += dxh[j] * xhat[j]; }
  s1 = wave_sum(s1) * (1.0f / PC); s2 = wave_sum(s2) * (1.0f / PC);
#pragma unroll
  for (int j = 0; j < NC; ++j) dx[j] = rstd * (dxh[j] - s1 - xhat[j] * s2);
}
// a tap of the dilated depthwise conv reads row m + off only inside the same utterance (zero padding, modules.py:709-712)
__device__ __forceinline__ bool tap_ok(const int32_t* utt, const float* rowmask, int m, int off, int R)
{
  const int mm = m + off;
  return mm >= 0 && mm < R && utt[mm] == utt[m] && rowmask[mm] != 0.f;
}

// h1 = dwconv_d(x) + b for row m (x rows are masked: rows outside an utterance's frames are zero)
__device__ __forceinline__ void sep_row(const float* __restrict__ x, int ldx, const float (&w)[3][NC], const float (&b)[NC],
                                        const int32_t* utt, const float* rowmask, int m, int d, int R, int lane, float (&h1)[NC])
{
#pragma unroll
  for (int j = 0; j < NC; ++j) h1[j] = b[j];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int off = (k - 1) * d;
    if (k != 1 && !tap_ok(utt, rowmask, m, off, R)) continue;
    const float* xr = x + (size_t)(m + off) * ldx;
#pragma unroll
    for (int j = 0; j < NC; ++j) h1[j] += w[k][j] * xr[lane + 64 * j];
  }
}

}  // namespace gtdds
