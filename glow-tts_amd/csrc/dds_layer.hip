// One DilatedDepthSeparableConv layer (modules.py:718-735) per launch and direction, gfx950.
//
// The per-op path of predictor_ops.hip takes three launches forward (gt_dds_sep_fwd, the split 1x1 GEMM, gt_dds_out_fwd) and four
// backward, and every activation row crosses HBM between them (a1 as bf16x3, h2, d h2 as bf16x3, d a1).  Everything between the
// depthwise conv and the residual is row-local, and the depthwise conv is the layer's FIRST op: its +-d neighbour rows are rows of the
// layer's input, read from global memory.  So a workgroup that owns TILE consecutive rows needs no halo recomputation:
//
//   forward   phase 1 (VALU)  a1 = gelu(LN1(dwconv_d(x) + b))      -> LDS as a bf16 hi / lo pair (+ the saved [hi | hi | lo] rows)
//             phase 2 (MFMA)  h2 = a1_hi w_hi + a1_hi w_lo + a1_lo w_hi   from the flag-8 image [w_hi ; w_lo ; w_hi], fp32 accumulate
//             phase 3 (VALU)  out = (x + dropout(gelu(LN2(h2 + bias)))) * mask
//   backward  phase A (VALU)  dy -> d h2 (LN2 / GELU / dropout backward from the saved h2)    -> LDS hi / lo pair (+ the hi rows)
//             phase B (MFMA)  d a1 = d h2 (x) the flag-8 data-gradient image                  -> LDS, fp32
//             phase C (VALU)  d a1 -> d h1 (GELU / LN1 backward, h1 recomputed from x)
//   gt_dds_dw_bwd (predictor_ops.hip) follows the backward: dx[m] needs d h1[m +- d], which crosses tiles.
//
// The row arithmetic is dds_rows.h, the same functions the per-op kernels call; the two paths differ in the summation order of the
// 1x1 product only (here the three bf16 products of one 16-wide K step are accumulated together, there one K third after the other).
// 256 threads: in the row phases wave w walks rows [16 w, 16 w + 16) of the tile, a lane owning channels lane + 64 j; in the MFMA
// phase wave w owns the 32-row block w & 1 and the 96 channels of group w >> 1 (3 accumulators of 32 x 32) and loads its weight
// fragments from the row-major image in global memory (221 KB per image: L2-resident) — 16 bytes per lane, no LDS staging.
// LDS: ONE 50 176-byte tile, first the operand rows (64 x [192 hi | 192 lo | 8 pad] bf16, pitch 784 B), then, behind a barrier,
// the fp32 product (64 x [192 | 4 pad], the same pitch); the pitch is 16 mod 128 bytes, so the 16-byte fragment reads and the
// accumulator stores of 32 consecutive rows fall on distinct banks.
#include "common.h"
#include "internal.h"
#include "mfma_frag.h"
#include "dds_rows.h"
#include "../../include/glowtts_hip.h"

namespace {

using namespace gtdds;

constexpr int TILE = 64;                      // rows per workgroup
constexpr int RPWV = TILE / 4;                // rows per wave in the row phases
constexpr int AP = 2 * PC + 8;                // bf16 per operand row in LDS
constexpr int HP = PC + 4;                    // floats per product row in LDS
constexpr int TILE_BYTES = TILE * AP * 2;
static_assert(AP * 2 == HP * 4 && (AP * 2) % 128 == 16, "the two views of the tile share one pitch");
static_assert(PC % 32 == 0 && PC / 32 == 6, "2 row blocks x 6 channel blocks over 4 waves");

// this wave's 32 rows x 96 channels of  A[rows, hi | lo] (x) W[channel][w_hi ; w_lo ; ...]  (row-major image, Kp halfs per row)
__device__ __forceinline__ void tile_gemm_split3(const bf16_t* __restrict__ W, int Kp, const bf16_t* As, int wave, int lane, f32x16_t (&acc)[3])
{
  const int r = lane & 31, h = lane >> 5, wm = wave & 1, wn = wave >> 1;
  acc_zero(acc);
  const bf16_t* ap = As + (32 * wm + r) * AP + 8 * h;
  const bf16_t* wp = W + (size_t)(96 * wn + r) * Kp + 8 * h;
#pragma unroll 2
  for (int ks = 0; ks < PC / 16; ++ks) {
    const bf16x8_t ahi = *reinterpret_cast<const bf16x8_t*>(ap + 16 * ks);
    const bf16x8_t alo = *reinterpret_cast<const bf16x8_t*>(ap + PC + 16 * ks);
#pragma unroll
    for (int nb = 0; nb < 3; ++nb) {
      const bf16_t* wr = wp + (size_t)(32 * nb) * Kp + 16 * ks;
      const bf16x8_t whi = asfrag(*reinterpret_cast<const uint4*>(wr));
      const bf16x8_t wlo = asfrag(*reinterpret_cast<const uint4*>(wr + PC));
      acc[nb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(whi, ahi, acc[nb], 0, 0, 0);
      acc[nb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wlo, ahi, acc[nb], 0, 0, 0);
      acc[nb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(whi, alo, acc[nb], 0, 0, 0);
    }
  }
}
// accumulators -> the fp32 view of the tile: lane (r, h) holds row r, channels 8 g + 4 h + i of each 32-channel block
__device__ __forceinline__ void tile_store_acc(float* Hs, int wave, int lane, const f32x16_t (&acc)[3])
{
  const int r = lane & 31, h = lane >> 5, wm = wave & 1, wn = wave >> 1;
#pragma unroll
  for (int nb = 0; nb < 3; ++nb)
#pragma unroll
    for (int g = 0; g < 4; ++g)
      *reinterpret_cast<float4*>(&Hs[(32 * wm + r) * HP + 96 * wn + 32 * nb + 8 * g + 4 * h]) =
          make_float4(acc[nb][4 * g], acc[nb][4 * g + 1], acc[nb][4 * g + 2], acc[nb][4 * g + 3]);
}
// one operand row into the bf16 view: [hi | lo]
__device__ __forceinline__ void tile_store_pair(bf16_t* as, int lane, const float (&v)[NC])
{
#pragma unroll
  for (int j = 0; j < NC; ++j) {
    const bf16_t hi = f2bf(v[j]);
    as[lane + 64 * j] = hi; as[PC + lane + 64 * j] = f2bf(v[j] - bf2f(hi));
  }
}

__global__ __launch_bounds__(256) void gt_dds_layer_fwd_kernel(
    const float* __restrict__ x, int ldx, const float* __restrict__ w, const float* __restrict__ b,
    const float* __restrict__ gamma1, const float* __restrict__ beta1, const bf16_t* __restrict__ Wp, int Kp, const float* __restrict__ bias,
    const float* __restrict__ gamma2, const float* __restrict__ beta2, const int32_t* __restrict__ utt, const float* __restrict__ rowmask,
    bf16_t* __restrict__ a1, int lda, float* __restrict__ h2, float* __restrict__ out, bf16_t* __restrict__ out3, int ldo3,
    int R, int d, float eps, uint32_t thresh, uint32_t seed, const uint32_t* __restrict__ seed_dev, float scale)
{
  __shared__ __attribute__((aligned(16))) unsigned char smem[TILE_BYTES];
  bf16_t* As = reinterpret_cast<bf16_t*>(smem);
  float* Hs = reinterpret_cast<float*>(smem);
  if (seed_dev) seed ^= *seed_dev;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int m0 = blockIdx.x * TILE;
  {
    float wk[3][NC], bb[NC], g[NC], be[NC];
#pragma unroll
    for (int j = 0; j < NC; ++j) {
      const int c = lane + 64 * j;
      wk[0][j] = w[c * 3]; wk[1][j] = w[c * 3 + 1]; wk[2][j] = w[c * 3 + 2];
      bb[j] = b[c]; g[j] = gamma1[c]; be[j] = beta1[c];
    }
    for (int i = 0; i < RPWV; ++i) {
      const int rl = wave * RPWV + i, m = m0 + rl;
      float v[NC] = {};                                            // masked rows and the rows past R: zero operand rows
      if (m < R && rowmask[m] != 0.f) {
        float h1[NC], mean, rstd;
        sep_row(x, ldx, wk, bb, utt, rowmask, m, d, R, lane, h1);
        ln_stats(h1, eps, mean, rstd);
#pragma unroll
        for (int j = 0; j < NC; ++j) v[j] = gelu_f((h1[j] - mean) * rstd * g[j] + be[j]);
      }
      tile_store_pair(As + rl * AP, lane, v);
      if (m < R) {
#pragma unroll
        for (int j = 0; j < NC; ++j) split3_store(a1 + (size_t)m * lda, lane + 64 * j, v[j]);
      }
    }
  }
  __syncthreads();
  {
    f32x16_t acc[3];
    tile_gemm_split3(Wp, Kp, As, wave, lane, acc);
    __syncthreads();                                               // every wave has read its operand rows: the tile becomes the product
    tile_store_acc(Hs, wave, lane, acc);
  }
  __syncthreads();
  float g[NC], be[NC], bs[NC];
  ld3(gamma2, lane, g); ld3(beta2, lane, be); ld3(bias, lane, bs);
  for (int i = 0; i < RPWV; ++i) {
    const int rl = wave * RPWV + i, m = m0 + rl;
    if (m >= R) break;
    float h[NC], v[NC] = {};
#pragma unroll
    for (int j = 0; j < NC; ++j) {
      h[j] = Hs[rl * HP + lane + 64 * j] + bs[j];                  // masked rows: the bias alone, as the per-op GEMM leaves them
      h2[(size_t)m * PC + lane + 64 * j] = h[j];
    }
    if (rowmask[m] != 0.f) {
      float mean, rstd;
      ln_stats(h, eps, mean, rstd);
#pragma unroll
      for (int j = 0; j < NC; ++j) {
        float y = gelu_f((h[j] - mean) * rstd * g[j] + be[j]);
        if (thresh) y = drop_keep(seed, m, lane + 64 * j, thresh) ? y * scale : 0.f;
        v[j] = x[(size_t)m * ldx + lane + 64 * j] + y;
      }
    }
#pragma unroll
    for (int j = 0; j < NC; ++j) {
      out[(size_t)m * PC + lane + 64 * j] = v[j];
      if (out3) split3_store(out3 + (size_t)m * ldo3, lane + 64 * j, v[j]);
    }
  }
}

// partials (optional): [2 * gridDim.x][2 PC] — row blockIdx.x = this workgroup's [d gamma2 | d beta2], row gridDim.x + blockIdx.x its
// [d gamma1 | d beta1]: two buffers of the [rows][Ca + Cb] form gt_param_partials_reduce sums, back to back
__global__ __launch_bounds__(256) void gt_dds_layer_bwd_kernel(
    const float* __restrict__ x, int ldx, const float* __restrict__ w, const float* __restrict__ b,
    const float* __restrict__ gamma1, const float* __restrict__ beta1, const bf16_t* __restrict__ Wd, int Kp,
    const float* __restrict__ gamma2, const float* __restrict__ beta2, const int32_t* __restrict__ utt, const float* __restrict__ rowmask,
    const float* __restrict__ h2, const float* __restrict__ dy, bf16_t* __restrict__ dh2, int lddh, float* __restrict__ dh1,
    float* __restrict__ dgamma2, float* __restrict__ dbeta2, float* __restrict__ dgamma1, float* __restrict__ dbeta1,
    float* __restrict__ partials, int R, int d, float eps, uint32_t thresh, uint32_t seed, const uint32_t* __restrict__ seed_dev, float scale)
{
  __shared__ __attribute__((aligned(16))) unsigned char smem[TILE_BYTES];
  __shared__ float fold_sm[256];
  bf16_t* As = reinterpret_cast<bf16_t*>(smem);
  float* Hs = reinterpret_cast<float*>(smem);
  if (seed_dev) seed ^= *seed_dev;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int m0 = blockIdx.x * TILE;
  {
    float g[NC], be[NC], ag[NC] = {}, ab[NC] = {};
    ld3(gamma2, lane, g); ld3(beta2, lane, be);
    for (int i = 0; i < RPWV; ++i) {
      const int rl = wave * RPWV + i, m = m0 + rl;
      float o[NC] = {};
      if (m < R && rowmask[m] != 0.f) {
        float h[NC], dd[NC], xh[NC], du[NC], mean, rstd;
        ld3(h2 + (size_t)m * PC, lane, h);
        ld3(dy + (size_t)m * PC, lane, dd);
        ln_stats(h, eps, mean, rstd);
#pragma unroll
        for (int j = 0; j < NC; ++j) {
          xh[j] = (h[j] - mean) * rstd;
          float da = dd[j];
          if (thresh) da = drop_keep(seed, m, lane + 64 * j, thresh) ? da * scale : 0.f;
          du[j] = da * gelu_grad(xh[j] * g[j] + be[j]);
          ag[j] += du[j] * xh[j]; ab[j] += du[j];
        }
        ln_bwd_row(du, xh, g, rstd, o);
      }
      tile_store_pair(As + rl * AP, lane, o);
      if (m < R) {
#pragma unroll
        for (int j = 0; j < NC; ++j) dh2[(size_t)m * lddh + lane + 64 * j] = f2bf(o[j]);      // hi part: operand of the deferred weight gradient
      }
    }
    float* pr = partials ? partials + (size_t)blockIdx.x * 2 * PC : nullptr;                 // [gamma2 | beta2]
#pragma unroll
    for (int j = 0; j < NC; ++j) {
      const int c = lane + 64 * j;
      wg_fold_out(dgamma2 + c, pr ? pr + c : nullptr, ag[j], fold_sm, lane, wave);
      wg_fold_out(dbeta2 + c, pr ? pr + PC + c : nullptr, ab[j], fold_sm, lane, wave);
    }
  }                                                                // (the folds end in a barrier: the operand rows are complete)
  {
    f32x16_t acc[3];
    tile_gemm_split3(Wd, Kp, As, wave, lane, acc);
    __syncthreads();
    tile_store_acc(Hs, wave, lane, acc);
  }
  __syncthreads();
  float wk[3][NC], bb[NC], g[NC], be[NC], ag[NC] = {}, ab[NC] = {};
#pragma unroll
  for (int j = 0; j < NC; ++j) {
    const int c = lane + 64 * j;
    wk[0][j] = w[c * 3]; wk[1][j] = w[c * 3 + 1]; wk[2][j] = w[c * 3 + 2];
    bb[j] = b[c]; g[j] = gamma1[c]; be[j] = beta1[c];
  }
  for (int i = 0; i < RPWV; ++i) {
    const int rl = wave * RPWV + i, m = m0 + rl;
    if (m >= R) break;
    float o[NC] = {};
    if (rowmask[m] != 0.f) {
      float h1[NC], xh[NC], du[NC], mean, rstd;
      sep_row(x, ldx, wk, bb, utt, rowmask, m, d, R, lane, h1);
      ln_stats(h1, eps, mean, rstd);
#pragma unroll
      for (int j = 0; j < NC; ++j) {
        xh[j] = (h1[j] - mean) * rstd;
        du[j] = Hs[rl * HP + lane + 64 * j] * gelu_grad(xh[j] * g[j] + be[j]);
        ag[j] += du[j] * xh[j]; ab[j] += du[j];
      }
      ln_bwd_row(du, xh, g, rstd, o);
    }
#pragma unroll
    for (int j = 0; j < NC; ++j) dh1[(size_t)m * PC + lane + 64 * j] = o[j];
  }
  float* pr = partials ? partials + (size_t)(gridDim.x + blockIdx.x) * 2 * PC : nullptr;    // [gamma1 | beta1]
#pragma unroll
  for (int j = 0; j < NC; ++j) {
    const int c = lane + 64 * j;
    wg_fold_out(dgamma1 + c, pr ? pr + c : nullptr, ag[j], fold_sm, lane, wave);
    wg_fold_out(dbeta1 + c, pr ? pr + PC + c : nullptr, ab[j], fold_sm, lane, wave);
  }
}

inline int tiles(int R) { return (R + TILE - 1) / TILE; }
inline bool pow3(int d) { if (d <= 0) return false; while (d % 3 == 0) d /= 3; return d == 1; }

}  // namespace

extern "C" int gt_dds_layer_tile_rows(void) { return TILE; }
extern "C" int gt_dds_layer_partial_rows(int R) { return R > 0 ? 2 * tiles(R) : 0; }

extern "C" int gt_dds_layer_fwd(const float* x, int ldx, const float* w_sep, const float* b_sep, const float* gamma1, const float* beta1,
                                const void* w1x1_split, int Kp, const float* b1x1, const float* gamma2, const float* beta2,
                                const int32_t* utt, const float* rowmask, void* a1_bf16, int lda, float* h2, float* out,
                                void* out_split3, int ldo3, int R, int C, int dilation, float eps, float drop_p, uint32_t seed,
                                const uint32_t* seed_dev, void* stream)
{
  if (!x || !w_sep || !b_sep || !gamma1 || !beta1 || !w1x1_split || !b1x1 || !gamma2 || !beta2 || !utt || !rowmask || !a1_bf16 || !h2 || !out)
    return GT_E_INVAL;
  if (C != PC || !pow3(dilation) || R <= 0) return GT_E_UNSUPPORTED;
  if (!(drop_p >= 0.f && drop_p < 1.f)) return GT_E_INVAL;
  if (ldx < PC || lda < 3 * PC || (out_split3 && ldo3 < 3 * PC) || Kp < 3 * PC || (Kp & 7) || !al16(w1x1_split)) return GT_E_ALIGN;
  uint32_t th; float sc; gt_drop_params(drop_p, &th, &sc);
  hipLaunchKernelGGL(gt_dds_layer_fwd_kernel, dim3(tiles(R)), dim3(256), 0, GT_ST(stream), x, ldx, w_sep, b_sep, gamma1, beta1,
                     static_cast<const bf16_t*>(w1x1_split), Kp, b1x1, gamma2, beta2, utt, rowmask, static_cast<bf16_t*>(a1_bf16), lda, h2, out,
                     static_cast<bf16_t*>(out_split3), ldo3, R, dilation, eps, th, seed, seed_dev, sc);
  return gt_launch_status(__func__);
}

extern "C" int gt_dds_layer_bwd(const float* x, int ldx, const float* w_sep, const float* b_sep, const float* gamma1, const float* beta1,
                                const void* w1x1_dgrad_split, int Kp, const float* gamma2, const float* beta2,
                                const int32_t* utt, const float* rowmask, const float* h2, const float* dy, void* dh2_bf16, int lddh,
                                float* dh1, float* dgamma2, float* dbeta2, float* dgamma1, float* dbeta1, float* partials,
                                int R, int C, int dilation, float eps, float drop_p, uint32_t seed, const uint32_t* seed_dev, void* stream)
{
  if (!x || !w_sep || !b_sep || !gamma1 || !beta1 || !w1x1_dgrad_split || !gamma2 || !beta2 || !utt || !rowmask || !h2 || !dy || !dh2_bf16 ||
      !dh1 || (!partials && (!dgamma2 || !dbeta2 || !dgamma1 || !dbeta1)))
    return GT_E_INVAL;
  if (C != PC || !pow3(dilation) || R <= 0) return GT_E_UNSUPPORTED;
  if (!(drop_p >= 0.f && drop_p < 1.f)) return GT_E_INVAL;
  if (ldx < PC || lddh < PC || Kp < 3 * PC || (Kp & 7) || !al16(w1x1_dgrad_split)) return GT_E_ALIGN;
  uint32_t th; float sc; gt_drop_params(drop_p, &th, &sc);
  hipLaunchKernelGGL(gt_dds_layer_bwd_kernel, dim3(tiles(R)), dim3(256), 0, GT_ST(stream), x, ldx, w_sep, b_sep, gamma1, beta1,
                     static_cast<const bf16_t*>(w1x1_dgrad_split), Kp, gamma2, beta2, utt, rowmask, h2, dy, static_cast<bf16_t*>(dh2_bf16), lddh,
                     dh1, dgamma2, dbeta2, dgamma1, dbeta1, partials, R, dilation, eps, th, seed, seed_dev, sc);
  return gt_launch_status(__func__);
}
