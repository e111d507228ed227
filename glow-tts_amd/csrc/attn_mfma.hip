// Relative-position multi-head attention forward on bf16 MFMA for gfx950 (reference
// attentions.py:241-336 in its 9-diagonal band form; D = 96, window 4, T <= 256).
//
// One workgroup = 4 waves = 128 query rows of one (utterance, head); K and V of that (utterance,
// head) are staged once in LDS.  Per wave (32 query rows), everything stays in registers:
//   S^T = K Q^T            MFMA A = K rows from LDS (ds_read_b128, pitch 208 B), B = Q^T fragments loaded
//                          straight from HBM; a lane then owns ONE query and 16 keys per 32-key tile, so
//                          the softmax row reductions are in-lane + one xor-32 exchange.
//   QE  = Ek Q^T           the relative-key logits q_i.Ek[r] as one more MFMA chain (Ek padded to 32 rows)
//   P   = softmax((S^T + band(QE)) / sqrt(D)), saved fp32 for the backward, dropout replayable
//   O^T = V^T P^T          "accumulator tile as the next MFMA's operand" (guide §3): P^T registers are
//                          converted pairwise to bf16 and fed as B; V^T comes from LDS through
//                          ds_read_b64_tr_b16 (pitch 192 B) in the permuted k order that map requires.
//   O^T += Ev^T band(P)^T  the relative-value term as one K=16 MFMA per 32 channels.
// Each of these steps is one piece of attn_frag.h, shared with attn_long.hip; a kernel owns where its operands live, its tile
// loops and its barriers.  The two kernels of the cfg 2 training step (gt_attn_fwd_mfma_kernel, gt_attn_bwd_fused_kernel) call the
// leaves only: row geometry, Ek / Ev stagers, rel-table chain, band MFMA, store_row96, dE contraction, Acc flush.
#include <stdlib.h>
#include <type_traits>
#include "attn_frag.h"
#include "internal.h"

#ifndef ATTN_PHASES
#define ATTN_PHASES 0                         // dev: shader-clock stamps of the 8 waves of the T <= 160 backward (tools/attn_bwd_phases.py), 0 in every build that ships
#endif

namespace {
using namespace gt_attn_frag;

#if ATTN_PHASES
// [8 waves][128 workgroups][16]
__device__ unsigned long long g_attn_ph[8 * 128 * 16];
#define APH(i) do { const unsigned wg_ = blockIdx.y * gridDim.x + blockIdx.x;                                                       \
                    if ((threadIdx.x & 63) == 0 && wg_ < 128)                                                                       \
                      g_attn_ph[((threadIdx.x >> 6) * 128 + wg_) * 16 + (i)] = __builtin_amdgcn_s_memtime(); } while (0)
#else
#define APH(i) do { } while (0)
#endif

// rows 0 .. n - 1 of a [rows][ld] operand (head h) into an LDS image of pitch pa, rows >= T zero; nth threads
GT_ATTN_DEV void stage_rows(bf16_t* A, int pa, const bf16_t* a, int lda, int n, int T, int h, const Rows& rows, int tid, int nth) {
  for (int i = tid; i < n * (D / 8); i += nth) {
    const int j = i / (D / 8), c8 = i - j * (D / 8);
    uint4 aa = make_uint4(0, 0, 0, 0);
    if (j < T) aa = *reinterpret_cast<const uint4*>(a + rows.rw(j) * lda + h * D + c8 * 8);
    *reinterpret_cast<uint4*>(A + j * pa + c8 * 8) = aa;
  }
}
// ... of two operands in one walk, both loads of a row in flight together
GT_ATTN_DEV void stage_rows2(bf16_t* A, int pa, const bf16_t* a, int lda, bf16_t* B, int pb, const bf16_t* b_, int ldb,
                             int n, int T, int h, const Rows& rows, int tid, int nth) {
  for (int i = tid; i < n * (D / 8); i += nth) {
    const int j = i / (D / 8), c8 = i - j * (D / 8);
    uint4 aa = make_uint4(0, 0, 0, 0), bb = aa;
    if (j < T) {
      aa = *reinterpret_cast<const uint4*>(a + rows.rw(j) * lda + h * D + c8 * 8);
      bb = *reinterpret_cast<const uint4*>(b_ + rows.rw(j) * ldb + h * D + c8 * 8);
    }
    *reinterpret_cast<uint4*>(A + j * pa + c8 * 8) = aa;
    *reinterpret_cast<uint4*>(B + j * pb + c8 * 8) = bb;
  }
}

template <int NT>   // key tiles of 32 (T <= 32*NT)
__global__ __launch_bounds__(256, 1) void gt_attn_fwd_mfma_kernel(
    const bf16_t* __restrict__ q, const bf16_t* __restrict__ k, const bf16_t* __restrict__ v, int ld,
    const float* __restrict__ Ek, const float* __restrict__ Ev, const int32_t* __restrict__ lens,
    bf16_t* __restrict__ out, int ldo, float* __restrict__ Pout,
    int T, int Tp, const int32_t* row0, int H, uint32_t drop_thresh, uint32_t drop_seed, float drop_scale, const uint32_t* __restrict__ seed_dev)
{
  if (seed_dev) drop_seed ^= *seed_dev;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  constexpr int TPAD = NT * 32;
  bf16_t* Ks  = reinterpret_cast<bf16_t*>(smem);                 // [TPAD][KP]
  bf16_t* Vs  = Ks + TPAD * KP;                                  // [TPAD][VP]
  bf16_t* Eks = Vs + TPAD * VP;                                  // [32][KP]   rows >= 9 are zero
  bf16_t* EvT = Eks + 32 * KP;                                   // [96][16]   EvT[d][r], r >= 9 zero
  float*  QE  = reinterpret_cast<float*>(EvT + D * 16);          // [4 waves][32][NW]
  bf16_t* PB  = reinterpret_cast<bf16_t*>(QE + 4 * 32 * NW);     // [4 waves][32][16]

  const int b = blockIdx.z, h = blockIdx.y;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const Lane ln(lane);
  const int r = ln.r, hh = ln.hh;
  const int len = lens[b];
  const Rows rows(row0, b, Tp);

  // ---- stage K, V (zero rows >= T), Ek, Ev^T
  for (int i = tid; i < TPAD * (D / 8); i += 256) {
    const int j = i / (D / 8), c8 = i - j * (D / 8);
    uint4 kk = make_uint4(0, 0, 0, 0), vv = kk;
    if (j < T) {
      kk = *reinterpret_cast<const uint4*>(k + rows.rw(j) * ld + h * D + c8 * 8);
      vv = *reinterpret_cast<const uint4*>(v + rows.rw(j) * ld + h * D + c8 * 8);
    }
    *reinterpret_cast<uint4*>(Ks + j * KP + c8 * 8) = kk;
    *reinterpret_cast<uint4*>(Vs + j * VP + c8 * 8) = vv;
  }
  stage_rel_rows(Eks, Ek, tid, 256);
  stage_rel_tr(EvT, Ev, tid, 256);
  for (int i = tid; i < 4 * 32 * 16; i += 256) PB[i] = 0;
  __syncthreads();

  const int i0 = blockIdx.x * 128 + 32 * w;
  if (i0 >= T) return;                                           // wave-uniform, after the only block barrier
  const int i = i0 + r;                                          // this lane's query
  const int ic = i < T ? i : T - 1;
  float* qe = QE + w * 32 * NW;
  bf16_t* pb = PB + w * 32 * 16;

  // ---- Q^T fragments straight from HBM: lane (query r, k-half hh), 6 k-steps of 16 channels; QE = Ek Q^T
  bf16x8_t qf[6];
#pragma unroll
  for (int ks = 0; ks < 6; ++ks)
    qf[ks] = *reinterpret_cast<const bf16x8_t*>(q + rows.rw(ic) * ld + h * D + ks * 16 + 8 * hh);
  rel_table(qe, Eks, qf, ln);

  // The tile loops below are this kernel's own text (it is on the cfg 2 training step and <8> has no register to give): of
  // attn_frag.h it takes the leaves only
  // ---- S^T = K Q^T
  f32x16_t s[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) {
#pragma unroll
    for (int e = 0; e < 16; ++e) s[t][e] = 0.f;
#pragma unroll
    for (int ks = 0; ks < 6; ++ks) {
      const bf16x8_t af = *reinterpret_cast<const bf16x8_t*>(Ks + (32 * t + r) * KP + ks * 16 + 8 * hh);
      s[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af, qf[ks], s[t], 0, 0, 0);
    }
  }
  __builtin_amdgcn_wave_barrier();                               // qe written by both lane halves

  // ---- softmax over keys (in-lane + xor 32)
  const float inv_sqrt = rsqrtf((float)D);
  float mx = -3.0e38f;
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int j = 32 * t + (e & 3) + 8 * (e >> 2) + 4 * hh;
      float sc = s[t][e];
      const int rel = j - i + WIN;
      if ((unsigned)rel <= 2u * WIN) sc += qe[r * NW + rel];
      sc *= inv_sqrt;
      if (j >= T) sc = -3.0e38f;                                 // not a key at all
      else if (j >= len || i >= len) sc = -1e4f;                 // masked_fill(mask == 0, -1e4), attentions.py:260
      s[t][e] = sc;
      mx = fmaxf(mx, sc);
    }
  mx = fmaxf(mx, __shfl_xor(mx, 32));
  float den = 0.f;
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int e = 0; e < 16; ++e) { const float ex = __expf(s[t][e] - mx); s[t][e] = ex; den += ex; }
  den += __shfl_xor(den, 32);
  const float rden = 1.0f / den;
  float* prow = Pout + (((size_t)b * H + h) * T + ic) * T;
  const uint32_t drow = (uint32_t)((b * H + h) * T + i);
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int j0 = 32 * t + 8 * g + 4 * hh;
      float p4[4];
#pragma unroll
      for (int e2 = 0; e2 < 4; ++e2) p4[e2] = s[t][4 * g + e2] * rden;
      if (i < T) {
        if (j0 + 3 < T && (T & 3) == 0) *reinterpret_cast<float4*>(prow + j0) = make_float4(p4[0], p4[1], p4[2], p4[3]);
        else {
#pragma unroll
          for (int e2 = 0; e2 < 4; ++e2) if (j0 + e2 < T) prow[j0 + e2] = p4[e2];
        }
      }
#pragma unroll
      for (int e2 = 0; e2 < 4; ++e2) {
        const int j = j0 + e2;
        float pd = p4[e2];
        if (drop_thresh) pd = drop_keep(drop_seed, drow, j, drop_thresh) ? pd * drop_scale : 0.f;
        s[t][4 * g + e2] = pd;
        const int rel = j - i + WIN;
        if ((unsigned)rel <= 2u * WIN && j < T) pb[r * 16 + rel] = f2bf(pd);
      }
    }
  __builtin_amdgcn_wave_barrier();

  // ---- O^T = V^T P^T (+ Ev^T band(P)^T)
  const int li = lane & 15, qd = li >> 2, pp = li & 3, colhalf = ((lane >> 4) & 1) * 16;
  f32x16_t o[3];
#pragma unroll
  for (int dt = 0; dt < 3; ++dt) {
#pragma unroll
    for (int e = 0; e < 16; ++e) o[dt][e] = 0.f;
  }
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int s2 = 0; s2 < 2; ++s2) {
      float f8[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) f8[e] = s[t][8 * s2 + e];
      const bf16x8_t pf = pack8(f8);                             // k order: row 16*s2 + 8*(e>>2) + 4*hh + (e&3) of the tile
#pragma unroll
      for (int dt = 0; dt < 3; ++dt) {
        const bf16_t* va = Vs + (32 * t + 16 * s2 + 4 * hh + qd) * VP + 32 * dt + colhalf + 4 * pp;
        const bf16x8_t af = tr_frag8(va, va + 8 * VP);           // V^T[d][keys 4hh..4hh+3 | 8+4hh..8+4hh+3]
        o[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af, pf, o[dt], 0, 0, 0);
      }
    }
  band_mfma(o, EvT, pb, ln);
  if (i < T && rows.owns(i)) store_row96(out + (rows.rbase + i) * ldo + h * D, o, hh);
}

template <int NT>
int launch_fwd(const gt_attn_call& c)
{
  constexpr int TPAD = NT * 32;
  const size_t lds = (size_t)TPAD * KP * 2 + (size_t)TPAD * VP * 2 + 32 * KP * 2 + D * 16 * 2 + 4 * 32 * NW * 4 + 4 * 32 * 16 * 2;
  if (const int rc = gt_allow_lds<&gt_attn_fwd_mfma_kernel<NT>>(160 * 1024)) return rc;
  hipLaunchKernelGGL(gt_attn_fwd_mfma_kernel<NT>, dim3((c.T + 127) / 128, c.H, c.B), dim3(256), lds, c.stream,
                     c.q, c.k, c.v, c.ld, c.Ek, c.Ev, c.lens, c.out, c.ldo, c.P, c.T, c.Tp, c.row0, c.H, c.th, c.sd, c.sc, c.seed_dev);
  return gt_launch_status(__func__);
}

// -----------------------------------------------------------------------------------------
// Long sequences (256 < T <= 384: configs/base_blank.json interleaves blanks, T_x <= 375).  K and V no longer fit the
// LDS together and NT score tiles no longer fit the register file, so: V stays in LDS (it is read through transposing
// reads), K fragments (plain row reads) come straight from L2 with a one-tile register prefetch, and the wave walks the
// key tiles twice — pass 1 an online max / denominator, pass 2 recomputes each tile's scores, normalises, writes P and
// feeds O^T at once.  Live state: one tile + the O^T accumulators, whatever NT is.
template <int NT>
__global__ __launch_bounds__(256, 1) void gt_attn_fwd_mfma_long_kernel(
    const bf16_t* __restrict__ q, const bf16_t* __restrict__ k, const bf16_t* __restrict__ v, int ld,
    const float* __restrict__ Ek, const float* __restrict__ Ev, const int32_t* __restrict__ lens,
    bf16_t* __restrict__ out, int ldo, float* __restrict__ Pout,
    int T, int Tp, const int32_t* row0, int H, uint32_t drop_thresh, uint32_t drop_seed, float drop_scale, const uint32_t* __restrict__ seed_dev)
{
  if (seed_dev) drop_seed ^= *seed_dev;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  constexpr int TPAD = NT * 32;
  bf16_t* Vs  = reinterpret_cast<bf16_t*>(smem);                 // [TPAD][VP]
  bf16_t* Eks = Vs + TPAD * VP;                                  // [32][KP]   rows >= 9 are zero
  bf16_t* EvT = Eks + 32 * KP;                                   // [96][16]   EvT[d][r], r >= 9 zero
  float*  QE  = reinterpret_cast<float*>(EvT + D * 16);          // [4 waves][32][NW]
  bf16_t* PB  = reinterpret_cast<bf16_t*>(QE + 4 * 32 * NW);     // [4 waves][32][16]

  const int b = blockIdx.z, h = blockIdx.y;
  const int tid = threadIdx.x, w = tid >> 6;
  const Lane ln(tid & 63);
  const int r = ln.r, hh = ln.hh;
  const int len = lens[b];
  const Rows rows(row0, b, Tp);

  stage_rows(Vs, VP, v, ld, TPAD, T, h, rows, tid, 256);
  stage_rel_rows(Eks, Ek, tid, 256);
  stage_rel_tr(EvT, Ev, tid, 256);
  for (int i = tid; i < 4 * 32 * 16; i += 256) PB[i] = 0;
  __syncthreads();

  const int i0 = blockIdx.x * 128 + 32 * w;
  if (i0 >= T) return;                                           // wave-uniform, after the only block barrier
  const int i = i0 + r;
  const int ic = i < T ? i : T - 1;
  float* qe = QE + w * 32 * NW;
  bf16_t* pb = PB + w * 32 * 16;

  bf16x8_t qf[6];
  load_frag6(qf, q + rows.rw(ic) * ld + h * D, hh);
  rel_table(qe, Eks, qf, ln);
  __builtin_amdgcn_wave_barrier();

  const int nt = (T + 31) >> 5;                                  // key tiles that hold keys (wave-uniform)
  const float inv_sqrt = rsqrtf((float)D);
  // masked, scaled scores of one tile from its K fragments (L2, one tile ahead)
  auto scores = [&](int t, const bf16x8_t* kf, f32x16_t& st) {
    mfma6(st, kf, qf);
    score_tile(st, t, qe + r * NW, i, hh, T, len, inv_sqrt);
  };

  // ---- pass 1: online max / denominator over this lane's keys, then the two lane halves are merged
  float mx = -3.0e38f, den = 0.f;
  bf16x8_t kf[6], kn[6];
  load_tile_frag6(kf, k, ld, h, 0, T, rows, ln);
#pragma unroll 1
  for (int t = 0; t < nt; ++t) {
    if (t + 1 < nt) load_tile_frag6(kn, k, ld, h, t + 1, T, rows, ln);
    f32x16_t st;
    scores(t, kf, st);
    online_tile(st, mx, den);
    copy_frag6(kf, kn);
  }
  online_merge(mx, den);
  const float rden = 1.0f / den;

  // ---- pass 2: P = softmax, dropout, O^T = V^T P^T (+ Ev^T band(P)^T)
  float* prow = Pout + (((size_t)b * H + h) * T + ic) * T;
  const Drop drop{drop_thresh, drop_seed, (uint32_t)((b * H + h) * T + i), drop_scale};
  const bool vec = (T & 3) == 0;
  f32x16_t o[3];
  zero3(o);
  load_tile_frag6(kf, k, ld, h, 0, T, rows, ln);
#pragma unroll 1
  for (int t = 0; t < nt; ++t) {
    if (t + 1 < nt) load_tile_frag6(kn, k, ld, h, t + 1, T, rows, ln);
    f32x16_t st;
    scores(t, kf, st);
#pragma unroll
    for (int e = 0; e < 16; ++e) st[e] = __expf(st[e] - mx) * rden;
    p_tile_out<true>(st, t, prow, vec, i, ln, T, drop, pb);
    acc_operand(o, st, Vs + 32 * t * VP, ln);
    copy_frag6(kf, kn);
  }
  __builtin_amdgcn_wave_barrier();
  band_mfma(o, EvT, pb, ln);
  if (i < T && rows.owns(i)) store_row96(out + (rows.rbase + i) * ldo + h * D, o, hh);
}

template <int NT>
int launch_fwd_long(const gt_attn_call& c)
{
  constexpr int TPAD = NT * 32;
  const size_t lds = (size_t)TPAD * VP * 2 + 32 * KP * 2 + D * 16 * 2 + 4 * 32 * NW * 4 + 4 * 32 * 16 * 2;
  if (const int rc = gt_allow_lds<&gt_attn_fwd_mfma_long_kernel<NT>>(160 * 1024)) return rc;
  hipLaunchKernelGGL(gt_attn_fwd_mfma_long_kernel<NT>, dim3((c.T + 127) / 128, c.H, c.B), dim3(256), lds, c.stream,
                     c.q, c.k, c.v, c.ld, c.Ek, c.Ev, c.lens, c.out, c.ldo, c.P, c.T, c.Tp, c.row0, c.H, c.th, c.sd, c.sc, c.seed_dev);
  return gt_launch_status(__func__);
}

// =========================================================================================
// Backward.  Pass 1 (per 32-query block, same wave/lane mapping as the forward):
//   dPd^T = V dO^T (+ band: Ev dO^T)      dP = dropout'(dPd)       Dsum_i = sum_j dP P
//   dS^T  = P (dP - Dsum) / sqrt(D), masked entries 0
//   dQ^T  = K^T dS^T + Ek^T band(dS)^T     (accumulator-as-operand, K^T through transposing reads)
//   dEk  += band(dS)^T Q,  dEv += band(dropout(P))^T dO   (MFMA over the 32 queries of the wave)
//   dS^T and dropout(P)^T leave as bf16 [B,H,T,TI] (query index contiguous) for pass 2.
// Pass 2 (per 32-key block): dK^T = Q^T dS, dV^T = dO^T dropout(P) with Q^T / dO^T through
// transposing reads of LDS-staged Q / dO and the B operands straight from the pass-1 buffers.
template <int NT, int WV>
__global__ __launch_bounds__(64 * WV, 1) void gt_attn_bwd_q_mfma_kernel(
    const bf16_t* __restrict__ q, const bf16_t* __restrict__ k, const bf16_t* __restrict__ v, int ld,
    const float* __restrict__ Ek, const float* __restrict__ Ev, const int32_t* __restrict__ lens,
    const bf16_t* __restrict__ dout, int lddo, const float* __restrict__ P,
    bf16_t* __restrict__ dST, bf16_t* __restrict__ PdT, int TI,
    bf16_t* __restrict__ dq, int lddq, float* __restrict__ dEk, float* __restrict__ dEv,
    int T, int Tp, const int32_t* row0, int H, uint32_t drop_thresh, uint32_t drop_seed, float drop_scale, const uint32_t* __restrict__ seed_dev)
{
  if (seed_dev) drop_seed ^= *seed_dev;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  constexpr int TPAD = NT * 32, NTH = 64 * WV;
  constexpr bool VG = NT > 8;                                    // long sequences: V rows (plain row reads) come from L2, not LDS
  bf16_t* Vs  = reinterpret_cast<bf16_t*>(smem);                 // [TPAD][KP]  A of dPd^T (ds_read_b128); absent if VG
  bf16_t* Ks  = Vs + (VG ? 0 : TPAD * KP);                       // [TPAD][VP]  A of dQ^T (transposing reads)
  bf16_t* Evs = Ks + TPAD * VP;                                  // [32][KP]    rows >= 9 zero
  bf16_t* EkT = Evs + 32 * KP;                                   // [96][16]
  float*  Acc = reinterpret_cast<float*>(EkT + D * 16);          // [2][NW][D]  block-local dEk | dEv
  float*  DOE = Acc + 2 * NW * D;                                // [WV][32][NW]
  bf16_t* WB  = reinterpret_cast<bf16_t*>(DOE + WV * 32 * NW);   // per wave: dSB[32][16] | dSBT[16][BTP] | PdBT[16][BTP] | Qw[32][VP] | dOw[32][VP]
  constexpr int WBN = BAND_TABLES + 2 * 32 * VP;

  const int b = blockIdx.z, h = blockIdx.y;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const Lane ln(lane);
  const int r = ln.r, hh = ln.hh;
  const int len = lens[b];
  const Rows rows(row0, b, Tp);

  if (VG) stage_rows(Ks, VP, k, ld, TPAD, T, h, rows, tid, NTH);
  else stage_rows2(Ks, VP, k, ld, Vs, KP, v, ld, TPAD, T, h, rows, tid, NTH);
  stage_rel_rows(Evs, Ev, tid, NTH);
  stage_rel_tr(EkT, Ek, tid, NTH);
  for (int i = tid; i < 2 * NW * D; i += NTH) Acc[i] = 0.f;
  for (int i = tid; i < WV * BAND_TABLES; i += NTH) {            // band tables start at zero
    const int ww = i / BAND_TABLES, o = i - ww * BAND_TABLES;
    WB[ww * WBN + o] = 0;
  }
  __syncthreads();

  const int i0 = (blockIdx.x * WV + w) * 32;
  const bool active = i0 < T;                                    // wave-uniform
  const int i = i0 + r;
  const int ic = i < T ? i : T - 1;
  float* doe = DOE + w * 32 * NW;
  bf16_t* bt = WB + w * WBN;                                     // dSB | dSBT | PdBT
  bf16_t* Qw = bt + BAND_TABLES;
  bf16_t* dOw = Qw + 32 * VP;

  if (active) {
    // per-wave Q / dO tiles (rows >= T zero) for the dEk / dEv contraction
    for (int c = lane; c < 32 * (D / 8); c += 64) {
      const int rr = c / (D / 8), c8 = c - rr * (D / 8);
      uint4 qq = make_uint4(0, 0, 0, 0), dd = qq;
      if (i0 + rr < T) {
        qq = *reinterpret_cast<const uint4*>(q + rows.rw(i0 + rr) * ld + h * D + c8 * 8);
        dd = *reinterpret_cast<const uint4*>(dout + rows.rw(i0 + rr) * lddo + h * D + c8 * 8);
      }
      *reinterpret_cast<uint4*>(Qw + rr * VP + c8 * 8) = qq;
      *reinterpret_cast<uint4*>(dOw + rr * VP + c8 * 8) = dd;
    }
    bf16x8_t dof[6];
    load_frag6(dof, dout + rows.rw(ic) * lddo + h * D, hh);
    rel_table(doe, Evs, dof, ln);
    const float inv_sqrt = rsqrtf((float)D);
    const float* prow = P + (((size_t)b * H + h) * T + ic) * T;
    const Drop drop{drop_thresh, drop_seed, (uint32_t)((b * H + h) * T + i), drop_scale};
    const int palign = (T & 3) == 0 ? 4 : 1;
    bf16_t* dst_base = dST + ((size_t)b * H + h) * T * TI;
    bf16_t* pdt_base = PdT + ((size_t)b * H + h) * T * TI;
    f32x16_t o[3];
    zero3(o);
    // 161 <= T <= 384 (T <= 160: gt_attn_bwd_fused_kernel below): holding all NT score tiles of a wave (NT*16 accumulators)
    // next to P and the dropout masks does not fit the register file.  One tile at a time instead: pass A walks the key tiles for Dsum only, pass B
    // RECOMPUTES each tile's dPd^T (6 MFMAs, operands already in LDS / registers), turns it into dS^T, stores it and
    // feeds dQ^T straight away — live state is one tile + the dQ^T accumulators, whatever NT is.
    auto dp_tile = [&](int t, f32x16_t& st) {
      if (VG) {
        bf16x8_t vf[6];
        load_tile_frag6(vf, v, ld, h, t, T, rows, ln);
        mfma6(st, vf, dof);
      } else {
        mfma6(st, Vs + (32 * t + r) * KP, dof, hh);
      }
    };
    __builtin_amdgcn_wave_barrier();
    float dsum = 0.f;
#pragma unroll 1
    for (int t = 0; t < NT; ++t) {
      if (32 * t >= T) break;                                      // wave-uniform
      f32x16_t st;
      dp_tile(t, st);
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int j0 = 32 * t + 8 * g + 4 * hh;
        float p4[4];
        load_p4(prow, j0, T, palign, p4);
#pragma unroll
        for (int e2 = 0; e2 < 4; ++e2) dsum += dp_elem(st[4 * g + e2], doe + r * NW, i, j0 + e2, T, drop) * p4[e2];
      }
    }
    dsum += __shfl_xor(dsum, 32);
#pragma unroll 1
    for (int t = 0; t < NT; ++t) {
      if (32 * t >= T) break;
      f32x16_t st;
      dp_tile(t, st);
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int j0 = 32 * t + 8 * g + 4 * hh;
        float p4[4];
        load_p4(prow, j0, T, palign, p4);
#pragma unroll
        for (int e2 = 0; e2 < 4; ++e2) {
          const int j = j0 + e2;
          float pd;
          const float ds = ds_elem(p4[e2], dp_elem(st[4 * g + e2], doe + r * NW, i, j, T, drop), dsum, inv_sqrt, i, j, T, len, drop, pd);
          st[4 * g + e2] = ds;
          if (j < T) {
            dst_base[(size_t)j * TI + i] = f2bf(ds);
            pdt_base[(size_t)j * TI + i] = f2bf(pd);
            band_tables(bt, r, i, j, ds, pd);
          }
        }
      }
#pragma unroll
      for (int s2 = 0; s2 < 2; ++s2) {                             // acc_operand, kept here: through the call both instances take 10 more VGPRs and lose their third wave
        float f8[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) f8[e] = st[8 * s2 + e];
        const bf16x8_t pf = pack8(f8);
#pragma unroll
        for (int dt = 0; dt < 3; ++dt) {
          const bf16_t* ka = Ks + (32 * t + 16 * s2 + 4 * hh) * VP + 32 * dt + ln.tr;
          o[dt] = mfma(tr_frag8(ka, ka + 8 * VP), pf, o[dt]);
        }
      }
    }
    __builtin_amdgcn_wave_barrier();
    band_mfma(o, EkT, bt, ln);
    if (i < T && rows.owns(i)) store_row96(dq + (rows.rbase + i) * lddq + h * D, o, hh);
    // dEk[r'][d] += sum_i dSBT[r'][i] Q[i][d];  dEv[r'][d] += sum_i PdBT[r'][i] dO[i][d]   (K = 32 queries)
    de_contract(Acc, bt + 32 * 16, Qw, ln);
    de_contract(Acc + NW * D, bt + 32 * 16 + 16 * BTP, dOw, ln);
  }
  __syncthreads();
  acc_flush(Acc, dEk, dEv, tid, NTH);
}

template <int NT>
__global__ __launch_bounds__(256, 1) void gt_attn_bwd_kv_mfma_kernel(
    const bf16_t* __restrict__ q, int ld, const bf16_t* __restrict__ dout, int lddo,
    const bf16_t* __restrict__ dST, const bf16_t* __restrict__ PdT, int TI,
    bf16_t* __restrict__ dk, bf16_t* __restrict__ dv, int lddk, int T, int Tp, const int32_t* row0, int H)
{
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  constexpr int TPAD = NT * 32;
  bf16_t* Qs  = reinterpret_cast<bf16_t*>(smem);                 // [TPAD][VP]
  bf16_t* dOs = Qs + TPAD * VP;                                  // [TPAD][VP]
  const int b = blockIdx.z, h = blockIdx.y;
  const int tid = threadIdx.x, w = tid >> 6;
  const Lane ln(tid & 63);
  const int r = ln.r, hh = ln.hh;
  const Rows rows(row0, b, Tp);
  stage_rows2(Qs, VP, q, ld, dOs, VP, dout, lddo, TPAD, T, h, rows, tid, 256);
  __syncthreads();
  const int j0 = blockIdx.x * 128 + 32 * w;
  if (j0 >= T) return;
  const int j = j0 + r, jc = j < T ? j : T - 1;
  const bf16_t* dsr = dST + (((size_t)b * H + h) * T + jc) * TI;
  const bf16_t* pdr = PdT + (((size_t)b * H + h) * T + jc) * TI;
  f32x16_t ak[3], av[3];
  zero3(ak);
  zero3(av);
  const int nks = TI / 16;
  for (int ks = 0; ks < nks; ++ks) {
    const bf16x8_t bds = *reinterpret_cast<const bf16x8_t*>(dsr + 16 * ks + 8 * hh);     // dS[i = 16ks+8hh.., j]
    const bf16x8_t bpd = *reinterpret_cast<const bf16x8_t*>(pdr + 16 * ks + 8 * hh);
#pragma unroll
    for (int dt = 0; dt < 3; ++dt) {                              // kv_pair, kept here: through the call <8> and <12> swap their occupancy (3 <-> 4)
      const bf16_t* qa = Qs + (16 * ks + 8 * hh) * VP + 32 * dt + ln.tr;
      const bf16_t* da = dOs + (16 * ks + 8 * hh) * VP + 32 * dt + ln.tr;
      ak[dt] = mfma(tr_frag8(qa, qa + 4 * VP), bds, ak[dt]);
      av[dt] = mfma(tr_frag8(da, da + 4 * VP), bpd, av[dt]);
    }
  }
  if (j < T && rows.owns(j)) {
    store_row96(dk + rows.rw(j) * lddk + h * D, ak, hh);
    store_row96(dv + rows.rw(j) * lddk + h * D, av, hh);
  }
}

// =========================================================================================
// Backward for T <= 160: the two passes above in ONE workgroup of 8 waves per (utterance, head), grid (H, B).
//   phase 1  waves 0..4 take one 32-query tile each (one score tile live at a time, as the kernel above): the dropout bit of an
//            element is hashed ONCE (16 bits per key tile kept between the Dsum pass and the dS pass), the band code runs only
//            for the key tiles w-1, w, w+1 that can meet the band of query tile w.  dS^T goes to LDS [j][i]; P'^T leaves per
//            32 x 32 tile through a per-wave LDS stage as 16-byte row segments.  P is read in both passes (8-byte loads for even
//            T): all 80 values of a lane held between the passes need 256 + 29 registers at two waves per SIMD (spills).
//   barrier  (with its workgroup-scope fences: phase 2 reads P'^T rows other waves stored)
//   phase 2  Q over K's area, dO over V's; waves 0..4 take one 32-key tile each (dK^T = Q^T dS, dV^T = dO^T P' with dS^T from LDS
//            and P'^T from the L2-hot workspace, the whole row in flight under the staging); waves 5..7 take the dEk / dEv
//            contraction of query tiles {0, 3}, {1, 4}, {2} (one LDS accumulation per wave, one global atomic per address); all waves then
//            store the dS^T rows (16-byte segments, LDS -> workspace) — last, because a store in front of a load holds that load's
//            wait (one counter for both).
// The tile loops, with the dropout bits kept between the passes and the tile index a compile-time constant, are this kernel's own;
// of attn_frag.h it takes the leaves that have no loop over tiles.
// LDS (bytes): K|Q [160][VP] 30720, V|dO [160][KP] 33280, dS^T [160][DSP] 53760, EkT 3072, Ev [9][KP] 1872 and DOE [5][32][9] 5760
// (the dE accumulators alias these two in phase 2), band tables 5 x 3584, P'^T stage 5 x 2560: 159184.
constexpr int FNT = 5, FTP = FNT * 32, FTH = 512;
constexpr int DSP = 168;           // dS^T pitch in halfs (336 B): conflict-free ds_read_b128 over 16 rows, 16-byte row segments
constexpr int PWP = 40;            // pitch of the per-wave P'^T stage [32 keys][32 queries + pad]
constexpr int FBAND = BAND_TABLES;
constexpr size_t FUSED_LDS = (size_t)FTP * VP * 2 + FTP * KP * 2 + FTP * DSP * 2 + D * 16 * 2 + NW * KP * 2 + FNT * 32 * NW * 4 +
                             FNT * FBAND * 2 + FNT * 32 * PWP * 2;
static_assert(2 * NW * D * 4 <= NW * KP * 2 + FNT * 32 * NW * 4, "the dE accumulators alias Ev | DOE");
static_assert(FUSED_LDS <= 160 * 1024, "LDS budget");

template <int N> using ic_t = std::integral_constant<int, N>;

__global__ __launch_bounds__(FTH, 1) void gt_attn_bwd_fused_kernel(
    const bf16_t* __restrict__ q, const bf16_t* __restrict__ k, const bf16_t* __restrict__ v, int ld,
    const float* __restrict__ Ek, const float* __restrict__ Ev, const int32_t* __restrict__ lens,
    const bf16_t* __restrict__ dout, int lddo, const float* __restrict__ P,
    bf16_t* dST, bf16_t* PdT, int TI,
    bf16_t* __restrict__ dq, bf16_t* __restrict__ dk, bf16_t* __restrict__ dv, int lddq, float* __restrict__ dEk, float* __restrict__ dEv,
    int T, int Tp, const int32_t* row0, int H, uint32_t drop_thresh, uint32_t drop_seed, float drop_scale, const uint32_t* __restrict__ seed_dev)
{
  APH(0);
  if (seed_dev) drop_seed ^= *seed_dev;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  bf16_t* Ks  = reinterpret_cast<bf16_t*>(smem);                 // [FTP][VP]   A of dQ^T (transposing reads); phase 2: Q
  bf16_t* Vs  = Ks + FTP * VP;                                   // [FTP][KP]   A of dPd^T (ds_read_b128);     phase 2: dO [FTP][VP]
  bf16_t* dSs = Vs + FTP * KP;                                   // [FTP][DSP]  dS^T[j][i]
  bf16_t* EkT = dSs + FTP * DSP;                                 // [96][16]
  bf16_t* Evs = EkT + D * 16;                                    // [NW][KP]
  float*  DOE = reinterpret_cast<float*>(Evs + NW * KP);         // [FNT][32][NW]
  bf16_t* WB  = reinterpret_cast<bf16_t*>(DOE + FNT * 32 * NW);  // per query tile: dSB[32][16] | dSBT[16][BTP] | PdBT[16][BTP]
  bf16_t* PW  = WB + FNT * FBAND;                                // per query tile: P'^T stage [32][PWP]
  float*  Acc = reinterpret_cast<float*>(Evs);                   // [2][NW][D]  dEk | dEv of this (b, h): phase 2 only

  const int b = blockIdx.y, h = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const Lane ln(lane);
  const int r = ln.r, hh = ln.hh;
  const int len = lens[b];
  const Rows rows(row0, b, Tp);
  bf16_t* dst_base = dST + ((size_t)b * H + h) * T * TI;
  bf16_t* pdt_base = PdT + ((size_t)b * H + h) * T * TI;
  const int li = lane & 15, qd = li >> 2, pp = li & 3, colhalf = ((lane >> 4) & 1) * 16;
  const bool tile = w < FNT && 32 * w < T;                       // wave-uniform: this wave owns query tile w, later key tile w

  for (int x = tid; x < FTP * (D / 8); x += FTH) {
    const int j = x / (D / 8), c8 = x - j * (D / 8);
    uint4 kk = make_uint4(0, 0, 0, 0), vv = kk;
    if (j < T) {
      kk = *reinterpret_cast<const uint4*>(k + rows.rw(j) * ld + h * D + c8 * 8);
      vv = *reinterpret_cast<const uint4*>(v + rows.rw(j) * ld + h * D + c8 * 8);
    }
    *reinterpret_cast<uint4*>(Ks + j * VP + c8 * 8) = kk;
    *reinterpret_cast<uint4*>(Vs + j * KP + c8 * 8) = vv;
  }
  for (int x = tid; x < NW * D; x += FTH) { const int rr = x / D, c = x - rr * D; Evs[rr * KP + c] = f2bf(Ev[x]); }   // own image: no zero rows kept
  stage_rel_tr(EkT, Ek, tid, FTH);
  for (int x = tid; x < FNT * FBAND; x += FTH) WB[x] = 0;         // band tables start at zero
  __syncthreads();
  APH(1);

  if (tile) {
    const int i = 32 * w + r;                                    // this lane's query
    const int ic = i < T ? i : T - 1;
    float* doe = DOE + w * 32 * NW;
    bf16_t* dSB = WB + w * FBAND;
    bf16_t* dSBT = dSB + 32 * 16;
    bf16_t* PdBT = dSBT + 16 * BTP;
    bf16_t* pw = PW + w * 32 * PWP;
    const float* prow = P + (((size_t)b * H + h) * T + ic) * T;

    const int palign = (T & 3) == 0 ? 4 : (T & 1) == 0 ? 2 : 1;  // alignment (floats) of prow + a multiple of 4
    auto load_p = [&](int t, float* pt) {
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int j0 = 32 * t + 8 * g + 4 * hh;
        float* p4 = pt + 4 * g;
        p4[0] = p4[1] = p4[2] = p4[3] = 0.f;
        if (palign == 4 && j0 + 3 < T) { const float4 pv = *reinterpret_cast<const float4*>(prow + j0); p4[0] = pv.x; p4[1] = pv.y; p4[2] = pv.z; p4[3] = pv.w; }
        else if (palign == 2 && j0 + 3 < T) {
          const float2 pa = *reinterpret_cast<const float2*>(prow + j0), pc = *reinterpret_cast<const float2*>(prow + j0 + 2);
          p4[0] = pa.x; p4[1] = pa.y; p4[2] = pc.x; p4[3] = pc.y;
        } else {
#pragma unroll
          for (int e2 = 0; e2 < 4; ++e2) if (j0 + e2 < T) p4[e2] = prow[j0 + e2];
        }
      }
    };

    bf16x8_t dof[6];
#pragma unroll
    for (int ks = 0; ks < 6; ++ks)
      dof[ks] = *reinterpret_cast<const bf16x8_t*>(dout + rows.rw(ic) * lddo + h * D + ks * 16 + 8 * hh);
    {                                                            // the rel-table chain over this kernel's 9-row Ev image
      f32x16_t acc;
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[e] = 0.f;
#pragma unroll
      for (int ks = 0; ks < 6; ++ks) {
        const uint4 z = make_uint4(0, 0, 0, 0);
        bf16x8_t af = __builtin_bit_cast(bf16x8_t, z);           // rows >= 9 of Ev are zero and not kept
        if (r < NW) af = *reinterpret_cast<const bf16x8_t*>(Evs + r * KP + ks * 16 + 8 * hh);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af, dof[ks], acc, 0, 0, 0);
      }
      rel_store(doe, acc, ln);
    }
    const float inv_sqrt = rsqrtf((float)D);
    const uint32_t drow = (uint32_t)((b * H + h) * T + i);
    const bool qdead = i >= len || i >= T;
    const int jlive = len < T ? len : T;
    f32x16_t o[3];
    auto dp_tile = [&](int t, f32x16_t& st) {
#pragma unroll
      for (int e = 0; e < 16; ++e) st[e] = 0.f;
#pragma unroll
      for (int ks = 0; ks < 6; ++ks) {
        const bf16x8_t af = *reinterpret_cast<const bf16x8_t*>(Vs + (32 * t + r) * KP + ks * 16 + 8 * hh);
        st = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af, dof[ks], st, 0, 0, 0);
      }
    };
    __builtin_amdgcn_wave_barrier();                             // doe written by both lane halves
    APH(2);

    // pass A: Dsum; the dropout bits of the wave's elements, 16 per key tile
    uint32_t km[FNT];
    float dsum = 0.f;
    auto pass_a = [&](auto tc, auto bandc) {
      constexpr int t = decltype(tc)::value;
      constexpr bool BAND = decltype(bandc)::value;
      f32x16_t st;
      dp_tile(t, st);
      float pt[16];
      load_p(t, pt);
      uint32_t m = 0;
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int j = 32 * t + 8 * (e >> 2) + 4 * hh + (e & 3);
        float dp = st[e];
        if (BAND) { const int rel = j - i + WIN; if ((unsigned)rel <= 2u * WIN) dp += doe[r * NW + rel]; }
        if (drop_thresh) {
          const bool keep = drop_keep(drop_seed, drow, j, drop_thresh);
          m |= (uint32_t)keep << e;
          dp = keep ? dp * drop_scale : 0.f;
        }
        dsum += dp * pt[e];                                      // j >= T: P is 0 and dp finite (V rows of zeros, DOE), the term is 0
      }
      km[t] = m;
    };
    // pass B: the tile's dPd^T again (6 MFMAs), dS^T into LDS, P'^T through the stage, the band tables, then dQ^T
    auto pass_b = [&](auto tc, auto bandc) {
      constexpr int t = decltype(tc)::value;
      constexpr bool BAND = decltype(bandc)::value;
      f32x16_t st;
      dp_tile(t, st);
      float pt[16];
      load_p(t, pt);
      const uint32_t m = km[t];
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int jl = 8 * (e >> 2) + 4 * hh + (e & 3), j = 32 * t + jl;
        const bool keep = (m >> e) & 1u;
        float dp = st[e];
        if (BAND) { const int rel = j - i + WIN; if ((unsigned)rel <= 2u * WIN) dp += doe[r * NW + rel]; }
        if (drop_thresh) dp = keep ? dp * drop_scale : 0.f;
        float ds = pt[e] * (dp - dsum) * inv_sqrt;
        float pd = pt[e];
        if (drop_thresh) pd = keep ? pd * drop_scale : 0.f;
        if (j >= jlive || qdead) ds = 0.f;                                   // masked_fill blocks the gradient (keys >= T or >= len)
        if (qdead) pd = 0.f;                                                 // padded queries carry no upstream gradient
        st[e] = ds;
        const bf16_t db = f2bf(ds), pb = f2bf(pd);
        dSs[j * DSP + i] = db;
        pw[jl * PWP + r] = pb;
        if (BAND) {
          const int rel = j - i + WIN;
          if ((unsigned)rel <= 2u * WIN && j < T) { dSB[r * 16 + rel] = db; dSBT[rel * BTP + r] = db; PdBT[rel * BTP + r] = pb; }
        }
      }
#pragma unroll
      for (int s2 = 0; s2 < 2; ++s2) {
        float f8[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) f8[e] = st[8 * s2 + e];
        const bf16x8_t pf = pack8(f8);
#pragma unroll
        for (int dt = 0; dt < 3; ++dt) {
          const bf16_t* ka = Ks + (32 * t + 16 * s2 + 4 * hh + qd) * VP + 32 * dt + colhalf + 4 * pp;
          const bf16x8_t af = tr_frag8(ka, ka + 8 * VP);
          o[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af, pf, o[dt], 0, 0, 0);
        }
      }
      // the tile's P'^T rows (keys) leave as 16-byte segments of 8 queries: lane -> (row, segment), two rows per lane
      __builtin_amdgcn_wave_barrier();
#pragma unroll
      for (int s2 = 0; s2 < 2; ++s2) {
        const int row = (lane >> 2) + 16 * s2, seg = lane & 3;
        const bf16x8_t x = *reinterpret_cast<const bf16x8_t*>(pw + row * PWP + 8 * seg);
        if (32 * t + row < T) *reinterpret_cast<bf16x8_t*>(pdt_base + (size_t)(32 * t + row) * TI + 32 * w + 8 * seg) = x;
      }
      __builtin_amdgcn_wave_barrier();
    };
    // key tiles below T, unrolled with the tile index a constant (as runtime loops over t, next tile's P prefetched, the kernel
    // measured 51.4 instead of 47.4 us at T = 150); the band of query tile w meets the key tiles w-1, w, w+1 only
    auto tiles = [&](auto&& f) {
      auto one = [&](auto tc) {
        constexpr int t = decltype(tc)::value;
        if (32 * t < T) {                                        // wave-uniform
          if (t + 1 >= w && t <= w + 1) f(tc, std::true_type{}); else f(tc, std::false_type{});
        }
      };
      one(ic_t<0>{}); one(ic_t<1>{}); one(ic_t<2>{}); one(ic_t<3>{}); one(ic_t<4>{});
    };
#pragma unroll
    for (int t = 0; t < FNT; ++t) km[t] = 0;
    tiles(pass_a);
    dsum += __shfl_xor(dsum, 32);
    APH(3);
#pragma unroll
    for (int dt = 0; dt < 3; ++dt) {
#pragma unroll
      for (int e = 0; e < 16; ++e) o[dt][e] = 0.f;
    }
    tiles(pass_b);
    APH(4);
    band_mfma(o, EkT, dSB, ln);
    if (i < T && rows.owns(i)) store_row96(dq + (rows.rbase + i) * lddq + h * D, o, hh);
  }
  APH(5);
  __syncthreads();                                               // with its workgroup-scope fences: the P'^T rows stored above are read back below by other waves of this workgroup
  APH(6);

  // ---- phase 2: K, V, Ev and DOE are dead; Q and dO take the operand areas
  const int nks = TI / 16;
  bf16x8_t bpd[2 * FNT];                                          // key 32 w + r's whole P'^T row: in flight under the staging below
  if (tile) {
    const int j = 32 * w + r, jc = j < T ? j : T - 1;
    const bf16_t* pdr = pdt_base + (size_t)jc * TI;
#pragma unroll
    for (int ks = 0; ks < 2 * FNT; ++ks) {
      const uint4 z = make_uint4(0, 0, 0, 0);
      bpd[ks] = __builtin_bit_cast(bf16x8_t, z);
      if (ks < nks) bpd[ks] = *reinterpret_cast<const bf16x8_t*>(pdr + 16 * ks + 8 * hh);
    }
  }
  bf16_t* Qs = Ks;
  bf16_t* dOs = Vs;                                              // [FTP][VP]
  for (int x = tid; x < FTP * (D / 8); x += FTH) {
    const int j = x / (D / 8), c8 = x - j * (D / 8);
    uint4 qq = make_uint4(0, 0, 0, 0), dd = qq;
    if (j < T) {
      qq = *reinterpret_cast<const uint4*>(q + rows.rw(j) * ld + h * D + c8 * 8);
      dd = *reinterpret_cast<const uint4*>(dout + rows.rw(j) * lddo + h * D + c8 * 8);
    }
    *reinterpret_cast<uint4*>(Qs + j * VP + c8 * 8) = qq;
    *reinterpret_cast<uint4*>(dOs + j * VP + c8 * 8) = dd;
  }
  for (int x = tid; x < 2 * NW * D; x += FTH) Acc[x] = 0.f;
  __syncthreads();
  APH(7);

  if (tile) {                                                    // key tile w: dK^T = Q^T dS, dV^T = dO^T P'
    const int j = 32 * w + r;
    const bf16_t* dsr = dSs + j * DSP;
    f32x16_t ak[3], av[3];
#pragma unroll
    for (int dt = 0; dt < 3; ++dt) {
#pragma unroll
      for (int e = 0; e < 16; ++e) { ak[dt][e] = 0.f; av[dt][e] = 0.f; }
    }
#pragma unroll
    for (int ks = 0; ks < 2 * FNT; ++ks) {
      if (ks < nks) {
        const bf16x8_t bds = *reinterpret_cast<const bf16x8_t*>(dsr + 16 * ks + 8 * hh);   // dS[i = 16ks+8hh.., j]
#pragma unroll
        for (int dt = 0; dt < 3; ++dt) {
          const bf16_t* qa = Qs + (16 * ks + 8 * hh + qd) * VP + 32 * dt + colhalf + 4 * pp;
          const bf16_t* da = dOs + (16 * ks + 8 * hh + qd) * VP + 32 * dt + colhalf + 4 * pp;
          ak[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(tr_frag8(qa, qa + 4 * VP), bds, ak[dt], 0, 0, 0);
          av[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(tr_frag8(da, da + 4 * VP), bpd[ks], av[dt], 0, 0, 0);
        }
      }
    }
    if (j < T && rows.owns(j)) {
      store_row96(dk + rows.rw(j) * lddq + h * D, ak, hh);
      store_row96(dv + rows.rw(j) * lddq + h * D, av, hh);
    }
  }
  APH(9);
  // dEk[r'][d] += sum_i dSBT[r'][i] Q[i][d];  dEv[r'][d] += sum_i PdBT[r'][i] dO[i][d]: the three waves without a key tile, query
  // tiles {0, 3}, {1, 4}, {2} chained in the MFMA accumulators (K = the queries of the wave's tiles), one LDS accumulation per wave
  if (w >= FNT && 32 * (w - FNT) < T) {
#pragma unroll
    for (int which = 0; which < 2; ++which) {
#pragma unroll
      for (int dt = 0; dt < 3; ++dt) {
        f32x16_t acc;
        zero16(acc);
#pragma unroll 1
        for (int x = w - FNT; x < FNT && 32 * x < T; x += 8 - FNT)
          de_chain(acc, WB + x * FBAND + 32 * 16 + (which ? 16 * BTP : 0), (which ? dOs : Qs) + 32 * x * VP, dt, ln);
        de_add(Acc + which * NW * D, acc, dt, ln);
      }
    }
  }
  APH(10);
  {                                                              // dS^T rows j < T, all TI columns, as 16-byte segments
    const int nseg = TI >> 3;
    for (int x = tid; x < T * nseg; x += FTH) {
      const int j = x / nseg, s = x - j * nseg;
      *reinterpret_cast<bf16x8_t*>(dst_base + (size_t)j * TI + 8 * s) = *reinterpret_cast<const bf16x8_t*>(dSs + j * DSP + 8 * s);
    }
  }
  __syncthreads();
  acc_flush(Acc, dEk, dEv, tid, FTH);
  APH(11);
}

int launch_bwd_fused(const gt_attn_call& c)        // T <= FTP
{
  const gt_attn_bwd_ws w(c);
  if (const int rc = gt_allow_lds<&gt_attn_bwd_fused_kernel>(160 * 1024)) return rc;
  hipLaunchKernelGGL(gt_attn_bwd_fused_kernel, dim3(c.H, c.B), dim3(FTH), FUSED_LDS, c.stream,
                     c.q, c.k, c.v, c.ld, c.Ek, c.Ev, c.lens, c.dout, c.lddo, c.P, w.dST, w.PdT, w.TI, c.dq, c.dk, c.dv, c.lddq, c.dEk, c.dEv,
                     c.T, c.Tp, c.row0, c.H, c.th, c.sd, c.sc, c.seed_dev);
  return gt_launch_status(__func__);
}

template <int NT, int WV>
int launch_bwd(const gt_attn_call& c)
{
  constexpr int TPAD = NT * 32;
  constexpr int WBN = BAND_TABLES + 2 * 32 * VP;
  constexpr size_t lds1 = (NT > 8 ? 0 : (size_t)TPAD * KP * 2) + (size_t)TPAD * VP * 2 + 32 * KP * 2 + D * 16 * 2 + 2 * NW * D * 4 +
                          (size_t)WV * 32 * NW * 4 + (size_t)WV * WBN * 2;
  constexpr size_t lds2 = (size_t)2 * TPAD * VP * 2;
  static_assert(lds1 <= 160 * 1024 && lds2 <= 160 * 1024, "LDS budget");
  const gt_attn_bwd_ws w(c);
  if (const int rc = gt_allow_lds<&gt_attn_bwd_q_mfma_kernel<NT, WV>>(160 * 1024)) return rc;
  if (const int rc = gt_allow_lds<&gt_attn_bwd_kv_mfma_kernel<NT>>(160 * 1024)) return rc;
  hipLaunchKernelGGL((gt_attn_bwd_q_mfma_kernel<NT, WV>), dim3((c.T + 32 * WV - 1) / (32 * WV), c.H, c.B), dim3(64 * WV), lds1, c.stream,
                     c.q, c.k, c.v, c.ld, c.Ek, c.Ev, c.lens, c.dout, c.lddo, c.P, w.dST, w.PdT, w.TI, c.dq, c.lddq, c.dEk, c.dEv,
                     c.T, c.Tp, c.row0, c.H, c.th, c.sd, c.sc, c.seed_dev);
  hipLaunchKernelGGL(gt_attn_bwd_kv_mfma_kernel<NT>, dim3((c.T + 127) / 128, c.H, c.B), dim3(256), lds2, c.stream,
                     c.q, c.ld, c.dout, c.lddo, w.dST, w.PdT, w.TI, c.dk, c.dv, c.lddq, c.T, c.Tp, c.row0, c.H);
  return gt_launch_status(__func__);
}

}  // namespace

#if ATTN_PHASES
extern "C" int gt_dev_attn_phases(void* dst, size_t bytes)
{
  return hipMemcpyFromSymbol(dst, HIP_SYMBOL(g_attn_ph), bytes < sizeof(g_attn_ph) ? bytes : sizeof(g_attn_ph)) == hipSuccess ? 0 : -1;
}
#endif

size_t gt_attn_bwd_mfma_ws_bytes(int B, int T, int H)
{
  const size_t TI = (size_t)((T + 31) / 32) * 32;
  return (size_t)2 * B * H * T * TI * 2;
}

// Which kernels a shape runs on: the one place where T is compared with the thresholds between the paths (internal.h names them).
// 160, 256, 384: what 5, 8, 12 key tiles of 32 hold; 505: the last T at which the generic backward's LDS holds an utterance-head.
gt_attn_path gt_attn_route(int T, int Dh, int win)
{
  static_assert(FTP == 160, "FUSED160 is what the one-workgroup backward holds: launch_bwd_fused checks no T of its own");
  if (T > GT_ATTN_LONG_MAX_T) return GT_ATTN_NONE;
  if (Dh != D || win != WIN) return GT_ATTN_GENERIC;
  if (T <= 160) return GT_ATTN_FUSED160;
  if (T <= 256) return GT_ATTN_MFMA256;
  if (T <= 384) return GT_ATTN_MFMA384;
  return T <= 505 ? GT_ATTN_GENERIC : GT_ATTN_LONG_P;
}

// The shapes the MFMA kernels take, in both directions (the generic kernels of encoder_ops.hip take the rest), exported so that a
// caller can tell which kernels a launch runs.
extern "C" int gt_attn_mfma_shape(int T, int Dh, int win)
{
  const gt_attn_path p = gt_attn_route(T, Dh, win);
  return p == GT_ATTN_FUSED160 || p == GT_ATTN_MFMA256 || p == GT_ATTN_MFMA384;
}

int gt_attn_bwd_mfma_impl(const gt_attn_call& c, gt_attn_path path)
{
  // T <= 160: the whole backward of one (utterance, head) in one workgroup (gt_attn_bwd_fused_kernel)
  if (path == GT_ATTN_FUSED160) return launch_bwd_fused(c);
  // 161 <= T <= 256: 8 key tiles, 2 waves per workgroup (153 KB of LDS), one score tile live at a time (recompute form:
  // the first version kept all 8 tiles in registers, needed scratch and faulted — see DESIGN.md §4.5)
  if (path == GT_ATTN_MFMA256) return launch_bwd<8, 2>(c);
  // 257 <= T <= 384 (cfg3): 12 key tiles; K^T (transposing reads) stays in LDS, the V rows come from L2
  return launch_bwd<12, 4>(c);
}

int gt_attn_fwd_mfma_impl(const gt_attn_call& c, gt_attn_path path)
{
  if (path == GT_ATTN_FUSED160) return launch_fwd<5>(c);
  if (path == GT_ATTN_MFMA256) return launch_fwd<8>(c);
  return launch_fwd_long<12>(c);
}
