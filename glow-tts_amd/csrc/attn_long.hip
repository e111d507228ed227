// Relative-position attention for long texts (505 < T <= GT_ATTN_LONG_MAX_T; D = 96, window 4) on bf16 MFMA for gfx950.
//
// Same contract, lane mapping and arithmetic as the <12> kernels of attn_mfma.hip (read that file first; the tile pieces both files
// are made of are in attn_frag.h): one score tile live at a time, two walks over the key tiles.  What changes: the tile count is a
// runtime loop and NO full-length operand sits in LDS or in registers.
//   * operands read as plain rows (K in the forward, V in the backward pass 1, the dS^T / P'^T columns in pass 2) come
//     straight from L2 into registers, one tile ahead;
//   * operands read through transposing LDS reads (V in the forward, K in pass 1, Q and dO in pass 2) are staged per
//     32-row tile in a two-slot LDS ring shared by the workgroup: every thread loads its share of tile t+1 into registers
//     before tile t is consumed, drops it into the other slot afterwards, and ONE barrier per tile closes the step (slot
//     (t+1)&1 was last read in step t-1, which every wave has left).  Waves that own no query (key) rows still stage.
// LDS per workgroup: forward 30 720 B, pass 1 72 448 B, pass 2 24 576 B — whatever T is.
#include <stdlib.h>
#include "attn_frag.h"
#include "internal.h"

namespace {
using namespace gt_attn_frag;

constexpr int TILE_U4 = 32 * (D / 8);          // uint4s of one staged [32][VP] tile (384)

// one [32][VP] tile of rows 32t .. 32t+31 (rows >= T zero): thread tid holds uint4 x = tid + 256u, u < 2.  Both macros read the
// kernel's own tid, h and T, and the load its Rows `rows`
#define GT_TILE_LOAD(regs, src, lds_, t)                                                       \
  _Pragma("unroll") for (int u_ = 0; u_ < 2; ++u_) {                                           \
    const int x_ = tid + 256 * u_;                                                             \
    const int row_ = x_ / (D / 8), c8_ = x_ - row_ * (D / 8);                                  \
    uint4 val_ = make_uint4(0, 0, 0, 0);                                                       \
    if (x_ < TILE_U4 && 32 * (t) + row_ < T)                                                   \
      val_ = *reinterpret_cast<const uint4*>((src) + rows.rw(32 * (t) + row_) * (lds_) + h * D + c8_ * 8); \
    (regs)[u_] = val_;                                                                         \
  }
#define GT_TILE_STORE(slot, regs)                                                              \
  _Pragma("unroll") for (int u_ = 0; u_ < 2; ++u_) {                                           \
    const int x_ = tid + 256 * u_;                                                             \
    const int row_ = x_ / (D / 8), c8_ = x_ - row_ * (D / 8);                                  \
    if (x_ < TILE_U4) *reinterpret_cast<uint4*>((slot) + row_ * VP + c8_ * 8) = (regs)[u_];    \
  }

// =========================================================================================
// Forward: one workgroup per (utterance, head, 128 queries), a wave owns 32 queries.  One body, three kernels:
// STORE_P = false (gt_attn_fwd with P == NULL: a forward nobody differentiates, synthesis): pass 2 leaves out its P stores and
// nothing else, so `out` is the same bit for bit.
// STATS (gt_attn_long_fwd_stats_kernel, gt_attn_fwd_stats: the training forward whose backward recomputes P): no P either; after
// pass 1 every query row i < T, padded ones included, stores the pair it holds, (mx, rden) = (maximum of the masked, scaled scores,
// 1 / denominator), to Pout = stats[B, H, T, 2].  With them P[i, j] = __expf(s - mx) * rden is pass 2's expression on the same values.
template <bool STORE_P, bool STATS>
GT_ATTN_DEV void long_fwd_body(
    const bf16_t* __restrict__ q, const bf16_t* __restrict__ k, const bf16_t* __restrict__ v, int ld,
    const float* __restrict__ Ek, const float* __restrict__ Ev, const int32_t* __restrict__ lens,
    bf16_t* __restrict__ out, int ldo, float* __restrict__ Pout,
    int T, int Tp, const int32_t* row0, int H, uint32_t drop_thresh, uint32_t drop_seed, float drop_scale, const uint32_t* __restrict__ seed_dev)
{
  if (seed_dev) drop_seed ^= *seed_dev;
  __shared__ __attribute__((aligned(16))) bf16_t Vr[2 * 32 * VP];   // V ring: two [32][VP] tiles
  __shared__ __attribute__((aligned(16))) bf16_t Eks[32 * KP];      // rows >= 9 are zero
  __shared__ __attribute__((aligned(16))) bf16_t EvT[D * 16];       // EvT[d][r], r >= 9 zero
  __shared__ __attribute__((aligned(16))) float  QE[4 * 32 * NW];
  __shared__ __attribute__((aligned(16))) bf16_t PB[4 * 32 * 16];

  const int b = blockIdx.z, h = blockIdx.y;
  const int tid = threadIdx.x, w = tid >> 6;
  const Lane ln(tid & 63);
  const int r = ln.r, hh = ln.hh;
  const int len = lens[b];
  const Rows rows(row0, b, Tp);

  stage_rel_rows(Eks, Ek, tid, 256);
  stage_rel_tr(EvT, Ev, tid, 256);
  for (int i = tid; i < 4 * 32 * 16; i += 256) PB[i] = 0;
  const int nt = (T + 31) >> 5;                                  // key tiles that hold keys (uniform)
  uint4 vr[2];
  GT_TILE_LOAD(vr, v, ld, 0)
  GT_TILE_STORE(Vr, vr)
  __syncthreads();

  const int i0 = blockIdx.x * 128 + 32 * w;
  const bool active = i0 < T;                                    // wave-uniform
  const int i = i0 + r;
  const int ic = i < T ? i : T - 1;
  float* qe = QE + w * 32 * NW;
  bf16_t* pb = PB + w * 32 * 16;
  const float inv_sqrt = rsqrtf((float)D);

  bf16x8_t qf[6];
  load_frag6(qf, q + rows.rw(ic) * ld + h * D, hh);
  if (active) rel_table(qe, Eks, qf, ln);
  __builtin_amdgcn_wave_barrier();

  // masked, scaled scores of one tile from its K fragments (L2, one tile ahead)
  auto scores = [&](int t, const bf16x8_t* kf, f32x16_t& st) {
    mfma6(st, kf, qf);
    score_tile(st, t, qe + r * NW, i, hh, T, len, inv_sqrt);
  };

  // ---- pass 1 (no LDS operand, no barrier): online max / denominator over this lane's keys, then the lane halves merge
  float mx = -3.0e38f, den = 0.f;
  bf16x8_t kf[6], kn[6];
  if (active) {
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
  }
  const float rden = active ? 1.0f / den : 0.f;
  if (STATS && active && hh == 0 && i < T)                        // every query row, padded ones included
    *reinterpret_cast<float2*>(Pout + (((size_t)b * H + h) * T + i) * 2) = make_float2(mx, rden);

  // ---- pass 2: P = softmax, dropout, O^T = V^T P^T (+ Ev^T band(P)^T); V tile t in ring slot t & 1
  float* prow = STORE_P ? Pout + (((size_t)b * H + h) * T + ic) * T : nullptr;
  const Drop drop{drop_thresh, drop_seed, (uint32_t)((b * H + h) * T + i), drop_scale};
  const bool vec = (T & 3) == 0;
  f32x16_t o[3];
  zero3(o);
  if (active) load_tile_frag6(kf, k, ld, h, 0, T, rows, ln);
#pragma unroll 1
  for (int t = 0; t < nt; ++t) {
    if (t + 1 < nt) {
      GT_TILE_LOAD(vr, v, ld, t + 1)
      if (active) load_tile_frag6(kn, k, ld, h, t + 1, T, rows, ln);
    }
    if (active) {
      f32x16_t st;
      scores(t, kf, st);
#pragma unroll
      for (int e = 0; e < 16; ++e) st[e] = __expf(st[e] - mx) * rden;
      p_tile_out<STORE_P>(st, t, prow, vec, i, ln, T, drop, pb);
      acc_operand(o, st, Vr + (t & 1) * 32 * VP, ln);
      copy_frag6(kf, kn);
    }
    if (t + 1 < nt) { GT_TILE_STORE(Vr + ((t + 1) & 1) * 32 * VP, vr) }
    __syncthreads();
  }
  if (!active) return;
  band_mfma(o, EvT, pb, ln);
  if (i < T && rows.owns(i)) store_row96(out + (rows.rbase + i) * ldo + h * D, o, hh);
}

template <bool STORE_P>
__global__ __launch_bounds__(256, 2) void gt_attn_long_fwd_kernel(
    const bf16_t* __restrict__ q, const bf16_t* __restrict__ k, const bf16_t* __restrict__ v, int ld,
    const float* __restrict__ Ek, const float* __restrict__ Ev, const int32_t* __restrict__ lens,
    bf16_t* __restrict__ out, int ldo, float* __restrict__ Pout,
    int T, int Tp, const int32_t* row0, int H, uint32_t drop_thresh, uint32_t drop_seed, float drop_scale, const uint32_t* __restrict__ seed_dev)
{
  long_fwd_body<STORE_P, false>(q, k, v, ld, Ek, Ev, lens, out, ldo, Pout, T, Tp, row0, H, drop_thresh, drop_seed, drop_scale, seed_dev);
}

__global__ __launch_bounds__(256, 2) void gt_attn_long_fwd_stats_kernel(
    const bf16_t* __restrict__ q, const bf16_t* __restrict__ k, const bf16_t* __restrict__ v, int ld,
    const float* __restrict__ Ek, const float* __restrict__ Ev, const int32_t* __restrict__ lens,
    bf16_t* __restrict__ out, int ldo, float* __restrict__ Pout,
    int T, int Tp, const int32_t* row0, int H, uint32_t drop_thresh, uint32_t drop_seed, float drop_scale, const uint32_t* __restrict__ seed_dev)
{
  long_fwd_body<false, true>(q, k, v, ld, Ek, Ev, lens, out, ldo, Pout, T, Tp, row0, H, drop_thresh, drop_seed, drop_scale, seed_dev);
}

// =========================================================================================
// Backward pass 1 (dS, P', dQ, dEk, dEv): the one-tile recompute form of gt_attn_bwd_q_mfma_kernel<12, 4>, 4 waves x 32 queries, in
// one body for two kernels.
// Saved P (gt_attn_long_bwd_q_kernel): pass A (Dsum) reads V rows and P only — no LDS operand, no barrier; pass B stages K per tile
// for the transposing reads of dQ^T (tile t in ring slot t & 1) and stores dS^T / P'^T for pass 2.
// STATS (gt_attn_long_bwd_q_stats_kernel, the P-free backward gt_attn_bwd_stats: nothing of size T^2 is read or written): P is
// recomputed tile by tile from q, k, Ek and the forward's row statistics, P[i, j] = __expf(s[i, j] - mx_i) * rden_i — the forward's
// `scores` (K fragment as A, Q fragment as B, band, scale, mask) and its P expression — so P, Dsum, the bf16 dS operand and the dQ
// chain are the saved-P kernel's bit for bit: it is the same code.  What it adds:
//   * a QE table next to DOE (LDS_BWD_QS); the bf16 Ek rows of its chain are read out of EkT (the same f2bf values as the forward's
//     Eks image), so no second Ek image is staged;
//   * this wave's Q rows sit in its QD strip (free until the dEk / dEv contractions at the end) and the Q fragment of an MFMA is a
//     16-byte row read there: 24 registers fewer than holding them.  Rows >= T are zero; the forward read row T - 1 there, and in
//     both nothing computed for such a query is stored;
//   * the K fragments of the score MFMAs are 16-byte row reads of the K ring that pass B stages anyway; pass A stages the same ring
//     (one barrier per tile there too) instead of holding a second set of K fragments and their prefetch copy in registers: that
//     keeps the kernel at two workgroups per CU.  Tile t of pass A sits in slot t & 1; its last step stages tile 0 again (and
//     prefetches V of tile 0), so tile t of pass B sits in slot (nt + t) & 1;
//   * no dS^T / P'^T workspace; instead one record of WSQ floats per query row i < T of every (b, h) for the key side:
//       [0] Dsum_i   [1 .. 9] q_i . Ek[r]   [10 .. 18] dO_i . Ev[r]   [19] zero
//     (the qe / doe band tables, so both kernels add the same bits on the band).
// The Q / dO tiles of the dEk / dEv contraction share the per-wave QD area, loaded one after the other at the end.
constexpr int WSQ = 20;
constexpr int LWBN = BAND_TABLES + 32 * VP;                    // per wave: dSB[32][16] | dSBT[16][BTP] | PdBT[16][BTP] | QD[32][VP]
constexpr size_t LDS_BWD_Q = (size_t)2 * 32 * VP * 2 + 32 * KP * 2 + D * 16 * 2 + 2 * NW * D * 4 + 4 * 32 * NW * 4 + (size_t)4 * LWBN * 2;
constexpr size_t LDS_BWD_QS = LDS_BWD_Q + (size_t)4 * 32 * NW * 4;

template <bool STATS>
GT_ATTN_DEV void long_bwd_q_body(
    const bf16_t* __restrict__ q, const bf16_t* __restrict__ k, const bf16_t* __restrict__ v, int ld,
    const float* __restrict__ Ek, const float* __restrict__ Ev, const int32_t* __restrict__ lens,
    const bf16_t* __restrict__ dout, int lddo, const float* __restrict__ P, const float* __restrict__ stats, float* __restrict__ wsq,
    bf16_t* __restrict__ dST, bf16_t* __restrict__ PdT, int TI,
    bf16_t* __restrict__ dq, int lddq, float* __restrict__ dEk, float* __restrict__ dEv,
    int T, int Tp, const int32_t* row0, int H, uint32_t drop_thresh, uint32_t drop_seed, float drop_scale, const uint32_t* __restrict__ seed_dev)
{
  if (seed_dev) drop_seed ^= *seed_dev;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  bf16_t* Kr  = reinterpret_cast<bf16_t*>(smem);                 // K ring: two [32][VP] tiles
  bf16_t* Evs = Kr + 2 * 32 * VP;                                // [32][KP]    rows >= 9 zero
  bf16_t* EkT = Evs + 32 * KP;                                   // [96][16]
  float*  Acc = reinterpret_cast<float*>(EkT + D * 16);          // [2][NW][D]  block-local dEk | dEv
  float*  DOE = Acc + 2 * NW * D;                                // [4][32][NW]
  float*  QE  = STATS ? DOE + 4 * 32 * NW : nullptr;             // [4][32][NW] STATS only
  bf16_t* WB  = reinterpret_cast<bf16_t*>(DOE + (STATS ? 2 : 1) * 4 * 32 * NW);   // [4][LWBN]

  const int b = blockIdx.z, h = blockIdx.y;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const Lane ln(lane);
  const int r = ln.r, hh = ln.hh;
  const int len = lens[b];
  const Rows rows(row0, b, Tp);

  stage_rel_rows(Evs, Ev, tid, 256);
  stage_rel_tr(EkT, Ek, tid, 256);
  for (int i = tid; i < 2 * NW * D; i += 256) Acc[i] = 0.f;
  for (int i = tid; i < 4 * BAND_TABLES; i += 256) {             // band tables start at zero
    const int ww = i / BAND_TABLES, o = i - ww * BAND_TABLES;
    WB[ww * LWBN + o] = 0;
  }
  const int nt = (T + 31) >> 5;                                  // key tiles that hold keys (uniform)
  uint4 kr[2];
  GT_TILE_LOAD(kr, k, ld, 0)
  GT_TILE_STORE(Kr, kr)
  __syncthreads();

  const int i0 = (blockIdx.x * 4 + w) * 32;
  const bool active = i0 < T;                                    // wave-uniform
  const int i = i0 + r;
  const int ic = i < T ? i : T - 1;
  float* doe = DOE + w * 32 * NW;
  float* qe = STATS ? QE + w * 32 * NW : nullptr;
  bf16_t* bt = WB + w * LWBN;                                    // dSB | dSBT | PdBT
  bf16_t* QD = bt + BAND_TABLES;
  const size_t bhT = ((size_t)b * H + h) * T;

  bf16x8_t dof[6];
  load_frag6(dof, dout + rows.rw(ic) * lddo + h * D, hh);
  // this wave's rows of src (Q or dO) into its QD strip, rows >= T zero
  auto stage_qd = [&](const bf16_t* src, int lds_) {
    for (int c = lane; c < 32 * (D / 8); c += 64) {
      const int rr = c / (D / 8), c8 = c - rr * (D / 8);
      uint4 x = make_uint4(0, 0, 0, 0);
      if (i0 + rr < T) x = *reinterpret_cast<const uint4*>(src + rows.rw(i0 + rr) * lds_ + h * D + c8 * 8);
      *reinterpret_cast<uint4*>(QD + rr * VP + c8 * 8) = x;
    }
  };
  auto qf = [&](int ks) { return *reinterpret_cast<const bf16x8_t*>(QD + r * VP + ks * 16 + 8 * hh); };   // STATS
  if constexpr (STATS) {
    stage_qd(q, ld);
    __builtin_amdgcn_wave_barrier();
  }
  if (active) {
    rel_table(doe, Evs, dof, ln);
    if constexpr (STATS) {
      f32x16_t acq;
      zero16(acq);
#pragma unroll
      for (int ks = 0; ks < 6; ++ks) {
        s16x8_t ek = {0, 0, 0, 0, 0, 0, 0, 0};                      // row r of bf16 Ek (rows >= 9 zero), out of its transposed image
        if (r < NW) {
#pragma unroll
          for (int x = 0; x < 8; ++x) ek[x] = (short)EkT[(ks * 16 + 8 * hh + x) * 16 + r];
        }
        acq = mfma(__builtin_bit_cast(bf16x8_t, ek), qf(ks), acq);
      }
      rel_store(qe, acq, ln);
    }
  }
  __builtin_amdgcn_wave_barrier();

  const float inv_sqrt = rsqrtf((float)D);
  const Drop drop{drop_thresh, drop_seed, (uint32_t)((b * H + h) * T + i), drop_scale};
  const float* prow = nullptr;
  bf16_t* dst_base = nullptr;
  bf16_t* pdt_base = nullptr;
  float mx = 0.f, rden = 0.f;
  if constexpr (STATS) { mx = stats[(bhT + ic) * 2]; rden = stats[(bhT + ic) * 2 + 1]; }
  else { prow = P + (bhT + ic) * T; dst_base = dST + bhT * TI; pdt_base = PdT + bhT * TI; }
  const int palign = (T & 3) == 0 ? 4 : 1;

  // STATS: P of one tile from the staged K tile Ks (rows >= T zero, as the forward's K fragments): the forward's scores, then its
  // P expression (element e <-> key 32t + (e&3) + 8(e>>2) + 4hh)
  auto p_tile = [&](int t, const bf16_t* Ks, f32x16_t& sp) {
    zero16(sp);
#pragma unroll
    for (int ks = 0; ks < 6; ++ks) sp = mfma(*reinterpret_cast<const bf16x8_t*>(Ks + r * VP + ks * 16 + 8 * hh), qf(ks), sp);
    score_tile(sp, t, qe + r * NW, i, hh, T, len, inv_sqrt);
#pragma unroll
    for (int e = 0; e < 16; ++e) sp[e] = __expf(sp[e] - mx) * rden;
  };

  // ---- pass A: Dsum = sum_j dP P
  float dsum = 0.f;
  bf16x8_t vf[6], vn[6];
  if (active) load_tile_frag6(vf, v, ld, h, 0, T, rows, ln);
#pragma unroll 1
  for (int t = 0; t < nt; ++t) {
    const int tn = t + 1 < nt ? t + 1 : 0;                       // STATS wraps to tile 0
    if constexpr (STATS) { GT_TILE_LOAD(kr, k, ld, tn) }
    if (active) {
      if (STATS || t + 1 < nt) load_tile_frag6(vn, v, ld, h, tn, T, rows, ln);
      f32x16_t st;
      [[maybe_unused]] f32x16_t sp;                              // STATS: P of the tile
      if constexpr (STATS) p_tile(t, Kr + (t & 1) * 32 * VP, sp);
      mfma6(st, vf, dof);
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int j0 = 32 * t + 8 * g + 4 * hh;
        float p4[4];
        if constexpr (STATS) {
#pragma unroll
          for (int e2 = 0; e2 < 4; ++e2) p4[e2] = sp[4 * g + e2];
        } else {
          load_p4(prow, j0, T, palign, p4);                      // the saved row
        }
#pragma unroll
        for (int e2 = 0; e2 < 4; ++e2) dsum += dp_elem(st[4 * g + e2], doe + r * NW, i, j0 + e2, T, drop) * p4[e2];
      }
      copy_frag6(vf, vn);
    }
    if constexpr (STATS) {
      GT_TILE_STORE(Kr + ((t + 1) & 1) * 32 * VP, kr)
      __syncthreads();
    }
  }
  if (active) {
    dsum += __shfl_xor(dsum, 32);
    if (STATS && i < T) {                                        // what the key side needs of this query row
      float* rec = wsq + (bhT + i) * WSQ;
      const float* tab = hh ? doe : qe;
      if (hh == 0) rec[0] = dsum; else rec[WSQ - 1] = 0.f;
#pragma unroll
      for (int x = 0; x < NW; ++x) rec[1 + NW * hh + x] = tab[r * NW + x];
    }
    if constexpr (!STATS) load_tile_frag6(vf, v, ld, h, 0, T, rows, ln);
  }

  // ---- pass B: dPd^T (and P) per tile again, dS^T, dQ^T += K^T dS^T; K tile t in ring slot (slot0 + t) & 1
  const int slot0 = STATS ? nt & 1 : 0;
  f32x16_t o[3];
  zero3(o);
#pragma unroll 1
  for (int t = 0; t < nt; ++t) {
    if (t + 1 < nt) {
      GT_TILE_LOAD(kr, k, ld, t + 1)
      if (active) load_tile_frag6(vn, v, ld, h, t + 1, T, rows, ln);
    }
    if (active) {
      const bf16_t* Ks = Kr + ((slot0 + t) & 1) * 32 * VP;
      f32x16_t st;
      [[maybe_unused]] f32x16_t sp;
      if constexpr (STATS) p_tile(t, Ks, sp);
      mfma6(st, vf, dof);
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int j0 = 32 * t + 8 * g + 4 * hh;
        float p4[4];
        if constexpr (STATS) {
#pragma unroll
          for (int e2 = 0; e2 < 4; ++e2) p4[e2] = sp[4 * g + e2];
        } else {
          load_p4(prow, j0, T, palign, p4);                      // the saved row
        }
#pragma unroll
        for (int e2 = 0; e2 < 4; ++e2) {
          const int j = j0 + e2;
          float pd;
          const float ds = ds_elem(p4[e2], dp_elem(st[4 * g + e2], doe + r * NW, i, j, T, drop), dsum, inv_sqrt, i, j, T, len, drop, pd);
          st[4 * g + e2] = ds;
          if (j < T) {
            if constexpr (!STATS) {
              dst_base[(size_t)j * TI + i] = f2bf(ds);
              pdt_base[(size_t)j * TI + i] = f2bf(pd);
            }
            band_tables(bt, r, i, j, ds, pd);
          }
        }
      }
      acc_operand(o, st, Ks, ln);
      copy_frag6(vf, vn);
    }
    if (t + 1 < nt) { GT_TILE_STORE(Kr + ((slot0 + t + 1) & 1) * 32 * VP, kr) }
    __syncthreads();
  }

  if (active) {
    band_mfma(o, EkT, bt, ln);
    if (i < T && rows.owns(i)) store_row96(dq + (rows.rbase + i) * lddq + h * D, o, hh);
    // dEk[r'][d] += sum_i dSBT[r'][i] Q[i][d];  dEv[r'][d] += sum_i PdBT[r'][i] dO[i][d]   (K = 32 queries, one MFMA chain)
#pragma unroll 1
    for (int which = 0; which < 2; ++which) {
      __builtin_amdgcn_wave_barrier();                             // the previous contraction has read QD
      stage_qd(which ? dout : q, which ? lddo : ld);
      __builtin_amdgcn_wave_barrier();
      de_contract(Acc + which * NW * D, bt + 32 * 16 + which * 16 * BTP, QD, ln);
    }
  }
  __syncthreads();
  acc_flush(Acc, dEk, dEv, tid, 256);
}

__global__ __launch_bounds__(256, 2) void gt_attn_long_bwd_q_kernel(
    const bf16_t* __restrict__ q, const bf16_t* __restrict__ k, const bf16_t* __restrict__ v, int ld,
    const float* __restrict__ Ek, const float* __restrict__ Ev, const int32_t* __restrict__ lens,
    const bf16_t* __restrict__ dout, int lddo, const float* __restrict__ P,
    bf16_t* __restrict__ dST, bf16_t* __restrict__ PdT, int TI,
    bf16_t* __restrict__ dq, int lddq, float* __restrict__ dEk, float* __restrict__ dEv,
    int T, int Tp, const int32_t* row0, int H, uint32_t drop_thresh, uint32_t drop_seed, float drop_scale, const uint32_t* __restrict__ seed_dev)
{
  long_bwd_q_body<false>(q, k, v, ld, Ek, Ev, lens, dout, lddo, P, nullptr, nullptr, dST, PdT, TI, dq, lddq, dEk, dEv,
                         T, Tp, row0, H, drop_thresh, drop_seed, drop_scale, seed_dev);
}

__global__ __launch_bounds__(256, 2) void gt_attn_long_bwd_q_stats_kernel(
    const bf16_t* __restrict__ q, const bf16_t* __restrict__ k, const bf16_t* __restrict__ v, int ld,
    const float* __restrict__ Ek, const float* __restrict__ Ev, const int32_t* __restrict__ lens,
    const bf16_t* __restrict__ dout, int lddo, const float* __restrict__ stats, float* __restrict__ wsq,
    bf16_t* __restrict__ dq, int lddq, float* __restrict__ dEk, float* __restrict__ dEv,
    int T, int Tp, const int32_t* row0, int H, uint32_t drop_thresh, uint32_t drop_seed, float drop_scale, const uint32_t* __restrict__ seed_dev)
{
  long_bwd_q_body<true>(q, k, v, ld, Ek, Ev, lens, dout, lddo, nullptr, stats, wsq, nullptr, nullptr, 0, dq, lddq, dEk, dEv,
                        T, Tp, row0, H, drop_thresh, drop_seed, drop_scale, seed_dev);
}

// =========================================================================================
// Backward pass 2 (dK, dV): one workgroup per (utterance, head, 128 keys), a wave owns 32 keys and walks the 32-query
// tiles.  Q and dO rows of a tile go through the LDS ring (transposing reads); the dS^T / P'^T columns of the wave's keys
// come straight from the pass-1 workspace, one tile ahead.  dK = dS^T Q and dV = P'^T dO accumulate in registers.
__global__ __launch_bounds__(256, 2) void gt_attn_long_bwd_kv_kernel(
    const bf16_t* __restrict__ q, int ld, const bf16_t* __restrict__ dout, int lddo,
    const bf16_t* __restrict__ dST, const bf16_t* __restrict__ PdT, int TI,
    bf16_t* __restrict__ dk, bf16_t* __restrict__ dv, int lddk, int T, int Tp, const int32_t* row0, int H)
{
  __shared__ __attribute__((aligned(16))) bf16_t Qr[2 * 32 * VP];   // Q ring: two [32][VP] tiles
  __shared__ __attribute__((aligned(16))) bf16_t Or[2 * 32 * VP];   // dO ring
  const int b = blockIdx.z, h = blockIdx.y;
  const int tid = threadIdx.x, w = tid >> 6;
  const Lane ln(tid & 63);
  const int r = ln.r, hh = ln.hh;
  const Rows rows(row0, b, Tp);

  const int nqt = TI >> 5;                                       // query tiles (uniform); TI = ceil(T/32)*32
  uint4 qr[2], dr[2];
  GT_TILE_LOAD(qr, q, ld, 0)
  GT_TILE_LOAD(dr, dout, lddo, 0)
  GT_TILE_STORE(Qr, qr)
  GT_TILE_STORE(Or, dr)
  __syncthreads();

  const int j0 = blockIdx.x * 128 + 32 * w;
  const bool active = j0 < T;                                    // wave-uniform
  const int j = j0 + r, jc = j < T ? j : T - 1;
  const bf16_t* dsr = dST + (((size_t)b * H + h) * T + jc) * TI;
  const bf16_t* pdr = PdT + (((size_t)b * H + h) * T + jc) * TI;
  f32x16_t ak[3], av[3];
  zero3(ak);
  zero3(av);
  // columns i = 32t + 16ks + 8hh .. +7 of this lane's key row: dS[i, j], P'[i, j]
  auto load_cols = [&](int t, bf16x8_t* bds, bf16x8_t* bpd) {
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      bds[ks] = *reinterpret_cast<const bf16x8_t*>(dsr + 32 * t + 16 * ks + 8 * hh);
      bpd[ks] = *reinterpret_cast<const bf16x8_t*>(pdr + 32 * t + 16 * ks + 8 * hh);
    }
  };
  bf16x8_t bds[2], bpd[2], nds[2], npd[2];
  if (active) load_cols(0, bds, bpd);
#pragma unroll 1
  for (int t = 0; t < nqt; ++t) {
    if (t + 1 < nqt) {
      GT_TILE_LOAD(qr, q, ld, t + 1)
      GT_TILE_LOAD(dr, dout, lddo, t + 1)
      if (active) load_cols(t + 1, nds, npd);
    }
    if (active) {
#pragma unroll
      for (int ks = 0; ks < 2; ++ks)
        kv_pair(ak, av, Qr + (t & 1) * 32 * VP, Or + (t & 1) * 32 * VP, ks, bds[ks], bpd[ks], ln);
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) { bds[ks] = nds[ks]; bpd[ks] = npd[ks]; }
    }
    if (t + 1 < nqt) {
      GT_TILE_STORE(Qr + ((t + 1) & 1) * 32 * VP, qr)
      GT_TILE_STORE(Or + ((t + 1) & 1) * 32 * VP, dr)
    }
    __syncthreads();
  }
  if (active && j < T && rows.owns(j)) {
    store_row96(dk + rows.rw(j) * lddk + h * D, ak, hh);
    store_row96(dv + rows.rw(j) * lddk + h * D, av, hh);
  }
}

// Key side of the P-free backward: one workgroup per (utterance, head, 128 keys), a wave owns 32 keys, keeps their K and V fragments
// in registers (lane = key r, k-half hh) and walks the 32-query tiles below lens[b] (tiles wholly past it add nothing).
// Per tile:  S = Q K^T and dP' = dO V^T with the tile's Q / dO rows (16-byte row reads of the ring) as the A operand and the
// wave's K / V fragments as B, so a lane holds key j = j0 + r and accumulator element e holds query
//     i = 32t + (e&3) + 8(e>>2) + 4hh;
// the band terms come from the query side's records (only the tiles next to the wave's keys touch the band), then P, the keep
// bit, dS and P' as on the query side, per-query mx / rden / Dsum out of an LDS ring staged one tile ahead.
// The accumulators are then the B operand of dK^T = Q^T dS and dV^T = dO^T P' (acc_operand, with queries where the forward's P'V
// product and the query side's dQ product have keys).
// One workgroup per CU: the K / V fragments (48 registers), the two accumulator sets (96) and the two score tiles (32) do not fit
// the 256 registers a lane has at two.
__global__ __launch_bounds__(256, 1) void gt_attn_long_bwd_kv_stats_kernel(
    const bf16_t* __restrict__ q, const bf16_t* __restrict__ k, const bf16_t* __restrict__ v, int ld,
    const int32_t* __restrict__ lens, const bf16_t* __restrict__ dout, int lddo,
    const float* __restrict__ stats, const float* __restrict__ wsq,
    bf16_t* __restrict__ dk, bf16_t* __restrict__ dv, int lddk, int T, int Tp, const int32_t* row0, int H,
    uint32_t drop_thresh, uint32_t drop_seed, float drop_scale, const uint32_t* __restrict__ seed_dev)
{
  if (seed_dev) drop_seed ^= *seed_dev;
  __shared__ __attribute__((aligned(16))) bf16_t Qr[2 * 32 * VP];   // Q ring: two [32][VP] tiles
  __shared__ __attribute__((aligned(16))) bf16_t Or[2 * 32 * VP];   // dO ring
  __shared__ __attribute__((aligned(16))) float  Sr[2 * 3 * 32];    // per-query ring: mx[32] | rden[32] | Dsum[32]
  const int b = blockIdx.z, h = blockIdx.y;
  const int tid = threadIdx.x, w = tid >> 6;
  const Lane ln(tid & 63);
  const int r = ln.r, hh = ln.hh;
  const int len = lens[b];
  const Rows rows(row0, b, Tp);
  const size_t bhT = ((size_t)b * H + h) * T;

  const int nq = len < T ? len : T;
  const int nqt = (nq + 31) >> 5;                                // query tiles that hold an unpadded query (uniform)
  // the per-query triple of tile t: thread tid < 96 holds entry tid of mx[32] | rden[32] | Dsum[32]; queries >= T zero
  auto load_row = [&](int t) {
    const int i = 32 * t + (tid & 31);
    if (tid >= 96 || i >= T) return 0.f;
    return tid < 64 ? stats[(bhT + i) * 2 + (tid >> 5)] : wsq[(bhT + i) * WSQ];
  };
  uint4 qr[2], dr[2];
  float sr = load_row(0);
  GT_TILE_LOAD(qr, q, ld, 0)
  GT_TILE_LOAD(dr, dout, lddo, 0)
  GT_TILE_STORE(Qr, qr)
  GT_TILE_STORE(Or, dr)
  if (tid < 96) Sr[tid] = sr;
  __syncthreads();

  const int j0 = blockIdx.x * 128 + 32 * w;
  const bool active = j0 < T;                                    // wave-uniform
  const int j = j0 + r;
  const int tj = j0 >> 5;                                        // the query tile of this wave's keys: tiles tj - 1 .. tj + 1 touch the band
  const float inv_sqrt = rsqrtf((float)D);
  bf16x8_t kf[6], vf[6];
  if (active && j < T) {
    load_frag6(kf, k + rows.rw(j) * ld + h * D, hh);
    load_frag6(vf, v + rows.rw(j) * ld + h * D, hh);
  } else {
    zero_frag6(kf);
    zero_frag6(vf);
  }
  f32x16_t ak[3], av[3];
  zero3(ak);
  zero3(av);
#pragma unroll 1
  for (int t = 0; t < nqt; ++t) {
    if (t + 1 < nqt) {
      GT_TILE_LOAD(qr, q, ld, t + 1)
      GT_TILE_LOAD(dr, dout, lddo, t + 1)
      sr = load_row(t + 1);
    }
    if (active) {
      const bf16_t* Qs = Qr + (t & 1) * 32 * VP;
      const bf16_t* dOs = Or + (t & 1) * 32 * VP;
      const float* Ss = Sr + (t & 1) * 96;
      f32x16_t ss, sd;
      zero16(ss);
      zero16(sd);
#pragma unroll
      for (int ks = 0; ks < 6; ++ks) {
        ss = mfma(*reinterpret_cast<const bf16x8_t*>(Qs + r * VP + ks * 16 + 8 * hh), kf[ks], ss);
        sd = mfma(*reinterpret_cast<const bf16x8_t*>(dOs + r * VP + ks * 16 + 8 * hh), vf[ks], sd);
      }
      const bool band = t + 1 >= tj && t <= tj + 1;              // wave-uniform
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const float4 mx4 = *reinterpret_cast<const float4*>(Ss + 8 * g + 4 * hh);
        const float4 rd4 = *reinterpret_cast<const float4*>(Ss + 32 + 8 * g + 4 * hh);
        const float4 ds4 = *reinterpret_cast<const float4*>(Ss + 64 + 8 * g + 4 * hh);
        const float mxs[4] = {mx4.x, mx4.y, mx4.z, mx4.w}, rds[4] = {rd4.x, rd4.y, rd4.z, rd4.w}, dss[4] = {ds4.x, ds4.y, ds4.z, ds4.w};
#pragma unroll
        for (int e2 = 0; e2 < 4; ++e2) {
          const int i = 32 * t + 8 * g + 4 * hh + e2;
          float sc = ss[4 * g + e2], dp = sd[4 * g + e2];
          if (band) {
            const int rel = j - i + WIN;
            if ((unsigned)rel <= 2u * WIN && i < T) {
              const float* rec = wsq + (bhT + i) * WSQ;
              sc += rec[1 + rel];
              dp += rec[1 + NW + rel];
            }
          }
          const float p = __expf(mask_scale(sc, i, j, T, len, inv_sqrt) - mxs[e2]) * rds[e2];
          float pd = p;
          if (drop_thresh) {
            const bool keep = drop_keep(drop_seed, (uint32_t)((b * H + h) * T + i), j, drop_thresh);
            dp = keep ? dp * drop_scale : 0.f;
            pd = keep ? pd * drop_scale : 0.f;
          }
          if (j >= T) dp = 0.f;
          float ds = p * (dp - dss[e2]) * inv_sqrt;
          if (j >= T || j >= len || i >= len || i >= T) ds = 0.f;            // masked_fill blocks the gradient
          if (j >= T || i >= len || i >= T) pd = 0.f;                        // padded queries carry no upstream gradient
          ss[4 * g + e2] = ds;
          sd[4 * g + e2] = pd;
        }
      }
      acc_operand(ak, ss, Qs, ln);                               // bf16 operands, as the saved-P path's workspace held them
      acc_operand(av, sd, dOs, ln);
    }
    if (t + 1 < nqt) {
      GT_TILE_STORE(Qr + ((t + 1) & 1) * 32 * VP, qr)
      GT_TILE_STORE(Or + ((t + 1) & 1) * 32 * VP, dr)
      if (tid < 96) Sr[((t + 1) & 1) * 96 + tid] = sr;
    }
    __syncthreads();
  }
  if (active && j < T && rows.owns(j)) {
    store_row96(dk + rows.rw(j) * lddk + h * D, ak, hh);
    store_row96(dv + rows.rw(j) * lddk + h * D, av, hh);
  }
}

#undef GT_TILE_LOAD
#undef GT_TILE_STORE

}  // namespace

// The shapes the key-tiled kernels take, in both directions: past the last T at which the generic backward's LDS holds an
// utterance-head, up to the token limit of gt_mas_long_f32 (gt_attn_route).
extern "C" int gt_attn_long_shape(int T, int Dh, int win) { return gt_attn_route(T, Dh, win) == GT_ATTN_LONG_P; }

// The three forwards differ in what pass 2 leaves behind: P (LONG_P), nothing (LONG_NOP), the row statistics (LONG_STATS).
int gt_attn_fwd_long_impl(const gt_attn_call& c, gt_attn_path path)
{
  const dim3 grid((c.T + 127) / 128, c.H, c.B);
  if (path == GT_ATTN_LONG_STATS) {
    hipLaunchKernelGGL(gt_attn_long_fwd_stats_kernel, grid, dim3(256), 0, c.stream,
                       c.q, c.k, c.v, c.ld, c.Ek, c.Ev, c.lens, c.out, c.ldo, c.stats, c.T, c.Tp, c.row0, c.H, c.th, c.sd, c.sc, c.seed_dev);
    return gt_launch_status("gt_attn_fwd_long_stats_impl");
  }
  hipLaunchKernelGGL(path == GT_ATTN_LONG_P ? gt_attn_long_fwd_kernel<true> : gt_attn_long_fwd_kernel<false>, grid, dim3(256), 0, c.stream,
                     c.q, c.k, c.v, c.ld, c.Ek, c.Ev, c.lens, c.out, c.ldo, c.P, c.T, c.Tp, c.row0, c.H, c.th, c.sd, c.sc, c.seed_dev);
  return gt_launch_status(__func__);
}

size_t gt_attn_long_stats_ws_bytes(int B, int T, int H) { return (size_t)B * H * T * WSQ * sizeof(float); }

int gt_attn_bwd_long_impl(const gt_attn_call& c, gt_attn_path path)
{
  const dim3 grid((c.T + 127) / 128, c.H, c.B);
  if (path == GT_ATTN_LONG_STATS) {
    if (const int rc = gt_allow_lds<&gt_attn_long_bwd_q_stats_kernel>((int)LDS_BWD_QS)) return rc;
    float* wsq = static_cast<float*>(c.ws);
    hipLaunchKernelGGL(gt_attn_long_bwd_q_stats_kernel, grid, dim3(256), LDS_BWD_QS, c.stream,
                       c.q, c.k, c.v, c.ld, c.Ek, c.Ev, c.lens, c.dout, c.lddo, c.stats, wsq, c.dq, c.lddq, c.dEk, c.dEv,
                       c.T, c.Tp, c.row0, c.H, c.th, c.sd, c.sc, c.seed_dev);
    hipLaunchKernelGGL(gt_attn_long_bwd_kv_stats_kernel, grid, dim3(256), 0, c.stream,
                       c.q, c.k, c.v, c.ld, c.lens, c.dout, c.lddo, c.stats, wsq, c.dk, c.dv, c.lddq, c.T, c.Tp, c.row0, c.H,
                       c.th, c.sd, c.sc, c.seed_dev);
    return gt_launch_status("gt_attn_bwd_long_stats_impl");
  }
  const gt_attn_bwd_ws w(c);                                     // the MFMA family's workspace format
  if (const int rc = gt_allow_lds<&gt_attn_long_bwd_q_kernel>((int)LDS_BWD_Q)) return rc;
  hipLaunchKernelGGL(gt_attn_long_bwd_q_kernel, grid, dim3(256), LDS_BWD_Q, c.stream,
                     c.q, c.k, c.v, c.ld, c.Ek, c.Ev, c.lens, c.dout, c.lddo, c.P, w.dST, w.PdT, w.TI, c.dq, c.lddq, c.dEk, c.dEv,
                     c.T, c.Tp, c.row0, c.H, c.th, c.sd, c.sc, c.seed_dev);
  hipLaunchKernelGGL(gt_attn_long_bwd_kv_kernel, grid, dim3(256), 0, c.stream,
                     c.q, c.ld, c.dout, c.lddo, w.dST, w.PdT, w.TI, c.dk, c.dv, c.lddq, c.T, c.Tp, c.row0, c.H);
  return gt_launch_status(__func__);
}
