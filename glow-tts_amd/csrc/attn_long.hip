// Relative-position attention for long texts (505 < T <= GT_ATTN_LONG_MAX_T; D = 96, window 4) on bf16 MFMA for gfx950.
//
// Same contract, lane mapping and arithmetic as the <12> kernels of attn_mfma.hip (read that file first): one score tile
// live at a time, two walks over the key tiles.  What changes: the tile count is a runtime loop and NO full-length operand
// sits in LDS or in registers.
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

// one [32][VP] tile of rows 32t .. 32t+31 (rows >= T zero): thread tid holds uint4 x = tid + 256u, u < 2
#define GT_TILE_LOAD(regs, src, lds_, t)                                                       \
  _Pragma("unroll") for (int u_ = 0; u_ < 2; ++u_) {                                           \
    const int x_ = tid + 256 * u_;                                                             \
    const int row_ = x_ / (D / 8), c8_ = x_ - row_ * (D / 8);                                  \
    uint4 val_ = make_uint4(0, 0, 0, 0);                                                       \
    if (x_ < TILE_U4 && 32 * (t) + row_ < T)                                                   \
      val_ = *reinterpret_cast<const uint4*>((src) + RW(32 * (t) + row_) * (lds_) + h * D + c8_ * 8); \
    (regs)[u_] = val_;                                                                         \
  }
#define GT_TILE_STORE(slot, regs)                                                              \
  _Pragma("unroll") for (int u_ = 0; u_ < 2; ++u_) {                                           \
    const int x_ = tid + 256 * u_;                                                             \
    const int row_ = x_ / (D / 8), c8_ = x_ - row_ * (D / 8);                                  \
    if (x_ < TILE_U4) *reinterpret_cast<uint4*>((slot) + row_ * VP + c8_ * 8) = (regs)[u_];    \
  }

// =========================================================================================
// Forward: one workgroup per (utterance, head, 128 queries), a wave owns 32 queries.
// STORE_P = false (gt_attn_fwd with P == NULL: a forward nobody differentiates, synthesis): pass 2 leaves out its P stores and
// nothing else, so `out` is the same bit for bit.
// STATS (gt_attn_long_fwd_stats_kernel, gt_attn_fwd_stats: the training forward whose backward recomputes P): no P either; after
// pass 1 every query row i < T, padded ones included, stores the pair it holds, (mx, rden) = (maximum of the masked, scaled scores,
// 1 / denominator), to Pout = stats[B, H, T, 2].  With them P[i, j] = __expf(s - mx) * rden is pass 2's expression on the same values.
template <bool STORE_P>
__global__ __launch_bounds__(256, 2) void gt_attn_long_fwd_kernel(
    const bf16_t* __restrict__ q, const bf16_t* __restrict__ k, const bf16_t* __restrict__ v, int ld,
    const float* __restrict__ Ek, const float* __restrict__ Ev, const int32_t* __restrict__ lens,
    bf16_t* __restrict__ out, int ldo, float* __restrict__ Pout,
    int T, int Tp, const int32_t* row0, int H, uint32_t drop_thresh, uint32_t drop_seed, float drop_scale, const uint32_t* __restrict__ seed_dev)
{
  constexpr bool STATS = false;
#include "attn_long_fwd_body.inc"
}

__global__ __launch_bounds__(256, 2) void gt_attn_long_fwd_stats_kernel(
    const bf16_t* __restrict__ q, const bf16_t* __restrict__ k, const bf16_t* __restrict__ v, int ld,
    const float* __restrict__ Ek, const float* __restrict__ Ev, const int32_t* __restrict__ lens,
    bf16_t* __restrict__ out, int ldo, float* __restrict__ Pout,
    int T, int Tp, const int32_t* row0, int H, uint32_t drop_thresh, uint32_t drop_seed, float drop_scale, const uint32_t* __restrict__ seed_dev)
{
  constexpr bool STORE_P = false, STATS = true;
#include "attn_long_fwd_body.inc"
}

// =========================================================================================
// Backward pass 1 (dS, P', dQ, dEk, dEv): the one-tile recompute form of gt_attn_bwd_q_mfma_kernel<12, 4, true>, 4 waves x
// 32 queries.  Pass A (Dsum) reads V rows and P only; pass B stages K per tile for the transposing reads of dQ^T.  The
// Q / dO tiles of the dEk / dEv contraction share one per-wave [32][VP] area, loaded one after the other at the end.
constexpr int LWBN = 32 * 16 + 2 * 16 * BTP + 32 * VP;         // per wave: dSB[32][16] | dSBT[16][BTP] | PdBT[16][BTP] | QD[32][VP]
constexpr size_t LDS_BWD_Q = (size_t)2 * 32 * VP * 2 + 32 * KP * 2 + D * 16 * 2 + 2 * NW * D * 4 + 4 * 32 * NW * 4 + (size_t)4 * LWBN * 2;

__global__ __launch_bounds__(256, 2) void gt_attn_long_bwd_q_kernel(
    const bf16_t* __restrict__ q, const bf16_t* __restrict__ k, const bf16_t* __restrict__ v, int ld,
    const float* __restrict__ Ek, const float* __restrict__ Ev, const int32_t* __restrict__ lens,
    const bf16_t* __restrict__ dout, int lddo, const float* __restrict__ P,
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
  bf16_t* WB  = reinterpret_cast<bf16_t*>(DOE + 4 * 32 * NW);    // [4][LWBN]

  const int b = blockIdx.z, h = blockIdx.y;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int r = lane & 31, hh = lane >> 5;
  const int len = lens[b];
  const size_t rbase = (size_t)gt_row_base(row0, b, Tp) + HALO;
  const int nv1 = gt_row_count(row0, b, Tp) - HALO - 1;          // see gt_attn_bwd_q_mfma_kernel
  auto RW = [&](int t) { return rbase + (size_t)(t < nv1 ? t : nv1); };

  for (int i = tid; i < 32 * D; i += 256) { const int rr = i / D, c = i - rr * D; Evs[rr * KP + c] = rr < NW ? f2bf(Ev[rr * D + c]) : (bf16_t)0; }
  for (int i = tid; i < D * 16; i += 256) { const int d = i >> 4, rr = i & 15; EkT[i] = rr < NW ? f2bf(Ek[rr * D + d]) : (bf16_t)0; }
  for (int i = tid; i < 2 * NW * D; i += 256) Acc[i] = 0.f;
  for (int i = tid; i < 4 * (32 * 16 + 2 * 16 * BTP); i += 256) {             // band tables start at zero
    const int ww = i / (32 * 16 + 2 * 16 * BTP), o = i - ww * (32 * 16 + 2 * 16 * BTP);
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
  bf16_t* dSB = WB + w * LWBN;
  bf16_t* dSBT = dSB + 32 * 16;
  bf16_t* PdBT = dSBT + 16 * BTP;
  bf16_t* QD = PdBT + 16 * BTP;
  const int li = lane & 15, qd = li >> 2, pp = li & 3, colhalf = ((lane >> 4) & 1) * 16;

  bf16x8_t dof[6];
#pragma unroll
  for (int ks = 0; ks < 6; ++ks)
    dof[ks] = *reinterpret_cast<const bf16x8_t*>(dout + RW(ic) * lddo + h * D + ks * 16 + 8 * hh);
  if (active) {
    f32x16_t acc;
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[e] = 0.f;
#pragma unroll
    for (int ks = 0; ks < 6; ++ks) {
      const bf16x8_t af = *reinterpret_cast<const bf16x8_t*>(Evs + r * KP + ks * 16 + 8 * hh);
      acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af, dof[ks], acc, 0, 0, 0);
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) doe[r * NW + e + 4 * hh] = acc[e];
    if (hh == 0) doe[r * NW + 8] = acc[4];
  }
  __builtin_amdgcn_wave_barrier();

  const float inv_sqrt = rsqrtf((float)D);
  const float* prow = P + (((size_t)b * H + h) * T + ic) * T;
  const uint32_t drow = (uint32_t)((b * H + h) * T + i);
  const bool vec = (T & 3) == 0;
  bf16_t* dst_base = dST + ((size_t)b * H + h) * T * TI;
  bf16_t* pdt_base = PdT + ((size_t)b * H + h) * T * TI;

  // V fragments of key tile t: lane (key r of the tile, k-half hh); rows >= T are zero
  auto load_v = [&](int t, bf16x8_t* vf) {
    const int j = 32 * t + r;
    if (j < T) {
#pragma unroll
      for (int ks = 0; ks < 6; ++ks) vf[ks] = *reinterpret_cast<const bf16x8_t*>(v + RW(j) * ld + h * D + ks * 16 + 8 * hh);
    } else {
      const uint4 z = make_uint4(0, 0, 0, 0);
#pragma unroll
      for (int ks = 0; ks < 6; ++ks) vf[ks] = __builtin_bit_cast(bf16x8_t, z);
    }
  };
  auto dp_tile = [&](const bf16x8_t* vf, f32x16_t& st) {
#pragma unroll
    for (int e = 0; e < 16; ++e) st[e] = 0.f;
#pragma unroll
    for (int ks = 0; ks < 6; ++ks) st = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vf[ks], dof[ks], st, 0, 0, 0);
  };
  auto load_p4 = [&](int j0, float* p4) {
    p4[0] = p4[1] = p4[2] = p4[3] = 0.f;
    if (vec && j0 + 3 < T) { const float4 pv = *reinterpret_cast<const float4*>(prow + j0); p4[0] = pv.x; p4[1] = pv.y; p4[2] = pv.z; p4[3] = pv.w; }
    else {
#pragma unroll
      for (int e2 = 0; e2 < 4; ++e2) if (j0 + e2 < T) p4[e2] = prow[j0 + e2];
    }
  };
  auto dp_elem = [&](float dp, int j) {
    const int rel = j - i + WIN;
    if ((unsigned)rel <= 2u * WIN) dp += doe[r * NW + rel];
    if (drop_thresh) dp = drop_keep(drop_seed, drow, j, drop_thresh) ? dp * drop_scale : 0.f;
    return j >= T ? 0.f : dp;
  };

  // ---- pass A (no LDS operand, no barrier): Dsum = sum_j dP P
  float dsum = 0.f;
  bf16x8_t vf[6], vn[6];
  if (active) {
    load_v(0, vf);
#pragma unroll 1
    for (int t = 0; t < nt; ++t) {
      if (t + 1 < nt) load_v(t + 1, vn);
      f32x16_t st;
      dp_tile(vf, st);
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int j0 = 32 * t + 8 * g + 4 * hh;
        float p4[4];
        load_p4(j0, p4);
#pragma unroll
        for (int e2 = 0; e2 < 4; ++e2) dsum += dp_elem(st[4 * g + e2], j0 + e2) * p4[e2];
      }
#pragma unroll
      for (int ks = 0; ks < 6; ++ks) vf[ks] = vn[ks];
    }
    dsum += __shfl_xor(dsum, 32);
  }

  // ---- pass B: recompute dPd^T per tile, dS^T, store dS^T / P'^T, dQ^T += K^T dS^T; K tile t in ring slot t & 1
  f32x16_t o[3];
#pragma unroll
  for (int dt = 0; dt < 3; ++dt) {
#pragma unroll
    for (int e = 0; e < 16; ++e) o[dt][e] = 0.f;
  }
  if (active) load_v(0, vf);
#pragma unroll 1
  for (int t = 0; t < nt; ++t) {
    if (t + 1 < nt) {
      GT_TILE_LOAD(kr, k, ld, t + 1)
      if (active) load_v(t + 1, vn);
    }
    if (active) {
      const bf16_t* Ks = Kr + (t & 1) * 32 * VP;
      f32x16_t st;
      dp_tile(vf, st);
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int j0 = 32 * t + 8 * g + 4 * hh;
        float p4[4];
        load_p4(j0, p4);
#pragma unroll
        for (int e2 = 0; e2 < 4; ++e2) {
          const int j = j0 + e2;
          float ds = p4[e2] * (dp_elem(st[4 * g + e2], j) - dsum) * inv_sqrt;
          float pd = p4[e2];
          if (drop_thresh) pd = drop_keep(drop_seed, drow, j, drop_thresh) ? pd * drop_scale : 0.f;
          if (j >= T || j >= len || i >= len || i >= T) ds = 0.f;          // masked_fill blocks the gradient
          if (i >= len || i >= T) pd = 0.f;                                // padded queries carry no upstream gradient
          st[4 * g + e2] = ds;
          if (j < T) {
            dst_base[(size_t)j * TI + i] = f2bf(ds);
            pdt_base[(size_t)j * TI + i] = f2bf(pd);
            const int rel = j - i + WIN;
            if ((unsigned)rel <= 2u * WIN) { const bf16_t db = f2bf(ds); dSB[r * 16 + rel] = db; dSBT[rel * BTP + r] = db; PdBT[rel * BTP + r] = f2bf(pd); }
          }
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
          const bf16_t* ka = Ks + (16 * s2 + 4 * hh + qd) * VP + 32 * dt + colhalf + 4 * pp;
          const bf16x8_t af = tr_frag8(ka, ka + 8 * VP);
          o[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af, pf, o[dt], 0, 0, 0);
        }
      }
#pragma unroll
      for (int ks = 0; ks < 6; ++ks) vf[ks] = vn[ks];
    }
    if (t + 1 < nt) { GT_TILE_STORE(Kr + ((t + 1) & 1) * 32 * VP, kr) }
    __syncthreads();
  }

  if (active) {
    {
      const bf16x8_t bfp = *reinterpret_cast<const bf16x8_t*>(dSB + r * 16 + 8 * hh);
#pragma unroll
      for (int dt = 0; dt < 3; ++dt) {
        const bf16x8_t af = *reinterpret_cast<const bf16x8_t*>(EkT + (32 * dt + r) * 16 + 8 * hh);
        o[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af, bfp, o[dt], 0, 0, 0);
      }
    }
    if (i < T && i <= nv1) {
#pragma unroll
      for (int dt = 0; dt < 3; ++dt)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int d = 32 * dt + 8 * g + 4 * hh;
          *reinterpret_cast<uint2*>(dq + (rbase + i) * lddq + h * D + d) =
              make_uint2(pack2bf(o[dt][4 * g], o[dt][4 * g + 1]), pack2bf(o[dt][4 * g + 2], o[dt][4 * g + 3]));
        }
    }
    // dEk[r'][d] += sum_i dSBT[r'][i] Q[i][d];  dEv[r'][d] += sum_i PdBT[r'][i] dO[i][d]   (K = 32 queries, one MFMA chain)
#pragma unroll 1
    for (int which = 0; which < 2; ++which) {
      const bf16_t* At = which ? PdBT : dSBT;
      const bf16_t* src = which ? dout : q;
      const int lds_ = which ? lddo : ld;
      __builtin_amdgcn_wave_barrier();                             // the previous contraction has read QD
      for (int c = lane; c < 32 * (D / 8); c += 64) {              // this wave's Q (dO) rows, rows >= T zero
        const int rr = c / (D / 8), c8 = c - rr * (D / 8);
        uint4 x = make_uint4(0, 0, 0, 0);
        if (i0 + rr < T) x = *reinterpret_cast<const uint4*>(src + RW(i0 + rr) * lds_ + h * D + c8 * 8);
        *reinterpret_cast<uint4*>(QD + rr * VP + c8 * 8) = x;
      }
      __builtin_amdgcn_wave_barrier();
#pragma unroll
      for (int dt = 0; dt < 3; ++dt) {
        f32x16_t acc;
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[e] = 0.f;
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
          bf16x8_t af = *reinterpret_cast<const bf16x8_t*>(At + (r & 15) * BTP + 16 * ks + 8 * hh);
          if (r >= 16) { const uint4 z = make_uint4(0, 0, 0, 0); af = __builtin_bit_cast(bf16x8_t, z); }
          const bf16_t* ba = QD + (16 * ks + 8 * hh + qd) * VP + 32 * dt + colhalf + 4 * pp;
          const bf16x8_t bf_ = tr_frag8(ba, ba + 4 * VP);
          acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af, bf_, acc, 0, 0, 0);
        }
        float* dstA = Acc + which * NW * D;
        const int d = 32 * dt + r;                                   // D layout: column = d (lane&31), row r' = (e&3)+8(e>>2)+4hh
#pragma unroll
        for (int e = 0; e < 4; ++e) atomicAdd(dstA + (e + 4 * hh) * D + d, acc[e]);
        if (hh == 0) atomicAdd(dstA + 8 * D + d, acc[4]);
      }
    }
  }
  __syncthreads();
  for (int x = tid; x < NW * D; x += 256) {
    if (Acc[x] != 0.f) atomicAdd(dEk + x, Acc[x]);
    if (Acc[NW * D + x] != 0.f) atomicAdd(dEv + x, Acc[NW * D + x]);
  }
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
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int r = lane & 31, hh = lane >> 5;
  const size_t rbase = (size_t)gt_row_base(row0, b, Tp) + HALO;
  const int nv1 = gt_row_count(row0, b, Tp) - HALO - 1;          // see gt_attn_bwd_kv_mfma_kernel
  auto RW = [&](int t) { return rbase + (size_t)(t < nv1 ? t : nv1); };

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
  const int li = lane & 15, qd = li >> 2, pp = li & 3, colhalf = ((lane >> 4) & 1) * 16;
  const bf16_t* dsr = dST + (((size_t)b * H + h) * T + jc) * TI;
  const bf16_t* pdr = PdT + (((size_t)b * H + h) * T + jc) * TI;
  f32x16_t ak[3], av[3];
#pragma unroll
  for (int dt = 0; dt < 3; ++dt) {
#pragma unroll
    for (int e = 0; e < 16; ++e) { ak[dt][e] = 0.f; av[dt][e] = 0.f; }
  }
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
      const bf16_t* Qs = Qr + (t & 1) * 32 * VP;
      const bf16_t* dOs = Or + (t & 1) * 32 * VP;
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
#pragma unroll
        for (int dt = 0; dt < 3; ++dt) {
          const bf16_t* qa = Qs + (16 * ks + 8 * hh + qd) * VP + 32 * dt + colhalf + 4 * pp;
          const bf16_t* da = dOs + (16 * ks + 8 * hh + qd) * VP + 32 * dt + colhalf + 4 * pp;
          ak[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(tr_frag8(qa, qa + 4 * VP), bds[ks], ak[dt], 0, 0, 0);
          av[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(tr_frag8(da, da + 4 * VP), bpd[ks], av[dt], 0, 0, 0);
        }
      }
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) { bds[ks] = nds[ks]; bpd[ks] = npd[ks]; }
    }
    if (t + 1 < nqt) {
      GT_TILE_STORE(Qr + ((t + 1) & 1) * 32 * VP, qr)
      GT_TILE_STORE(Or + ((t + 1) & 1) * 32 * VP, dr)
    }
    __syncthreads();
  }
  if (active && j < T && j <= nv1) {
#pragma unroll
    for (int dt = 0; dt < 3; ++dt)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int d = 32 * dt + 8 * g + 4 * hh;
        *reinterpret_cast<uint2*>(dk + RW(j) * lddk + h * D + d) =
            make_uint2(pack2bf(ak[dt][4 * g], ak[dt][4 * g + 1]), pack2bf(ak[dt][4 * g + 2], ak[dt][4 * g + 3]));
        *reinterpret_cast<uint2*>(dv + RW(j) * lddk + h * D + d) =
            make_uint2(pack2bf(av[dt][4 * g], av[dt][4 * g + 1]), pack2bf(av[dt][4 * g + 2], av[dt][4 * g + 3]));
      }
  }
}

// =========================================================================================
// P-free backward (gt_attn_bwd_stats): nothing of size T^2 is read or written.  Both kernels recompute P tile by tile from q, k, Ek
// and the forward's row statistics (mx, rden): P[i, j] = __expf(s[i, j] - mx_i) * rden_i, the forward's own expression.
// Between them goes one record of WSQ floats per query row i < T of every (b, h):
//   [0] Dsum_i   [1 .. 9] q_i . Ek[r]   [10 .. 18] dO_i . Ev[r]   [19] zero
// (the qe / doe band tables of the query side, so both kernels add the same bits on the band).
constexpr int WSQ = 20;

// Query side: gt_attn_long_bwd_q_kernel with load_p4 replaced by the forward's `scores` (K fragment as A, Q fragment as B, band,
// scale, mask) and the forward's P expression, so P, Dsum, the bf16 dS operand and the dQ chain are the saved-P kernel's bit for
// bit.  The K fragments of the score MFMAs are 16-byte row reads of the K ring that pass B stages anyway; pass A stages the same
// ring (one barrier per tile there too) instead of holding a second set of K fragments and their prefetch copy in registers: that
// keeps the kernel at two workgroups per CU.  Tile t of pass A sits in slot t & 1; its last step stages tile 0 again, so tile t
// of pass B sits in slot (nt + t) & 1.  The bf16 Ek rows of the qe table are read out of EkT (the same f2bf values as the
// forward's Eks image), so no second Ek image is staged.
constexpr size_t LDS_BWD_QS = LDS_BWD_Q + (size_t)4 * 32 * NW * 4;

__global__ __launch_bounds__(256, 2) void gt_attn_long_bwd_q_stats_kernel(
    const bf16_t* __restrict__ q, const bf16_t* __restrict__ k, const bf16_t* __restrict__ v, int ld,
    const float* __restrict__ Ek, const float* __restrict__ Ev, const int32_t* __restrict__ lens,
    const bf16_t* __restrict__ dout, int lddo, const float* __restrict__ stats, float* __restrict__ wsq,
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
  float*  QE  = DOE + 4 * 32 * NW;                               // [4][32][NW]
  bf16_t* WB  = reinterpret_cast<bf16_t*>(QE + 4 * 32 * NW);     // [4][LWBN]

  const int b = blockIdx.z, h = blockIdx.y;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int r = lane & 31, hh = lane >> 5;
  const int len = lens[b];
  const size_t rbase = (size_t)gt_row_base(row0, b, Tp) + HALO;
  const int nv1 = gt_row_count(row0, b, Tp) - HALO - 1;          // see gt_attn_bwd_q_mfma_kernel
  auto RW = [&](int t) { return rbase + (size_t)(t < nv1 ? t : nv1); };

  for (int i = tid; i < 32 * D; i += 256) { const int rr = i / D, c = i - rr * D; Evs[rr * KP + c] = rr < NW ? f2bf(Ev[rr * D + c]) : (bf16_t)0; }
  for (int i = tid; i < D * 16; i += 256) { const int d = i >> 4, rr = i & 15; EkT[i] = rr < NW ? f2bf(Ek[rr * D + d]) : (bf16_t)0; }
  for (int i = tid; i < 2 * NW * D; i += 256) Acc[i] = 0.f;
  for (int i = tid; i < 4 * (32 * 16 + 2 * 16 * BTP); i += 256) {             // band tables start at zero
    const int ww = i / (32 * 16 + 2 * 16 * BTP), o = i - ww * (32 * 16 + 2 * 16 * BTP);
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
  float* qe = QE + w * 32 * NW;
  bf16_t* dSB = WB + w * LWBN;
  bf16_t* dSBT = dSB + 32 * 16;
  bf16_t* PdBT = dSBT + 16 * BTP;
  bf16_t* QD = PdBT + 16 * BTP;
  const int li = lane & 15, qd = li >> 2, pp = li & 3, colhalf = ((lane >> 4) & 1) * 16;
  const size_t bhT = ((size_t)b * H + h) * T;

  bf16x8_t dof[6];
#pragma unroll
  for (int ks = 0; ks < 6; ++ks)
    dof[ks] = *reinterpret_cast<const bf16x8_t*>(dout + RW(ic) * lddo + h * D + ks * 16 + 8 * hh);
  // This wave's Q rows sit in its QD strip (free until the dEk / dEv contractions at the end) and the Q fragment of an MFMA is a
  // 16-byte row read there: 24 registers fewer than holding them.  Rows >= T are zero; the forward read row T - 1 there, and in
  // both nothing computed for such a query is stored.
  for (int c = lane; c < 32 * (D / 8); c += 64) {
    const int rr = c / (D / 8), c8 = c - rr * (D / 8);
    uint4 x = make_uint4(0, 0, 0, 0);
    if (i0 + rr < T) x = *reinterpret_cast<const uint4*>(q + RW(i0 + rr) * ld + h * D + c8 * 8);
    *reinterpret_cast<uint4*>(QD + rr * VP + c8 * 8) = x;
  }
  __builtin_amdgcn_wave_barrier();
  auto qf = [&](int ks) { return *reinterpret_cast<const bf16x8_t*>(QD + r * VP + ks * 16 + 8 * hh); };
  if (active) {
    f32x16_t acc, acq;
#pragma unroll
    for (int e = 0; e < 16; ++e) { acc[e] = 0.f; acq[e] = 0.f; }
#pragma unroll
    for (int ks = 0; ks < 6; ++ks) {
      const bf16x8_t af = *reinterpret_cast<const bf16x8_t*>(Evs + r * KP + ks * 16 + 8 * hh);
      acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af, dof[ks], acc, 0, 0, 0);
      s16x8_t ek = {0, 0, 0, 0, 0, 0, 0, 0};                      // row r of bf16 Ek (rows >= 9 zero), out of its transposed image
      if (r < NW) {
#pragma unroll
        for (int x = 0; x < 8; ++x) ek[x] = (short)EkT[(ks * 16 + 8 * hh + x) * 16 + r];
      }
      acq = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8_t, ek), qf(ks), acq, 0, 0, 0);
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) { doe[r * NW + e + 4 * hh] = acc[e]; qe[r * NW + e + 4 * hh] = acq[e]; }
    if (hh == 0) { doe[r * NW + 8] = acc[4]; qe[r * NW + 8] = acq[4]; }
  }
  __builtin_amdgcn_wave_barrier();

  const float inv_sqrt = rsqrtf((float)D);
  const float mx = stats[(bhT + ic) * 2], rden = stats[(bhT + ic) * 2 + 1];
  const uint32_t drow = (uint32_t)((b * H + h) * T + i);

  // V fragments of key tile t: lane (key r of the tile, k-half hh); rows >= T are zero
  auto load_v = [&](int t, bf16x8_t* vf) {
    const int j = 32 * t + r;
    if (j < T) {
#pragma unroll
      for (int ks = 0; ks < 6; ++ks) vf[ks] = *reinterpret_cast<const bf16x8_t*>(v + RW(j) * ld + h * D + ks * 16 + 8 * hh);
    } else {
      const uint4 z = make_uint4(0, 0, 0, 0);
#pragma unroll
      for (int ks = 0; ks < 6; ++ks) vf[ks] = __builtin_bit_cast(bf16x8_t, z);
    }
  };
  auto dp_tile = [&](const bf16x8_t* vf, f32x16_t& st) {
#pragma unroll
    for (int e = 0; e < 16; ++e) st[e] = 0.f;
#pragma unroll
    for (int ks = 0; ks < 6; ++ks) st = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vf[ks], dof[ks], st, 0, 0, 0);
  };
  // P of one tile from the staged K tile Ks (rows >= T zero, as load_k of the forward leaves them): the forward's scores lambda,
  // then its P expression (element e <-> key 32t + (e&3) + 8(e>>2) + 4hh)
  auto p_tile = [&](int t, const bf16_t* Ks, f32x16_t& sp) {
#pragma unroll
    for (int e = 0; e < 16; ++e) sp[e] = 0.f;
#pragma unroll
    for (int ks = 0; ks < 6; ++ks) {
      const bf16x8_t kf = *reinterpret_cast<const bf16x8_t*>(Ks + r * VP + ks * 16 + 8 * hh);
      sp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf, qf(ks), sp, 0, 0, 0);
    }
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int j = 32 * t + (e & 3) + 8 * (e >> 2) + 4 * hh;
      float sc = sp[e];
      const int rel = j - i + WIN;
      if ((unsigned)rel <= 2u * WIN) sc += qe[r * NW + rel];
      sc *= inv_sqrt;
      if (j >= T) sc = -3.0e38f;                                 // not a key at all
      else if (j >= len || i >= len) sc = -1e4f;
      sp[e] = __expf(sc - mx) * rden;
    }
  };
  auto dp_elem = [&](float dp, int j) {
    const int rel = j - i + WIN;
    if ((unsigned)rel <= 2u * WIN) dp += doe[r * NW + rel];
    if (drop_thresh) dp = drop_keep(drop_seed, drow, j, drop_thresh) ? dp * drop_scale : 0.f;
    return j >= T ? 0.f : dp;
  };

  // ---- pass A: Dsum = sum_j dP P; K tile t in ring slot t & 1, the last step stages tile 0 for pass B
  float dsum = 0.f;
  bf16x8_t vf[6], vn[6];
  if (active) load_v(0, vf);
#pragma unroll 1
  for (int t = 0; t < nt; ++t) {
    const int tn = t + 1 < nt ? t + 1 : 0;
    GT_TILE_LOAD(kr, k, ld, tn)
    if (active) {
      load_v(tn, vn);
      f32x16_t st, sp;
      p_tile(t, Kr + (t & 1) * 32 * VP, sp);
      dp_tile(vf, st);
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int j0 = 32 * t + 8 * g + 4 * hh;
#pragma unroll
        for (int e2 = 0; e2 < 4; ++e2) dsum += dp_elem(st[4 * g + e2], j0 + e2) * sp[4 * g + e2];
      }
#pragma unroll
      for (int ks = 0; ks < 6; ++ks) vf[ks] = vn[ks];
    }
    GT_TILE_STORE(Kr + ((t + 1) & 1) * 32 * VP, kr)
    __syncthreads();
  }
  if (active) {
    dsum += __shfl_xor(dsum, 32);
    if (i < T) {                                                 // what the key side needs of this query row
      float* rec = wsq + (bhT + i) * WSQ;
      const float* tab = hh ? doe : qe;
      if (hh == 0) rec[0] = dsum; else rec[WSQ - 1] = 0.f;
#pragma unroll
      for (int x = 0; x < NW; ++x) rec[1 + NW * hh + x] = tab[r * NW + x];
    }
  }

  // ---- pass B: recompute P and dPd^T per tile, dS^T, dQ^T += K^T dS^T; K tile t in ring slot (nt + t) & 1
  f32x16_t o[3];
#pragma unroll
  for (int dt = 0; dt < 3; ++dt) {
#pragma unroll
    for (int e = 0; e < 16; ++e) o[dt][e] = 0.f;
  }
#pragma unroll 1
  for (int t = 0; t < nt; ++t) {
    if (t + 1 < nt) {
      GT_TILE_LOAD(kr, k, ld, t + 1)
      if (active) load_v(t + 1, vn);
    }
    if (active) {
      const bf16_t* Ks = Kr + ((nt + t) & 1) * 32 * VP;
      f32x16_t st, sp;
      p_tile(t, Ks, sp);
      dp_tile(vf, st);
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int j0 = 32 * t + 8 * g + 4 * hh;
#pragma unroll
        for (int e2 = 0; e2 < 4; ++e2) {
          const int j = j0 + e2;
          const float p = sp[4 * g + e2];
          float ds = p * (dp_elem(st[4 * g + e2], j) - dsum) * inv_sqrt;
          float pd = p;
          if (drop_thresh) pd = drop_keep(drop_seed, drow, j, drop_thresh) ? pd * drop_scale : 0.f;
          if (j >= T || j >= len || i >= len || i >= T) ds = 0.f;          // masked_fill blocks the gradient
          if (i >= len || i >= T) pd = 0.f;                                // padded queries carry no upstream gradient
          st[4 * g + e2] = ds;
          if (j < T) {
            const int rel = j - i + WIN;
            if ((unsigned)rel <= 2u * WIN) { const bf16_t db = f2bf(ds); dSB[r * 16 + rel] = db; dSBT[rel * BTP + r] = db; PdBT[rel * BTP + r] = f2bf(pd); }
          }
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
          const bf16_t* ka = Ks + (16 * s2 + 4 * hh + qd) * VP + 32 * dt + colhalf + 4 * pp;
          const bf16x8_t af = tr_frag8(ka, ka + 8 * VP);
          o[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af, pf, o[dt], 0, 0, 0);
        }
      }
#pragma unroll
      for (int ks = 0; ks < 6; ++ks) vf[ks] = vn[ks];
    }
    if (t + 1 < nt) { GT_TILE_STORE(Kr + ((nt + t + 1) & 1) * 32 * VP, kr) }
    __syncthreads();
  }

  if (active) {
    {
      const bf16x8_t bfp = *reinterpret_cast<const bf16x8_t*>(dSB + r * 16 + 8 * hh);
#pragma unroll
      for (int dt = 0; dt < 3; ++dt) {
        const bf16x8_t af = *reinterpret_cast<const bf16x8_t*>(EkT + (32 * dt + r) * 16 + 8 * hh);
        o[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af, bfp, o[dt], 0, 0, 0);
      }
    }
    if (i < T && i <= nv1) {
#pragma unroll
      for (int dt = 0; dt < 3; ++dt)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int d = 32 * dt + 8 * g + 4 * hh;
          *reinterpret_cast<uint2*>(dq + (rbase + i) * lddq + h * D + d) =
              make_uint2(pack2bf(o[dt][4 * g], o[dt][4 * g + 1]), pack2bf(o[dt][4 * g + 2], o[dt][4 * g + 3]));
        }
    }
    // dEk[r'][d] += sum_i dSBT[r'][i] Q[i][d];  dEv[r'][d] += sum_i PdBT[r'][i] dO[i][d]   (K = 32 queries, one MFMA chain)
#pragma unroll 1
    for (int which = 0; which < 2; ++which) {
      const bf16_t* At = which ? PdBT : dSBT;
      const bf16_t* src = which ? dout : q;
      const int lds_ = which ? lddo : ld;
      __builtin_amdgcn_wave_barrier();                             // the previous contraction has read QD
      for (int c = lane; c < 32 * (D / 8); c += 64) {              // this wave's Q (dO) rows, rows >= T zero
        const int rr = c / (D / 8), c8 = c - rr * (D / 8);
        uint4 x = make_uint4(0, 0, 0, 0);
        if (i0 + rr < T) x = *reinterpret_cast<const uint4*>(src + RW(i0 + rr) * lds_ + h * D + c8 * 8);
        *reinterpret_cast<uint4*>(QD + rr * VP + c8 * 8) = x;
      }
      __builtin_amdgcn_wave_barrier();
#pragma unroll
      for (int dt = 0; dt < 3; ++dt) {
        f32x16_t acc;
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[e] = 0.f;
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
          bf16x8_t af = *reinterpret_cast<const bf16x8_t*>(At + (r & 15) * BTP + 16 * ks + 8 * hh);
          if (r >= 16) { const uint4 z = make_uint4(0, 0, 0, 0); af = __builtin_bit_cast(bf16x8_t, z); }
          const bf16_t* ba = QD + (16 * ks + 8 * hh + qd) * VP + 32 * dt + colhalf + 4 * pp;
          const bf16x8_t bf_ = tr_frag8(ba, ba + 4 * VP);
          acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af, bf_, acc, 0, 0, 0);
        }
        float* dstA = Acc + which * NW * D;
        const int d = 32 * dt + r;                                   // D layout: column = d (lane&31), row r' = (e&3)+8(e>>2)+4hh
#pragma unroll
        for (int e = 0; e < 4; ++e) atomicAdd(dstA + (e + 4 * hh) * D + d, acc[e]);
        if (hh == 0) atomicAdd(dstA + 8 * D + d, acc[4]);
      }
    }
  }
  __syncthreads();
  for (int x = tid; x < NW * D; x += 256) {
    if (Acc[x] != 0.f) atomicAdd(dEk + x, Acc[x]);
    if (Acc[NW * D + x] != 0.f) atomicAdd(dEv + x, Acc[NW * D + x]);
  }
}

// Key side: one workgroup per (utterance, head, 128 keys), a wave owns 32 keys, keeps their K and V fragments in registers (lane =
// key r, k-half hh, as load_k / load_v form them) and walks the 32-query tiles below lens[b] (tiles wholly past it add nothing).
// Per tile:  S = Q K^T and dP' = dO V^T with the tile's Q / dO rows (16-byte row reads of the ring) as the A operand and the
// wave's K / V fragments as B, so a lane holds key j = j0 + r and accumulator element e holds query
//     i = 32t + (e&3) + 8(e>>2) + 4hh;
// the band terms come from the query side's records (only the tiles next to the wave's keys touch the band), then P, the keep
// bit, dS and P' as on the query side, per-query mx / rden / Dsum out of an LDS ring staged one tile ahead.
// The accumulators are then the B operand of dK^T = Q^T dS and dV^T = dO^T P' up to a permutation of the k index: MFMA s2 takes
// pack8(st + 8 s2), i.e. k index 8hh + kk <-> query 32t + 16 s2 + 4hh + (kk&3) + 8(kk>>2), and the A fragment
// tr_frag8(a + (16 s2 + 4hh + qd) VP ..., ... + 8 VP) reads the ring's rows in that same order (the forward's P'V product and the
// query side's dQ product, with queries where they have keys).
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
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int r = lane & 31, hh = lane >> 5;
  const int len = lens[b];
  const size_t rbase = (size_t)gt_row_base(row0, b, Tp) + HALO;
  const int nv1 = gt_row_count(row0, b, Tp) - HALO - 1;          // see gt_attn_bwd_kv_mfma_kernel
  auto RW = [&](int t) { return rbase + (size_t)(t < nv1 ? t : nv1); };
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
  const int li = lane & 15, qd = li >> 2, pp = li & 3, colhalf = ((lane >> 4) & 1) * 16;
  const float inv_sqrt = rsqrtf((float)D);
  bf16x8_t kf[6], vf[6];
  if (active && j < T) {
#pragma unroll
    for (int ks = 0; ks < 6; ++ks) {
      kf[ks] = *reinterpret_cast<const bf16x8_t*>(k + RW(j) * ld + h * D + ks * 16 + 8 * hh);
      vf[ks] = *reinterpret_cast<const bf16x8_t*>(v + RW(j) * ld + h * D + ks * 16 + 8 * hh);
    }
  } else {
    const uint4 z = make_uint4(0, 0, 0, 0);
#pragma unroll
    for (int ks = 0; ks < 6; ++ks) { kf[ks] = __builtin_bit_cast(bf16x8_t, z); vf[ks] = __builtin_bit_cast(bf16x8_t, z); }
  }
  f32x16_t ak[3], av[3];
#pragma unroll
  for (int dt = 0; dt < 3; ++dt) {
#pragma unroll
    for (int e = 0; e < 16; ++e) { ak[dt][e] = 0.f; av[dt][e] = 0.f; }
  }
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
#pragma unroll
      for (int e = 0; e < 16; ++e) { ss[e] = 0.f; sd[e] = 0.f; }
#pragma unroll
      for (int ks = 0; ks < 6; ++ks) {
        const bf16x8_t qa = *reinterpret_cast<const bf16x8_t*>(Qs + r * VP + ks * 16 + 8 * hh);
        const bf16x8_t da = *reinterpret_cast<const bf16x8_t*>(dOs + r * VP + ks * 16 + 8 * hh);
        ss = __builtin_amdgcn_mfma_f32_32x32x16_bf16(qa, kf[ks], ss, 0, 0, 0);
        sd = __builtin_amdgcn_mfma_f32_32x32x16_bf16(da, vf[ks], sd, 0, 0, 0);
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
          sc *= inv_sqrt;
          if (j >= T) sc = -3.0e38f;                             // not a key at all
          else if (j >= len || i >= len) sc = -1e4f;
          const float p = __expf(sc - mxs[e2]) * rds[e2];
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
#pragma unroll
      for (int s2 = 0; s2 < 2; ++s2) {
        float f8[8], g8[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) { f8[e] = ss[8 * s2 + e]; g8[e] = sd[8 * s2 + e]; }
        const bf16x8_t bds = pack8(f8), bpd = pack8(g8);         // bf16, as the saved-P path's workspace held them
#pragma unroll
        for (int dt = 0; dt < 3; ++dt) {
          const bf16_t* qa = Qs + (16 * s2 + 4 * hh + qd) * VP + 32 * dt + colhalf + 4 * pp;
          const bf16_t* da = dOs + (16 * s2 + 4 * hh + qd) * VP + 32 * dt + colhalf + 4 * pp;
          ak[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(tr_frag8(qa, qa + 8 * VP), bds, ak[dt], 0, 0, 0);
          av[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(tr_frag8(da, da + 8 * VP), bpd, av[dt], 0, 0, 0);
        }
      }
    }
    if (t + 1 < nqt) {
      GT_TILE_STORE(Qr + ((t + 1) & 1) * 32 * VP, qr)
      GT_TILE_STORE(Or + ((t + 1) & 1) * 32 * VP, dr)
      if (tid < 96) Sr[((t + 1) & 1) * 96 + tid] = sr;
    }
    __syncthreads();
  }
  if (active && j < T && j <= nv1) {
#pragma unroll
    for (int dt = 0; dt < 3; ++dt)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int d = 32 * dt + 8 * g + 4 * hh;
        *reinterpret_cast<uint2*>(dk + RW(j) * lddk + h * D + d) =
            make_uint2(pack2bf(ak[dt][4 * g], ak[dt][4 * g + 1]), pack2bf(ak[dt][4 * g + 2], ak[dt][4 * g + 3]));
        *reinterpret_cast<uint2*>(dv + RW(j) * lddk + h * D + d) =
            make_uint2(pack2bf(av[dt][4 * g], av[dt][4 * g + 1]), pack2bf(av[dt][4 * g + 2], av[dt][4 * g + 3]));
      }
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
