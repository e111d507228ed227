// What the MFMA attention kernels (attn_mfma.hip: T <= 384, attn_long.hip: 505 < T <= 4096) share: the head shape, the LDS
// pitches, the lane mapping and every step of a 32 x 32 tile that does not depend on WHERE a kernel keeps its operands (LDS whole,
// LDS ring, L2 with a register prefetch) — those, the tile loops, the barriers and the prefetch order stay in the kernels.
// All MFMAs are 32x32x16 bf16: a lane holds row / column r = lane & 31 and k-half hh = lane >> 5 of the operands, and accumulator
// element e of a lane is row (e&3) + 8(e>>2) + 4hh, column r.
#pragma once
#include "common.h"
#include "../../include/glowtts_hip.h"

namespace gt_attn_frag {

constexpr int HALO = GT_HALO;
constexpr int D = 96, WIN = 4, NW = 9;
constexpr int KP = 104;            // K / Ek pitch in halfs (208 B): conflict-free ds_read_b128 over 16 rows
constexpr int VP = 96;             // V pitch in halfs (192 B): conflict-free transposing reads
constexpr int BTP = 40;            // pitch (halfs) of the transposed band tables [16][32 + pad]

typedef __attribute__((__vector_size__(4 * sizeof(short)))) short s16x4_t;
typedef __attribute__((__vector_size__(8 * sizeof(short)))) short s16x8_t;

#define GT_ATTN_DEV __device__ __forceinline__

GT_ATTN_DEV bf16x8_t tr_frag8(const bf16_t* p0, const bf16_t* p1) {
  const s16x4_t lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4_t*)(uintptr_t)p0);
  const s16x4_t hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4_t*)(uintptr_t)p1);
  s16x8_t v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
  return __builtin_bit_cast(bf16x8_t, v);
}
GT_ATTN_DEV bf16x8_t pack8(const float* f) {
  const uint4 u = make_uint4(pack2bf(f[0], f[1]), pack2bf(f[2], f[3]), pack2bf(f[4], f[5]), pack2bf(f[6], f[7]));
  return __builtin_bit_cast(bf16x8_t, u);
}
GT_ATTN_DEV bf16x8_t zero8() { const uint4 z = make_uint4(0, 0, 0, 0); return __builtin_bit_cast(bf16x8_t, z); }
GT_ATTN_DEV f32x16_t mfma(bf16x8_t a, bf16x8_t b, f32x16_t c) { return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0); }
GT_ATTN_DEV void zero16(f32x16_t& a) {
#pragma unroll
  for (int e = 0; e < 16; ++e) a[e] = 0.f;
}
GT_ATTN_DEV void zero3(f32x16_t* o) { zero16(o[0]); zero16(o[1]); zero16(o[2]); }

struct Lane {
  int r, hh;                       // lane & 31, lane >> 5
  int tr;                          // offset of this lane's transposing read in a [rows][VP] tile: row qd, column colhalf + 4 pp
  GT_ATTN_DEV explicit Lane(int lane) : r(lane & 31), hh(lane >> 5), tr(((lane & 15) >> 2) * VP + ((lane >> 4) & 1) * 16 + 4 * (lane & 3)) {}
};

// Rows of utterance b behind its leading halo.  nv1 + 1 is the number of rows it owns there (frames + trailing halo): in the ragged
// layout frame indices past them belong to the NEXT utterance, so reads are clamped onto the (zero) trailing halo row — rw() — and
// stores are dropped — owns().
struct Rows {
  size_t rbase;
  int nv1;
  GT_ATTN_DEV Rows(const int32_t* row0, int b, int Tp) : rbase((size_t)gt_row_base(row0, b, Tp) + HALO), nv1(gt_row_count(row0, b, Tp) - HALO - 1) {}
  GT_ATTN_DEV size_t rw(int t) const { return rbase + (size_t)(t < nv1 ? t : nv1); }
  GT_ATTN_DEV bool owns(int t) const { return t <= nv1; }
};

// The dropout of one (query row, key) element; row = (b H + h) T + i
struct Drop {
  uint32_t thresh, seed, row;
  float scale;
  GT_ATTN_DEV bool keep(int j) const { return drop_keep(seed, row, j, thresh); }
  GT_ATTN_DEV float operator()(float x, int j) const { return thresh ? (keep(j) ? x * scale : 0.f) : x; }
};

// ---- the images of a relative table E[NW][D] (Ek or Ev): rows, [32][KP] with rows >= 9 zero (the A operand of the rel-table
// chain), and transpose, [D][16] with columns >= 9 zero (the A operand of the band MFMA); nth threads
GT_ATTN_DEV void stage_rel_rows(bf16_t* Es, const float* E, int tid, int nth) {
  for (int i = tid; i < 32 * D; i += nth) { const int rr = i / D, c = i - rr * D; Es[rr * KP + c] = rr < NW ? f2bf(E[rr * D + c]) : (bf16_t)0; }
}
GT_ATTN_DEV void stage_rel_tr(bf16_t* ET, const float* E, int tid, int nth) {
  for (int i = tid; i < D * 16; i += nth) { const int d = i >> 4, rr = i & 15; ET[i] = rr < NW ? f2bf(E[rr * D + d]) : (bf16_t)0; }
}

// six k-steps of one operand row (16 channels each, this lane's 8), or zeros
GT_ATTN_DEV void load_frag6(bf16x8_t* f, const bf16_t* row, int hh) {
#pragma unroll
  for (int ks = 0; ks < 6; ++ks) f[ks] = *reinterpret_cast<const bf16x8_t*>(row + ks * 16 + 8 * hh);
}
GT_ATTN_DEV void zero_frag6(bf16x8_t* f) {
#pragma unroll
  for (int ks = 0; ks < 6; ++ks) f[ks] = zero8();
}
// the fragments of row 32t + r of a [rows][ld] operand in L2 (head h), lane = (row r of tile t, k-half hh); rows >= T are zero
GT_ATTN_DEV void load_tile_frag6(bf16x8_t* f, const bf16_t* src, int ld, int h, int t, int T, const Rows& rows, const Lane& ln) {
  const int j = 32 * t + ln.r;
  if (j < T) load_frag6(f, src + rows.rw(j) * ld + h * D, ln.hh); else zero_frag6(f);
}
GT_ATTN_DEV void copy_frag6(bf16x8_t* f, const bf16x8_t* n) {
#pragma unroll
  for (int ks = 0; ks < 6; ++ks) f[ks] = n[ks];
}
// st = A X^T over the 96 channels: A rows `a` (this lane's row of an LDS image, any pitch), X fragments xf
GT_ATTN_DEV void mfma6(f32x16_t& st, const bf16_t* a, const bf16x8_t* xf, int hh) {
  zero16(st);
#pragma unroll
  for (int ks = 0; ks < 6; ++ks) st = mfma(*reinterpret_cast<const bf16x8_t*>(a + ks * 16 + 8 * hh), xf[ks], st);
}
GT_ATTN_DEV void mfma6(f32x16_t& st, const bf16x8_t* af, const bf16x8_t* xf) {
  zero16(st);
#pragma unroll
  for (int ks = 0; ks < 6; ++ks) st = mfma(af[ks], xf[ks], st);
}

// ---- the rel-table chain: tab[32][NW] of the wave, tab[query r][r'] = E[r'] . x_r (QE = Ek Q^T, DOE = Ev dO^T): accumulator rows
// r' < 9 leave (both lane halves write: a wave barrier goes between this and the first read)
GT_ATTN_DEV void rel_store(float* tab, const f32x16_t& acc, const Lane& ln) {
#pragma unroll
  for (int e = 0; e < 4; ++e) tab[ln.r * NW + e + 4 * ln.hh] = acc[e];
  if (ln.hh == 0) tab[ln.r * NW + 8] = acc[4];
}
GT_ATTN_DEV void rel_table(float* tab, const bf16_t* Es, const bf16x8_t* xf, const Lane& ln) {
  f32x16_t acc;
  mfma6(acc, Es + ln.r * KP, xf, ln.hh);
  rel_store(tab, acc, ln);
}

// ---- one score element of query i, key j: the band term out of the wave's table row, the scale, the two masks
GT_ATTN_DEV float band_add(float x, const float* row, int i, int j) {
  const int rel = j - i + WIN;
  if ((unsigned)rel <= 2u * WIN) x += row[rel];
  return x;
}
GT_ATTN_DEV float mask_scale(float sc, int i, int j, int T, int len, float inv_sqrt) {
  sc *= inv_sqrt;
  if (j >= T) sc = -3.0e38f;                                     // not a key at all
  else if (j >= len || i >= len) sc = -1e4f;                     // masked_fill(mask == 0, -1e4), attentions.py:260
  return sc;
}
// the masked, scaled scores of key tile t in place (element e <-> key 32t + (e&3) + 8(e>>2) + 4hh)
GT_ATTN_DEV void score_tile(f32x16_t& st, int t, const float* qerow, int i, int hh, int T, int len, float inv_sqrt) {
#pragma unroll
  for (int e = 0; e < 16; ++e) {
    const int j = 32 * t + (e & 3) + 8 * (e >> 2) + 4 * hh;
    st[e] = mask_scale(band_add(st[e], qerow, i, j), i, j, T, len, inv_sqrt);
  }
}

// ---- the online softmax of the two-walk forwards: one tile of masked scores into this lane's running (max, denominator), and the
// merge of the two lane halves of a query after the last tile
GT_ATTN_DEV void online_tile(const f32x16_t& st, float& mx, float& den) {
  float tm = st[0];
#pragma unroll
  for (int e = 1; e < 16; ++e) tm = fmaxf(tm, st[e]);
  const float mn = fmaxf(mx, tm);
  float add = 0.f;
#pragma unroll
  for (int e = 0; e < 16; ++e) add += __expf(st[e] - mn);
  den = den * __expf(mx - mn) + add;
  mx = mn;
}
GT_ATTN_DEV void online_merge(float& mx, float& den) {
  const float mo = __shfl_xor(mx, 32), dn = __shfl_xor(den, 32);
  const float mm = fmaxf(mx, mo);
  den = den * __expf(mx - mm) + dn * __expf(mo - mm);
  mx = mm;
}

// ---- four consecutive P values of a row: 16-byte form where T allows (palign 4), 8-byte (palign 2, loads only), else scalar
GT_ATTN_DEV void store_p4(float* prow, int j0, int T, bool vec, const float* p4) {
  if (vec && j0 + 3 < T) *reinterpret_cast<float4*>(prow + j0) = make_float4(p4[0], p4[1], p4[2], p4[3]);
  else {
#pragma unroll
    for (int e2 = 0; e2 < 4; ++e2) if (j0 + e2 < T) prow[j0 + e2] = p4[e2];
  }
}
GT_ATTN_DEV void load_p4(const float* prow, int j0, int T, int palign, float* p4) {
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

// ---- the forwards' P tile (st holds P of key tile t): the row leaves (STORE_P, query i < T), dropout in place, and the
// band entries go to the wave's table pb[32][16]
template <bool STORE_P>
GT_ATTN_DEV void p_tile_out(f32x16_t& st, int t, float* prow, bool vec, int i, const Lane& ln, int T, const Drop& drop, bf16_t* pb) {
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    const int j0 = 32 * t + 8 * g + 4 * ln.hh;
    float p4[4];
#pragma unroll
    for (int e2 = 0; e2 < 4; ++e2) p4[e2] = st[4 * g + e2];
    if (STORE_P && i < T) store_p4(prow, j0, T, vec, p4);
#pragma unroll
    for (int e2 = 0; e2 < 4; ++e2) {
      const int j = j0 + e2;
      const float pd = drop(p4[e2], j);
      st[4 * g + e2] = pd;
      const int rel = j - i + WIN;
      if ((unsigned)rel <= 2u * WIN && j < T) pb[ln.r * 16 + rel] = f2bf(pd);
    }
  }
}

// ---- the accumulator tile as the next MFMA's operand: o^T[d][.] += X^T[d][k] st[k][.] over the 32 rows k of tile X [32][VP]
// (O^T += V^T P^T, dQ^T += K^T dS^T, dK^T += Q^T dS, dV^T += dO^T P').  MFMA s2 takes pack8(st + 8 s2), i.e. k index 8hh + kk <-> row
// 16 s2 + 4hh + (kk&3) + 8(kk>>2) of the tile, and the transposing reads take the rows in that same order.
GT_ATTN_DEV void acc_operand(f32x16_t* o, const f32x16_t& st, const bf16_t* X, const Lane& ln) {
#pragma unroll
  for (int s2 = 0; s2 < 2; ++s2) {
    float f8[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) f8[e] = st[8 * s2 + e];
    const bf16x8_t pf = pack8(f8);
#pragma unroll
    for (int dt = 0; dt < 3; ++dt) {
      const bf16_t* xa = X + (16 * s2 + 4 * ln.hh) * VP + 32 * dt + ln.tr;
      o[dt] = mfma(tr_frag8(xa, xa + 8 * VP), pf, o[dt]);
    }
  }
}

// ---- the band MFMA (K = 16): o^T += ET^T band^T with ET [D][16] and the wave's band table [32][16] (k = rel)
GT_ATTN_DEV void band_mfma(f32x16_t* o, const bf16_t* ET, const bf16_t* band, const Lane& ln) {
  const bf16x8_t bfp = *reinterpret_cast<const bf16x8_t*>(band + ln.r * 16 + 8 * ln.hh);
#pragma unroll
  for (int dt = 0; dt < 3; ++dt) o[dt] = mfma(*reinterpret_cast<const bf16x8_t*>(ET + (32 * dt + ln.r) * 16 + 8 * ln.hh), bfp, o[dt]);
}

// ---- this lane's 48 of the 96 channels of one output row (dst: the row's head slice), bf16 in 8-byte pieces
GT_ATTN_DEV void store_row96(bf16_t* dst, const f32x16_t* o, int hh) {
#pragma unroll
  for (int dt = 0; dt < 3; ++dt)
#pragma unroll
    for (int g = 0; g < 4; ++g)
      *reinterpret_cast<uint2*>(dst + 32 * dt + 8 * g + 4 * hh) =
          make_uint2(pack2bf(o[dt][4 * g], o[dt][4 * g + 1]), pack2bf(o[dt][4 * g + 2], o[dt][4 * g + 3]));
}

// ---- query side of the backward.  dP of one element out of dPd: band term, dropout, 0 past T
GT_ATTN_DEV float dp_elem(float dp, const float* doerow, int i, int j, int T, const Drop& drop) {
  dp = drop(band_add(dp, doerow, i, j), j);
  return j >= T ? 0.f : dp;
}
// dS of one element (returned) and its P' (pd), both masked
GT_ATTN_DEV float ds_elem(float p, float dp, float dsum, float inv_sqrt, int i, int j, int T, int len, const Drop& drop, float& pd) {
  float ds = p * (dp - dsum) * inv_sqrt;
  pd = drop(p, j);
  if (j >= T || j >= len || i >= len || i >= T) ds = 0.f;          // masked_fill blocks the gradient
  if (i >= len || i >= T) pd = 0.f;                                // padded queries carry no upstream gradient
  return ds;
}
// ... which enter the wave's band tables bt = dSB[32][16] | dSBT[16][BTP] | PdBT[16][BTP] where key j < T is on the band of query i
constexpr int BAND_TABLES = 32 * 16 + 2 * 16 * BTP;
GT_ATTN_DEV void band_tables(bf16_t* bt, int r, int i, int j, float ds, float pd) {
  const int rel = j - i + WIN;
  if ((unsigned)rel <= 2u * WIN) {
    const bf16_t db = f2bf(ds);
    bt[r * 16 + rel] = db; bt[32 * 16 + rel * BTP + r] = db; bt[32 * 16 + 16 * BTP + rel * BTP + r] = f2bf(pd);
  }
}
// the dE contraction of one 32-query tile: acc[r'][d] += sum_i At[r'][i] X[i][d] for the 32 channels 32 dt .. of X [32][VP]
// (dEk: At = dSBT, X = Q; dEv: At = PdBT, X = dO), then the wave's nine rows into the block's accumulator accA[NW][D]
GT_ATTN_DEV void de_chain(f32x16_t& acc, const bf16_t* At, const bf16_t* X, int dt, const Lane& ln) {
#pragma unroll
  for (int ks = 0; ks < 2; ++ks) {
    bf16x8_t af = *reinterpret_cast<const bf16x8_t*>(At + (ln.r & 15) * BTP + 16 * ks + 8 * ln.hh);
    if (ln.r >= 16) af = zero8();
    const bf16_t* ba = X + (16 * ks + 8 * ln.hh) * VP + 32 * dt + ln.tr;
    acc = mfma(af, tr_frag8(ba, ba + 4 * VP), acc);
  }
}
GT_ATTN_DEV void de_add(float* accA, const f32x16_t& acc, int dt, const Lane& ln) {
  const int d = 32 * dt + ln.r;                                  // D layout: column = d (lane&31), row r' = (e&3)+8(e>>2)+4hh
#pragma unroll
  for (int e = 0; e < 4; ++e) atomicAdd(accA + (e + 4 * ln.hh) * D + d, acc[e]);
  if (ln.hh == 0) atomicAdd(accA + 8 * D + d, acc[4]);
}
GT_ATTN_DEV void de_contract(float* accA, const bf16_t* At, const bf16_t* X, const Lane& ln) {
#pragma unroll
  for (int dt = 0; dt < 3; ++dt) {
    f32x16_t acc;
    zero16(acc);
    de_chain(acc, At, X, dt, ln);
    de_add(accA, acc, dt, ln);
  }
}
// the block's accumulator Acc[2][NW][D] (dEk | dEv) into the global gradients, after a block barrier
GT_ATTN_DEV void acc_flush(const float* Acc, float* dEk, float* dEv, int tid, int nth) {
  for (int x = tid; x < NW * D; x += nth) {
    if (Acc[x] != 0.f) atomicAdd(dEk + x, Acc[x]);
    if (Acc[NW * D + x] != 0.f) atomicAdd(dEv + x, Acc[NW * D + x]);
  }
}

// ---- key side of the backward: dK^T += Q^T dS and dV^T += dO^T P' over the 16 queries 16 ks .. of the [rows][VP] images Qs / dOs
GT_ATTN_DEV void kv_pair(f32x16_t* ak, f32x16_t* av, const bf16_t* Qs, const bf16_t* dOs, int ks, bf16x8_t bds, bf16x8_t bpd, const Lane& ln) {
#pragma unroll
  for (int dt = 0; dt < 3; ++dt) {
    const bf16_t* qa = Qs + (16 * ks + 8 * ln.hh) * VP + 32 * dt + ln.tr;
    const bf16_t* da = dOs + (16 * ks + 8 * ln.hh) * VP + 32 * dt + ln.tr;
    ak[dt] = mfma(tr_frag8(qa, qa + 4 * VP), bds, ak[dt]);
    av[dt] = mfma(tr_frag8(da, da + 4 * VP), bpd, av[dt]);
  }
}

}  // namespace gt_attn_frag
