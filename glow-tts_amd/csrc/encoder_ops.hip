// Text-encoder / glue kernels for gfx950 in the rows layout (see glowtts_hip.h):
//   channel LayerNorm (+residual, dropout, relu)   modules.py:26-44, attentions.py:79-84, modules.py:95-102
//   relative-position multi-head attention          attentions.py:241-336 (9-diagonal band form, SURVEY App. A iii)
//   embedding * sqrt(H)                             models.py:693
//   row tables, per-utterance vectors and the fills at the head of a step
// (what lies between the decoder and the loss is csrc/align_loss.hip).  fp32 math throughout; bf16 only for tensors that feed MFMA GEMMs.
#include <stdlib.h>
#include "common.h"
#include "../../include/glowtts_hip.h"
#include "internal.h"

namespace {

constexpr int HALO = GT_HALO;

// ------------------------------------------------------------------ LayerNorm over channels
// s = a + drop_in(y);  n = (s-mean)*rstd*gamma + beta;  o = drop_out(relu?(n));
// out_f32 = o*mask, out_bf16 = o*mask.  One wave per row, C <= 256 (4 values per lane).
struct LnArgs {
  const float* a; const bf16_t* y; int ldy;
  const float* gamma; const float* beta;
  const float* rowmask;
  float* out_f32; bf16_t* out_bf16; int ldo;
  float* mean; float* rstd;
  int R, C; float eps;
  uint32_t din_thresh, din_seed; float din_scale;
  uint32_t dout_thresh, dout_seed; float dout_scale;
  int relu;
  const uint32_t* seed_dev;                    // optional device word XOR-ed into both seeds (graph replay)
};

// Every load of a row goes out before the first use: which of a / y (and, backward, dout_f32 / dout_bf16) exist is a template
// parameter, channels past C read channel C - 1 (an address only: the value is never used), rows past the end read row R - 1,
// and the optional rowmask / seed word come through a pointer chosen beforehand (gamma stands in where they are absent).  A
// wave then waits ONCE for its row instead of once per operand.  The arithmetic is the former kernels'.
// ln_landed: the compiler otherwise sinks a load into the first block that uses it, behind that block's branch: an empty statement that
// names the loaded register after ALL the loads were issued keeps them together in front of it.
template <typename T> __device__ __forceinline__ void ln_landed(T& x) { asm volatile("" : "+v"(x)); }

template <bool HAS_A, bool HAS_Y>
__global__ __launch_bounds__(256) void gt_layernorm_fwd_kernel(LnArgs p)
{
  const int m = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (m >= p.R) return;
  const uint32_t sx = *(p.seed_dev ? p.seed_dev : reinterpret_cast<const uint32_t*>(p.gamma));
  float rmv = *(p.rowmask ? p.rowmask + m : p.gamma);
  float av[4], gv[4], bv[4]; uint32_t yv[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int cl = min(lane + 64 * k, p.C - 1);
    if (HAS_A) av[k] = p.a[(size_t)m * p.C + cl];
    if (HAS_Y) yv[k] = p.y[(size_t)m * p.ldy + cl];
    gv[k] = p.gamma[cl]; bv[k] = p.beta[cl];
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    if (HAS_A) ln_landed(av[k]);
    if (HAS_Y) ln_landed(yv[k]);
    ln_landed(gv[k]); ln_landed(bv[k]);
  }
  ln_landed(rmv);
  if (p.seed_dev) { p.din_seed ^= sx; p.dout_seed ^= sx; }
  float s[4]; float sum = 0.f;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int c = lane + 64 * k;
    float v = 0.f;
    if (c < p.C) {
      if (HAS_A) v = av[k];
      if (HAS_Y) {
        float yy = bf2f((bf16_t)yv[k]);
        if (p.din_thresh) yy = drop_keep(p.din_seed, m, c, p.din_thresh) ? yy * p.din_scale : 0.f;
        v += yy;
      }
      sum += v;
    }
    s[k] = v;
  }
  const float mean = wave_sum(sum) / (float)p.C;
  float var = 0.f;
#pragma unroll
  for (int k = 0; k < 4; ++k) { const int c = lane + 64 * k; if (c < p.C) { const float d = s[k] - mean; var += d * d; } }
  const float rstd = rsqrtf(wave_sum(var) / (float)p.C + p.eps);
  if (lane == 0) { p.mean[m] = mean; p.rstd[m] = rstd; }
  const float rm = p.rowmask ? rmv : 1.0f;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int c = lane + 64 * k;
    if (c < p.C) {
      float o = (s[k] - mean) * rstd * gv[k] + bv[k];
      if (p.relu) o = fmaxf(o, 0.f);
      if (p.dout_thresh) o = drop_keep(p.dout_seed, m, c, p.dout_thresh) ? o * p.dout_scale : 0.f;
      o *= rm;
      if (p.out_f32) p.out_f32[(size_t)m * p.C + c] = o;
      if (p.out_bf16) p.out_bf16[(size_t)m * p.ldo + c] = f2bf(o);
    }
  }
}

struct LnBwdArgs {
  LnArgs f;                                    // forward description (inputs, mean/rstd, flags)
  const float* dout_f32; const bf16_t* dout_bf16; int lddo;
  float* da; bf16_t* dy; int lddy;             // gradients wrt a (fp32) and y (bf16, dropout replayed)
  float* dgamma; float* dbeta;                 // accumulated (atomics)
  float* partials;                             // or: row blockIdx.x of [gridDim.x][2 C] receives this workgroup's sums (no atomics)
};

// LNB_WAVES waves x LNB_ROWS rows per wave (a workgroup takes LNB_WAVES * LNB_ROWS rows; wave w takes rows w, w + LNB_WAVES, ... in
// that order); gamma/beta partials are folded in LDS so that each channel gets ONE atomic per workgroup (same-address float
// atomics serialise at L2, ~50 ns each: 32 rows per workgroup keeps both the atomic chain and the per-wave row loop short).
// The loads of ALL the wave's rows are in flight before the first row's arithmetic.
template <int LNB_WAVES, int LNB_ROWS, bool HAS_A, bool HAS_Y, bool HAS_DF, bool HAS_DB>
__global__ __launch_bounds__(64 * LNB_WAVES) void gt_layernorm_bwd_kernel(LnBwdArgs q)
{
  const LnArgs& p = q.f;
  __shared__ float sg[LNB_WAVES][256], sb[LNB_WAVES][256];
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  constexpr int RPB = LNB_WAVES * LNB_ROWS;
  const int m0 = blockIdx.x * RPB, m1 = min(p.R, m0 + RPB);
  const uint32_t sx = *(p.seed_dev ? p.seed_dev : reinterpret_cast<const uint32_t*>(p.gamma));
  float gv[4], bv[4];
  float meanv[LNB_ROWS], rstdv[LNB_ROWS], rmv[LNB_ROWS], av[LNB_ROWS][4], dfv[LNB_ROWS][4];
  uint32_t yv[LNB_ROWS][4], dbv[LNB_ROWS][4];
#pragma unroll
  for (int r = 0; r < LNB_ROWS; ++r) {
    const int ml = min(m0 + w + r * LNB_WAVES, p.R - 1);
    meanv[r] = p.mean[ml]; rstdv[r] = p.rstd[ml];
    rmv[r] = *(p.rowmask ? p.rowmask + ml : p.gamma);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int cl = min(lane + 64 * k, p.C - 1);
      if (HAS_A) av[r][k] = p.a[(size_t)ml * p.C + cl];
      if (HAS_Y) yv[r][k] = p.y[(size_t)ml * p.ldy + cl];
      if (HAS_DF) dfv[r][k] = q.dout_f32[(size_t)ml * p.C + cl];
      if (HAS_DB) dbv[r][k] = q.dout_bf16[(size_t)ml * q.lddo + cl];
    }
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) { const int cl = min(lane + 64 * k, p.C - 1); gv[k] = p.gamma[cl]; bv[k] = p.beta[cl]; }
#pragma unroll
  for (int r = 0; r < LNB_ROWS; ++r) {
    ln_landed(meanv[r]); ln_landed(rstdv[r]); ln_landed(rmv[r]);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (HAS_A) ln_landed(av[r][k]);
      if (HAS_Y) ln_landed(yv[r][k]);
      if (HAS_DF) ln_landed(dfv[r][k]);
      if (HAS_DB) ln_landed(dbv[r][k]);
    }
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) { ln_landed(gv[k]); ln_landed(bv[k]); }
  const uint32_t din_seed = p.seed_dev ? p.din_seed ^ sx : p.din_seed, dout_seed = p.seed_dev ? p.dout_seed ^ sx : p.dout_seed;
  float accg[4] = {0, 0, 0, 0}, accb[4] = {0, 0, 0, 0};
#pragma unroll
  for (int r = 0; r < LNB_ROWS; ++r) {
    const int m = m0 + w + r * LNB_WAVES;
    if (m >= m1) break;
    const float mean = meanv[r], rstd = rstdv[r];
    const float rm = p.rowmask ? rmv[r] : 1.0f;
    float xh[4], dn[4]; bool keep_in[4];
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int c = lane + 64 * k;
      xh[k] = 0.f; dn[k] = 0.f; keep_in[k] = true;
      if (c < p.C) {
        float v = HAS_A ? av[r][k] : 0.f;
        if (HAS_Y) {
          const bf16_t yraw = (bf16_t)yv[r][k];
          float yy = bf2f(yraw);
          if (p.din_thresh) { keep_in[k] = drop_keep(din_seed, m, c, p.din_thresh); yy = keep_in[k] ? yy * p.din_scale : 0.f; }
          if ((p.relu & 2) && !(yraw & 0x7fff)) keep_in[k] = false;      // y is a ReLU's output: no gradient through its zeros
          v += yy;
        }
        xh[k] = (v - mean) * rstd;
        float d = 0.f;
        if (HAS_DF) d += dfv[r][k];
        if (HAS_DB) d += bf2f((bf16_t)dbv[r][k]);
        d *= rm;
        if (p.dout_thresh) d = drop_keep(dout_seed, m, c, p.dout_thresh) ? d * p.dout_scale : 0.f;
        if ((p.relu & 1) && (xh[k] * gv[k] + bv[k]) <= 0.f) d = 0.f;
        accg[k] += d * xh[k]; accb[k] += d;
        dn[k] = d * gv[k];
        s1 += dn[k]; s2 += dn[k] * xh[k];
      }
    }
    s1 = wave_sum(s1) / (float)p.C; s2 = wave_sum(s2) / (float)p.C;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int c = lane + 64 * k;
      if (c < p.C) {
        const float ds = rstd * (dn[k] - s1 - xh[k] * s2);
        if (q.da) q.da[(size_t)m * p.C + c] = ds;
        if (q.dy) q.dy[(size_t)m * q.lddy + c] = f2bf((p.din_thresh || (p.relu & 2)) ? (keep_in[k] ? ds * p.din_scale : 0.f) : ds);
      }
    }
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) { sg[w][lane + 64 * k] = accg[k]; sb[w][lane + 64 * k] = accb[k]; }
  __syncthreads();
  const int c = threadIdx.x;
  if (c < p.C) {
    float tg = 0.f, tb = 0.f;
#pragma unroll
    for (int i = 0; i < LNB_WAVES; ++i) { tg += sg[i][c]; tb += sb[i][c]; }
    if (q.partials) {
      q.partials[(size_t)blockIdx.x * 2 * p.C + c] = tg;
      q.partials[(size_t)blockIdx.x * 2 * p.C + p.C + c] = tb;
    } else {
      atomicAdd(q.dgamma + c, tg);
      atomicAdd(q.dbeta + c, tb);
    }
  }
}

// Parameter gradients from the partial rows backward launches left (gt_layernorm_bwd_partials, gt_dds_*_bwd with `partials`): the
// column sums of up to GT_PARTIALS_MAX buffers [n_rows][Ca + Cb] are ADDED to dst_a[Ca] | dst_b[Cb] — one launch at the end of a
// module's backward instead of same-address atomics from every workgroup of every one of them.
// block (x: 64-column group, y: job, z: slice of the rows — PARTIALS_ZS adders per address); thread = (column, row phase)
constexpr int PARTIALS_ZS = 4;
__global__ __launch_bounds__(256) void gt_param_partials_reduce_kernel(gt_partials_args a)
{
  __shared__ float red[4][64];
  const gt_partials_job j = a.job[blockIdx.y];
  const int W = j.Ca + j.Cb;
  const int c = blockIdx.x * 64 + (threadIdx.x & 63), ph = threadIdx.x >> 6;
  if (blockIdx.x * 64 >= W) return;
  const int per = ((j.n_rows + PARTIALS_ZS - 1) / PARTIALS_ZS + 3) & ~3, r0 = blockIdx.z * per, r1 = min(j.n_rows, r0 + per);
  float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
  if (c < W) {
    const float* pp = j.partials + c;
    const size_t st = (size_t)W;
    int r = r0 + ph;
    for (; r + 12 < r1; r += 16) {
      const float v0 = pp[(size_t)r * st], v1 = pp[(size_t)(r + 4) * st], v2 = pp[(size_t)(r + 8) * st], v3 = pp[(size_t)(r + 12) * st];
      s0 += v0; s1 += v1; s2 += v2; s3 += v3;
    }
    for (; r < r1; r += 4) s0 += pp[(size_t)r * st];
  }
  red[ph][threadIdx.x & 63] = (s0 + s1) + (s2 + s3);
  __syncthreads();
  if (ph == 0 && c < W) {
    const float t = (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]);
    float* d = c < j.Ca ? j.dst_a + c : j.dst_b + (c - j.Ca);
    atomicAdd(d, t);
  }
}

// ------------------------------------------------------------------ relative-position attention
// q,k,v: rows [R, H*D] bf16 (head h = channels [h*D, (h+1)*D)), D <= 96, window w (2w+1 taps, shared
// by heads).  One workgroup per (query tile of 16 rows, head, utterance); K and V of the
// utterance-head staged in LDS as fp32-convertible bf16 with an odd dword pitch.
//   score[i,j] = (q_i.k_j + [|j-i|<=w] q_i.Ek[j-i+w]) / sqrt(D);  key j >= len -> -1e4
//   p = softmax_j(score);  pd = dropout(p);  out_i = sum_j pd[i,j] v_j + sum_{|j-i|<=w} pd[i,j] Ev[j-i+w]
// P (pre-dropout, fp32) is saved to Pout [B,H,T,T] for the backward pass.
constexpr int AT_QT = 16;
constexpr int AT_MAXD = 96;

__device__ __forceinline__ void at_stage(bf16_t* dst, const bf16_t* src, int ld, size_t rbase, int h, int T, int D, int KP, int tid, int nv1)
{
  for (int i = tid; i < T * (D / 2); i += 256) {
    const int j = i / (D / 2), c2 = i - j * (D / 2);
    *reinterpret_cast<uint32_t*>(dst + (size_t)j * KP + 2 * c2) = *reinterpret_cast<const uint32_t*>(src + (rbase + (j < nv1 ? j : nv1)) * ld + h * D + 2 * c2);
  }
}
__device__ __forceinline__ float at_dot(const float* qv, const bf16_t* row, int D)
{
  float s = 0.f;
  for (int c = 0; c < D; c += 2) {
    const uint32_t kk = *reinterpret_cast<const uint32_t*>(row + c);
    s += qv[c] * bf2f(kk & 0xffff) + qv[c + 1] * bf2f(kk >> 16);
  }
  return s;
}

// LDS: one [T][D+2] bf16 staging buffer (K then V), band tables, per-wave q row, [16][T] score rows.
__global__ __launch_bounds__(256) void gt_attn_fwd_kernel(
    const bf16_t* __restrict__ q, const bf16_t* __restrict__ k, const bf16_t* __restrict__ v, int ld,
    const float* __restrict__ Ek, const float* __restrict__ Ev, const int32_t* __restrict__ lens,
    bf16_t* __restrict__ out, int ldo, float* __restrict__ Pout,
    int T, int Tp, const int32_t* row0, int H, int D, int win, uint32_t drop_thresh, uint32_t drop_seed, float drop_scale, const uint32_t* __restrict__ seed_dev)
{
  if (seed_dev) drop_seed ^= *seed_dev;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int b = blockIdx.z, h = blockIdx.y, i0 = blockIdx.x * AT_QT;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int KP = D + 2, NW = 2 * win + 1;                // odd dword pitch
  bf16_t* St = reinterpret_cast<bf16_t*>(smem);          // [T][KP]
  float* Es = reinterpret_cast<float*>(St + (size_t)T * KP + (((size_t)T * KP) & 1));   // Ek [NW][D], Ev [NW][D]
  float* Qs = Es + 2 * NW * D;                           // [4 waves][D]
  float* Ps = Qs + 4 * D;                                // [AT_QT][T]
  const int len = lens[b];
  const size_t rbase = (size_t)gt_row_base(row0, b, Tp) + HALO;
  const int nv1 = gt_row_count(row0, b, Tp) - HALO - 1;          // ragged layout: last own row behind rbase (attn_mfma.hip)
  auto RW = [&](int t) { return rbase + (size_t)(t < nv1 ? t : nv1); };
  at_stage(St, k, ld, rbase, h, T, D, KP, tid, nv1);
  for (int i = tid; i < NW * D; i += 256) { Es[i] = Ek[i]; Es[NW * D + i] = Ev[i]; }
  __syncthreads();
  const float inv_sqrt = rsqrtf((float)D);
  float* qv = Qs + w * D;
  for (int ii = w; ii < AT_QT; ii += 4) {
    const int i = i0 + ii;
    if (i >= T) break;                                   // wave-uniform
    float* pv = Ps + (size_t)ii * T;
    for (int c = lane; c < D; c += 64) qv[c] = bf2f(q[RW(i) * ld + h * D + c]);
    __builtin_amdgcn_wave_barrier();
    float mx = -3.0e38f;
    for (int j = lane; j < T; j += 64) {
      float s = at_dot(qv, St + (size_t)j * KP, D);
      const int rel = j - i + win;
      if (rel >= 0 && rel <= 2 * win) { const float* e = Es + rel * D; float t = 0.f; for (int c = 0; c < D; ++c) t += qv[c] * e[c]; s += t; }
      s *= inv_sqrt;
      if (j >= len || i >= len) s = -1e4f;                // masked_fill(mask == 0, -1e4), attentions.py:260
      pv[j] = s; mx = fmaxf(mx, s);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
    float den = 0.f;
    for (int j = lane; j < T; j += 64) { const float e = __expf(pv[j] - mx); pv[j] = e; den += e; }
    den = wave_sum(den);
    const float rden = 1.0f / den;
    float* prow = Pout + (((size_t)b * H + h) * T + i) * T;
    for (int j = lane; j < T; j += 64) {
      const float pj = pv[j] * rden;
      prow[j] = pj;
      float pd = pj;
      if (drop_thresh) pd = drop_keep(drop_seed, (uint32_t)((b * H + h) * T + i), j, drop_thresh) ? pj * drop_scale : 0.f;
      pv[j] = pd;
    }
    __builtin_amdgcn_wave_barrier();
  }
  __syncthreads();
  at_stage(St, v, ld, rbase, h, T, D, KP, tid, nv1);
  __syncthreads();
  for (int ii = w; ii < AT_QT; ii += 4) {
    const int i = i0 + ii;
    if (i >= T) break;
    const float* pv = Ps + (size_t)ii * T;
    for (int c = lane; c < D; c += 64) {
      float acc = 0.f;
      for (int j = 0; j < T; ++j) acc += pv[j] * bf2f(St[(size_t)j * KP + c]);
      for (int rel = 0; rel <= 2 * win; ++rel) { const int j = i + rel - win; if (j >= 0 && j < T) acc += pv[j] * Es[NW * D + rel * D + c]; }
      if (i <= nv1) out[(rbase + i) * ldo + h * D + c] = f2bf(acc);
    }
  }
}

// backward, pass 1 (per query row): dS row -> dSout [B,H,T,T] fp32 (scaled by 1/sqrt(D)), dQ, dEk, dEv.
__global__ __launch_bounds__(256) void gt_attn_bwd_q_kernel(
    const bf16_t* __restrict__ q, const bf16_t* __restrict__ k, const bf16_t* __restrict__ v, int ld,
    const float* __restrict__ Ek, const float* __restrict__ Ev, const int32_t* __restrict__ lens,
    const bf16_t* __restrict__ dout, int lddo, const float* __restrict__ P, float* __restrict__ dS,
    bf16_t* __restrict__ dq, int lddq, float* __restrict__ dEk, float* __restrict__ dEv,
    int T, int Tp, const int32_t* row0, int H, int D, int win, uint32_t drop_thresh, uint32_t drop_seed, float drop_scale, const uint32_t* __restrict__ seed_dev)
{
  if (seed_dev) drop_seed ^= *seed_dev;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int b = blockIdx.z, h = blockIdx.y, i0 = blockIdx.x * AT_QT;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int KP = D + 2, NW = 2 * win + 1;
  bf16_t* St = reinterpret_cast<bf16_t*>(smem);
  float* Es = reinterpret_cast<float*>(St + (size_t)T * KP + (((size_t)T * KP) & 1));
  float* Acc = Es + 2 * NW * D;                          // block-local dEk | dEv accumulators [2][NW][D]
  float* Qs = Acc + 2 * NW * D;                          // [AT_QT][2*D]: q row and dO row
  float* Ps = Qs + AT_QT * 2 * D;                        // [AT_QT][T]
  const int len = lens[b];
  const size_t rbase = (size_t)gt_row_base(row0, b, Tp) + HALO;
  const int nv1 = gt_row_count(row0, b, Tp) - HALO - 1;          // ragged layout: last own row behind rbase (attn_mfma.hip)
  auto RW = [&](int t) { return rbase + (size_t)(t < nv1 ? t : nv1); };
  at_stage(St, v, ld, rbase, h, T, D, KP, tid, nv1);
  for (int i = tid; i < NW * D; i += 256) { Es[i] = Ek[i]; Es[NW * D + i] = Ev[i]; Acc[i] = 0.f; Acc[NW * D + i] = 0.f; }
  __syncthreads();
  const float inv_sqrt = rsqrtf((float)D);
  for (int ii = w; ii < AT_QT; ii += 4) {
    const int i = i0 + ii;
    if (i >= T) break;
    float* qv = Qs + ii * 2 * D; float* dov = qv + D;
    float* pv = Ps + (size_t)ii * T;
    for (int c = lane; c < D; c += 64) { qv[c] = bf2f(q[RW(i) * ld + h * D + c]); dov[c] = bf2f(dout[RW(i) * lddo + h * D + c]); }
    __builtin_amdgcn_wave_barrier();
    const float* prow = P + (((size_t)b * H + h) * T + i) * T;
    // dPd_j = dO.V_j + [band] dO.Ev[rel];  dP_j = dropout'(dPd_j);  Dsum = sum_j dP_j P_j
    float dsum = 0.f;
    for (int j = lane; j < T; j += 64) {
      float s = at_dot(dov, St + (size_t)j * KP, D);
      const int rel = j - i + win;
      if (rel >= 0 && rel <= 2 * win) { const float* e = Es + NW * D + rel * D; float t = 0.f; for (int c = 0; c < D; ++c) t += dov[c] * e[c]; s += t; }
      if (drop_thresh) s = drop_keep(drop_seed, (uint32_t)((b * H + h) * T + i), j, drop_thresh) ? s * drop_scale : 0.f;
      pv[j] = s;
      dsum += s * prow[j];
    }
    dsum = wave_sum(dsum);
    float* dsrow = dS + (((size_t)b * H + h) * T + i) * T;
    for (int j = lane; j < T; j += 64) {
      float ds = prow[j] * (pv[j] - dsum) * inv_sqrt;
      if (j >= len || i >= len) ds = 0.f;                 // masked_fill blocks the gradient
      pv[j] = ds; dsrow[j] = ds;
    }
    __builtin_amdgcn_wave_barrier();
  }
  __syncthreads();
  at_stage(St, k, ld, rbase, h, T, D, KP, tid, nv1);
  __syncthreads();
  for (int ii = w; ii < AT_QT; ii += 4) {
    const int i = i0 + ii;
    if (i >= T) break;
    const float* qv = Qs + ii * 2 * D; const float* dov = qv + D;
    const float* pv = Ps + (size_t)ii * T;
    const float* prow = P + (((size_t)b * H + h) * T + i) * T;
    for (int c = lane; c < D; c += 64) {
      float acc = 0.f;
      for (int j = 0; j < T; ++j) acc += pv[j] * bf2f(St[(size_t)j * KP + c]);
      for (int rel = 0; rel <= 2 * win; ++rel) {
        const int j = i + rel - win;
        if (j >= 0 && j < T) {
          acc += pv[j] * Es[rel * D + c];
          if (pv[j] != 0.f) atomicAdd(Acc + rel * D + c, pv[j] * qv[c]);
          float pd = prow[j];                              // dEv[rel] += dropout(P)[i,j] * dO_i
          if (drop_thresh) pd = drop_keep(drop_seed, (uint32_t)((b * H + h) * T + i), j, drop_thresh) ? pd * drop_scale : 0.f;
          if (pd != 0.f && i < len) atomicAdd(Acc + NW * D + rel * D + c, pd * dov[c]);
        }
      }
      if (i <= nv1) dq[(rbase + i) * lddq + h * D + c] = f2bf(acc);
    }
  }
  __syncthreads();
  for (int i = tid; i < NW * D; i += 256) {
    if (Acc[i] != 0.f) atomicAdd(dEk + i, Acc[i]);
    if (Acc[NW * D + i] != 0.f) atomicAdd(dEv + i, Acc[NW * D + i]);
  }
}

// backward, pass 2 (per key row j): dK_j = sum_i dS[i,j] q_i ;  dV_j = sum_i pd[i,j] dO_i.
__global__ __launch_bounds__(256) void gt_attn_bwd_kv_kernel(
    const bf16_t* __restrict__ q, int ld, const bf16_t* __restrict__ dout, int lddo, const float* __restrict__ P,
    const float* __restrict__ dS, const int32_t* __restrict__ lens, bf16_t* __restrict__ dk, bf16_t* __restrict__ dv, int lddk,
    int T, int Tp, const int32_t* row0, int H, int D, uint32_t drop_thresh, uint32_t drop_seed, float drop_scale, const uint32_t* __restrict__ seed_dev)
{
  if (seed_dev) drop_seed ^= *seed_dev;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int b = blockIdx.z, h = blockIdx.y, j0 = blockIdx.x * AT_QT;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int KP = D + 2;
  bf16_t* St = reinterpret_cast<bf16_t*>(smem);          // [T][KP] q rows, then dO rows
  float* Cs = reinterpret_cast<float*>(St + (size_t)T * KP + (((size_t)T * KP) & 1));   // [AT_QT][2*T] dS column | pd column
  const size_t rbase = (size_t)gt_row_base(row0, b, Tp) + HALO;
  const int nv1 = gt_row_count(row0, b, Tp) - HALO - 1;          // ragged layout: last own row behind rbase (attn_mfma.hip)
  auto RW = [&](int t) { return rbase + (size_t)(t < nv1 ? t : nv1); };
  const int len = lens[b];
  at_stage(St, q, ld, rbase, h, T, D, KP, tid, nv1);
  for (int jj = w; jj < AT_QT; jj += 4) {
    const int j = j0 + jj;
    if (j >= T) break;
    float* dsc = Cs + (size_t)jj * 2 * T; float* pdc = dsc + T;
    for (int i = lane; i < T; i += 64) {
      const size_t o = (((size_t)b * H + h) * T + i) * T + j;
      dsc[i] = dS[o];
      float pd = (i < len) ? P[o] : 0.f;                  // query rows >= len carry no upstream gradient
      if (drop_thresh) pd = drop_keep(drop_seed, (uint32_t)((b * H + h) * T + i), j, drop_thresh) ? pd * drop_scale : 0.f;
      pdc[i] = pd;
    }
  }
  __syncthreads();
  for (int jj = w; jj < AT_QT; jj += 4) {
    const int j = j0 + jj;
    if (j >= T) break;
    const float* dsc = Cs + (size_t)jj * 2 * T;
    for (int c = lane; c < D; c += 64) {
      float ak = 0.f;
      for (int i = 0; i < T; ++i) ak += dsc[i] * bf2f(St[(size_t)i * KP + c]);
      if (j <= nv1) dk[(rbase + j) * lddk + h * D + c] = f2bf(ak);
    }
  }
  __syncthreads();
  at_stage(St, dout, lddo, rbase, h, T, D, KP, tid, nv1);
  __syncthreads();
  for (int jj = w; jj < AT_QT; jj += 4) {
    const int j = j0 + jj;
    if (j >= T) break;
    const float* pdc = Cs + (size_t)jj * 2 * T + T;
    for (int c = lane; c < D; c += 64) {
      float av = 0.f;
      for (int i = 0; i < T; ++i) av += pdc[i] * bf2f(St[(size_t)i * KP + c]);
      if (j <= nv1) dv[(rbase + j) * lddk + h * D + c] = f2bf(av);
    }
  }
}

// ------------------------------------------------------------------ embedding
// rows[b*Tp+HALO+t, :] = emb[ids[b,t], :] * scale * (t < len[b]);  fp32 + bf16 copies; halos zero.
__global__ __launch_bounds__(256) void gt_embedding_fwd_kernel(const int64_t* __restrict__ ids, const float* __restrict__ emb,
                                                               const int32_t* __restrict__ lens, float* __restrict__ out_f32,
                                                               bf16_t* __restrict__ out_bf16, int B, int T, int Tp, int C, float scale,
                                                               const int32_t* __restrict__ row0, int R, int ld)
{
  const int m = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (m >= R) return;
  const int b = gt_row_batch(row0, B, m, Tp), t = m - gt_row_base(row0, b, Tp) - HALO;
  const bool valid = t >= 0 && t < T && t < lens[b];
  const int64_t id = valid ? ids[(size_t)b * T + t] : 0;
  for (int c = lane; c < C; c += 64) {
    const float v = valid ? emb[(size_t)id * C + c] * scale : 0.f;
    if (out_f32) out_f32[(size_t)m * ld + c] = v;
    if (out_bf16) out_bf16[(size_t)m * ld + c] = f2bf(v);
  }
}
__global__ __launch_bounds__(256) void gt_embedding_bwd_kernel(const int64_t* __restrict__ ids, const float* __restrict__ dx,
                                                               const int32_t* __restrict__ lens, float* __restrict__ demb,
                                                               int B, int T, int Tp, int C, float scale,
                                                               const int32_t* __restrict__ row0, int R, int ld)
{
  const int m = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (m >= R) return;
  const int b = gt_row_batch(row0, B, m, Tp), t = m - gt_row_base(row0, b, Tp) - HALO;
  if (t < 0 || t >= T || t >= lens[b]) return;
  const int64_t id = ids[(size_t)b * T + t];
  for (int c = lane; c < C; c += 64) atomicAdd(demb + (size_t)id * C + c, dx[(size_t)m * ld + c] * scale);
}

// ------------------------------------------------------------------ per-utterance vector added to every valid row
// out[m,:] = (x[m,:] + cond[batch(m),:]) * rowmask[m]: the speaker vector of attentions.py:66-67 (Encoder.cond_g) and
// models.py:587-589 (DurationPredictor.cond), which the reference broadcasts over time.  Source fp32 (x) or bf16 (xb);
// fp32 and/or bf16 output; halo / padded rows stay zero.
__global__ __launch_bounds__(256) void gt_rows_add_cond_kernel(const float* __restrict__ x, int ldx, const bf16_t* __restrict__ xb, int ldxb,
                                                               const float* __restrict__ cond, const float* __restrict__ rowmask,
                                                               float* __restrict__ out, int ldo, bf16_t* __restrict__ outb, int ldob,
                                                               int B, int R, int C, int Tp, const int32_t* __restrict__ row0)
{
  const int m = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (m >= R) return;
  const bool valid = rowmask[m] != 0.f;
  const int b = valid ? gt_row_batch(row0, B, m, Tp) : 0;
  for (int c = lane; c < C; c += 64) {
    float v = 0.f;
    if (valid) v = (x ? x[(size_t)m * ldx + c] : bf2f(xb[(size_t)m * ldxb + c])) + cond[(size_t)b * C + c];
    if (out) out[(size_t)m * ldo + c] = v;
    if (outb) outb[(size_t)m * ldob + c] = f2bf(v);
  }
}

// out[b, c] (+)= sum over the rows m of utterance b of y[m, c] * rowmask[m]: the gradient of a per-utterance vector
// (gt_rows_add_cond; the cond input of the WN gate, modules.py:148-156).  One workgroup per (utterance, 64 channels):
// waves stride the rows, lanes own channels, one LDS fold — no atomics.
template <bool F32>
__global__ __launch_bounds__(1024) void gt_rows_utt_sum_kernel(const void* __restrict__ y, int ldy, const float* __restrict__ rowmask,
                                                               float* __restrict__ out, int ldo, int accumulate,
                                                               int B, int C, int Tp, const int32_t* __restrict__ row0)
{
  // latency-bound (a few hundred rows of 128 B per workgroup): 16 waves, 4 independent row loads in flight per lane
  __shared__ float part[16][64];
  const int b = blockIdx.x, c = blockIdx.y * 64 + (threadIdx.x & 63), w = threadIdx.x >> 6;
  const int base = gt_row_base(row0, b, Tp), cnt = gt_row_count(row0, b, Tp);
  auto ld1 = [&](int t) -> float {
    if (t >= cnt) return 0.f;
    const size_t m = (size_t)(base + t);
    const float k = rowmask ? rowmask[m] : 1.f;             // both loads independent; masked rows may hold anything
    const float val = F32 ? static_cast<const float*>(y)[m * ldy + c] : bf2f(static_cast<const bf16_t*>(y)[m * ldy + c]);
    return k != 0.f ? k * val : 0.f;
  };
  float acc = 0.f;
  if (c < C)
    for (int t = w; t < cnt; t += 64) {
      const float a0 = ld1(t), a1 = ld1(t + 16), a2 = ld1(t + 32), a3 = ld1(t + 48);
      acc += (a0 + a1) + (a2 + a3);
    }
  part[w][threadIdx.x & 63] = acc;
  __syncthreads();
  if (w == 0 && c < C) {
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) s += part[i][threadIdx.x];
    float* o = out + (size_t)b * ldo + c;
    *o = accumulate ? *o + s : s;
  }
}

// ragged rows layout: row -> (utterance, frame, valid) tables from the row offsets, one launch (was a dozen host-side ops)
__global__ __launch_bounds__(256) void gt_rows_ctx_fill_kernel(const int32_t* __restrict__ row0, const int32_t* __restrict__ lens,
                                                               int64_t* __restrict__ rowbatch, int32_t* __restrict__ rowframe,
                                                               float* __restrict__ rowmask, int32_t* __restrict__ rowutt, int B, int R)
{
  const int m = blockIdx.x * 256 + threadIdx.x;
  if (m >= R) return;
  const int b = gt_row_batch(row0, B, m, 0);
  const int t = m - row0[b] - HALO;
  rowbatch[m] = b;
  if (rowutt) rowutt[m] = b;
  rowframe[m] = t;
  rowmask[m] = (t >= 0 && t < lens[b]) ? 1.f : 0.f;
}

// One launch for everything a replayed step needs from its batch: the inputs copied into the graph's padded static buffers (rows of
// src_words 4-byte words into rows of dst_words >= src_words, the rest zeroed) and the row tables of up to three ragged contexts rebuilt
// from the row offsets / lengths the host left in pinned memory (read once per workgroup, over PCIe, into LDS).  Was ten launches of
// 4-6 us each between two graph replays: serial time of every step.
__global__ __launch_bounds__(256) void gt_step_inputs_kernel(gt_step_inputs_args a)
{
  __shared__ int32_t geo[2 * GT_STEP_MAX_B + 1];
  const int blk = blockIdx.x;
  for (int j = 0; j < a.n_copy; ++j) {
    const gt_step_copy c = a.copy[j];
    const int nb = (int)(((size_t)c.rows * c.dst_words + 1023) / 1024);
    if (blk >= c.blk0 && blk < c.blk0 + nb) {
      const uint32_t* __restrict__ src = static_cast<const uint32_t*>(c.src);
      uint32_t* __restrict__ dst = static_cast<uint32_t*>(c.dst);
      const size_t total = (size_t)c.rows * c.dst_words;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const size_t w = (size_t)(blk - c.blk0) * 1024 + i * 256 + threadIdx.x;
        if (w < total) {
          const int row = (int)(w / c.dst_words), col = (int)(w - (size_t)row * c.dst_words);
          dst[w] = col < c.src_words ? src[(size_t)row * c.src_words + col] : 0u;
        }
      }
      return;
    }
  }
  for (int j = 0; j < a.n_ctx; ++j) {
    const gt_step_ctx c = a.ctx[j];
    const int nb = (c.R + 255) / 256;
    if (blk >= c.blk0 && blk < c.blk0 + nb) {
      for (int i = threadIdx.x; i < 2 * c.B + 1; i += 256) {
        const int32_t v = c.geo_src[i];
        geo[i] = v;
        if (blk == c.blk0) c.geo_dst[i] = v;            // the device copy later kernels read (row0[B+1] | lengths[B])
      }
      __syncthreads();
      const int m = (blk - c.blk0) * 256 + threadIdx.x;
      if (m >= c.R) return;
      const int b = gt_row_batch(geo, c.B, m, 0);
      const int t = m - geo[b] - HALO;
      c.rowbatch[m] = b;
      if (c.rowutt) c.rowutt[m] = b;
      c.rowframe[m] = t;
      c.rowmask[m] = (t >= 0 && t < geo[c.B + 1 + b]) ? 1.f : 0.f;
      return;
    }
  }
}

// The fills at the head of a training step in one launch: up to GT_ZERO_MAX regions cleared (16-byte aligned, sizes multiples of 16) and
// the dropout seed word advanced (the step's accumulator arena, its pre-zeroed buffer region, the accumulated-gradient slice of the flat
// buffer: three fills and an add before — serial launches in front of both branches of the step).
__global__ __launch_bounds__(256) void gt_step_zero_kernel(gt_step_zero_args a)
{
  if (blockIdx.x == 0 && threadIdx.x == 0 && a.seed_word) *a.seed_word += a.seed_inc;
  size_t w = (size_t)blockIdx.x * 256 + threadIdx.x;               // 16-byte word of the concatenated regions
  for (int j = 0; j < a.n; ++j) {
    const size_t nw = a.bytes[j] >> 4;
    if (w < nw) { reinterpret_cast<uint4*>(a.ptr[j])[w] = make_uint4(0, 0, 0, 0); return; }
    w -= nw;
  }
}

}  // namespace

static int fill_ln(LnArgs& p, const float* a, const void* y, int ldy, const float* gamma, const float* beta, const float* rowmask,
                   float* out_f32, void* out_bf16, int ldo, float* mean, float* rstd, int R, int C, float eps,
                   float p_in, uint32_t seed_in, float p_out, uint32_t seed_out, int relu, const uint32_t* seed_dev)
{
  if ((!a && !y) || !gamma || !beta || !mean || !rstd || R <= 0 || C <= 0 || C > 256) return GT_E_INVAL;
  if (p_in >= 1.f || p_out >= 1.f) return GT_E_INVAL;
  p.a = a; p.y = static_cast<const bf16_t*>(y); p.ldy = ldy; p.gamma = gamma; p.beta = beta; p.rowmask = rowmask;
  p.out_f32 = out_f32; p.out_bf16 = static_cast<bf16_t*>(out_bf16); p.ldo = ldo; p.mean = mean; p.rstd = rstd;
  p.R = R; p.C = C; p.eps = eps; p.relu = relu; p.seed_dev = seed_dev;
  p.din_seed = seed_in; p.dout_seed = seed_out;
  gt_drop_params(p_in, &p.din_thresh, &p.din_scale);
  gt_drop_params(p_out, &p.dout_thresh, &p.dout_scale);
  return GT_OK;
}

extern "C" int gt_layernorm_fwd(const float* a, const void* y, int ldy, const float* gamma, const float* beta, const float* rowmask,
                                float* out_f32, void* out_bf16, int ldo, float* mean, float* rstd, int R, int C, float eps,
                                float p_in, uint32_t seed_in, float p_out, uint32_t seed_out, int relu, const uint32_t* seed_dev, void* stream)
{
  LnArgs p;
  const int rc = fill_ln(p, a, y, ldy, gamma, beta, rowmask, out_f32, out_bf16, ldo, mean, rstd, R, C, eps, p_in, seed_in, p_out, seed_out, relu, seed_dev);
  if (rc) return rc;
  const dim3 grid((R + 3) / 4), block(256);
  if (a && y) hipLaunchKernelGGL((gt_layernorm_fwd_kernel<true, true>), grid, block, 0, GT_ST(stream), p);
  else if (a) hipLaunchKernelGGL((gt_layernorm_fwd_kernel<true, false>), grid, block, 0, GT_ST(stream), p);
  else hipLaunchKernelGGL((gt_layernorm_fwd_kernel<false, true>), grid, block, 0, GT_ST(stream), p);
  GT_RET();
}

// One backward instantiation per (geometry, which of a / y / dout_f32 / dout_bf16 exist); fill_ln and the entries have made sure
// that one of each pair does.
template <int LNB_WAVES, int LNB_ROWS>
static void launch_ln_bwd(const LnBwdArgs& q, void* stream)
{
  const dim3 grid((q.f.R + LNB_WAVES * LNB_ROWS - 1) / (LNB_WAVES * LNB_ROWS)), block(64 * LNB_WAVES);
  const int have = (q.f.a ? 1 : 0) | (q.f.y ? 2 : 0) | (q.dout_f32 ? 4 : 0) | (q.dout_bf16 ? 8 : 0);
  switch (have) {
#define LN_BWD_CASE(F) \
    case F: hipLaunchKernelGGL((gt_layernorm_bwd_kernel<LNB_WAVES, LNB_ROWS, ((F) & 1) != 0, ((F) & 2) != 0, ((F) & 4) != 0, ((F) & 8) != 0>), \
                               grid, block, 0, GT_ST(stream), q); break;
    LN_BWD_CASE(5) LN_BWD_CASE(6) LN_BWD_CASE(7) LN_BWD_CASE(9) LN_BWD_CASE(10) LN_BWD_CASE(11) LN_BWD_CASE(13) LN_BWD_CASE(14) LN_BWD_CASE(15)
#undef LN_BWD_CASE
  }
}

extern "C" int gt_layernorm_bwd(const float* a, const void* y, int ldy, const float* gamma, const float* beta, const float* rowmask,
                                const float* mean, const float* rstd, int R, int C, float eps,
                                float p_in, uint32_t seed_in, float p_out, uint32_t seed_out, int relu, const uint32_t* seed_dev,
                                const float* dout_f32, const void* dout_bf16, int lddo,
                                float* da, void* dy, int lddy, float* dgamma, float* dbeta, void* stream)
{
  LnBwdArgs q;
  const int rc = fill_ln(q.f, a, y, ldy, gamma, beta, rowmask, nullptr, nullptr, 0, const_cast<float*>(mean), const_cast<float*>(rstd),
                         R, C, eps, p_in, seed_in, p_out, seed_out, relu, seed_dev);
  if (rc) return rc;
  if ((!dout_f32 && !dout_bf16) || !dgamma || !dbeta) return GT_E_INVAL;
  q.dout_f32 = dout_f32; q.dout_bf16 = static_cast<const bf16_t*>(dout_bf16); q.lddo = lddo;
  q.da = da; q.dy = static_cast<bf16_t*>(dy); q.lddy = lddy; q.dgamma = dgamma; q.dbeta = dbeta; q.partials = nullptr;
  // geometry: 16 waves x 32 rows per workgroup (the gamma / beta partials are folded in LDS before the atomics) while
  // that still gives >= 64 workgroups; short inputs fall back to 4 waves x 16 rows so the chip is not left idle
  if (R >= 64 * 32) launch_ln_bwd<16, 2>(q, stream);
  else launch_ln_bwd<4, 4>(q, stream);
  GT_RET();
}

// The partials form: 16 rows per workgroup, the workgroup's dgamma | dbeta sums to row blockIdx.x of `partials` — no atomics, whose
// same-address chains grow with the number of workgroups.  4 waves x 4 rows (the 48 row loads of a wave in flight together, 8 KB of
// fold LDS), not 16 waves x 1 row: alone on the machine the 16-wave form is the faster one (5.9 against 8.2 us at 3472 x 192, cold
// operands), but a 1024-thread workgroup with 32 KB cannot share a CU with the decoder's whole-WaveNet workgroups, and inside the
// step the 256-thread form is the one that shortens it (profiles/enc_latency_kernels.txt).
constexpr int LNP_WAVES = 4, LNP_ROWS = 4;
static_assert(LNP_WAVES * LNP_ROWS == 16, "gt_layernorm_bwd_partial_rows");
extern "C" int gt_layernorm_bwd_partial_rows(int R) { return R > 0 ? (R + 15) / 16 : 0; }

extern "C" int gt_layernorm_bwd_partials(const float* a, const void* y, int ldy, const float* gamma, const float* beta, const float* rowmask,
                                         const float* mean, const float* rstd, int R, int C, float eps,
                                         float p_in, uint32_t seed_in, float p_out, uint32_t seed_out, int relu, const uint32_t* seed_dev,
                                         const float* dout_f32, const void* dout_bf16, int lddo,
                                         float* da, void* dy, int lddy, float* partials, void* stream)
{
  LnBwdArgs q;
  const int rc = fill_ln(q.f, a, y, ldy, gamma, beta, rowmask, nullptr, nullptr, 0, const_cast<float*>(mean), const_cast<float*>(rstd),
                         R, C, eps, p_in, seed_in, p_out, seed_out, relu, seed_dev);
  if (rc) return rc;
  if ((!dout_f32 && !dout_bf16) || !partials) return GT_E_INVAL;
  q.dout_f32 = dout_f32; q.dout_bf16 = static_cast<const bf16_t*>(dout_bf16); q.lddo = lddo;
  q.da = da; q.dy = static_cast<bf16_t*>(dy); q.lddy = lddy; q.dgamma = nullptr; q.dbeta = nullptr; q.partials = partials;
  launch_ln_bwd<LNP_WAVES, LNP_ROWS>(q, stream);
  GT_RET();
}

extern "C" int gt_param_partials_reduce(const gt_partials_args* args, void* stream)
{
  if (!args || args->n_jobs <= 0 || args->n_jobs > GT_PARTIALS_MAX) return GT_E_INVAL;
  int maxw = 0;
  for (int j = 0; j < args->n_jobs; ++j) {
    const gt_partials_job& b = args->job[j];
    if (!b.partials || !b.dst_a || b.n_rows <= 0 || b.Ca <= 0 || b.Cb < 0 || (b.Cb > 0 && !b.dst_b)) return GT_E_INVAL;
    maxw = b.Ca + b.Cb > maxw ? b.Ca + b.Cb : maxw;
  }
  hipLaunchKernelGGL(gt_param_partials_reduce_kernel, dim3((maxw + 63) / 64, args->n_jobs, PARTIALS_ZS), dim3(256), 0, GT_ST(stream), *args);
  GT_RET();
}

static size_t attn_lds(int T, int D, int win, size_t extra_floats)
{
  size_t halfs = (size_t)T * (D + 2); halfs += halfs & 1;     // keep the float area 4-byte aligned
  return halfs * 2 + (size_t)2 * (2 * win + 1) * D * 4 + extra_floats * 4;
}

// What the four attention entries share of a gt_attn_call; each adds its own direction's fields.  After the entry's checks: p < 1.
static gt_attn_call attn_call(const void* q, const void* k, const void* v, int ld, const float* Ek, const float* Ev, const int32_t* lens,
                              int B, int T, int Tp, const int32_t* row0, int H, int D, int win, float drop_p, uint32_t drop_seed,
                              const uint32_t* seed_dev, void* stream)
{
  gt_attn_call c = {};
  c.q = gt_bf16(q); c.k = gt_bf16(k); c.v = gt_bf16(v); c.ld = ld; c.Ek = Ek; c.Ev = Ev; c.lens = lens;
  c.B = B; c.T = T; c.Tp = Tp; c.row0 = row0; c.H = H; c.D = D; c.win = win;
  gt_drop_params(drop_p, &c.th, &c.sc);
  c.sd = drop_seed; c.seed_dev = seed_dev; c.stream = GT_ST(stream);
  return c;
}

extern "C" int gt_attn_fwd(const void* q, const void* k, const void* v, int ld, const float* Ek, const float* Ev,
                           const int32_t* lens, void* out, int ldo, float* P, int B, int T, int Tp, const int32_t* row0, int H, int D, int win,
                           float drop_p, uint32_t drop_seed, const uint32_t* seed_dev, void* stream)
{
  if (!q || !k || !v || !Ek || !Ev || !lens || !out || B <= 0 || T <= 0 || H <= 0) return GT_E_INVAL;
  const gt_attn_path path = gt_attn_route(T, D, win);
  if (D > AT_MAXD || (D & 1) || win < 0 || drop_p >= 1.f || path == GT_ATTN_NONE) return GT_E_UNSUPPORTED;
  gt_attn_call c = attn_call(q, k, v, ld, Ek, Ev, lens, B, T, Tp, row0, H, D, win, drop_p, drop_seed, seed_dev, stream);
  c.out = gt_bf16(out); c.ldo = ldo; c.P = P;
  const bool mfma_layout = gt_attn_mfma_layout(c);
  if (!P) {                                        // a forward that stores no P: the key-tiled kernel, and nothing else
    if (path != GT_ATTN_LONG_P) return GT_E_INVAL;
    return mfma_layout ? gt_attn_fwd_long_impl(c, GT_ATTN_LONG_NOP) : GT_E_ALIGN;
  }
  switch (path) {
    case GT_ATTN_FUSED160: case GT_ATTN_MFMA256: case GT_ATTN_MFMA384:
      if (mfma_layout) return gt_attn_fwd_mfma_impl(c, path);
      break;                                       // a layout the MFMA kernels do not take (row pitch, operand alignment): the generic kernel runs
    case GT_ATTN_LONG_P:
      if (mfma_layout) return gt_attn_fwd_long_impl(c, path);
      break;                                       // likewise; the generic LDS holds a forward to T = 597 (the backward to 505): GT_E_UNSUPPORTED past it
    default: break;
  }
  const size_t lds = attn_lds(T, D, win, (size_t)4 * D + (size_t)AT_QT * T);
  if (lds > 160 * 1024) return GT_E_UNSUPPORTED;
  if (const int rc = gt_allow_lds<&gt_attn_fwd_kernel>(160 * 1024)) return rc;
  hipLaunchKernelGGL(gt_attn_fwd_kernel, dim3((T + AT_QT - 1) / AT_QT, H, B), dim3(256), lds, c.stream,
                     c.q, c.k, c.v, c.ld, c.Ek, c.Ev, c.lens, c.out, c.ldo, c.P, c.T, c.Tp, c.row0, c.H, c.D, c.win, c.th, c.sd, c.sc, c.seed_dev);
  GT_RET();
}

// Room for either workspace format: the generic kernels' fp32 dS [B, H, T, T] or the MFMA families' bf16 pair (which of the two a
// call writes depends on D, win and the layout, which this function is not told).
extern "C" size_t gt_attn_bwd_workspace_bytes(int B, int T, int H)
{
  if (B <= 0 || T <= 0 || H <= 0) return 0;
  const size_t generic = (size_t)B * H * T * T * sizeof(float);
  const size_t mfma = gt_attn_bwd_mfma_ws_bytes(B, T, H);
  return (generic > mfma ? generic : mfma) + 256;
}

extern "C" int gt_attn_bwd(const void* q, const void* k, const void* v, int ld, const float* Ek, const float* Ev,
                           const int32_t* lens, const void* dout, int lddo, const float* P, void* workspace, size_t workspace_bytes,
                           void* dq, void* dk, void* dv, int lddq, float* dEk, float* dEv,
                           int B, int T, int Tp, const int32_t* row0, int H, int D, int win, float drop_p, uint32_t drop_seed, const uint32_t* seed_dev, void* stream)
{
  if (!q || !k || !v || !Ek || !Ev || !lens || !dout || !P || !workspace || !dq || !dk || !dv || !dEk || !dEv) return GT_E_INVAL;
  const gt_attn_path path = gt_attn_route(T, D, win);
  if (D > AT_MAXD || (D & 1) || win < 0 || drop_p >= 1.f || path == GT_ATTN_NONE) return GT_E_UNSUPPORTED;
  if (workspace_bytes < gt_attn_bwd_workspace_bytes(B, T, H)) return GT_E_INVAL;
  gt_attn_call c = attn_call(q, k, v, ld, Ek, Ev, lens, B, T, Tp, row0, H, D, win, drop_p, drop_seed, seed_dev, stream);
  c.dout = gt_bf16(dout); c.lddo = lddo; c.P = const_cast<float*>(P);      // only read from here on
  c.ws = workspace; c.ws_bytes = workspace_bytes;
  c.dq = gt_bf16(dq); c.dk = gt_bf16(dk); c.dv = gt_bf16(dv); c.lddq = lddq; c.dEk = dEk; c.dEv = dEv;
  const bool mfma_layout = gt_attn_mfma_layout(c) && workspace_bytes >= gt_attn_bwd_mfma_ws_bytes(B, T, H);
  switch (path) {                                  // the forward's two hand-ons (gt_attn_fwd); a LONG_P call handed on is refused below
    case GT_ATTN_FUSED160: case GT_ATTN_MFMA256: case GT_ATTN_MFMA384:
      if (mfma_layout) return gt_attn_bwd_mfma_impl(c, path);
      break;
    case GT_ATTN_LONG_P:
      if (mfma_layout) return gt_attn_bwd_long_impl(c, path);
      break;
    default: break;
  }
  const size_t lds1 = attn_lds(T, D, win, (size_t)2 * (2 * win + 1) * D + (size_t)AT_QT * 2 * D + (size_t)AT_QT * T);
  size_t halfs2 = (size_t)T * (D + 2); halfs2 += halfs2 & 1;
  const size_t lds2 = halfs2 * 2 + (size_t)AT_QT * 2 * T * 4;
  if (lds1 > 160 * 1024 || lds2 > 160 * 1024) return GT_E_UNSUPPORTED;
  if (const int rc = gt_allow_lds<&gt_attn_bwd_q_kernel>(160 * 1024)) return rc;
  if (const int rc = gt_allow_lds<&gt_attn_bwd_kv_kernel>(160 * 1024)) return rc;
  float* dS_ws = static_cast<float*>(workspace);
  const dim3 grid((T + AT_QT - 1) / AT_QT, H, B);
  hipLaunchKernelGGL(gt_attn_bwd_q_kernel, grid, dim3(256), lds1, c.stream,
                     c.q, c.k, c.v, c.ld, c.Ek, c.Ev, c.lens, c.dout, c.lddo, c.P, dS_ws, c.dq, c.lddq, c.dEk, c.dEv,
                     c.T, c.Tp, c.row0, c.H, c.D, c.win, c.th, c.sd, c.sc, c.seed_dev);
  hipLaunchKernelGGL(gt_attn_bwd_kv_kernel, grid, dim3(256), lds2, c.stream,
                     c.q, c.ld, c.dout, c.lddo, c.P, dS_ws, c.lens, c.dk, c.dv, c.lddq, c.T, c.Tp, c.row0, c.H, c.D, c.th, c.sd, c.sc, c.seed_dev);
  GT_RET();
}

// The P-free pair: the key-tiled family only, no fallback.  Checks in the header's order: NULL pointers, the token limit and the
// shape, the workspace size, alignment.
extern "C" size_t gt_attn_stats_bytes(int B, int T, int H)
{
  if (B <= 0 || T <= 0 || H <= 0) return 0;
  return (size_t)B * H * T * 2 * sizeof(float);
}

extern "C" size_t gt_attn_bwd_stats_workspace_bytes(int B, int T, int H)
{
  if (B <= 0 || T <= 0 || H <= 0) return 0;
  return gt_attn_long_stats_ws_bytes(B, T, H);
}

extern "C" int gt_attn_fwd_stats(const void* q, const void* k, const void* v, int ld, const float* Ek, const float* Ev,
                                 const int32_t* lens, void* out, int ldo, float* stats, int B, int T, int Tp, const int32_t* row0, int H, int D,
                                 int win, float drop_p, uint32_t drop_seed, const uint32_t* seed_dev, void* stream)
{
  if (!q || !k || !v || !Ek || !Ev || !lens || !out || !stats || B <= 0 || T <= 0 || H <= 0) return GT_E_INVAL;
  if (gt_attn_route(T, D, win) != GT_ATTN_LONG_P || drop_p >= 1.f) return GT_E_UNSUPPORTED;
  gt_attn_call c = attn_call(q, k, v, ld, Ek, Ev, lens, B, T, Tp, row0, H, D, win, drop_p, drop_seed, seed_dev, stream);
  c.out = gt_bf16(out); c.ldo = ldo; c.stats = stats;
  return gt_attn_mfma_layout(c) ? gt_attn_fwd_long_impl(c, GT_ATTN_LONG_STATS) : GT_E_ALIGN;
}

extern "C" int gt_attn_bwd_stats(const void* q, const void* k, const void* v, int ld, const float* Ek, const float* Ev,
                                 const int32_t* lens, const void* dout, int lddo, const float* stats, void* workspace, size_t workspace_bytes,
                                 void* dq, void* dk, void* dv, int lddq, float* dEk, float* dEv,
                                 int B, int T, int Tp, const int32_t* row0, int H, int D, int win, float drop_p, uint32_t drop_seed,
                                 const uint32_t* seed_dev, void* stream)
{
  if (!q || !k || !v || !Ek || !Ev || !lens || !dout || !stats || !workspace || !dq || !dk || !dv || !dEk || !dEv || B <= 0 || T <= 0 || H <= 0)
    return GT_E_INVAL;
  if (gt_attn_route(T, D, win) != GT_ATTN_LONG_P || drop_p >= 1.f) return GT_E_UNSUPPORTED;
  if (workspace_bytes < gt_attn_bwd_stats_workspace_bytes(B, T, H)) return GT_E_INVAL;
  gt_attn_call c = attn_call(q, k, v, ld, Ek, Ev, lens, B, T, Tp, row0, H, D, win, drop_p, drop_seed, seed_dev, stream);
  c.dout = gt_bf16(dout); c.lddo = lddo; c.stats = const_cast<float*>(stats);   // only read from here on
  c.ws = workspace; c.ws_bytes = workspace_bytes;
  c.dq = gt_bf16(dq); c.dk = gt_bf16(dk); c.dv = gt_bf16(dv); c.lddq = lddq; c.dEk = dEk; c.dEv = dEv;
  return gt_attn_mfma_layout(c) ? gt_attn_bwd_long_impl(c, GT_ATTN_LONG_STATS) : GT_E_ALIGN;
}

extern "C" int gt_embedding_fwd(const int64_t* ids, const float* emb, const int32_t* lens, float* out_f32, void* out_bf16,
                                int B, int T, int Tp, const int32_t* row0, int R, int C, int ld, float scale, void* stream)
{
  if (!ids || !emb || !lens || (!out_f32 && !out_bf16) || B <= 0 || T <= 0 || C <= 0 || R <= 0 || ld < C) return GT_E_INVAL;
  if (!row0 && R != B * Tp) return GT_E_INVAL;
  hipLaunchKernelGGL(gt_embedding_fwd_kernel, dim3((R + 3) / 4), dim3(256), 0, GT_ST(stream), ids, emb, lens, out_f32,
                     static_cast<bf16_t*>(out_bf16), B, T, Tp, C, scale, row0, R, ld);
  GT_RET();
}
extern "C" int gt_rows_add_cond(const float* x, int ldx, const void* xb, int ldxb, const float* cond, const float* rowmask,
                               float* out, int ldo, void* outb, int ldob, int B, int R, int C, int Tp, const int32_t* row0, void* stream)
{
  if ((!x && !xb) || !cond || !rowmask || (!out && !outb) || B <= 0 || R <= 0 || C <= 0) return GT_E_INVAL;
  if (!row0 && R != B * Tp) return GT_E_INVAL;
  hipLaunchKernelGGL(gt_rows_add_cond_kernel, dim3((R + 3) / 4), dim3(256), 0, GT_ST(stream), x, ldx, static_cast<const bf16_t*>(xb), ldxb,
                     cond, rowmask, out, ldo, static_cast<bf16_t*>(outb), ldob, B, R, C, Tp, row0);
  GT_RET();
}
extern "C" int gt_rows_utt_sum(const void* y, int ldy, int is_f32, const float* rowmask, float* out, int ldo, int accumulate,
                              int B, int R, int C, int Tp, const int32_t* row0, void* stream)
{
  if (!y || !out || B <= 0 || R <= 0 || C <= 0 || ldy < C || ldo < C) return GT_E_INVAL;
  if (!row0 && R != B * Tp) return GT_E_INVAL;
  const dim3 grid(B, (C + 63) / 64);
  if (is_f32) hipLaunchKernelGGL(gt_rows_utt_sum_kernel<true>, grid, dim3(1024), 0, GT_ST(stream), y, ldy, rowmask, out, ldo, accumulate, B, C, Tp, row0);
  else        hipLaunchKernelGGL(gt_rows_utt_sum_kernel<false>, grid, dim3(1024), 0, GT_ST(stream), y, ldy, rowmask, out, ldo, accumulate, B, C, Tp, row0);
  GT_RET();
}
extern "C" int gt_rows_ctx_fill(const int32_t* row0, const int32_t* lens, int64_t* rowbatch, int32_t* rowframe, float* rowmask, int32_t* rowutt,
                               int B, int R, void* stream)
{
  if (!row0 || !lens || !rowbatch || !rowframe || !rowmask || B <= 0 || R <= 0) return GT_E_INVAL;
  hipLaunchKernelGGL(gt_rows_ctx_fill_kernel, dim3((R + 255) / 256), dim3(256), 0, GT_ST(stream), row0, lens, rowbatch, rowframe, rowmask, rowutt, B, R);
  GT_RET();
}
extern "C" int gt_step_zero(const gt_step_zero_args* args, void* stream)
{
  if (!args || args->n < 0 || args->n > GT_ZERO_MAX) return GT_E_INVAL;
  size_t words = 0;
  for (int j = 0; j < args->n; ++j) {
    if (!args->ptr[j] || (args->bytes[j] & 15) || ((uintptr_t)args->ptr[j] & 15)) return GT_E_ALIGN;
    words += args->bytes[j] >> 4;
  }
  if (!words && !args->seed_word) return GT_OK;
  if (words > ((size_t)1 << 31)) return GT_E_UNSUPPORTED;
  hipLaunchKernelGGL(gt_step_zero_kernel, dim3((unsigned)((words + 255) / 256) + (words ? 0 : 1)), dim3(256), 0, GT_ST(stream), *args);
  GT_RET();
}
extern "C" int gt_step_inputs(const gt_step_inputs_args* args, void* stream)
{
  if (!args || args->n_copy < 0 || args->n_copy > GT_STEP_MAX_COPIES || args->n_ctx < 0 || args->n_ctx > GT_STEP_MAX_CTX) return GT_E_INVAL;
  gt_step_inputs_args a = *args;
  int blocks = 0;
  for (int j = 0; j < a.n_copy; ++j) {
    gt_step_copy& c = a.copy[j];
    if (!c.src || !c.dst || c.rows <= 0 || c.src_words < 0 || c.dst_words < c.src_words || c.dst_words <= 0) return GT_E_INVAL;
    if (((uintptr_t)c.src | (uintptr_t)c.dst) & 3) return GT_E_ALIGN;
    c.blk0 = blocks;
    blocks += (int)(((size_t)c.rows * c.dst_words + 1023) / 1024);
  }
  for (int j = 0; j < a.n_ctx; ++j) {
    gt_step_ctx& c = a.ctx[j];
    if (!c.geo_src || !c.geo_dst || !c.rowbatch || !c.rowframe || !c.rowmask || c.B <= 0 || c.B > GT_STEP_MAX_B || c.R <= 0) return GT_E_INVAL;
    c.blk0 = blocks;
    blocks += (c.R + 255) / 256;
  }
  if (!blocks) return GT_OK;
  hipLaunchKernelGGL(gt_step_inputs_kernel, dim3(blocks), dim3(256), 0, GT_ST(stream), a);
  GT_RET();
}
extern "C" int gt_embedding_bwd(const int64_t* ids, const float* dx, const int32_t* lens, float* demb,
                                int B, int T, int Tp, const int32_t* row0, int R, int C, int ld, float scale, void* stream)
{
  if (!ids || !dx || !lens || !demb || B <= 0 || T <= 0 || C <= 0 || R <= 0 || ld < C) return GT_E_INVAL;
  if (!row0 && R != B * Tp) return GT_E_INVAL;
  hipLaunchKernelGGL(gt_embedding_bwd_kernel, dim3((R + 3) / 4), dim3(256), 0, GT_ST(stream), ids, dx, lens, demb, B, T, Tp, C, scale, row0, R, ld);
  GT_RET();
}

__global__ void gt_mark_kernel(unsigned long long* slot) { *slot = (unsigned long long)wall_clock64(); }

extern "C" int gt_mark(unsigned long long* slot, void* stream)
{
  if (!slot) return -1;
  hipLaunchKernelGGL(gt_mark_kernel, dim3(1), dim3(1), 0, GT_ST(stream), slot);
  return hipGetLastError() == hipSuccess ? 0 : -2;
}
