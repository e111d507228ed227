// Everything between the decoder and the loss, fp32 throughout, on [B, C, T] tensors (see glowtts_hip.h):
//   logp lattice                                    models.py:1076-1082
//   prior expansion (gather) and its backward       models.py:1118-1119
//   mle loss: partial sums, scalar tail, backward   commons.py:28-33
//   length mask                                     commons.sequence_mask
//   duration loss and its backward                  models.py:1089-1092
//   the alignment -> loss chain in three launches   gt_align_loss_fwd / _finish / _bwd
// The fused chain and the unfused entries are both live (train.Trainer takes either from one step to the next) and must give the
// same numbers bit for bit.  THE RULE: a step's arithmetic lives in ONE __device__ helper below; the fused and the unfused kernel
// that call it differ only in their index maps and in what they store.  An edit to a helper changes both chains together; an
// expression copied out of a helper into a kernel breaks the rule (tools/align_loss_equality.py prints what to compare).
#include <stdlib.h>
#include "common.h"
#include "../../include/glowtts_hip.h"
#include "internal.h"

namespace {

// ------------------------------------------------------------------ logp lattice (models.py:1076-1082)
// logp[b,i,j] = sum_d(-0.5 log 2pi - s_id) + sum_d e^{-2 s_id} (-0.5 z_jd^2) + sum_d m_id e^{-2 s_id} z_jd
//               + sum_d -0.5 m_id^2 e^{-2 s_id}
// x_m, x_logs: [B, C, T_x] fp32; z: [B, C, T_y] fp32.  exact-fp32 MFMA (v_mfma_f32_32x32x2_f32): one wave
// per 32x32 lattice tile, K = 2C interleaved as (e^{-2s}, -0.5 z^2) and (m e^{-2s}, z) pairs.
__global__ __launch_bounds__(256) void gt_logp_kernel(const float* __restrict__ xm, const float* __restrict__ xlogs,
                                                      const float* __restrict__ z, float* __restrict__ logp,
                                                      int B, int C, int Tx, int Ty)
{
  const int b = blockIdx.z;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int i0 = blockIdx.y * 32, j0 = (blockIdx.x * 4 + w) * 32;
  if (j0 >= Ty) return;
  const int r = lane & 31, kh = lane >> 5;
  const int i = i0 + r, j = j0 + r;
  const float* xmb = xm + (size_t)b * C * Tx;
  const float* xsb = xlogs ? xlogs + (size_t)b * C * Tx : nullptr;
  const float* zb = z + (size_t)b * C * Ty;
  f32x16_t acc;
#pragma unroll
  for (int e = 0; e < 16; ++e) acc[e] = 0.f;
  float rowc = 0.f;                                       // logp1 + logp4 of row i (lanes kh==0 and kh==1 split d)
  // 8 k-pairs per trip with their loads issued together: one trip = one memory round trip for 16 MFMAs (a load / MFMA pair per
  // trip left the wave waiting on 80 dependent round trips: 33 us for a lattice whose MFMAs take 4)
  constexpr int U = 8;
  for (int d0 = 0; d0 < C; d0 += 2 * U) {
    float m[U], sv[U], zz[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int dd = d0 + 2 * u + kh;                     // this lane's k index
      m[u] = 0.f; sv[u] = 0.f; zz[u] = 0.f;
      if (dd < C) {
        if (i < Tx) { m[u] = xmb[(size_t)dd * Tx + i]; if (xsb) sv[u] = xsb[(size_t)dd * Tx + i]; }
        if (j < Ty) zz[u] = zb[(size_t)dd * Ty + j];
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const bool in = d0 + 2 * u + kh < C;
      const float e2 = xsb ? __expf(-2.0f * sv[u]) : 1.0f;
      if (in) rowc += -0.9189385332046727f - sv[u] - 0.5f * m[u] * m[u] * e2;
      if (d0 + 2 * u < C) {                                 // wave-uniform (C is even): whole k pairs only
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(in ? e2 : 0.f, -0.5f * zz[u] * zz[u], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(in ? m[u] * e2 : 0.f, zz[u], acc, 0, 0, 0);
      }
    }
  }
  rowc += __shfl_xor(rowc, 32);                           // both k halves -> full sum over d, indexed by r = row i0+r
  // C/D layout: col = lane&31 (= j), row = (e&3) + 8*(e>>2) + 4*kh (= i offset)
#pragma unroll
  for (int e = 0; e < 16; ++e) {
    const int ri = (e & 3) + 8 * (e >> 2) + 4 * kh;
    const float rc = __shfl(rowc, ri);                    // lane ri holds row i0+ri's constant
    if (i0 + ri < Tx && j < Ty) logp[((size_t)b * Tx + i0 + ri) * Ty + j] = acc[e] + rc;
  }
}

// ------------------------------------------------------------------ the steps, one body each
// Duration loss of the deterministic predictor (models.py:1089-1092): l[b] = sum_t (logw[b,t] - log(w[b,t] + 1e-8) mask)^2 / sum(mask);
// backward: d logw[b,t] = g * 2 (logw - logw_) / sum(mask) on valid tokens (w comes from MAS: no gradient).  One wave per utterance.
__device__ __forceinline__ float dur_tot(const int32_t* __restrict__ len, int B, int lane)
{
  float tot = 0.f;
  for (int i = lane; i < B; i += 64) tot += (float)len[i];
  return wave_sum(tot);
}
__device__ __forceinline__ float dur_diff(const float* __restrict__ logw, const float* __restrict__ w, int b, int Tx, int t, int n)
{
  const float lw = logw[(size_t)b * Tx + t];
  const float ref = t < n ? __logf(w[(size_t)b * Tx + t] + 1e-8f) : 0.f;
  return lw - ref;
}
// l[b], on every lane (the caller stores lane 0's)
__device__ __forceinline__ float dur_loss_fwd_wave(const float* __restrict__ logw, const float* __restrict__ w,
                                                   const int32_t* __restrict__ len, int b, int B, int Tx, int lane)
{
  const float tot = dur_tot(len, B, lane);
  float a = 0.f;
  const int n = len[b];
  for (int t = lane; t < Tx; t += 64) {
    const float d = dur_diff(logw, w, b, Tx, t, n);
    a += d * d;
  }
  a = wave_sum(a);
  return a / tot;
}
// g: the gradient of l[b] (g[b] unfused, *gscale in the chain)
__device__ __forceinline__ void dur_loss_bwd_wave(const float* __restrict__ logw, const float* __restrict__ w,
                                                  const int32_t* __restrict__ len, float g, int b, int B, int Tx, int lane,
                                                  float* __restrict__ dlogw)
{
  const float tot = dur_tot(len, B, lane);
  const int n = len[b];
  const float gb = 2.0f * g / tot;
  for (int t = lane; t < Tx; t += 64) dlogw[(size_t)b * Tx + t] = gb * dur_diff(logw, w, b, Tx, t, n);
}

// mle loss partial sums (commons.py:28-33) of four neighbours: a0 += sum logs,  a1 += sum exp(-2 logs) (z-m)^2
__device__ __forceinline__ void mle_quad(const float4 zz, const float4 mm, const float4 ll, float& a0, float& a1)
{
  const float d0 = zz.x - mm.x, d1 = zz.y - mm.y, d2 = zz.z - mm.z, d3 = zz.w - mm.w;
  a0 += ll.x + ll.y + ll.z + ll.w;
  a1 += __expf(-2.0f * ll.x) * d0 * d0 + __expf(-2.0f * ll.y) * d1 * d1 + __expf(-2.0f * ll.z) * d2 * d2 + __expf(-2.0f * ll.w) * d3 * d3;
}
// ... and a 256-thread workgroup's sums of them: one partial pair per workgroup, the finish kernel adds the GT_MLE_PARTS of them
// (512 workgroups x 2 same-address atomics and four dependent load rounds per thread before: 16.7 us)
__device__ __forceinline__ void mle_partial_store(float a0, float a1, float* __restrict__ acc)
{
  __shared__ float red[2][4];
  a0 = wave_sum(a0); a1 = wave_sum(a1);
  if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = a0; red[1][threadIdx.x >> 6] = a1; }
  __syncthreads();
  if (threadIdx.x == 0) {
    acc[2 * blockIdx.x] = red[0][0] + red[0][1] + red[0][2] + red[0][3];
    acc[2 * blockIdx.x + 1] = red[1][0] + red[1][1] + red[1][2] + red[1][3];
  }
}
// the gradient of one element: v = dz = g * exp(-2 logs) (z-m) (dm = -v), gl = dlogs = g * (1 - exp(-2 logs)(z-m)^2)
__device__ __forceinline__ void mle_grad(float g, float l, float z, float m, float& v, float& gl)
{
  const float e = __expf(-2.0f * l), d = z - m;
  v = g * e * d;
  gl = g * (1.0f - e * d * d);
}

// The backward of the gather, dxm[b,c,i] = sum of dzm[b,c,j] over the frames j aligned to token i, for NV values per frame at once.
// One wave per (b, c) row walks the frames 64 at a time (coalesced), sums each run of equal tokens with a segmented wave scan (the MAS
// path is monotone: runs are contiguous) and the run's last lane adds it to the row's token accumulators in LDS — fixed order, no
// atomics.  load(j, v) gives frame j's NV values (and stores what else the caller makes of them); f2t is the utterance's row, a[k]
// Tx floats of LDS, out[k] the row of the k-th result.  (The first form — a thread per (b, c, token) looping over its frames — took
// 74 us on the step's critical path: autograd runs it before the decoder's backward.)
template <int NV> struct SegRows { float* p[NV]; };
template <int NV, typename Load>
__device__ __forceinline__ void segmented_walk(Load load, const int32_t* __restrict__ f2t, int Ty, int Tx, int lane, SegRows<NV> a, SegRows<NV> out)
{
  // the loops over k have NV = 1 or 2 trips: unrolled, v and u stay registers (the build refuses scratch)
  for (int i = lane; i < Tx; i += 64)
    for (int k = 0; k < NV; ++k) a.p[k][i] = 0.f;
  for (int j0 = 0; j0 < Ty; j0 += 64) {
    const int j = j0 + lane;
    int t = -1; float v[NV] = {};
    if (j < Ty) { t = f2t[j]; load(j, v); }
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      float u[NV];
      for (int k = 0; k < NV; ++k) u[k] = __shfl_up(v[k], off);
      const int tt = __shfl_up(t, off);
      if (lane >= off && tt == t)
        for (int k = 0; k < NV; ++k) v[k] += u[k];
    }
    const int tn = __shfl_down(t, 1);
    if (t >= 0 && t < Tx && (lane == 63 || tn != t))        // a run that crosses the chunk boundary continues in the next chunk
      for (int k = 0; k < NV; ++k) a.p[k][t] += v[k];
  }
  for (int i = lane; i < Tx; i += 64)
    for (int k = 0; k < NV; ++k) out.p[k][i] = a.p[k][i];
}

// ------------------------------------------------------------------ prior expansion + mle loss, a launch per step
// z_m[b,c,j] = x_m[b,c,tok[b,j]] (0 where tok < 0)  — models.py:1118 as a gather.
__global__ __launch_bounds__(256) void gt_prior_expand_kernel(const float* __restrict__ xm, const int32_t* __restrict__ tok,
                                                              float* __restrict__ zm, int B, int C, int Tx, int Ty)
{
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= B * C * Ty) return;
  const int j = idx % Ty, bc = idx / Ty, b = bc / C;
  const int t = tok[(size_t)b * Ty + j];
  zm[idx] = t >= 0 ? xm[(size_t)bc * Tx + t] : 0.f;
}
// Its backward: segmented_walk over dzm.  Tx <= 512: four waves (rows) per workgroup, acc[4][512].  LONG, where that ends: one wave
// per workgroup and (b, c) row, the row's Tx accumulators in dynamic LDS.  Waves are independent: no workgroup barrier.
template <bool LONG>
__global__ __launch_bounds__(LONG ? 64 : 256) void gt_prior_expand_bwd_kernel(const float* __restrict__ dzm, const int32_t* __restrict__ f2t,
                                                                              float* __restrict__ dxm, int B, int C, int Tx, int Ty)
{
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int bc = LONG ? blockIdx.x : blockIdx.x * 4 + wave;
  if (bc >= B * C) return;
  float* a;
  if constexpr (LONG) { extern __shared__ float acc_long[]; a = acc_long; }
  else { __shared__ float acc[4][512]; a = acc[wave]; }
  const float* row = dzm + (size_t)bc * Ty;
  segmented_walk<1>([&](int j, float (&v)[1]) { v[0] = row[j]; }, f2t + (size_t)(bc / C) * Ty, Ty, Tx, lane,
                    SegRows<1>{{a}}, SegRows<1>{{dxm + (size_t)bc * Tx}});
}
// mle loss partial sums over [B,C,T] tensors flattened to n elements (logs may be NULL = 0)
__global__ __launch_bounds__(256) void gt_mle_sums_kernel(const float* __restrict__ z, const float* __restrict__ m,
                                                          const float* __restrict__ logs, float* __restrict__ acc, size_t n)
{
  float a0 = 0.f, a1 = 0.f;
  const size_t n4 = n >> 2;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (size_t)gridDim.x * 256) {
    const float4 zz = reinterpret_cast<const float4*>(z)[i], mm = reinterpret_cast<const float4*>(m)[i];
    float4 ll = make_float4(0.f, 0.f, 0.f, 0.f);
    if (logs) ll = reinterpret_cast<const float4*>(logs)[i];
    mle_quad(zz, mm, ll, a0, a1);
  }
  if (blockIdx.x == 0) {                                    // the n % 4 elements past the last quad (the chain has none: T_y % 4 == 0)
    for (size_t i = (n4 << 2) + threadIdx.x; i < n; i += 256) {
      const float l = logs ? logs[i] : 0.f, d = z[i] - m[i];
      a0 += l; a1 += __expf(-2.0f * l) * d * d;
    }
  }
  mle_partial_store(a0, a1, acc);
}
// dz = v, dm = -v, dlogs = gl of mle_grad with g = *gscale (/ *gdenom)
__global__ __launch_bounds__(256) void gt_mle_bwd_kernel(const float* __restrict__ z, const float* __restrict__ m,
                                                         const float* __restrict__ logs, const float* __restrict__ gscale,
                                                         float* __restrict__ dz, float* __restrict__ dm, float* __restrict__ dlogs, size_t n,
                                                         const float* __restrict__ gdenom, float* __restrict__ dlogdet, int B)
{
  const float g = gdenom ? *gscale / *gdenom : *gscale;
  if (dlogdet && blockIdx.x == 0)
    for (int b = threadIdx.x; b < B; b += 256) dlogdet[b] = -g;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
    float v, gl;
    mle_grad(g, logs ? logs[i] : 0.f, z[i], m[i], v, gl);
    if (dz) dz[i] = v;
    if (dm) dm[i] = -v;
    if (dlogs) dlogs[i] = gl;
  }
}

// commons.sequence_mask as floats: mask[b, t] = t < len[b]  (lengths int32 or int64)
__global__ __launch_bounds__(256) void gt_length_mask_kernel(const void* __restrict__ len, int is64, float* __restrict__ mask, int B, int T)
{
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= B * T) return;
  const int b = idx / T, t = idx - b * T;
  const long long n = is64 ? static_cast<const long long*>(len)[b] : (long long)static_cast<const int32_t*>(len)[b];
  mask[idx] = t < n ? 1.f : 0.f;
}

__global__ void gt_duration_loss_fwd_kernel(const float* __restrict__ logw, const float* __restrict__ w, const int32_t* __restrict__ len,
                                            int B, int Tx, float* __restrict__ out)
{
  const int b = blockIdx.x, lane = threadIdx.x;
  const float l = dur_loss_fwd_wave(logw, w, len, b, B, Tx, lane);
  if (lane == 0) out[b] = l;
}
__global__ void gt_duration_loss_bwd_kernel(const float* __restrict__ logw, const float* __restrict__ w, const int32_t* __restrict__ len,
                                            const float* __restrict__ g, int B, int Tx, float* __restrict__ dlogw)
{
  const int b = blockIdx.x;
  dur_loss_bwd_wave(logw, w, len, g[b], b, B, Tx, threadIdx.x, dlogw);
}

// ------------------------------------------------------------------ alignment -> loss chain in three launches
// Everything between MAS and the decoder's backward is elementwise, a gather or a segmented sum over the same [B, C, T_y] index
// space; as launches of their own (prior_expand, mle_sums, mle_finish, sum, add, mle_bwd, prior_expand_bwd, duration loss and its
// backward) each paid its in-graph launch cost on a stretch where both streams are joined.  The kernels below call the helpers the
// unfused kernels call, in their summation order: every output is bit-identical to theirs.
//
// Forward.  Workgroups 0 .. GT_MLE_PARTS-1: gt_mle_sums_kernel's index map (float4 i of the flat space -> thread i mod
// (GT_MLE_PARTS * 256)) with m (and logs) gathered through frame2token and stored as z_m (z_logs) on the way.  T_y % 4 == 0: a
// float4 never straddles two rows.  Workgroups GT_MLE_PARTS .. GT_MLE_PARTS+B-1 (logw given): the duration loss in wave 0.
__global__ __launch_bounds__(256) void gt_align_loss_fwd_kernel(const float* __restrict__ z, const float* __restrict__ xm,
                                                                const float* __restrict__ xlogs, const int32_t* __restrict__ f2t,
                                                                const float* __restrict__ logw, const float* __restrict__ w,
                                                                const int32_t* __restrict__ len, float* __restrict__ zm,
                                                                float* __restrict__ zlogs, float* __restrict__ acc,
                                                                float* __restrict__ l_length, int B, int C, int Tx, int Ty)
{
  if (blockIdx.x >= GT_MLE_PARTS) {
    const int b = blockIdx.x - GT_MLE_PARTS, lane = threadIdx.x;
    if (lane >= 64) return;
    const float l = dur_loss_fwd_wave(logw, w, len, b, B, Tx, lane);
    if (lane == 0) l_length[b] = l;
    return;
  }
  float a0 = 0.f, a1 = 0.f;
  const unsigned ty4 = (unsigned)Ty >> 2;
  const unsigned n4 = (unsigned)B * C * ty4;                   // B * C * T_y < 2^31 (the entry refuses more)
  for (unsigned i = blockIdx.x * 256 + threadIdx.x; i < n4; i += GT_MLE_PARTS * 256) {
    const unsigned bc = i / ty4, j4 = i - bc * ty4, b = bc / C;
    const int4 t = reinterpret_cast<const int4*>(f2t)[(size_t)b * ty4 + j4];
    const bool v0 = (unsigned)t.x < (unsigned)Tx, v1 = (unsigned)t.y < (unsigned)Tx, v2 = (unsigned)t.z < (unsigned)Tx,
               v3 = (unsigned)t.w < (unsigned)Tx;                // -1 = padded frame
    const float* xr = xm + (size_t)bc * Tx;
    const float4 zz = reinterpret_cast<const float4*>(z)[i];
    const float4 mm = make_float4(v0 ? xr[t.x] : 0.f, v1 ? xr[t.y] : 0.f, v2 ? xr[t.z] : 0.f, v3 ? xr[t.w] : 0.f);
    float4 ll = make_float4(0.f, 0.f, 0.f, 0.f);
    if (xlogs) {
      const float* sr = xlogs + (size_t)bc * Tx;
      ll = make_float4(v0 ? sr[t.x] : 0.f, v1 ? sr[t.y] : 0.f, v2 ? sr[t.z] : 0.f, v3 ? sr[t.w] : 0.f);
      reinterpret_cast<float4*>(zlogs)[i] = ll;
    }
    reinterpret_cast<float4*>(zm)[i] = mm;
    mle_quad(zz, mm, ll, a0, a1);
  }
  mle_partial_store(a0, a1, acc);
}

// The scalars: mle_loss's tail (commons.py:31-33) in one launch.  out[0] = loss = (acc[0] + 0.5 acc[1] - sum logdet) / denom +
// 0.5 log 2pi, out[1] = denom = C * sum(mask)  (= sum(ones_like(z) * mask)); that is all of gt_mle_finish (TOTAL = false: out has two
// floats).  TOTAL: out[2] = sum_b l_length[b] in the order ATen's sum gives a short contiguous fp32 vector (B < 128): lane t < nt =
// the largest power of two <= min(B, 64) adds l_length[t], l_length[t + nt], ..., then a shuffle-down tree over the nt lanes — so
// that the total equals mle + torch.sum(l_length) bit for bit.  out[3] = out[0] + out[2].
template <bool TOTAL>
__global__ __launch_bounds__(1024) void gt_align_loss_finish_kernel(const float* __restrict__ acc, const float* __restrict__ logdet,
                                                                    const float* __restrict__ mask, int n_mask,
                                                                    const float* __restrict__ l_length, int B, int C, float* __restrict__ out)
{
  // one workgroup (the result is a few scalars), 1024 threads and 16-byte loads: the mask is B x T floats (25 k at cfg 2) and a
  // 256-thread scalar loop over it sat 40 us on the step's critical path
  __shared__ float red[2][16];
  __shared__ float red2[2];
  {                                                          // the GT_MLE_PARTS partial pairs of mle_partial_store
    float p0 = 0.f, p1 = 0.f;
    for (int i = threadIdx.x; i < GT_MLE_PARTS; i += 1024) { const float2 v = reinterpret_cast<const float2*>(acc)[i]; p0 += v.x; p1 += v.y; }
    p0 = wave_sum(p0); p1 = wave_sum(p1);
    if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = p0; red[1][threadIdx.x >> 6] = p1; }
    __syncthreads();
    if (threadIdx.x == 0) {
      p0 = 0.f; p1 = 0.f;
#pragma unroll
      for (int i = 0; i < 16; ++i) { p0 += red[0][i]; p1 += red[1][i]; }
      red2[0] = p0; red2[1] = p1;
    }
    __syncthreads();
  }
  float sl = 0.f, sn = 0.f;
  for (int b = threadIdx.x; b < B; b += 1024) sl += logdet[b];
  const int n4 = ((reinterpret_cast<uintptr_t>(mask) & 15) == 0) ? n_mask >> 2 : 0;
  for (int i = threadIdx.x; i < n4; i += 1024) { const float4 v = reinterpret_cast<const float4*>(mask)[i]; sn += (v.x + v.y) + (v.z + v.w); }
  for (int i = (n4 << 2) + threadIdx.x; i < n_mask; i += 1024) sn += mask[i];
  sl = wave_sum(sl); sn = wave_sum(sn);
  if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = sl; red[1][threadIdx.x >> 6] = sn; }
  float ll = 0.f;
  if (TOTAL && l_length && threadIdx.x < 64) {                 // wave 0 (wave-uniform branch)
    int nt = 1;
    while (nt * 2 <= B && nt < 64) nt <<= 1;
    if ((int)threadIdx.x < nt)
      for (int i = threadIdx.x; i < B; i += nt) ll += l_length[i];
    for (int off = 1; off < nt; off <<= 1) ll += __shfl_down(ll, off);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    sl = 0.f; sn = 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) { sl += red[0][i]; sn += red[1][i]; }
    const float denom = sn * (float)C;
    const float mle = (red2[0] + 0.5f * red2[1] - sl) / denom + 0.91893853320467274f;
    out[0] = mle;
    out[1] = denom;
    if (TOTAL) {
      out[2] = ll;
      out[3] = mle + ll;
    }
  }
}

// Backward.  gt_prior_expand_bwd_kernel's geometry (four rows per workgroup, acc[..][4][512]) with mle_grad formed in the walk's
// loader (g = *gscale / *gdenom): dz = v is stored, -v goes into the scan (what dm was), and with logs gl goes into a second
// accumulator strip (what dlogs was).  Past the row workgroups: one sets dlogdet[b] = -g, B more do the duration loss's backward in
// wave 0 with g = *gscale.
template <bool LOGS>
__global__ __launch_bounds__(256) void gt_align_loss_bwd_kernel(const float* __restrict__ z, const float* __restrict__ zm,
                                                                const float* __restrict__ zlogs, const int32_t* __restrict__ f2t,
                                                                const float* __restrict__ logw, const float* __restrict__ w,
                                                                const int32_t* __restrict__ len, const float* __restrict__ gscale,
                                                                const float* __restrict__ gdenom, float* __restrict__ dz,
                                                                float* __restrict__ dxm, float* __restrict__ dxlogs,
                                                                float* __restrict__ dlogdet, float* __restrict__ dlogw,
                                                                int B, int C, int Tx, int Ty, int row_blocks)
{
  constexpr int NV = LOGS ? 2 : 1;
  __shared__ float acc[NV][4][512];
  if ((int)blockIdx.x >= row_blocks) {
    const int e = blockIdx.x - row_blocks;
    if (e == 0) {
      const float g = *gscale / *gdenom;
      for (int b = threadIdx.x; b < B; b += 256) dlogdet[b] = -g;
      return;
    }
    if (threadIdx.x >= 64) return;
    dur_loss_bwd_wave(logw, w, len, *gscale, e - 1, B, Tx, threadIdx.x, dlogw);
    return;
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int bc = blockIdx.x * 4 + wave;
  if (bc >= B * C) return;                                  // waves are independent: no workgroup barrier below
  const float g = *gscale / *gdenom;
  const size_t r = (size_t)bc * Ty;
  SegRows<NV> a, out;
  a.p[0] = acc[0][wave]; out.p[0] = dxm + (size_t)bc * Tx;
  if constexpr (LOGS) { a.p[1] = acc[1][wave]; out.p[1] = dxlogs + (size_t)bc * Tx; }
  segmented_walk<NV>([&](int j, float (&s)[NV]) {
    float v, gl;
    mle_grad(g, LOGS ? zlogs[r + j] : 0.f, z[r + j], zm[r + j], v, gl);
    dz[r + j] = v;
    s[0] = -v;
    if constexpr (LOGS) s[1] = gl;
  }, f2t + (size_t)(bc / C) * Ty, Ty, Tx, lane, a, out);
}

}  // namespace

extern "C" int gt_logp_f32(const float* x_m, const float* x_logs, const float* z, float* logp, int B, int C, int Tx, int Ty, void* stream)
{
  if (!x_m || !z || !logp || B <= 0 || C <= 0 || (C & 1) || Tx <= 0 || Ty <= 0) return GT_E_INVAL;
  hipLaunchKernelGGL(gt_logp_kernel, dim3((Ty + 127) / 128, (Tx + 31) / 32, B), dim3(256), 0, GT_ST(stream), x_m, x_logs, z, logp, B, C, Tx, Ty);
  GT_RET();
}

extern "C" int gt_prior_expand(const float* x_m, const int32_t* frame2token, float* z_m, int B, int C, int Tx, int Ty, void* stream)
{
  if (!x_m || !frame2token || !z_m || B <= 0 || C <= 0 || Tx <= 0 || Ty <= 0) return GT_E_INVAL;
  hipLaunchKernelGGL(gt_prior_expand_kernel, dim3(((size_t)B * C * Ty + 255) / 256), dim3(256), 0, GT_ST(stream), x_m, frame2token, z_m, B, C, Tx, Ty);
  GT_RET();
}
extern "C" int gt_prior_expand_bwd(const float* dz_m, const int32_t* frame2token, float* dx_m, int B, int C, int Tx, int Ty, void* stream)
{
  if (!dz_m || !frame2token || !dx_m || B <= 0 || C <= 0 || Tx <= 0 || Ty <= 0) return GT_E_INVAL;
  if (Tx > 16384) return GT_E_UNSUPPORTED;                    // 64 KiB of LDS per row; gt_mas_long_f32 stops at 4096 tokens
  if (Tx > 512)                                               // past acc[4][512]: a wave per workgroup, Tx floats of dynamic LDS
    hipLaunchKernelGGL(gt_prior_expand_bwd_kernel<true>, dim3((unsigned)((size_t)B * C)), dim3(64), (size_t)Tx * 4, GT_ST(stream),
                       dz_m, frame2token, dx_m, B, C, Tx, Ty);
  else
    hipLaunchKernelGGL(gt_prior_expand_bwd_kernel<false>, dim3(((size_t)B * C + 3) / 4), dim3(256), 0, GT_ST(stream),
                       dz_m, frame2token, dx_m, B, C, Tx, Ty);
  GT_RET();
}
extern "C" int gt_mle_sums(const float* z, const float* m, const float* logs, float* acc2, size_t n, void* stream)
{
  if (!acc2 || (n && (!z || !m))) return GT_E_INVAL;
  // n == 0 launches too: the kernel then reads nothing and stores GT_MLE_PARTS zero pairs, which is what gt_mle_finish sums
  if (((uintptr_t)z | (uintptr_t)m | (uintptr_t)logs) & 15) return GT_E_ALIGN;
  if ((uintptr_t)acc2 & 7) return GT_E_ALIGN;
  hipLaunchKernelGGL(gt_mle_sums_kernel, dim3(GT_MLE_PARTS), dim3(256), 0, GT_ST(stream), z, m, logs, acc2, n);
  GT_RET();
}
extern "C" int gt_length_mask(const void* lengths, int is_int64, float* mask, int B, int T, void* stream)
{
  if (!lengths || !mask || B <= 0 || T <= 0) return GT_E_INVAL;
  hipLaunchKernelGGL(gt_length_mask_kernel, dim3(((size_t)B * T + 255) / 256), dim3(256), 0, GT_ST(stream), lengths, is_int64, mask, B, T);
  GT_RET();
}
extern "C" int gt_mle_finish(const float* acc2, const float* logdet, const float* mask, int n_mask, int B, int C, float* out2, void* stream)
{
  if (!acc2 || !logdet || !mask || !out2 || B <= 0 || C <= 0 || n_mask <= 0) return GT_E_INVAL;
  hipLaunchKernelGGL(gt_align_loss_finish_kernel<false>, dim3(1), dim3(1024), 0, GT_ST(stream), acc2, logdet, mask, n_mask, nullptr, B, C, out2);
  GT_RET();
}
extern "C" int gt_duration_loss_fwd(const float* logw, const float* w, const int32_t* x_lengths, int B, int Tx, float* l_length, void* stream)
{
  if (!logw || !w || !x_lengths || !l_length || B <= 0 || Tx <= 0) return GT_E_INVAL;
  hipLaunchKernelGGL(gt_duration_loss_fwd_kernel, dim3(B), dim3(64), 0, GT_ST(stream), logw, w, x_lengths, B, Tx, l_length);
  GT_RET();
}
extern "C" int gt_duration_loss_bwd(const float* logw, const float* w, const int32_t* x_lengths, const float* g, int B, int Tx,
                                    float* dlogw, void* stream)
{
  if (!logw || !w || !x_lengths || !g || !dlogw || B <= 0 || Tx <= 0) return GT_E_INVAL;
  hipLaunchKernelGGL(gt_duration_loss_bwd_kernel, dim3(B), dim3(64), 0, GT_ST(stream), logw, w, x_lengths, g, B, Tx, dlogw);
  GT_RET();
}
extern "C" int gt_align_loss_fwd(const float* z, const float* x_m, const float* x_logs, const int32_t* frame2token, const float* logw,
                                 const float* w, const int32_t* x_lengths, float* z_m, float* z_logs, float* acc2, float* l_length,
                                 int B, int C, int Tx, int Ty, void* stream)
{
  if (!z || !x_m || !frame2token || !z_m || !acc2 || (x_logs && !z_logs) || B <= 0 || C <= 0 || Tx <= 0 || Ty <= 0) return GT_E_INVAL;
  if ((logw != nullptr) != (w != nullptr) || (logw && (!x_lengths || !l_length))) return GT_E_INVAL;
  if (Tx > 512) return GT_E_UNSUPPORTED;                      // gt_align_loss_bwd's token accumulators end there: the unfused entries go on
  if ((size_t)B * C * Ty > 0x7fffffffu) return GT_E_UNSUPPORTED;
  if (Ty & 3) return GT_E_ALIGN;                              // a float4 of the flat index space must not straddle two rows
  if (((uintptr_t)z | (uintptr_t)z_m | (uintptr_t)z_logs | (uintptr_t)frame2token) & 15) return GT_E_ALIGN;
  if ((uintptr_t)acc2 & 7) return GT_E_ALIGN;
  hipLaunchKernelGGL(gt_align_loss_fwd_kernel, dim3(GT_MLE_PARTS + (logw ? B : 0)), dim3(256), 0, GT_ST(stream), z, x_m, x_logs, frame2token,
                     logw, w, x_lengths, z_m, z_logs, acc2, l_length, B, C, Tx, Ty);
  GT_RET();
}
extern "C" int gt_align_loss_finish(const float* acc2, const float* logdet, const float* mask, int n_mask, const float* l_length, int B, int C,
                                    float* out4, void* stream)
{
  if (!acc2 || !logdet || !mask || !out4 || B <= 0 || C <= 0 || n_mask <= 0) return GT_E_INVAL;
  if ((uintptr_t)acc2 & 7) return GT_E_ALIGN;
  hipLaunchKernelGGL(gt_align_loss_finish_kernel<true>, dim3(1), dim3(1024), 0, GT_ST(stream), acc2, logdet, mask, n_mask, l_length, B, C, out4);
  GT_RET();
}
extern "C" int gt_align_loss_bwd(const float* z, const float* z_m, const float* z_logs, const int32_t* frame2token, const float* logw,
                                 const float* w, const int32_t* x_lengths, const float* gscale, const float* gdenom, float* dz, float* dx_m,
                                 float* dx_logs, float* dlogdet, float* dlogw, int B, int C, int Tx, int Ty, void* stream)
{
  if (!z || !z_m || !frame2token || !gscale || !gdenom || !dz || !dx_m || !dlogdet || (z_logs && !dx_logs) || B <= 0 || C <= 0 || Tx <= 0 ||
      Ty <= 0)
    return GT_E_INVAL;
  if ((logw != nullptr) != (w != nullptr) || (logw && (!x_lengths || !dlogw))) return GT_E_INVAL;
  if (Tx > 512) return GT_E_UNSUPPORTED;                      // acc[..][4][512]: past it gt_prior_expand_bwd's long form (the unfused chain)
  if ((size_t)B * C * Ty > 0x7fffffffu) return GT_E_UNSUPPORTED;
  const int row_blocks = (int)(((size_t)B * C + 3) / 4);
  const dim3 grid(row_blocks + 1 + (logw ? B : 0));
  if (z_logs)
    hipLaunchKernelGGL(gt_align_loss_bwd_kernel<true>, grid, dim3(256), 0, GT_ST(stream), z, z_m, z_logs, frame2token, logw, w, x_lengths, gscale,
                       gdenom, dz, dx_m, dx_logs, dlogdet, dlogw, B, C, Tx, Ty, row_blocks);
  else
    hipLaunchKernelGGL(gt_align_loss_bwd_kernel<false>, grid, dim3(256), 0, GT_ST(stream), z, z_m, z_logs, frame2token, logw, w, x_lengths, gscale,
                       gdenom, dz, dx_m, dx_logs, dlogdet, dlogw, B, C, Tx, Ty, row_blocks);
  GT_RET();
}
extern "C" int gt_mle_bwd(const float* z, const float* m, const float* logs, const float* gscale, float* dz, float* dm, float* dlogs,
                          size_t n, const float* gdenom, float* dlogdet, int B, void* stream)
{
  if (!z || !m || !gscale) return GT_E_INVAL;
  if (n == 0) return GT_OK;
  size_t blocks = (n + 255) / 256; if (blocks > 2048) blocks = 2048;
  hipLaunchKernelGGL(gt_mle_bwd_kernel, dim3((unsigned)blocks), dim3(256), 0, GT_ST(stream), z, m, logs, gscale, dz, dm, dlogs, n, gdenom, dlogdet, B);
  GT_RET();
}
