// Everything BETWEEN two WaveNets of the flow decoder as one kernel, forward and backward (and, further down, the reverse
// direction that synthesis runs), gfx950.
//
// reference, per flow block b (models.py:765-785 runs ActNorm, InvConvNear, CouplingBlock in turn):
//     y      = InvConvNear(ActNorm(x))                                        modules.py:584-599, 635-665
//     h      = start(y0) * mask                                               attentions.py:147
//     out    = WN(h)           = (sum_i skip_i(acts_i)) * mask                modules.py:144-171
//     m|logs = end(out)                                                       attentions.py:162-165
//     z      = [y0 | (m + exp(logs) * y1) * mask],  logdet += sum logs * mask attentions.py:171-184
// All of it except the WaveNet's k=5 layers is ROW-LOCAL (1x1 convs, elementwise maps, 4x4 channel mixing, per-utterance
// sums).  Round 1 ran it as five launches per block forward (skip GEMM, end conv, coupling, ActNorm+InvConv, start conv)
// and five backward, ~13 us each on the decoder's dependent chain for a few microseconds of work.  Here a workgroup owns
// 64 rows and walks the whole chain on them, tile after tile in LDS:
//
//   forward  [tail of block b]    acts [64, 4H] -> skip GEMM (K = 768) -> wn_out -> end conv (K = 192) -> m | logs
//                                 -> coupling -> z (HBM: the flow state, saved for the backward) + per-utterance log-det
//            [head of block b+1]  ActNorm + InvConvNear on the z tile -> y (HBM), y0 (bf16) -> start conv (K = 80) -> h
//   backward [head of block b+1]  d h -> start data gradient (K = 192, N = 80) + identity path -> ActNorm / InvConvNear
//                                 backward (parameter gradients folded over the tile in LDS, then atomics)
//            [tail of block b]    coupling backward -> d[m | logs] -> end data gradient (K = 160) -> d wn_out -> skip data
//                                 gradient (N = 768) -> the skip-path gradient of every layer's gated activations
// The first / last kernels of a pass have only a head or only a tail.  MFMA A = weights in fragment order straight from
// L2 (every workgroup reads the same 0.4 MB: L2-resident), B = the bf16 LDS tile; accumulators e = 4g + j of lane (r, h)
// are row r, column 32 * block + 8g + 4h + j.  What leaves for HBM is what the batched weight gradients and the next
// pass read anyway (wn_out, y0, d out, d wn_out) plus the fp32 flow state.
// The row maths are flow_rows.h's, shared with flow_ops.hip; what the three kernels do alike to a tile is a step below ("tile steps").
#include "common.h"
#include "internal.h"
#include "mfma_frag.h"
#include "flow_rows.h"
#include "../../include/glowtts_hip.h"

namespace {

constexpr int H = 192, C = 160, HALF = 80, NL = 4, G = C / 4;
constexpr int BM = 64;
constexpr int AP = H + 8;                     // bf16 tile pitch (halfs): 400 B = 16 mod 128 -> conflict-free ds_read_b128
constexpr int XP = 136;                       // y0 tile pitch (halfs): K = 80 -> 5 k-steps; 272 B = 16 mod 128
constexpr int ZP = C + 4;                     // fp32 tile pitch (floats)
constexpr int RD = 8;                         // weight-fragment ring: k-steps in flight per wave
// Barriers are __syncthreads().  One that waits for LDS traffic only (no vmcnt(0)) measured (round 3, back to back) 28.3 vs 28.1 us
// forward, 28.9 vs 28.7 us backward: the drains are not what the phases wait for.
#ifndef WNB_PHASES
#define WNB_PHASES 0                          // dev: per-phase shader-clock stamps of wave 0 (tools/wn_stack_phases.py), 0 in every build that ships
#endif
#if WNB_PHASES
__device__ unsigned long long g_wnb_ph[1024 * 48];
#define PH(i) do { if (threadIdx.x == 0 && blockIdx.x < 1024) g_wnb_ph[blockIdx.x * 48 + (i)] = __builtin_amdgcn_s_memtime(); } while (0)
#else
#define PH(i) do { } while (0)
#endif

// acc[bn] += W[block nb0 + bn][k-steps 0 .. KK) x Bt: W in fragment order with KS k-steps per block row; Brow points at
// (this lane's row, 8h) of the bf16 LDS tile, k-step kk is 16 halfs further.  The first ring of fragments is fetched by
// gemm_prefetch, which callers issue BEFORE the phase that produces the tile (weights do not depend on it), so the L2
// latency of a stage hides under the previous stage's epilogue.
template <int NB, int KK>
struct WRing { uint4 v[(KK < RD ? KK : RD)][NB]; };

template <int NB, int KK>
__device__ __forceinline__ void gemm_prefetch(const bf16_t* __restrict__ W, int KS, int nb0, int lane, WRing<NB, KK>& ring)
{
  constexpr int D = KK < RD ? KK : RD;
#pragma unroll
  for (int p = 0; p < D; ++p)
#pragma unroll
    for (int bn = 0; bn < NB; ++bn) ring.v[p][bn] = ldfrag(W, (nb0 + bn) * KS + p, lane);
}
template <int NB, int KK>
__device__ __forceinline__ void gemm_run(const bf16_t* __restrict__ W, int KS, int nb0, const bf16_t* Brow, int lane, WRing<NB, KK>& ring,
                                         f32x16_t (&acc)[NB])
{
  // blocks of CH k-steps: their MFMAs, then the loads that refill the ring slots those MFMAs have just read.  (A load placed behind
  // every MFMA holds the wave's issue for longer than the MFMA it was meant to hide behind: wn_stack.hip, round 3.)
  constexpr int D = KK < RD ? KK : RD, CH = 4;
#pragma unroll
  for (int k0 = 0; k0 < KK; k0 += CH) {
#pragma unroll
    for (int kk = k0; kk < k0 + CH && kk < KK; ++kk) {
      const bf16x8_t bfm = *reinterpret_cast<const bf16x8_t*>(Brow + kk * 16);
#pragma unroll
      for (int bn = 0; bn < NB; ++bn) acc[bn] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(asfrag(ring.v[kk % D][bn]), bfm, acc[bn], 0, 0, 0);
    }
    if (k0 + D < KK) {
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int kk = k0; kk < k0 + CH && kk + D < KK; ++kk)
#pragma unroll
        for (int bn = 0; bn < NB; ++bn) ring.v[kk % D][bn] = ldfrag(W, (nb0 + bn) * KS + kk + D, lane);
      __builtin_amdgcn_sched_barrier(0);
    }
  }
}

// per-utterance sum of 64 per-row values (one wave; rows of an utterance are consecutive): segmented scan, then ONE
// atomic per utterance run of the tile (per-row atomics onto B addresses would serialise at L2)
__device__ __forceinline__ void utt_atomic_add(float* __restrict__ dst, float s, int utt, int lane)
{
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const float v = __shfl_up(s, off);
    const int u = __shfl_up(utt, off);
    if (lane >= off && u == utt) s += v;
  }
  const int un = __shfl_down(utt, 1);
  if ((lane == 63 || un != utt) && s != 0.0f) atomicAdd(dst + utt, s);
}

// layer slice L of the skip GEMM (K = 4H in four LDS tiles): registers -> LDS, barrier, 12 k-steps; the weight ring runs
// across the slices (L is a template parameter so that every ring / staging index is a compile-time constant)
struct Lane { int lane, r, h, wm, wn; };   // lane (r, h) of wave (wm, wn): rows 32 wm .., column blocks 3 wn .. (2 wn .. where N = 80)

template <int L>
__device__ __forceinline__ void skip_slice(const u32x4_t (&xr)[6], bf16_t* As, const bf16_t* __restrict__ Wskip, const Lane& t,
                                           uint4 (&ring)[RD][3], f32x16_t (&acc)[3])
{
  const int wm = t.wm, wn = t.wn, r = t.r, h = t.h, lane = t.lane;
  constexpr int KK = NL * H / 16, kbase = L * (H / 16);
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    const int chunk = threadIdx.x + 256 * i, row = chunk / 24, c8 = chunk - row * 24;
    *reinterpret_cast<u32x4_t*>(As + (L * BM + row) * AP + c8 * 8) = xr[i];
  }
  __syncthreads();
  const bf16_t* brow = As + (L * BM + 32 * wm + r) * AP + 8 * h;
  constexpr int CH = 4;
#pragma unroll
  for (int k0 = 0; k0 < H / 16; k0 += CH) {
#pragma unroll
    for (int k2 = k0; k2 < k0 + CH; ++k2) {
      const bf16x8_t bfm = *reinterpret_cast<const bf16x8_t*>(brow + k2 * 16);
#pragma unroll
      for (int bn = 0; bn < 3; ++bn) acc[bn] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(asfrag(ring[(kbase + k2) % RD][bn]), bfm, acc[bn], 0, 0, 0);
    }
    if (kbase + k0 + RD < KK) {
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int k2 = k0; k2 < k0 + CH; ++k2)
#pragma unroll
        for (int bn = 0; bn < 3; ++bn)
          if (kbase + k2 + RD < KK) ring[(kbase + k2) % RD][bn] = ldfrag(Wskip, (3 * wn + bn) * KK + kbase + k2 + RD, lane);
      __builtin_amdgcn_sched_barrier(0);
    }
  }
}

// A finished [64][AP] bf16 tile -> global rows m0 .. m0 + 63 (row stride ld, 192 channels): 16 bytes per lane, consecutive lanes on
// consecutive addresses.  Stored straight from the MFMA accumulator layout, one instruction writes 16 bytes to each of 32 rows —
// partial lines that the memory pipeline handles one request at a time (wn_stack.hip measured the difference: -5 us per launch).
__device__ __forceinline__ void coop_store_rows(bf16_t* __restrict__ dst, int ld, const bf16_t* __restrict__ tile, int m0, int R)
{
  constexpr int CPR = H / 8;
#pragma unroll
  for (int i = 0; i < BM * CPR / 256; ++i) {
    const int idx = threadIdx.x + 256 * i, row = idx / CPR, c8 = idx - row * CPR, gm = m0 + row;
    if (gm < R) *reinterpret_cast<uint4*>(dst + (size_t)gm * ld + c8 * 8) = *reinterpret_cast<const uint4*>(tile + row * AP + c8 * 8);
  }
}

// Prefetch workgroups.  The launch that FOLLOWS a boundary launch on the decoder's chain is a whole WaveNet, and every one of its
// workgroups streams all 3.2 MB of that WaveNet's weight images — first touched there, they come from HBM (the step's 2 GB of saved
// activations have pushed everything else out of the 256 MB Infinity Cache) and every workgroup waits on the same misses: + 13 us
// on a forward launch, + 9 us on a backward one, all of it gone once the images are back in the cache (tools/wn_layer_bench.py,
// WN_BENCH_COLD).  A boundary launch runs 152 workgroups on 256 CUs: PF_WGS extra workgroups (blockIdx >= the row tiles) read
// those images once, on CUs that were idle, and retire within a few microseconds.
//
// The loads have no consumer, so something must keep the compiler from deleting them.  KEEP = true feeds their XOR to an empty
// asm volatile: no store, nothing the caller owns is touched, whatever bytes the buffers hold (tests/test_wn_boundary_fp64_gpu.py,
// test_prefetch_buffers_are_inert).  It used to be a store of the XOR to a caller's pointer — the forward's logdet — under a
// comparison with one magic word, on the claim that bf16 weight bits never form that word: they can, and logdet[0] then lost every
// earlier block's log-det.
// Only the FORWARD kernels pass KEEP = true.  The backward and reverse kernels passed a NULL sink, the compiler deleted their loads,
// and their prefetch workgroups are EMPTY in the current build and in its parent (the branch is a bare s_endpgm;
// profiles/wn_boundary_prefetch_isa.txt; earlier builds were not disassembled): with such code only the forward's of the two
// savings quoted above can come from these workgroups.  KEEP = false keeps that device code
// byte-identical; turning it on is a performance change that needs its own measurement.
constexpr int PF_WGS = 64;
template <bool KEEP>
__device__ __forceinline__ void prefetch_images(const void* const (&ptr)[16], const uint32_t (&bytes)[16], int wg)
{
  uint32_t acc = 0;
  const int gid = wg * 256 + threadIdx.x, nthr = PF_WGS * 256;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    if (!ptr[i]) break;
    const uint4* src = static_cast<const uint4*>(ptr[i]);
    const int n16 = (int)(bytes[i] >> 4);
    for (int c = gid; c < n16; c += 4 * nthr) {                       // four independent loads in flight per thread
      const uint4 v0 = src[c];
      const uint4 v1 = c + nthr < n16 ? src[c + nthr] : make_uint4(0, 0, 0, 0);
      const uint4 v2 = c + 2 * nthr < n16 ? src[c + 2 * nthr] : make_uint4(0, 0, 0, 0);
      const uint4 v3 = c + 3 * nthr < n16 ? src[c + 3 * nthr] : make_uint4(0, 0, 0, 0);
      acc ^= v0.x ^ v1.y ^ v2.z ^ v3.w;
    }
  }
  if (KEEP) asm volatile("" :: "v"(acc));                               // consumes the loads; emits nothing
}

// ------------------------------------------------------------------------------------------------ tile steps
// Barriers stay in the bodies except start_conv_stage's; the forward's stamps 1, 9, 10 fall inside a step: written there under STAMP.
// b_skip [192] | b_end [160 (+ 32 zero)] | b_start [192] -> Bs, the tile's row mask -> Bs + 3 H, staged once: from global memory the biases
// cost an L2 round trip per (block, group) in the epilogues, and a mask load in a loop that also stores waits for those stores
template <bool TAIL, bool HEAD>
__device__ __forceinline__ void stage_bias_mask(float* Bs, const float* b_skip, const float* b_end, const float* b_start, const float* rowmask, int m0, int R)
{
  if (threadIdx.x < 3 * H / 4) {
    const int which = threadIdx.x / (H / 4), o = threadIdx.x - which * (H / 4);
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (which == 0) { if (TAIL) v = reinterpret_cast<const float4*>(b_skip)[o]; }
    else if (which == 1) { if (TAIL && o < C / 4) v = reinterpret_cast<const float4*>(b_end)[o]; }
    else if (HEAD) v = reinterpret_cast<const float4*>(b_start)[o];
    reinterpret_cast<float4*>(Bs)[threadIdx.x] = v;
  }
  if (threadIdx.x >= 192) {
    const int row = threadIdx.x - 192;
    Bs[3 * H + row] = m0 + row < R ? rowmask[m0 + row] : 0.0f;
  }
}

// the tile's gated activations, all four layers: 6 x 16 B per thread and slice, in flight together (plain vector: stays in registers)
__device__ __forceinline__ void load_acts(u32x4_t (&xr)[NL][6], const bf16_t* acts, int ldacts, int m0, int R)
{
#pragma unroll
  for (int l = 0; l < NL; ++l)
#pragma unroll
    for (int i = 0; i < 6; ++i) {
      const int chunk = threadIdx.x + 256 * i, row = chunk / 24, c8 = chunk - row * 24;
      const int gm = m0 + row < R ? m0 + row : R - 1;
      xr[l][i] = *reinterpret_cast<const u32x4_t*>(acts + (size_t)gm * ldacts + l * H + c8 * 8);
    }
}

// skip GEMM: acc = acts @ Wskip^T (K = 768: 48 k-steps, four slices through LDS); three barriers behind it every wave is past slices 0..2
template <bool STAMP>
__device__ __forceinline__ void skip_gemm(const u32x4_t (&xr)[NL][6], bf16_t* As, const bf16_t* Wskip, const Lane& t, f32x16_t (&acc)[3])
{
  acc_zero<3>(acc);
  constexpr int KK = NL * H / 16;
  uint4 ring[RD][3];
#pragma unroll
  for (int p = 0; p < RD; ++p)
#pragma unroll
    for (int bn = 0; bn < 3; ++bn) ring[p][bn] = ldfrag(Wskip, (3 * t.wn + bn) * KK + p, t.lane);
  if (STAMP) PH(1);
  skip_slice<0>(xr[0], As, Wskip, t, ring, acc);
  skip_slice<1>(xr[1], As, Wskip, t, ring, acc);
  skip_slice<2>(xr[2], As, Wskip, t, ring, acc);
  skip_slice<3>(xr[3], As, Wskip, t, ring, acc);
}

// accumulators (+ bias, * the lane's row mask) -> bf16 -> a [64][AP] LDS tile: the GEMM epilogues that end in bf16 (the backward's
// mask-only one keeps its own copy, see there)
template <bool BIAS, bool MASK>
__device__ __forceinline__ void pack_tile(const f32x16_t (&acc)[3], const float* bias, float rm_l, bf16_t* tile, const Lane& t)
{
#pragma unroll
  for (int bn = 0; bn < 3; ++bn)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int n = 32 * (3 * t.wn + bn) + 8 * g + 4 * t.h;
      float v[4] = {acc[bn][4 * g], acc[bn][4 * g + 1], acc[bn][4 * g + 2], acc[bn][4 * g + 3]};
      if (BIAS) { const float4 b4 = *reinterpret_cast<const float4*>(bias + n); v[0] = v[0] + b4.x; v[1] = v[1] + b4.y; v[2] = v[2] + b4.z; v[3] = v[3] + b4.w; }
      if (MASK) { v[0] = v[0] * rm_l; v[1] = v[1] * rm_l; v[2] = v[2] * rm_l; v[3] = v[3] * rm_l; }
      *reinterpret_cast<uint2*>(tile + (32 * t.wm + t.r) * AP + n) = pack4(v[0], v[1], v[2], v[3]);
    }
}

// the end conv's accumulators + bias -> the fp32 [m | logs] tile (N = 160: blocks 0..4, block 5 is the image's zero padding)
__device__ __forceinline__ void end_epilogue(const f32x16_t (&acc)[3], const float* bias, float* Ot, const Lane& t)
{
#pragma unroll
  for (int bn = 0; bn < 3; ++bn)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int n = 32 * (3 * t.wn + bn) + 8 * g + 4 * t.h;
      if (n < C) {
        const float4 b4 = *reinterpret_cast<const float4*>(bias + n);
        *reinterpret_cast<float4*>(Ot + (32 * t.wm + t.r) * ZP + n) =
            make_float4(acc[bn][4 * g] + b4.x, acc[bn][4 * g + 1] + b4.y, acc[bn][4 * g + 2] + b4.z, acc[bn][4 * g + 3] + b4.w);
      }
    }
}

// start conv: h = (y0 @ Wstart^T + b) * mask (K = 80: 5 k-steps, fragments prefetched into ring) from the bf16 y0 tile, out through Hst
template <bool STAMP>
__device__ __forceinline__ void start_conv_stage(const bf16_t* Wstart, int ks_start, WRing<3, HALF / 16>& ring, const bf16_t* X0t, const float* bias,
                                                 float rm_l, bf16_t* Hst, bf16_t* h_next, int m0, int R, const Lane& t)
{
  f32x16_t acc[3];
  acc_zero<3>(acc);
  gemm_run<3, HALF / 16>(Wstart, ks_start, 3 * t.wn, X0t + (32 * t.wm + t.r) * XP + 8 * t.h, t.lane, ring, acc);
  if (STAMP) PH(9);
  pack_tile<true, true>(acc, bias, rm_l, Hst, t);
  __syncthreads();
  if (STAMP) PH(10);
  coop_store_rows(h_next, H, Hst, m0, R);
}

// first kernel of a pass: the tile's rows, read as rows or gathered from [B, 80, T] (then also kept in rows_out); put() fills the tile
template <bool KEPT, class Put>
__device__ __forceinline__ void first_rows(const float* bct, const float* rows_in, float* rows_out,
                                           const int64_t* rowbatch, const int32_t* rowframe, const int32_t* len,
                                           int T, int m0, int R, Put put)
{
#pragma unroll
  for (int k = 0; k < 10; ++k) {
    const int item = threadIdx.x + 256 * k, row = item / 40, c = 4 * (item - row * 40), gm = m0 + row;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (gm < R) {
      if (bct) {
        const int b = (int)rowbatch[gm], t = rowframe[gm];
        if (t >= 0 && t < len[b]) v = fr::sq_gather4(bct, b, t, c, T, HALF);
        if (KEPT || rows_out) *reinterpret_cast<float4*>(rows_out + (size_t)gm * C + c) = v;   // KEPT: the entry has checked rows_out
      } else v = *reinterpret_cast<const float4*>(rows_in + (size_t)gm * C + c);
    }
    put(row, c, v);
  }
}

// ------------------------------------------------------------------------------------------------ forward
constexpr int F_AS = 0;                                    // acts slices [4][64][AP] bf16; later At [64][AP] (slice 0) / y0 tile
constexpr int F_O = BM * AP * 2;                           // m | logs tile [64][ZP] fp32 (over slices 1, 2 once they are dead)
constexpr int F_Z = F_O + BM * ZP * 4;                     // z tile [64][ZP] fp32
constexpr int F_RS = (F_Z + BM * ZP * 4 > NL * BM * AP * 2 ? F_Z + BM * ZP * 4 : NL * BM * AP * 2);   // row sums [64] fp32
constexpr int F_BIAS = F_RS + BM * 4;                      // b_skip [192] | b_end [160 (+ 32 zero)] | b_start [192] fp32, staged once
constexpr int FWD_LDS = F_BIAS + 3 * H * 4 + BM * 4;       // + the tile's row mask [64]
static_assert(F_O + BM * ZP * 4 <= 3 * BM * AP * 2, "the m | logs tile must stay clear of acts slice 3");

// (waves_per_eu: 110 KB of tiles admit one workgroup per CU whatever the registers; without the ceiling <0,1> stops at 120 + 48, three waves, for 124 + 48)
template <bool TAIL, bool HEAD>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 2))) void gt_wn_boundary_fwd_kernel(gt_boundary_fwd_args a)
{
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int n_tiles = (a.R + BM - 1) / BM;
  if ((int)blockIdx.x >= n_tiles) { prefetch_images<true>(a.pf_ptr, a.pf_bytes, blockIdx.x - n_tiles); return; }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = lane & 31, h = lane >> 5, wm = wave >> 1, wn = wave & 1;
  const int m0 = blockIdx.x * BM, R = a.R;
  bf16_t* As = reinterpret_cast<bf16_t*>(smem + F_AS);
  float* Ot = reinterpret_cast<float*>(smem + F_O);
  float* Zt = reinterpret_cast<float*>(smem + F_Z);
  float* rowsum = reinterpret_cast<float*>(smem + F_RS);
  const Lane ln{lane, r, h, wm, wn};
  const int mrow = m0 + 32 * wm + r;                        // this lane's row in the MFMA epilogues
  const float rm_l = mrow < R ? a.rowmask[mrow] : 0.0f;
  float* Bs = reinterpret_cast<float*>(smem + F_BIAS);
  float* Rm = Bs + 3 * H;
  stage_bias_mask<TAIL, HEAD>(Bs, a.b_skip, a.b_end, a.b_start, a.rowmask, m0, R);
  PH(0);

  if (TAIL) {
    u32x4_t xr[NL][6];
    load_acts(xr, static_cast<const bf16_t*>(a.acts), a.ldacts, m0, R);
    if (threadIdx.x < BM) rowsum[threadIdx.x] = 0.0f;
    // skip GEMM: wn_out = (acts @ Wskip^T + b) * mask
    f32x16_t acc[3];
    skip_gemm<true>(xr, As, static_cast<const bf16_t*>(a.w_skip), ln, acc);
    PH(2);
    // the end conv's first weight fragments fly under this epilogue
    WRing<3, H / 16> ring2;
    gemm_prefetch<3, H / 16>(static_cast<const bf16_t*>(a.w_end), a.ks_end, 3 * wn, lane, ring2);
    pack_tile<true, true>(acc, Bs, rm_l, As, ln);                    // At = slice 0's region
    __syncthreads();
    PH(3);
    coop_store_rows(static_cast<bf16_t*>(a.wn_out), H, As, m0, R);   // whole rows from the tile (see coop_store_rows)
    // end conv: [m | logs] = wn_out @ Wend^T + b
    // the coupling's inputs (this block's y, written by the previous launch) fly under the end conv
    float4 cy0[5], cy1[5];
    float crm[5];
#pragma unroll
    for (int k = 0; k < 5; ++k) {
      const int item = threadIdx.x + 256 * k, row = item / 20, c = 4 * (item - row * 20), gm = m0 + row < R ? m0 + row : R - 1;
      cy0[k] = *reinterpret_cast<const float4*>(a.y + (size_t)gm * C + c);
      cy1[k] = *reinterpret_cast<const float4*>(a.y + (size_t)gm * C + HALF + c);
      crm[k] = a.rowmask[gm];
    }
    f32x16_t acc2[3];
    acc_zero<3>(acc2);
    gemm_run<3, H / 16>(static_cast<const bf16_t*>(a.w_end), a.ks_end, 3 * wn, As + (32 * wm + r) * AP + 8 * h, lane, ring2, acc2);
    PH(4);
    end_epilogue(acc2, Bs + H, Ot, ln);
    __syncthreads();
    PH(5);
    // affine coupling on (row, 4 channels): z = [y0 | (m + exp(logs) y1) mask]
#pragma unroll
    for (int k = 0; k < 5; ++k) {
      const int item = threadIdx.x + 256 * k, row = item / 20, c = 4 * (item - row * 20), gm = m0 + row;
      float4 z0 = make_float4(0.f, 0.f, 0.f, 0.f), z1 = z0;
      if (gm < R) {
        const float rm = crm[k];
        const float4 mm = *reinterpret_cast<const float4*>(Ot + row * ZP + c);
        const float4 lr = *reinterpret_cast<const float4*>(Ot + row * ZP + HALF + c);
        z0 = cy0[k];
        const float4 y1 = cy1[k];
        float lg[4] = {lr.x, lr.y, lr.z, lr.w}; fr::coupling_lg(lg, a.sigmoid_scale);
        z1 = make_float4(fr::coupling_fwd(mm.x, lg[0], y1.x, rm), fr::coupling_fwd(mm.y, lg[1], y1.y, rm),
                         fr::coupling_fwd(mm.z, lg[2], y1.z, rm), fr::coupling_fwd(mm.w, lg[3], y1.w, rm));
        if (a.z) {
          *reinterpret_cast<float4*>(a.z + (size_t)gm * C + c) = z0;
          *reinterpret_cast<float4*>(a.z + (size_t)gm * C + HALF + c) = z1;
        }
        if (a.z_bct) {                                             // the unsqueeze: straight into [B, 80, T] (pre-zeroed by the caller)
          const int b = (int)a.rowbatch[gm], t = a.rowframe[gm];
          if (t >= 0 && t < a.len[b]) { fr::sq_scatter4(a.z_bct, b, t, c, a.T, HALF, z0); fr::sq_scatter4(a.z_bct, b, t, HALF + c, a.T, HALF, z1); }
        }
        *reinterpret_cast<float4*>(a.logs_raw + (size_t)gm * HALF + c) = lr;       // the backward needs logs only
        const float s = (lg[0] + lg[1] + lg[2] + lg[3]) * rm;
        if (s != 0.0f) atomicAdd(rowsum + row, s);
      }
      if (HEAD) {
        *reinterpret_cast<float4*>(Zt + row * ZP + c) = z0;
        *reinterpret_cast<float4*>(Zt + row * ZP + HALF + c) = z1;
      }
    }
    __syncthreads();
    PH(6);
    // (the per-utterance log-det atomics are issued at the very end of the kernel: vector-memory operations retire in order, and a
    // float atomic takes microseconds to come back — issued here, every later wait for a load waited for them too)
    if (!HEAD && wave == 0) {
      const int gm = m0 + lane < R ? m0 + lane : R - 1;
      utt_atomic_add(a.logdet, rowsum[lane], a.rowutt[gm], lane);
    }
    PH(7);
  } else {
    // first block: the squeezed mel rows are the flow state (gathered, they are ActNorm's input and kept in z for the backward)
    first_rows<false>(a.y_bct, a.x_in, a.z, a.rowbatch, a.rowframe, a.len, a.T, m0, R,
               [&](int row, int c, const float4& v) { *reinterpret_cast<float4*>(Zt + row * ZP + c) = v; });
    __syncthreads();
  }
  if (!HEAD) return;

  // ActNorm + InvConvNear of the next block on (row, channel group g)
  bf16_t* X0t = reinterpret_cast<bf16_t*>(smem + F_AS);      // At is dead: every wave is past the end conv
  WRing<3, HALF / 16> ring3;                                 // the start conv's weights fly under the ActNorm / InvConvNear phase
  gemm_prefetch<3, HALF / 16>(static_cast<const bf16_t*>(a.w_start), a.ks_start, 3 * wn, lane, ring3);
  {
    // thread = (channel group g, row phase): the group's ActNorm scale / bias are formed ONCE per thread (as items tid + 256 k every
    // item had another group: eight parameter loads and four exponentials per item, 8 k of the launch's 47 k cycles)
    float Wm[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) Wm[i] = a.w_ic[i];
    bf16_t* y0b = static_cast<bf16_t*>(a.y0_bf16);
    constexpr int NPH = 256 / G;                               // 6 row phases of 40 threads (16 threads idle)
    const int g = threadIdx.x % G, ph = threadIdx.x / G;
    if (ph < NPH) {
      int ch[4]; fr::group_channels(g, HALF, ch);
      const float el[4] = {__expf(a.an_logs[ch[0]]), __expf(a.an_logs[ch[1]]), __expf(a.an_logs[ch[2]]), __expf(a.an_logs[ch[3]])};
      const float bs[4] = {a.an_bias[ch[0]], a.an_bias[ch[1]], a.an_bias[ch[2]], a.an_bias[ch[3]]};
#pragma unroll
      for (int k = 0; k < (BM + NPH - 1) / NPH; ++k) {
        const int row = ph + NPH * k, gm = m0 + row;
        if (row < BM) {
          const float rm = Rm[row];
          const float2 xa = *reinterpret_cast<const float2*>(Zt + row * ZP + 2 * g);
          const float2 xb = *reinterpret_cast<const float2*>(Zt + row * ZP + HALF + 2 * g);
          const float xv[4] = {xa.x, xa.y, xb.x, xb.y};
          float o[4];
          fr::actnorm_invconv_fwd(xv, el, bs, Wm, rm, o);
          const uint32_t p01 = pack2bf(o[0], o[1]);
          if (gm < R) {
            *reinterpret_cast<float2*>(a.y_next + (size_t)gm * C + 2 * g) = make_float2(o[0], o[1]);
            *reinterpret_cast<float2*>(a.y_next + (size_t)gm * C + HALF + 2 * g) = make_float2(o[2], o[3]);
            *reinterpret_cast<uint32_t*>(y0b + (size_t)gm * HALF + 2 * g) = p01;
          }
          *reinterpret_cast<uint32_t*>(X0t + row * XP + 2 * g) = p01;
        }
      }
    }
  }
  __syncthreads();
  PH(8);
  // start conv through the dead m | logs tile
  start_conv_stage<true>(static_cast<const bf16_t*>(a.w_start), a.ks_start, ring3, X0t, Bs + 2 * H, rm_l, reinterpret_cast<bf16_t*>(smem + F_O),
                   static_cast<bf16_t*>(a.h_next), m0, R, ln);
  if (TAIL && wave == 0) {                                   // the coupling's log-det (row sums folded in LDS above)
    const int gm = m0 + lane < R ? m0 + lane : R - 1;
    utt_atomic_add(a.logdet, rowsum[lane], a.rowutt[gm], lane);
  }
  if (blockIdx.x == 0) {                                     // ActNorm + InvConvNear's log-det
    const float per_frame = fr::pair_logdet_per_frame(a.scal, G);
    for (int b = threadIdx.x; b < a.B; b += 256) atomicAdd(a.logdet + b, per_frame * (float)a.len[b]);
  }
  PH(11);
}

// ------------------------------------------------------------------------------------------------ backward
constexpr int PG = 2 * C + 16;                 // a workgroup's partial sums: d logs [C] | d bias [C] | d W [16]

// ActNorm / InvConvNear parameter gradients of one workgroup, from the four row phases' sums in LDS (fr::param_fold): as atomics
// (fr::param_fold_atomics), or as ONE ROW of partials per workgroup (plain stores; gt_boundary_param_reduce adds the rows up after the pass):
// 152 workgroups adding to the same 336 addresses serialise at L2 — ~10 us per launch that either sit in front of every later
// wait (issued mid-kernel) or hold the kernel open (issued at its end).  extra = this launch's log-det bookkeeping term (workgroup 0).
__device__ __forceinline__ void param_grad_partials(const gt_boundary_bwd_args& a, const float* sL, const float* sB, const float* sW, float extra)
{
  float* row = a.pg_partial + (size_t)blockIdx.x * PG;
  for (int t = threadIdx.x; t < PG; t += 256) {              // 336 values, 256 threads
    if (t < 2 * C) {
      const int c = t < C ? t : t - C, hi = c >= HALF, cc = c - HALF * hi, g = cc >> 1, k = 2 * hi + (cc & 1);
      const float* sp = t < C ? sL : sB;
      float v = fr::fold4(sp, g, k);
      if (t < C) v += extra;
      row[t] = v;
    } else {
      const int i = t - 2 * C;
      row[t] = fr::fold4W(sW, i) + (float)G * extra * a.scal[2 + i];
    }
  }
}

constexpr int B_DH = 0;                                    // d h tile [64][AP] bf16; later d wn_out tile
constexpr int B_D = BM * AP * 2;                           // fp32 gradient tile [64][ZP]
constexpr int B_DO = B_D + BM * ZP * 4;                    // d[m | logs] tile [64][AP] bf16
constexpr int B_RED = B_DO + BM * AP * 2;                  // parameter-gradient fold: sL, sB [4][64][4], sW [4][16], sred[4]
constexpr int BWD_LDS = B_RED + 2 * 4 * 64 * 4 * 4 + 4 * 16 * 4 + 16;

template <bool HEADB, bool TAILB>
__global__ __launch_bounds__(256) void gt_wn_boundary_bwd_kernel(gt_boundary_bwd_args a)
{
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int n_tiles = (a.R + BM - 1) / BM;
  if ((int)blockIdx.x >= n_tiles) { prefetch_images<false>(a.pf_ptr, a.pf_bytes, blockIdx.x - n_tiles); return; }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = lane & 31, h = lane >> 5, wm = wave >> 1, wn = wave & 1;
  const int m0 = blockIdx.x * BM, R = a.R;
  bf16_t* Dh = reinterpret_cast<bf16_t*>(smem + B_DH);
  float* Dt = reinterpret_cast<float*>(smem + B_D);
  bf16_t* Dout = reinterpret_cast<bf16_t*>(smem + B_DO);
  const Lane ln{lane, r, h, wm, wn};
  const int mrow = m0 + 32 * wm + r;
  const float rm_l = mrow < R ? a.rowmask[mrow] : 0.0f;
  PH(0);

  if (HEADB) {
    // d y0 (start conv part) = d h @ Wstart: N = 80 (blocks 0..2 of the padded image; wave wn takes 2 wn, 2 wn + 1)
    const bf16_t* dh = static_cast<const bf16_t*>(a.dh);
#pragma unroll
    for (int i = 0; i < 6; ++i) {
      const int chunk = threadIdx.x + 256 * i, row = chunk / 24, c8 = chunk - row * 24;
      const int gm = m0 + row < R ? m0 + row : R - 1;
      *reinterpret_cast<uint4*>(Dh + row * AP + c8 * 8) = *reinterpret_cast<const uint4*>(dh + (size_t)gm * H + c8 * 8);
    }
    WRing<2, H / 16> ring1;
    gemm_prefetch<2, H / 16>(static_cast<const bf16_t*>(a.w_start_d), a.ks_start_d, 2 * wn, lane, ring1);
    __syncthreads();
    PH(1);
    f32x16_t acc[2];
    acc_zero<2>(acc);
    gemm_run<2, H / 16>(static_cast<const bf16_t*>(a.w_start_d), a.ks_start_d, 2 * wn, Dh + (32 * wm + r) * AP + 8 * h, lane, ring1, acc);
#pragma unroll
    for (int bn = 0; bn < 2; ++bn)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int n = 32 * (2 * wn + bn) + 8 * g + 4 * h;
        if (n < HALF)
          *reinterpret_cast<float4*>(Dt + (32 * wm + r) * ZP + n) = make_float4(acc[bn][4 * g], acc[bn][4 * g + 1], acc[bn][4 * g + 2], acc[bn][4 * g + 3]);
      }
    __syncthreads();
    PH(2);
    // ActNorm + InvConvNear backward: wave = row phase (rows ph, ph + 4, ..), lane = channel group
    float* sL = reinterpret_cast<float*>(smem + B_RED);
    float* sB = sL + 4 * 64 * 4;
    float* sW = sB + 4 * 64 * 4;
    float* sred = sW + 4 * 16;
    float extra = 0.f;
    if (blockIdx.x == 0) {                                   // backward of the log-det bookkeeping
      const float sv = fr::dlogdet_len_sum(a.dlogdet, a.len, a.B, sred);
      if (a.pg_partial) extra = sv;
      else fr::pair_logdet_bwd_atomics(a.d_an_logs, a.d_w_ic, a.scal, sv, C);
    }
    const int g = lane, ph = wave;
    float accW[16], accL[4] = {0, 0, 0, 0}, accB[4] = {0, 0, 0, 0};
#pragma unroll
    for (int i = 0; i < 16; ++i) accW[i] = 0.f;
    if (g < G) {
      int ch[4]; fr::group_channels(g, HALF, ch);
      float el[4], bs[4], Wm[16];
#pragma unroll
      for (int k = 0; k < 4; ++k) { el[k] = __expf(a.an_logs[ch[k]]); bs[k] = a.an_bias[ch[k]]; }
#pragma unroll
      for (int i = 0; i < 16; ++i) Wm[i] = a.w_ic[i];
      const float* __restrict__ xp = a.x;
      const float* __restrict__ dip = a.dx_in;
#pragma unroll
      for (int rb = 0; rb < BM / 4; rb += 8) {               // this wave's 16 rows in two batches: the batch's loads fly together
        float2 xa[8], xb[8], da[8], db[8];
        float rmv[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          const int row = ph + 4 * (rb + u), gm = m0 + row < R ? m0 + row : R - 1;
          xa[u] = *reinterpret_cast<const float2*>(xp + (size_t)gm * C + 2 * g);
          xb[u] = *reinterpret_cast<const float2*>(xp + (size_t)gm * C + HALF + 2 * g);
          da[u] = *reinterpret_cast<const float2*>(dip + (size_t)gm * C + 2 * g);          // identity path of d y0
          db[u] = *reinterpret_cast<const float2*>(dip + (size_t)gm * C + HALF + 2 * g);
          rmv[u] = m0 + row < R ? a.rowmask[gm] : 0.0f;
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          const int row = ph + 4 * (rb + u), gm = m0 + row;
          const float rm = rmv[u];
          const float2 ds = *reinterpret_cast<const float2*>(Dt + row * ZP + 2 * g);
          const float xv[4] = {xa[u].x, xa[u].y, xb[u].x, xb[u].y};
          const float dym[4] = {(da[u].x + ds.x) * rm, (da[u].y + ds.y) * rm, db[u].x * rm, db[u].y * rm};
          // (fr::actnorm_invconv_bwd's text: through the leaf other pairs are packed, other products contract, the last bits change)
          float av[4], d_a[4], dxv[4];
#pragma unroll
          for (int k = 0; k < 4; ++k) av[k] = bs[k] + el[k] * xv[k];
#pragma unroll
          for (int i = 0; i < 4; ++i) d_a[i] = Wm[i] * dym[0] + Wm[4 + i] * dym[1] + Wm[8 + i] * dym[2] + Wm[12 + i] * dym[3];
#pragma unroll
          for (int o = 0; o < 4; ++o)
#pragma unroll
            for (int i = 0; i < 4; ++i) accW[o * 4 + i] += dym[o] * av[i];
#pragma unroll
          for (int k = 0; k < 4; ++k) { accB[k] += d_a[k]; accL[k] += d_a[k] * xv[k] * el[k]; dxv[k] = d_a[k] * el[k]; }
          if (TAILB) {
            *reinterpret_cast<float2*>(Dt + row * ZP + 2 * g) = make_float2(dxv[0], dxv[1]);
            *reinterpret_cast<float2*>(Dt + row * ZP + HALF + 2 * g) = make_float2(dxv[2], dxv[3]);
          } else if (gm < R) {
            if (a.dx_bct) {                                        // the unsqueeze of the decoder's input gradient
              const int b = (int)a.rowbatch[gm], t = a.rowframe[gm];
              if (t >= 0 && t < a.len[b]) {                      // (fr::unsq_scatter_group's text: through the leaf <1,0>'s row loads merge
                float* d0 = a.dx_bct + ((size_t)b * HALF + 2 * g) * a.T + 2 * t;   // otherwise and its launch is 0.2 - 0.5 us slower)
                d0[0] = dxv[0]; d0[(size_t)a.T] = dxv[1]; d0[1] = dxv[2]; d0[(size_t)a.T + 1] = dxv[3];
              }
            } else {
              *reinterpret_cast<float2*>(a.dx_out + (size_t)gm * C + 2 * g) = make_float2(dxv[0], dxv[1]);
              *reinterpret_cast<float2*>(a.dx_out + (size_t)gm * C + HALF + 2 * g) = make_float2(dxv[2], dxv[3]);
            }
          }
        }
      }
    }
    PH(3);
    // one atomic per channel per workgroup (same-address float atomics serialise at L2): fold the row phases in LDS
    fr::param_fold(sL, sB, sW, ph, g, accL, accB, accW);
    __syncthreads();
    // The workgroup's 336 parameter-gradient atomics (152 workgroups add to the same 336 addresses: they serialise at L2 and take
    // microseconds to retire) are issued at the END of the kernel: vector-memory operations retire in order, so issued here every
    // later wait for a load — the coupling's operands, the next weight fragments — waited for them too (10 k of the launch's 58 k
    // cycles, tools/wn_boundary_phases.py).  The folded sums stay in their LDS region (nothing below reuses it).
    PH(4);
    if (a.pg_partial) param_grad_partials(a, sL, sB, sW, extra);     // plain stores: nothing later waits long for them
    if (!TAILB) {
      if (!a.pg_partial) fr::param_fold_atomics(a.d_an_logs, a.d_an_bias, a.d_w_ic, sL, sB, sW, wave, lane, G, HALF);
      return;
    }
  } else {
    // last block: the squeezed gradient of the decoder's output is d z
    first_rows<false>(a.dz_bct, a.dz_in, nullptr, a.rowbatch, a.rowframe, a.len, a.T, m0, R,
               [&](int row, int c, const float4& v) { *reinterpret_cast<float4*>(Dt + row * ZP + c) = v; });
    __syncthreads();
  }

  // coupling backward on (row, 4 channels): d x = [d z0 | d z1 exp(logs)], d m = d z1, d logs = d z1 exp(logs) y1 + d logdet
  bf16_t* dout = static_cast<bf16_t*>(a.dout);
  WRing<3, C / 16> ring2;                                    // the end conv's data-gradient weights fly under this phase
  gemm_prefetch<3, C / 16>(static_cast<const bf16_t*>(a.w_end_d), a.ks_end_d, 3 * wn, lane, ring2);
  {
    float4 lr4[5], y14[5];
    float rmv[5], dldv[5];
#pragma unroll
    for (int k = 0; k < 5; ++k) {                            // all of the phase's HBM reads first
      const int item = threadIdx.x + 256 * k, row = item / 20, c = 4 * (item - row * 20), gm = m0 + row < R ? m0 + row : R - 1;
      lr4[k] = *reinterpret_cast<const float4*>(a.logs_raw + (size_t)gm * HALF + c);
      y14[k] = *reinterpret_cast<const float4*>(a.y + (size_t)gm * C + HALF + c);
      rmv[k] = a.rowmask[gm];
      dldv[k] = a.dlogdet[a.rowutt[gm]];
    }
#pragma unroll
    for (int k = 0; k < 5; ++k) {
      const int item = threadIdx.x + 256 * k, row = item / 20, c = 4 * (item - row * 20), gm = m0 + row;
      uint2 pm = make_uint2(0, 0), pl = make_uint2(0, 0);
      if (gm < R) {
        const float rm = rmv[k];
        const float4 dz0 = *reinterpret_cast<const float4*>(Dt + row * ZP + c);
        const float4 dz1r = *reinterpret_cast<const float4*>(Dt + row * ZP + HALF + c);
        const float dld = dldv[k] * rm;
        const float dz1[4] = {dz1r.x * rm, dz1r.y * rm, dz1r.z * rm, dz1r.w * rm};
        const float lraw[4] = {lr4[k].x, lr4[k].y, lr4[k].z, lr4[k].w}, y1v[4] = {y14[k].x, y14[k].y, y14[k].z, y14[k].w};
        float dx1[4], dlg[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          float dl_draw;
          const float lg = fr::coupling_lg(lraw[j], a.sigmoid_scale, dl_draw);
          fr::coupling_bwd(dz1[j], lg, dl_draw, y1v[j], dld, dx1[j], dlg[j]);
        }
        *reinterpret_cast<float4*>(a.dx_out + (size_t)gm * C + c) = dz0;
        *reinterpret_cast<float4*>(a.dx_out + (size_t)gm * C + HALF + c) = make_float4(dx1[0], dx1[1], dx1[2], dx1[3]);
        pm = pack4(dz1[0], dz1[1], dz1[2], dz1[3]);
        pl = pack4(dlg[0], dlg[1], dlg[2], dlg[3]);
        *reinterpret_cast<uint2*>(dout + (size_t)gm * C + c) = pm;
        *reinterpret_cast<uint2*>(dout + (size_t)gm * C + HALF + c) = pl;
      }
      *reinterpret_cast<uint2*>(Dout + row * AP + c) = pm;
      *reinterpret_cast<uint2*>(Dout + row * AP + HALF + c) = pl;
    }
  }
  __syncthreads();
  PH(5);
  // end conv data gradient: d wn_out = (d out @ Wend) * mask   (K = 160: 10 k-steps)
  bf16_t* At = Dh;                                           // the d h tile is dead
  const bf16_t* Wsd = static_cast<const bf16_t*>(a.w_skip_d);
  constexpr int KS2 = H / 16, NS = NL * KS2;                 // skip data gradient: 4 layer windows x 12 k-steps, ONE weight stream
  uint4 ring3[RD][3];
  {
    f32x16_t acc[3];
    acc_zero<3>(acc);
    gemm_run<3, C / 16>(static_cast<const bf16_t*>(a.w_end_d), a.ks_end_d, 3 * wn, Dout + (32 * wm + r) * AP + 8 * h, lane, ring2, acc);
    PH(6);
#pragma unroll
    for (int p = 0; p < RD; ++p)                             // the skip stage's first fragments fly under this epilogue
#pragma unroll
      for (int bn = 0; bn < 3; ++bn) ring3[p][bn] = ldfrag(Wsd, (6 * (p / KS2) + 3 * wn + bn) * a.ks_skip_d + p % KS2, lane);
    // (its own copy of pack_tile<false, true>: through the shared step <false, true> takes 218 VGPRs and loses its second wave)
#pragma unroll
    for (int bn = 0; bn < 3; ++bn)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int n = 32 * (3 * wn + bn) + 8 * g + 4 * h;
        const uint2 v = pack4(acc[bn][4 * g] * rm_l, acc[bn][4 * g + 1] * rm_l, acc[bn][4 * g + 2] * rm_l, acc[bn][4 * g + 3] * rm_l);
        *reinterpret_cast<uint2*>(At + (32 * wm + r) * AP + n) = v;
      }
  }
  __syncthreads();
  PH(7);
  coop_store_rows(static_cast<bf16_t*>(a.dwn_out), H, At, m0, R);
  PH(8);
  // skip data gradient: d acts_l (skip path) = d wn_out @ Wskip_l, one layer window per pass
  // (its own ring loop, not skip_gemm's: four ACCUMULATOR windows over one resident tile, fragment address 6 (st / 12) + 3 wn + bn)
  bf16_t* via = static_cast<bf16_t*>(a.via_skip);
  const bf16_t* brow = At + (32 * wm + r) * AP + 8 * h;
#pragma unroll
  for (int l = 0; l < NL; ++l) {
    f32x16_t acc[3];
    acc_zero<3>(acc);
#pragma unroll
    for (int k0 = 0; k0 < KS2; k0 += 4) {
#pragma unroll
      for (int kk = k0; kk < k0 + 4; ++kk) {
        const int st = l * KS2 + kk;
        const bf16x8_t bfm = *reinterpret_cast<const bf16x8_t*>(brow + kk * 16);
#pragma unroll
        for (int bn = 0; bn < 3; ++bn) acc[bn] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(asfrag(ring3[st % RD][bn]), bfm, acc[bn], 0, 0, 0);
      }
      if (l * KS2 + k0 + RD < NS) {
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int kk = k0; kk < k0 + 4; ++kk) {
          const int st = l * KS2 + kk, nx = st + RD;
#pragma unroll
          for (int bn = 0; bn < 3; ++bn)
            if (nx < NS) ring3[st % RD][bn] = ldfrag(Wsd, (6 * (nx / KS2) + 3 * wn + bn) * a.ks_skip_d + nx % KS2, lane);
        }
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    // out through one of two dead tiles (the fp32 gradient tile / the d[m | logs] tile), alternating: one barrier per layer window
    bf16_t* Vst = reinterpret_cast<bf16_t*>(smem + ((l & 1) ? B_DO : B_D));
    pack_tile<false, false>(acc, nullptr, 0.0f, Vst, ln);
    __syncthreads();
    coop_store_rows(via + l * H, a.ldvs, Vst, m0, R);
    PH(9 + l);
  }
  if (HEADB && !a.pg_partial) {
    const float* sL = reinterpret_cast<const float*>(smem + B_RED);
    fr::param_fold_atomics(a.d_an_logs, a.d_an_bias, a.d_w_ic, sL, sL + 4 * 64 * 4, sL + 2 * 4 * 64 * 4, wave, lane, G, HALF);
  }
}

// rows of per-workgroup partials [n_blocks][n_wg][PG] -> += into every block's d logs / d bias / d W (one writer per address)
__global__ __launch_bounds__(384) void gt_boundary_param_reduce_kernel(const float* __restrict__ pg, int n_wg, float* const* __restrict__ dst)
{
  // grid (block of the decoder, eighth of the partial rows): 8 adders per address (one thread walking all ~150 rows took 38 dependent
  // load rounds: 20 us on the decoder's backward chain)
  const int b = blockIdx.x, t = threadIdx.x;
  if (t >= PG) return;
  const int per = (n_wg + gridDim.y - 1) / gridDim.y, w0 = blockIdx.y * per, w1 = min(n_wg, w0 + per);
  const float* p = pg + (size_t)b * n_wg * PG + t;
  float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
  int w = w0;
  for (; w + 4 <= w1; w += 4) { s0 += p[(size_t)w * PG]; s1 += p[(size_t)(w + 1) * PG]; s2 += p[(size_t)(w + 2) * PG]; s3 += p[(size_t)(w + 3) * PG]; }
  for (; w < w1; ++w) s0 += p[(size_t)w * PG];
  float* d = t < C ? dst[3 * b] + t : (t < 2 * C ? dst[3 * b + 1] + (t - C) : dst[3 * b + 2] + (t - 2 * C));
  atomicAdd(d, (s0 + s1) + (s2 + s3));
}

// ------------------------------------------------------------------------------------------------ reverse (synthesis)
// The mirror of the forward kernel for the inverse maps (models.py:765-785 with reverse=True): going from block b to block b-1,
//   [tail of block b]    acts [64, 4H] -> skip GEMM -> wn_out (bf16, LDS only) -> end conv -> m | logs -> coupling^-1 on the flow
//                        state z -> u -> InvConvNear^-1, ActNorm^-1 -> x (HBM: the flow state the next launch's tail reads)
//   [head of block b-1]  x0 = bf16(x[:, :C/2]) -> start conv (K = 80) -> h (HBM: the next WaveNet's input)
// No log-det and nothing kept for a backward: wn_out, m | logs and x0 never leave LDS.  Same tiles, pitches, weight rings and
// rounding points (bf16 acts, wn_out, x0) as the forward kernel and as the launch sequence it replaces (gt_conv_gemm_bf16 x 3,
// gt_coupling_rev, gt_actnorm_invconv_rev), whose elementwise formulas are flow_rows.h's (coupling_inv, actnorm_invconv_inv).
constexpr int REV_LDS = FWD_LDS;               // the forward's layout: acts slices / At / x0 tile, m | logs tile, u tile, biases, row mask

template <bool TAIL, bool HEAD>
__global__ __launch_bounds__(256) void gt_wn_boundary_rev_kernel(gt_boundary_rev_args a)
{
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int n_tiles = (a.R + BM - 1) / BM;
  if ((int)blockIdx.x >= n_tiles) { prefetch_images<false>(a.pf_ptr, a.pf_bytes, blockIdx.x - n_tiles); return; }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = lane & 31, h = lane >> 5, wm = wave >> 1, wn = wave & 1;
  const int m0 = blockIdx.x * BM, R = a.R;
  bf16_t* As = reinterpret_cast<bf16_t*>(smem + F_AS);
  float* Ot = reinterpret_cast<float*>(smem + F_O);
  float* Zt = reinterpret_cast<float*>(smem + F_Z);
  bf16_t* X0t = reinterpret_cast<bf16_t*>(smem + F_AS);      // the x0 tile takes At's place once the end conv is done
  const Lane ln{lane, r, h, wm, wn};
  const int mrow = m0 + 32 * wm + r;                        // this lane's row in the MFMA epilogues
  const float rm_l = mrow < R ? a.rowmask[mrow] : 0.0f;
  float* Bs = reinterpret_cast<float*>(smem + F_BIAS);
  float* Rm = Bs + 3 * H;
  stage_bias_mask<TAIL, HEAD>(Bs, a.b_skip, a.b_end, a.b_start, a.rowmask, m0, R);
  WRing<3, HALF / 16> ring3;                                 // the start conv's weights: they depend on nothing computed here

  if (TAIL) {
    u32x4_t xr[NL][6];
    load_acts(xr, static_cast<const bf16_t*>(a.acts), a.ldacts, m0, R);
    // skip GEMM: wn_out = bf16((acts @ Wskip^T + b) * mask)
    f32x16_t acc[3];
    skip_gemm<false>(xr, As, static_cast<const bf16_t*>(a.w_skip), ln, acc);
    WRing<3, H / 16> ring2;                                 // the end conv's first weight fragments fly under this epilogue
    gemm_prefetch<3, H / 16>(static_cast<const bf16_t*>(a.w_end), a.ks_end, 3 * wn, lane, ring2);
    pack_tile<true, true>(acc, Bs, rm_l, As, ln);                    // At = slice 0's region
    __syncthreads();
    // the coupling's input (the flow state the previous launch wrote) flies under the end conv
    // (written out item by item: as an array filled in a loop the ten values were given a stack slot)
    auto z_load = [&](int k, int half) {
      const int item = threadIdx.x + 256 * k, row = item / 20, c = 4 * (item - row * 20), gm = m0 + row < R ? m0 + row : R - 1;
      return *reinterpret_cast<const float4*>(a.z + (size_t)gm * C + half * HALF + c);
    };
    const float4 za0 = z_load(0, 0), za1 = z_load(1, 0), za2 = z_load(2, 0), za3 = z_load(3, 0), za4 = z_load(4, 0);
    const float4 zb0 = z_load(0, 1), zb1 = z_load(1, 1), zb2 = z_load(2, 1), zb3 = z_load(3, 1), zb4 = z_load(4, 1);
    // end conv: [m | logs] = wn_out @ Wend^T + b   (N = 160: blocks 0..4, block 5 is the image's zero padding)
    f32x16_t acc2[3];
    acc_zero<3>(acc2);
    gemm_run<3, H / 16>(static_cast<const bf16_t*>(a.w_end), a.ks_end, 3 * wn, As + (32 * wm + r) * AP + 8 * h, lane, ring2, acc2);
    if (HEAD) gemm_prefetch<3, HALF / 16>(static_cast<const bf16_t*>(a.w_start), a.ks_start, 3 * wn, lane, ring3);
    // z into the u tile (the acts slices under it are dead: every wave is past the skip GEMM); the coupling below works in place,
    // every thread on the items it writes here
    auto z_put = [&](int k, const float4& v0, const float4& v1) {
      const int item = threadIdx.x + 256 * k, row = item / 20, c = 4 * (item - row * 20);
      *reinterpret_cast<float4*>(Zt + row * ZP + c) = v0;
      *reinterpret_cast<float4*>(Zt + row * ZP + HALF + c) = v1;
    };
    z_put(0, za0, zb0); z_put(1, za1, zb1); z_put(2, za2, zb2); z_put(3, za3, zb3); z_put(4, za4, zb4);
    end_epilogue(acc2, Bs + H, Ot, ln);
    __syncthreads();
    // inverse coupling on (row, 4 channels): u = [z0 | (z1 - m) exp(-logs) mask]   (attentions.py:178-180)
#pragma unroll
    for (int k = 0; k < 5; ++k) {
      const int item = threadIdx.x + 256 * k, row = item / 20, c = 4 * (item - row * 20);
      const float rm = Rm[row];
      const float4 mm = *reinterpret_cast<const float4*>(Ot + row * ZP + c);
      const float4 lr = *reinterpret_cast<const float4*>(Ot + row * ZP + HALF + c);
      float lg[4] = {lr.x, lr.y, lr.z, lr.w}; fr::coupling_lg(lg, a.sigmoid_scale);
      const float4 z1 = *reinterpret_cast<const float4*>(Zt + row * ZP + HALF + c);
      *reinterpret_cast<float4*>(Zt + row * ZP + HALF + c) =
          make_float4(fr::coupling_inv(mm.x, lg[0], z1.x, rm), fr::coupling_inv(mm.y, lg[1], z1.y, rm),
                      fr::coupling_inv(mm.z, lg[2], z1.z, rm), fr::coupling_inv(mm.w, lg[3], z1.w, rm));
    }
    __syncthreads();
    // InvConvNear^-1 then ActNorm^-1 on (row, channel group g) (modules.py:647-652, 592-594).  thread = (group, row phase): the group's
    // sixteen weights, four scales and four biases are formed once per thread
    {
      constexpr int NPH = 256 / G;                             // 6 row phases of 40 threads (16 threads idle)
      const int g = threadIdx.x % G, ph = threadIdx.x / G;
      if (ph < NPH) {
        float Wi[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) Wi[i] = a.scal[2 + i];
        int ch[4]; fr::group_channels(g, HALF, ch);
        const float eli[4] = {__expf(-a.an_logs[ch[0]]), __expf(-a.an_logs[ch[1]]), __expf(-a.an_logs[ch[2]]), __expf(-a.an_logs[ch[3]])};
        const float bs[4] = {a.an_bias[ch[0]], a.an_bias[ch[1]], a.an_bias[ch[2]], a.an_bias[ch[3]]};
#pragma unroll
        for (int k = 0; k < (BM + NPH - 1) / NPH; ++k) {
          const int row = ph + NPH * k, gm = m0 + row;
          if (row < BM) {
            const float rm = Rm[row];
            const float2 ua = *reinterpret_cast<const float2*>(Zt + row * ZP + 2 * g);
            const float2 ub = *reinterpret_cast<const float2*>(Zt + row * ZP + HALF + 2 * g);
            const float uv[4] = {ua.x, ua.y, ub.x, ub.y};
            float o[4];
            fr::actnorm_invconv_inv<false>(uv, eli, bs, Wi, rm, o);
            if (gm < R) {
              if (a.x) {
                *reinterpret_cast<float2*>(a.x + (size_t)gm * C + 2 * g) = make_float2(o[0], o[1]);
                *reinterpret_cast<float2*>(a.x + (size_t)gm * C + HALF + 2 * g) = make_float2(o[2], o[3]);
              }
              if (!HEAD && a.x_bct) {                                // the unsqueeze: straight into [B, 80, T] (pre-zeroed by the caller)
                const int b = (int)a.rowbatch[gm], t = a.rowframe[gm];
                if (t >= 0 && t < a.len[b]) fr::unsq_scatter_group(a.x_bct, b, t, g, a.T, HALF, o);
              }
            }
            if (HEAD) *reinterpret_cast<uint32_t*>(X0t + row * XP + 2 * g) = pack2bf(o[0], o[1]);
          }
        }
      }
    }
  } else {
    // first launch of the pass: the squeezed latent rows are the flow state; only the start conv of the last block runs
    gemm_prefetch<3, HALF / 16>(static_cast<const bf16_t*>(a.w_start), a.ks_start, 3 * wn, lane, ring3);
    // (gathered, the squeezed rows also go to x: what the next launch's tail reads)
    first_rows<true>(a.z_bct, a.x_in, a.x, a.rowbatch, a.rowframe, a.len, a.T, m0, R, [&](int row, int c, const float4& v) {
      if (c < HALF) *reinterpret_cast<uint2*>(X0t + row * XP + c) = pack4(v.x, v.y, v.z, v.w);
    });
  }
  if (!HEAD) return;
  __syncthreads();
  // start conv of block b-1 through the dead m | logs tile
  start_conv_stage<false>(static_cast<const bf16_t*>(a.w_start), a.ks_start, ring3, X0t, Bs + 2 * H, rm_l, reinterpret_cast<bf16_t*>(smem + F_O),
                   static_cast<bf16_t*>(a.h_next), m0, R, ln);
}

// the three entries' launch: LDS opt-in (> 64 KB, once per process), the prefetch list's alignment, the grid, the form the halves select
template <auto K11, auto K10, auto K01, class Args>
int launch_boundary(const Args& a, bool first, bool second, int lds, void* stream, const char* who)
{
  if (gt_allow_lds<K11>(lds) || gt_allow_lds<K10>(lds) || gt_allow_lds<K01>(lds)) return GT_E_LAUNCH;
  for (int i = 0; i < 16; ++i) if (a.pf_ptr[i] && (!al16(a.pf_ptr[i]) || (a.pf_bytes[i] & 15))) return GT_E_ALIGN;
  const dim3 grid((a.R + BM - 1) / BM + (a.pf_ptr[0] ? PF_WGS : 0)), block(256);
  hipLaunchKernelGGL(first && second ? K11 : (first ? K10 : K01), grid, block, lds, static_cast<hipStream_t>(stream), a);
  return gt_launch_status(who);
}

}  // namespace

#if WNB_PHASES
extern "C" int gt_dev_wnb_phases(void* dst, size_t bytes)
{
  return hipMemcpyFromSymbol(dst, HIP_SYMBOL(g_wnb_ph), bytes < sizeof(g_wnb_ph) ? bytes : sizeof(g_wnb_ph)) == hipSuccess ? 0 : -1;
}
#endif

extern "C" int gt_wn_boundary_fwd(const gt_boundary_fwd_args* args, void* stream)
{
  if (!args) return GT_E_INVAL;
  const gt_boundary_fwd_args& a = *args;
  if (a.R < 0) return GT_E_INVAL;
  if (a.R == 0) return GT_OK;
  if (a.H != H || a.C != C || a.n_layers != NL) return GT_E_UNSUPPORTED;
  const bool tail = a.acts != nullptr, head = a.y_next != nullptr;
  if (!tail && !head) return GT_E_INVAL;
  if (!a.rowmask) return GT_E_INVAL;
  if (tail) {
    if (!a.w_skip || !a.b_skip || !a.w_end || !a.b_end || !a.y || !a.wn_out || !a.logs_raw || (!a.z && !a.z_bct) || !a.logdet || !a.rowutt) return GT_E_INVAL;
    if (a.z_bct && (head || !a.rowbatch || !a.rowframe || !a.len || a.T <= 0)) return GT_E_INVAL;
    if (a.ldacts < NL * H || (a.ldacts & 7) || a.ks_end < H / 16) return GT_E_INVAL;
    if (!al16(a.acts) || !al16(a.w_skip) || !al16(a.w_end) || !al16(a.b_skip) || !al16(a.b_end) || !al16(a.y) || !al16(a.wn_out) ||
        !al16(a.logs_raw) || !al16(a.z)) return GT_E_ALIGN;
  } else if (a.y_bct ? (!a.rowbatch || !a.rowframe || a.T <= 0) : (!a.x_in || !al16(a.x_in))) return GT_E_INVAL;
  if (head) {
    if (!a.an_logs || !a.an_bias || !a.w_ic || !a.scal || !a.len || a.B <= 0 || !a.logdet || !a.y0_bf16 || !a.w_start || !a.b_start || !a.h_next)
      return GT_E_INVAL;
    if (a.ks_start < HALF / 16) return GT_E_INVAL;
    if (!al16(a.y_next) || !al16(a.y0_bf16) || !al16(a.w_start) || !al16(a.b_start) || !al16(a.h_next)) return GT_E_ALIGN;
  }
  return launch_boundary<&gt_wn_boundary_fwd_kernel<true, true>, &gt_wn_boundary_fwd_kernel<true, false>, &gt_wn_boundary_fwd_kernel<false, true>>(
      a, tail, head, FWD_LDS, stream, __func__);
}

extern "C" int gt_boundary_rev_args_size(void) { return (int)sizeof(gt_boundary_rev_args); }

extern "C" int gt_wn_boundary_rev(const gt_boundary_rev_args* args, void* stream)
{
  if (!args) return GT_E_INVAL;
  const gt_boundary_rev_args& a = *args;
  if (a.R < 0) return GT_E_INVAL;
  if (a.R == 0) return GT_OK;
  if (a.H != H || a.C != C || a.n_layers != NL) return GT_E_INVAL;
  const bool tail = a.acts != nullptr, head = a.h_next != nullptr;
  if (!tail && !head) return GT_E_INVAL;
  if (!a.rowmask) return GT_E_INVAL;
  if ((a.z_bct || a.x_bct) && (!a.rowbatch || !a.rowframe || !a.len || a.T <= 0 || (a.T & 1))) return GT_E_INVAL;
  if (tail) {
    if (!a.w_skip || !a.b_skip || !a.w_end || !a.b_end || !a.z || !a.an_logs || !a.an_bias || !a.scal || (!a.x && !a.x_bct)) return GT_E_INVAL;
    if (a.x_bct && head) return GT_E_INVAL;                 // the unsqueeze belongs to the last launch of a pass
    if (head && !a.x) return GT_E_INVAL;
    if (a.ldacts < NL * H || (a.ldacts & 7) || a.ks_end < H / 16) return GT_E_INVAL;
    if (!al16(a.acts) || !al16(a.w_skip) || !al16(a.w_end) || !al16(a.b_skip) || !al16(a.b_end) || !al16(a.z) || !al16(a.x)) return GT_E_ALIGN;
  } else {
    if (a.z_bct ? !a.x : !a.x_in) return GT_E_INVAL;        // the squeezed rows are written out for the next launch's tail
    if (!al16(a.x_in) || !al16(a.x)) return GT_E_ALIGN;
  }
  if (head) {
    if (!a.w_start || !a.b_start || a.ks_start < HALF / 16) return GT_E_INVAL;
    if (!al16(a.w_start) || !al16(a.b_start) || !al16(a.h_next)) return GT_E_ALIGN;
  }
  return launch_boundary<&gt_wn_boundary_rev_kernel<true, true>, &gt_wn_boundary_rev_kernel<true, false>, &gt_wn_boundary_rev_kernel<false, true>>(
      a, tail, head, REV_LDS, stream, __func__);
}

extern "C" int gt_boundary_param_partials(void) { return PG; }

extern "C" int gt_boundary_param_reduce(const float* partials, int n_wg, int n_blocks, float* const* dst, void* stream)
{
  if (!partials || !dst || n_wg <= 0 || n_blocks < 0) return GT_E_INVAL;
  if (n_blocks == 0) return GT_OK;
  hipLaunchKernelGGL(gt_boundary_param_reduce_kernel, dim3(n_blocks, 8), dim3(384), 0, static_cast<hipStream_t>(stream), partials, n_wg, dst);
  return gt_launch_status(__func__);
}

extern "C" int gt_wn_boundary_bwd(const gt_boundary_bwd_args* args, void* stream)
{
  if (!args) return GT_E_INVAL;
  const gt_boundary_bwd_args& a = *args;
  if (a.R < 0) return GT_E_INVAL;
  if (a.R == 0) return GT_OK;
  if (a.H != H || a.C != C || a.n_layers != NL) return GT_E_UNSUPPORTED;
  const bool headb = a.dh != nullptr, tailb = a.dout != nullptr;
  if (!headb && !tailb) return GT_E_INVAL;
  if (!a.rowmask || (!a.dx_out && !a.dx_bct) || !al16(a.dx_out)) return GT_E_INVAL;
  if ((a.dx_bct || a.dz_bct) && (!a.rowbatch || !a.rowframe || !a.len || a.T <= 0)) return GT_E_INVAL;
  if (a.dx_bct && tailb) return GT_E_INVAL;
  if (headb) {
    if (!a.w_start_d || !a.dx_in || !a.x || !a.an_logs || !a.an_bias || !a.w_ic || !a.scal || !a.len || !a.dlogdet || a.B <= 0 ||
        !a.d_an_logs || !a.d_an_bias || !a.d_w_ic) return GT_E_INVAL;
    if (a.ks_start_d < H / 16) return GT_E_INVAL;
    if (!al16(a.dh) || !al16(a.w_start_d) || !al16(a.dx_in) || !al16(a.x)) return GT_E_ALIGN;
  } else if (!a.dz_bct && (!a.dz_in || !al16(a.dz_in))) return GT_E_INVAL;
  if (tailb) {
    if (!a.logs_raw || !a.y || !a.dlogdet || !a.rowutt || !a.w_end_d || !a.dwn_out || !a.w_skip_d || !a.via_skip) return GT_E_INVAL;
    if (a.ks_end_d < C / 16 || a.ks_skip_d < H / 16 || a.ldvs < NL * H || (a.ldvs & 7)) return GT_E_INVAL;
    if (!al16(a.logs_raw) || !al16(a.y) || !al16(a.dout) || !al16(a.w_end_d) || !al16(a.dwn_out) || !al16(a.w_skip_d) || !al16(a.via_skip))
      return GT_E_ALIGN;
  }
  return launch_boundary<&gt_wn_boundary_bwd_kernel<true, true>, &gt_wn_boundary_bwd_kernel<true, false>, &gt_wn_boundary_bwd_kernel<false, true>>(
      a, headb, tailb, BWD_LDS, stream, __func__);
}
