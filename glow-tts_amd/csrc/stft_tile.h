// What the waveform kernels share (mel_front.hip, griffin_lim.hip, gl_mel.hip): the folded analysis tile of the framed, windowed DFT
// (n_fft = win = 1024, hop = 256) and the layout of the complex-spectrum workspace.  Defined here and nowhere else.
//
// A framed, windowed DFT is a GEMM, here in exact fp32 on v_mfma_f32_32x32x2_f32 (a k-ordered fmaf chain, as in gt_logp_f32):
//
//   fold      the periodic Hann window and cos are even about n = 512, sin is odd, and w[0] = 0, so
//               re[k] = sum_{n=1..512} C[k][n] (x[n] + x[1024-n])      C[k][n] = basis[k][n], C[k][512] = basis[k][512] / 2 (exact)
//               im[k] = sum_{n=1..511} S[k][n] (x[n] - x[1024-n])      S[k][n] = basis[513+k][n]
//             K drops from 1024 to 512.  Bin 512 has no imaginary part (sin(pi n) = 0) and is a VALU dot product per frame.
//   tile      one workgroup (4 waves) = 64 frames of one utterance x all 513 bins.  The 17 152 samples the 64 frames span are staged
//             ONCE in LDS (reflected, int16 scaled by 1/32768) and the MFMA's frame operand is read from them in place: frame i,
//             sample n is word 257 i + n + (n >> 8) (one pad word per 256: the 32 frames of a ds_read_b32 lane group fall on 32 banks).
//   operands  A = the basis (bin on the lane row), straight from global memory in fragment order (gt_mel_pack: 32 bytes per lane and
//             4 K steps, cos then sin); B = the folded samples (frame on the lane column).  So an accumulator holds its frame on the
//             lane and 16 bins in its registers, cos and sin of one bin in the same lane: register e of lane half h is bin
//             acc_row(e, h) of the 32-bin tile.  Wave w walks bin tiles 4 w .. 4 w + 3.
//
// The order of every sum depends on nothing but the frame's index within its utterance.
#pragma once
#include <type_traits>
#include "common.h"

namespace gtstft {

constexpr int NFFT = 1024, HOP = 256, NBIN = 513;
constexpr int TF = 64;                                   // frames per workgroup; the spectrum workspace's frame granularity
constexpr int SPAN = (TF - 1) * HOP + NFFT;              // samples the tile spans
constexpr int LDS_FLOATS = 17220;                        // SPAN + one pad word per 256, rounded to 16 bytes
static_assert(SPAN - 1 + ((SPAN - 1) >> 8) < LDS_FLOATS, "sample buffer");

// gt_mel_pack's image (floats): basis [16 bin tiles][64 step groups][64 lanes][cos 4 | sin 4], bin 512's folded cos row [512],
// mel [16 bin tiles][4 mel tiles][64 lanes][16], mel_basis[:, 512] [128]
constexpr int OFF_NYQ = 16 * 64 * 64 * 8;
constexpr int OFF_MEL = OFF_NYQ + 512;
constexpr int OFF_MELNYQ = OFF_MEL + 16 * 4 * 64 * 16;
constexpr int PACK_FLOATS = OFF_MELNYQ + 128;

__device__ __forceinline__ int acc_row(int e, int h) { return (e & 3) + 8 * (e >> 2) + 4 * h; }

// Stage the samples of the tile that starts at frame f0 of an utterance of L samples (`row`: fp32, or int16 scaled by 1/32768):
// reflected about the utterance's own ends, the index clamped into [0, L) whatever L is.  All 256 threads; barrier is the caller's.
template <typename T>
__device__ __forceinline__ void stage_tile(float* lds, const T* __restrict__ row, int L, int f0, int tid)
{
  const int s0 = f0 * HOP - NFFT / 2;
  constexpr int TRIPS = SPAN / 256, UNR = 8;             // 67 samples per thread, 8 loads in flight at a time: a load per trip
  static_assert(TRIPS * 256 == SPAN, "whole trips");     // would pay 67 dependent memory round trips before the first MFMA
#pragma unroll
  for (int t0 = 0; t0 < TRIPS; t0 += UNR) {
    float v[UNR];
#pragma unroll
    for (int u = 0; u < UNR; ++u)
      if (t0 + u < TRIPS) {
        int s = s0 + (t0 + u) * 256 + tid;
        if (s < 0) s = -s;
        if (s >= L) s = 2 * (L - 1) - s;
        s = s < 0 ? 0 : (s > L - 1 ? L - 1 : s);
        v[u] = std::is_same<T, int16_t>::value ? (float)row[s] * (1.0f / 32768.0f) : (float)row[s];
      }
#pragma unroll
    for (int u = 0; u < UNR; ++u)
      if (t0 + u < TRIPS) {
        const int p = (t0 + u) * 256 + tid;
        lds[p + (p >> 8)] = v[u];
      }
  }
}

// Bin 512 on the VALU: thread (frame lane, quarter w) sums 128 folded samples; the caller adds the four quarters in wave order.
__device__ __forceinline__ float nyquist_partial(const float* lds, const float* __restrict__ packed, int lane, int w)
{
  float part = 0.f;
  const int base = lane * 257;
  const float* nq = packed + OFF_NYQ + w * 128;
#pragma unroll 16
  for (int m = 0; m < 128; ++m) {                        // one chain in m order; unrolled so that the LDS reads run ahead of it
    const int n = 1 + w * 128 + m, nd = NFFT - n;
    part = fmaf(nq[m], lds[base + n + (n >> 8)] + lds[base + nd + (nd >> 8)], part);
  }
  return part;
}

// The DFT of bin tile bt (32 bins) x the tile's 64 frames: ac[ft] / as[ft] = re / im of frames 32 ft + (lane & 31), bin
// 32 bt + acc_row(e, lane >> 5) in register e.  One wave; the accumulators are zeroed here.
__device__ __forceinline__ void dft_tile(const float* lds, const float* __restrict__ packed, int bt, int lane, f32x16_t (&ac)[2],
                                         f32x16_t (&as)[2])
{
  const int j = lane & 31, h = lane >> 5;
#pragma unroll
  for (int ft = 0; ft < 2; ++ft)
#pragma unroll
    for (int e = 0; e < 16; ++e) { ac[ft][e] = 0.f; as[ft][e] = 0.f; }
  const float4* ip = reinterpret_cast<const float4*>(packed) + ((size_t)bt * 64 * 64 + lane) * 2;
  // Software pipeline, pinned with scheduling barriers (left to itself the compiler sinks every load to its first use and one
  // wave per SIMD then waits out a memory round trip per group): the NEXT group's basis fragments are requested before this
  // group's 16 MFMAs, the NEXT step's four samples before this step's four MFMAs.
  const auto samples = [&](int t, float (&xa)[2], float (&xd)[2]) {     // K step t: sample n = 1 + 2 t + h and its mirror 1024 - n
    const int n = 1 + 2 * t + h, nd = NFFT - n;
    const int oa = n + (n >> 8), od = nd + (nd >> 8);
#pragma unroll
    for (int ft = 0; ft < 2; ++ft) {
      const int base = (ft * 32 + j) * 257;
      xa[ft] = lds[base + oa]; xd[ft] = lds[base + od];
    }
  };
  float4 c4 = ip[0], s4 = ip[1];
  float xa[2], xd[2];
  samples(0, xa, xd);
  for (int tg = 0; tg < 64; ++tg) {
    const int tn = tg < 63 ? tg + 1 : tg;
    const float4 nc = ip[(size_t)tn * 128], ns = ip[(size_t)tn * 128 + 1];
    const float cc[4] = {c4.x, c4.y, c4.z, c4.w}, ss[4] = {s4.x, s4.y, s4.z, s4.w};
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      float nxa[2], nxd[2];
      samples(4 * tg + s + 1, nxa, nxd);                 // step 256 (behind the last) reads inside the frame and is dropped
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int ft = 0; ft < 2; ++ft) {
        ac[ft] = __builtin_amdgcn_mfma_f32_32x32x2f32(cc[s], xa[ft] + xd[ft], ac[ft], 0, 0, 0);
        as[ft] = __builtin_amdgcn_mfma_f32_32x32x2f32(ss[s], xa[ft] - xd[ft], as[ft], 0, 0, 0);
      }
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int ft = 0; ft < 2; ++ft) { xa[ft] = nxa[ft]; xd[ft] = nxd[ft]; }
    }
    c4 = nc; s4 = ns;
  }
}

// ---- the spectrum workspace: the complex spectrum Y [513 bins][F frames] of a batch, in the FRAGMENT ORDER of the inverse's B
// operand.  Per utterance [Fp / 32 frame groups][64 bin groups][64 lanes][re 4 | im 4] with lane = 32 (bin & 1) + (frame & 31),
// word = (bin & 7) >> 1, bin group = bin >> 3 (bins 0..511), then Re of bin 512 [Fp]; Fp = F_max rounded up to TF.  Im of bins 0
// and 512 meets a zero basis row: bin 512's is not kept.  audio.spec_unpack is the Python mirror (tests).
constexpr int SPEC_GROUP_F4 = 64 * 64 * 2;               // float4s of one frame group; a bin group is 64 * 2 = 128 of them

__host__ __device__ __forceinline__ int frames_padded(int F_max) { return (F_max + TF - 1) / TF * TF; }
__host__ __device__ __forceinline__ size_t spec_row_floats(int Fp) { return (size_t)Fp * (2 * (NBIN - 1) + 1); }
// (frame group g, bin group tg, lane) -> its float4 pair in an utterance's row: [0] = re, [1] = im of the lane's four bins
__host__ __device__ constexpr size_t spec_slot(int g, int tg, int lane) { return (((size_t)g * 64 + tg) * 64 + lane) * 2; }
// what a slot holds: frame spec_frame(g, lane), and in word s of re / im bin spec_bin(tg, lane, s)
__device__ __forceinline__ int spec_frame(int g, int lane) { return g * 32 + (lane & 31); }
__device__ __forceinline__ int spec_bin(int tg, int lane, int s) { return 8 * tg + 2 * s + (lane >> 5); }
// Re of bin 512 of frame f: a float index into the row
__device__ __forceinline__ size_t spec_nyq_slot(int Fp, int f) { return (size_t)Fp * (2 * (NBIN - 1)) + f; }

}  // namespace gtstft
