// Mel inversion in front of the Griffin-Lim loop: ragged log-mel [B, n_mel, F] -> the linear magnitudes
//   mag[b][j][f] = max(sum_k mel_pinv[j][k] expf(mel[b][k][f]), 0)      [B, 513, F_max], zero from frame F_b on
// and the loop's initial complex spectrum mag (cos phi, sin phi), written directly in the fragment order gt_istft reads (the spectrum
// workspace of stft_tile.h: spec_slot / spec_frame / spec_bin / spec_nyq_slot).
//   phase      phi = pi t, t = 2 u - 1, u = ((h >> 9) + 0.5) 2^-23, h = hash_u32(randn_key(seed, 4, b) + f K1 + j K2): common.h's
//              counter generator on stream 4 (0..3 are the prior, duration, pitch and energy draws).  t is exact in fp32, so the phase is
//              a function of (seed, b, f, j) alone; (sin, cos) = sincospif(t).  Im of bin 0 is stored as gt_gl_polar stores it
//              (mag sin phi: it meets a zero basis row), Im of bin 512 has no slot.
//   sum        ONE fmaf chain over k ascending per element, on the VALU: the GEMM is 513 x n_mel MAC per frame (82 kFLOP at
//              n_mel = 80) against the loop's 2.15 MFLOP per frame and iteration — 1/26 of one iteration, 1/790 of thirty.  Its bits
//              depend on (the utterance's data, j, f) alone, never on B, F_max, the strides or the tile.
//   F_b        min(max(n_frames[b], 0), F_max): an utterance of ONE frame keeps its frame 0 in mag and spec (gt_gl_polar zeroes
//              F_b < 2); gt_istft and gt_gl_project both treat F_b < 2 as no utterance, so nothing of it reaches a sample.
// One workgroup = 32 frames x 32 bins of one utterance (wave = one bin group of 8, thread = one slot, as in gt_gl_polar_kernel): the 32
// frames' expf(mel) [n_mel][32] and the 32 bins' rows of mel_pinv [32][n_mel] are staged in LDS once, both read conflict-free (a
// half-wave reads 32 consecutive words of E, and one word of P as a broadcast).  A frame >= F_b is never loaded: its E is 0.
#include "common.h"
#include "internal.h"
#include "stft_tile.h"
#include "../../include/glowtts_hip.h"

namespace {

using namespace gtstft;

constexpr int FG = 32;                                   // frames per workgroup = one frame group of the layout
constexpr int BG = 32;                                   // bins per workgroup: 4 waves x one bin group of 8
constexpr int PS = GT_MEL_MAX_N_MEL + 1;                 // row pitch of the staged mel_pinv rows
constexpr uint32_t PHASE_STREAM = 4u;

__device__ __forceinline__ void unit_phasor(uint32_t key, int f, int j, float& sn, float& cs)
{
  const uint32_t h = hash_u32(key + (uint32_t)f * 0x9E3779B1U + (uint32_t)j * 0x85EBCA6BU);
  const float u = ((float)(h >> 9) + 0.5f) * 1.1920928955078125e-7f;
  sincospif(2.0f * u - 1.0f, &sn, &cs);
}

__global__ __launch_bounds__(256) void gt_gl_from_mel_kernel(const float* __restrict__ mel, int64_t stride_b, int64_t stride_c,
                                                             const int32_t* __restrict__ n_frames, int F_max, int Fp, int n_mel,
                                                             const float* __restrict__ pinv, uint32_t seed,
                                                             const uint32_t* __restrict__ seed_dev, float* __restrict__ mag,
                                                             float* __restrict__ spec)
{
  __shared__ float E[GT_MEL_MAX_N_MEL * FG];             // [k][frame]
  __shared__ float P[BG * PS];                           // [bin][k]
  const int b = blockIdx.y, g = blockIdx.x >> 4, bq = blockIdx.x & 15;     // frame group, bins 32 bq .. 32 bq + 31
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  int Fb = n_frames[b];
  Fb = Fb < 0 ? 0 : (Fb < F_max ? Fb : F_max);
  const int f0 = g * FG;

  const float* mb = mel + (size_t)b * stride_b;
  for (int i = tid; i < n_mel * FG; i += 256) {
    const int k = i >> 5, f = f0 + (i & 31);
    E[i] = f < Fb ? expf(mb[(size_t)k * stride_c + f]) : 0.f;
  }
  for (int i = tid; i < BG * n_mel; i += 256) {
    const int r = i / n_mel, k = i - r * n_mel;
    P[r * PS + k] = pinv[(size_t)(bq * BG) * n_mel + i];
  }
  __syncthreads();

  const uint32_t key = randn_key(seed_dev ? *seed_dev : seed, PHASE_STREAM, (uint32_t)b);
  const int tg = bq * 4 + w, fl = lane & 31, hk = lane >> 5, f = spec_frame(g, lane);
  const bool live = f < Fb;
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  const float* pr = P + (w * 8 + hk) * PS;               // bins 8 tg + 2 s + hk: rows 2 s apart
  for (int k = 0; k < n_mel; ++k) {
    const float e = E[k * FG + fl];
#pragma unroll
    for (int s = 0; s < 4; ++s) acc[s] = fmaf(pr[2 * s * PS + k], e, acc[s]);
  }
  float re[4], im[4];
  float* mo = mag + (size_t)b * NBIN * F_max;
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    const int j = spec_bin(tg, lane, s);
    const float m = live ? fmaxf(acc[s], 0.f) : 0.f;
    float sn, cs;
    unit_phasor(key, f, j, sn, cs);
    re[s] = m * cs; im[s] = m * sn;
    if (f < F_max) mo[(size_t)j * F_max + f] = m;
  }
  float* sb = spec + (size_t)b * spec_row_floats(Fp);
  float4* o = reinterpret_cast<float4*>(sb) + spec_slot(g, tg, lane);
  o[0] = make_float4(re[0], re[1], re[2], re[3]);
  o[1] = make_float4(im[0], im[1], im[2], im[3]);

  if (bq == 0 && w == 0 && hk == 0) {                    // bin 512: real in the layout; its mel_pinv row comes from global memory
    const float* p512 = pinv + (size_t)512 * n_mel;
    float a = 0.f;
    for (int k = 0; k < n_mel; ++k) a = fmaf(p512[k], E[k * FG + fl], a);
    const float m = live ? fmaxf(a, 0.f) : 0.f;
    float sn, cs;
    unit_phasor(key, f, 512, sn, cs);
    if (f < F_max) mo[(size_t)512 * F_max + f] = m;
    sb[spec_nyq_slot(Fp, f)] = m * cs;
  }
}

}  // namespace

extern "C" int gt_gl_from_mel(const float* mel, int64_t stride_b, int64_t stride_c, const int32_t* n_frames, int B, int F_max, int n_mel,
                              const float* mel_pinv, uint32_t seed, const uint32_t* seed_dev, float* mag, float* spec, void* stream)
{
  if (!mel || !n_frames || !mel_pinv || !mag || !spec || gl_shape_bad(B, F_max) ||
      n_mel <= 0 || n_mel > GT_MEL_MAX_N_MEL || stride_b < F_max || stride_c < F_max) return GT_E_INVAL;
  if (!al16(mag) || !al16(spec) || !al16(mel_pinv) || ((uintptr_t)mel & 3) || ((uintptr_t)n_frames & 3) || ((uintptr_t)seed_dev & 3))
    return GT_E_ALIGN;
  const int Fp = frames_padded(F_max);
  hipLaunchKernelGGL(gt_gl_from_mel_kernel, dim3(Fp / FG * 16, B), dim3(256), 0, static_cast<hipStream_t>(stream), mel, stride_b,
                     stride_c, n_frames, F_max, Fp, n_mel, mel_pinv, seed, seed_dev, mag, spec);
  return gt_launch_status(__func__);
}
