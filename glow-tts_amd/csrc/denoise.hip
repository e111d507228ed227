// Spectral-subtraction denoiser behind the vocoders: the analysis half of NVIDIA's WaveGlow `Denoiser`
// (denoiser.py, mode = "zeros": audio_denoised = STFT.inverse(clamp(|X| - strength bias_spec, min = 0), angle X)), every utterance of a
// ragged batch on its own, n_fft = win = 1024, hop = 256, in exact fp32 on v_mfma_f32_32x32x2_f32 (k-ordered fmaf chains).
//
//   analysis   stft_tile.h's folded DFT tile, the functions gt_mel_front_kernel and gt_gl_project_kernel run (same packed basis image,
//              same staging, K = 512): 256 threads, 64 frames per workgroup, four bin-tile passes per wave.
//   epilogue   Y = X max(|X| - c_k, 0) / |X| with c_k = strength * bias[k], in registers (re and im of a bin sit in one lane), written in
//              the spectrum workspace's order (stft_tile.h) for gt_istft; |X|^2 == 0 gives (max(-c_k, 0), 0), as atan2(0, 0) = 0 gives
//              the reference.  No atan2f / cosf / sinf.  The strength is ONE fp32 word read on the device: a replayed graph picks up a new
//              value.  The 16 c_k of a lane's bins are loaded once per pass, in front of the pass's MFMAs.
//   bin 512    real, through the four-quarter LDS reduction: y = sign(x) max(|x| - c_512, 0).
//   geometry   the vocoders' rows hold 256 max(n_b - lost, 0) samples for n_b mel frames: the analysis has Fa_b = samples_b / 256 + 1
//              frames, 0 where there is no sample.  The kernel derives Fa_b and writes it to frames_out[b] (one lane of block (0, b)):
//              gt_istft runs on frames_out at the capacity Fa_max = F_max - lost + 1.  Tiles past Fa_b write zeros and read no sample.
// Every sum's order depends on the sample's index within its utterance alone.
#include "common.h"
#include "internal.h"
#include "stft_tile.h"
#include "../../include/glowtts_hip.h"

namespace {

using namespace gtstft;

__global__ __launch_bounds__(256, 2) void gt_denoise_spec_kernel(const float* __restrict__ wav, int ld_wav,
                                                                 const float* __restrict__ bias, const float* __restrict__ strength,
                                                                 const int32_t* __restrict__ n_frames, int lost, int F_max, int Fp,
                                                                 const float* __restrict__ packed, float* __restrict__ spec,
                                                                 int32_t* __restrict__ frames_out)
{
  __shared__ float lds[LDS_FLOATS];
  const int b = blockIdx.y, f0 = blockIdx.x * TF;
  const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
  int hops = n_frames[b];
  hops = (hops < F_max ? hops : F_max) - lost;           // hops of 256 samples the vocoder wrote for this utterance
  hops = hops < ld_wav / HOP ? hops : ld_wav / HOP;
  const int Fb = hops > 0 ? hops + 1 : 0;                // analysis frames
  const int L = HOP * (Fb - 1);                          // samples of this utterance (not used where Fb == 0)
  float* sb = spec + (size_t)b * spec_row_floats(Fp);
  float4* sb4 = reinterpret_cast<float4*>(sb);
  const int g0 = f0 >> 5;                                // the tile's two frame groups: g0, g0 + 1
  if (blockIdx.x == 0 && tid == 0) frames_out[b] = Fb;

  if (f0 >= Fb) {                                        // a tile past the utterance's end: zeros, no sample is read
    const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
    float4* img = sb4 + spec_slot(g0, 0, 0);
    for (int idx = tid; idx < 2 * SPEC_GROUP_F4; idx += 256) img[idx] = z;
    if (tid < TF) sb[spec_nyq_slot(Fp, f0 + tid)] = 0.f;
    return;
  }

  const float st = strength[0];
  stage_tile(lds, wav + (size_t)b * ld_wav, L, f0, tid);
  __syncthreads();
  const float nyq_part = nyquist_partial(lds, packed, lane, w);

  // ---- the DFT: wave w, bin tiles 4 w .. 4 w + 3, 64 frames each; then Y = X max(|X| - c, 0) / |X| where it stands
  const int j = lane & 31, h = lane >> 5;
  for (int pass = 0; pass < 4; ++pass) {
    const int bt = w * 4 + pass;
    float c[16];                                         // the lane's 16 bins of this pass: requested in front of the MFMAs
#pragma unroll
    for (int e = 0; e < 16; ++e) c[e] = bias[bt * 32 + acc_row(e, h)];
    f32x16_t ac[2], as[2];
    dft_tile(lds, packed, bt, lane, ac, as);
#pragma unroll
    for (int e = 0; e < 16; ++e) c[e] *= st;
    // register e of lane half h is bin k = 32 bt + acc_row(e, h): bin group 4 bt + (e >> 2), lane 32 (e & 1) + j, word
    // 2 h + ((e & 3) >> 1) — registers e and e + 2 (e & 3 < 2) are neighbours: one 8-byte store each for re and im
#pragma unroll
    for (int ft = 0; ft < 2; ++ft) {
      const bool live = f0 + ft * 32 + j < Fb;
      float yr[16], yi[16];
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const float re = ac[ft][e], im = as[ft][e];
        const float m2 = fmaf(im, im, re * re);
        const float m = sqrtf(m2);
        const float sc = fmaxf(m - c[e], 0.f) / m;
        yr[e] = !live ? 0.f : (m2 == 0.f ? fmaxf(0.f - c[e], 0.f) : re * sc);
        yi[e] = !live || m2 == 0.f ? 0.f : im * sc;
      }
#pragma unroll
      for (int e = 0; e < 16; ++e)
        if ((e & 3) < 2) {
          float* o = reinterpret_cast<float*>(sb4 + spec_slot(g0 + ft, bt * 4 + (e >> 2), (e & 1) * 32 + j)) + 2 * h;
          *reinterpret_cast<float2*>(o) = make_float2(yr[e], yr[e + 2]);
          *reinterpret_cast<float2*>(o + 4) = make_float2(yi[e], yi[e + 2]);
        }
    }
  }
  __syncthreads();                                       // every wave is done with the samples: the buffer becomes the reduction's

  // ---- bin 512: the four quarters in wave order; it is real, so Y = sign(x) max(|x| - c, 0)
  float* nbuf = lds;                                     // [4][TF]
  nbuf[w * TF + lane] = nyq_part;
  __syncthreads();
  if (tid < TF) {
    const int f = f0 + tid;
    const float x = ((nbuf[tid] + nbuf[TF + tid]) + nbuf[2 * TF + tid]) + nbuf[3 * TF + tid];
    float y = 0.f;
    if (f < Fb) {
      const float m = fmaxf(fabsf(x) - st * bias[NBIN - 1], 0.f);
      y = x < 0.f ? -m : m;
    }
    sb[spec_nyq_slot(Fp, f)] = y;
  }
}

}  // namespace

extern "C" int gt_denoise_spec_args_size(void) { return (int)sizeof(gt_denoise_spec_args); }

extern "C" int gt_denoise_spec(const gt_denoise_spec_args* a, void* stream)
{
  if (!a) return GT_E_INVAL;
  if (!a->wav || !a->bias || !a->strength || !a->n_frames || !a->mel_packed || !a->spec || !a->frames_out) return GT_E_INVAL;
  if (a->lost < 0 || a->lost > 1 || a->ld_wav <= 0 || gl_shape_bad(a->B, a->F_max)) return GT_E_INVAL;
  const int Fa_max = a->F_max - a->lost + 1;             // the analysis frames of a full row
  if (gl_shape_bad(a->B, Fa_max)) return GT_E_INVAL;
  if (a->n_fft != NFFT || a->hop != HOP || a->win != NFFT) return GT_E_UNSUPPORTED;
  if (!al16(a->wav) || !al16(a->mel_packed) || !al16(a->spec) || (a->ld_wav & 3)) return GT_E_ALIGN;
  if (((uintptr_t)a->bias & 3) || ((uintptr_t)a->strength & 3) || ((uintptr_t)a->n_frames & 3) || ((uintptr_t)a->frames_out & 3))
    return GT_E_ALIGN;
  const int Fp = frames_padded(Fa_max);
  hipLaunchKernelGGL(gt_denoise_spec_kernel, dim3(Fp / TF, a->B), dim3(256), 0, GT_ST(stream), a->wav, a->ld_wav, a->bias, a->strength,
                     a->n_frames, a->lost, a->F_max, Fp, static_cast<const float*>(a->mel_packed), a->spec, a->frames_out);
  return gt_launch_status(__func__);
}
