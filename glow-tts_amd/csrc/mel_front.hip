// Device mel front end: padded waveforms -> log-mel, energy and (optionally) the magnitude spectrogram in ONE kernel,
// with the semantics of the reference's TacotronSTFT (stft.py:78-101 CUDA branch, commons.py:298-317, audio_processing.py:78-84)
// applied to every utterance on its own: reflect padding about the utterance's own ends, n_fft = win = 1024, hop = 256.
//
// The framed, windowed DFT in exact fp32 is stft_tile.h's folded tile (the fold, the staged 64-frame tile, the MFMA operands and the
// packed image's offsets are described and defined there; gt_gl_project_kernel runs the same functions).  This kernel's own:
//
//   mag       an accumulator holds its frame on the lane and 16 bins in its registers, cos and sin of one bin in the same lane:
//             mag = sqrt(re^2 + im^2) needs no exchange,
//   mel       and the 32 x 32 magnitude tile IS the B operand of the projection mel[m][f] += melb[m][bin] mag[bin][f] (register e of
//             lane half h is bin acc_row(e, h): the mel image is packed in that k order) — no LDS, no transposition.
//   walk      wave w walks bin tiles 4 w .. 4 w + 3 and keeps the partial energy and mel of its 128 bins in registers; the four
//             partials meet in LDS (the sample buffer, behind a barrier) in the order ((w0 + w1) + w2) + w3, then bin 512, then
//             sqrt / log.  No atomics; the order of every sum depends on nothing but the frame's index within its utterance.
#include "common.h"
#include "internal.h"
#include "stft_tile.h"
#include "../../include/glowtts_hip.h"

namespace {

using namespace gtstft;

static_assert(4 * 32 * TF + 2 * 4 * TF <= LDS_FLOATS, "the reduction buffers alias the sample buffer");

__global__ __launch_bounds__(256) void gt_mel_pack_kernel(const float* __restrict__ basis, const float* __restrict__ melb, int n_mel,
                                                          float* __restrict__ out)
{
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= PACK_FLOATS) return;
  float v;
  if (i < OFF_NYQ) {
    const int s = i & 3, cs = (i >> 2) & 1, lane = (i >> 3) & 63, tg = (i >> 9) & 63, bt = i >> 15;
    const int bin = bt * 32 + (lane & 31), n = 1 + 2 * (4 * tg + s) + (lane >> 5);
    if (cs == 0) v = basis[(size_t)bin * NFFT + n] * (n == 512 ? 0.5f : 1.0f);
    else v = n == 512 ? 0.f : basis[(size_t)(NBIN + bin) * NFFT + n];
  } else if (i < OFF_MEL) {
    const int n = i - OFF_NYQ + 1;
    v = basis[(size_t)512 * NFFT + n] * (n == 512 ? 0.5f : 1.0f);
  } else if (i < OFF_MELNYQ) {
    const int k = i - OFF_MEL, e = k & 15, lane = (k >> 4) & 63, mt = (k >> 10) & 3, bt = k >> 12;
    const int m = mt * 32 + (lane & 31), bin = bt * 32 + acc_row(e, lane >> 5);
    v = m < n_mel ? melb[(size_t)m * NBIN + bin] : 0.f;
  } else {
    const int m = i - OFF_MELNYQ;
    v = m < n_mel ? melb[(size_t)m * NBIN + 512] : 0.f;
  }
  out[i] = v;
}

template <int MT>                                        // 32-row tiles of the mel projection: 3 (n_mel <= 96) or 4
__global__ __launch_bounds__(256, 2) void gt_mel_front_kernel(const void* __restrict__ wav, int is_i16, int ld_wav,
                                                              const int32_t* __restrict__ wav_len, int F_max,
                                                              const float* __restrict__ packed, int n_mel, float clip,
                                                              float* __restrict__ mel, float* __restrict__ energy, float* __restrict__ mag)
{
  __shared__ float lds[LDS_FLOATS];
  const int b = blockIdx.y, f0 = blockIdx.x * TF;
  const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
  int L = wav_len[b];
  L = L < ld_wav ? L : ld_wav;
  int Fb = L > 0 ? 1 + L / HOP : 0;                      // frames of this utterance; everything from Fb on is written as 0
  Fb = Fb < F_max ? Fb : F_max;
  float* melo = mel + (size_t)b * n_mel * F_max;
  float* eno = energy + (size_t)b * F_max;
  float* mago = mag ? mag + (size_t)b * NBIN * F_max : nullptr;

  if (f0 >= Fb) {                                        // a tile past the utterance's end: zeros, no sample is read
    const int rows = n_mel + 1 + (mago ? NBIN : 0);
    for (int idx = tid; idx < rows * TF; idx += 256) {
      const int row = idx >> 6, f = f0 + (idx & 63);
      if (f >= F_max) continue;
      if (row < n_mel) melo[(size_t)row * F_max + f] = 0.f;
      else if (row == n_mel) eno[f] = 0.f;
      else mago[(size_t)(row - n_mel - 1) * F_max + f] = 0.f;
    }
    return;
  }

  if (is_i16) stage_tile(lds, static_cast<const int16_t*>(wav) + (size_t)b * ld_wav, L, f0, tid);
  else stage_tile(lds, static_cast<const float*>(wav) + (size_t)b * ld_wav, L, f0, tid);
  __syncthreads();
  const float nyq_part = nyquist_partial(lds, packed, lane, w);       // bin 512: the quarters meet in the reduction

  // ---- the DFT: wave w, bin tiles 4 w .. 4 w + 3, 64 frames each
  const int j = lane & 31, h = lane >> 5;
  float esum[2] = {0.f, 0.f};
  f32x16_t macc[2][MT];
#pragma unroll
  for (int ft = 0; ft < 2; ++ft)
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
      for (int e = 0; e < 16; ++e) macc[ft][mt][e] = 0.f;

  for (int pass = 0; pass < 4; ++pass) {
    const int bt = w * 4 + pass;
    f32x16_t ac[2], as[2];
    dft_tile(lds, packed, bt, lane, ac, as);
    // magnitudes of the tile: frame on the lane, bin bt * 32 + acc_row(e, h) in register e
    float mg[2][16];
#pragma unroll
    for (int ft = 0; ft < 2; ++ft) {
      const int f = f0 + ft * 32 + j;
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        mg[ft][e] = sqrtf(ac[ft][e] * ac[ft][e] + as[ft][e] * as[ft][e]);
        esum[ft] = fmaf(mg[ft][e], mg[ft][e], esum[ft]);
        if (mago && f < F_max) mago[(size_t)(bt * 32 + acc_row(e, h)) * F_max + f] = f < Fb ? mg[ft][e] : 0.f;
      }
    }
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
      const float4* mp = reinterpret_cast<const float4*>(packed + OFF_MEL) + (((size_t)bt * 4 + mt) * 64 + lane) * 4;
      const float4 m0 = mp[0], m1 = mp[1], m2 = mp[2], m3 = mp[3];
      const float ma[16] = {m0.x, m0.y, m0.z, m0.w, m1.x, m1.y, m1.z, m1.w, m2.x, m2.y, m2.z, m2.w, m3.x, m3.y, m3.z, m3.w};
#pragma unroll
      for (int ft = 0; ft < 2; ++ft)
#pragma unroll
        for (int e = 0; e < 16; ++e) macc[ft][mt] = __builtin_amdgcn_mfma_f32_32x32x2f32(ma[e], mg[ft][e], macc[ft][mt], 0, 0, 0);
    }
  }
  __syncthreads();                                       // every wave is done with the samples: the buffer becomes the reduction's

  // ---- the four waves' partials, in wave order; then bin 512, sqrt and log
  float* melbuf = lds;                                   // [MT * 32][TF]
  float* ebuf = lds + 4 * 32 * TF;                       // [4][TF]
  float* nbuf = ebuf + 4 * TF;                           // [4][TF]
#pragma unroll
  for (int ft = 0; ft < 2; ++ft) {
    const float e2 = esum[ft] + __shfl_xor(esum[ft], 32);
    if (h == 0) ebuf[w * TF + ft * 32 + j] = e2;
  }
  nbuf[w * TF + lane] = nyq_part;
  for (int r = 0; r < 4; ++r) {
    if (w == r) {
#pragma unroll
      for (int ft = 0; ft < 2; ++ft)
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
          for (int e = 0; e < 16; ++e) {
            const int idx = (mt * 32 + acc_row(e, h)) * TF + ft * 32 + j;
            melbuf[idx] = r == 0 ? macc[ft][mt][e] : melbuf[idx] + macc[ft][mt][e];
          }
    }
    __syncthreads();
  }
  const float* melnyq = packed + OFF_MELNYQ;
  for (int idx = tid; idx < (n_mel + 2) * TF; idx += 256) {
    const int row = idx >> 6, fl = idx & 63, f = f0 + fl;
    if (f >= F_max) continue;
    const float m512 = fabsf(((nbuf[fl] + nbuf[TF + fl]) + nbuf[2 * TF + fl]) + nbuf[3 * TF + fl]);
    if (row < n_mel) {
      const float v = fmaf(melnyq[row], m512, melbuf[row * TF + fl]);
      melo[(size_t)row * F_max + f] = f < Fb ? logf(fmaxf(v, clip)) : 0.f;
    } else if (row == n_mel) {
      const float e2 = fmaf(m512, m512, ((ebuf[fl] + ebuf[TF + fl]) + ebuf[2 * TF + fl]) + ebuf[3 * TF + fl]);
      eno[f] = f < Fb ? sqrtf(e2) : 0.f;
    } else if (mago) {
      mago[(size_t)512 * F_max + f] = f < Fb ? m512 : 0.f;
    }
  }
}


}  // namespace

extern "C" size_t gt_mel_pack_bytes(void) { return (size_t)PACK_FLOATS * sizeof(float); }
extern "C" int gt_mel_tile_frames(void) { return TF; }

extern "C" int gt_mel_pack(const float* basis, const float* mel_basis, int n_fft, int n_mel, void* packed, void* stream)
{
  if (!basis || !mel_basis || !packed || n_mel <= 0) return GT_E_INVAL;
  if (n_fft != NFFT || n_mel > GT_MEL_MAX_N_MEL) return GT_E_UNSUPPORTED;
  if (!al16(basis) || !al16(mel_basis) || !al16(packed)) return GT_E_ALIGN;
  hipLaunchKernelGGL(gt_mel_pack_kernel, dim3((PACK_FLOATS + 255) / 256), dim3(256), 0, GT_ST(stream), basis, mel_basis, n_mel,
                     static_cast<float*>(packed));
  return gt_launch_status(__func__);
}

extern "C" int gt_mel_spectrogram(const void* wav, int is_i16, int ld_wav, const int32_t* wav_len, int B, int F_max,
                                  const void* packed, int n_fft, int hop, int win, int n_mel, float clip,
                                  float* mel, float* energy, float* mag, void* stream)
{
  if (!wav || !wav_len || !packed || !mel || !energy) return GT_E_INVAL;
  if (B <= 0 || B > GT_MEL_MAX_B || F_max <= 0 || F_max > GT_MEL_MAX_FRAMES || ld_wav <= 0 || n_mel <= 0) return GT_E_INVAL;
  if (n_fft != NFFT || hop != HOP || win != NFFT || n_mel > GT_MEL_MAX_N_MEL) return GT_E_UNSUPPORTED;
  if (!al16(wav) || !al16(packed) || !al16(mel) || !al16(energy) || !al16(mag) || ((uintptr_t)wav_len & 3) || (ld_wav & 3)) return GT_E_ALIGN;
  const dim3 grid((F_max + TF - 1) / TF, B);
  const float* pk = static_cast<const float*>(packed);
  if (n_mel <= 96)
    hipLaunchKernelGGL(gt_mel_front_kernel<3>, grid, dim3(256), 0, GT_ST(stream), wav, is_i16, ld_wav, wav_len, F_max, pk, n_mel, clip, mel, energy, mag);
  else
    hipLaunchKernelGGL(gt_mel_front_kernel<4>, grid, dim3(256), 0, GT_ST(stream), wav, is_i16, ld_wav, wav_len, F_max, pk, n_mel, clip, mel, energy, mag);
  return gt_launch_status(__func__);
}
