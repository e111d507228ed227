// Device waveform back end: the reference's STFT.inverse (stft.py:121-148 CUDA branch, audio_processing.py:7-56)
// and the two halves of a Griffin-Lim iteration (audio_processing.py:59-75), every utterance of a ragged batch on its own,
// n_fft = win = 1024, hop = 256, in exact fp32 on v_mfma_f32_32x32x2_f32 (k-ordered fmaf chains).
//
//   spectrum   the complex spectrum Y [513 bins][F frames] of a batch lives in a device workspace in the FRAGMENT ORDER of the
//              inverse's B operand (stft_tile.h: the layout is defined there, every index below goes through spec_slot /
//              spec_nyq_slot but gt_istft's two fragment pointers, which are pinned to spec_slot by a static_assert).  gt_gl_polar
//              and gt_gl_project write it (zeros from frame F_b on), gt_istft reads it with two 16-byte loads per lane, frame
//              tile and 4 K steps.
//   project    the analysis half = stft_tile.h's folded DFT tile, the functions gt_mel_front_kernel runs (same packed basis image,
//              same staging, K = 512), with the epilogue Y = M X / |X| in registers (re and im of a bin sit in one lane);
//              |X|^2 == 0 gives (M, 0).  No atan2f / cosf / sinf.
//   istft      the inverse folds like the forward: the windowed inverse basis is even (cos rows) / odd (sin rows) about n = 512, so
//                a[n] = sum_k ibc[k][n] Re[k],  b[n] = sum_k ibs[k][n] Im[k],  x[n] = a[n] + b[n],  x[1024 - n] = a[n] - b[n]
//              for n = 1..512 (x[0] = 0: w[0] = 0; b[512] = 0).  One workgroup = 64 frames h0 - 1 .. h0 + 62 of one utterance = the
//              61 output hops h0 .. h0 + 60 that lie wholly inside them (a 3-frame halo is recomputed: no atomics, no second pass).
//              n is tiled: in pass p (0..3) wave w owns the 32 columns n = r, 256 - r, 256 + r, 512 - r (w = 0..3) of
//              r = 32 p + 1 .. 32 p + 32 — with their mirrors exactly the columns the output offsets r and 256 - r of every hop
//              need (r = 128 is its own partner: its two spare columns are n = 256 and n = 512, which offset 0 needs).  The pass's
//              8 x 32 x 64 values go through LDS ([row][65]: conflict-free both ways) and are overlap-added from there:
//              out[256 h + r] = 4 (x_{h-1}[768 + r] + x_h[512 + r] + x_{h+1}[256 + r] + x_{h+2}[r]) / env, frames outside
//              [0, F_b) skipped, env = the same frames' w^2 summed in the same (ascending) order — the reference's window_sumsquare.
// Every sum's order depends on the sample's index within its utterance alone.
#include <cfloat>
#include "common.h"
#include "internal.h"
#include "stft_tile.h"
#include "../../include/glowtts_hip.h"

namespace {

using namespace gtstft;                                  // TF frames per workgroup (both kernels), the tile, the spectrum layout

constexpr int TH = TF - 3;                               // output hops an istft workgroup completes

// the inverse's packed image (floats): basis [16 column tiles][64 bin groups][64 lanes][cos 4 | sin 4], bin 512's row by
// [column tile][row] [512], the squared window [1024]
constexpr int INV_OFF_NYQ = 16 * 64 * 64 * 8;
constexpr int INV_OFF_W2 = INV_OFF_NYQ + 512;
constexpr int INV_PACK_FLOATS = INV_OFF_W2 + NFFT;
constexpr int XS = TF + 1;                               // row pitch of the pass buffer
constexpr int XBUF_FLOATS = 4 * 2 * 32 * XS;

// column n of row i of column tile t = 4 pass + wave
__device__ __forceinline__ int tile_n(int t, int i)
{
  const int w = t & 3, r = 1 + 32 * (t >> 2) + i;
  return w == 0 ? r : w == 1 ? (r == 128 ? 256 : 256 - r) : w == 2 ? 256 + r : (r == 128 ? 512 : 512 - r);
}

// sample n (1..1023) of a frame -> its row of the pass buffer, (2 wave + mirror) * 32 + row; the pass is that of its offset
__device__ __forceinline__ int src_row(int n)
{
  const int pm = n > 512;
  if (pm) n = NFFT - n;
  int w, r;
  if (n == 256) { w = 1; r = 128; }
  else if (n == 512) { w = 3; r = 128; }
  else if (n <= 128) { w = 0; r = n; }
  else if (n < 256) { w = 1; r = 256 - n; }
  else if (n <= 384) { w = 2; r = n - 256; }
  else { w = 3; r = 512 - n; }
  return (w * 2 + pm) * 32 + ((r - 1) & 31);
}

__global__ __launch_bounds__(256) void gt_gl_pack_kernel(const float* __restrict__ ib, float* __restrict__ out)
{
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= INV_PACK_FLOATS) return;
  float v;
  if (i < INV_OFF_NYQ) {
    const int s = i & 3, cs = (i >> 2) & 1, lane = (i >> 3) & 63, tg = (i >> 9) & 63, t = i >> 15;
    const int n = tile_n(t, lane & 31), k = 2 * (4 * tg + s) + (lane >> 5);
    if (cs == 0) v = ib[(size_t)k * NFFT + n];
    else v = n == 512 ? 0.f : ib[(size_t)(NBIN + k) * NFFT + n];
  } else if (i < INV_OFF_W2) {
    const int idx = i - INV_OFF_NYQ;
    v = ib[(size_t)512 * NFFT + tile_n(idx >> 5, idx & 31)];
  } else {
    const float w = ib[i - INV_OFF_W2] * 4096.0f;            // row 0 of the inverse basis is the window / (1024 * 4): exact
    v = w * w;
  }
  out[i] = v;
}

// one thread = one slot of the spectrum image: bins spec_bin(tg, lane, s), s = 0..3, of frame spec_frame(g, lane)
__global__ __launch_bounds__(256) void gt_gl_polar_kernel(const float* __restrict__ mag, const float* __restrict__ phase,
                                                          const int32_t* __restrict__ n_frames, int F_max, int Fp,
                                                          float* __restrict__ spec)
{
  const int b = blockIdx.y;
  const int idx = blockIdx.x * 256 + threadIdx.x;         // [Fp / 32][64][64]
  const int lane = idx & 63, tg = (idx >> 6) & 63, g = idx >> 12;
  const int f = spec_frame(g, lane);
  int Fb = n_frames[b];
  Fb = Fb < 2 ? 0 : (Fb < F_max ? Fb : F_max);
  float* sb = spec + (size_t)b * spec_row_floats(Fp);
  float re[4] = {0.f, 0.f, 0.f, 0.f}, im[4] = {0.f, 0.f, 0.f, 0.f};
  if (f < Fb) {
    float m[4], p[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const size_t a = ((size_t)b * NBIN + spec_bin(tg, lane, s)) * F_max + f;
      m[s] = mag[a]; p[s] = phase[a];
    }
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      float sn, cs;
      sincosf(p[s], &sn, &cs);
      re[s] = m[s] * cs; im[s] = m[s] * sn;
    }
  }
  float4* o = reinterpret_cast<float4*>(sb) + spec_slot(g, tg, lane);
  o[0] = make_float4(re[0], re[1], re[2], re[3]);
  o[1] = make_float4(im[0], im[1], im[2], im[3]);
  if (tg == 0 && lane < 32) {
    float v = 0.f;
    if (f < Fb) {
      const size_t a = ((size_t)b * NBIN + 512) * F_max + f;
      v = mag[a] * cosf(phase[a]);
    }
    sb[spec_nyq_slot(Fp, f)] = v;
  }
}

__global__ __launch_bounds__(256, 2) void gt_gl_project_kernel(const float* __restrict__ wav, int ld_wav,
                                                               const float* __restrict__ mag, const int32_t* __restrict__ n_frames,
                                                               int F_max, int Fp, const float* __restrict__ packed,
                                                               float* __restrict__ spec)
{
  __shared__ float lds[LDS_FLOATS];
  const int b = blockIdx.y, f0 = blockIdx.x * TF;
  const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
  int Fb = n_frames[b];
  Fb = Fb < F_max ? Fb : F_max;
  Fb = Fb < 1 + ld_wav / HOP ? Fb : 1 + ld_wav / HOP;
  Fb = Fb < 2 ? 0 : Fb;
  const int L = HOP * (Fb - 1);                          // samples of this utterance
  float* sb = spec + (size_t)b * spec_row_floats(Fp);
  float4* sb4 = reinterpret_cast<float4*>(sb);
  const int g0 = f0 >> 5;                                // the tile's two frame groups: g0, g0 + 1

  if (f0 >= Fb) {                                        // a tile past the utterance's end: zeros, no sample is read
    const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
    float4* img = sb4 + spec_slot(g0, 0, 0);
    for (int idx = tid; idx < 2 * SPEC_GROUP_F4; idx += 256) img[idx] = z;
    if (tid < TF) sb[spec_nyq_slot(Fp, f0 + tid)] = 0.f;
    return;
  }

  stage_tile(lds, wav + (size_t)b * ld_wav, L, f0, tid);
  __syncthreads();
  const float nyq_part = nyquist_partial(lds, packed, lane, w);

  // ---- the DFT: wave w, bin tiles 4 w .. 4 w + 3, 64 frames each; then Y = M X / |X| where it stands
  const int j = lane & 31, h = lane >> 5;
  const float* mb = mag + (size_t)b * NBIN * F_max;
  for (int pass = 0; pass < 4; ++pass) {
    const int bt = w * 4 + pass;
    f32x16_t ac[2], as[2];
    dft_tile(lds, packed, bt, lane, ac, as);
    // register e of lane half h is bin k = 32 bt + acc_row(e, h): bin group 4 bt + (e >> 2), lane 32 (e & 1) + j, word
    // 2 h + ((e & 3) >> 1) — registers e and e + 2 (e & 3 < 2) are neighbours: one 8-byte store each for re and im
#pragma unroll
    for (int ft = 0; ft < 2; ++ft) {
      const int f = f0 + ft * 32 + j;
      const bool live = f < Fb;
      float yr[16], yi[16];
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const float re = ac[ft][e], im = as[ft][e];
        const float m = live ? mb[(size_t)(bt * 32 + acc_row(e, h)) * F_max + f] : 0.f;
        const float m2 = fmaf(im, im, re * re);
        const float sc = m / sqrtf(m2);
        yr[e] = m2 == 0.f ? m : re * sc;
        yi[e] = m2 == 0.f ? 0.f : im * sc;
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

  // ---- bin 512: the four quarters in wave order; it is real, so Y = +-M
  float* nbuf = lds;                                     // [4][TF]
  nbuf[w * TF + lane] = nyq_part;
  __syncthreads();
  if (tid < TF) {
    const int f = f0 + tid;
    const float x = ((nbuf[tid] + nbuf[TF + tid]) + nbuf[2 * TF + tid]) + nbuf[3 * TF + tid];
    float y = 0.f;
    if (f < Fb) {
      const float m = mb[(size_t)512 * F_max + f];
      y = x < 0.f ? -m : m;
    }
    sb[spec_nyq_slot(Fp, f)] = y;
  }
}

__global__ __launch_bounds__(256, 2) void gt_istft_kernel(const float* __restrict__ spec, const int32_t* __restrict__ n_frames,
                                                          int F_max, int Fp, const float* __restrict__ packed,
                                                          float* __restrict__ wav, int ld_wav)
{
  __shared__ float xbuf[XBUF_FLOATS];                    // [wave][plain | mirror][32 rows][XS]
  const int b = blockIdx.y, h0 = blockIdx.x * TH, fbase = h0 - 1;
  const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
  int Fb = n_frames[b];
  Fb = Fb < 2 ? 0 : (Fb < F_max ? Fb : F_max);
  float* o = wav + (size_t)b * ld_wav;
  const int hops = (F_max - 1 - h0) < TH ? (F_max - 1 - h0) : TH;          // hops of this tile inside the output row (>= 1)

  if (h0 >= Fb - 1) {                                    // a tile behind the utterance's last hop: zeros, nothing is read
    for (int idx = tid; idx < hops * HOP; idx += 256) o[(size_t)h0 * HOP + idx] = 0.f;
    return;
  }

  const int j = lane & 31, h = lane >> 5;
  const float* sb = spec + (size_t)b * spec_row_floats(Fp);
  bool ok[2];
  const float4* yp[2];
  float re512[2];
#pragma unroll
  for (int ft = 0; ft < 2; ++ft) {
    const int f = fbase + ft * 32 + j;
    ok[ft] = f >= 0 && f < Fb;
    const int fc = ok[ft] ? f : 0;
    // = spec_slot(fc >> 5, 0, h * 32 + (fc & 31)), bin group 0 (the loop strides 128), WRITTEN OUT: through the function this kernel is
    // allocated differently and measured 1.2 % slower at B = 32 (profiles/stft_tile_bench.json); so it stays the parent's kernel
    static_assert(spec_slot(3, 0, 37) == ((size_t)3 * 4096 + 37) * 2, "the written-out index is stft_tile.h's");
    yp[ft] = reinterpret_cast<const float4*>(sb) + ((size_t)(fc >> 5) * 4096 + h * 32 + (fc & 31)) * 2;
    re512[ft] = ok[ft] ? sb[spec_nyq_slot(Fp, fc)] : 0.f;
  }
  const auto keep = [](bool k, const float4 v) { return make_float4(k ? v.x : 0.f, k ? v.y : 0.f, k ? v.z : 0.f, k ? v.w : 0.f); };

  for (int pass = 0; pass < 4; ++pass) {
    const int t = pass * 4 + w;
    f32x16_t aa[2], ab[2];
#pragma unroll
    for (int ft = 0; ft < 2; ++ft)
#pragma unroll
      for (int e = 0; e < 16; ++e) { aa[ft][e] = 0.f; ab[ft][e] = 0.f; }
    const float4* ip = reinterpret_cast<const float4*>(packed) + ((size_t)t * 64 * 64 + lane) * 2;
    // the NEXT bin group's basis and spectrum fragments (six 16-byte loads) are requested before this group's 16 MFMAs; the frames
    // outside the utterance are zeroed when the registers rotate, behind the MFMAs, so that the select does not wait in front of them
    float4 c4 = ip[0], s4 = ip[1], r4[2], i4[2];
#pragma unroll
    for (int ft = 0; ft < 2; ++ft) {
      r4[ft] = keep(ok[ft], yp[ft][0]); i4[ft] = keep(ok[ft], yp[ft][1]);
    }
    for (int tg = 0; tg < 64; ++tg) {
      const int tn = tg < 63 ? tg + 1 : tg;
      const float4 nc = ip[(size_t)tn * 128], ns = ip[(size_t)tn * 128 + 1];
      float4 nr[2], ni[2];
#pragma unroll
      for (int ft = 0; ft < 2; ++ft) { nr[ft] = yp[ft][(size_t)tn * 128]; ni[ft] = yp[ft][(size_t)tn * 128 + 1]; }
      const float cc[4] = {c4.x, c4.y, c4.z, c4.w}, ss[4] = {s4.x, s4.y, s4.z, s4.w};
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int ft = 0; ft < 2; ++ft) {
        const float yr[4] = {r4[ft].x, r4[ft].y, r4[ft].z, r4[ft].w}, yi[4] = {i4[ft].x, i4[ft].y, i4[ft].z, i4[ft].w};
#pragma unroll
        for (int s = 0; s < 4; ++s) {
          aa[ft] = __builtin_amdgcn_mfma_f32_32x32x2f32(cc[s], yr[s], aa[ft], 0, 0, 0);
          ab[ft] = __builtin_amdgcn_mfma_f32_32x32x2f32(ss[s], yi[s], ab[ft], 0, 0, 0);
        }
      }
      __builtin_amdgcn_sched_barrier(0);
      c4 = nc; s4 = ns;
#pragma unroll
      for (int ft = 0; ft < 2; ++ft) { r4[ft] = keep(ok[ft], nr[ft]); i4[ft] = keep(ok[ft], ni[ft]); }
    }
    // bin 512 closes the cos chain; then x[n] = a + b and x[1024 - n] = a - b go to the pass buffer
    const float* nq = packed + INV_OFF_NYQ + t * 32;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int row = acc_row(e, h);
      const float q = nq[row];
#pragma unroll
      for (int ft = 0; ft < 2; ++ft) {
        const float a = fmaf(q, re512[ft], aa[ft][e]), bb = ab[ft][e];
        xbuf[((w * 2 + 0) * 32 + row) * XS + ft * 32 + j] = a + bb;
        xbuf[((w * 2 + 1) * 32 + row) * XS + ft * 32 + j] = a - bb;
      }
    }
    __syncthreads();

    // ---- overlap-add of the pass's offsets r and 256 - r (and 0 in the last pass): lane = offset, wave = hop mod 4
    const int nr_off = pass == 3 ? 65 : 64;
    for (int ri = lane; ri < nr_off; ri += 64) {
      if (pass == 3 && ri == 63) continue;               // 256 - 128 = 128 again
      const int r = ri < 32 ? 1 + 32 * pass + ri : (ri < 64 ? 256 - (1 + 32 * pass + (ri - 32)) : 0);
      int row[4];
      float w2[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int n = r + 256 * q;
        row[q] = n ? src_row(n) * XS : -1;               // n = 0: w[0] = 0, nothing to add
        w2[q] = packed[INV_OFF_W2 + n];
      }
      for (int hl = w; hl < hops; hl += 4) {
        const int hop = h0 + hl;
        float acc = 0.f, env = 0.f;
#pragma unroll
        for (int q = 3; q >= 0; --q) {                   // frames hop - 1, hop, hop + 1, hop + 2: ascending
          const int f = hop + 2 - q;
          if (f >= 0 && f < Fb && row[q] >= 0) {
            acc += xbuf[row[q] + hl + 3 - q];
            env += w2[q];
          }
        }
        float v = 0.f;
        if (hop < Fb - 1) v = (env > FLT_MIN ? acc / env : acc) * (float)(NFFT / HOP);
        o[(size_t)hop * HOP + r] = v;
      }
    }
    __syncthreads();
  }
}


}  // namespace

extern "C" size_t gt_gl_pack_bytes(void) { return (size_t)INV_PACK_FLOATS * sizeof(float); }
extern "C" int gt_gl_tile_frames(void) { return TF; }
extern "C" int gt_gl_tile_hops(void) { return TH; }
extern "C" size_t gt_gl_spec_bytes(int B, int F_max)
{
  if (gl_shape_bad(B, F_max)) return 0;
  return (size_t)B * spec_row_floats(frames_padded(F_max)) * sizeof(float);
}

extern "C" int gt_gl_pack(const float* inverse_basis, int n_fft, void* packed, void* stream)
{
  if (!inverse_basis || !packed) return GT_E_INVAL;
  if (n_fft != NFFT) return GT_E_UNSUPPORTED;
  if (!al16(inverse_basis) || !al16(packed)) return GT_E_ALIGN;
  hipLaunchKernelGGL(gt_gl_pack_kernel, dim3((INV_PACK_FLOATS + 255) / 256), dim3(256), 0, GT_ST(stream), inverse_basis,
                     static_cast<float*>(packed));
  return gt_launch_status(__func__);
}

extern "C" int gt_gl_polar(const float* mag, const float* phase, const int32_t* n_frames, int B, int F_max, int n_fft, int hop,
                           int win, float* spec, void* stream)
{
  if (!mag || !phase || !n_frames || !spec || gl_shape_bad(B, F_max)) return GT_E_INVAL;
  if (n_fft != NFFT || hop != HOP || win != NFFT) return GT_E_UNSUPPORTED;
  if (!al16(mag) || !al16(phase) || !al16(spec) || ((uintptr_t)n_frames & 3)) return GT_E_ALIGN;
  const int Fp = frames_padded(F_max);
  hipLaunchKernelGGL(gt_gl_polar_kernel, dim3(Fp / 32 * 16, B), dim3(256), 0, GT_ST(stream), mag, phase, n_frames, F_max, Fp, spec);
  return gt_launch_status(__func__);
}

extern "C" int gt_gl_project(const float* wav, int ld_wav, const float* mag, const int32_t* n_frames, int B, int F_max,
                             const void* mel_packed, int n_fft, int hop, int win, float* spec, void* stream)
{
  if (!wav || !mag || !n_frames || !mel_packed || !spec || gl_shape_bad(B, F_max) || ld_wav <= 0) return GT_E_INVAL;
  if (n_fft != NFFT || hop != HOP || win != NFFT) return GT_E_UNSUPPORTED;
  if (!al16(wav) || !al16(mag) || !al16(mel_packed) || !al16(spec) || ((uintptr_t)n_frames & 3) || (ld_wav & 3)) return GT_E_ALIGN;
  const int Fp = frames_padded(F_max);
  hipLaunchKernelGGL(gt_gl_project_kernel, dim3(Fp / TF, B), dim3(256), 0, GT_ST(stream), wav, ld_wav, mag, n_frames, F_max, Fp,
                     static_cast<const float*>(mel_packed), spec);
  return gt_launch_status(__func__);
}

extern "C" int gt_istft(const float* spec, const int32_t* n_frames, int B, int F_max, const void* gl_packed, int n_fft, int hop,
                        int win, float* wav, int ld_wav, void* stream)
{
  if (!spec || !n_frames || !gl_packed || !wav || gl_shape_bad(B, F_max) || ld_wav <= 0) return GT_E_INVAL;
  if ((long long)ld_wav < (long long)HOP * (F_max - 1)) return GT_E_INVAL;
  if (n_fft != NFFT || hop != HOP || win != NFFT) return GT_E_UNSUPPORTED;
  if (!al16(spec) || !al16(gl_packed) || !al16(wav) || ((uintptr_t)n_frames & 3) || (ld_wav & 3)) return GT_E_ALIGN;
  if (F_max == 1) return GT_OK;                          // one frame has no hop: the output row has no column
  const int Fp = frames_padded(F_max);
  hipLaunchKernelGGL(gt_istft_kernel, dim3((F_max - 1 + TH - 1) / TH, B), dim3(256), 0, GT_ST(stream), spec, n_frames, F_max, Fp,
                     static_cast<const float*>(gl_packed), wav, ld_wav);
  return gt_launch_status(__func__);
}
