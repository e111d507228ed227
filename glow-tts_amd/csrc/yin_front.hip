// Device pitch front end: padded waveforms -> the YIN f0 contour (and, optionally, the harmonic rate and the argmin
// pitch) in ONE kernel, with the semantics of the reference's yin.compute_yin (yin.py:70-119) as get_f0 calls it, applied to every
// utterance on its own: frame i is samples 256 i .. 256 i + 1023 (not centred, not reflected), n_b = ceil((L - 1024) / 256) frames.
//
// fp32, direct differences (no energy - 2 autocorrelation: that cancels at the minima of d, where the pitch is decided).
//
//   sharing   consecutive frames overlap by 75 %.  Per hop h (256 samples) and lag t, with r = t mod 256,
//               F_t[h] = sum_{n = 256 h}^{256 h + 255} (x[n] - x[n + t])^2        T_t[h] = the same sum stopped after 256 - r terms
//             and the frame's difference function is
//               d_f[t] = ((F[f] + F[f+1]) + F[f+2]) + T[f+3]   (0 < t < 256)        d_f[t] = (F[f] + F[f+1]) + T[f+2]   (256 <= t < 512)
//             every sample used lies inside frame f.  256 terms per (hop, lag) instead of 1024 - t per (frame, lag).
//   tile      one workgroup (2 waves) = TF = 16 consecutive frames of one utterance.  Its (TF + 3) 256 + 512 samples are staged ONCE in
//             LDS (zeros from the utterance's end on, int16 scaled by 1/32768).  Thread i owns the four lags 4 i .. 4 i + 3 (wave 0:
//             lags < 256, wave 1: lags >= 256) and walks the tile's hops with F's running sums in registers.
//   blocking  per 16 terms a thread reads x[n .. n + 15] (one address per wave: a broadcast) and x[n + t .. n + t + 19] (consecutive
//             16-byte slots across the lanes: conflict-free) as nine ds_read_b128 for 64 terms, which run on the packed pipe: one
//             v_pk_add_f32 and one v_pk_fma_f32 per two lags and sample.
//   order     F: one fmaf chain in n order.  T: the chain's value at the start of the 16-term block the stop falls into (one select
//             per block) carried on over that block's terms up to the stop, behind the walk of the hop: the same chain, 64 masked
//             terms per hop instead of a select per term.  Fixed by (hop, lag) alone: a batch row is the utterance alone, bit for bit.
//   decide    d goes to a ring of four frames in LDS [4][512]: wave 1 closes its half of frame f in hop f + 2, wave 0 in hop f + 3,
//             and behind that hop's barrier (the walk's only one) wave f & 1 decides the frame while the other walks on.  Lane l
//             owns lags 8 l .. 8 l + 7: prefix sum = 8 in the lane, then a Hillis-Steele scan over the lanes; c = d t / sum (1 where
//             the sum is 0: digital silence); the threshold search and getPitch's descent are a ballot each per owned lag and
//             scalar bit searches, the argmin a butterfly.
#include <type_traits>
#include "common.h"
#include "internal.h"
#include "../../include/glowtts_hip.h"

namespace {

constexpr int WLEN = 1024, HOP = 256, NLAG = 512;
constexpr int TF = 16;                                   // frames per workgroup
constexpr int NS = (TF + 3) * HOP + NLAG;                // samples staged per tile
constexpr int NT = 128;                                  // threads: four lags each
constexpr int CH = 16;                                   // terms per block of the walk
constexpr int RING = 4;                                  // frames of d in LDS at a time

typedef float f32x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ void ld4(const float* p, float* v)
{
  const float4 t = *reinterpret_cast<const float4*>(p);
  v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
}

// the same, with the four words pinned as loaded: left alone the compiler re-reads the odd-aligned pairs of the packed operands from
// LDS as ds_read2_b32 (27 more LDS instructions per two blocks: the LDS would set the walk's pace) instead of forming them from registers with v_pk_mov_b32
__device__ __forceinline__ void ld4_pinned(const float* p, float* v)
{
  ld4(p, v);
  asm("" : "+v"(v[0]), "+v"(v[1]), "+v"(v[2]), "+v"(v[3]));
}

__global__ __launch_bounds__(NT) void gt_yin_f0_kernel(const void* __restrict__ wav, int is_i16, int ld_wav,
                                                        const int32_t* __restrict__ wav_len, int F_max, int tau_min, int tau_max,
                                                        float sr, float thresh, int lead, float* __restrict__ f0o,
                                                        float* __restrict__ harmo, float* __restrict__ amino)
{
  __shared__ __attribute__((aligned(16))) float xs[NS];
  __shared__ __attribute__((aligned(16))) float dring[RING * NLAG];
  const int b = blockIdx.y, fr0 = blockIdx.x * TF;
  const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
  int L = wav_len[b];
  L = L < ld_wav ? L : ld_wav;
  const int nb = L > WLEN ? (L - WLEN + HOP - 1) / HOP : 0;          // analysis frames of this utterance
  float* f0r = f0o + (size_t)b * F_max;
  float* hr = harmo ? harmo + (size_t)b * F_max : nullptr;
  float* ar = amino ? amino + (size_t)b * F_max : nullptr;

  // ---- every position of the tile that carries no frame is written as 0: the lead (tile 0) and everything from lead + nb on
  if (blockIdx.x == 0) {
    const int head = lead < F_max ? lead : F_max;
    for (int p = tid; p < head; p += NT) {
      f0r[p] = 0.f;
      if (hr) hr[p] = 0.f;
      if (ar) ar[p] = 0.f;
    }
  }
  if (tid < TF) {
    const int fr = fr0 + tid;
    if (fr >= nb && fr < F_max - lead) {                              // lead + fr < F_max without the overflow
      f0r[lead + fr] = 0.f;
      if (hr) hr[lead + fr] = 0.f;
      if (ar) ar[lead + fr] = 0.f;
    }
  }
  if (fr0 >= nb) return;                                              // a tile past the utterance's end: no sample is read
  const int nfr = nb - fr0 < TF ? nb - fr0 : TF;                      // frames of this tile, >= 1

  // ---- stage the tile's samples; nothing at or beyond index L is read
  {
    const int s0 = fr0 * HOP;                                         // < GT_MEL_MAX_FRAMES * 256 = 2^28
    const float* wf = static_cast<const float*>(wav) + (size_t)b * ld_wav;
    const int16_t* wi = static_cast<const int16_t*>(wav) + (size_t)b * ld_wav;
    const auto stage = [&](auto i16) {
      constexpr int TRIPS = NS / NT, UNR = 7;
      static_assert(TRIPS * NT == NS && TRIPS % UNR == 0, "whole trips");
      const int used = (nfr + 3) * HOP + NLAG;                        // what the walk of nfr frames reads
      for (int t0 = 0; t0 < TRIPS; t0 += UNR) {
        if (t0 * NT >= used) break;
        float v[UNR];
#pragma unroll
        for (int u = 0; u < UNR; ++u) {                               // unconditional loads (all in flight) of a clamped index
          const int s = s0 + (t0 + u) * NT + tid, sc = s < L ? s : L - 1;
          const float x = decltype(i16)::value ? (float)wi[sc] * (1.0f / 32768.0f) : wf[sc];
          v[u] = s < L ? x : 0.f;
        }
#pragma unroll
        for (int u = 0; u < UNR; ++u) xs[(t0 + u) * NT + tid] = v[u];
      }
    };
    if (is_i16) stage(std::true_type{}); else stage(std::false_type{});
  }
  __syncthreads();

  // ---- the walk over the hops: thread = lags t0 .. t0 + 3, r = t mod 256 = 4 lane + q
  {
    const int t0 = 256 * w + 4 * lane;
    const int ck = 15 - (lane >> 2);                                  // the block the stop of T falls into: term 255 - r
    const int jq0 = 15 - 4 * (lane & 3);                              // ... and its place in that block, for q = 0 (q: minus q)
    float s1[4] = {0.f, 0.f, 0.f, 0.f}, s2[4] = {0.f, 0.f, 0.f, 0.f}, s3[4] = {0.f, 0.f, 0.f, 0.f};
    const int nh = nfr + 3 - w;                                       // wave 1's last frame closes one hop earlier
    const float inf = __builtin_inff();
    for (int h = 0; h < nfr + 3; ++h) {
      if (h < nh) {                                                   // (wave 1 only waits in the tile's last hop)
        const float* xh = xs + h * HOP;
        float tst[4] = {0.f, 0.f, 0.f, 0.f};
        f32x2 a01 = {0.f, 0.f}, a23 = {0.f, 0.f};                       // the chains of lags (t0, t0 + 1) and (t0 + 2, t0 + 3)
#pragma unroll 2
        for (int c = 0; c < HOP / CH; ++c) {
          float xa[CH], xb[CH + 4];
#pragma unroll
          for (int i = 0; i < CH / 4; ++i) ld4(xh + c * CH + 4 * i, xa + 4 * i);
#pragma unroll
          for (int i = 0; i < CH / 4 + 1; ++i) ld4_pinned(xh + c * CH + t0 + 4 * i, xb + 4 * i);
          const bool mine = c == ck;
          tst[0] = mine ? a01.x : tst[0]; tst[1] = mine ? a01.y : tst[1];
          tst[2] = mine ? a23.x : tst[2]; tst[3] = mine ? a23.y : tst[3];
#pragma unroll
          for (int j = 0; j < CH; ++j) {                                // two packed subtractions and two packed fmas per sample
            const f32x2 x = {xa[j], xa[j]}, b01 = {xb[j], xb[j + 1]}, b23 = {xb[j + 2], xb[j + 3]};
            const f32x2 d01 = x - b01, d23 = x - b23;
            a01 = __builtin_elementwise_fma(d01, d01, a01);
            a23 = __builtin_elementwise_fma(d23, d23, a23);
          }
        }
        const float acc[4] = {a01.x, a01.y, a23.x, a23.y};
        {                                                               // T: the chain carried on from its block's start to the stop
          float xa[CH], xb[CH + 4];
#pragma unroll
          for (int i = 0; i < CH / 4; ++i) ld4(xh + ck * CH + 4 * i, xa + 4 * i);
#pragma unroll
          for (int i = 0; i < CH / 4 + 1; ++i) ld4(xh + ck * CH + t0 + 4 * i, xb + 4 * i);
#pragma unroll
          for (int j = 0; j < CH; ++j)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
              float d = xa[j] - xb[j + q];
              d = j <= jq0 - q ? d : 0.f;
              tst[q] = fmaf(d, d, tst[q]);
            }
        }
        const int fr = h - 3 + w;                                       // the frame this hop closes for this wave's lags
        if (fr >= 0) {
          float4 dv;
          if (w == 0) dv = make_float4(s3[0] + tst[0], s3[1] + tst[1], s3[2] + tst[2], s3[3] + tst[3]);
          else dv = make_float4(s2[0] + tst[0], s2[1] + tst[1], s2[2] + tst[2], s2[3] + tst[3]);
          *reinterpret_cast<float4*>(dring + (fr & (RING - 1)) * NLAG + t0) = dv;
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) { s3[q] = s2[q] + acc[q]; s2[q] = s1[q] + acc[q]; s1[q] = acc[q]; }
      }
      __syncthreads();                                                // frame h - 3 is whole: wave 1 wrote its half a hop ago
      const int fl = h - 3;
      if (fl < 0 || (fl & 1) != w) continue;                          // the waves take the frames in turn
      const float* drow = dring + (fl & (RING - 1)) * NLAG;           // rewritten by frame fl + 4: three barriers from here
      int ln = lane;                                                    // re-formed per frame: hoisted out of the loop, the lane
      asm volatile("" : "+v"(ln));                                       // masks of every comparison below cost some 60 SGPRs
      float dv[8], c[8];
      ld4(drow + 8 * ln, dv);
      ld4(drow + 8 * ln + 4, dv + 4);
      float ps[8];
      ps[0] = ln == 0 ? 0.f : dv[0];                                  // d[0] takes no part in the sum (it is 0)
#pragma unroll
      for (int k = 1; k < 8; ++k) ps[k] = ps[k - 1] + dv[k];
      float run = ps[7];                                                // inclusive scan over the lanes
#pragma unroll
      for (int off = 1; off < 64; off <<= 1) {
        const float o = __shfl_up(run, off);
        run = ln >= off ? run + o : run;
      }
      float excl = __shfl_up(run, 1);
      excl = ln == 0 ? 0.f : excl;
      float bestv = inf;
      int besti = 0;
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const int t = 8 * ln + k;
        const float sum = excl + ps[k];
        float v = sum > 0.f ? dv[k] * (float)t / sum : 1.0f;            // a lag whose running sum is 0 (digital silence): c = 1
        v = t == 0 ? 1.0f : v;
        c[k] = t < tau_max ? v : inf;
        if (c[k] < bestv) { bestv = c[k]; besti = t; }
      }
      const float cn7 = __shfl_down(c[0], 1);
      int first = NLAG;                                                 // the first lag in [tau_min, tau_max) below the threshold
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const int t = 8 * ln + k;
        const unsigned long long mb = __ballot(t >= tau_min && t < tau_max && c[k] < thresh);
        if (mb) {
          const int tb = 8 * (int)__builtin_ctzll(mb) + k;
          first = tb < first ? tb : first;
        }
      }
      int p = 0;
      if (first < NLAG) {                                               // forward to the first lag whose successor is not smaller
        p = NLAG;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          const int t = 8 * ln + k;
          const float cn = k < 7 ? c[k < 7 ? k + 1 : 7] : (ln == 63 ? inf : cn7);
          const unsigned long long m = __ballot(t >= first && !(t + 1 < tau_max && cn < c[k]));
          if (m) {
            const int ts = 8 * (int)__builtin_ctzll(m) + k;
            p = ts < p ? ts : p;
          }
        }
      }
#pragma unroll
      for (int off = 32; off >= 1; off >>= 1) {                         // argmin: the smallest c, the smaller lag among equals
        const float ov = __shfl_xor(bestv, off);
        const int oi = __shfl_xor(besti, off);
        const bool take = ov < bestv || (ov == bestv && oi < besti);
        bestv = take ? ov : bestv;
        besti = take ? oi : besti;
      }
      float cp = c[0];
#pragma unroll
      for (int k = 1; k < 8; ++k) cp = (p & 7) == k ? c[k] : cp;
      cp = __shfl(cp, p >> 3);
      const int fr = fr0 + fl;
      if (lane == 0 && fr < F_max - lead) {
        f0r[lead + fr] = p ? sr / (float)p : 0.f;
        if (hr) hr[lead + fr] = p ? cp : bestv;
        if (ar) ar[lead + fr] = besti > tau_min ? sr / (float)besti : 0.f;
      }
    }
  }
}


}  // namespace

extern "C" int gt_yin_tile_frames(void) { return TF; }

extern "C" int gt_yin_f0(const void* wav, int is_i16, int ld_wav, const int32_t* wav_len, int B, int F_max,
                         int w_len, int hop, int tau_min, int tau_max, float sr, float thresh, int lead,
                         float* f0, float* harm, float* argmin_f0, void* stream)
{
  if (!wav || !wav_len || !f0) return GT_E_INVAL;
  if (B <= 0 || B > GT_MEL_MAX_B || F_max <= 0 || F_max > GT_MEL_MAX_FRAMES || ld_wav <= 0 || lead < 0) return GT_E_INVAL;
  if (w_len <= 0 || hop <= 0 || tau_min < 1 || tau_max <= tau_min || !(sr > 0.f)) return GT_E_INVAL;
  if (w_len != WLEN || hop != HOP || tau_max > GT_YIN_MAX_TAU) return GT_E_UNSUPPORTED;
  if (!al16(wav) || !al16(f0) || !al16(harm) || !al16(argmin_f0) || ((uintptr_t)wav_len & 3) || (ld_wav & 3)) return GT_E_ALIGN;
  const dim3 grid((F_max + TF - 1) / TF, B);
  hipLaunchKernelGGL(gt_yin_f0_kernel, grid, dim3(NT), 0, GT_ST(stream), wav, is_i16, ld_wav, wav_len, F_max, tau_min, tau_max, sr,
                     thresh, lead, f0, harm, argmin_f0);
  return gt_launch_status(__func__);
}
