// Device sample-rate conversion: padded waveforms at one rate -> padded waveforms at another in ONE kernel, with the
// definition of scipy.signal.resample_poly(x, up, down) (window ('kaiser', 5.0), zero padding) applied to every utterance on its own.
//
//   definition  half = 10 max(up, down); the prototype h has 2 half + 1 taps; bank[p][j] = h[p + j up] (0 past the end of h), T = taps
//               per phase.  Output n of an utterance of L samples: q = n down + half, p = q mod up, k0 = q div up,
//                 y[n] = sum_{j = 0}^{T - 1} bank[p][j] x[k0 - j]        x[k] = 0 outside [0, L)        n < ceil(L up / down)
//   tile        one workgroup (4 waves) = up to `tpw` consecutive tiles of TO = 512 outputs of one utterance.  The bank is staged in LDS
//               ONCE per workgroup, rows at an ODD pitch (T | 1) and in LANE order: consecutive outputs step the phase by d = down mod up,
//               so phase p is kept in row s = p d^-1 mod up and output j of a tile reads row (s0 + j) mod up — consecutive lanes read
//               consecutive rows, which an odd pitch spreads over distinct banks (rows in phase order would meet at random: measured,
//               0.087 ms against 0.078 ms for the bench batch).  Per tile the input span k0(first) - (T - 1) .. k0(last) is staged (zeros
//               outside the utterance, int16 scaled by 1/32768) and thread i computes outputs i and i + 256 of the tile, the two
//               chains interleaved.
//   order       ONE fmaf chain over j ascending per output, from 0: fixed by (n, up, down) alone.  tpw only sizes the grid (the host
//               picks it from the batch's output count), the tile only says which thread computes an output: a batch row is the
//               utterance alone and an int16 input its fp32 image, bit for bit.
//   arithmetic  q = n down + half is formed in 64 bits once per tile (n0); inside a tile p0 + j down < 2^31 by the LDS bound below.
//   LDS         dynamic, 4 (round4(up (T | 1)) + round4(span)) bytes with span = (up - 1 + 511 down) div up + T, at most 64 KB:
//               a (up, down) that needs more is GT_E_UNSUPPORTED.  48 000 -> 22 050 Hz: 31.1 KB, five workgroups on a CU.
#include "common.h"
#include "internal.h"
#include "../../include/glowtts_hip.h"

namespace {

constexpr int NT = 256;                                  // threads
constexpr int TO = 512;                                  // outputs per tile: two per thread
constexpr int LDS_FLOATS = 16384;                        // bank + span, 64 KB
constexpr int MAX_TPW = 8;                               // tiles per workgroup, at most
constexpr int TARGET_WG = 2048;                          // the grid the host aims at before it lets a workgroup take more tiles

struct Plan { int taps, pitch, bank_floats, lds_bytes, dinv; };

// host: what a reduced (up, down) needs; false where it does not fit (or is not reduced)
bool plan(int up, int down, Plan* pl)
{
  if (up <= 0 || down <= 0) return false;
  long long a = up, b = down;
  while (b) { const long long t = a % b; a = b; b = t; }
  if (a != 1) return false;
  const long long mx = up > down ? up : down, ntap = 20 * mx + 1, T = (ntap + up - 1) / up, pitch = T | 1;
  if (pitch * up > LDS_FLOATS) return false;
  const long long bank = (pitch * up + 3) / 4 * 4, span = ((long long)up - 1 + (long long)(TO - 1) * down) / up + T;
  const long long total = bank + (span + 3) / 4 * 4;
  if (total > LDS_FLOATS) return false;
  pl->taps = (int)T; pl->pitch = (int)pitch; pl->bank_floats = (int)bank; pl->lds_bytes = (int)(4 * total);
  pl->dinv = 0;                                                       // (down mod up)^-1 mod up; up <= LDS_FLOATS here
  for (int v = 1; v < up; ++v)
    if ((long long)v * (down % up) % up == 1) { pl->dinv = v; break; }
  return true;
}

__global__ __launch_bounds__(NT) void gt_resample_kernel(const void* __restrict__ wav, int is_i16, int ld_wav,
                                                          const int32_t* __restrict__ wav_len, const float* __restrict__ bank, int up,
                                                          int down, int taps, int pitch, int bank_floats, int dinv, int tpw,
                                                          float* __restrict__ out, int ld_out, int32_t* __restrict__ out_len)
{
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* bk = lds;                                                    // [up][pitch], phase p in row p dinv mod up
  float* xs = lds + bank_floats;                                      // the tile's input span
  const int b = blockIdx.y, tid = threadIdx.x;
  int L = wav_len[b];
  L = L < ld_wav ? L : ld_wav;
  L = L < GT_RESAMPLE_MAX_LEN ? L : GT_RESAMPLE_MAX_LEN;
  L = L > 0 ? L : 0;
  const long long n_full = ((long long)L * up + down - 1) / down;     // ceil(L up / down)
  const int n_out = n_full < ld_out ? (int)n_full : ld_out;
  if (out_len && blockIdx.x == 0 && tid == 0) out_len[b] = n_out;
  float* orow = out + (size_t)b * ld_out;
  const long long n_base = (long long)blockIdx.x * tpw * TO;
  const int half = 10 * (up > down ? up : down);

  if (n_base < n_out) {                                               // the bank, once; a workgroup behind the utterance only fills zeros
    int r = tid / taps, c = tid - r * taps;
    const int dr = NT / taps, dc = NT - dr * taps;
    for (int i = tid; i < up * taps; i += NT) {
      bk[(r * dinv) % up * pitch + c] = bank[i];                    // r dinv < up^2 <= 2^28
      r += dr; c += dc;
      if (c >= taps) { c -= taps; ++r; }
    }
  }

  for (int t = 0; t < tpw; ++t) {
    const long long n0l = n_base + (long long)t * TO;
    if (n0l >= ld_out) break;
    const int n0 = (int)n0l;
    const int na = n0 + tid, nb = na + NT;                            // this thread's outputs (n0 + 511 <= ld_out + 510: no overflow, ld_out <= 2^30)
    if (n0 >= n_out) {                                                // behind the utterance: zeros, no sample is read
      if (na < ld_out) orow[na] = 0.f;
      if (nb < ld_out) orow[nb] = 0.f;
      continue;
    }
    const long long q0 = (long long)n0 * down + half;
    const int p0 = (int)(q0 % up), k00 = (int)(q0 / up);             // k00 <= L + half / up
    const int nt = n_out - n0 < TO ? n_out - n0 : TO;                 // outputs of this tile, >= 1
    const int span = (p0 + (nt - 1) * down) / up + taps;              // <= the host's bound
    const int s0 = k00 - (taps - 1);
    __syncthreads();                                                  // the tile before is done with xs
    if (is_i16) {
      const int16_t* w = static_cast<const int16_t*>(wav) + (size_t)b * ld_wav;
      for (int i = tid; i < span; i += NT) {
        const int s = s0 + i, sc = s < 0 ? 0 : (s < L ? s : L - 1);   // L >= 1 here; nothing at or beyond index L is read
        const float x = (float)w[sc] * (1.0f / 32768.0f);
        xs[i] = s >= 0 && s < L ? x : 0.f;
      }
    } else {
      const float* w = static_cast<const float*>(wav) + (size_t)b * ld_wav;
      for (int i = tid; i < span; i += NT) {
        const int s = s0 + i, sc = s < 0 ? 0 : (s < L ? s : L - 1);
        const float x = w[sc];
        xs[i] = s >= 0 && s < L ? x : 0.f;
      }
    }
    __syncthreads();                                                  // (and the bank, before the first tile)
    const bool va = tid < nt, vb = tid + NT < nt;
    const int qa = p0 + (va ? tid : 0) * down, qb = p0 + (vb ? tid + NT : 0) * down;
    const int ka = qa / up, kb = qb / up;
    const int r0 = (p0 * dinv) % up;                                  // the row of the tile's first output; output j: row (r0 + j) mod up
    const float* ba = bk + (r0 + (va ? tid : 0)) % up * pitch;
    const float* bb = bk + (r0 + (vb ? tid + NT : 0)) % up * pitch;
    const float* xa = xs + ka + (taps - 1);
    const float* xb = xs + kb + (taps - 1);
    float ya = 0.f, yb = 0.f;
#pragma unroll 4
    for (int j = 0; j < taps; ++j) {
      ya = fmaf(ba[j], xa[-j], ya);
      yb = fmaf(bb[j], xb[-j], yb);
    }
    if (na < ld_out) orow[na] = va ? ya : 0.f;
    if (nb < ld_out) orow[nb] = vb ? yb : 0.f;
  }
}


}  // namespace

extern "C" int gt_resample_tile_out(void) { return TO; }

extern "C" int gt_resample_taps(int up, int down)
{
  Plan pl;
  return plan(up, down, &pl) ? pl.taps : 0;
}

extern "C" size_t gt_resample_lds_bytes(int up, int down)
{
  Plan pl;
  return plan(up, down, &pl) ? (size_t)pl.lds_bytes : 0;
}

extern "C" int gt_resample(const void* wav, int is_i16, int ld_wav, const int32_t* wav_len, int B, const float* bank, int up, int down,
                           int taps, float* out, int ld_out, int32_t* out_len, void* stream)
{
  if (!wav || !wav_len || !bank || !out) return GT_E_INVAL;
  if (B <= 0 || B > GT_MEL_MAX_B || ld_wav <= 0 || ld_out <= 0 || up <= 0 || down <= 0 || taps <= 0) return GT_E_INVAL;
  const long long mx = up > down ? up : down;
  if (taps != (20 * mx + 1 + up - 1) / up) return GT_E_INVAL;
  Plan pl;
  if (!plan(up, down, &pl) || ld_out > GT_RESAMPLE_MAX_OUT) return GT_E_UNSUPPORTED;
  if (!al16(wav) || !al16(bank) || !al16(out) || ((uintptr_t)wav_len & 3) || ((uintptr_t)out_len & 3) || (ld_wav & 3) || (ld_out & 3))
    return GT_E_ALIGN;
  const long long tiles = (ld_out + TO - 1) / TO;
  long long tpw = tiles * B / TARGET_WG;                              // sizes the grid only: no output depends on it
  tpw = tpw < 1 ? 1 : (tpw > MAX_TPW ? MAX_TPW : tpw);
  const dim3 grid((unsigned)((tiles + tpw - 1) / tpw), B);
  hipLaunchKernelGGL(gt_resample_kernel, grid, dim3(NT), pl.lds_bytes, GT_ST(stream), wav, is_i16, ld_wav, wav_len, bank, up, down,
                     taps, pl.pitch, pl.bank_floats, pl.dinv, (int)tpw, out, ld_out, out_len);
  return gt_launch_status(__func__);
}
