// Vocos vocoder on the device: the three kernels the frame-rate ConvNeXt backbone and its iSTFT head need next to
// gt_voc_conv (embedding, head Linear) and gt_istft.  Activations are dense channels-last, every utterance of a ragged batch on its own.
//
//   gt_vocos_norm   depthwise k = 7 convolution (optional) + LayerNorm over the channels of a row: one wave per row, a lane owns the
//                   C / 64 channels lane + 64 j.  h = bd[c] + sum_j wd[c][j] x[t + j - 3, c] as ONE fmaf chain, j ascending, a tap outside
//                   [0, len) skipped (not read); mean, then the variance of the centred values (dds_rows.h::ln_stats' form), rsqrtf;
//                   fp32 or bf16 out.  Four waves x 8 rows = 32 positions per workgroup; no LDS.
//   gt_vocos_mlp    the block's pointwise MLP with its residual, the hidden activation never leaving the chip:
//                     u = bf16(gelu(b1 + A W1^T)),  Y = R + b2 + u W2^T
//                   on v_mfma_f32_32x32x16_bf16.  A workgroup of four waves owns TM = 64 positions: their A tile [64][C] bf16 sits in LDS for
//                   the whole kernel; the hidden dimension is walked in chunks of HC = 128 units.  Per chunk wave w forms the 32 hidden
//                   units 32 (4 i + w) .. + 31 of all 64 positions (first product TRANSPOSED — hidden unit on the accumulator's rows, position on
//                   its lane — so that a register quad holds four consecutive hidden units of one position: one 8-byte LDS store), applies
//                   the exact GELU in fp32, rounds to bf16 into one of TWO u buffers [64][128] in LDS; then every wave accumulates the chunk's
//                   contribution to ITS C / 4 output columns of all 64 positions (C / 128 column tiles x 2 row tiles of 16 registers: 128
//                   accumulator registers at C = 512).  The loop is software-pipelined over the two buffers: chunk i's first product and
//                   GELU are issued around chunk i - 1's second product, one barrier per chunk (the library erff branches, so the compiler
//                   does not interleave the GELU with the MFMAs: DESIGN.md 4.25 has what that costs).
//                   Weight fragments come straight from global memory (voc_pack's order, taps = 1): 3 MB per block at 512 / 1536, L2-resident.
//   LDS             A: 64 rows of C + 8 bf16 (pitch 1040 bytes = 65 16-byte slots at C = 512, odd: the 16 rows of a ds_read_b128 lane group fall
//                   into distinct slots), u: 2 x 64 rows of 136 bf16 (17 slots).  66 560 + 34 816 = 101 376 bytes at C = 512: one workgroup a CU.
//   gt_vocos_polar  (log-magnitude, phase) rows [.., 1026] -> gt_istft's spectrum layout (stft_tile.h): m = min(expf(x), 100),
//                   (re, im) = m (cosf, sinf)(p) with the accurate library functions.  A workgroup takes 32 frames x 128 bins through LDS
//                   ([32][129] re and im: rows read coalesced, slots written as two 16-byte stores per lane).
//   order           every sum's order depends on the channel / hidden index and the shape alone: a batch row is bit-identical to the utterance
//                   computed alone, in a buffer of any capacity.
//   bounds          every global read is at a position < len_b, every write at a position < L_cap (polar: inside the spectrum image, whose
//                   size is a function of (B, F_max)); LDS indices are < the buffers by construction; all offsets are size_t.
#include "common.h"
#include "internal.h"
#include "dds_rows.h"
#include "mfma_frag.h"
#include "stft_tile.h"
#include "../../include/glowtts_hip.h"

namespace {

constexpr int NT = 256;                                  // threads: four waves

__device__ __forceinline__ int utt_len(const int32_t* n_frames, int b, int L_cap)
{
  int nf = n_frames[b];
  nf = nf > 0 ? nf : 0;
  return nf < L_cap ? nf : L_cap;
}

// ---------------------------------------------------------------------------------------------------------------- norm
constexpr int NRW = 8;                                   // rows a wave walks
constexpr int NTM = 4 * NRW;                             // positions per workgroup
constexpr int DW = 7;                                    // depthwise taps

template <int NC>
__global__ __launch_bounds__(NT) void gt_vocos_norm_kernel(const gt_vocos_norm_args a)
{
  constexpr int C = NC * 64;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int b = blockIdx.y, t0 = blockIdx.x * NTM + wave * NRW;
  if (t0 >= a.L_cap) return;
  const int len = utt_len(a.n_frames, b, a.L_cap);
  const int t_end = t0 + NRW < a.L_cap ? t0 + NRW : a.L_cap;
  const size_t ybase = (size_t)b * (size_t)a.y_stride_b;
  const float* x = a.X + (size_t)b * (size_t)a.x_stride_b;    // Y may be X (wd == NULL): no __restrict__
  const bool dw = a.wd != nullptr;

  float g[NC], be[NC], bd[NC], wd[DW][NC];
#pragma unroll
  for (int j = 0; j < NC; ++j) {
    const int c = lane + 64 * j;
    g[j] = a.g[c]; be[j] = a.be[c];
    bd[j] = dw ? a.bd[c] : 0.f;
#pragma unroll
    for (int k = 0; k < DW; ++k) wd[k][j] = dw ? a.wd[c * DW + k] : 0.f;
  }
  for (int t = t0; t < t_end; ++t) {
    const size_t yo = ybase + (size_t)t * C + lane;
    if (t >= len) {                                      // behind the utterance: zeros, nothing is read
#pragma unroll
      for (int j = 0; j < NC; ++j) {
        if (a.y_bf16) static_cast<bf16_t*>(a.Y)[yo + 64 * j] = 0; else static_cast<float*>(a.Y)[yo + 64 * j] = 0.f;
      }
      continue;
    }
    float v[NC];
    if (dw) {
#pragma unroll
      for (int j = 0; j < NC; ++j) v[j] = bd[j];
#pragma unroll
      for (int k = 0; k < DW; ++k) {
        const int p = t + k - DW / 2;
        if (p < 0 || p >= len) continue;                 // wave-uniform
        const float* xr = x + (size_t)p * C + lane;
#pragma unroll
        for (int j = 0; j < NC; ++j) v[j] = fmaf(wd[k][j], xr[64 * j], v[j]);
      }
    } else {
      const float* xr = x + (size_t)t * C + lane;
#pragma unroll
      for (int j = 0; j < NC; ++j) v[j] = xr[64 * j];
    }
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < NC; ++j) s += v[j];
    const float mean = wave_sum(s) * (1.0f / C);
    float q = 0.f;
#pragma unroll
    for (int j = 0; j < NC; ++j) { v[j] -= mean; q += v[j] * v[j]; }
    const float rstd = rsqrtf(wave_sum(q) * (1.0f / C) + a.eps);
#pragma unroll
    for (int j = 0; j < NC; ++j) {
      const float y = fmaf(v[j] * rstd, g[j], be[j]);
      if (a.y_bf16) static_cast<bf16_t*>(a.Y)[yo + 64 * j] = f2bf(y); else static_cast<float*>(a.Y)[yo + 64 * j] = y;
    }
  }
}

template <int NC>
int launch_norm(const gt_vocos_norm_args& a, hipStream_t st)
{
  hipLaunchKernelGGL(gt_vocos_norm_kernel<NC>, dim3((a.L_cap + NTM - 1) / NTM, a.B), dim3(NT), 0, st, a);
  return gt_launch_status("gt_vocos_norm");
}

// ---------------------------------------------------------------------------------------------------------------- mlp
constexpr int TM = 64;                                   // positions per workgroup
constexpr int HC = 128;                                  // hidden units per chunk: one 32-unit tile per wave
constexpr int MT = TM / 32;                              // 32-position tiles
constexpr int PU = HC + 8;                               // u row pitch, bf16 elements
constexpr int KS2 = HC / 16;                             // k-steps of the second product per chunk
constexpr int MAX_H = 2048;

__host__ __device__ constexpr int mlp_lds_bytes(int C) { return TM * (C + 8) * 2 + 2 * TM * PU * 2; }

template <int C>
__global__ __launch_bounds__(NT) void gt_vocos_mlp_kernel(const gt_vocos_mlp_args a)
{
  constexpr int NTW = C / 128, KS1 = C / 16, PA = C + 8;
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
  bf16_t* as = reinterpret_cast<bf16_t*>(lds_raw);                                // [TM][PA]
  bf16_t* us = as + TM * PA;                                                      // [2][TM][PU]

  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r32 = lane & 31, h = lane >> 5;
  const int b = blockIdx.y, t0 = blockIdx.x * TM;
  const int len = utt_len(a.n_frames, b, a.L_cap);
  float* Y = a.Y + (size_t)b * (size_t)a.y_stride_b;                              // may be R: no __restrict__

  if (t0 >= len) {                                                                // behind the utterance: zeros, nothing is read
    for (int i = tid; i < TM * C; i += NT) {
      const int t = t0 + i / C;
      if (t < a.L_cap) Y[(size_t)t * C + i % C] = 0.f;
    }
    return;
  }

  {                                                                               // the A tile, zeros behind the utterance
    const bf16_t* A = static_cast<const bf16_t*>(a.A) + (size_t)b * (size_t)a.a_stride_b;
    constexpr int CPR = C / 8;
    for (int i = tid; i < TM * CPR; i += NT) {
      const int row = i / CPR, cg = (i - row * CPR) * 8, p = t0 + row;
      uint4 o = make_uint4(0, 0, 0, 0);
      if (p < len) o = *reinterpret_cast<const uint4*>(A + (size_t)p * C + cg);
      *reinterpret_cast<uint4*>(as + row * PA + cg) = o;
    }
  }
  __syncthreads();

  const bf16_t* W1 = static_cast<const bf16_t*>(a.W1);
  const bf16_t* W2 = static_cast<const bf16_t*>(a.W2);
  const int NCH = a.H / HC, KST2 = a.H / 16;
  bf16_t* Ug = a.U ? static_cast<bf16_t*>(a.U) + (size_t)b * (size_t)a.u_stride_b : nullptr;

  f32x16_t acc2[MT][NTW];
  acc_zero(acc2);

  // first product of chunk i, transposed: rows = this wave's 32 hidden units, lane = position
  const auto first = [&](int i, f32x16_t (&acc1)[MT]) {
    acc_zero(acc1);
    const int ht = i * 4 + wave;
    const bf16_t* ar = as + r32 * PA + 8 * h;
#pragma unroll 8
    for (int ks = 0; ks < KS1; ++ks) {
      const bf16x8_t wf = asfrag(ldfrag(W1, ht * KS1 + ks, lane));
#pragma unroll
      for (int pt = 0; pt < MT; ++pt) {
        const bf16x8_t af = asfrag(*reinterpret_cast<const uint4*>(ar + pt * 32 * PA + ks * 16));
        acc1[pt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wf, af, acc1[pt], 0, 0, 0);
      }
    }
  };
  // bias, GELU, bf16: register quad q of lane half h is hidden units 8 q + 4 h .. + 3 of the wave's tile, position pt * 32 + r32
  const auto activate = [&](int i, const f32x16_t (&acc1)[MT]) {
    bf16_t* ub = us + (i & 1) * TM * PU;
    const int hid = (i * 4 + wave) * 32 + 4 * h;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const float b0 = a.b1[hid + 8 * q], b1 = a.b1[hid + 8 * q + 1], b2 = a.b1[hid + 8 * q + 2], b3 = a.b1[hid + 8 * q + 3];
#pragma unroll
      for (int pt = 0; pt < MT; ++pt) {
        const uint2 pk = pack4(gtdds::gelu_f(acc1[pt][4 * q] + b0), gtdds::gelu_f(acc1[pt][4 * q + 1] + b1), gtdds::gelu_f(acc1[pt][4 * q + 2] + b2),
                               gtdds::gelu_f(acc1[pt][4 * q + 3] + b3));
        *reinterpret_cast<uint2*>(ub + (pt * 32 + r32) * PU + wave * 32 + 8 * q + 4 * h) = pk;
        const int t = t0 + pt * 32 + r32;
        if (Ug && t < len) *reinterpret_cast<uint2*>(Ug + (size_t)t * a.H + hid + 8 * q) = pk;
      }
    }
  };
  // second product of chunk i: this wave's NTW column tiles of all TM positions
  const auto second = [&](int i) {
    const bf16_t* ur = us + (i & 1) * TM * PU + r32 * PU + 8 * h;
#pragma unroll
    for (int ks = 0; ks < KS2; ++ks) {
      bf16x8_t uf[MT];
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) uf[mt] = asfrag(*reinterpret_cast<const uint4*>(ur + mt * 32 * PU + ks * 16));
#pragma unroll
      for (int nt = 0; nt < NTW; ++nt) {
        const bf16x8_t wf = asfrag(ldfrag(W2, (wave * NTW + nt) * KST2 + i * KS2 + ks, lane));
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) acc2[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(uf[mt], wf, acc2[mt][nt], 0, 0, 0);
      }
    }
  };

  {
    f32x16_t acc1[MT];
    first(0, acc1);
    activate(0, acc1);
  }
  __syncthreads();
  for (int i = 1; i < NCH; ++i) {
    f32x16_t acc1[MT];
    first(i, acc1);
    second(i - 1);                                                                // reads buffer (i - 1) & 1 ...
    activate(i, acc1);                                                            // ... while buffer i & 1 is written
    __syncthreads();
  }
  second(NCH - 1);

  // epilogue: column = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5): 32 lanes store 32 consecutive channels
  const float* R = a.R + (size_t)b * (size_t)a.r_stride_b;
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) {
#pragma unroll
    for (int nt = 0; nt < NTW; ++nt) {
      const int n = (wave * NTW + nt) * 32 + r32;
      const float bn = a.b2[n];
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int t = t0 + mt * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
        if (t >= a.L_cap) continue;
        const size_t off = (size_t)t * C + n;
        float v = 0.f;
        if (t < len) v = (acc2[mt][nt][r] + bn) + R[off];
        Y[off] = v;
      }
    }
  }
}

template <int C>
int launch_mlp(const gt_vocos_mlp_args& a, hipStream_t st)
{
  constexpr int lds = mlp_lds_bytes(C);
  if (lds > 64 * 1024) {
    const int rc = gt_allow_lds<gt_vocos_mlp_kernel<C>>(lds);
    if (rc) return rc;
  }
  hipLaunchKernelGGL(gt_vocos_mlp_kernel<C>, dim3((a.L_cap + TM - 1) / TM, a.B), dim3(NT), lds, st, a);
  return gt_launch_status("gt_vocos_mlp");
}

// ---------------------------------------------------------------------------------------------------------------- polar
using namespace gtstft;

constexpr int PB = 128;                                  // bins per workgroup (16 bin groups)
constexpr int PP = PB + 1;                               // LDS row pitch, floats
constexpr float MAG_CLIP = 100.0f;

__global__ __launch_bounds__(NT) void gt_vocos_polar_kernel(const gt_vocos_polar_args a, int Fp)
{
  __shared__ float re_s[32 * PP], im_s[32 * PP];
  const int tid = threadIdx.x;
  const int b = blockIdx.y, g = blockIdx.x >> 2, kb = blockIdx.x & 3;
  const int f0 = g * 32, k0 = kb * PB;
  int Fb = a.n_frames[b];
  Fb = Fb < 2 ? 0 : (Fb < a.F_max ? Fb : a.F_max);
  const float* __restrict__ O = a.O + (size_t)b * (size_t)a.o_stride_b;
  float* sb = a.spec + (size_t)b * spec_row_floats(Fp);

  for (int i = tid; i < 32 * PB; i += NT) {              // rows read coalesced: bin fastest
    const int k = i & (PB - 1), fl = i >> 7, f = f0 + fl;
    float re = 0.f, im = 0.f;
    if (f < Fb) {
      const float* row = O + (size_t)f * (2 * NBIN);
      const float m = fminf(expf(row[k0 + k]), MAG_CLIP);
      float sn, cs;
      sincosf(row[NBIN + k0 + k], &sn, &cs);
      re = m * cs; im = m * sn;
    }
    re_s[fl * PP + k] = re; im_s[fl * PP + k] = im;
  }
  __syncthreads();
  float4* sb4 = reinterpret_cast<float4*>(sb);
  for (int i = tid; i < 16 * 64; i += NT) {              // this workgroup's 16 bin groups x 64 lanes
    const int lane = i & 63, tl = i >> 6, fl = lane & 31;
    float re[4], im[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const int k = 8 * tl + 2 * s + (lane >> 5);        // spec_bin(tg, lane, s) - k0
      re[s] = re_s[fl * PP + k]; im[s] = im_s[fl * PP + k];
    }
    float4* o = sb4 + spec_slot(g, kb * 16 + tl, lane);
    o[0] = make_float4(re[0], re[1], re[2], re[3]);
    o[1] = make_float4(im[0], im[1], im[2], im[3]);
  }
  if (kb == 0 && tid < 32) {                             // Re of bin 512; its Im is not kept
    const int f = f0 + tid;
    float v = 0.f;
    if (f < Fb) {
      const float* row = O + (size_t)f * (2 * NBIN);
      v = fminf(expf(row[512]), MAG_CLIP) * cosf(row[NBIN + 512]);
    }
    sb[spec_nyq_slot(Fp, f)] = v;
  }
}

}  // namespace

extern "C" int gt_vocos_norm_args_size(void) { return (int)sizeof(gt_vocos_norm_args); }
extern "C" int gt_vocos_mlp_args_size(void) { return (int)sizeof(gt_vocos_mlp_args); }
extern "C" int gt_vocos_polar_args_size(void) { return (int)sizeof(gt_vocos_polar_args); }
extern "C" int gt_vocos_norm_tile_positions(void) { return NTM; }
extern "C" int gt_vocos_tile_positions(void) { return TM; }
extern "C" int gt_vocos_hidden_chunk(void) { return HC; }
extern "C" size_t gt_vocos_mlp_lds_bytes(int C) { return (C == 128 || C == 256 || C == 512) ? (size_t)mlp_lds_bytes(C) : 0; }

extern "C" int gt_vocos_norm(const gt_vocos_norm_args* args, void* stream)
{
  if (!args) return GT_E_INVAL;
  const gt_vocos_norm_args& a = *args;
  if (!a.X || !a.g || !a.be || !a.Y || !a.n_frames) return GT_E_INVAL;
  if ((a.wd == nullptr) != (a.bd == nullptr)) return GT_E_INVAL;
  if (a.B <= 0 || a.L_cap <= 0 || a.C <= 0 || !(a.eps >= 0.f)) return GT_E_INVAL;
  if (a.x_stride_b < (long long)a.L_cap * a.C || a.y_stride_b < (long long)a.L_cap * a.C) return GT_E_INVAL;
  if (a.Y == (const void*)a.X && (a.wd || a.y_bf16)) return GT_E_INVAL;
  if (a.C % 64 || a.C > 512 || a.B > 65535) return GT_E_UNSUPPORTED;
  if ((long long)a.B * a.L_cap * a.C >= (1ll << 31)) return GT_E_UNSUPPORTED;
  if (((uintptr_t)a.X & 3) || ((uintptr_t)a.wd & 3) || ((uintptr_t)a.bd & 3) || ((uintptr_t)a.g & 3) || ((uintptr_t)a.be & 3) ||
      ((uintptr_t)a.n_frames & 3) || ((uintptr_t)a.Y & (a.y_bf16 ? 1 : 3)))
    return GT_E_ALIGN;
  hipStream_t st = static_cast<hipStream_t>(stream);
  switch (a.C / 64) {
    case 1: return launch_norm<1>(a, st);
    case 2: return launch_norm<2>(a, st);
    case 3: return launch_norm<3>(a, st);
    case 4: return launch_norm<4>(a, st);
    case 5: return launch_norm<5>(a, st);
    case 6: return launch_norm<6>(a, st);
    case 7: return launch_norm<7>(a, st);
    default: return launch_norm<8>(a, st);
  }
}

extern "C" int gt_vocos_mlp(const gt_vocos_mlp_args* args, void* stream)
{
  if (!args) return GT_E_INVAL;
  const gt_vocos_mlp_args& a = *args;
  if (!a.A || !a.W1 || !a.b1 || !a.W2 || !a.b2 || !a.R || !a.Y || !a.n_frames) return GT_E_INVAL;
  if (a.B <= 0 || a.L_cap <= 0 || a.C <= 0 || a.H <= 0) return GT_E_INVAL;
  const long long rowC = (long long)a.L_cap * a.C;
  if (a.a_stride_b < rowC || a.r_stride_b < rowC || a.y_stride_b < rowC) return GT_E_INVAL;
  if (a.U && a.u_stride_b < (long long)a.L_cap * a.H) return GT_E_INVAL;
  if ((const void*)a.Y == a.A || (a.U && (a.U == (void*)a.Y || a.U == (void*)a.R || a.U == a.A))) return GT_E_INVAL;
  if ((a.C != 128 && a.C != 256 && a.C != 512) || a.H % HC || a.H > MAX_H || a.B > 65535) return GT_E_UNSUPPORTED;
  if ((long long)a.B * a.L_cap * (a.C > a.H ? a.C : a.H) >= (1ll << 31)) return GT_E_UNSUPPORTED;
  if (!al16(a.A) || !al16(a.W1) || !al16(a.W2) || (a.a_stride_b & 7)) return GT_E_ALIGN;
  if (((uintptr_t)a.b1 & 3) || ((uintptr_t)a.b2 & 3) || ((uintptr_t)a.R & 3) || ((uintptr_t)a.Y & 3) || ((uintptr_t)a.n_frames & 3))
    return GT_E_ALIGN;
  if (a.U && (((uintptr_t)a.U & 7) || (a.u_stride_b & 3))) return GT_E_ALIGN;
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (a.C == 128) return launch_mlp<128>(a, st);
  if (a.C == 256) return launch_mlp<256>(a, st);
  return launch_mlp<512>(a, st);
}

extern "C" int gt_vocos_polar(const gt_vocos_polar_args* args, void* stream)
{
  if (!args) return GT_E_INVAL;
  const gt_vocos_polar_args& a = *args;
  if (!a.O || !a.n_frames || !a.spec || gl_shape_bad(a.B, a.F_max)) return GT_E_INVAL;
  if (a.o_stride_b < (long long)a.F_max * (2 * NBIN)) return GT_E_INVAL;
  if (a.n_fft != NFFT) return GT_E_UNSUPPORTED;
  if (((uintptr_t)a.O & 3) || ((uintptr_t)a.n_frames & 3) || !al16(a.spec)) return GT_E_ALIGN;
  const int Fp = frames_padded(a.F_max);
  hipLaunchKernelGGL(gt_vocos_polar_kernel, dim3(Fp / 32 * 4, a.B), dim3(NT), 0, static_cast<hipStream_t>(stream), a, Fp);
  return gt_launch_status("gt_vocos_polar");
}
