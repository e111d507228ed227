// WaveGlow's reverse flow on the device: the two kernels gt_voc_conv (csrc/hifigan.hip) does not cover.
//
// gt_wg_gate      one WaveNet layer's in_layer (dilated, taps x C from the fp32 residual stream) + its slice of the conditioning layer
//                 (Cs = 640 from the bf16 spect) + the gate, as ONE implicit GEMM on v_mfma_f32_32x32x16_bf16 with gt_voc_conv's tiling:
//   tile        a workgroup of four waves owns TM = 128 positions x 128 gate channels of one utterance; a wave takes all 128 positions x
//               32 gate channels = TWO 32-column accumulator tiles, the tanh half and the sigmoid half of the same channels (the host
//               interleaves the image's 32-row groups), so acts[n] and acts[n + C] meet in one lane and the gate needs no LDS round trip.
//               No two waves load the same weight fragment.
//   K walk      per 64-channel chunk of X: TM + (taps - 1) dil positions staged in LDS once (fp32 -> bf16, zeros outside the utterance),
//               the taps walked over that tile (tap j of output row m is LDS row m + j dil); then per 64-channel chunk of S: TM rows, no
//               halo, copied as they are.
//   LDS         dynamic, (TM + (taps - 1) dil) rows of 144 bytes (64 bf16 + 16: 9 16-byte slots, odd — gt_voc_conv's conflict-free pitch);
//               taps 3, dil 128: 384 rows = 55 296 bytes, two workgroups a CU.
//   order       fp32 accumulation in the MFMA over (X chunk, tap, k-step) then (S chunk, k-step) ascending, fixed by (t mod TM, n, C,
//               taps) alone.
//   bounds      every global access is predicated by position (< len_b for reads, < L_cap for writes); channels are whole chunks (C and
//               Cs are multiples of 64); LDS rows are < TM + (taps - 1) dil by construction; all offsets are size_t.
//
// gt_wg_boundary  everything between two WaveNets, fp32 on the vector ALU: a wave owns 8 consecutive positions and handles them one
//               after the other — skip[C] read coalesced (lane, lane + 64, ...), the end convolution as per-lane fmaf chains and the
//               wave's xor butterfly, the coupling inverse and the noise in every lane alike, the inverse 1x1 one row per lane and
//               handed round by __shfl (8 slots in registers, all indices compile-time), the next start convolution written
//               coalesced with the skip row cleared behind it.  No LDS.
//   bounds      positions are predicated by < len_b (reads and writes; the last form writes zeros up to L_cap), channels by < C;
//               the images are [C][8], [8][8] and [C][8] by contract; all offsets are size_t.
#include "common.h"
#include "internal.h"
#include "mfma_frag.h"
#include "../../include/glowtts_hip.h"

namespace {

constexpr int NT = 256;                                  // threads: four waves
constexpr int TM = 128;                                  // positions per workgroup of the gate kernel
constexpr int KC = 64, KS = KC / 16, PITCH = KC + 8;     // staged chunk, its 16-deep k-steps, the LDS row pitch in bf16 elements
constexpr int MT = TM / 32;                              // 32-row accumulator tiles per wave
constexpr int MAX_LDS = 64 * 1024;
constexpr int BT = 32, BP = BT / 4;                      // positions per workgroup and per wave of the boundary kernel

__device__ __forceinline__ int utt_len(const int32_t* n_frames, int b, int len_mul, int L_cap)
{
  int nf = n_frames[b];
  nf = nf > 0 ? nf : 0;
  const long long len64 = (long long)nf * len_mul;
  return len64 < L_cap ? (int)len64 : L_cap;
}

__global__ __launch_bounds__(NT, 2) void gt_wg_gate_kernel(const gt_wg_gate_args a)
{
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
  bf16_t* xs = reinterpret_cast<bf16_t*>(lds_raw);                                // [rows][PITCH]

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.z, t0 = blockIdx.x * TM;
  const int len = utt_len(a.n_frames, b, a.len_mul, a.L_cap);
  bf16_t* G = static_cast<bf16_t*>(a.G) + (size_t)b * (size_t)a.g_stride_b;

  if (t0 >= len) {                                                                // behind the utterance: zeros, nothing is read
    for (int i = tid; i < TM * 128; i += NT) {
      const int t = t0 + (i >> 7), n = blockIdx.y * 128 + (i & 127);
      if (t < a.L_cap && n < a.C) G[(size_t)t * a.C + n] = 0;
    }
    return;
  }

  const int hl = (a.taps >> 1) * a.dil, rows = TM + 2 * hl;
  const int q = blockIdx.y * 4 + wave;                                            // this wave's 32 gate channels: 32 q .. 32 q + 31
  const bool live = q < (a.C >> 5);                                               // wave-uniform (C = 64: two waves have no channels)
  const int Np32 = a.C >> 4;                                                      // 32-row tiles of the interleaved 2C rows
  const int r32 = lane & 31, h = lane >> 5;
  const bf16_t* Win = static_cast<const bf16_t*>(a.W_in);
  const bf16_t* Wc = static_cast<const bf16_t*>(a.W_cond);

  f32x16_t acc[MT][2];
  acc_zero(acc);

  // ---- taps x C from the residual stream --------------------------------------------------------------------------------------------
  const float* X = a.X + (size_t)b * (size_t)a.x_stride_b;
  const int KSTx = a.C >> 4;
  for (int c0 = 0; c0 < a.C; c0 += KC) {
    if (c0) __syncthreads();                                                      // the chunk before is consumed
    for (int i = tid; i < rows * (KC / 8); i += NT) {
      const int row = i >> 3, cg = (i & 7) * 8, p = t0 - hl + row;
      uint4 o = make_uint4(0, 0, 0, 0);
      if (p >= 0 && p < len) {
        const float* src = X + (size_t)p * a.ldx + c0 + cg;
        const float4 q0 = *reinterpret_cast<const float4*>(src);
        const float4 q1 = *reinterpret_cast<const float4*>(src + 4);
        o = make_uint4(pack2bf(q0.x, q0.y), pack2bf(q0.z, q0.w), pack2bf(q1.x, q1.y), pack2bf(q1.z, q1.w));
      }
      *reinterpret_cast<uint4*>(xs + row * PITCH + cg) = o;
    }
    __syncthreads();
    if (live) {
      const int ks0 = (c0 / KC) * KS;
      for (int j = 0; j < a.taps; ++j) {
        const bf16_t* xr = xs + (r32 + j * a.dil) * PITCH + 8 * h;               // row <= TM - 1 + (taps - 1) dil = rows - 1
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
          bf16x8_t af[MT];
#pragma unroll
          for (int mt = 0; mt < MT; ++mt) af[mt] = asfrag(*reinterpret_cast<const uint4*>(xr + mt * 32 * PITCH + ks * 16));
#pragma unroll
          for (int nt = 0; nt < 2; ++nt) {
            const bf16x8_t bfr = asfrag(ldfrag(Win, (j * Np32 + 2 * q + nt) * KSTx + ks0 + ks, lane));
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) acc[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[mt], bfr, acc[mt][nt], 0, 0, 0);
          }
        }
      }
    }
  }

  // ---- Cs from the spect: the conditioning layer's slice as further K steps ---------------------------------------------------------
  const bf16_t* S = static_cast<const bf16_t*>(a.S) + (size_t)b * (size_t)a.s_stride_b;
  const int KSTs = a.Cs >> 4;
  for (int c0 = 0; c0 < a.Cs; c0 += KC) {
    __syncthreads();
    for (int i = tid; i < TM * (KC / 8); i += NT) {
      const int row = i >> 3, cg = (i & 7) * 8, p = t0 + row;
      uint4 o = make_uint4(0, 0, 0, 0);
      if (p < len) o = *reinterpret_cast<const uint4*>(S + (size_t)p * a.Cs + c0 + cg);
      *reinterpret_cast<uint4*>(xs + row * PITCH + cg) = o;
    }
    __syncthreads();
    if (live) {
      const int ks0 = (c0 / KC) * KS;
      const bf16_t* xr = xs + r32 * PITCH + 8 * h;
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
        bf16x8_t af[MT];
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) af[mt] = asfrag(*reinterpret_cast<const uint4*>(xr + mt * 32 * PITCH + ks * 16));
#pragma unroll
        for (int nt = 0; nt < 2; ++nt) {
          const bf16x8_t bfr = asfrag(ldfrag(Wc, (2 * q + nt) * KSTs + ks0 + ks, lane));
#pragma unroll
          for (int mt = 0; mt < MT; ++mt) acc[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[mt], bfr, acc[mt][nt], 0, 0, 0);
        }
      }
    }
  }

  // ---- the gate, from the accumulators: column = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5) --------------------------
  if (!live) return;
  const int n = q * 32 + r32;                                                     // < C
  const float bt0 = a.b_in[n], bt1 = a.b_cond[n], bs0 = a.b_in[n + a.C], bs1 = a.b_cond[n + a.C];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int t = t0 + mt * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
      if (t >= a.L_cap) continue;
      float g = 0.f;
      if (t < len) g = tanhf_(acc[mt][0][r] + bt0 + bt1) * sigmoidf_(acc[mt][1][r] + bs0 + bs1);
      G[(size_t)t * a.C + n] = f2bf(g);
    }
  }
}

__global__ __launch_bounds__(NT) void gt_wg_boundary_kernel(const gt_wg_boundary_args a)
{
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int b = blockIdx.z;
  const int len = utt_len(a.n_frames, b, a.len_mul, a.L_cap);
  const int lo = 8 - a.c_in, first1 = 8 - (a.c_in >> 1);                          // the window before, its coupled half
  const int lo2 = 8 - a.c_out, hi2 = lo2 + (a.c_out >> 1);                        // the window after, the half the next WaveNet reads
  const uint32_t key = randn_key(a.seed_dev ? *a.seed_dev : a.seed, GT_WG_NOISE_STREAM, (uint32_t)b);
  float* st = a.state + (size_t)b * (size_t)a.st_stride_b;
  float* A = a.A + (size_t)b * (size_t)a.a_stride_b;
  const int C = a.C;
  float wi[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};                        // row (lane & 7) of the inverse 1x1's image
  if (a.w_inv) {
    const float4 i0 = *reinterpret_cast<const float4*>(a.w_inv + (lane & 7) * 8), i1 = *reinterpret_cast<const float4*>(a.w_inv + (lane & 7) * 8 + 4);
    wi[0] = i0.x; wi[1] = i0.y; wi[2] = i0.z; wi[3] = i0.w; wi[4] = i1.x; wi[5] = i1.y; wi[6] = i1.z; wi[7] = i1.w;
  }

  for (int i = 0; i < BP; ++i) {
    const int t = blockIdx.x * BT + wave * BP + i;
    if (t >= a.L_cap) break;
    if (t >= len) {                                                               // behind the utterance: the last form leaves zeros
      if (!a.w_start && lane < 8) A[(size_t)t * 8 + lane] = 0.f;
      continue;
    }
    float v[8];
#pragma unroll
    for (int s = 0; s < 8; ++s) v[s] = 0.f;
    if (a.w_end) {
      const float4 q0 = *reinterpret_cast<const float4*>(A + (size_t)t * 8), q1 = *reinterpret_cast<const float4*>(A + (size_t)t * 8 + 4);
      const float in[8] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w};
#pragma unroll
      for (int s = 0; s < 8; ++s) v[s] = s >= lo ? in[s] : 0.f;
      // 1. the end convolution of the coupled slots (4 .. 7 at the most): shift es, log-scale el
      float es[4], el[4];
#pragma unroll
      for (int s = 0; s < 4; ++s) es[s] = el[s] = 0.f;
      const float* sk = st + (size_t)t * a.ld + C;
      for (int c = lane; c < C; c += 64) {
        const float x = sk[c];
        const float4 w0 = *reinterpret_cast<const float4*>(a.w_end + (size_t)c * 8), w1 = *reinterpret_cast<const float4*>(a.w_end + (size_t)c * 8 + 4);
        const float wv[8] = {w0.x, w0.y, w0.z, w0.w, w1.x, w1.y, w1.z, w1.w};
#pragma unroll
        for (int s = 0; s < 4; ++s) {
          if (4 + s >= first1) {
            es[s] = fmaf(x, wv[s], es[s]);
            el[s] = fmaf(x, wv[4 + s], el[s]);
          }
        }
      }
      // 2. the coupling inverse
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        if (4 + s >= first1) {                                                    // wave-uniform: every lane takes part in the butterfly
          const float sh = wave_sum(es[s]) + a.b_end[s], ls = wave_sum(el[s]) + a.b_end[4 + s];
          v[4 + s] = (v[4 + s] - sh) * expf(-ls);
        }
      }
      // 3. the inverse 1x1 convolution on the 8-slot image: lane s computes row s, every lane then takes all eight
      float row = 0.f;
#pragma unroll
      for (int k = 0; k < 8; ++k) row = fmaf(wi[k], v[k], row);
#pragma unroll
      for (int s = 0; s < 8; ++s) {
        const float r = __shfl(row, s);
        v[s] = s >= lo ? r : 0.f;
      }
    }
    // 4. the new slots [lo2, lo): the latent, pair p by lane p and handed to every lane
    if (lo2 < lo) {
      float e0, e1;
      randn_pair(key, (uint32_t)t, (uint32_t)(lane & 3), e0, e1);
#pragma unroll
      for (int p = 0; p < 4; ++p) {
        const float n0 = __shfl(e0, p), n1 = __shfl(e1, p);
        if (2 * p >= lo2 && 2 * p < lo) { v[2 * p] = a.sigma * n0; v[2 * p + 1] = a.sigma * n1; }
      }
    }
    if (lane == 0) {
      *reinterpret_cast<float4*>(A + (size_t)t * 8) = make_float4(v[0], v[1], v[2], v[3]);
      *reinterpret_cast<float4*>(A + (size_t)t * 8 + 4) = make_float4(v[4], v[5], v[6], v[7]);
    }
    // 5. the next WaveNet's start convolution into the residual stream; its skip accumulator starts from 0
    if (a.w_start) {
      float* xr = st + (size_t)t * a.ld;
      for (int n = lane; n < C; n += 64) {
        const float4 w0 = *reinterpret_cast<const float4*>(a.w_start + (size_t)n * 8);
        const float4 w1 = *reinterpret_cast<const float4*>(a.w_start + (size_t)n * 8 + 4);
        const float ws[8] = {w0.x, w0.y, w0.z, w0.w, w1.x, w1.y, w1.z, w1.w};
        float acc = a.b_start[n];
#pragma unroll
        for (int s = 0; s < 8; ++s)
          if (s >= lo2 && s < hi2) acc = fmaf(ws[s], v[s], acc);
        xr[n] = acc;
        xr[C + n] = 0.f;
      }
    }
  }
}

}  // namespace

extern "C" int gt_wg_tile_positions(void) { return TM; }
extern "C" int gt_wg_gate_args_size(void) { return (int)sizeof(gt_wg_gate_args); }
extern "C" int gt_wg_boundary_args_size(void) { return (int)sizeof(gt_wg_boundary_args); }

extern "C" size_t gt_wg_gate_lds_bytes(int C, int taps, int dil)
{
  if (C <= 0 || C % 64 || taps <= 0 || !(taps & 1) || taps > GT_VOC_MAX_TAPS || dil <= 0) return 0;
  const long long bytes = ((long long)TM + (long long)(taps - 1) * dil) * (PITCH * 2);
  return bytes > MAX_LDS ? 0 : (size_t)bytes;
}

extern "C" int gt_wg_gate(const gt_wg_gate_args* args, void* stream)
{
  if (!args) return GT_E_INVAL;
  const gt_wg_gate_args& a = *args;
  if (!a.X || !a.S || !a.W_in || !a.W_cond || !a.b_in || !a.b_cond || !a.G || !a.n_frames) return GT_E_INVAL;
  if (a.B <= 0 || a.L_cap <= 0 || a.C <= 0 || a.Cs <= 0 || a.dil <= 0 || a.len_mul <= 0 || a.taps <= 0 || !(a.taps & 1)) return GT_E_INVAL;
  if (a.ldx < a.C || a.x_stride_b < (long long)a.L_cap * a.ldx || a.s_stride_b < (long long)a.L_cap * a.Cs ||
      a.g_stride_b < (long long)a.L_cap * a.C)
    return GT_E_INVAL;
  if (a.G == (const void*)a.X || a.G == a.S) return GT_E_INVAL;
  if (a.taps > GT_VOC_MAX_TAPS || a.C % 64 || a.Cs % 64 || a.B > 65535) return GT_E_UNSUPPORTED;
  const long long width = a.ldx > a.Cs ? a.ldx : a.Cs;
  if ((long long)a.B * a.L_cap * width >= (1ll << 31)) return GT_E_UNSUPPORTED;
  const size_t lds = gt_wg_gate_lds_bytes(a.C, a.taps, a.dil);
  if (!lds) return GT_E_UNSUPPORTED;
  if (!al16(a.X) || !al16(a.S) || !al16(a.W_in) || !al16(a.W_cond) || ((uintptr_t)a.b_in & 3) || ((uintptr_t)a.b_cond & 3) ||
      ((uintptr_t)a.G & 3) || ((uintptr_t)a.n_frames & 3) || (a.ldx & 3) || (a.x_stride_b & 3) || (a.s_stride_b & 7))
    return GT_E_ALIGN;
  const dim3 grid((a.L_cap + TM - 1) / TM, (a.C + 127) / 128, a.B);
  hipLaunchKernelGGL(gt_wg_gate_kernel, grid, dim3(NT), lds, GT_ST(stream), a);
  GT_RET();
}

extern "C" int gt_wg_boundary(const gt_wg_boundary_args* args, void* stream)
{
  if (!args) return GT_E_INVAL;
  const gt_wg_boundary_args& a = *args;
  if (!a.state || !a.A || !a.n_frames) return GT_E_INVAL;
  if (a.B <= 0 || a.L_cap <= 0 || a.C <= 0 || a.len_mul <= 0) return GT_E_INVAL;
  if (a.ld < 2ll * a.C || a.st_stride_b < (long long)a.L_cap * a.ld || a.a_stride_b < 8ll * a.L_cap) return GT_E_INVAL;
  if ((a.c_in & 1) || (a.c_out & 1) || a.c_in < 0 || a.c_in > 8 || a.c_out < 2 || a.c_out > 8 || a.c_out < a.c_in) return GT_E_INVAL;
  const int n_end = (a.w_end != nullptr) + (a.b_end != nullptr) + (a.w_inv != nullptr);
  if ((n_end != 0 && n_end != 3) || (n_end != 0) != (a.c_in > 0)) return GT_E_INVAL;
  if ((a.w_start != nullptr) != (a.b_start != nullptr) || (!a.w_start && a.c_out != 8)) return GT_E_INVAL;
  if (!(a.sigma >= 0.f)) return GT_E_INVAL;
  if (a.C % 64 || a.C > GT_WG_MAX_C || a.B > 65535 || (long long)a.B * a.L_cap * a.ld >= (1ll << 31)) return GT_E_UNSUPPORTED;
  if (!al16(a.A) || !al16(a.w_inv) || !al16(a.w_start) || !al16(a.w_end) || ((uintptr_t)a.state & 3) || ((uintptr_t)a.b_end & 3) ||
      ((uintptr_t)a.b_start & 3) || ((uintptr_t)a.n_frames & 3) || ((uintptr_t)a.seed_dev & 3) || (a.ld & 3) || (a.st_stride_b & 3) ||
      (a.a_stride_b & 3))
    return GT_E_ALIGN;
  const dim3 grid((a.L_cap + BT - 1) / BT, 1, a.B);
  hipLaunchKernelGGL(gt_wg_boundary_kernel, grid, dim3(NT), 0, GT_ST(stream), a);
  GT_RET();
}
