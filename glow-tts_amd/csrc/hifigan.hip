// HiFi-GAN generator on the device: ONE kernel carries every layer — a dilated 1-D convolution on dense channels-last
// activations as an implicit GEMM on v_mfma_f32_32x32x16_bf16, with a leaky-ReLU prologue and a bias / residual / MRF-sum / scale / tanh
// epilogue.  The transposed convolutions are this kernel too (a 3-tap convolution to u * Cout channels, read back as u times the
// positions), conv_pre reads the decoder's channel-major mel through a transposing staging pass, conv_post is N = 1 in a padded image.
//
//   definition  Y[b, t, n] = epi( sum_{j < taps} sum_{ci} bf16( lrelu_slope( X[b, t + (j - taps / 2) dil, ci] ) ) W[j][n][ci] ),  t < len_b
//               len_b = min(max(n_frames[b], 0) len_mul, L_cap); a tap outside [0, len_b) contributes 0 and is never read; outputs at
//               [len_b, L_cap) are written as 0.  epi(s) = tanh?( (s + bias[n] + res + acc) scale ).
//   tile        a workgroup of four waves owns TM = 128 positions x BN channels of one utterance; BN = 128 (waves 1 x 4: each all 128
//               positions x 32 channels), 64 (waves 2 x 2, 64 x 32) or 32 (4 x 1, 32 x 32), chosen by N.  A wave takes ONE 32-column
//               tile wherever N allows: no two waves of a workgroup then load the same weight fragment (measured on the bench batch:
//               58.1 -> 45.6 ms against waves of 64 x 64 / 32 x 64, whose column tiles were loaded twice / four times).  Per Cin chunk of KC = 64 channels (32 where Cin is no
//               multiple of 64) it stages TM + (taps - 1) dil positions in LDS ONCE — prologue applied, bf16, zeros outside the
//               utterance — and walks the taps over that one tile: tap j of output row m is LDS row m + j dil.
//   LDS         dynamic, (TM + (taps - 1) dil) rows of KC bf16 + 16 bytes: a row pitch of 144 (80) bytes = 9 (5) 16-byte slots, odd, so
//               the 16 rows one ds_read_b128 lane group touches (any 16 rows with distinct row mod 16: the groups of 16 lanes are
//               rows {0-3, 12-15, 20-27} and {4-11, 16-19, 28-31} of the fragment plus a common tap shift) fall into 16 distinct slots.
//               At most 64 KB; taps 11, dil 5: 178 rows = 25 632 bytes.
//   weights     the image is in MFMA-fragment order, [taps][Np / 32][Kp / 16][64 lanes][8] bf16 with lane = 32 h + r holding
//               W[j][32 nt + r][16 ks + 8 h + e] (zeros for n >= N and ci >= Cin; Np = N rounded up to 32, Kp = Cin rounded up to KC): a
//               B fragment is one coalesced 16-byte load per lane straight from global memory (L2), no LDS.
//   order       fp32 accumulation in the MFMA over (chunk, tap, k-step) ascending, fixed by (t mod TM, n, Cin, taps) alone: a batch row is
//               bit-identical to the utterance computed alone, and to the same utterance in a buffer of another capacity.
//   bounds      every global access is predicated by position (< len_b for reads, < L_cap for writes) and channel (< Cin, < N); LDS rows
//               are < TM + (taps - 1) dil by construction; all offsets are size_t.
#include "common.h"
#include "internal.h"
#include "mfma_frag.h"
#include "../../include/glowtts_hip.h"

namespace {

constexpr int NT = 256;                                  // threads: four waves
constexpr int TM = 128;                                  // positions per workgroup
constexpr int MAX_LDS = 64 * 1024;

__host__ __device__ constexpr int k_chunk(int Cin) { return (Cin % 64) ? 32 : 64; }

__device__ __forceinline__ float lrelu(float v, float slope) { return v < 0.f ? v * slope : v; }

// WM waves along the positions, MT 32-row and NTW 32-column accumulator tiles per wave, KS 16-deep k-steps per staged chunk
template <int WM, int MT, int NTW, int KS>
__global__ __launch_bounds__(NT, 2) void gt_voc_conv_kernel(const gt_voc_conv_args a)
{
  static_assert(WM * MT * 32 == TM, "a workgroup owns TM positions");
  constexpr int WN = 4 / WM, BN = WN * NTW * 32, KC = KS * 16, PITCH = KC + 8;   // PITCH in bf16 elements
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
  bf16_t* xs = reinterpret_cast<bf16_t*>(lds_raw);                                // [rows][PITCH]

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.z, t0 = blockIdx.x * TM, n0 = blockIdx.y * BN;
  int nf = a.n_frames[b];
  nf = nf > 0 ? nf : 0;
  const long long len64 = (long long)nf * a.len_mul;
  const int len = len64 < a.L_cap ? (int)len64 : a.L_cap;
  const size_t ybase = (size_t)b * (size_t)a.y_stride_b;

  if (t0 >= len) {                                                                // behind the utterance: zeros, nothing is read
    for (int i = tid; i < TM * BN; i += NT) {
      const int t = t0 + i / BN, n = n0 + i % BN;
      if (t < a.L_cap && n < a.N) {
        const size_t off = ybase + (size_t)t * a.ldy + n;
        if (a.y_bf16) static_cast<bf16_t*>(a.Y)[off] = 0; else static_cast<float*>(a.Y)[off] = 0.f;
      }
    }
    return;
  }

  const int hl = (a.taps >> 1) * a.dil, rows = TM + 2 * hl;
  const int Np32 = (a.N + 31) >> 5, KST = ((a.Cin + KC - 1) / KC) * KS;           // 32-column tiles and 16-deep k-steps of the image
  const int wm = wave % WM, wn = wave / WM;
  const int m_base = wm * MT * 32, nt_base = (n0 >> 5) + wn * NTW;                // this wave's first row and first 32-column tile
  const int r32 = lane & 31, h = lane >> 5;
  const bf16_t* Wimg = static_cast<const bf16_t*>(a.W);

  f32x16_t acc[MT][NTW];
  acc_zero(acc);

  for (int c0 = 0; c0 < a.Cin; c0 += KC) {
    if (c0) __syncthreads();                                                      // the chunk before is consumed
    if (a.x_mel) {                                                                // [B, Cin, >= L] frames contiguous: transposing pass
      const float* X = static_cast<const float*>(a.X) + (size_t)b * (size_t)a.x_stride_b;
      for (int i = tid; i < KC * rows; i += NT) {
        const int cc = i / rows, row = i - cc * rows, p = t0 - hl + row, c = c0 + cc;
        float v = 0.f;
        if (p >= 0 && p < len && c < a.Cin) v = lrelu(X[(size_t)c * (size_t)a.x_stride_c + p], a.slope);
        xs[row * PITCH + cc] = f2bf(v);
      }
    } else {
      constexpr int CPR = KC / 8;                                                 // 8-channel pieces per row
      for (int i = tid; i < rows * CPR; i += NT) {
        const int row = i / CPR, cg = (i - row * CPR) * 8, p = t0 - hl + row, c = c0 + cg;
        uint4 o = make_uint4(0, 0, 0, 0);
        if (p >= 0 && p < len && c < a.Cin) {                                     // Cin % 16 == 0: the piece is inside the row
          const size_t off = (size_t)b * (size_t)a.x_stride_b + (size_t)p * a.Cin + c;
          float v[8];
          if (a.x_bf16) {
            const uint4 u = *reinterpret_cast<const uint4*>(static_cast<const bf16_t*>(a.X) + off);
            v[0] = bf2f(u.x & 0xffff); v[1] = bf2f(u.x >> 16); v[2] = bf2f(u.y & 0xffff); v[3] = bf2f(u.y >> 16);
            v[4] = bf2f(u.z & 0xffff); v[5] = bf2f(u.z >> 16); v[6] = bf2f(u.w & 0xffff); v[7] = bf2f(u.w >> 16);
          } else {
            const float4 q0 = *reinterpret_cast<const float4*>(static_cast<const float*>(a.X) + off);
            const float4 q1 = *reinterpret_cast<const float4*>(static_cast<const float*>(a.X) + off + 4);
            v[0] = q0.x; v[1] = q0.y; v[2] = q0.z; v[3] = q0.w; v[4] = q1.x; v[5] = q1.y; v[6] = q1.z; v[7] = q1.w;
          }
#pragma unroll
          for (int e = 0; e < 8; ++e) v[e] = lrelu(v[e], a.slope);
          o = make_uint4(pack2bf(v[0], v[1]), pack2bf(v[2], v[3]), pack2bf(v[4], v[5]), pack2bf(v[6], v[7]));
        }
        *reinterpret_cast<uint4*>(xs + row * PITCH + cg) = o;
      }
    }
    __syncthreads();

    const int ks0 = (c0 / KC) * KS;
    for (int j = 0; j < a.taps; ++j) {
      const bf16_t* xr = xs + (m_base + r32 + j * a.dil) * PITCH + 8 * h;        // row <= TM - 1 + (taps - 1) dil = rows - 1
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
        bf16x8_t af[MT];
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) af[mt] = asfrag(*reinterpret_cast<const uint4*>(xr + mt * 32 * PITCH + ks * 16));
#pragma unroll
        for (int nt = 0; nt < NTW; ++nt) {
          if (nt_base + nt < Np32) {                                              // wave-uniform: tiles past the image do not exist
            const bf16x8_t bfr = asfrag(ldfrag(Wimg, (j * Np32 + nt_base + nt) * KST + ks0 + ks, lane));
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) acc[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[mt], bfr, acc[mt][nt], 0, 0, 0);
          }
        }
      }
    }
  }

  // epilogue from the accumulators: column = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5): 32 lanes store 32 consecutive channels
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) {
#pragma unroll
    for (int nt = 0; nt < NTW; ++nt) {
      const int n = (nt_base + nt) * 32 + r32;
      if (n >= a.N) continue;
      const float bn = a.bias[n];
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int t = t0 + m_base + mt * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
        if (t >= a.L_cap) continue;
        const size_t off = ybase + (size_t)t * a.ldy + n;
        float v = 0.f;
        if (t < len) {
          v = acc[mt][nt][r] + bn;
          if (a.res) v += a.res[off];
          if (a.acc) v += a.acc[off];
          v *= a.scale;
          if (a.tanh_out) v = tanhf_(v);
        }
        if (a.y_bf16) static_cast<bf16_t*>(a.Y)[off] = f2bf(v); else static_cast<float*>(a.Y)[off] = v;
      }
    }
  }
}

template <int WM, int MT, int NTW, int KS>
int launch(const gt_voc_conv_args& a, int lds, hipStream_t stream)
{
  constexpr int BN = (4 / WM) * NTW * 32;
  const dim3 grid((a.L_cap + TM - 1) / TM, (a.N + BN - 1) / BN, a.B);
  hipLaunchKernelGGL((gt_voc_conv_kernel<WM, MT, NTW, KS>), grid, dim3(NT), lds, stream, a);
  return gt_launch_status("gt_voc_conv");
}

}  // namespace

extern "C" int gt_voc_tile_positions(void) { return TM; }
extern "C" int gt_voc_conv_args_size(void) { return (int)sizeof(gt_voc_conv_args); }
extern "C" int gt_voc_k_chunk(int Cin) { return (Cin <= 0 || Cin % 16) ? 0 : k_chunk(Cin); }

extern "C" size_t gt_voc_lds_bytes(int Cin, int taps, int dil)
{
  if (Cin <= 0 || Cin % 16 || taps <= 0 || !(taps & 1) || taps > GT_VOC_MAX_TAPS || dil <= 0) return 0;
  const long long bytes = ((long long)TM + (long long)(taps - 1) * dil) * (k_chunk(Cin) * 2 + 16);
  return bytes > MAX_LDS ? 0 : (size_t)bytes;
}

extern "C" int gt_voc_conv(const gt_voc_conv_args* args, void* stream)
{
  if (!args) return GT_E_INVAL;
  const gt_voc_conv_args& a = *args;
  if (!a.X || !a.W || !a.bias || !a.Y || !a.n_frames) return GT_E_INVAL;
  if (a.B <= 0 || a.L_cap <= 0 || a.Cin <= 0 || a.N <= 0 || a.taps <= 0 || !(a.taps & 1) || a.dil <= 0 || a.len_mul <= 0) return GT_E_INVAL;
  if (a.ldy < (a.N > 1 ? a.N : 1) || a.y_stride_b < (long long)a.L_cap * a.ldy) return GT_E_INVAL;
  if (a.x_mel ? (a.x_stride_c < a.L_cap || a.x_stride_b < a.L_cap || a.x_bf16) : a.x_stride_b < (long long)a.L_cap * a.Cin) return GT_E_INVAL;
  if (a.Y == a.X) return GT_E_INVAL;
  if (a.taps > GT_VOC_MAX_TAPS || a.Cin % 16 || a.B > 65535) return GT_E_UNSUPPORTED;
  const long long width = a.Cin > a.N ? a.Cin : a.N;
  if ((long long)a.B * a.L_cap * width >= (1ll << 31)) return GT_E_UNSUPPORTED;
  const size_t lds = gt_voc_lds_bytes(a.Cin, a.taps, a.dil);
  if (!lds) return GT_E_UNSUPPORTED;
  if (!al16(a.W) || ((uintptr_t)a.bias & 3) || ((uintptr_t)a.n_frames & 3) || ((uintptr_t)a.Y & 3) || ((uintptr_t)a.res & 3) ||
      ((uintptr_t)a.acc & 3))
    return GT_E_ALIGN;
  if (a.x_mel ? ((uintptr_t)a.X & 3) != 0 : (!al16(a.X) || (a.x_stride_b & 7))) return GT_E_ALIGN;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const bool k64 = k_chunk(a.Cin) == 64;
  if (a.N > 64) return k64 ? launch<1, 4, 1, 4>(a, (int)lds, st) : launch<1, 4, 1, 2>(a, (int)lds, st);
  if (a.N > 32) return k64 ? launch<2, 2, 1, 4>(a, (int)lds, st) : launch<2, 2, 1, 2>(a, (int)lds, st);
  return k64 ? launch<4, 1, 1, 4>(a, (int)lds, st) : launch<4, 1, 1, 2>(a, (int)lds, st);
}
