// Objective synthesis metrics on the device: mel cepstra, dynamic time warping and F0 statistics along the warping path.
//
//   gt_mel_cepstrum   ragged log-mel [B, N, ld] (channel-major) -> [B, F_max, 16] rows of 64 bytes: c[k] = sum_n dct[k][n] m[n], ONE
//                     mul + add chain over n ascending per coefficient (contraction is off).  A lane owns a frame, so the reads are
//                     coalesced along time; the matrix sits in LDS as [n][16] and is read by broadcast.
//   gt_dtw_f32        D(i,j) = d(i,j) + min(D(i-1,j-1), D(i-1,j), D(i,j-1)), first of that order on ties, d = alpha sqrt(sum_k (a-b)^2),
//                     one workgroup per utterance:
//     lanes    lane l of a band owns row i = 64 band + l, its 16 features in registers.  Columns are walked skewed by one per lane
//              (lane l is at column t - l at wave step t), so D(i-1, j) is lane l-1's value of the step before (one wave_shr:1 DPP),
//              D(i-1, j-1) is what that DPP returned one step earlier and D(i, j-1) is the lane's own last value.
//     waves    wave w owns bands w, w + W, ...; a band runs LAG = 3 chunks of 32 steps behind the band above it (96 >= 63 + 32 + 1
//              steps: the last row of the band above reaches column j at its step j + 63), one barrier per chunk.  Lane 63's values
//              cross to the next wave through a ring of 128 floats per wave in LDS; past 16 bands the rows take several passes and
//              the last band of a pass leaves its whole last row in LDS for the first band of the next.
//     columns  b's features come from an LDS image [k / 4][j] of float4 (lane l reads slot t - l: consecutive 16-byte slots, no bank
//              conflict for ds_read_b128) where it fits next to the rings, else straight from global memory through L1.
//     bits     the fp32 lattice is never stored: a cell emits 2 direction bits (0 diagonal, 1 (i-1, j), 2 (i, j-1)), 16 cells to a
//              dword, into the workspace [B, Fa_max, nq] (nq = words per row rounded up to 4).
//     path     a second kernel behind the DP (the walk is serial: the DP's waves have nothing to do in it, and a kernel of its own
//              shows in a trace what the walk costs).  Its wave 0 walks back: lane l holds the four direction words of row i - l
//              around column j (one 16-byte load per 64 x 64 cell tile), a v_readlane hands the walk the word it is at, so a
//              dependent global load is paid once per tile, not once per step.  The cells go, packed (i << 16 | j), to the
//              workspace in walk order; then the workgroup writes the path forward from (0, 0) and -1 behind it.
//              cost is the DP's own last cell.
//   gt_dtw_f0_stats   counts and sums over the path's steps, one workgroup per utterance: per-thread sums in path order with stride
//                     256, then one LDS tree in a fixed order — no atomics, a batch row is the utterance alone.  The cents term and the
//                     gross-error compare are formed in fp64: fp32 log2 of a ratio next to 1 keeps no relative accuracy.
//
// No arithmetic of a cell depends on B, the capacities, the schedule or the LDS / global choice: a batch row is bit-identical to the
// utterance alone.  Correctly rounded sqrtf and IEEE adds only (contraction off).
#include <hip/hip_runtime.h>
#include "common.h"
#pragma clang fp contract(off)
#include <stdint.h>
#include "../../include/glowtts_hip.h"
#include "internal.h"

namespace {

constexpr int CHS  = 32;                 // wave steps per chunk: one barrier per chunk
constexpr int LAG  = 3;                  // chunks a band runs behind the band above it
constexpr int RING = 128;                // floats of a wave's boundary ring (a column is read 96..127 steps after it was written)
constexpr int MAXW = 16;                 // waves of a workgroup
constexpr size_t LDS_CAP = 160 * 1024;

__host__ __device__ inline int dtw_nq(int Fb_max) { return ((Fb_max + 15) / 16 + 3) & ~3; }
__host__ __device__ inline int dtw_revcap(int Fa_max, int Fb_max) { return (Fa_max + Fb_max + 63) & ~63; }
inline int dtw_waves(int Fa_max) { const int nb = (Fa_max + 63) / 64; return nb < MAXW ? nb : MAXW; }

// LDS of one workgroup: [b image, 64 Fb_max bytes, where it fits] [W rings] [the pass row, Fb_max floats, past 16 bands]
size_t dtw_lds(int Fa_max, int Fb_max, bool* image)
{
  const size_t fixed = (size_t)dtw_waves(Fa_max) * RING * 4 + (Fa_max > 64 * MAXW ? ((size_t)Fb_max * 4 + 15) / 16 * 16 : 0);
  const size_t img = (size_t)Fb_max * 64;
  *image = fixed + img <= LDS_CAP;
  return *image ? fixed + img : fixed;
}

__device__ __forceinline__ float dpp_shr1(float old, float src) {
  // lane l <- src[l - 1]; lane 0 keeps `old` (bound_ctrl off)
  return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(old), __float_as_int(src), 0x138 /*wave_shr:1*/, 0xf, 0xf, false));
}

struct DtwArgs {
  const float* a; const float* b; const int32_t* a_len; const int32_t* b_len;
  float* cost; int32_t* path_len; int32_t* path; uint32_t* dirs; uint32_t* rev; int32_t* status;
  int Fa_max, Fb_max, ld_path, nq; float alpha;
};

template <bool IMAGE>
__global__ __launch_bounds__(1024) void gt_dtw_kernel(DtwArgs p)
{
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int W = blockDim.x >> 6, NT = blockDim.x;
  const int Fbm = p.Fb_max;

  int Fa = p.a_len[b], Fb = p.b_len[b];
  if (Fa < 0 || Fb < 0 || Fa > p.Fa_max || Fb > Fbm) {
    if (tid == 0 && p.status) atomicOr(p.status, GT_DTW_ST_BAD_LEN);
    Fa = 0; Fb = 0;
  }
  if (Fa == 0 || Fb == 0) { Fa = 0; Fb = 0; }                    // an empty side: cost 0, no path

  float4* bimg    = reinterpret_cast<float4*>(smem);              // [4][Fb_max]
  float*  rings   = reinterpret_cast<float*>(smem + (IMAGE ? (size_t)Fbm * 64 : 0));
  float*  passrow = rings + W * RING;                             // only past 16 bands (the host sized it then)
  const float4* ag = reinterpret_cast<const float4*>(p.a) + (size_t)b * p.Fa_max * 4;
  const float4* bg = reinterpret_cast<const float4*>(p.b) + (size_t)b * Fbm * 4;

  if (IMAGE) {
    for (int idx = tid; idx < Fb * 4; idx += NT) bimg[(idx & 3) * Fbm + (idx >> 2)] = bg[idx];
  }
  __syncthreads();

  // ---------------- forward DP: direction bits into the workspace ----------------
  const int nb = (Fa + 63) >> 6;                                  // bands of this utterance
  const int NC = (Fb + 63 + CHS - 1) / CHS;                       // chunks of one band: Fb + 63 wave steps
  const int P  = (NC > LAG * W ? NC : LAG * W) + 1;               // chunks between the passes of one wave
  const int total = nb ? ((nb - 1) / W) * P + LAG * ((nb - 1) % W) + NC : 0;
  const float INF = __builtin_inff();

  float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f, a4 = 0.f, a5 = 0.f, a6 = 0.f, a7 = 0.f;
  float a8 = 0.f, a9 = 0.f, a10 = 0.f, a11 = 0.f, a12 = 0.f, a13 = 0.f, a14 = 0.f, a15 = 0.f;
  float cur = INF, upp = INF;
  unsigned dw = 0;
  int row = 0;
  bool row_ok = false, has_in = false;
  const float* rin = rings;
  float* rout = rings;
  unsigned imask = RING - 1, omask = RING - 1;
  uint32_t* drow = p.dirs;

  for (int k = 0; k < total; ++k) {
    const int kk = k - LAG * w;
    if (kk >= 0) {
      const int pass = kk / P, c = kk - pass * P;
      const int g = pass * W + w;
      if (c < NC && g < nb) {
        if (c == 0) {                                             // a new band: its rows' features, an empty column behind it
          row = g * 64 + lane;
          row_ok = row < Fa;
          float4 f0 = make_float4(0.f, 0.f, 0.f, 0.f), f1 = f0, f2 = f0, f3 = f0;
          if (row_ok) { f0 = ag[row * 4]; f1 = ag[row * 4 + 1]; f2 = ag[row * 4 + 2]; f3 = ag[row * 4 + 3]; }
          __builtin_amdgcn_s_waitcnt(0x0F70);                     // vmcnt(0) here: else every step below waits for its own stores
          a0 = f0.x; a1 = f0.y; a2 = f0.z; a3 = f0.w; a4 = f1.x; a5 = f1.y; a6 = f1.z; a7 = f1.w;
          a8 = f2.x; a9 = f2.y; a10 = f2.z; a11 = f2.w; a12 = f3.x; a13 = f3.y; a14 = f3.z; a15 = f3.w;
          cur = INF;
          upp = (g == 0 && lane == 0) ? 0.f : INF;                // D(-1, -1) = 0 makes D(0, 0) = d(0, 0)
          dw = 0;
          has_in = g > 0;
          if (w == 0) { rin = passrow; imask = 0xffffffffu; } else { rin = rings + (w - 1) * RING; imask = RING - 1; }
          if (w == W - 1 && nb > W) { rout = passrow; omask = 0xffffffffu; } else { rout = rings + w * RING; omask = RING - 1; }
          drow = p.dirs + ((size_t)b * p.Fa_max + (row_ok ? row : 0)) * p.nq;
        }
        // the column's features and lane 0's row above, one step ahead of their use: the loads' latency hides behind the step
        // before (columns clamped into [0, Fb): what a lane outside the lattice reads is never used)
        float4 n0, n1, n2, n3;
        float bn = INF;                                           // D(64 g - 1, t): lane 0's row above
        auto fetch = [&](int t) {
          if (has_in) bn = rin[(unsigned)(t < Fb ? t : Fb - 1) & imask];
          const int j = t - lane, jc = j < 0 ? 0 : (j < Fb ? j : Fb - 1);
          if (IMAGE) { n0 = bimg[jc]; n1 = bimg[Fbm + jc]; n2 = bimg[2 * Fbm + jc]; n3 = bimg[3 * Fbm + jc]; }
          else       { n0 = bg[jc * 4]; n1 = bg[jc * 4 + 1]; n2 = bg[jc * 4 + 2]; n3 = bg[jc * 4 + 3]; }
        };
        fetch(c * CHS);
#pragma unroll 2
        for (int s = 0; s < CHS; ++s) {
          const int t = c * CHS + s;
          const int j = t - lane;
          const bool act = row_ok && j >= 0 && j < Fb;
          const float4 q0 = n0, q1 = n1, q2 = n2, q3 = n3;
          const float bnd = bn;
          fetch(t + 1);
          float e, acc;
          e = a0 - q0.x;  acc = e * e;
          e = a1 - q0.y;  acc = acc + e * e;
          e = a2 - q0.z;  acc = acc + e * e;
          e = a3 - q0.w;  acc = acc + e * e;
          e = a4 - q1.x;  acc = acc + e * e;
          e = a5 - q1.y;  acc = acc + e * e;
          e = a6 - q1.z;  acc = acc + e * e;
          e = a7 - q1.w;  acc = acc + e * e;
          e = a8 - q2.x;  acc = acc + e * e;
          e = a9 - q2.y;  acc = acc + e * e;
          e = a10 - q2.z; acc = acc + e * e;
          e = a11 - q2.w; acc = acc + e * e;
          e = a12 - q3.x; acc = acc + e * e;
          e = a13 - q3.y; acc = acc + e * e;
          e = a14 - q3.z; acc = acc + e * e;
          e = a15 - q3.w; acc = acc + e * e;
          const float d = p.alpha * sqrtf(acc);

          const float up = dpp_shr1(bnd, cur);                    // D(i - 1, j)
          const float dg = upp;                                   // D(i - 1, j - 1)
          upp = up;
          float m = dg;
          unsigned dir = 0;
          if (up < m)  { m = up;  dir = 1; }
          if (cur < m) { m = cur; dir = 2; }
          const float nv = d + m;
          if (act) {
            cur = nv;
            dw |= dir << ((j & 15) * 2);
            if (lane == 63) rout[(unsigned)j & omask] = nv;
            if ((j & 15) == 15 || j == Fb - 1) { drow[j >> 4] = dw; dw = 0; }
            if (row == Fa - 1 && j == Fb - 1) p.cost[b] = nv;
          }
        }
      }
    }
    __syncthreads();
  }
}

// The path of one utterance from its direction words: wave 0 walks back, then the workgroup writes the path forward.  A kernel of its
// own behind the DP: the walk is serial, and the DP's sixteen waves have nothing to do in it.
__global__ __launch_bounds__(256) void gt_dtw_path_kernel(DtwArgs p)
{
  __shared__ int plen_sh;
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int Fbm = p.Fb_max;
  int Fa = p.a_len[b], Fb = p.b_len[b];
  if (Fa < 0 || Fb < 0 || Fa > p.Fa_max || Fb > Fbm) { Fa = 0; Fb = 0; }   // the DP kernel has set the status bit
  if (Fa == 0 || Fb == 0) { Fa = 0; Fb = 0; }

  // ---------------- backtrack (wave 0): 64 x 64 cell tiles of direction words in registers ----------------
  uint32_t* rev = p.rev + (size_t)b * dtw_revcap(p.Fa_max, Fbm);
  int plen = 0;
  if (w == 0 && Fa > 0) {
    const uint32_t* dbase = p.dirs + (size_t)b * p.Fa_max * p.nq;
    int i = Fa - 1, j = Fb - 1, n = 0;
    unsigned outv = 0;
    bool done = false;
    while (!done) {
      const int qb = (j >> 4) & ~3, jlo = qb << 4, ibase = i;
      const int r = i - lane;                                     // lane l: the words of row i - l
      uint4 tw = make_uint4(0u, 0u, 0u, 0u);
      if (r >= 0) tw = *reinterpret_cast<const uint4*>(dbase + (size_t)r * p.nq + qb);
      do {
        if (lane == (n & 63)) outv = ((unsigned)i << 16) | (unsigned)j;
        if ((n & 63) == 63) rev[(n & ~63) + lane] = outv;
        ++n;
        if (i == 0 && j == 0) { done = true; break; }
        const int ql = (j >> 4) & 3;
        const unsigned sel = ql == 0 ? tw.x : (ql == 1 ? tw.y : (ql == 2 ? tw.z : tw.w));
        const unsigned word = (unsigned)__builtin_amdgcn_readlane((int)sel, ibase - i);
        unsigned dir = (word >> ((j & 15) * 2)) & 3u;
        if (i == 0) dir = 2; else if (j == 0) dir = 1;            // the lattice's edges: one predecessor
        if (dir != 2) --i;
        if (dir != 1) --j;
      } while (i > ibase - 64 && j >= jlo);
    }
    if ((n & 63) && lane < (n & 63)) rev[(n & ~63) + lane] = outv;
    plen = n;
  }
  if (tid == 0) {
    plen_sh = plen;
    p.path_len[b] = plen;
    if (plen == 0) p.cost[b] = 0.f;
  }
  __syncthreads();
  plen = plen_sh;

  // ---------------- the path, forward from (0, 0); -1 behind it ----------------
  int2* prow = reinterpret_cast<int2*>(p.path) + (size_t)b * p.ld_path;
  for (int n = tid; n < p.ld_path; n += 256) {
    int2 v = make_int2(-1, -1);
    if (n < plen) { const unsigned u = rev[plen - 1 - n]; v.x = (int)(u >> 16); v.y = (int)(u & 0xffffu); }
    prow[n] = v;
  }
}

__global__ __launch_bounds__(256) void gt_mel_cepstrum_kernel(const float* __restrict__ mel, int ld, const int32_t* __restrict__ len,
                                                              const float* __restrict__ dct, int N, int K, int F_max,
                                                              float* __restrict__ out)
{
  __shared__ __attribute__((aligned(16))) float wsh[GT_MEL_MAX_N_MEL * 16];   // [n][16]: a frame's 16 coefficients read by broadcast
  const int b = blockIdx.y, tid = threadIdx.x;
  for (int i = tid; i < N * 16; i += 256) { const int n = i >> 4, k = i & 15; wsh[i] = k < K ? dct[k * N + n] : 0.f; }
  __syncthreads();
  int L = len[b];
  L = L < 0 ? 0 : (L < F_max ? L : F_max);
  const int f = blockIdx.x * 256 + tid;
  if (f >= F_max) return;
  float c[16];
#pragma unroll
  for (int k = 0; k < 16; ++k) c[k] = 0.f;
  if (f < L) {
    const float* m = mel + (size_t)b * N * ld + f;
    for (int n = 0; n < N; ++n) {
      const float v = m[(size_t)n * ld];
      const float4* wr = reinterpret_cast<const float4*>(wsh + n * 16);
      const float4 w0 = wr[0], w1 = wr[1], w2 = wr[2], w3 = wr[3];
      c[0]  = c[0]  + w0.x * v; c[1]  = c[1]  + w0.y * v; c[2]  = c[2]  + w0.z * v; c[3]  = c[3]  + w0.w * v;
      c[4]  = c[4]  + w1.x * v; c[5]  = c[5]  + w1.y * v; c[6]  = c[6]  + w1.z * v; c[7]  = c[7]  + w1.w * v;
      c[8]  = c[8]  + w2.x * v; c[9]  = c[9]  + w2.y * v; c[10] = c[10] + w2.z * v; c[11] = c[11] + w2.w * v;
      c[12] = c[12] + w3.x * v; c[13] = c[13] + w3.y * v; c[14] = c[14] + w3.z * v; c[15] = c[15] + w3.w * v;
    }
#pragma unroll
    for (int k = 0; k < 16; ++k) c[k] = k < K ? c[k] : 0.f;
  }
  float4* o = reinterpret_cast<float4*>(out + ((size_t)b * F_max + f) * 16);
  o[0] = make_float4(c[0], c[1], c[2], c[3]);
  o[1] = make_float4(c[4], c[5], c[6], c[7]);
  o[2] = make_float4(c[8], c[9], c[10], c[11]);
  o[3] = make_float4(c[12], c[13], c[14], c[15]);
}

__global__ __launch_bounds__(256) void gt_dtw_f0_stats_kernel(const int32_t* __restrict__ path, int ld_path,
                                                              const int32_t* __restrict__ path_len, const float* __restrict__ f0_a,
                                                              int ld_a, const float* __restrict__ f0_b, int ld_b,
                                                              int32_t* __restrict__ counts, float* __restrict__ sums)
{
  __shared__ float sf[2][256];
  __shared__ int si[3][256];
  const int b = blockIdx.x, tid = threadIdx.x;
  int P = path_len[b];
  P = P < 0 ? 0 : (P < ld_path ? P : ld_path);
  const int2* pr = reinterpret_cast<const int2*>(path) + (size_t)b * ld_path;
  const float* fa = f0_a + (size_t)b * ld_a;
  const float* fb = f0_b + (size_t)b * ld_b;
  int n_vv = 0, n_vu = 0, n_gross = 0;
  float s_hz = 0.f, s_ct = 0.f;
  for (int n = tid; n < P; n += 256) {
    const int2 ij = pr[n];
    if ((unsigned)ij.x >= (unsigned)ld_a || (unsigned)ij.y >= (unsigned)ld_b) continue;
    const float x = fa[ij.x], y = fb[ij.y];
    const bool va = x > 0.f, vb = y > 0.f;
    if (va && vb) {
      ++n_vv;
      const float dh = x - y;
      s_hz = s_hz + dh * dh;
      const double ct = 1200.0 * log2((double)x / (double)y);
      s_ct = s_ct + (float)(ct * ct);
      if (fabs((double)x - (double)y) > 0.2 * (double)y) ++n_gross;
    } else if (va != vb) {
      ++n_vu;
    }
  }
  sf[0][tid] = s_hz; sf[1][tid] = s_ct; si[0][tid] = n_vv; si[1][tid] = n_vu; si[2][tid] = n_gross;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) {
      sf[0][tid] = sf[0][tid] + sf[0][tid + o]; sf[1][tid] = sf[1][tid] + sf[1][tid + o];
      si[0][tid] += si[0][tid + o]; si[1][tid] += si[1][tid + o]; si[2][tid] += si[2][tid + o];
    }
    __syncthreads();
  }
  if (tid == 0) {
    counts[b * 3] = si[0][0]; counts[b * 3 + 1] = si[1][0]; counts[b * 3 + 2] = si[2][0];
    sums[b * 2] = sf[0][0]; sums[b * 2 + 1] = sf[1][0];
  }
}

inline bool al4(const void* p) { return !((uintptr_t)p & 3); }

}  // namespace

extern "C" size_t gt_dtw_lds_bytes(int Fa_max, int Fb_max)
{
  if (Fa_max <= 0 || Fb_max <= 0 || Fa_max > GT_DTW_MAX_F || Fb_max > GT_DTW_MAX_F) return 0;
  bool image;
  return dtw_lds(Fa_max, Fb_max, &image);
}

extern "C" size_t gt_dtw_workspace_bytes(int B, int Fa_max, int Fb_max)
{
  if (B <= 0 || Fa_max <= 0 || Fb_max <= 0 || Fa_max > GT_DTW_MAX_F || Fb_max > GT_DTW_MAX_F) return 0;
  const size_t dirs = (size_t)B * Fa_max * dtw_nq(Fb_max) * 4, rev = (size_t)B * dtw_revcap(Fa_max, Fb_max) * 4;
  return (dirs + rev + 255) & ~(size_t)255;
}

extern "C" int gt_mel_cepstrum(const float* mel, int ld, const int32_t* len, const float* dct, int B, int N, int K, int F_max,
                               float* out, void* stream)
{
  if (!mel || !len || !dct || !out) return GT_E_INVAL;
  if (B <= 0 || B > GT_MEL_MAX_B || N <= 0 || K <= 0 || F_max <= 0 || F_max > GT_MEL_MAX_FRAMES || ld < F_max) return GT_E_INVAL;
  if (N > GT_MEL_MAX_N_MEL || K > 16) return GT_E_UNSUPPORTED;
  if (!al16(out) || !al4(mel) || !al4(len) || !al4(dct)) return GT_E_ALIGN;
  hipLaunchKernelGGL(gt_mel_cepstrum_kernel, dim3((F_max + 255) / 256, B), dim3(256), 0, GT_ST(stream), mel, ld, len, dct, N, K, F_max,
                     out);
  return gt_launch_status(__func__);
}

extern "C" int gt_dtw_f32(const float* a, const float* b, const int32_t* a_len, const int32_t* b_len, int B, int Fa_max, int Fb_max,
                          float alpha, float* cost, int32_t* path_len, int32_t* path, int ld_path, void* workspace,
                          size_t workspace_bytes, int32_t* status, void* stream)
{
  if (!a || !b || !a_len || !b_len || !cost || !path_len || !path || !workspace) return GT_E_INVAL;
  if (B <= 0 || B > GT_MEL_MAX_B || Fa_max <= 0 || Fb_max <= 0) return GT_E_INVAL;
  if ((long long)ld_path < (long long)Fa_max + Fb_max - 1) return GT_E_INVAL;
  if (workspace_bytes < gt_dtw_workspace_bytes(B, Fa_max, Fb_max)) return GT_E_INVAL;
  if (Fa_max > GT_DTW_MAX_F || Fb_max > GT_DTW_MAX_F) return GT_E_UNSUPPORTED;
  if (!al16(a) || !al16(b) || !al16(path) || !al16(workspace) || !al4(a_len) || !al4(b_len) || !al4(cost) || !al4(path_len) ||
      !al4(status))
    return GT_E_ALIGN;

  bool image;
  const size_t lds = dtw_lds(Fa_max, Fb_max, &image);
  DtwArgs p;
  p.a = a; p.b = b; p.a_len = a_len; p.b_len = b_len; p.cost = cost; p.path_len = path_len; p.path = path;
  p.nq = dtw_nq(Fb_max);
  p.dirs = static_cast<uint32_t*>(workspace);
  p.rev = p.dirs + (size_t)B * Fa_max * p.nq;
  p.status = status; p.Fa_max = Fa_max; p.Fb_max = Fb_max; p.ld_path = ld_path; p.alpha = alpha;

  using KernT = void (*)(DtwArgs);
  static const KernT kerns[2] = {gt_dtw_kernel<false>, gt_dtw_kernel<true>};
  static bool attr_set[2] = {false, false};                       // benign one-time cache
  const int k = image ? 1 : 0;
  if (!attr_set[k]) {
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(kerns[k]), hipFuncAttributeMaxDynamicSharedMemorySize, (int)LDS_CAP) !=
        hipSuccess)
      return GT_E_LAUNCH;
    attr_set[k] = true;
  }
  hipLaunchKernelGGL(kerns[k], dim3(B), dim3(dtw_waves(Fa_max) * 64), lds, GT_ST(stream), p);
  if (gt_launch_status(__func__)) return GT_E_LAUNCH;
  hipLaunchKernelGGL(gt_dtw_path_kernel, dim3(B), dim3(256), 0, GT_ST(stream), p);
  return gt_launch_status(__func__);
}

extern "C" int gt_dtw_f0_stats(const int32_t* path, int ld_path, const int32_t* path_len, const float* f0_a, int ld_a,
                               const float* f0_b, int ld_b, int B, int32_t* counts, float* sums, void* stream)
{
  if (!path || !path_len || !f0_a || !f0_b || !counts || !sums) return GT_E_INVAL;
  if (B <= 0 || B > GT_MEL_MAX_B || ld_path <= 0 || ld_a <= 0 || ld_b <= 0) return GT_E_INVAL;
  if (((uintptr_t)path & 7) || !al4(path_len) || !al4(f0_a) || !al4(f0_b) || !al4(counts) || !al4(sums)) return GT_E_ALIGN;
  hipLaunchKernelGGL(gt_dtw_f0_stats_kernel, dim3(B), dim3(256), 0, GT_ST(stream), path, ld_path, path_len, f0_a, ld_a, f0_b, ld_b, counts,
                     sums);
  return gt_launch_status(__func__);
}
