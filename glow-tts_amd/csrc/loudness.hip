// ITU-R BS.1770-4 integrated loudness and normalisation to a target behind the vocoders: the K-weighting cascade of
// two biquads (a serial recurrence along time), 400 ms blocks at 75 % overlap, the absolute and the relative gate, the gain and the
// scale pass, every utterance of a ragged batch on its own, the recurrence, every sum and the gating in double.
//
// The cascade is a linear system with a 4-number state (two transposed direct form II biquads: s1, s2 of the shelf, s1, s2 of the
// high-pass).  Every utterance is cut into chunks of Lc samples, Lc the largest divisor of Ns = fs / 10 not above 50, so a chunk lies in
// ONE 100 ms segment.  One thread runs one chunk; a workgroup of 256 threads stages its 256 Lc consecutive samples through LDS
// (coalesced loads; chunk c at pitch Lc | 1 words, so the 64 lanes of a wave read 64 banks).
//
//   gt_loud_chunk<false>   pass 1: every chunk from ZERO state -> its end state e_k                              ws.state[b][k]
//   gt_loud_scan_kernel    pass 2: s_k = M s_{k-1} + e_k per utterance, M the transition over Lc samples; one workgroup per
//                          utterance in three levels: thread t scans its run of 16 chunks from zero; the 256 run ends are scanned
//                          with M16 = M^16 the same way one level up (16 threads, 16 run ends each, the 16 group ends by thread 0
//                          with M256 = M^256); thread t runs its 16 chunks again from its run's true start.  A serial depth of
//                          5 * 16 steps for 4096 chunks.  state[b][k] becomes the START state of chunk k (s_{k-1}), in place.
//   gt_loud_chunk<true>    pass 3: every chunk from its true start state -> sum z^2 (double, in sample order) and max |x|
//   gt_loud_gate_kernel    one workgroup per utterance: segment sums (a segment's chunks in order), blocks, both gates, L, peak, g
//   gt_loud_apply_kernel   y = fp32(g) x over the utterance's samples, zeros behind them up to the row's capacity
//
// No atomics; the order of every sum depends on the sample's, chunk's or block's index within its utterance alone, so a batch row is
// bit-identical to the utterance alone.  Nothing at or behind an utterance's last sample is read.  Coefficients, both transition
// matrices, the target and the peak ceiling are doubles read from device memory (`params`, built by audio.py in float64).
#include "common.h"
#include "internal.h"
#include "../../include/glowtts_hip.h"

namespace {

constexpr int TPB = 256;                       // threads = chunks per workgroup
constexpr int LC_MAX = 50, LC_MIN = 16;        // chunk lengths the kernels take
constexpr int PITCH_MAX = LC_MAX | 1;
constexpr int RUN = 16;                        // chunks per thread in the scan's first level, runs per thread in its second
constexpr int GROUPS = TPB / RUN;              // groups of RUN runs in a round of TPB runs
constexpr int P_SHELF = 0, P_HP = 5, P_M = 10, P_M16 = 26, P_TARGET = 42, P_CEIL = 43, P_M256 = 44;   // doubles of `params` (GT_LOUD_PARAMS = 64)
static_assert(GROUPS == RUN && P_M256 + 16 <= GT_LOUD_PARAMS, "the scan's three levels");

struct Geo { int Ns, Lc; };

// Ns = fs / 10 and the chunk length: the largest divisor of Ns in [LC_MIN, LC_MAX]; Lc == 0: a rate the kernels do not take
static Geo geometry(int fs)
{
  Geo g = {0, 0};
  if (fs < 8000 || fs > 192000 || fs % 10) return g;
  g.Ns = fs / 10;
  for (int d = LC_MAX; d >= LC_MIN; --d)
    if (g.Ns % d == 0) { g.Lc = d; break; }
  return g;
}

static inline int64_t chunks_cap(int L_cap, int Lc) { return ((int64_t)L_cap + Lc - 1) / Lc; }
static inline int64_t segs_cap(int L_cap, int Ns) { return (int64_t)L_cap / Ns + 1; }

// the workspace: state double [B][Kc][4] | sums double [B][Kc] | segs double [B][Sc] | peaks float [B][Kc]
struct Ws { double* state; double* sums; double* segs; float* peaks; int Kc, Sc; };
static size_t ws_layout(void* base, int B, int L_cap, Geo g, Ws* w)
{
  const int64_t Kc = chunks_cap(L_cap, g.Lc), Sc = segs_cap(L_cap, g.Ns);
  char* p = static_cast<char*>(base);
  size_t off = 0;
  w->state = reinterpret_cast<double*>(p + off); off += (size_t)B * Kc * 4 * sizeof(double);
  w->sums = reinterpret_cast<double*>(p + off);  off += (size_t)B * Kc * sizeof(double);
  w->segs = reinterpret_cast<double*>(p + off);  off += (size_t)B * Sc * sizeof(double);
  w->peaks = reinterpret_cast<float*>(p + off);  off += (size_t)B * Kc * sizeof(float);
  w->Kc = (int)Kc; w->Sc = (int)Sc;
  return (off + 15) & ~(size_t)15;
}

// samples of utterance b: hop max(n_frames[b] - lost, 0), at most the row's capacity
__device__ __forceinline__ int utt_samples(const int32_t* n_frames, int b, int hop, int lost, int L_cap)
{
  const long long n = (long long)hop * (long long)max(n_frames[b] - lost, 0);
  return (int)min(n, (long long)L_cap);
}

struct Coef { double b0, b1, b2, a1, a2, c0, c1, c2, d1, d2; };
__device__ __forceinline__ Coef load_coef(const double* __restrict__ p)
{
  return {p[P_SHELF], p[P_SHELF + 1], p[P_SHELF + 2], p[P_SHELF + 3], p[P_SHELF + 4], p[P_HP], p[P_HP + 1], p[P_HP + 2], p[P_HP + 3], p[P_HP + 4]};
}

// one sample through the cascade (transposed direct form II, twice): s = (s1, s2 of the shelf, s1, s2 of the high-pass) -> z
__device__ __forceinline__ double kw_step(const Coef& c, double x, double (&s)[4])
{
  const double y = fma(c.b0, x, s[0]);
  s[0] = fma(c.b1, x, fma(-c.a1, y, s[1]));
  s[1] = fma(c.b2, x, -c.a2 * y);
  const double z = fma(c.c0, y, s[2]);
  s[2] = fma(c.c1, y, fma(-c.d1, z, s[3]));
  s[3] = fma(c.c2, y, -c.d2 * z);
  return z;
}

// out = m s + e, m row-major 4 x 4, each row one chain over j = 0 .. 3 on top of e
__device__ __forceinline__ void mat_step(const double* __restrict__ m, const double (&s)[4], const double (&e)[4], double (&out)[4])
{
#pragma unroll
  for (int i = 0; i < 4; ++i) out[i] = fma(m[4 * i + 3], s[3], fma(m[4 * i + 2], s[2], fma(m[4 * i + 1], s[1], fma(m[4 * i], s[0], e[i]))));
}

// the workgroup's 256 Lc samples [base, base + count) of the row into LDS, chunk c at c * pitch; nothing at or behind `count` is read
__device__ __forceinline__ void stage(float* lds, const void* __restrict__ row, int is_i16, int base, int count, int Lc, int pitch, int tid)
{
  const float* xf = static_cast<const float*>(row) + base;
  const int16_t* xi = static_cast<const int16_t*>(row) + base;
  for (int i = tid; i < count; i += TPB) {
    const int c = i / Lc;
    lds[c * pitch + (i - c * Lc)] = is_i16 ? (float)xi[i] * (1.0f / 32768.0f) : xf[i];
  }
}

template <bool SUMS>
__global__ __launch_bounds__(TPB) void gt_loud_chunk_kernel(const void* __restrict__ wav, long long ld_bytes, int is_i16,
                                                            const int32_t* __restrict__ n_frames, int hop, int lost, int L_cap, int Lc,
                                                            const double* __restrict__ params, double* __restrict__ state,
                                                            double* __restrict__ sums, float* __restrict__ peaks, int Kc)
{
  __shared__ float lds[TPB * PITCH_MAX];
  const int b = blockIdx.y, tid = threadIdx.x;
  const int N = utt_samples(n_frames, b, hop, lost, L_cap);
  const long long base = (long long)blockIdx.x * TPB * Lc;
  if (base >= N) return;                                   // the whole workgroup lies behind the utterance: no sample is read
  const int count = (int)min((long long)TPB * Lc, (long long)N - base), pitch = Lc | 1;
  stage(lds, static_cast<const char*>(wav) + (long long)b * ld_bytes, is_i16, (int)base, count, Lc, pitch, tid);
  __syncthreads();
  const int len = min(Lc, count - tid * Lc);
  if (len <= 0) return;
  const int k = blockIdx.x * TPB + tid;                    // the chunk within its utterance
  const Coef c = load_coef(params);
  double* st = state + ((size_t)b * Kc + k) * 4;
  double s[4] = {0.0, 0.0, 0.0, 0.0};
  const float* x = lds + tid * pitch;
  if (!SUMS) {
    for (int i = 0; i < len; ++i) kw_step(c, (double)x[i], s);
    *reinterpret_cast<double2*>(st) = make_double2(s[0], s[1]);
    *reinterpret_cast<double2*>(st + 2) = make_double2(s[2], s[3]);
  } else {
    if (k) {
      const double2 lo = *reinterpret_cast<const double2*>(st), hi = *reinterpret_cast<const double2*>(st + 2);
      s[0] = lo.x; s[1] = lo.y; s[2] = hi.x; s[3] = hi.y;
    }
    double acc = 0.0;
    float pk = 0.f;
    for (int i = 0; i < len; ++i) {
      const float xv = x[i];
      const double z = kw_step(c, (double)xv, s);
      acc = fma(z, z, acc);
      pk = fmaxf(pk, fabsf(xv));
    }
    sums[(size_t)b * Kc + k] = acc;
    peaks[(size_t)b * Kc + k] = pk;
  }
}

__global__ __launch_bounds__(TPB) void gt_loud_scan_kernel(const int32_t* __restrict__ n_frames, int hop, int lost, int L_cap, int Lc,
                                                           const double* __restrict__ params, double* __restrict__ state, int Kc)
{
  __shared__ double ends[TPB][4];                          // the runs' end states from zero, then their true start states
  __shared__ double grp[GROUPS][4];                        // the same one level up: 16 groups of 16 runs
  __shared__ double carry[4];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int N = utt_samples(n_frames, b, hop, lost, L_cap);
  const int K = (N + Lc - 1) / Lc;                         // the utterance's chunks
  const double* M = params + P_M;
  const double* M16 = params + P_M16;
  const double* M256 = params + P_M256;
  double* st = state + (size_t)b * Kc * 4;
  if (tid < 4) carry[tid] = 0.0;
  for (int base = 0; base < K; base += TPB * RUN) {        // uniform across the workgroup
    const int k0 = base + tid * RUN, n = min(RUN, K - k0);  // this thread's run: chunks k0 .. k0 + n - 1 (n <= 0: none)
    double2 e[RUN][2];                                     // the run's end states, all loads in flight at once; kept for the second pass
#pragma unroll
    for (int i = 0; i < RUN; ++i)
      if (i < n) {
        e[i][0] = *reinterpret_cast<const double2*>(st + (size_t)(k0 + i) * 4);
        e[i][1] = *reinterpret_cast<const double2*>(st + (size_t)(k0 + i) * 4 + 2);
      }
    double r[4] = {0.0, 0.0, 0.0, 0.0}, t[4];
#pragma unroll
    for (int i = 0; i < RUN; ++i)                          // the run from zero
      if (i < n) {
        const double ei[4] = {e[i][0].x, e[i][0].y, e[i][1].x, e[i][1].y};
        mat_step(M, r, ei, t);
#pragma unroll
        for (int c = 0; c < 4; ++c) r[c] = t[c];
      }
#pragma unroll
    for (int c = 0; c < 4; ++c) ends[tid][c] = r[c];
    __syncthreads();
    // the run ends in order, S_t = M16 S_{t-1} + r_t, by the same three steps one level up: 16 threads scan 16 run ends each from
    // zero, thread 0 scans the 16 group ends with M256 = M^256, the 16 threads scan again from their group's true start.  A round
    // that is not full (runs < 256) is the utterance's last: its carry is not used.
    const int runs = min(TPB, (K - base + RUN - 1) / RUN);
    if (tid < GROUPS) {
      double g[4] = {0.0, 0.0, 0.0, 0.0};
      for (int q = tid * RUN; q < min(tid * RUN + RUN, runs); ++q) {
        const double eq[4] = {ends[q][0], ends[q][1], ends[q][2], ends[q][3]};
        mat_step(M16, g, eq, t);
#pragma unroll
        for (int c = 0; c < 4; ++c) g[c] = t[c];
      }
#pragma unroll
      for (int c = 0; c < 4; ++c) grp[tid][c] = g[c];
    }
    __syncthreads();
    if (tid == 0) {
      double S[4] = {carry[0], carry[1], carry[2], carry[3]};
      for (int q = 0; q * RUN < runs; ++q) {
        double eq[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) { eq[c] = grp[q][c]; grp[q][c] = S[c]; }
        mat_step(M256, S, eq, t);
#pragma unroll
        for (int c = 0; c < 4; ++c) S[c] = t[c];
      }
#pragma unroll
      for (int c = 0; c < 4; ++c) carry[c] = S[c];
    }
    __syncthreads();
    if (tid < GROUPS) {
      double g[4] = {grp[tid][0], grp[tid][1], grp[tid][2], grp[tid][3]};
      for (int q = tid * RUN; q < min(tid * RUN + RUN, runs); ++q) {
        double eq[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) { eq[c] = ends[q][c]; ends[q][c] = g[c]; }
        mat_step(M16, g, eq, t);
#pragma unroll
        for (int c = 0; c < 4; ++c) g[c] = t[c];
      }
    }
    __syncthreads();
#pragma unroll
    for (int c = 0; c < 4; ++c) r[c] = ends[tid][c];
#pragma unroll
    for (int i = 0; i < RUN; ++i)                          // the run again from its true start: state[k] = s_{k-1}
      if (i < n) {
        *reinterpret_cast<double2*>(st + (size_t)(k0 + i) * 4) = make_double2(r[0], r[1]);
        *reinterpret_cast<double2*>(st + (size_t)(k0 + i) * 4 + 2) = make_double2(r[2], r[3]);
        const double ei[4] = {e[i][0].x, e[i][0].y, e[i][1].x, e[i][1].y};
        mat_step(M, r, ei, t);
#pragma unroll
        for (int c = 0; c < 4; ++c) r[c] = t[c];
      }
    __syncthreads();
  }
}

// fixed-order sum of one double per thread: a tree over thread indices
__device__ __forceinline__ double block_sum(double v, double* red, int tid)
{
  __syncthreads();
  red[tid] = v;
  __syncthreads();
  for (int w = TPB / 2; w > 0; w >>= 1) {
    if (tid < w) red[tid] += red[tid + w];
    __syncthreads();
  }
  return red[0];
}

// p[0] + p[1] + ... + p[n - 1] added in this order, eight loads in flight at a time
__device__ __forceinline__ double ordered_sum(const double* __restrict__ p, int n)
{
  double a = 0.0;
  int i = 0;
  for (; i + 8 <= n; i += 8) {
    double v[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) v[q] = p[i + q];
#pragma unroll
    for (int q = 0; q < 8; ++q) a += v[q];
  }
  for (; i < n; ++i) a += p[i];
  return a;
}

__device__ __forceinline__ double lkfs(double z) { return -0.691 + 10.0 * log10(z); }

__global__ __launch_bounds__(TPB) void gt_loud_gate_kernel(const int32_t* __restrict__ n_frames, int hop, int lost, int L_cap, int Lc, int Ns,
                                                           const double* __restrict__ params, const double* __restrict__ sums,
                                                           const float* __restrict__ peaks, double* __restrict__ segs, int Kc, int Sc,
                                                           float* __restrict__ stats)
{
  __shared__ double red[TPB];
  __shared__ float redf[TPB];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int N = utt_samples(n_frames, b, hop, lost, L_cap);
  const int K = (N + Lc - 1) / Lc, cps = Ns / Lc, Nb = 4 * Ns;
  const double* cs = sums + (size_t)b * Kc;
  double* sg = segs + (size_t)b * Sc;
  // the sample peak: max is exact in any order
  float pk = 0.f;
  for (int k = tid; k < K; k += TPB) pk = fmaxf(pk, peaks[(size_t)b * Kc + k]);
  redf[tid] = pk;
  __syncthreads();
  for (int w = TPB / 2; w > 0; w >>= 1) {
    if (tid < w) redf[tid] = fmaxf(redf[tid], redf[tid + w]);
    __syncthreads();
  }
  pk = redf[0];

  int J;
  const int S = N / Ns;                                    // whole segments
  if (N >= Nb) {
    J = S - 3;
    for (int s = tid; s < S; s += TPB) sg[s] = ordered_sum(cs + (size_t)s * cps, cps);   // a segment's chunks in order
  } else {                                                 // below 400 ms: one block over the whole utterance
    J = N > 0 ? 1 : 0;
    if (tid == 0) sg[0] = ordered_sum(cs, K);
  }
  __syncthreads();
  const double inv = N >= Nb ? 1.0 / (double)Nb : (N > 0 ? 1.0 / (double)N : 0.0);
  auto block = [&](int j) { return N >= Nb ? (((sg[j] + sg[j + 1]) + sg[j + 2]) + sg[j + 3]) * inv : sg[0] * inv; };

  double za = 0.0, na = 0.0;                               // the absolute gate
  for (int j = tid; j < J; j += TPB) {
    const double z = block(j);
    if (lkfs(z) > -70.0) { za += z; na += 1.0; }
  }
  za = block_sum(za, red, tid);
  na = block_sum(na, red, tid);
  const double gamma = na > 0.0 ? lkfs(za / na) - 10.0 : 0.0;
  double zr = 0.0, nr = 0.0;                               // the relative gate, within the absolute one
  for (int j = tid; j < J; j += TPB) {
    const double z = block(j);
    const double l = lkfs(z);
    if (l > -70.0 && l > gamma) { zr += z; nr += 1.0; }
  }
  zr = block_sum(zr, red, tid);
  nr = block_sum(nr, red, tid);
  if (tid == 0) {
    // nr > 0 wherever na > 0: the loudest block of A lies above A's mean - 10
    const double L = na > 0.0 && nr > 0.0 ? lkfs(zr / nr) : -HUGE_VAL;
    double g = 1.0;
    if (L > -HUGE_VAL) {
      g = pow(10.0, (params[P_TARGET] - L) / 20.0);
      const double ceil_lin = params[P_CEIL];
      if (pk > 0.f && g * (double)pk > ceil_lin) g = ceil_lin / (double)pk;
    }
    float* o = stats + (size_t)b * GT_LOUD_STATS;
    o[0] = (float)L; o[1] = pk; o[2] = (float)g; o[3] = (float)J; o[4] = (float)na; o[5] = (float)nr;
    o[6] = na > 0.0 ? (float)gamma : -HUGE_VALF; o[7] = (float)N;
  }
}

__global__ __launch_bounds__(TPB) void gt_loud_apply_kernel(const float* wav, int ld, float* out, int ld_out,      // out may be wav
                                                            const int32_t* __restrict__ n_frames, int hop, int lost, int L_cap,
                                                            const float* __restrict__ stats)
{
  const int b = blockIdx.y;
  const int N = utt_samples(n_frames, b, hop, lost, L_cap);
  const float g = stats[(size_t)b * GT_LOUD_STATS + 2];
  const float* x = wav + (size_t)b * ld;
  float* y = out + (size_t)b * ld_out;
  const int i0 = blockIdx.x * (TPB * 4) + threadIdx.x;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int i = i0 + j * TPB;
    if (i < L_cap) y[i] = i < N ? g * x[i] : 0.f;
  }
}

// the checks both entries share; 0 or a status.  `apply`: the scale pass (fp32 rows only, no workspace)
static int check(const gt_loudness_args* a, bool apply, Geo* geo)
{
  if (!a) return GT_E_INVAL;
  if (!a->wav || !a->n_frames || !a->stats || (!apply && (!a->params || !a->ws))) return GT_E_INVAL;
  if (a->B <= 0 || a->B > GT_MEL_MAX_B || a->L_cap <= 0 || a->ld < a->L_cap || a->hop <= 0 || a->lost < 0) return GT_E_INVAL;
  if (apply && a->out && a->ld_out < a->L_cap) return GT_E_INVAL;
  *geo = geometry(a->fs);
  if (!apply && geo->Lc && a->ws_bytes < (int64_t)gt_loudness_ws_bytes(a->B, a->L_cap, a->fs)) return GT_E_INVAL;
  if (!geo->Lc || (apply && a->is_i16)) return GT_E_UNSUPPORTED;
  if (!apply && gt_loudness_ws_bytes(a->B, a->L_cap, a->fs) == 0) return GT_E_UNSUPPORTED;
  const uintptr_t el = a->is_i16 ? 1 : 3;
  if (((uintptr_t)a->wav & el) || ((uintptr_t)a->n_frames & 3) || ((uintptr_t)a->stats & 3) || ((uintptr_t)a->out & 3)) return GT_E_ALIGN;
  if (!apply && (((uintptr_t)a->params & 7) || !al16(a->ws))) return GT_E_ALIGN;
  return GT_OK;
}

}  // namespace

extern "C" int gt_loudness_args_size(void) { return (int)sizeof(gt_loudness_args); }

extern "C" int gt_loudness_chunk(int fs) { return geometry(fs).Lc; }

extern "C" size_t gt_loudness_ws_bytes(int B, int L_cap, int fs)
{
  const Geo g = geometry(fs);
  if (!g.Lc || B <= 0 || B > GT_MEL_MAX_B || L_cap <= 0) return 0;
  const int64_t Kc = chunks_cap(L_cap, g.Lc);
  if ((int64_t)B * Kc * 4 >= ((int64_t)1 << 31)) return 0;   // every element index the kernels form stays below 2^31
  Ws w;
  return ws_layout(nullptr, B, L_cap, g, &w);
}

extern "C" int gt_loudness_measure(const gt_loudness_args* a, void* stream)
{
  Geo g;
  if (const int rc = check(a, false, &g)) return rc;
  Ws w;
  ws_layout(a->ws, a->B, a->L_cap, g, &w);
  const long long ld_bytes = (long long)a->ld * (a->is_i16 ? 2 : 4);
  const dim3 grid((unsigned)((w.Kc + TPB - 1) / TPB), (unsigned)a->B);
  hipLaunchKernelGGL(gt_loud_chunk_kernel<false>, grid, dim3(TPB), 0, GT_ST(stream), a->wav, ld_bytes, a->is_i16, a->n_frames, a->hop,
                     a->lost, a->L_cap, g.Lc, a->params, w.state, w.sums, w.peaks, w.Kc);
  hipLaunchKernelGGL(gt_loud_scan_kernel, dim3(a->B), dim3(TPB), 0, GT_ST(stream), a->n_frames, a->hop, a->lost, a->L_cap, g.Lc, a->params,
                     w.state, w.Kc);
  hipLaunchKernelGGL(gt_loud_chunk_kernel<true>, grid, dim3(TPB), 0, GT_ST(stream), a->wav, ld_bytes, a->is_i16, a->n_frames, a->hop,
                     a->lost, a->L_cap, g.Lc, a->params, w.state, w.sums, w.peaks, w.Kc);
  hipLaunchKernelGGL(gt_loud_gate_kernel, dim3(a->B), dim3(TPB), 0, GT_ST(stream), a->n_frames, a->hop, a->lost, a->L_cap, g.Lc, g.Ns,
                     a->params, w.sums, w.peaks, w.segs, w.Kc, w.Sc, a->stats);
  return gt_launch_status(__func__);
}

extern "C" int gt_loudness_apply(const gt_loudness_args* a, void* stream)
{
  Geo g;
  if (const int rc = check(a, true, &g)) return rc;
  float* wav = static_cast<float*>(a->wav);
  const dim3 grid((unsigned)((a->L_cap + TPB * 4 - 1) / (TPB * 4)), (unsigned)a->B);
  hipLaunchKernelGGL(gt_loud_apply_kernel, grid, dim3(TPB), 0, GT_ST(stream), wav, a->ld, a->out ? a->out : wav, a->out ? a->ld_out : a->ld,
                     a->n_frames, a->hop, a->lost, a->L_cap, a->stats);
  return gt_launch_status(__func__);
}
