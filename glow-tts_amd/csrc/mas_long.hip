// Monotonic Alignment Search for lattices gt_mas_f32 (mas.hip) refuses — more than 512 tokens, or direction bits past
// its 160 KiB of LDS.  Same contract, same outputs, bit-exact with reference monotonic_align/core.pyx:9-45.
//
// What changes against mas.hip (read that file's header first; the column, the skew, the boundary ring, the logp ring and
// the backtrack are its own, shared through mas_common.h):
//
//   * Rows in bands.  Still one workgroup per utterance, W <= 8 waves of 64 rows; the workgroup walks the rows in bands of
//     64 W.  In band k wave w owns the GLOBAL row block u = W k + w (rows 64u .. 64u+63): the two chunks that hold x == y
//     cells are 2u and 2u+1, the first chunk it computes is 2u, and only u == 0 has no row above it.  A band runs the
//     skewed step loop of mas.hip from chunk 2 W k on and drains before the next one starts.
//   * The band boundary.  The Q values of a band's last row (one float per column) are the x-1 operand of the next band's
//     first wave.  The last wave copies each finished boundary slot (32 floats) from LDS to a per-utterance buffer in the
//     workspace, shifted by one column (q[y + 1] = Q[row, y]) so that the reader's chunk c is the aligned run q[32c ..
//     32c+31] and needs no carry.  Wave 0 of the next band loads that run three chunks ahead into a register and drops
//     it into a boundary area of its own, two chunks ahead, so it reads its operand from LDS exactly like waves 1..W-1 do.
//     Two buffers, by band parity: band k writes one while it reads the other, and bands are separated by a barrier.
//   * Direction words in HBM.  dirs[b][chunk][row], rows padded to a multiple of 64: the wave's 64 words of one chunk are
//     one coalesced 256-byte store, and in the backtrack lane l's word of row idx - l is one coalesced load.  The store
//     is issued BEHIND the counted vmcnt wait of the logp ring, so the ring's wait only ever gets stricter by it.
//   * Nothing in LDS grows with T_x * T_y: tile ring + W + 1 boundary areas + (T_x + 2) row starts.
#include <hip/hip_runtime.h>
#include "common.h"
#pragma clang fp contract(off)   // bit-exact IEEE adds/compares only
#include <stdint.h>
#include "../../include/glowtts_hip.h"
#include "mas_common.h"
#include "internal.h"

namespace {

constexpr int    MAXW    = 8;                 // waves per workgroup: 512-row bands
constexpr size_t LDS_CAP = 160 * 1024;
constexpr int    TX_MAX  = GT_MAS_LONG_MAX_TX;
constexpr int    TY_MAX  = GT_MAS_LONG_MAX_TY;

struct MasLongArgs {
  const float* logp; const float* mask;
  const int32_t* t_x; const int32_t* t_y;
  float* durations; int32_t* frame2token;
  int32_t*  starts;                        // workspace head: [B, T_x + 1]
  float*    bandq;                         // [B][2][gbf] last-row Q of a band, shifted by one column
  unsigned* dirs;                          // [B][nchT][R] direction words, chunk-major
  int T_x, T_y; int64_t stride_b, stride_x;
  int32_t* status;
  int gbf;                                 // floats of one band buffer
  int R;                                   // rows, padded to a multiple of 64
  int nchT;                                // chunks of the lattice
  int depth;                               // ring depth D (2..MAXD)
};

__host__ __device__ inline int ml_nch(int T_y) { return (T_y + CH - 1) / CH; }
__host__ __device__ inline int ml_rows(int T_x) { return (T_x + 63) / 64 * 64; }
__host__ __device__ inline int ml_gbf(int T_y) { return ml_nch(T_y) * CH + 64; }

inline size_t ml_align(size_t n) { return (n + 255) & ~(size_t)255; }
inline size_t ml_starts_bytes(int B, int T_x) { return ml_align((size_t)B * (size_t)(T_x + 1) * 4); }
inline size_t ml_bandq_bytes(int B, int T_y) { return ml_align((size_t)B * 2 * (size_t)ml_gbf(T_y) * 4); }
inline size_t ml_dirs_bytes(int B, int T_x, int T_y) { return ml_align((size_t)B * (size_t)ml_nch(T_y) * (size_t)ml_rows(T_x) * 4); }
inline size_t ml_lds_fixed(int W, int T_x) { return (size_t)(W + 1) * BND_F * 4 + (size_t)(T_x + 2) * 4 + 8; }

template <bool DMA, bool MASK>
__global__ __launch_bounds__(512) void gt_mas_long_dp_kernel(MasLongArgs a)
{
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int b    = blockIdx.x;
  const int tid  = threadIdx.x;
  const int lane = tid & 63;
  const int w    = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int W    = blockDim.x >> 6;
  const int NT   = blockDim.x;
  const int T_x = a.T_x, T_y = a.T_y, R = a.R;
  const int D   = DMA ? a.depth : 1;

  int t_x = a.t_x[b], t_y = a.t_y[b];
  {
    int st = 0;
    if (t_x < 0 || t_y < 0 || t_x > T_x || t_y > T_y) st |= GT_MAS_ST_BAD_LEN;
    else if (t_x > t_y) st |= GT_MAS_ST_TX_GT_TY;
    if (st) { if (tid == 0 && a.status) atomicOr(a.status, st); t_x = 0; t_y = 0; }
    if (t_x == 0 || t_y == 0) { t_x = 0; t_y = 0; }            // empty utterance -> all-zero path
  }

  // LDS carve: [W][D] tiles | [W + 1] boundary areas (area W: the band operand of wave 0) | starts [T_x + 2]
  float* ring     = reinterpret_cast<float*>(smem) + (size_t)w * D * TILE_F;
  float* bndall   = reinterpret_cast<float*>(smem) + (size_t)W * D * TILE_F;
  float* prevarea = bndall + W * BND_F;
  int*   starts   = reinterpret_cast<int*>(bndall + (W + 1) * BND_F);

  const int nch    = (t_y + CH - 1) / CH;
  const int nblk   = (t_x + 63) >> 6;                          // row blocks of this utterance
  const int nbands = (nblk + W - 1) / W;

  const float* lp = a.logp + (int64_t)b * a.stride_b;
  const float* mp = MASK ? a.mask + (int64_t)b * a.stride_b : nullptr;
  float*    gq    = a.bandq + (size_t)b * 2 * a.gbf;
  unsigned* dirsg = a.dirs + (size_t)b * a.nchT * R;

  int u = w;                                                    // global row block of this wave in the current band
  // ---- tile fill: chunk c of row block u -> ring slot c % D (addresses clamped onto valid cells, see mas.hip)
  auto fill_dma = [&](int c) {                                  // 8 x global_load_lds_dwordx4
    float* slot = ring + (c % D) * TILE_F;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int rr = i * 8 + (lane >> 3);
      const int q  = (lane & 7) ^ ((rr >> 1) & 7);              // swizzle on the SOURCE side
      int row = u * 64 + rr;  row = row < T_x ? row : T_x - 1;
      int col = c * CH + q * 4; col = col < T_y ? col : T_y - 4;
      const float* g = lp + (int64_t)row * a.stride_x + col;
      const unsigned dst = __builtin_amdgcn_readfirstlane(lds_off(slot + i * 256));
      unsigned keep;
      asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\t"
                   "global_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                   : "=&s"(keep) : "v"(g), "s"(dst) : "memory");
    }
  };
  auto fill_regs = [&](int c) {                                 // generic: any alignment, optional mask
    float* slot = ring + (c % D) * TILE_F;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int rr = i * 8 + (lane >> 3);
      int row = u * 64 + rr;  row = row < T_x ? row : T_x - 1;
      const int col = c * CH + (lane & 7) * 4;
      const int c0 = col     < T_y ? col     : T_y - 1;
      const int c1 = col + 1 < T_y ? col + 1 : T_y - 1;
      const int c2 = col + 2 < T_y ? col + 2 : T_y - 1;
      const int c3 = col + 3 < T_y ? col + 3 : T_y - 1;
      const float* p = lp + (int64_t)row * a.stride_x;
      float4 v = make_float4(p[c0], p[c1], p[c2], p[c3]);
      if (MASK) {                                               // value*mask, __init__.py:11
        const float* pm = mp + (int64_t)row * a.stride_x;
        v.x *= pm[c0]; v.y *= pm[c1]; v.z *= pm[c2]; v.w *= pm[c3];
      }
      *reinterpret_cast<float4*>(slot + rr * CH + (((lane & 7) ^ ((rr >> 1) & 7)) << 2)) = v;
    }
  };

  int issued = 0;                                               // next chunk this wave fetches
  auto issue_upto = [&](int target) {
    if (DMA) { while (issued <= target && issued < nch) { fill_dma(issued); ++issued; } }
  };
  // wait until at most `n` DMA groups (8 loads each) are still in flight.  The wave's other vector memory operations (direction
  // words, band boundary) are issued right behind this wait: they are older than every group it lets pass, or they count as
  // part of the newest 8n and make it wait for more than it has to, never for less.
  auto wait_groups = [&](int n) {
    if (!DMA) return;
    if      (n >= 3) asm volatile("s_waitcnt vmcnt(24)" ::: "memory");
    else if (n == 2) asm volatile("s_waitcnt vmcnt(16)" ::: "memory");
    else if (n == 1) asm volatile("s_waitcnt vmcnt(8)"  ::: "memory");
    else             asm volatile("s_waitcnt vmcnt(0)"  ::: "memory");
  };
  auto step_barrier = [&]() {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");          // asm ds_writes are invisible to hipcc
    __builtin_amdgcn_s_barrier();
  };

#ifdef MAS_STAMPS
  unsigned long long st0 = __builtin_readcyclecounter();
#endif
  // ---------------- forward DP, band by band: direction bits into the workspace ----------------
  for (int k = 0; k < nbands; ++k) {
    u = k * W + w;
    const bool wave_active = u < nblk;
    const int  Wact = (nblk - k * W) < W ? (nblk - k * W) : W;
    const int  x    = u * 64 + lane;
    const int  c0   = 2 * k * W;                                // first chunk of the band (of its wave 0)
    const bool top       = (u == 0);                            // no row above: core.pyx:23-27
    const bool from_band = (w == 0 && k > 0);                   // x-1 operand = last row of band k-1
    const bool to_band   = (w == W - 1 && k + 1 < nbands);      // last row of this band feeds band k+1
    const float* gprev = gq + ((k + 1) & 1) * a.gbf;            // band k-1 wrote buffer (k-1) & 1
    float*       gcur  = gq + (k & 1) * a.gbf;
    float nb = 0.0f;                                            // wave 0: boundary run of chunk c+2, in flight / in hand

    issued = 2 * u;
    if (wave_active) {
      if (DMA) { issue_upto(2 * u + D - 2); wait_groups(issued - (2 * u + 1)); }
      else if (2 * u < nch) fill_regs(2 * u);
      if (from_band && lane < CH) {                             // chunks c0, c0+1 into both slots, c0+2 into the register
        prevarea[(c0 & 1) * BND_SLOT + lane] = __hip_atomic_load(gprev + CH * c0 + lane, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (c0 + 1 < nch)
          prevarea[((c0 + 1) & 1) * BND_SLOT + lane] = __hip_atomic_load(gprev + CH * (c0 + 1) + lane, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (c0 + 2 < nch) nb = __hip_atomic_load(gprev + CH * (c0 + 2) + lane, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
    }
    step_barrier();

    float Q = 0.0f, carry = NEG, Pneg = NEG;
    const float* bin_base  = (w > 0) ? bndall + (w - 1) * BND_F : prevarea;   // producer = wave w-1, or the band below
    float*       bout_base = bndall + w * BND_F;
    const int nsteps = (nch - c0) + Wact - 1;
    for (int s = 0; s < nsteps; ++s) {
      const int c = c0 + s - w;
      if (wave_active && c >= 2 * u && c < nch) {
        issue_upto(c + D - 1);
        const float* slot = ring + (c % D) * TILE_F;
        const float* bin  = bin_base + (c & 1) * BND_SLOT;
        float* bout = (lane == 63) ? (bout_base + (c & 1) * BND_SLOT) : (bout_base + 2 * BND_SLOT + lane);
        const int sw = (lane >> 1) & 7;
        float4 V[8], B[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) V[q] = *reinterpret_cast<const float4*>(slot + lane * CH + ((q ^ sw) << 2));
        if (!top) {
#pragma unroll
          for (int q = 0; q < 8; ++q) B[q] = *reinterpret_cast<const float4*>(bin + q * 4);   // broadcast reads
          if (w > 0) {
            B[0].x = carry;
            carry = bin[CH];                                    // Q[64u-1, last column of this chunk]
          }                                                     // (the band buffer is shifted: its entry 0 is that value already)
        }
        unsigned dir = 0;
        if ((c >> 1) == u) {                                    // chunk holds x == y cells
          if (top) mas_chunk_diag<true >(V, B, bout, x, c, Q, dir);
          else     mas_chunk_diag<false>(V, B, bout, x, c, Q, dir);
        } else {
          const unsigned ba = lds_off(bout);
          if (top) {
            mas_cols4_w0< 0>(Q, dir, Pneg, V[0], ba); mas_cols4_w0< 4>(Q, dir, Pneg, V[1], ba);
            mas_cols4_w0< 8>(Q, dir, Pneg, V[2], ba); mas_cols4_w0<12>(Q, dir, Pneg, V[3], ba);
            mas_cols4_w0<16>(Q, dir, Pneg, V[4], ba); mas_cols4_w0<20>(Q, dir, Pneg, V[5], ba);
            mas_cols4_w0<24>(Q, dir, Pneg, V[6], ba); mas_cols4_w0<28>(Q, dir, Pneg, V[7], ba);
          } else {
            mas_cols4< 0>(Q, dir, B[0], V[0], ba); mas_cols4< 4>(Q, dir, B[1], V[1], ba);
            mas_cols4< 8>(Q, dir, B[2], V[2], ba); mas_cols4<12>(Q, dir, B[3], V[3], ba);
            mas_cols4<16>(Q, dir, B[4], V[4], ba); mas_cols4<20>(Q, dir, B[5], V[5], ba);
            mas_cols4<24>(Q, dir, B[6], V[6], ba); mas_cols4<28>(Q, dir, B[7], V[7], ba);
          }
        }
        if (DMA) wait_groups(issued - (c + 2));                 // chunk c+1 has landed
        else if (c + 1 < nch) fill_regs(c + 1);                 // D == 1: refill the only slot
        dirsg[(size_t)c * R + x] = dir;                         // x < R: coalesced 256 B per wave
        if (to_band) {
          asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");    // lane 63's asm ds_writes of this chunk
          if (lane < CH) gcur[CH * c + lane + 1] = bout_base[(c & 1) * BND_SLOT + 1 + lane];
        }
        if (from_band && lane < CH) {                           // slot c & 1 was read above: it takes chunk c+2
          prevarea[(c & 1) * BND_SLOT + lane] = nb;
          if (c + 3 < nch) nb = __hip_atomic_load(gprev + CH * (c + 3) + lane, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
      } else if (wave_active && w > 0 && c == 2 * u - 1) {
        // the chunk before this wave's first: pick up Q[64u-1, 64u-1] as carry-in
        carry = bin_base[(c & 1) * BND_SLOT + CH];
      }
      step_barrier();
    }
    __syncthreads();                                            // the band's stores to gcur are visible to the next band's loads
  }
  __syncthreads();                                              // every direction word is in memory

#ifdef MAS_STAMPS
  unsigned long long st1 = __builtin_readcyclecounter();
#endif
  // ---------------- backtrack (wave 0): rows, not columns ----------------
  // direction word of (row, chunk): column 32c+j at bit 31-j
  if (w == 0) {
    int idx = t_x - 1;
    int y   = t_y - 1;
    while (y >= 0 && idx > 0) {                      // idx==0: no further moves (core.pyx:34 `index != 0`)
      const int c  = y >> 5;
      const int r  = idx - lane;                      // lane l holds the word of row idx-l
      const unsigned wv = (r >= 0) ? dirsg[(size_t)c * R + r] : 0u;
      const int base = idx;
      const int ylo  = c << 5;
      do {
        const unsigned word = (unsigned)__builtin_amdgcn_readlane((int)wv, base - idx);
        const unsigned m = word >> (31 - (y & 31));   // column y at bit 0, y-1 at bit 1, ...
        if (m == 0u) { y = ylo - 1; break; }          // stays on this row down to the chunk start
        const int yp = y - __builtin_ctz(m);          // first column (going down) with a diagonal move
        starts[idx] = yp;                             // row idx occupies columns [yp, ...); uniform store
        idx -= 1;
        y = yp - 1;
      } while (idx > 0 && y >= ylo);                  // at most 32 rows per chunk: base - idx < 64
    }
    if (t_x > 0) starts[0] = 0;
  }
  __syncthreads();
  for (int xx = t_x + tid; xx <= T_x; xx += NT) starts[xx] = t_y;   // rows >= t_x: empty interval
  __syncthreads();

#ifdef MAS_STAMPS
  unsigned long long st2 = __builtin_readcyclecounter();
#endif
  // ---------------- outputs: intervals, durations, frame -> token ----------------
  for (int xx = tid; xx <= T_x; xx += NT) a.starts[(int64_t)b * (T_x + 1) + xx] = starts[xx];
  if (a.durations) {
    for (int xx = tid; xx < T_x; xx += NT)
      a.durations[(int64_t)b * T_x + xx] = (float)(starts[xx + 1] - starts[xx]);
  }
  if (a.frame2token) {
    for (int yy = tid; yy < T_y; yy += NT) {
      int tok = -1;
      if (yy < t_y) {                                 // largest row with starts[row] <= yy
        int lo = 0, hi = t_x - 1;
        while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (starts[mid] <= yy) lo = mid; else hi = mid - 1; }
        tok = lo;
      }
      a.frame2token[(int64_t)b * T_y + yy] = tok;
    }
  }
#ifdef MAS_STAMPS
  if (b == 0 && tid == 0 && a.status) {
    unsigned long long st3 = __builtin_readcyclecounter();
    a.status[1] = (int)(st1 - st0); a.status[2] = (int)(st2 - st1); a.status[3] = (int)(st3 - st2);
  }
#endif
}

}  // namespace

extern "C" size_t gt_mas_long_workspace_bytes(int B, int T_x, int T_y)
{
  if (B <= 0 || T_x <= 0 || T_y <= 0) return 0;
  return ml_starts_bytes(B, T_x) + ml_bandq_bytes(B, T_y) + ml_dirs_bytes(B, T_x, T_y);
}

extern "C" int gt_mas_long_f32(const float* logp, const float* mask,
                               const int32_t* t_x, const int32_t* t_y,
                               void* path, int path_dtype,
                               float* durations, int32_t* frame2token,
                               int B, int T_x, int T_y, int64_t stride_b, int64_t stride_x,
                               void* workspace, size_t workspace_bytes,
                               int32_t* status, void* stream)
{
  if (B < 0 || T_x < 0 || T_y < 0) return GT_E_INVAL;
  if (B == 0 || T_x == 0 || T_y == 0) return GT_OK;            // nothing to write
  if (!logp || !t_x || !t_y) return GT_E_INVAL;
  if (path && (path_dtype < GT_DT_F32 || path_dtype > GT_DT_U8)) return GT_E_INVAL;
  if (stride_x < T_y || stride_b < (int64_t)T_x * stride_x) return GT_E_INVAL;
  if (!workspace) return GT_E_INVAL;
  if (T_x > TX_MAX || T_y > TY_MAX || B > GT_MAS_LONG_MAX_B) return GT_E_UNSUPPORTED;
  if (workspace_bytes < gt_mas_long_workspace_bytes(B, T_x, T_y)) return GT_E_INVAL;
  if ((uintptr_t)workspace % 4) return GT_E_ALIGN;

  const int nblk = (T_x + 63) / 64;
  const int W = nblk < MAXW ? nblk : MAXW;
  const bool dma = !mask && T_y >= 4 && (T_y % 4 == 0) && (stride_x % 4 == 0) && (stride_b % 4 == 0) &&
                   ((uintptr_t)logp % 16 == 0);
  int depth = 1;                                               // deepest ring that fits
  if (dma) {
    const size_t room = LDS_CAP - ml_lds_fixed(W, T_x);
    depth = (int)(room / ((size_t)W * TILE_F * 4));
    if (depth > MAXD) depth = MAXD;
    if (depth < 2) return GT_E_UNSUPPORTED;                    // not reached for T_x <= GT_MAS_LONG_MAX_TX
  }
  const size_t lds = ml_lds_fixed(W, T_x) + (size_t)W * depth * TILE_F * 4;
  if (lds > LDS_CAP) return GT_E_UNSUPPORTED;

  unsigned char* ws = static_cast<unsigned char*>(workspace);
  MasLongArgs a;
  a.logp = logp; a.mask = mask; a.t_x = t_x; a.t_y = t_y;
  a.durations = durations; a.frame2token = frame2token;
  a.starts = reinterpret_cast<int32_t*>(ws);
  a.bandq  = reinterpret_cast<float*>(ws + ml_starts_bytes(B, T_x));
  a.dirs   = reinterpret_cast<unsigned*>(ws + ml_starts_bytes(B, T_x) + ml_bandq_bytes(B, T_y));
  a.T_x = T_x; a.T_y = T_y; a.stride_b = stride_b; a.stride_x = stride_x; a.status = status;
  a.gbf = ml_gbf(T_y); a.R = ml_rows(T_x); a.nchT = ml_nch(T_y); a.depth = depth;

  hipStream_t st = static_cast<hipStream_t>(stream);
  using KernT = void (*)(MasLongArgs);
  static const KernT kerns[3] = {gt_mas_long_dp_kernel<true, false>, gt_mas_long_dp_kernel<false, false>,
                                 gt_mas_long_dp_kernel<false, true>};
  static bool attr_set[3] = {false, false, false};             // benign one-time cache, as in gt_mas_f32
  const int k = dma ? 0 : (mask ? 2 : 1);
  if (!attr_set[k]) {
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(kerns[k]),
                            hipFuncAttributeMaxDynamicSharedMemorySize, (int)LDS_CAP) != hipSuccess)
      return GT_E_LAUNCH;
    attr_set[k] = true;
  }
  hipLaunchKernelGGL(kerns[k], dim3(B), dim3(W * 64), lds, st, a);
  if (gt_launch_status(__func__)) return GT_E_LAUNCH;

  if (path && gt_mas_expand_launch(a.starts, path, path_dtype, B, T_x, T_y, stream)) return GT_E_LAUNCH;
  return GT_OK;
}
