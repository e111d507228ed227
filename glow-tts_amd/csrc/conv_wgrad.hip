// Weight gradient of the rows-layout 1-D convolution on bf16 MFMA for gfx950, plus the
// weight-norm backward that consumes it.  (The reference gets these from autograd through
// ATen conv backward + torch weight_norm: modules.py:127-141,152,165; attentions.py:103.)
//
//   dW[tap][co][ci] = sum_m dY[m, co] * X[m + tap - k/2, ci]          (reduction over ALL rows)
//
// MFMA A = dY^T (rows = co, k = row m), MFMA B = X (k = row m + tap shift, cols = ci).  Both
// operands have the reduction index strided in memory (channels-last), so tiles are staged
// row-major in LDS by coalesced 16-byte loads and consumed through ds_read_b64_tr_b16 (the
// hardware transposing read), pitch = row bytes + 64 so that the four rows of a read block hit
// disjoint bank windows.  One workgroup = 128 co x 64 ci x all taps over one slab of rows; slab
// partials go to a workspace [S][taps][Cout][Cin] with plain 128-byte-coalesced stores (float
// atomics would cap at ~1.3 TB/s) and are summed by the weight-norm backward kernel, which then
// maps dW to (dv, dg) or to a plain dw in the parameter's own [Cout, Cin, taps] layout.
#include <stdlib.h>
#include "common.h"
#include "internal.h"
#include "mfma_frag.h"
#include "../../include/glowtts_hip.h"

namespace {

constexpr int SLAB_Q = 64;                    // slab_rows is a multiple of this (host planners), so only a job's LAST slab ends ragged

typedef __attribute__((__vector_size__(4 * sizeof(short)))) short s16x4_t;

__device__ __forceinline__ unsigned lds_off(const void* p) { return (unsigned)reinterpret_cast<uintptr_t>(p); }

__device__ __forceinline__ bf16x8_t tr_frag(const unsigned char* p0, const unsigned char* p1) {
  // two transposing reads: rows kb..kb+3 and kb+4..kb+7 of this lane's column
  const s16x4_t lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4_t*)(uintptr_t)p0);
  const s16x4_t hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4_t*)(uintptr_t)p1);
  typedef __attribute__((__vector_size__(8 * sizeof(short)))) short s16x8_t;
  s16x8_t v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
  return __builtin_bit_cast(bf16x8_t, v);
}

// LDS-DMA: 16 bytes per lane from `base` + `off` bytes to LDS bytes [dst_base + 16 * lane, +16) — no VGPR destination, so the ring below
// costs no registers; in inline asm because hipcc drains vmcnt(0) in front of every LDS read while a builtin glds is in flight.
// A wave-uniform base and a 32-bit byte offset per lane: each lane's offsets within a stage stay in registers and the base moves from
// stage to stage with scalar arithmetic (no 64-bit vector address per load; measured against that form in
// `profiles/wgrad_pair_variants.txt` for the paired tile and `profiles/wgrad_share_bench.txt` for the 4-wave one).  s_nop 4: the base
// may come from a v_readfirstlane.
__device__ __forceinline__ void glds16s(const void* base, unsigned off, unsigned dst_base) {
  unsigned keep;
  asm volatile("s_nop 4\n\ts_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\t"
               "global_load_lds_dwordx4 %1, %2\n\ts_mov_b32 m0, %0"
               : "=&s"(keep) : "v"(off), "s"(base), "s"(dst_base) : "memory");
}
template <int N> __device__ __forceinline__ void wait_vm() { asm volatile("s_waitcnt vmcnt(%0)" :: "n"(N) : "memory"); }

// Geometry of one ring stage: KB rows of NY dY blocks (128 columns = 256 B per row and block) and KB + TAPS - 1 rows of the X tile (XCH
// 16-byte chunks per row: 64 NJ columns, NJ = 1 or 3, or two 64-column blocks side by side), both DENSE — an LDS-DMA instruction writes
// 64 lanes x 16 B to consecutive LDS bytes, so rows shorter than 1 KB cannot be padded.  Bank conflicts of the transposing reads (a
// 32-lane group reads 4 rows x 64 B in one LDS cycle if they fall into four different 64-byte windows of the 256-byte bank period) are
// avoided by permuting the 16-byte chunks of a row on the SOURCE side instead: LDS chunk c' of row r holds global chunk c' ^ 4 phase(r).
// Rows of 256 B (dY; X with two blocks) alias every row: phase r & 3.  Rows of 128 B or 384 B alias every second row, and rows r, r + 1
// sit in different halves of the period anyway: phase (r >> 1) & 1.
// NW waves form NW / 4 groups, each the 2 x 2 of 64 co x 32 ci waves that owns one 128 co x 64 NJ ci tile: group g takes dY block g of
// the stage if there are two, X block g if there are two.
template <int TAPS_, int NJ_, int KB_, int NST_, int NW_, int NY_, int XCH_> struct WgGeo {
  static constexpr int TAPS = TAPS_, NJ = NJ_, KB = KB_, NST = NST_, NW = NW_, NY = NY_, XCH = XCH_;
  static constexpr int NT = 64 * NW;                 // threads
  static constexpr int XR = KB + TAPS - 1;
  static constexpr bool XSW4 = XCH * 16 == 256;      // X rows take dY's row phase
  static constexpr int YB = NY * KB * 256, XB = XR * XCH * 16, STAGE = YB + XB;
  static constexpr int YI = NY * KB * 16 / NT;       // dY LDS-DMA instructions per wave and stage
  static constexpr int NWX = XR * XCH / NW;          // X chunks per wave and stage
  static constexpr int XI = (NWX + 63) / 64;         // ... instructions (the last one partially masked; every wave has a lane in each)
  static constexpr int NLD = YI + XI;                // LDS-DMA instructions one wave has in flight per stage
  static constexpr int NB = TAPS * NJ;               // X fragments (= MFMA pairs) per k-step and wave
  static constexpr int LDS = NST * STAGE;
  static constexpr int GA = NY == 2 ? KB * 256 : 0;                 // group g: byte offset of its dY block in the stage ...
  static constexpr int GX = XCH == 16 * NJ ? 8 : 0;                 // ... chunk offset of its X block in a row
  static constexpr int GCO = NY == 2 ? 128 : 0, GCI = GX * 8;       // ... and its tile's origin relative to (co0, ci0)
  static_assert(KB % 16 == 0 && SLAB_Q % KB == 0, "stage rows");
  static_assert((NY * KB * 16) % NT == 0 && (XR * XCH) % NW == 0, "chunks split evenly over the waves");
  static_assert(NWX > 64 * (XI - 1), "every wave issues all XI instructions");
  static_assert(STAGE % 256 == 0 && YB % 256 == 0, "stages keep the bank phase");
  static_assert(LDS <= (NW == 4 ? 80 : 160) * 1024, "two 4-wave workgroups or one 8-wave workgroup per CU");
  static_assert((NST - 2) * NLD <= 63, "vmcnt field");
  static_assert(TAPS == 1 || NJ == 1, "taps or channel groups");
  static_assert(NW == 4 * NY * (GX ? 2 : 1) && XCH == 8 * NJ * (GX ? 2 : 1), "one group per tile");
  static __device__ __forceinline__ int xphase(int r) { return XSW4 ? r & 3 : (r >> 1) & 1; }
};

// One (job, tile, slab): the dY view is Ncols columns wide; dY column c is output channel co_begin + c of a conv with Cout channels.
struct WgArgs {
  const bf16_t* X; int ldx; const bf16_t* dY; int ldy;
  float* part; float* part_bias; int R, Cin, Cout, slab_rows, co0, ci0, slab, co_begin, Ncols;
};
__device__ __forceinline__ WgArgs wg_args(const gt_wgrad_job& j, int co0, int ci0, int slab)
{
  return {static_cast<const bf16_t*>(j.X), j.ldx, static_cast<const bf16_t*>(j.dY), j.ldy, j.part, j.part_bias, j.R, j.Cin, j.Cout,
          j.slab_rows, co0, ci0, slab, j.co_begin, j.co_count};
}

// column sums of dY ride along: VALU adds on a dY^T fragment
__device__ __forceinline__ void bias_add(float& bsum, const bf16x8_t& a)
{
  const u32x4_t w4 = __builtin_bit_cast(u32x4_t, a);
#pragma unroll
  for (int d = 0; d < 4; ++d) bsum += __uint_as_float(w4[d] << 16) + __uint_as_float(w4[d] & 0xffff0000u);
}

// What every form of the tile does the same way: the stage filler, the ring's wait, the fragment reads and the stores.  Wave (wco, wci)
// of a group owns 64 output channels x (32 input channels of every 64-group) x all taps: per 16-row k-step 2 dY^T fragments + NB X
// fragments for 2 NB MFMAs.  The k-loops over these pieces are wgrad_tile and wgrad_pair_tile below.
//
// Round 3: the operands come through an NST-deep LDS ring filled by LDS-DMA.  The round-2 form (64-row stages staged through
// registers, one stage ahead) took 2.0 us per stage whatever the tap count — 0.53 us of MFMA work at k = 5, 0.1 us at k = 1: one
// HBM/L2 round trip per stage with nothing else in flight (serial profile of the step: 480 us for the decoder's k = 5 launch, 322 us
// for its k = 1 launch).  Now NST - 1 stages are in flight per workgroup, none of them holds a register, with <= 256 registers two
// 4-wave workgroups share a CU, and the k = 1 tile spans 192 input channels (2 + 3 fragments for 6 MFMAs instead of 2 + 1 for 2).
template <class G> struct WgTile {
  static constexpr int KB = G::KB, NST = G::NST, TAPS = G::TAPS, NJ = G::NJ, NB = G::NB, padl = TAPS >> 1;
  static constexpr int NOX = TAPS < 4 ? TAPS : 4;      // distinct row phases of the X swizzle over the taps
  const WgArgs a;
  unsigned char* const ring;                           // [NST][STAGE]
  const int tid, lane, wave, grp, wco, wci;
  const int gco0, gci0;                                // this group's tile
  const int mbeg, mend, nst;
  const int h;                                         // k half (rows 8h..8h+7 of a 16-row step)
  int yrow[G::YI], xrow[G::XI];                        // this lane's chunks of a stage: rows relative to the stage's first dY row ...
  unsigned yoff[G::YI], xoff[G::XI];                   // ... and byte offsets from the stage's first dY row / first X row (row mb - padl)
  bool xact[G::XI];
  int offA[2], offX[NOX];

  __device__ __forceinline__ WgTile(const WgArgs& a_, unsigned char* ring_)
      : a(a_), ring(ring_), tid(threadIdx.x), lane(tid & 63), wave(__builtin_amdgcn_readfirstlane(tid >> 6)),
        grp(G::NW == 8 ? wave >> 2 : 0), wco((wave >> 1) & 1), wci(wave & 1),
        gco0(a.co0 + grp * G::GCO), gci0(a.ci0 + grp * G::GCI),
        mbeg(a.slab * a.slab_rows), mend(min(a.R, mbeg + a.slab_rows)), nst((mend - mbeg + KB - 1) / KB), h(lane >> 5)
  {
    // ---- what this lane fetches per stage (the same rows and offsets in both fill paths): chunk L of the stage's dY part is row (L >> 4) % KB of block L / (16 KB), chunk L of its X part is row L / XCH
#pragma unroll
    for (int j = 0; j < G::YI; ++j) {
      const int L = j * G::NT + tid, r = (L >> 4) & (KB - 1), c = (L & 15) ^ ((r & 3) << 2);
      const int col = min(a.co0 + (G::NY == 2 ? L / (16 * KB) * 128 : 0) + c * 8, a.Ncols - 8);   // columns past the view: a valid chunk whose products nobody stores
      yrow[j] = r; yoff[j] = (unsigned)(r * a.ldy + col) * 2u;
    }
#pragma unroll
    for (int j = 0; j < G::XI; ++j) {
      const int Lw = j * 64 + lane, L = wave * G::NWX + Lw, r = L / G::XCH, c = (L - r * G::XCH) ^ (G::xphase(r) << 2);
      xact[j] = Lw < G::NWX;
      xrow[j] = r - padl; xoff[j] = (unsigned)(r * a.ldx + min(a.ci0 + c * 8, a.Cin - 8)) * 2u;
    }
    // ---- lane geometry of the transposing read (see cdna guide T10): within a 16-lane group lane
    // 4q+p supplies the address of block row q, columns 4p..4p+3 and receives column (lane&15).
    const int li = lane & 15, q = li >> 2, p = li & 3;
    const int colhalf = ((lane >> 4) & 1) * 16;          // which 16 columns of the 32-wide MFMA block
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int ch = wco * 8 + i * 4 + (colhalf >> 3) + (p >> 1);
      offA[i] = grp * G::GA + (8 * h + q) * 256 + ((ch ^ (q << 2)) << 4) + (p & 1) * 8;
    }
#pragma unroll
    for (int t = 0; t < NOX; ++t) {
      const int ch = grp * G::GX + wci * 4 + (colhalf >> 3) + (p >> 1);
      offX[t] = (8 * h + q) * (G::XCH * 16) + ((ch ^ (G::xphase(q + t) << 2)) << 4) + (p & 1) * 8;
    }
  }

  static __device__ __forceinline__ int next_slot(int sl) { return sl + 1 == NST ? 0 : sl + 1; }
  __device__ __forceinline__ const unsigned char* stage(int sl) const { return ring + (size_t)sl * G::STAGE; }

  __device__ __forceinline__ void issue(int s, int sl_i) const {        // stage s into ring slot sl_i (= s % NST, tracked by the caller)
    const int mb = mbeg + s * KB;
    const unsigned slot = lds_off(ring) + (unsigned)sl_i * G::STAGE;
    const bool edge = (mb - padl < 0) || (mb + KB + padl > a.R) || (mb + KB > mend);       // workgroup-uniform
    const unsigned char* ys = reinterpret_cast<const unsigned char*>(a.dY + (size_t)mb * a.ldy);
    const unsigned char* xs = reinterpret_cast<const unsigned char*>(a.X + (ptrdiff_t)(mb - padl) * a.ldx);
    if (!edge) {
#pragma unroll
      for (int j = 0; j < G::YI; ++j) glds16s(ys, yoff[j], slot + (unsigned)(j * G::NT + wave * 64) * 16);
#pragma unroll
      for (int j = 0; j < G::XI; ++j)
        if (xact[j]) glds16s(xs, xoff[j], slot + G::YB + (unsigned)(wave * G::NWX + j * 64) * 16);
    } else {
      // first stage of the tensor / last stage of a job: rows outside [0, R) and dY rows past the slab read as zero (plain loads; the
      // compiler's vmcnt(0) in front of the LDS writes also retires every LDS-DMA issued before)
      unsigned char* sl = ring + (size_t)sl_i * G::STAGE;
#pragma unroll
      for (int j = 0; j < G::YI; ++j) {
        const int m = mb + yrow[j];
        u32x4_t v = {0u, 0u, 0u, 0u};
        if (m < mend) v = *reinterpret_cast<const u32x4_t*>(ys + yoff[j]);
        *reinterpret_cast<u32x4_t*>(sl + (size_t)(j * G::NT + tid) * 16) = v;
      }
#pragma unroll
      for (int j = 0; j < G::XI; ++j) {
        const int m = mb + xrow[j];
        u32x4_t v = {0u, 0u, 0u, 0u};
        if (xact[j]) {
          if (m >= 0 && m < a.R) v = *reinterpret_cast<const u32x4_t*>(xs + xoff[j]);
          *reinterpret_cast<u32x4_t*>(sl + G::YB + (size_t)(wave * G::NWX + j * 64 + lane) * 16) = v;
        }
      }
    }
  }
  __device__ __forceinline__ void prefill() const {
#pragma unroll 1
    for (int s = 0; s < NST - 1 && s < nst; ++s) issue(s, s);
  }
  // This wave's share of stage s has landed when at most (stages issued after s) x NLD of its LDS-DMAs are still in flight; behind the
  // barrier everyone's share has and everyone has read the last fragment of stage s - 1, whose slot stage s + NST - 1 goes to.
  __device__ __forceinline__ void wait_stage(int s) const {
    const int after = min(nst - 1, s + NST - 2) - s;
    if (after >= NST - 2) wait_vm<(NST - 2) * G::NLD>();
    else wait_vm<0>();
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
  }

  // fragments of k-step ks of the stage whose dY part is at yb and X part at xb: the wave's two dY^T fragments; its X fragment (t, j)
  __device__ __forceinline__ void read_a(bf16x8_t (&af)[2], const unsigned char* yb, int ks) const {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const unsigned char* ya = yb + offA[i] + ks * 16 * 256;
      af[i] = tr_frag(ya, ya + 4 * 256);
    }
  }
  __device__ __forceinline__ bf16x8_t read_b(const unsigned char* xb, int ks, int t, int j) const {
    const unsigned char* xa = xb + offX[t & 3] + (ks * 16 + t) * (G::XCH * 16) + j * 128;
    return tr_frag(xa, xa + 4 * (G::XCH * 16));
  }

  // ---- slab partial: part[slab][tap][co][ci], lane = ci (128-byte rows per register)
  __device__ __forceinline__ void store_part(const f32x16_t (&acc)[NB][2]) const {
    const size_t row0 = (size_t)a.slab * TAPS * a.Cout + a.co_begin;           // of tap 0, column 0 of the view
#pragma unroll
    for (int t = 0; t < TAPS; ++t)
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        const int ci = gci0 + j * 64 + wci * 32 + (lane & 31);
        if (ci >= a.Cin) continue;
        float* pt = a.part + (row0 + (size_t)t * a.Cout) * a.Cin + ci;
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int e = 0; e < 16; ++e) {
            const int co = gco0 + wco * 64 + i * 32 + (e & 3) + 8 * (e >> 2) + 4 * h;
            if (co < a.Ncols) pt[(size_t)co * a.Cin] = acc[t * NJ + j][i][e];
          }
      }
  }
  // ---- column sums of the wave's dY^T fragment i
  __device__ __forceinline__ bool has_bias() const { return gci0 == 0 && a.part_bias; }
  __device__ __forceinline__ void store_bias(float bsum, int i) const {
    const float tot = bsum + __shfl_xor(bsum, 32);            // the two k halves of a column live 32 lanes apart
    const int co = gco0 + wco * 64 + i * 32 + (lane & 31);
    if (h == 0 && co < a.Ncols) a.part_bias[(size_t)a.slab * a.Cout + a.co_begin + co] = tot;
  }
};

template <int TAPS> struct WgSel;
// Per tap count: rows per ring stage (KB), ring depth (NST), input-channel groups of 64 per workgroup tile (NJ).
// (measured on the decoder's 48 k = 5 jobs of 8.9 k rows, `profiles/r03_wgrad_variants.txt`: 32-row stages x 5 deep 336-355 us, 64-row
//  stages x 3 deep 310-316 us — half the barriers; reading the fragments of k-step i + 1 ahead of the MFMAs of k-step i changed nothing
//  with two workgroups per CU and was dropped)
template <> struct WgSel<5> { static constexpr int NJ = 1, KB = 64, NST = 3; };
template <> struct WgSel<3> { static constexpr int NJ = 1, KB = 64, NST = 3; };
template <> struct WgSel<1> { static constexpr int NJ = 3, KB = 32, NST = 3; };
// The 4-wave tile: one workgroup = 128 output channels [co0, co0 + 128) x 64 NJ input channels x all taps, rows of one slab.
template <int TAPS> using WgGeo4 = WgGeo<TAPS, WgSel<TAPS>::NJ, WgSel<TAPS>::KB, WgSel<TAPS>::NST, 4, 1, 8 * WgSel<TAPS>::NJ>;
// The paired tile (TAPS = 5, 3): one 512-thread workgroup computes TWO 128 co x 64 ci tiles of one (job, slab) from one ring.
//   KIND 0, same-co pair: both groups read the one dY block [co0, co0 + 128); group g reads X columns [ci0 + 64 g, +64).  The X stage
//           has 256-byte rows.  A group whose columns start at or past Cin is dead (a SINGLE: the leftover tile of an odd x odd grid):
//           it issues its share of the loads and executes every barrier, but reads no fragment, issues no MFMA and stores nothing.
//   KIND 1, same-ci pair: both groups read the one X block [ci0, ci0 + 64); group g reads dY block [co0 + 128 g, +128).
// The 4-wave form stages every dY block once per ci tile and every X block once per co tile; here a stage is 33 KB (KIND 0) or 40.5 KB
// (KIND 1) for two tiles where two 4-wave workgroups staged 2 x 24.5 KB.  One workgroup per CU has the whole LDS: KIND 0 runs a
// 4-deep ring (132 KB), KIND 1 a 3-deep one (121.5 KB; 4 stages would be 162 KB).
template <int TAPS, int KIND> using WgGeo8 = WgGeo<TAPS, 1, 64, KIND ? 3 : 4, 8, KIND ? 2 : 1, KIND ? 8 : 16>;

// The 4-wave k-loop: all fragment reads of a k-step, then its MFMAs.  The wci = 0 waves sum the columns of both dY^T fragments.
template <class G> __device__ __forceinline__ void wgrad_tile(const WgArgs& a)
{
  constexpr int KB = G::KB, NST = G::NST, NB = G::NB;
  extern __shared__ __attribute__((aligned(1024))) unsigned char ring[];
  const WgTile<G> T(a, ring);
  const bool do_bias = T.has_bias() && T.wci == 0;

  f32x16_t acc[NB][2];
  float bsum[2] = {0.f, 0.f};
#pragma unroll
  for (int t = 0; t < NB; ++t)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[t][j][e] = 0.0f;
  bf16x8_t af[2], bfg[NB];

  T.prefill();
  int cslot = 0, islot = NST - 1;                               // ring slots of the stage computed / the stage issued in this iteration
#pragma unroll 1
  for (int s = 0; s < T.nst; ++s) {
    T.wait_stage(s);
    if (s + NST - 1 < T.nst) T.issue(s + NST - 1, islot);
    const unsigned char* yb = T.stage(cslot);
    const unsigned char* xb = yb + G::YB;
    cslot = T.next_slot(cslot);
    islot = T.next_slot(islot);
#pragma unroll
    for (int ks = 0; ks < KB / 16; ++ks) {
      // all 2 + NB fragment reads of the k-step go out back to back; the MFMAs start as they arrive (counted lgkmcnt), the other
      // workgroup of the CU computes meanwhile
      T.read_a(af, yb, ks);
#pragma unroll
      for (int t = 0; t < G::TAPS; ++t)
#pragma unroll
        for (int j = 0; j < G::NJ; ++j) bfg[t * G::NJ + j] = T.read_b(xb, ks, t, j);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int t = 0; t < NB; ++t)
#pragma unroll
        for (int i = 0; i < 2; ++i) acc[t][i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[i], bfg[t], acc[t][i], 0, 0, 0);
      if (do_bias) { bias_add(bsum[0], af[0]); bias_add(bsum[1], af[1]); }
    }
  }
  T.store_part(acc);
  if (do_bias) { T.store_bias(bsum[0], 0); T.store_bias(bsum[1], 1); }
}

// The paired k-loop.  Each accumulator sees the fragments wgrad_tile gives it, in the same ascending 16-row k-steps of the same 64-row
// stages: partials are bit-identical to the 4-wave form.
template <class G> __device__ __forceinline__ void wgrad_pair_tile(const WgArgs& a)
{
  constexpr int KB = G::KB, NST = G::NST, NB = G::NB;
  extern __shared__ __attribute__((aligned(1024))) unsigned char ring[];
  const WgTile<G> T(a, ring);
  const bool live = G::NY == 2 ? T.gco0 < a.Ncols : T.gci0 < a.Cin;                       // wave-uniform
  // column sums of dY: wave (wco, wci) sums the columns of its dY^T fragment wci (wgrad_tile: the wci = 0 waves sum both fragments and
  // are the last at every barrier); the additions of a column and their order are the same
  const bool do_bias = live && T.has_bias();

  f32x16_t acc[NB][2];
  float bsum = 0.f;
#pragma unroll
  for (int t = 0; t < NB; ++t)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[t][j][e] = 0.0f;

  // Fragments one k-step ahead.  The two waves of a SIMD run this same program behind the same barrier, so with wgrad_tile's order
  // (all reads of a k-step, then its MFMAs) both wait for their reads together and the matrix pipe idles meanwhile.  Here the dY^T
  // fragments are double-buffered (8 registers) and each X fragment is re-read for the NEXT k-step right behind the two MFMAs that
  // consume it, so the reads of k-step i + 1 travel under the MFMAs of k-step i.  The step to the next stage (wait, barrier, issue)
  // sits in front of a stage's LAST k-step, whose fragments are in registers by then, so the prefetch runs across stages too.
  bf16x8_t af[2][2], bfg[NB];
  // k-step ks on the fragments in registers; meanwhile fetch those of k-step ksn of the stage at ybn
  auto kstep = [&](int ks, const unsigned char* ybn, int ksn) {
    const int cur = ks & 1;
    T.read_a(af[cur ^ 1], ybn, ksn);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int t = 0; t < NB; ++t) {
#pragma unroll
      for (int i = 0; i < 2; ++i) acc[t][i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[cur][i], bfg[t], acc[t][i], 0, 0, 0);
      bfg[t] = T.read_b(ybn + G::YB, ksn, t, 0);
      __builtin_amdgcn_sched_barrier(0);
    }
    if (do_bias) bias_add(bsum, T.wci ? af[cur][1] : af[cur][0]);
  };

  T.prefill();
  int cslot = 0, islot = NST - 1;
  int pend_s = -1, pend_slot = 0;                               // group 1: the stage to issue, deferred (below)
  // Step to stage s.  Every wave, live or dead, runs this nst times: the wait counts, the barriers and the issues depend on s and nst alone.
  // Group 0 issues its share right behind the barrier, group 1 three k-steps later (the slot stays free until the next barrier, and
  // the share is issued before this wave's next wait either way): issuing together, the two waves of a SIMD left its matrix pipe idle
  // (measured: 303 -> 293 us for the decoder's launch, `profiles/wgrad_pair_variants.txt`).
  auto advance = [&](int s) {
    T.wait_stage(s);
    if (s + NST - 1 < T.nst) {
      if (T.grp == 0) T.issue(s + NST - 1, islot);
      else { pend_s = s + NST - 1; pend_slot = islot; }
    }
    islot = T.next_slot(islot);
  };
  advance(0);
  const unsigned char* yb = ring;
  if (live) {
    T.read_a(af[0], yb, 0);
#pragma unroll
    for (int t = 0; t < NB; ++t) bfg[t] = T.read_b(yb + G::YB, 0, t, 0);
  }
#pragma unroll 1
  for (int s = 0; s < T.nst; ++s) {
    if (live) {
#pragma unroll
      for (int ks = 0; ks < KB / 16 - 1; ++ks) kstep(ks, yb, ks + 1);
    }
    if (pend_s >= 0) { T.issue(pend_s, pend_slot); pend_s = -1; }
    if (s + 1 < T.nst) advance(s + 1);
    cslot = T.next_slot(cslot);
    yb = T.stage(cslot);
    // (behind the job's last stage this fetches fragments nobody uses, from a ring slot no LDS-DMA is in flight to)
    if (live) kstep(KB / 16 - 1, yb, 0);
  }
  if (!live) return;                                   // (past the last barrier)
  T.store_part(acc);
  if (do_bias) T.store_bias(bsum, T.wci);
}

template <int TAPS>
__global__ __launch_bounds__(256, 2) void gt_conv_wgrad_kernel(
    const bf16_t* __restrict__ X, int ldx, const bf16_t* __restrict__ dY, int ldy,
    float* __restrict__ part, float* __restrict__ part_bias, int R, int Cin, int Cout, int slab_rows)
{
  wgrad_tile<WgGeo4<TAPS>>({X, ldx, dY, ldy, part, part_bias, R, Cin, Cout, slab_rows,
                            (int)blockIdx.x * 128, (int)blockIdx.y * 64 * WgSel<TAPS>::NJ, (int)blockIdx.z, 0, Cout});
}

// Batched form: every workgroup reads its (job, tile) from device tables, so ONE launch per tap count
// covers the weight gradients of a whole network (the jobs' X / dY rows stay resident until then).
template <int TAPS>
__global__ __launch_bounds__(256, 2) void gt_conv_wgrad_batched_kernel(
    const gt_wgrad_job* __restrict__ jobs, const gt_wgrad_tile* __restrict__ tiles)
{
  const gt_wgrad_tile t = tiles[blockIdx.x];
  wgrad_tile<WgGeo4<TAPS>>(wg_args(jobs[t.job], t.co0, t.ci0, t.slab));
}

template <int TAPS>
__global__ __launch_bounds__(512, 1) void gt_conv_wgrad_paired_kernel(
    const gt_wgrad_job* __restrict__ jobs, const gt_wgrad_pair* __restrict__ pairs)
{
  const gt_wgrad_pair t = pairs[blockIdx.x];
  const WgArgs a = wg_args(jobs[t.job], t.co0, t.ci0, t.slab);
  if (t.kind == 0) wgrad_pair_tile<WgGeo8<TAPS, 0>>(a);
  else             wgrad_pair_tile<WgGeo8<TAPS, 1>>(a);
}

template <int TAPS> static int wgrad_lds_attr()
{
  // > 64 KiB of dynamic LDS needs the attribute once per kernel (outside graph capture: run one eager step first)
  if (gt_allow_lds<&gt_conv_wgrad_kernel<TAPS>>(WgGeo4<TAPS>::LDS) || gt_allow_lds<&gt_conv_wgrad_batched_kernel<TAPS>>(WgGeo4<TAPS>::LDS)) return GT_E_LAUNCH;
  return 0;
}
template <int TAPS> constexpr int wgrad_pair_lds() { return WgGeo8<TAPS, 0>::LDS > WgGeo8<TAPS, 1>::LDS ? WgGeo8<TAPS, 0>::LDS : WgGeo8<TAPS, 1>::LDS; }

// Sum the S slab partials and map to the parameter gradient(s).  One WAVE per output channel co (4 per workgroup):
//   plain conv:   dw[co][ci][tap] (+)= dW
//   weight-norm:  w = g v / ||v||  =>  dg = <dW, v>/||v|| ;  dv = g/||v|| (dW - v <dW,v>/||v||^2)
//   bias:         db[co] (+)= sum of the slab column sums
// (Round 2 ran one 256-thread workgroup per co with two __syncthreads and three dependent global round trips for <= 960 elements:
// 144 us for the decoder's 18 k rows, against ~60 us of HBM time for the partials, v and dv.  A wave needs no workgroup barrier —
// its row goes through its own LDS strip for the [tap][ci] -> [ci][tap] transposition — and 32+ rows are in flight per CU.)
constexpr int WNB_ROWS = 4;
__device__ __forceinline__ void weightnorm_bwd_row(
    const float* __restrict__ part, const float* __restrict__ part_bias, int S, const float* __restrict__ v,
    const float* __restrict__ g, const float* __restrict__ inv_norm, float* __restrict__ dv, float* __restrict__ dg,
    float* __restrict__ dbias, int Cout, int Cin, int taps, int accumulate, int co, float* dws)
{
  const int lane = threadIdx.x & 63, n = Cin * taps;
  if (dbias && lane == 0) {
    float sb = 0.f;
    for (int k = 0; k < S; ++k) sb += part_bias[(size_t)k * Cout + co];
    dbias[co] = accumulate ? dbias[co] + sb : sb;
  }
  // coalesced pass over the partials: consecutive lanes = consecutive ci of one (slab, tap) row
  const size_t sstride = (size_t)taps * Cout * Cin;              // one slab
  for (int tap = 0; tap < taps; ++tap) {
    const float* pt = part + ((size_t)tap * Cout + co) * Cin;
    for (int ci = lane; ci < Cin; ci += 64) {
      const float* pp = pt + ci;
      float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;               // 4 loads in flight per lane, not a dependent chain
      int k = 0;
      for (; k + 4 <= S; k += 4) {
        const float a0 = pp[(size_t)k * sstride], a1 = pp[(size_t)(k + 1) * sstride];
        const float a2 = pp[(size_t)(k + 2) * sstride], a3 = pp[(size_t)(k + 3) * sstride];
        s0 += a0; s1 += a1; s2 += a2; s3 += a3;
      }
      for (; k < S; ++k) s0 += pp[(size_t)k * sstride];
      dws[ci * taps + tap] = (s0 + s1) + (s2 + s3);
    }
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  const float* vr = v + (size_t)co * n;
  float* dr = dv + (size_t)co * n;
  if (!g) {
    for (int i = lane; i < n; i += 64) dr[i] = accumulate ? dr[i] + dws[i] : dws[i];
    return;
  }
  float dot = 0.f;
  for (int i = lane; i < n; i += 64) dot += dws[i] * vr[i];
  const float d = wave_sum(dot);
  const float inv = inv_norm[co], gg = g[co];
  if (lane == 0) dg[co] = accumulate ? dg[co] + d * inv : d * inv;
  const float a = gg * inv, bcoef = gg * d * inv * inv * inv;
  for (int i = lane; i < n; i += 64) {
    const float val = a * dws[i] - bcoef * vr[i];
    dr[i] = accumulate ? dr[i] + val : val;
  }
}

// The same row with 16-byte accesses (Cin % 4 == 0; part, v, dv 16-byte aligned, so every (slab, tap) row of the partials and every
// v / dv row starts on a 16-byte boundary).  weightnorm_bwd_row above runs three dependent phases of 4-byte accesses — 15 + 15 + 15
// wave instructions of 256 B for n = 960, the v row requested only after the partials have landed, the old dv row only inside the
// store loop.  Here a lane owns 16-byte CHUNKS: chunk c of the partials is 4 consecutive ci of one tap (c = tap * Cin/4 + ci/4), chunk
// c of v / dv is elements 4c .. 4c+3 of the row.  Per pass of WNF_P chunks per lane (1024 elements: one pass for the decoder's n = 960,
// three at n = 2304) EVERY global load of the pass is issued before the first use: the partials of one or two slabs (three and more go
// chunk by chunk, four loads in flight), the v chunks, and — ahead of the first pass — the old dv chunks, inv_norm, g and the bias partials.
// Results are bit-identical to weightnorm_bwd_row: the slab sum keeps (s0+s1)+(s2+s3) over groups of four slabs, the remainder
// into s0; <dW, v> keeps lane l adding i = l, l+64, ... ascending — v is staged beside dws in the wave's LDS strip and both are read
// back in that order; dv is elementwise from the same a, bcoef, dws[i], v[i].
constexpr int WNF_P = 4;                       // 16-byte chunks per lane and pass
typedef float wnf4_t __attribute__((ext_vector_type(4)));
// Global-address-space accesses: the batched kernel reads its pointers from the job table, which would make these flat instructions
// (counted by the LDS counter as well).  No load below is predicated per lane — a lane past the row's end reads the row's last chunk
// and drops it — and no loaded value is merged with a constant: either makes the compiler wait for each load where it is issued.
__device__ __forceinline__ wnf4_t wnf_ld4(const float* p) { return *(const __attribute__((address_space(1))) wnf4_t*)(uintptr_t)p; }
__device__ __forceinline__ float wnf_ld1(const float* p) { return *(const __attribute__((address_space(1))) float*)(uintptr_t)p; }
__device__ __forceinline__ void wnf_st4(float* p, wnf4_t x) { *(__attribute__((address_space(1))) wnf4_t*)(uintptr_t)p = x; }

// The roundings of the 4-byte form as the compiler emits it, spelled out so that the two forms cannot drift apart: dv = a dW - bcoef v
// is two products and a difference (left to itself the compiler fuses two of the four components of a chunk and not the others);
// the dot product and dg + d inv are fused multiply-adds.
__device__ __forceinline__ float wnf_dv(float a, float dw, float bcoef, float x)
{
#pragma clang fp contract(off)
  const float l = a * dw, r = bcoef * x;
  return l - r;
}

// slab sums of the pass's chunks, NS = S <= 2 slabs: every load of the pass at once.  (s0 + 0) + (0 + 0) is what the 4-byte form computes.
template <int NS>
__device__ __forceinline__ void wnf_slabs_few(const float* const (&pp)[WNF_P], size_t sstride, wnf4_t (&t)[WNF_P])
{
  // (keeps the compiler from hoisting the load the NS = 1 and NS = 2 branches have in common, and its wait, above the branch)
  asm volatile("; %0 slab(s) per pass" :: "n"(NS) : "memory");
  wnf4_t a[WNF_P][NS];
#pragma unroll
  for (int p = 0; p < WNF_P; ++p)
#pragma unroll
    for (int q = 0; q < NS; ++q) a[p][q] = wnf_ld4(pp[p] + (size_t)q * sstride);
#pragma unroll
  for (int p = 0; p < WNF_P; ++p) {
    wnf4_t s0 = 0.f;
#pragma unroll
    for (int q = 0; q < NS; ++q) s0 += a[p][q];
    t[p] = (s0 + 0.f) + (0.f + 0.f);
  }
}

__device__ __forceinline__ void weightnorm_bwd_row16(
    const float* __restrict__ part, const float* __restrict__ part_bias, int S, const float* __restrict__ v,
    const float* __restrict__ g, const float* __restrict__ inv_norm, float* __restrict__ dv, float* __restrict__ dg,
    float* __restrict__ dbias, int Cout, int Cin, int taps, int accumulate, int co, float* dws, float* vs)
{
  const int lane = threadIdx.x & 63, n = Cin * taps, nch = n >> 2;
  const unsigned c4 = (unsigned)Cin >> 2;
  const size_t sstride = (size_t)taps * Cout * Cin;              // one slab
  const float* vr = v + (size_t)co * n;
  float* dr = dv + (size_t)co * n;
  // the row's scalars and the old dv chunks of the first pass: requested now, used after the partials
  float pb, odb, inv, gg, odg;
  if (dbias) {
    pb = wnf_ld1(part_bias + (size_t)max(min(lane, S - 1), 0) * Cout + co);
    if (accumulate) odb = wnf_ld1(dbias + co);
  }
  if (g) {
    inv = wnf_ld1(inv_norm + co); gg = wnf_ld1(g + co);
    if (accumulate) odg = wnf_ld1(dg + co);
  }
  wnf4_t od[WNF_P];
  if (accumulate) {
#pragma unroll
    for (int p = 0; p < WNF_P; ++p) od[p] = wnf_ld4(dr + 4 * min(64 * p + lane, nch - 1));
  }
  for (int c0 = 0; c0 < nch; c0 += 64 * WNF_P) {
    const float* pp[WNF_P]; int o[WNF_P]; wnf4_t vv[WNF_P], t[WNF_P];
#pragma unroll
    for (int p = 0; p < WNF_P; ++p) {
      const unsigned c = (unsigned)min(c0 + 64 * p + lane, nch - 1);
      const unsigned tap = c / c4, ci = (c - tap * c4) * 4;
      pp[p] = part + ((size_t)tap * Cout + co) * Cin + ci;
      o[p] = (int)(ci * taps + tap);
    }
    if (g) {
#pragma unroll
      for (int p = 0; p < WNF_P; ++p) vv[p] = wnf_ld4(vr + 4 * min(c0 + 64 * p + lane, nch - 1));
    }
    // one or two slabs is the usual case (slabs exist to fill the chip; a network's worth of jobs does that alone)
    if (S <= 2) {
      if (S == 1) wnf_slabs_few<1>(pp, sstride, t);
      else        wnf_slabs_few<2>(pp, sstride, t);
#pragma unroll
      for (int p = 0; p < WNF_P; ++p) {
        if (c0 + 64 * p + lane >= nch) continue;
        float* d = dws + o[p];                                    // [tap][ci] -> [ci][tap]
        d[0] = t[p].x; d[taps] = t[p].y; d[2 * taps] = t[p].z; d[3 * taps] = t[p].w;
      }
    } else {
      // three slabs and more: chunk by chunk, four loads in flight as in the 4-byte form (all chunks at once would hold up to 128
      // registers of sums and operands and take resident waves from the usual case)
#pragma unroll 1
      for (int p = 0; p < WNF_P; ++p) {
        const int cp = c0 + 64 * p + lane;
        const unsigned c = (unsigned)min(cp, nch - 1);
        const unsigned tap = c / c4, ci = (c - tap * c4) * 4;
        const float* q = part + ((size_t)tap * Cout + co) * Cin + ci;
        wnf4_t s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
        int k = 0;
        for (; k + 4 <= S; k += 4) {
          const wnf4_t a0 = wnf_ld4(q + (size_t)k * sstride), a1 = wnf_ld4(q + (size_t)(k + 1) * sstride);
          const wnf4_t a2 = wnf_ld4(q + (size_t)(k + 2) * sstride), a3 = wnf_ld4(q + (size_t)(k + 3) * sstride);
          s0 += a0; s1 += a1; s2 += a2; s3 += a3;
        }
        for (; k < S; ++k) s0 += wnf_ld4(q + (size_t)k * sstride);
        const wnf4_t r = (s0 + s1) + (s2 + s3);
        if (cp < nch) {
          float* d = dws + ci * taps + tap;
          d[0] = r.x; d[taps] = r.y; d[2 * taps] = r.z; d[3 * taps] = r.w;
        }
      }
    }
    if (g) {
#pragma unroll
      for (int p = 0; p < WNF_P; ++p) {
        const int c = c0 + 64 * p + lane;
        if (c < nch) *reinterpret_cast<wnf4_t*>(vs + 4 * c) = vv[p];
      }
    }
  }
  if (dbias) {
    float sb = 0.f;
    for (int k0 = 0; k0 < S; k0 += 64) {
      if (k0) pb = wnf_ld1(part_bias + (size_t)min(k0 + lane, S - 1) * Cout + co);
      const int m = min(64, S - k0);
      for (int k = 0; k < m; ++k) sb += __shfl(pb, k);
    }
    if (lane == 0) dbias[co] = accumulate ? odb + sb : sb;
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  float a = 1.f, bcoef = 0.f;
  if (g) {
    float dot = 0.f;
    for (int i = lane; i < n; i += 64) dot = __builtin_fmaf(dws[i], vs[i], dot);
    const float d = wave_sum(dot);
    if (lane == 0) dg[co] = accumulate ? __builtin_fmaf(d, inv, odg) : d * inv;
    a = gg * inv; bcoef = gg * d * inv * inv * inv;
  }
  for (int c0 = 0; c0 < nch; c0 += 64 * WNF_P) {
    if (c0 && accumulate) {
#pragma unroll
      for (int p = 0; p < WNF_P; ++p) od[p] = wnf_ld4(dr + 4 * min(c0 + 64 * p + lane, nch - 1));
    }
#pragma unroll
    for (int p = 0; p < WNF_P; ++p) {
      const int c = c0 + 64 * p + lane;
      if (c >= nch) continue;
      wnf4_t val = *reinterpret_cast<const wnf4_t*>(dws + 4 * c);
      if (g) {
        const wnf4_t x = *reinterpret_cast<const wnf4_t*>(vs + 4 * c);
        val.x = wnf_dv(a, val.x, bcoef, x.x); val.y = wnf_dv(a, val.y, bcoef, x.y);
        val.z = wnf_dv(a, val.z, bcoef, x.z); val.w = wnf_dv(a, val.w, bcoef, x.w);
      }
      if (accumulate) { val.x = od[p].x + val.x; val.y = od[p].y + val.y; val.z = od[p].z + val.z; val.w = od[p].w + val.w; }
      wnf_st4(dr + 4 * c, val);
    }
  }
}

// One row through the 16-byte form where its shape and pointers allow it (a wave-uniform choice), else through weightnorm_bwd_row.
// `strip` is the wave's LDS: [2][strip_elems] floats (dws | v), strip_elems % 4 == 0.
__device__ __forceinline__ void weightnorm_bwd_dispatch(
    const float* __restrict__ part, const float* __restrict__ part_bias, int S, const float* __restrict__ v,
    const float* __restrict__ g, const float* __restrict__ inv_norm, float* __restrict__ dv, float* __restrict__ dg,
    float* __restrict__ dbias, int Cout, int Cin, int taps, int accumulate, int co, float* strip, int strip_elems)
{
  const bool wide = !(Cin & 3) && !((reinterpret_cast<uintptr_t>(part) | reinterpret_cast<uintptr_t>(v) | reinterpret_cast<uintptr_t>(dv)) & 15);
  if (wide) {
    weightnorm_bwd_row16(part, part_bias, S, v, g, inv_norm, dv, dg, dbias, Cout, Cin, taps, accumulate, co, strip, strip + strip_elems);
  } else {
    weightnorm_bwd_row(part, part_bias, S, v, g, inv_norm, dv, dg, dbias, Cout, Cin, taps, accumulate, co, strip);
    // vmcnt(0) lgkmcnt(0): the compiler lays this branch out ahead of the other one and, with flat accesses of this one pending on
    // paper, puts a full wait between every two groups of loads there
    __builtin_amdgcn_s_waitcnt(0x0070);
  }
}

// Rows (waves) per workgroup: blockDim.x / 64, from wnb_rows() on the host.
__global__ __launch_bounds__(64 * WNB_ROWS, 3) void gt_weightnorm_bwd_kernel(
    const float* __restrict__ part, const float* __restrict__ part_bias, int S, const float* __restrict__ v,
    const float* __restrict__ g, const float* __restrict__ inv_norm, float* __restrict__ dv, float* __restrict__ dg,
    float* __restrict__ dbias, int Cout, int Cin, int taps, int accumulate)
{
  extern __shared__ __attribute__((aligned(16))) float dws[];    // [rows][2][strip]: summed dW of a co in natural (ci, tap) order | its v row
  const int w = threadIdx.x >> 6, co = blockIdx.x * (blockDim.x >> 6) + w;
  if (co >= Cout) return;
  const int strip = (Cin * taps + 3) & ~3;
  weightnorm_bwd_dispatch(part, part_bias, S, v, g, inv_norm, dv, dg, dbias, Cout, Cin, taps, accumulate, co, dws + (size_t)w * 2 * strip, strip);
}

// Batched form: one wave per output channel of ANY conv.  The job of a row is the last one whose row_start is at or before it: every
// lane tests the row_start of one job (of four, 256 jobs per round of independent loads) and the ballots count the jobs at or before
// the row — one load latency where a bisection over 120 jobs spent seven dependent ones before the row's first useful load.
__global__ __launch_bounds__(64 * WNB_ROWS, 3) void gt_weightnorm_bwd_batched_kernel(const gt_wnb_job* __restrict__ jobs, int n_jobs, int total_rows,
                                                                                int max_row_elems)
{
  extern __shared__ __attribute__((aligned(16))) float dws[];
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63, row = blockIdx.x * (blockDim.x >> 6) + w;
  if (row >= total_rows) return;
  int cnt = 0;
  for (int i0 = 0; i0 < n_jobs; i0 += 256) {
    int rs[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int i = i0 + 64 * u + lane;
      rs[u] = jobs[min(i, n_jobs - 1)].row_start;                // unpredicated: the four loads leave together
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) cnt += __popcll(__ballot(i0 + 64 * u + lane < n_jobs && rs[u] <= row));
  }
  const int lo = __builtin_amdgcn_readfirstlane(cnt > 0 ? cnt - 1 : 0);
  const gt_wnb_job j = jobs[lo];
  const int strip = (max_row_elems + 3) & ~3;
  weightnorm_bwd_dispatch(j.part, j.part_bias, j.S, j.v, j.g, j.inv_norm, j.dv, j.dg, j.dbias, j.Cout, j.Cin, j.taps,
                          j.accumulate, row - j.row_start, dws + (size_t)w * 2 * strip, strip);
}

// LDS of a launch: every wave holds [2][strip] floats (dW | v of its row), strip = the longest row rounded up to 16 bytes.  Four rows
// per workgroup up to n = 1920; three at the packing limit n = 2304 (54 KB); two up to the n = 3840 the 4-byte form always took.
constexpr size_t WNB_LDS_MAX = 60 * 1024;
static size_t wnb_lds(int rows, int max_row_elems) { return (size_t)rows * 2 * ((max_row_elems + 3) & ~3) * sizeof(float); }
static int wnb_rows(int max_row_elems)
{
  int rows = WNB_ROWS;
  while (rows > 1 && wnb_lds(rows, max_row_elems) > WNB_LDS_MAX) --rows;
  return rows;
}

// Column sums over rows: out[n] (+)= sum_m Y[m, n] (bias gradients).  bf16 or fp32 input.
template <bool F32>
__global__ __launch_bounds__(256) void gt_colsum_kernel(const void* __restrict__ Y, int ldy, float* __restrict__ out,
                                                        int R, int N, int rows_per_block)
{
  // block (x: 64-column group, y: row slab); thread = (column c = tid&63, row phase tid>>6)
  __shared__ float red[4][64];
  const int c = blockIdx.x * 64 + (threadIdx.x & 63), ph = threadIdx.x >> 6;
  const int m0 = blockIdx.y * rows_per_block, m1 = min(R, m0 + rows_per_block);
  float s = 0.f;
  if (c < N) {
    for (int m = m0 + ph; m < m1; m += 4)
      s += F32 ? static_cast<const float*>(Y)[(size_t)m * ldy + c] : bf2f(static_cast<const bf16_t*>(Y)[(size_t)m * ldy + c]);
  }
  red[ph][threadIdx.x & 63] = s;
  __syncthreads();
  if (ph == 0 && c < N) atomicAdd(out + c, red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x]);
}

}  // namespace

extern "C" int gt_conv_wgrad_ci_tile(int taps)
{
  return taps == 1 ? 64 * WgSel<1>::NJ : taps == 3 ? 64 * WgSel<3>::NJ : taps == 5 ? 64 * WgSel<5>::NJ : 0;
}

extern "C" size_t gt_conv_wgrad_workspace_bytes(int R, int Cin, int Cout, int taps, int* slabs_out)
{
  if (R <= 0 || Cin <= 0 || Cout <= 0 || taps <= 0) { if (slabs_out) *slabs_out = 0; return 0; }
  const int cit = gt_conv_wgrad_ci_tile(taps) > 0 ? gt_conv_wgrad_ci_tile(taps) : 64;
  const int tiles = ((Cout + 127) / 128) * ((Cin + cit - 1) / cit);
  // slabs: enough workgroups to cover the chip, but every slab costs one full dW of partial traffic
  // (written here, re-read by gt_weightnorm_bwd) — ~160 workgroups in total, at most 16 slabs
  constexpr int target = 160;
  int S = (target + tiles - 1) / tiles;
  if (S > 16) S = 16;
  const int max_s = (R + SLAB_Q - 1) / SLAB_Q;
  if (S > max_s) S = max_s;
  if (S < 1) S = 1;
  if (slabs_out) *slabs_out = S;
  return ((size_t)S * taps * Cout * Cin + (size_t)S * Cout) * sizeof(float);     // weight partials | bias partials
}

extern "C" int gt_conv_wgrad_bf16(const void* X, int ldx, const void* dY, int ldy, int R, int Cin, int Cout,
                                  int taps, void* workspace, size_t workspace_bytes, void* stream)
{
  if (R <= 0 || Cin <= 0 || Cout <= 0) return GT_E_INVAL;
  if (!X || !dY || !workspace) return GT_E_INVAL;
  if (taps != 1 && taps != 3 && taps != 5) return GT_E_UNSUPPORTED;
  if ((Cin & 7) || (Cout & 7) || (ldx & 7) || (ldy & 7)) return GT_E_ALIGN;
  if (((uintptr_t)X | (uintptr_t)dY) & 15) return GT_E_ALIGN;
  int S = 0;
  if (workspace_bytes < gt_conv_wgrad_workspace_bytes(R, Cin, Cout, taps, &S)) return GT_E_INVAL;
  const int slab_rows = (((R + S - 1) / S) + SLAB_Q - 1) / SLAB_Q * SLAB_Q;
  const int cit = gt_conv_wgrad_ci_tile(taps);
  const dim3 grid((Cout + 127) / 128, (Cin + cit - 1) / cit, S);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const bf16_t* x = static_cast<const bf16_t*>(X); const bf16_t* dy = static_cast<const bf16_t*>(dY);
  float* part = static_cast<float*>(workspace);
  float* pb = part + (size_t)S * taps * Cout * Cin;
  if (wgrad_lds_attr<5>() || wgrad_lds_attr<3>() || wgrad_lds_attr<1>()) return GT_E_LAUNCH;
  if (taps == 5)      hipLaunchKernelGGL(gt_conv_wgrad_kernel<5>, grid, dim3(256), WgGeo4<5>::LDS, st, x, ldx, dy, ldy, part, pb, R, Cin, Cout, slab_rows);
  else if (taps == 3) hipLaunchKernelGGL(gt_conv_wgrad_kernel<3>, grid, dim3(256), WgGeo4<3>::LDS, st, x, ldx, dy, ldy, part, pb, R, Cin, Cout, slab_rows);
  else                hipLaunchKernelGGL(gt_conv_wgrad_kernel<1>, grid, dim3(256), WgGeo4<1>::LDS, st, x, ldx, dy, ldy, part, pb, R, Cin, Cout, slab_rows);
  return gt_launch_status(__func__);
}

extern "C" int gt_weightnorm_bwd(const void* workspace, int R, const float* v, const float* g, const float* inv_norm,
                                 float* dv, float* dg, float* dbias, int Cout, int Cin, int taps, int accumulate, void* stream)
{
  if (!workspace || !v || !dv || Cout <= 0 || Cin <= 0 || taps <= 0) return GT_E_INVAL;
  if (g && (!inv_norm || !dg)) return GT_E_INVAL;
  int S = 0;
  gt_conv_wgrad_workspace_bytes(R, Cin, Cout, taps, &S);
  if ((size_t)WNB_ROWS * Cin * taps * sizeof(float) > WNB_LDS_MAX) return GT_E_UNSUPPORTED;
  const int rows = wnb_rows(Cin * taps);
  const size_t lds = wnb_lds(rows, Cin * taps);
  const float* part = static_cast<const float*>(workspace);
  hipLaunchKernelGGL(gt_weightnorm_bwd_kernel, dim3((Cout + rows - 1) / rows), dim3(64 * rows), lds, static_cast<hipStream_t>(stream),
                     part, part + (size_t)S * taps * Cout * Cin, S, v, g, inv_norm, dv, dg, dbias, Cout, Cin, taps, accumulate);
  return gt_launch_status(__func__);
}

extern "C" int gt_conv_wgrad_batched(const void* jobs_device, const void* tiles_device, int n_tiles5, int n_tiles3,
                                     int n_tiles1, void* stream)
{
  if (!jobs_device || !tiles_device || n_tiles5 < 0 || n_tiles3 < 0 || n_tiles1 < 0) return GT_E_INVAL;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const gt_wgrad_job* jobs = static_cast<const gt_wgrad_job*>(jobs_device);
  const gt_wgrad_tile* tiles = static_cast<const gt_wgrad_tile*>(tiles_device);
  if (wgrad_lds_attr<5>() || wgrad_lds_attr<3>() || wgrad_lds_attr<1>()) return GT_E_LAUNCH;
  if (n_tiles5) hipLaunchKernelGGL(gt_conv_wgrad_batched_kernel<5>, dim3(n_tiles5), dim3(256), WgGeo4<5>::LDS, st, jobs, tiles);
  if (n_tiles3) hipLaunchKernelGGL(gt_conv_wgrad_batched_kernel<3>, dim3(n_tiles3), dim3(256), WgGeo4<3>::LDS, st, jobs, tiles + n_tiles5);
  if (n_tiles1) hipLaunchKernelGGL(gt_conv_wgrad_batched_kernel<1>, dim3(n_tiles1), dim3(256), WgGeo4<1>::LDS, st, jobs, tiles + n_tiles5 + n_tiles3);
  return gt_launch_status(__func__);
}

extern "C" int gt_conv_wgrad_paired(const void* jobs_device, const void* pairs_device, int n_pairs5, int n_pairs3, void* stream)
{
  if (!jobs_device || !pairs_device || n_pairs5 < 0 || n_pairs3 < 0) return GT_E_INVAL;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const gt_wgrad_job* jobs = static_cast<const gt_wgrad_job*>(jobs_device);
  const gt_wgrad_pair* pairs = static_cast<const gt_wgrad_pair*>(pairs_device);
  if (gt_allow_lds<&gt_conv_wgrad_paired_kernel<5>>(wgrad_pair_lds<5>()) || gt_allow_lds<&gt_conv_wgrad_paired_kernel<3>>(wgrad_pair_lds<3>())) return GT_E_LAUNCH;
  if (n_pairs5) hipLaunchKernelGGL(gt_conv_wgrad_paired_kernel<5>, dim3(n_pairs5), dim3(512), wgrad_pair_lds<5>(), st, jobs, pairs);
  if (n_pairs3) hipLaunchKernelGGL(gt_conv_wgrad_paired_kernel<3>, dim3(n_pairs3), dim3(512), wgrad_pair_lds<3>(), st, jobs, pairs + n_pairs5);
  return gt_launch_status(__func__);
}

extern "C" int gt_weightnorm_bwd_batched(const void* jobs_device, int n_jobs, int total_rows, int max_row_elems, void* stream)
{
  if (!jobs_device || n_jobs <= 0 || total_rows <= 0 || max_row_elems <= 0) return GT_E_INVAL;
  if ((size_t)WNB_ROWS * max_row_elems * sizeof(float) > WNB_LDS_MAX) return GT_E_UNSUPPORTED;
  const int rows = wnb_rows(max_row_elems);
  const size_t lds = wnb_lds(rows, max_row_elems);
  hipLaunchKernelGGL(gt_weightnorm_bwd_batched_kernel, dim3((total_rows + rows - 1) / rows), dim3(64 * rows), lds,
                     static_cast<hipStream_t>(stream), static_cast<const gt_wnb_job*>(jobs_device), n_jobs, total_rows, max_row_elems);
  return gt_launch_status(__func__);
}

extern "C" int gt_colsum(const void* Y, int ldy, int is_f32, float* out, int R, int N, void* stream)
{
  if (!Y || !out || R < 0 || N <= 0) return GT_E_INVAL;
  if (R == 0) return GT_OK;
  const int rows_per_block = 128;             // (512: 128 dependent loads per thread — 31 us for 17.8 k x 192 fp32 rows)
  const dim3 grid((N + 63) / 64, (R + rows_per_block - 1) / rows_per_block);
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (is_f32) hipLaunchKernelGGL(gt_colsum_kernel<true>,  grid, dim3(256), 0, st, Y, ldy, out, R, N, rows_per_block);
  else        hipLaunchKernelGGL(gt_colsum_kernel<false>, grid, dim3(256), 0, st, Y, ldy, out, R, N, rows_per_block);
  return gt_launch_status(__func__);
}
