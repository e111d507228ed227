// The Monotonic Alignment Search column shared by gt_mas_f32 (mas.hip: direction bits in LDS) and gt_mas_long_f32
// (mas_long.hip: direction bits in HBM, rows in bands): the constants of the LDS image, the hand-scheduled steady-state
// column and the plain-HIP chunk that holds the x == y cells.  Include after `#pragma clang fp contract(off)`.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#pragma clang fp contract(off)   // bit-exact IEEE adds/compares only

namespace {

constexpr int   CH       = 32;            // columns per chunk
constexpr int   TILE_F   = 64 * CH;       // floats of one wave's logp tile (8 KiB)
constexpr int   BND_SLOT = 36;            // floats per boundary slot (33 used)
constexpr int   BND_F    = 2 * BND_SLOT + 104;  // + dummy area for lanes != 63 -> 176 floats
constexpr float NEG      = -1e9f;         // reference max_neg_val (core.pyx:38)
constexpr int   MAXD     = 4;             // deepest LDS-DMA ring

__device__ __forceinline__ float dpp_wave_shr1(float old, float src) {
  // lane l <- src[l-1]; lane 0 keeps `old` (bound_ctrl off)
  return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(old), __float_as_int(src),
                                                    0x138 /*wave_shr:1*/, 0xf, 0xf, false));
}

__device__ __forceinline__ unsigned lds_off(const void* p) {
  return (unsigned)reinterpret_cast<uintptr_t>(p);          // low 32 bits of a shared pointer = LDS byte offset
}

// ---- steady-state columns, hand-scheduled -------------------------------------------
// Per column (q = running Q of this lane's row, p = boundary register whose lane 0 holds
// Q[x-1,y-1] of the row above the wave, v = logp[x,y]):
//   v_mov_b32_dpp p, q wave_shr:1     p[l] = q[l-1] (lane 0 keeps the boundary)
//   v_add_f32     ta, q, v            Q[x,y-1]   + v
//   v_cmp_lt_f32  vcc, q, p           direction bit: Q[x,y-1] < Q[x-1,y-1]   (core.pyx:34)
//   v_add_f32     tb, p, v            Q[x-1,y-1] + v
//   v_max_f32     q, ta, tb           == max(.,.) + v   (core.pyx:30)
//   v_addc_co_u32 d, vcc, d, d, vcc   d = 2*d + bit     (column j ends at bit 31-j)
//   ds_write_b32  ba, q offset        lane 63 -> boundary slot for wave w+1 (others: dummy)
// Wait states (gfx950): VALU write -> DPP read of q needs 2 (v_addc + ds_write sit between);
// VALU write of vcc -> VALU read as carry needs 2 (v_add + v_max sit between).  The leading
// s_nop 1 covers a compiler-generated VALU write of q directly in front of the statement.
#define MAS_COL(P, V, O)                                                        \
  "v_mov_b32_dpp " P ", %[q] wave_shr:1 row_mask:0xf bank_mask:0xf\n\t"        \
  "v_add_f32_e32 %[ta], %[q], " V "\n\t"                                        \
  "v_cmp_lt_f32_e32 vcc, %[q], " P "\n\t"                                       \
  "v_add_f32_e32 %[tb], " P ", " V "\n\t"                                       \
  "v_max_f32_e32 %[q], %[ta], %[tb]\n\t"                                        \
  "v_addc_co_u32_e32 %[d], vcc, %[d], %[d], vcc\n\t"                            \
  "ds_write_b32 %[ba], %[q] offset:" O "\n\t"

template <int J0>   // J0 = first column of the group inside the chunk (0,4,...,28)
__device__ __forceinline__ void mas_cols4(float& Q, unsigned& dir, float4& B, const float4& V, unsigned bout_addr)
{
  float ta, tb;
  asm volatile("s_nop 1\n\t"
               MAS_COL("%[p0]", "%[v0]", "%[o0]")
               MAS_COL("%[p1]", "%[v1]", "%[o1]")
               MAS_COL("%[p2]", "%[v2]", "%[o2]")
               MAS_COL("%[p3]", "%[v3]", "%[o3]")
               : [q] "+v"(Q), [d] "+v"(dir), [p0] "+v"(B.x), [p1] "+v"(B.y), [p2] "+v"(B.z), [p3] "+v"(B.w),
                 [ta] "=&v"(ta), [tb] "=&v"(tb)
               : [v0] "v"(V.x), [v1] "v"(V.y), [v2] "v"(V.z), [v3] "v"(V.w), [ba] "v"(bout_addr),
                 [o0] "i"((J0 + 1) * 4), [o1] "i"((J0 + 2) * 4), [o2] "i"((J0 + 3) * 4), [o3] "i"((J0 + 4) * 4)
               : "vcc", "memory");
}

// wave 0: the row above does not exist — lane 0 of the single register P stays max_neg_val
template <int J0>
__device__ __forceinline__ void mas_cols4_w0(float& Q, unsigned& dir, float& P, const float4& V, unsigned bout_addr)
{
  float ta, tb;
  asm volatile("s_nop 1\n\t"
               MAS_COL("%[p]", "%[v0]", "%[o0]")
               MAS_COL("%[p]", "%[v1]", "%[o1]")
               MAS_COL("%[p]", "%[v2]", "%[o2]")
               MAS_COL("%[p]", "%[v3]", "%[o3]")
               : [q] "+v"(Q), [d] "+v"(dir), [p] "+v"(P), [ta] "=&v"(ta), [tb] "=&v"(tb)
               : [v0] "v"(V.x), [v1] "v"(V.y), [v2] "v"(V.z), [v3] "v"(V.w), [ba] "v"(bout_addr),
                 [o0] "i"((J0 + 1) * 4), [o1] "i"((J0 + 2) * 4), [o2] "i"((J0 + 3) * 4), [o3] "i"((J0 + 4) * 4)
               : "vcc", "memory");
}

// A chunk that may contain the diagonal cell x==y of some lane (only chunks 2w, 2w+1 of wave
// w): plain HIP, core.pyx:19-20 handled with an explicit select.  V/B already in registers.
template <bool W0>
__device__ __forceinline__ void mas_chunk_diag(const float4 (&V)[8], const float4 (&B)[8], float* __restrict__ bout,
                                               int x, int c, float& Q, unsigned& dir_out)
{
  unsigned dir = 0;
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    const float vv[4] = {V[q].x, V[q].y, V[q].z, V[q].w};
    float bb[4] = {B[q].x, B[q].y, B[q].z, B[q].w};
    if (W0) { bb[0] = bb[1] = bb[2] = bb[3] = NEG; if (q == 0 && c == 0) bb[0] = 0.0f; }   // core.pyx:23-27
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int j = q * 4 + i;
      const float P = dpp_wave_shr1(bb[i], Q);                 // Q[x-1, y-1]
      const bool d = (x == c * CH + j);
      const float A = d ? NEG : Q;                             // core.pyx:19-20
      const bool lt = (A < P);                                 // core.pyx:34 predicate
      const float qa = A + vv[i];
      const float qp = P + vv[i];
      Q = (qp > qa) ? qp : qa;                                 // == max(A,P)+v bit-exactly
      dir = (dir << 1) | ((lt || d) ? 1u : 0u);
      bout[j + 1] = Q;
    }
  }
  dir_out = dir;
}

}  // namespace
