// What the MFMA attention kernels (attn_mfma.hip: T <= 384, attn_long.hip: 505 < T <= 4096) share: the head shape, the LDS
// pitches and the two fragment helpers.
#pragma once
#include "common.h"
#include "../../include/glowtts_hip.h"

namespace gt_attn_frag {

constexpr int HALO = GT_HALO;
constexpr int D = 96, WIN = 4, NW = 9;
constexpr int KP = 104;            // K / Ek pitch in halfs (208 B): conflict-free ds_read_b128 over 16 rows
constexpr int VP = 96;             // V pitch in halfs (192 B): conflict-free transposing reads
constexpr int BTP = 40;            // pitch (halfs) of the transposed band tables [16][32 + pad]

typedef __attribute__((__vector_size__(4 * sizeof(short)))) short s16x4_t;
typedef __attribute__((__vector_size__(8 * sizeof(short)))) short s16x8_t;

__device__ __forceinline__ bf16x8_t tr_frag8(const bf16_t* p0, const bf16_t* p1) {
  const s16x4_t lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4_t*)(uintptr_t)p0);
  const s16x4_t hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4_t*)(uintptr_t)p1);
  s16x8_t v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
  return __builtin_bit_cast(bf16x8_t, v);
}
__device__ __forceinline__ bf16x8_t pack8(const float* f) {
  const uint4 u = make_uint4(pack2bf(f[0], f[1]), pack2bf(f[2], f[3]), pack2bf(f[4], f[5]), pack2bf(f[6], f[7]));
  return __builtin_bit_cast(bf16x8_t, u);
}

}  // namespace gt_attn_frag
