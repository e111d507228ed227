// What the MFMA kernels share: fragment loads from the packed weight images, bf16 pack / unpack of accumulator quads,
// accumulator zeroing and bench.py's begin / end stamps.
#pragma once
#include "common.h"

typedef uint32_t u32x4_t __attribute__((ext_vector_type(4)));

// fragment f of a weight image in MFMA-fragment order: 64 lanes x 16 bytes, one coalesced load per lane
__device__ __forceinline__ uint4 ldfrag(const bf16_t* __restrict__ W, int f, int lane)
{
  return *reinterpret_cast<const uint4*>(W + ((size_t)f * 64 + lane) * 8);
}
// The same through an explicit GLOBAL pointer: a pointer that went through an opaque asm (wn_stack.hip's `pinned`) is generic to
// the compiler, and flat loads count on lgkmcnt as well as vmcnt — every LDS wait would then drain the weight prefetch.
// The two loaders give different instruction streams; which one a kernel uses is part of its measured form.
__device__ __forceinline__ uint4 ldfrag_global(const bf16_t* __restrict__ W, int f, int lane)
{
  typedef const u32x4_t __attribute__((address_space(1)))* gptr_t;
  const u32x4_t v = *reinterpret_cast<gptr_t>(reinterpret_cast<uintptr_t>(W + ((size_t)f * 64 + lane) * 8));
  return make_uint4(v.x, v.y, v.z, v.w);
}
__device__ __forceinline__ bf16x8_t asfrag(const uint4& u) { return __builtin_bit_cast(bf16x8_t, u); }
__device__ __forceinline__ uint2 pack4(float a, float b, float c, float d) { return make_uint2(pack2bf(a, b), pack2bf(c, d)); }
__device__ __forceinline__ void unpack4(const uint2& u, float (&v)[4])
{
  v[0] = bf2f(u.x & 0xffff); v[1] = bf2f(u.x >> 16); v[2] = bf2f(u.y & 0xffff); v[3] = bf2f(u.y >> 16);
}

template <int N>
__device__ __forceinline__ void acc_zero(f32x16_t (&a)[N])
{
#pragma unroll
  for (int i = 0; i < N; ++i)
#pragma unroll
    for (int e = 0; e < 16; ++e) a[i][e] = 0.0f;
}
template <int N, int M>
__device__ __forceinline__ void acc_zero(f32x16_t (&a)[N][M])
{
#pragma unroll
  for (int i = 0; i < N; ++i)
#pragma unroll
    for (int j = 0; j < M; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) a[i][j][e] = 0.0f;
}

// bench.py's live timing of a kernel inside a captured graph: stamps[2*slot] = start, [2*slot+1] = max end, slot = stamp_slot +
// *stamp_base (a per-step device counter).  Workgroup 0's start (the first dispatched) is kept in a register and stored at the end,
// every workgroup's end goes into one atomicMax AFTER its last wait: an atomic at the kernel's start sits in front of every later
// wait for a load (vector-memory operations retire in order).
template <typename Args>
__device__ __forceinline__ unsigned long long stamp_begin(const Args& a)
{
  return (a.stamps && threadIdx.x == 0 && blockIdx.x == 0) ? (unsigned long long)wall_clock64() : 0ull;
}
template <typename Args>
__device__ __forceinline__ void stamp_end(const Args& a, unsigned long long t_begin)
{
  if (a.stamps && threadIdx.x == 0) {
    unsigned long long* slot = a.stamps + 2 * (a.stamp_slot + (a.stamp_base ? *a.stamp_base : 0));
    if (blockIdx.x == 0) slot[0] = t_begin;
    atomicMax(slot + 1, (unsigned long long)wall_clock64());
  }
}
