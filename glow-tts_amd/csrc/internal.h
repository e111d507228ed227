// Cross-translation-unit helpers that are NOT part of the C-ABI (include/glowtts_hip.h).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "common.h"
#include "../../include/glowtts_hip.h"

static inline bool al16(const void* p) { return !((uintptr_t)p & 15); }   // NULL counts as aligned: optional pointers pass

// the batch and frame limits every entry point on the spectrum workspace shares (griffin_lim.hip, gl_mel.hip)
static inline bool gl_shape_bad(int B, int F_max) { return B <= 0 || B > GT_MEL_MAX_B || F_max <= 0 || F_max > GT_MEL_MAX_FRAMES; }

// Dropout probability -> what the kernels take: keep an element when its 32-bit hash >= thresh = p * 2^32 (common.h drop_keep),
// then scale by 1 / (1 - p); p <= 0 is no dropout (0, 1).  oracle/dropmask.py restates this rule: every kernel must agree with it.
// p >= 1 is the caller's to refuse.
static inline void gt_drop_params(float p, uint32_t* thresh, float* scale)
{
  *thresh = 0; *scale = 1.0f;
  if (p > 0.0f) { *thresh = (uint32_t)((double)p * 4294967296.0); *scale = 1.0f / (1.0f - p); }
}

// Raise a kernel's dynamic-LDS limit past the 64 KiB default, before its launch: once per kernel and process, the flag latched
// only after success.  0 or GT_E_LAUNCH.
template <auto Kernel>
int gt_allow_lds(int bytes)
{
  static bool done = false;
  if (!done) {
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize, bytes) != hipSuccess) return GT_E_LAUNCH;
    done = true;
  }
  return GT_OK;
}

// ---- attention: the host path under gt_attn_fwd / gt_attn_bwd / gt_attn_fwd_stats / gt_attn_bwd_stats (encoder_ops.hip) ----
// The seven kernel paths.  gt_attn_route is the ONLY place where T meets the thresholds between them.
enum gt_attn_path {
  GT_ATTN_NONE,         // T > GT_ATTN_LONG_MAX_T: no kernel takes it
  GT_ATTN_FUSED160,     // D = 96, win = 4, T <= 160: launch_fwd<5>, the one-workgroup fused backward          (attn_mfma.hip)
  GT_ATTN_MFMA256,      //                  161 .. 256: launch_fwd<8>, launch_bwd<8, 2>
  GT_ATTN_MFMA384,      //                  257 .. 384: launch_fwd_long<12>, launch_bwd<12, 4>
  GT_ATTN_GENERIC,      // 385 .. 505, or any other D / win: the VALU kernels of encoder_ops.hip, to what their LDS holds
  GT_ATTN_LONG_P,       // D = 96, win = 4, 506 .. GT_ATTN_LONG_MAX_T: key-tiled, P saved                      (attn_long.hip)
  GT_ATTN_LONG_NOP,     //   the same shapes, gt_attn_fwd with P == NULL: no P stored (synthesis)
  GT_ATTN_LONG_STATS,   //   the same shapes, gt_attn_fwd_stats / gt_attn_bwd_stats: row statistics, P recomputed
};
// One of NONE, FUSED160, MFMA256, MFMA384, GENERIC, LONG_P: what the entry was called with (a NULL P, the *_stats pair) turns
// LONG_P into the other two.
gt_attn_path gt_attn_route(int T, int D, int win);

static inline const bf16_t* gt_bf16(const void* p) { return static_cast<const bf16_t*>(p); }
static inline bf16_t* gt_bf16(void* p) { return static_cast<bf16_t*>(p); }

// What one attention call works on: filled once by the extern "C" entry after its NULL and limit checks, read by everything
// below it.  Host only (never a kernel parameter); a field a direction does not use stays 0.  P and stats serve both directions:
// the backward entries cast their const inputs in, nothing on the host writes through them, and the backward kernels take them
// as const float* again.
struct gt_attn_call {
  const bf16_t *q, *k, *v; int ld;                                // operands: windows of one rows buffer, pitch ld
  const float *Ek, *Ev; const int32_t* lens;
  bf16_t* out; int ldo;                                           // forward
  float* P;                                                       //   saved softmax (written forward, read backward), or NULL
  float* stats;                                                   //   [B, H, T, 2] row statistics of the P-free pair, likewise
  const bf16_t* dout; int lddo;                                   // backward
  bf16_t *dq, *dk, *dv; int lddq; float *dEk, *dEv;
  void* ws; size_t ws_bytes;
  int B, T, Tp; const int32_t* row0; int H, D, win;               // geometry
  uint32_t th, sd; float sc; const uint32_t* seed_dev;            // dropout: gt_drop_params' (thresh, scale), the seed, its device part
  hipStream_t stream;
};

// The layout every MFMA attention kernel needs, in either direction (unused fields are 0 and pass): 16-byte rows of q / k / v / dout,
// 8-byte rows of out / dq, 16-byte aligned operands and workspace, 8-byte aligned statistics.  A family that is handed another layout
// does not take the call; what happens then is the entry's business (encoder_ops.hip).
static inline bool gt_attn_mfma_layout(const gt_attn_call& c)
{
  if ((c.ld & 7) || (c.ldo & 3) || (c.lddo & 7) || (c.lddq & 3)) return false;
  return al16(c.q) && al16(c.k) && al16(c.v) && al16(c.dout) && al16(c.ws) && !((uintptr_t)c.stats & 7);
}

// attn_mfma.hip: path is FUSED160, MFMA256 or MFMA384, the layout gt_attn_mfma_layout's.  The backward's workspace, and the key-tiled
// saved-P backward's: gt_attn_bwd_mfma_ws_bytes(B, T, H) bytes, bf16 dS^T | P'^T, [B, H, T, TI] each (query index contiguous, padded).
size_t gt_attn_bwd_mfma_ws_bytes(int B, int T, int H);
struct gt_attn_bwd_ws {
  int TI; bf16_t *dST, *PdT;
  explicit gt_attn_bwd_ws(const gt_attn_call& c) : TI(((c.T + 31) / 32) * 32), dST(static_cast<bf16_t*>(c.ws)), PdT(dST + (size_t)c.B * c.H * c.T * TI) {}
};
int gt_attn_fwd_mfma_impl(const gt_attn_call& c, gt_attn_path path);
int gt_attn_bwd_mfma_impl(const gt_attn_call& c, gt_attn_path path);

// attn_long.hip: path is LONG_P, LONG_NOP (forward only) or LONG_STATS, the layout gt_attn_mfma_layout's.  The P-free backward's
// workspace is gt_attn_long_stats_ws_bytes(B, T, H) bytes.
size_t gt_attn_long_stats_ws_bytes(int B, int T, int H);
int gt_attn_fwd_long_impl(const gt_attn_call& c, gt_attn_path path);
int gt_attn_bwd_long_impl(const gt_attn_call& c, gt_attn_path path);

// The chip-wide kernel that writes the dense 0/1 path [B, T_x, T_y] (element type path_dtype, GT_DT_*) from the int32
// [B, T_x + 1] row start columns both MAS kernels leave in their workspace (mas.hip).  0 or GT_E_LAUNCH.
int gt_mas_expand_launch(const int32_t* starts, void* path, int path_dtype, int B, int T_x, int T_y, void* stream);
