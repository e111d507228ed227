// Cross-translation-unit helpers that are NOT part of the C-ABI (include/glowtts_hip.h).
#pragma once
#include <stdint.h>

static inline bool al16(const void* p) { return !((uintptr_t)p & 15); }   // NULL counts as aligned: optional pointers pass

// Dropout probability -> what the kernels take: keep an element when its 32-bit hash >= thresh = p * 2^32 (common.h drop_keep),
// then scale by 1 / (1 - p); p <= 0 is no dropout (0, 1).  oracle/dropmask.py restates this rule: every kernel must agree with it.
// p >= 1 is the caller's to refuse.
static inline void gt_drop_params(float p, uint32_t* thresh, float* scale)
{
  *thresh = 0; *scale = 1.0f;
  if (p > 0.0f) { *thresh = (uint32_t)((double)p * 4294967296.0); *scale = 1.0f / (1.0f - p); }
}

// MFMA attention forward for the configuration every reference config uses (D = 96, window 4) and
// T <= 256; returns 1 when the shape is not handled (caller falls back to the generic kernel).
int gt_attn_fwd_mfma_impl(const void* q, const void* k, const void* v, int ld, const float* Ek, const float* Ev,
                          const int32_t* lens, void* out, int ldo, float* P, int B, int T, int Tp, const int32_t* row0, int H, int Dh, int win,
                          uint32_t drop_thresh, uint32_t drop_seed, float drop_scale, const uint32_t* seed_dev, void* stream);

// MFMA attention backward (same shape limits).  ws: gt_attn_bwd_mfma_ws_bytes(B,T,H) bytes of scratch.
#include <stddef.h>
size_t gt_attn_bwd_mfma_ws_bytes(int B, int T, int H);
int gt_attn_bwd_mfma_impl(const void* q, const void* k, const void* v, int ld, const float* Ek, const float* Ev,
                          const int32_t* lens, const void* dout, int lddo, const float* P, void* ws, size_t ws_bytes,
                          void* dq, void* dk, void* dv, int lddq, float* dEk, float* dEv,
                          int B, int T, int Tp, const int32_t* row0, int H, int Dh, int win, uint32_t drop_thresh, uint32_t drop_seed, float drop_scale,
                          const uint32_t* seed_dev, void* stream);

// Key-tiled MFMA attention for 505 < T <= GT_ATTN_LONG_MAX_T (attn_long.hip, gt_attn_long_shape); same arguments, same workspace
// format and the same "returns 1 when the shape or the layout is not handled" as the two entries above.
int gt_attn_fwd_long_impl(const void* q, const void* k, const void* v, int ld, const float* Ek, const float* Ev,
                          const int32_t* lens, void* out, int ldo, float* P, int B, int T, int Tp, const int32_t* row0, int H, int Dh, int win,
                          uint32_t drop_thresh, uint32_t drop_seed, float drop_scale, const uint32_t* seed_dev, void* stream);
int gt_attn_bwd_long_impl(const void* q, const void* k, const void* v, int ld, const float* Ek, const float* Ev,
                          const int32_t* lens, const void* dout, int lddo, const float* P, void* ws, size_t ws_bytes,
                          void* dq, void* dk, void* dv, int lddq, float* dEk, float* dEv,
                          int B, int T, int Tp, const int32_t* row0, int H, int Dh, int win, uint32_t drop_thresh, uint32_t drop_seed, float drop_scale,
                          const uint32_t* seed_dev, void* stream);

// The P-free pair of the key-tiled family (gt_attn_fwd_stats / gt_attn_bwd_stats): the caller has checked gt_attn_long_shape and the
// workspace size (gt_attn_long_stats_ws_bytes); 1 = strides / operand alignment the kernels do not take.
size_t gt_attn_long_stats_ws_bytes(int B, int T, int H);
int gt_attn_fwd_long_stats_impl(const void* q, const void* k, const void* v, int ld, const float* Ek, const float* Ev,
                                const int32_t* lens, void* out, int ldo, float* stats, int B, int T, int Tp, const int32_t* row0, int H,
                                uint32_t drop_thresh, uint32_t drop_seed, float drop_scale, const uint32_t* seed_dev, void* stream);
int gt_attn_bwd_long_stats_impl(const void* q, const void* k, const void* v, int ld, const float* Ek, const float* Ev,
                                const int32_t* lens, const void* dout, int lddo, const float* stats, void* ws,
                                void* dq, void* dk, void* dv, int lddq, float* dEk, float* dEv,
                                int B, int T, int Tp, const int32_t* row0, int H, uint32_t drop_thresh, uint32_t drop_seed, float drop_scale,
                                const uint32_t* seed_dev, void* stream);

// The chip-wide kernel that writes the dense 0/1 path [B, T_x, T_y] (element type path_dtype, GT_DT_*) from the int32
// [B, T_x + 1] row start columns both MAS kernels leave in their workspace (mas.hip).  0 or GT_E_LAUNCH.
int gt_mas_expand_launch(const int32_t* starts, void* path, int path_dtype, int B, int T_x, int T_y, void* stream);
