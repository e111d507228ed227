"""ctypes binding of libglowtts_hip.so (the C-ABI declared in include/glowtts_hip.h).

The library is the product: there is NO fallback.  `lib()` raises if it is missing or does
not export a declared symbol.  PyTorch is used by callers only for device memory and streams.
"""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("GT_LIB") or os.path.join(_HERE, "libglowtts_hip.so")     # GT_LIB: dev (an experiment build, tools/exp_variant.py)

c_void_p, c_int, c_i64, c_size_t, c_float, c_u32 = (ctypes.c_void_p, ctypes.c_int, ctypes.c_int64,
                                                    ctypes.c_size_t, ctypes.c_float, ctypes.c_uint32)


class Pointer(ctypes.c_void_p):
    """Pointer parameter of a C-ABI entry: a tensor (anything with data_ptr()) passes its address, a ctypes structure passes by
    reference, everything else (None, int, c_void_p, a byref result) is what c_void_p takes."""

    @classmethod
    def from_param(cls, v):
        if hasattr(v, "data_ptr"):
            v = v.data_ptr()
        elif isinstance(v, ctypes.Structure):
            return ctypes.byref(v)
        return ctypes.c_void_p.from_param(v)


STATUS = "status"      # restype marker: the entry returns 0 or a GT_E_* code (bound as c_int; `call` raises GtError on non-zero)
c_void_p = Pointer     # for the table only: the structures below keep the real c_void_p, so reading a field gives an int

# name -> (restype, argtypes); mirrors include/glowtts_hip.h one to one (tests/test_cabi.py compares it with the declarations)
PROTOTYPES = {
    "gt_version": (ctypes.c_char_p, []),
    "gt_mas_f32": (STATUS, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p,
                            c_int, c_int, c_int, c_i64, c_i64, c_void_p, c_size_t, c_void_p, c_void_p]),
    "gt_mas_lds_bytes": (c_size_t, [c_int, c_int]),
    "gt_mas_workspace_bytes": (c_size_t, [c_int, c_int, c_int]),
    "gt_mas_long_f32": (STATUS, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p,
                                 c_int, c_int, c_int, c_i64, c_i64, c_void_p, c_size_t, c_void_p, c_void_p]),
    "gt_mas_long_workspace_bytes": (c_size_t, [c_int, c_int, c_int]),
    "gt_mas_lengths_from_mask_f32": (STATUS, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int,
                                              c_i64, c_i64, c_void_p]),
    "gt_conv_gemm_bf16": (STATUS, [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_int, c_void_p,
                                   c_void_p, c_int, c_int, c_void_p, c_int, c_void_p, c_void_p, c_int,
                                   c_int, c_int, c_int, c_int, c_int, c_int, c_int,
                                   c_int, c_int, c_float, c_u32, c_void_p, c_void_p, c_int, c_int, c_void_p]),
    "gt_conv_wgrad_workspace_bytes": (c_size_t, [c_int, c_int, c_int, c_int, c_void_p]),
    "gt_conv_wgrad_ci_tile": (c_int, [c_int]),
    "gt_conv_wgrad_bf16": (STATUS, [c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p, c_size_t, c_void_p]),
    "gt_weightnorm_bwd": (STATUS, [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                   c_int, c_int, c_int, c_int, c_void_p]),
    "gt_conv_wgrad_batched": (STATUS, [c_void_p, c_void_p, c_int, c_int, c_int, c_void_p]),
    "gt_weightnorm_bwd_batched": (STATUS, [c_void_p, c_int, c_int, c_int, c_void_p]),
    "gt_conv_wgrad_paired": (STATUS, [c_void_p, c_void_p, c_int, c_int, c_void_p]),
    "gt_adamw_flat": (STATUS, [c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p, c_void_p, c_void_p]),
    "gt_colsum": (STATUS, [c_void_p, c_int, c_int, c_void_p, c_int, c_int, c_void_p]),
    "gt_squeeze_rows_f32": (STATUS, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p]),
    "gt_unsqueeze_rows_f32": (STATUS, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p]),
    "gt_flow_scalars": (STATUS, [c_void_p, c_int, c_void_p, c_void_p, c_void_p]),
    "gt_flow_scalars_multi": (STATUS, [c_void_p, c_void_p, c_int, c_void_p, c_int, c_void_p]),
    "gt_actnorm_ddi": (STATUS, [c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    "gt_actnorm_invconv_fwd": (STATUS, [c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p,
                                        c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p]),
    "gt_actnorm_invconv_bwd": (STATUS, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                        c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p]),
    "gt_actnorm_invconv_rev": (STATUS, [c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p]),
    "gt_coupling_rev": (STATUS, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p]),
    "gt_coupling_fwd": (STATUS, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_int, c_void_p]),
    "gt_coupling_bwd": (STATUS, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                 c_int, c_int, c_int, c_int, c_void_p, c_int, c_void_p]),
    "gt_gate_bwd": (STATUS, [c_void_p, c_int, c_void_p, c_void_p, c_int, c_void_p, c_int, c_void_p,
                             c_int, c_int, c_float, c_u32, c_void_p, c_void_p]),
    "gt_relu_drop_bwd": (STATUS, [c_void_p, c_int, c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_float, c_void_p]),
    "gt_rows_add_bf16": (STATUS, [c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_void_p]),
    "gt_rows_f32_to_bf16": (STATUS, [c_void_p, c_int, c_void_p, c_int, c_void_p, c_int, c_int, c_void_p]),
    "gt_layernorm_fwd": (STATUS, [c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int,
                                  c_void_p, c_void_p, c_int, c_int, c_float, c_float, c_u32, c_float, c_u32, c_int, c_void_p, c_void_p]),
    "gt_layernorm_bwd": (STATUS, [c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int,
                                  c_float, c_float, c_u32, c_float, c_u32, c_int, c_void_p, c_void_p, c_void_p, c_int,
                                  c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p]),
    "gt_layernorm_bwd_partial_rows": (c_int, [c_int]),
    "gt_layernorm_bwd_partials": (STATUS, [c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int,
                                           c_float, c_float, c_u32, c_float, c_u32, c_int, c_void_p, c_void_p, c_void_p, c_int,
                                           c_void_p, c_void_p, c_int, c_void_p, c_void_p]),
    "gt_param_partials_reduce": (STATUS, [c_void_p, c_void_p]),
    "gt_dds_bwd_partial_rows": (c_int, [c_int]),
    "gt_attn_fwd": (STATUS, [c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p,
                             c_int, c_int, c_int, c_void_p, c_int, c_int, c_int, c_float, c_u32, c_void_p, c_void_p]),
    "gt_attn_bwd_workspace_bytes": (c_size_t, [c_int, c_int, c_int]),
    "gt_attn_mfma_shape": (c_int, [c_int, c_int, c_int]),
    "gt_attn_long_shape": (c_int, [c_int, c_int, c_int]),
    "gt_attn_bwd": (STATUS, [c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p,
                             c_void_p, c_size_t, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p,
                             c_int, c_int, c_int, c_void_p, c_int, c_int, c_int, c_float, c_u32, c_void_p, c_void_p]),
    "gt_attn_stats_bytes": (c_size_t, [c_int, c_int, c_int]),
    "gt_attn_bwd_stats_workspace_bytes": (c_size_t, [c_int, c_int, c_int]),
    "gt_attn_fwd_stats": (STATUS, [c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p,
                                   c_int, c_int, c_int, c_void_p, c_int, c_int, c_int, c_float, c_u32, c_void_p, c_void_p]),
    "gt_attn_bwd_stats": (STATUS, [c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p,
                                   c_void_p, c_size_t, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p,
                                   c_int, c_int, c_int, c_void_p, c_int, c_int, c_int, c_float, c_u32, c_void_p, c_void_p]),
    "gt_embedding_fwd": (STATUS, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_int, c_int, c_int, c_float, c_void_p]),
    "gt_embedding_bwd": (STATUS, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_int, c_int, c_int, c_float, c_void_p]),
    "gt_rows_add_cond": (STATUS, [c_void_p, c_int, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_int,
                                  c_int, c_int, c_int, c_int, c_void_p, c_void_p]),
    "gt_rows_ctx_fill": (STATUS, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p]),
    "gt_step_inputs": (STATUS, [c_void_p, c_void_p]),
    "gt_step_zero": (STATUS, [c_void_p, c_void_p]),
    "gt_rows_utt_sum": (STATUS, [c_void_p, c_int, c_int, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p]),
    "gt_logp_f32": (STATUS, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p]),
    "gt_prior_expand": (STATUS, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p]),
    "gt_rows_from_bct": (STATUS, [c_void_p, c_int, c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p]),
    "gt_bct_from_rows": (STATUS, [c_void_p, c_int, c_void_p, c_int, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p]),
    "gt_mle_finish": (STATUS, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p]),
    "gt_duration_loss_fwd": (STATUS, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p]),
    "gt_duration_loss_bwd": (STATUS, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p]),
    "gt_align_loss_fwd": (STATUS, [c_void_p] * 11 + [c_int, c_int, c_int, c_int, c_void_p]),
    "gt_align_loss_finish": (STATUS, [c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_int, c_int, c_void_p, c_void_p]),
    "gt_align_loss_bwd": (STATUS, [c_void_p] * 14 + [c_int, c_int, c_int, c_int, c_void_p]),
    "gt_prior_expand_bwd": (STATUS, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p]),
    "gt_mle_sums": (STATUS, [c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "gt_mle_bwd": (STATUS, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p, c_void_p, c_int, c_void_p]),
    "gt_mark": (STATUS, [c_void_p, c_void_p]),
    "gt_length_mask": (STATUS, [c_void_p, c_int, c_void_p, c_int, c_int, c_void_p]),
    "gt_wn_layer_fwd": (STATUS, [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_int, c_int, c_void_p,
                                 c_void_p, c_int, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_int,
                                 c_int, c_int, c_int, c_float, c_u32, c_void_p, c_void_p, c_int, c_void_p, c_void_p]),
    "gt_wn_layer_bwd": (STATUS, [c_void_p, c_int, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_int, c_void_p,
                                 c_void_p, c_int, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_float, c_u32,
                                 c_void_p, c_void_p, c_int, c_void_p, c_void_p]),
    "gt_wn_stack_fwd": (STATUS, [c_void_p, c_void_p]),
    "gt_wn_stack_rows_per_workgroup": (c_int, [c_int]),
    "gt_wn_stack_row_blocks": (c_int, [c_int, c_int, c_int]),
    "gt_cond_affine_grads": (STATUS, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p]),
    "gt_wn_stack_bwd": (STATUS, [c_void_p, c_void_p]),
    "gt_wn_boundary_fwd": (STATUS, [c_void_p, c_void_p]),
    "gt_wn_boundary_bwd": (STATUS, [c_void_p, c_void_p]),
    "gt_boundary_param_partials": (c_int, []),
    "gt_wn_boundary_rev": (STATUS, [c_void_p, c_void_p]),
    "gt_boundary_rev_args_size": (c_int, []),
    "gt_boundary_param_reduce": (STATUS, [c_void_p, c_int, c_int, c_void_p, c_void_p]),
    "gt_rows_split3": (STATUS, [c_void_p, c_int, c_int, c_void_p, c_int, c_void_p, c_int, c_int, c_void_p]),
    "gt_dds_sep_fwd": (STATUS, [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_float, c_void_p]),
    "gt_dds_out_fwd": (STATUS, [c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_float, c_float, c_u32, c_void_p, c_void_p]),
    "gt_dds_out_bwd": (STATUS, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_float, c_float, c_u32, c_void_p, c_void_p]),
    "gt_dds_sep_bwd": (STATUS, [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                c_void_p, c_int, c_int, c_int, c_float, c_void_p]),
    "gt_dds_dw_bwd": (STATUS, [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p]),
    "gt_dds_layer_tile_rows": (c_int, []),
    "gt_dds_layer_partial_rows": (c_int, [c_int]),
    "gt_dds_layer_fwd": (STATUS, [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p,
                                  c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_float, c_float,
                                  c_u32, c_void_p, c_void_p]),
    "gt_dds_layer_bwd": (STATUS, [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p,
                                  c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                  c_void_p, c_int, c_int, c_int, c_float, c_float, c_u32, c_void_p, c_void_p]),
    "gt_convflow_pre_fwd": (STATUS, [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p]),
    "gt_convflow_pre_bwd": (STATUS, [c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_int, c_int, c_void_p]),
    "gt_convflow_spline_fwd": (STATUS, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_float, c_int, c_int, c_int, c_void_p]),
    "gt_convflow_spline_bwd": (STATUS, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                        c_void_p, c_void_p, c_float, c_int, c_int, c_int, c_void_p]),
    "gt_convflow_spline_partial_rows": (c_int, [c_int]),
    "gt_convflow_spline_partial_width": (c_int, []),
    "gt_convflow_spline_inv": (STATUS, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p]),
    "gt_ea_fwd": (STATUS, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_float, c_int, c_int, c_void_p]),
    "gt_ea_bwd": (STATUS, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_float, c_int, c_void_p]),
    "gt_sdp_mid_fwd": (STATUS, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p]),
    "gt_sdp_mid_bwd": (STATUS, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p]),
    "gt_nll_gauss_fwd": (STATUS, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p]),
    "gt_nll_gauss_bwd": (STATUS, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p]),
    "gt_rows_gather_tokens": (STATUS, [c_void_p, c_int, c_void_p, c_int, c_void_p, c_int, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_int, c_int, c_void_p]),
    "gt_pack_conv_weights_multi": (STATUS, [c_void_p, c_int, c_int, c_int, c_void_p]),
    "gt_pack_conv_weights": (STATUS, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int,
                                      c_int, c_int, c_int, c_int, c_int, c_void_p]),
    "gt_synth_lengths": (STATUS, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p]),
    "gt_synth_prior": (STATUS, [c_void_p, c_void_p]),
    "gt_synth_lengths_long": (STATUS, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p]),
    "gt_synth_prior_long": (STATUS, [c_void_p, c_void_p]),
    "gt_synth_prior_args_size": (c_int, []),
    "gt_randn_rows": (STATUS, [c_void_p, c_int, c_int, c_u32, c_u32, c_float, c_void_p]),
    "gt_synth_call_size": (c_int, []),
    "gt_synth_geometry": (STATUS, [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                   c_void_p, c_void_p]),
    "gt_synth_prior_call": (STATUS, [c_void_p, c_void_p, c_void_p]),
    "gt_synth_prior_long_call": (STATUS, [c_void_p, c_void_p, c_void_p]),
    "gt_randn_rows_call": (STATUS, [c_void_p, c_int, c_int, c_void_p, c_u32, c_int, c_void_p]),
    "gt_synth_call_ext_size": (c_int, []),
    "gt_randn_keyed": (STATUS, [c_void_p, c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_u32, c_u32, c_float, c_void_p]),
    "gt_randn_keyed_call": (STATUS, [c_void_p, c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_void_p, c_u32, c_int, c_void_p]),
    "gt_synth_frame_geometry": (STATUS, [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                         c_void_p, c_void_p]),
    "gt_synth_contours": (STATUS, [c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_int, c_void_p, c_int, c_void_p, c_int, c_void_p,
                                   c_void_p, c_void_p, c_void_p, c_int, c_int, c_float, c_float, c_void_p]),
    "gt_synth_contours_call": (STATUS, [c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_int, c_void_p, c_int, c_void_p, c_int, c_void_p,
                                        c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p]),
    "gt_mel_pack_bytes": (c_size_t, []),
    "gt_mel_tile_frames": (c_int, []),
    "gt_mel_pack": (STATUS, [c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p]),
    "gt_mel_spectrogram": (STATUS, [c_void_p, c_int, c_int, c_void_p, c_int, c_int, c_void_p, c_int, c_int, c_int, c_int, c_float,
                                    c_void_p, c_void_p, c_void_p, c_void_p]),
    "gt_yin_tile_frames": (c_int, []),
    "gt_yin_f0": (STATUS, [c_void_p, c_int, c_int, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_float, c_float, c_int,
                           c_void_p, c_void_p, c_void_p, c_void_p]),
    "gt_gl_pack_bytes": (c_size_t, []),
    "gt_gl_tile_frames": (c_int, []),
    "gt_gl_tile_hops": (c_int, []),
    "gt_gl_spec_bytes": (c_size_t, [c_int, c_int]),
    "gt_gl_pack": (STATUS, [c_void_p, c_int, c_void_p, c_void_p]),
    "gt_gl_polar": (STATUS, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p]),
    "gt_gl_project": (STATUS, [c_void_p, c_int, c_void_p, c_void_p, c_int, c_int, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p]),
    "gt_istft": (STATUS, [c_void_p, c_void_p, c_int, c_int, c_void_p, c_int, c_int, c_int, c_void_p, c_int, c_void_p]),
    "gt_gl_from_mel": (STATUS, [c_void_p, c_i64, c_i64, c_void_p, c_int, c_int, c_int, c_void_p, c_u32, c_void_p, c_void_p, c_void_p, c_void_p]),
    "gt_resample_tile_out": (c_int, []),
    "gt_resample_taps": (c_int, [c_int, c_int]),
    "gt_resample_lds_bytes": (c_size_t, [c_int, c_int]),
    "gt_resample": (STATUS, [c_void_p, c_int, c_int, c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_void_p, c_int, c_void_p, c_void_p]),
    "gt_voc_conv": (STATUS, [c_void_p, c_void_p]),
    "gt_voc_conv_args_size": (c_int, []),
    "gt_voc_tile_positions": (c_int, []),
    "gt_voc_k_chunk": (c_int, [c_int]),
    "gt_voc_lds_bytes": (c_size_t, [c_int, c_int, c_int]),
    "gt_voc_snake": (STATUS, [c_void_p, c_void_p]),
    "gt_voc_snake_args_size": (c_int, []),
    "gt_voc_snake_tile_positions": (c_int, []),
    "gt_vocos_norm": (STATUS, [c_void_p, c_void_p]),
    "gt_vocos_norm_args_size": (c_int, []),
    "gt_vocos_norm_tile_positions": (c_int, []),
    "gt_vocos_mlp": (STATUS, [c_void_p, c_void_p]),
    "gt_vocos_mlp_args_size": (c_int, []),
    "gt_vocos_tile_positions": (c_int, []),
    "gt_vocos_hidden_chunk": (c_int, []),
    "gt_vocos_mlp_lds_bytes": (c_size_t, [c_int]),
    "gt_vocos_polar": (STATUS, [c_void_p, c_void_p]),
    "gt_vocos_polar_args_size": (c_int, []),
    "gt_dtw_lds_bytes": (c_size_t, [c_int, c_int]),
    "gt_dtw_workspace_bytes": (c_size_t, [c_int, c_int, c_int]),
    "gt_mel_cepstrum": (STATUS, [c_void_p, c_int, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p]),
    "gt_dtw_f32": (STATUS, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_float, c_void_p, c_void_p, c_void_p, c_int,
                            c_void_p, c_size_t, c_void_p, c_void_p]),
    "gt_dtw_f0_stats": (STATUS, [c_void_p, c_int, c_void_p, c_void_p, c_int, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    "gt_wg_gate": (STATUS, [c_void_p, c_void_p]),
    "gt_wg_gate_args_size": (c_int, []),
    "gt_wg_tile_positions": (c_int, []),
    "gt_wg_gate_lds_bytes": (c_size_t, [c_int, c_int, c_int]),
    "gt_wg_boundary": (STATUS, [c_void_p, c_void_p]),
    "gt_wg_boundary_args_size": (c_int, []),
    "gt_denoise_spec": (STATUS, [c_void_p, c_void_p]),
    "gt_denoise_spec_args_size": (c_int, []),
    "gt_loudness_measure": (STATUS, [c_void_p, c_void_p]),
    "gt_loudness_apply": (STATUS, [c_void_p, c_void_p]),
    "gt_loudness_args_size": (c_int, []),
    "gt_loudness_chunk": (c_int, [c_int]),
    "gt_loudness_ws_bytes": (c_size_t, [c_int, c_int, c_int]),
}
c_void_p = ctypes.c_void_p


class PackDesc(ctypes.Structure):
    """struct gt_pack_desc (include/glowtts_hip.h)"""
    _fields_ = [("v", c_void_p), ("g", c_void_p), ("pack_fwd", c_void_p), ("pack_dgrad", c_void_p), ("inv_norm", c_void_p),
                ("Cout", ctypes.c_int32), ("Cin", ctypes.c_int32), ("taps", ctypes.c_int32), ("Np_fwd", ctypes.c_int32),
                ("Kp_fwd", ctypes.c_int32), ("Np_dgrad", ctypes.c_int32), ("Kp_dgrad", ctypes.c_int32), ("gate", ctypes.c_int32),
                ("row_start", ctypes.c_int32), ("pad_", ctypes.c_int32)]


class StepCopy(ctypes.Structure):
    """struct gt_step_copy (include/glowtts_hip.h)"""
    _fields_ = [("src", c_void_p), ("dst", c_void_p), ("rows", ctypes.c_int32), ("src_words", ctypes.c_int32),
                ("dst_words", ctypes.c_int32), ("blk0", ctypes.c_int32)]


class StepCtx(ctypes.Structure):
    """struct gt_step_ctx (include/glowtts_hip.h)"""
    _fields_ = [("geo_src", c_void_p), ("geo_dst", c_void_p), ("rowbatch", c_void_p), ("rowframe", c_void_p), ("rowmask", c_void_p),
                ("rowutt", c_void_p), ("B", ctypes.c_int32), ("R", ctypes.c_int32), ("blk0", ctypes.c_int32), ("pad_", ctypes.c_int32)]


STEP_MAX_COPIES, STEP_MAX_CTX, STEP_MAX_B = 10, 3, 1024
MLE_PARTS = 2048                                 # GT_MLE_PARTS: partial pairs gt_mle_sums writes (tests/test_loss64.py compares it with the header)
SYNTH_MAX_TX, SYNTH_LONG_MAX_TX = 512, 4096      # tokens gt_synth_lengths / gt_synth_prior[_call] take, and their *_long forms (GT_SYNTH_LONG_MAX_TX)


class StepInputsArgs(ctypes.Structure):
    """struct gt_step_inputs_args (include/glowtts_hip.h)"""
    _fields_ = [("copy", StepCopy * STEP_MAX_COPIES), ("ctx", StepCtx * STEP_MAX_CTX), ("n_copy", ctypes.c_int32), ("n_ctx", ctypes.c_int32)]


class PartialsJob(ctypes.Structure):
    """struct gt_partials_job (include/glowtts_hip.h)"""
    _fields_ = [("partials", c_void_p), ("dst_a", c_void_p), ("dst_b", c_void_p), ("n_rows", ctypes.c_int32), ("Ca", ctypes.c_int32),
                ("Cb", ctypes.c_int32), ("pad_", ctypes.c_int32)]


PARTIALS_MAX = 32


class PartialsArgs(ctypes.Structure):
    """struct gt_partials_args (include/glowtts_hip.h)"""
    _fields_ = [("job", PartialsJob * PARTIALS_MAX), ("n_jobs", ctypes.c_int32)]


ZERO_MAX = 4


class StepZeroArgs(ctypes.Structure):
    """struct gt_step_zero_args (include/glowtts_hip.h)"""
    _fields_ = [("ptr", c_void_p * ZERO_MAX), ("bytes", ctypes.c_uint64 * ZERO_MAX), ("seed_word", c_void_p), ("seed_inc", ctypes.c_uint32),
                ("n", ctypes.c_int32)]


class WnStackFwdArgs(ctypes.Structure):
    """struct gt_wn_stack_fwd_args (include/glowtts_hip.h)"""
    _fields_ = [("x0", c_void_p), ("w_in", c_void_p * 4), ("b_in", c_void_p * 4), ("w_res", c_void_p * 4), ("b_res", c_void_p * 4),
                ("cond", c_void_p), ("ldc", c_int), ("row0", c_void_p), ("B", c_int), ("Tp", c_int), ("rowmask", c_void_p),
                ("acts", c_void_p), ("ldacts", c_int), ("gate_t", c_void_p * 4), ("gate_s", c_void_p * 4), ("x_out", c_void_p * 4),
                ("R", c_int), ("H", c_int), ("taps", c_int), ("n_layers", c_int), ("drop_p", c_float), ("drop_seed", c_u32),
                ("seed_dev", c_void_p), ("stamps", c_void_p), ("stamp_slot", c_int), ("stamp_base", c_void_p),
                ("aff_w", c_void_p), ("aff_b", c_void_p), ("aff_sig", c_void_p)]


class WnStackBwdArgs(ctypes.Structure):
    """struct gt_wn_stack_bwd_args (include/glowtts_hip.h)"""
    _fields_ = [("via_skip", c_void_p), ("ldvs", c_int), ("gate_t", c_void_p * 4), ("gate_s", c_void_p * 4), ("w_in_d", c_void_p * 4),
                ("w_res_d", c_void_p * 4), ("rowmask", c_void_p), ("dpre", c_void_p * 4), ("dpre_c", c_void_p * 4), ("dx", c_void_p * 4),
                ("R", c_int), ("H", c_int), ("taps", c_int), ("n_layers", c_int), ("drop_p", c_float), ("drop_seed", c_u32),
                ("seed_dev", c_void_p)]


class BoundaryFwdArgs(ctypes.Structure):
    """struct gt_boundary_fwd_args (include/glowtts_hip.h); pointer fields take tensor.data_ptr() or None"""
    _fields_ = [("acts", c_void_p), ("ldacts", c_int), ("w_skip", c_void_p), ("b_skip", c_void_p),
                ("w_end", c_void_p), ("b_end", c_void_p), ("ks_end", c_int), ("y", c_void_p), ("wn_out", c_void_p),
                ("logs_raw", c_void_p), ("z", c_void_p), ("logdet", c_void_p), ("rowutt", c_void_p), ("sigmoid_scale", c_int),
                ("x_in", c_void_p), ("an_logs", c_void_p), ("an_bias", c_void_p), ("w_ic", c_void_p), ("scal", c_void_p),
                ("len", c_void_p), ("B", c_int), ("y_next", c_void_p), ("y0_bf16", c_void_p), ("w_start", c_void_p),
                ("b_start", c_void_p), ("ks_start", c_int), ("h_next", c_void_p), ("rowmask", c_void_p),
                ("R", c_int), ("H", c_int), ("C", c_int), ("n_layers", c_int),
                ("y_bct", c_void_p), ("z_bct", c_void_p), ("T", c_int), ("rowbatch", c_void_p), ("rowframe", c_void_p),
                ("pf_ptr", c_void_p * 16), ("pf_bytes", c_u32 * 16)]


class BoundaryBwdArgs(ctypes.Structure):
    """struct gt_boundary_bwd_args (include/glowtts_hip.h)"""
    _fields_ = [("dh", c_void_p), ("w_start_d", c_void_p), ("ks_start_d", c_int), ("dx_in", c_void_p), ("x", c_void_p),
                ("an_logs", c_void_p), ("an_bias", c_void_p), ("w_ic", c_void_p), ("scal", c_void_p), ("len", c_void_p), ("B", c_int),
                ("d_an_logs", c_void_p), ("d_an_bias", c_void_p), ("d_w_ic", c_void_p),
                ("dz_in", c_void_p), ("logs_raw", c_void_p), ("y", c_void_p), ("dlogdet", c_void_p), ("rowutt", c_void_p),
                ("sigmoid_scale", c_int), ("dx_out", c_void_p), ("dout", c_void_p), ("w_end_d", c_void_p), ("ks_end_d", c_int),
                ("dwn_out", c_void_p), ("w_skip_d", c_void_p), ("ks_skip_d", c_int), ("via_skip", c_void_p), ("ldvs", c_int),
                ("rowmask", c_void_p), ("R", c_int), ("H", c_int), ("C", c_int), ("n_layers", c_int),
                ("dz_bct", c_void_p), ("dx_bct", c_void_p), ("T", c_int), ("rowbatch", c_void_p), ("rowframe", c_void_p),
                ("pg_partial", c_void_p), ("pf_ptr", c_void_p * 16), ("pf_bytes", c_u32 * 16)]


class BoundaryRevArgs(ctypes.Structure):
    """struct gt_boundary_rev_args (include/glowtts_hip.h); its size is checked against gt_boundary_rev_args_size() (tests/test_synthesis_cabi.py)"""
    _fields_ = [("acts", c_void_p), ("ldacts", c_int), ("w_skip", c_void_p), ("b_skip", c_void_p),
                ("w_end", c_void_p), ("b_end", c_void_p), ("ks_end", c_int), ("z", c_void_p), ("sigmoid_scale", c_int),
                ("an_logs", c_void_p), ("an_bias", c_void_p), ("scal", c_void_p), ("x", c_void_p),
                ("x_in", c_void_p), ("w_start", c_void_p), ("b_start", c_void_p), ("ks_start", c_int), ("h_next", c_void_p),
                ("rowmask", c_void_p), ("R", c_int), ("H", c_int), ("C", c_int), ("n_layers", c_int),
                ("z_bct", c_void_p), ("x_bct", c_void_p), ("T", c_int), ("rowbatch", c_void_p), ("rowframe", c_void_p), ("len", c_void_p),
                ("pf_ptr", c_void_p * 16), ("pf_bytes", c_u32 * 16)]


class SynthPriorArgs(ctypes.Structure):
    """struct gt_synth_prior_args (include/glowtts_hip.h); its size is checked against gt_synth_prior_args_size() (tests/test_synthesis_noise.py)"""
    _fields_ = [("x_m", c_void_p), ("x_logs", c_void_p), ("cum", c_void_p), ("x_len", c_void_p), ("y_len", c_void_p),
                ("row0", c_void_p), ("Tp", c_int), ("R", c_int), ("rows", c_void_p), ("z_m", c_void_p), ("z_logs", c_void_p),
                ("frame2token", c_void_p), ("attn", c_void_p), ("B", c_int), ("C", c_int), ("Tx", c_int), ("Ty", c_int),
                ("seed", c_u32), ("noise_scale", c_float)]


class SynthCall(ctypes.Structure):
    """struct gt_synth_call (include/glowtts_hip.h): the scalars of one synthesis call, read from device memory; its size is checked
    against gt_synth_call_size() (tests/test_synthesis_graph_cabi.py)"""
    _fields_ = [("seed", c_u32), ("noise_scale", c_float), ("noise_scale_w", c_float), ("length_scale", c_float)]


class SynthCallExt(ctypes.Structure):
    """struct gt_synth_call_ext (include/glowtts_hip.h): gt_synth_call + the scalars of the pitch / energy predictors; its size is
    checked against gt_synth_call_ext_size() (tests/test_synth_prosody_cabi.py)"""
    _fields_ = [("base", SynthCall), ("f0_noise_scale", c_float), ("energy_noise_scale", c_float), ("pitch_scale", c_float),
                ("energy_scale", c_float)]


class VocConvArgs(ctypes.Structure):
    """struct gt_voc_conv_args (include/glowtts_hip.h); its size is checked against gt_voc_conv_args_size() (tests/test_hifigan_cabi.py)"""
    _fields_ = [("X", c_void_p), ("x_stride_b", c_i64), ("x_stride_c", c_i64), ("W", c_void_p), ("bias", c_void_p), ("res", c_void_p),
                ("acc", c_void_p), ("Y", c_void_p), ("y_stride_b", c_i64), ("ldy", c_int), ("len_mul", c_int), ("n_frames", c_void_p),
                ("B", c_int), ("L_cap", c_int), ("Cin", c_int), ("N", c_int), ("taps", c_int), ("dil", c_int),
                ("x_bf16", c_int), ("x_mel", c_int), ("y_bf16", c_int), ("tanh_out", c_int), ("slope", c_float), ("scale", c_float)]


class VocSnakeArgs(ctypes.Structure):
    """struct gt_voc_snake_args (include/glowtts_hip.h); its size is checked against gt_voc_snake_args_size() (tests/test_voc_snake_cabi.py)"""
    _fields_ = [("X", c_void_p), ("x_stride_b", c_i64), ("P", c_void_p), ("Y", c_void_p), ("y_stride_b", c_i64), ("len_mul", c_int),
                ("n_frames", c_void_p), ("B", c_int), ("L_cap", c_int), ("C", c_int)]


class VocosNormArgs(ctypes.Structure):
    """struct gt_vocos_norm_args (include/glowtts_hip.h); its size is checked against gt_vocos_norm_args_size() (tests/test_vocos_cabi.py)"""
    _fields_ = [("X", c_void_p), ("x_stride_b", c_i64), ("wd", c_void_p), ("bd", c_void_p), ("g", c_void_p), ("be", c_void_p),
                ("Y", c_void_p), ("y_stride_b", c_i64), ("n_frames", c_void_p), ("B", c_int), ("L_cap", c_int), ("C", c_int),
                ("y_bf16", c_int), ("eps", c_float)]


class VocosMlpArgs(ctypes.Structure):
    """struct gt_vocos_mlp_args (include/glowtts_hip.h); its size is checked against gt_vocos_mlp_args_size() (tests/test_vocos_cabi.py)"""
    _fields_ = [("A", c_void_p), ("a_stride_b", c_i64), ("W1", c_void_p), ("b1", c_void_p), ("W2", c_void_p), ("b2", c_void_p),
                ("R", c_void_p), ("r_stride_b", c_i64), ("Y", c_void_p), ("y_stride_b", c_i64), ("U", c_void_p), ("u_stride_b", c_i64),
                ("n_frames", c_void_p), ("B", c_int), ("L_cap", c_int), ("C", c_int), ("H", c_int)]


class VocosPolarArgs(ctypes.Structure):
    """struct gt_vocos_polar_args (include/glowtts_hip.h); its size is checked against gt_vocos_polar_args_size() (tests/test_vocos_cabi.py)"""
    _fields_ = [("O", c_void_p), ("o_stride_b", c_i64), ("n_frames", c_void_p), ("spec", c_void_p), ("B", c_int), ("F_max", c_int),
                ("n_fft", c_int)]


class WgGateArgs(ctypes.Structure):
    """struct gt_wg_gate_args (include/glowtts_hip.h); its size is checked against gt_wg_gate_args_size() (tests/test_waveglow_cabi.py)"""
    _fields_ = [("X", c_void_p), ("x_stride_b", c_i64), ("ldx", c_int), ("Cs", c_int), ("S", c_void_p), ("s_stride_b", c_i64),
                ("W_in", c_void_p), ("W_cond", c_void_p), ("b_in", c_void_p), ("b_cond", c_void_p), ("G", c_void_p), ("g_stride_b", c_i64),
                ("len_mul", c_int), ("n_frames", c_void_p), ("B", c_int), ("L_cap", c_int), ("C", c_int), ("taps", c_int), ("dil", c_int)]


class WgBoundaryArgs(ctypes.Structure):
    """struct gt_wg_boundary_args (include/glowtts_hip.h); its size is checked against gt_wg_boundary_args_size() (tests/test_waveglow_cabi.py)"""
    _fields_ = [("state", c_void_p), ("st_stride_b", c_i64), ("ld", c_int), ("C", c_int), ("A", c_void_p), ("a_stride_b", c_i64),
                ("w_end", c_void_p), ("b_end", c_void_p), ("w_inv", c_void_p), ("w_start", c_void_p), ("b_start", c_void_p),
                ("n_frames", c_void_p), ("seed_dev", c_void_p), ("seed", c_u32), ("sigma", c_float), ("len_mul", c_int), ("B", c_int),
                ("L_cap", c_int), ("c_in", c_int), ("c_out", c_int)]


class DenoiseSpecArgs(ctypes.Structure):
    """struct gt_denoise_spec_args (include/glowtts_hip.h); its size is checked against gt_denoise_spec_args_size() (tests/test_denoise_cabi.py)"""
    _fields_ = [("wav", c_void_p), ("bias", c_void_p), ("strength", c_void_p), ("n_frames", c_void_p), ("mel_packed", c_void_p),
                ("spec", c_void_p), ("frames_out", c_void_p), ("ld_wav", c_int), ("lost", c_int), ("B", c_int), ("F_max", c_int),
                ("n_fft", c_int), ("hop", c_int), ("win", c_int)]


class LoudnessArgs(ctypes.Structure):
    """struct gt_loudness_args (include/glowtts_hip.h); its size is checked against gt_loudness_args_size() (tests/test_loudness_cabi.py)"""
    _fields_ = [("wav", c_void_p), ("n_frames", c_void_p), ("params", c_void_p), ("stats", c_void_p), ("ws", c_void_p), ("out", c_void_p),
                ("ws_bytes", c_i64), ("ld", c_int), ("ld_out", c_int), ("is_i16", c_int), ("hop", c_int), ("lost", c_int), ("B", c_int),
                ("L_cap", c_int), ("fs", c_int)]


LOUD_STATS, LOUD_PARAMS = 8, 64                  # GT_LOUD_STATS, GT_LOUD_PARAMS
WG_NOISE_STREAM, WG_MAX_C = 5, 512               # GT_WG_NOISE_STREAM, GT_WG_MAX_C


# mirror -> its C struct in include/glowtts_hip.h (tests/test_cabi.py compares every size and field offset with a C compiler's)
C_STRUCTS = {PackDesc: "gt_pack_desc", StepCopy: "gt_step_copy", StepCtx: "gt_step_ctx", StepInputsArgs: "gt_step_inputs_args",
             PartialsJob: "gt_partials_job", PartialsArgs: "gt_partials_args", StepZeroArgs: "gt_step_zero_args",
             WnStackFwdArgs: "gt_wn_stack_fwd_args", WnStackBwdArgs: "gt_wn_stack_bwd_args", BoundaryFwdArgs: "gt_boundary_fwd_args",
             BoundaryBwdArgs: "gt_boundary_bwd_args", BoundaryRevArgs: "gt_boundary_rev_args", SynthPriorArgs: "gt_synth_prior_args",
             SynthCall: "gt_synth_call", SynthCallExt: "gt_synth_call_ext", VocConvArgs: "gt_voc_conv_args",
             VocSnakeArgs: "gt_voc_snake_args", VocosNormArgs: "gt_vocos_norm_args", VocosMlpArgs: "gt_vocos_mlp_args",
             VocosPolarArgs: "gt_vocos_polar_args", WgGateArgs: "gt_wg_gate_args", WgBoundaryArgs: "gt_wg_boundary_args",
             DenoiseSpecArgs: "gt_denoise_spec_args", LoudnessArgs: "gt_loudness_args"}


def fill_args(cls, **kw):
    """ctypes struct from keyword arguments: tensors become device pointers, None stays NULL, ints stay ints."""
    a = cls()
    for k, v in kw.items():
        if isinstance(v, (list, tuple)):                  # pointer arrays: tensors / None per entry
            arr = getattr(a, k)
            for i, t in enumerate(v):
                arr[i] = None if t is None else (t.data_ptr() if hasattr(t, "data_ptr") else t)
        else:
            setattr(a, k, v.data_ptr() if hasattr(v, "data_ptr") else v)
    return a


GT_TILE_AUTO, GT_TILE_64x64, GT_TILE_64x128, GT_TILE_128x64, GT_TILE_128x128, GT_TILE_256x64, GT_TILE_64x64_TAPS = 0, 1, 2, 3, 4, 5, 6
GT_DT_F32, GT_DT_I32, GT_DT_F16, GT_DT_BF16, GT_DT_U8 = 0, 1, 2, 3, 4
GT_ERRORS = {-1: "GT_E_INVAL", -2: "GT_E_UNSUPPORTED", -3: "GT_E_ALIGN", -4: "GT_E_LAUNCH"}

_LIB = None


class HipLibraryMissing(RuntimeError):
    pass


def lib():
    """Load (once) and return the HIP library; raise loudly if it is not built.  The raw surface (with `check`, `ptr`,
    `current_stream`), for callers that inspect a status themselves: bench.py, the tests and tools/.  Product code uses `call`."""
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            raise HipLibraryMissing(
                f"{LIB_PATH} not found: the HIP extension is not built.  Run "
                "`python glow-tts_amd/build.py` (or __graft_entry__.build()).  There is no CPU fallback.")
        # PyTorch-ROCm ships its own libamdhip64: it must be in the process BEFORE our library is loaded,
        # otherwise the loader binds us to a second HIP runtime (/opt/rocm) that then reports
        # "no ROCm-capable device" next to torch's.
        import torch  # noqa: F401
        L = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in PROTOTYPES.items():
            try:
                fn = getattr(L, name)
            except AttributeError as e:
                raise HipLibraryMissing(f"{LIB_PATH} does not export {name}; rebuild it") from e
            fn.restype = c_int if res is STATUS else res
            fn.argtypes = args
        if os.environ.get("GT_TRACE_CALLS"):
            L = _Traced(L, os.environ["GT_TRACE_CALLS"])
        _LIB = L
    return _LIB


class _Traced:
    """dev (GT_TRACE_CALLS=<file>): the name of every C-ABI entry is written to the file BEFORE the call and the device is
    synchronised after it — after a GPU memory fault (which kills the process) the file names the launch that faulted."""

    def __init__(self, L, path):
        self._L, self._f, self._n = L, open(path, "w"), 0

    def __getattr__(self, name):
        fn = getattr(self._L, name)
        if not name.startswith("gt_"):
            return fn

        def call(*a):
            import torch
            self._n += 1
            self._f.seek(0); self._f.write(f"{self._n} {name}".ljust(96) + "\n"); self._f.flush()
            rc = fn(*a)
            if torch.cuda.is_available() and not torch.cuda.is_current_stream_capturing():
                torch.cuda.synchronize()
            self._f.seek(0); self._f.write(f"{self._n} {name} returned".ljust(96) + "\n"); self._f.flush()
            return rc
        return call


class _Recording:
    """the library with the name of every gt_* entry appended to `names` before the call (record_calls)"""

    def __init__(self, L, names):
        self._L, self._names = L, names

    def __getattr__(self, name):
        fn = getattr(self._L, name)
        if not name.startswith("gt_"):
            return fn

        def call(*a):
            self._names.append(name)
            return fn(*a)
        return call


class record_calls:
    """dev: `with _lib.record_calls() as names:` — the C-ABI entries called inside the block, in order (a test and tools/synth_bench.py
    count the launches of one pass with it).  Nothing is recorded, and nothing kept, outside such a block."""

    def __enter__(self):
        global _LIB
        self._prev, self.names = lib(), []
        _LIB = _Recording(self._prev, self.names)
        return self.names

    def __exit__(self, *exc):
        global _LIB
        _LIB = self._prev
        return False


class GtError(RuntimeError):
    """a C-ABI entry returned a GT_E_* status"""

    def __init__(self, entry, code):
        super().__init__(f"{entry} failed: {GT_ERRORS.get(code, code)}")
        self.entry, self.code = entry, code


class _Call:
    """`call.gt_x(a, b, ..., stream)`: the entry through lib() on every call (so record_calls and GT_TRACE_CALLS see it), tensors and
    structures passed as they are (Pointer); a status entry raises GtError on a non-zero return, a value entry returns its value."""

    def __getattr__(self, name):
        if name not in PROTOTYPES:
            raise AttributeError(f"{name} is not a C-ABI entry")
        status = PROTOTYPES[name][0] is STATUS

        def entry(*args):
            rc = getattr(lib(), name)(*args)
            if not status:
                return rc
            if rc != 0:
                raise GtError(name, rc)
        setattr(self, name, entry)
        return entry


call = _Call()


def check(rc, what):
    """raw surface: raise on a non-zero status of an entry called through lib()"""
    if rc != 0:
        raise GtError(what, rc)


def ptr(t):
    """raw surface: device pointer of a torch tensor (or None)."""
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def current_stream(device=None):
    """the device's current stream as the C-ABI's stream argument"""
    import torch
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


class CpuTensorError(RuntimeError, TypeError):
    """a CPU tensor where a device tensor is required: the wrong kind of argument (TypeError), raised as the RuntimeError callers of
    the first releases catch"""


def require_cuda(*tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise CpuTensorError("glow_tts_amd ops run on the MI355X only (got a CPU tensor); "
                               "there is no CPU fallback — use oracle/ for CPU checking in tests")
