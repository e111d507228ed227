"""CPU tests of the attention backward's host-side contract around T = 160, where the backward changes kernels: the shape predicate
and the workspace formula are host code and run without a GPU; no kernel is launched."""
import pytest


@pytest.mark.parametrize("T", [1, 160, 161])
def test_mfma_shape_and_workspace_around_the_one_workgroup_limit(built, T):
    from glow_tts_amd import _lib
    L = _lib.lib()
    assert L.gt_attn_mfma_shape(T, 96, 4) == 1
    assert L.gt_attn_mfma_shape(T, 64, 4) == 0 and L.gt_attn_mfma_shape(T, 96, 3) == 0
    B, H = 3, 2
    TI = -(-T // 32) * 32
    mfma = 2 * B * H * T * TI * 2                                     # bf16 dS^T [B,H,T,TI], then P'^T in the same shape
    generic = B * H * T * T * 4                                       # fp32 dS [B,H,T,T]
    assert L.gt_attn_bwd_workspace_bytes(B, T, H) == max(mfma, generic) + 256
