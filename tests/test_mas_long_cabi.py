"""CPU tests of the long-lattice MAS entry (gt_mas_long_f32, csrc/mas_long.hip): the argument checks and the workspace
formula are host code and run without a GPU; no kernel is launched."""
import pytest
import torch

FAKE = 0x1000           # a non-null, 16-byte aligned address that is never dereferenced: every case below returns before a launch


def _call(L, logp=FAKE, t_x=FAKE, t_y=FAKE, B=2, T_x=600, T_y=700, stride_b=None, stride_x=None, ws=FAKE, ws_bytes=None):
    stride_x = T_y if stride_x is None else stride_x
    stride_b = T_x * stride_x if stride_b is None else stride_b
    if ws_bytes is None:
        ws_bytes = L.gt_mas_long_workspace_bytes(B, T_x, T_y)
    return L.gt_mas_long_f32(logp, None, t_x, t_y, None, 0, None, None, B, T_x, T_y, stride_b, stride_x, ws, ws_bytes, None, None)


def test_argument_checks_come_before_any_launch(built):
    from glow_tts_amd import _lib
    L = _lib.lib()
    assert _call(L, logp=None) == -1 and _call(L, t_x=None) == -1 and _call(L, t_y=None) == -1 and _call(L, ws=None) == -1
    assert _call(L, B=0) == 0
    assert _call(L, B=-1) == -1 and _call(L, T_x=-1, stride_b=1, stride_x=1) == -1 and _call(L, T_y=-1, stride_b=1, stride_x=1) == -1
    need = L.gt_mas_long_workspace_bytes(2, 600, 700)
    assert _call(L, ws_bytes=need - 1) == -1                      # short workspace
    assert _call(L, ws_bytes=L.gt_mas_workspace_bytes(2, 600, 700)) == -1      # gt_mas_f32's workspace is not enough
    assert _call(L, stride_x=699) == -1                           # rows overlap
    # past the limits the header states (GT_MAS_LONG_MAX_TX / _TY / _B): unsupported, whatever workspace is offered
    assert _call(L, T_x=4097, T_y=5000) == -2
    assert _call(L, T_x=600, T_y=32769) == -2
    assert _call(L, B=65536, T_x=8, T_y=8) == -2
    assert _call(L, ws=FAKE + 2) == -3                            # workspace not 4-byte aligned


@pytest.mark.parametrize("B,T_x,T_y", [(1, 1, 1), (4, 513, 600), (2, 577, 641), (16, 384, 1304), (1, 2048, 16384), (3, 4096, 32768)])
def test_workspace_holds_the_row_starts_and_every_direction_word(built, B, T_x, T_y):
    from glow_tts_amd import _lib
    L = _lib.lib()
    assert L.gt_mas_long_workspace_bytes(B, T_x, T_y) >= B * (T_x + 1) * 4 + B * T_x * ((T_y + 31) // 32) * 4
    assert L.gt_mas_long_workspace_bytes(B, T_x, T_y) >= L.gt_mas_workspace_bytes(B, T_x, T_y)


def test_workspace_of_an_empty_batch_is_zero(built):
    from glow_tts_amd import _lib
    L = _lib.lib()
    assert L.gt_mas_long_workspace_bytes(0, 600, 700) == 0
    assert L.gt_mas_long_workspace_bytes(4, 0, 700) == 0
    assert L.gt_mas_long_workspace_bytes(4, 600, 0) == 0
    assert L.gt_mas_long_workspace_bytes(-1, 600, 700) == 0


def test_host_rule_sends_only_refused_lattices_to_the_long_kernel(built):
    """the dispatch rule of maximum_path_lengths(allow_long=True) is gt_mas_f32's own: T_x <= 512 and gt_mas_lds_bytes <= 160 KiB"""
    from glow_tts_amd import monotonic_align as ma
    assert ma.fits_lds_kernel(150, 800) and ma.fits_lds_kernel(375, 872)
    assert not ma.fits_lds_kernel(513, 600) and not ma.fits_lds_kernel(384, 1304) and not ma.fits_lds_kernel(150, 4800)
    from glow_tts_amd import _lib
    assert _lib.lib().gt_mas_lds_bytes(384, 1304) == 167056 and _lib.lib().gt_mas_lds_bytes(150, 4800) == 168016


def test_maximum_path_still_refuses_cpu_tensors(built):
    from glow_tts_amd import monotonic_align as ma
    with pytest.raises(TypeError, match="no CPU fallback"):
        ma.maximum_path(torch.zeros(1, 600, 700), torch.ones(1, 600, 700))
    with pytest.raises(RuntimeError, match="no CPU fallback"):      # and still the RuntimeError tests/test_cabi.py expects
        ma.maximum_path(torch.zeros(1, 2, 3), torch.ones(1, 2, 3))
