"""CPU tests of the attention host path (csrc/internal.h gt_attn_route, the dispatch of gt_attn_fwd in csrc/encoder_ops.hip): the two
hand-ons from a key-tiled shape whose layout the key-tiled kernel does not take, which end before any launch, and the one resolver of
what a forward saves (encoder_impl.save_mode).  No device is needed."""
import types

INVAL, UNSUPPORTED, ALIGN = -1, -2, -3
P = 4096                                                                          # a non-NULL, 16-byte aligned "pointer" that is never read
H, D = 2, 96
C = H * D


def attn_fwd(L, T, ld, P_):
    return L.gt_attn_fwd(P, P, P, ld, P, P, P, P, C, P_, 1, T, T + 2, None, H, D, 4, 0.0, 0, None, None)


def attn_bwd(L, T, ld):
    wsb = L.gt_attn_bwd_workspace_bytes(1, T, H)
    return L.gt_attn_bwd(P, P, P, ld, P, P, P, P, C, P, P, wsb, P, P, P, 3 * C, P, P, 1, T, T + 2, None, H, D, 4, 0.0, 0, None, None)


def test_long_shape_with_a_row_pitch_the_kernel_does_not_take(built):
    """D = 96, 505 < T, row pitch 3 C + 4 (no multiple of 8 halfs): the key-tiled kernels do not take the layout.  Without a P there is
    nothing behind them: GT_E_ALIGN.  With one the call is handed to the generic kernels, which refuse what their LDS does not hold,
    GT_E_UNSUPPORTED: the backward from T = 506, the forward from T = 598 (260 T + 8448 bytes against 160 KiB; at 506 .. 597 it
    launches, which a test without device memory must not do)."""
    from glow_tts_amd import _lib
    L = _lib.lib()
    assert L.gt_attn_long_shape(506, D, 4) == 1 and L.gt_attn_long_shape(598, D, 4) == 1
    assert attn_fwd(L, 506, 3 * C + 4, None) == ALIGN
    assert attn_fwd(L, 598, 3 * C + 4, None) == ALIGN
    assert attn_fwd(L, 598, 3 * C + 4, P) == UNSUPPORTED
    assert attn_bwd(L, 506, 3 * C + 4) == UNSUPPORTED


def test_save_mode_resolves_the_three_switches():
    from glow_tts_amd import encoder_impl as e
    assert (e.SAVE_P, e.SAVE_NONE, e.SAVE_STATS) == (True, False, "stats")
    att = lambda keep: types.SimpleNamespace(keep_p=keep)                                    # noqa: E731  MultiHeadAttention.keep_p
    enc = lambda keep: types.SimpleNamespace(rows_cfg=types.SimpleNamespace(attn_keep_p=keep))    # noqa: E731  RowsConfig.attn_keep_p
    for owner in (att, enc):
        assert e.save_mode(owner(True)) is e.SAVE_P and e.save_mode(owner(False)) == e.SAVE_STATS
        assert e.save_mode(owner(True), False) is e.SAVE_NONE and e.save_mode(owner(False), False) is e.SAVE_NONE    # synthesis
        assert e.save_mode(owner(True), e.SAVE_STATS) == e.SAVE_STATS
    assert e.save_mode(types.SimpleNamespace()) is e.SAVE_P                                  # no switch anywhere: P is kept
