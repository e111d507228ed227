"""CPU tests of the activation kernel's C-ABI (csrc/voc_snake.hip: gt_voc_snake and its helpers): every status returned before any
launch, in the order include/glowtts_hip.h declares — NULL / range errors GT_E_INVAL, then GT_E_UNSUPPORTED, then GT_E_ALIGN — with
pointers that are never read (the pattern of tests/test_hifigan_cabi.py), and the argument block's size against the ctypes mirror."""
import ctypes

INVAL, UNSUPPORTED, ALIGN = -1, -2, -3
P = 4096                                                                          # a non-NULL, 16-byte aligned "pointer" that is never read


def args(**kw):
    from glow_tts_amd import _lib
    base = dict(X=P, x_stride_b=200 * 32, P=3 * P, Y=2 * P, y_stride_b=200 * 32, len_mul=1, n_frames=P, B=2, L_cap=200, C=32)
    base.update(kw)
    return _lib.fill_args(_lib.VocSnakeArgs, **base)


def snake(L, **kw):
    return L.gt_voc_snake(args(**kw), None)


def test_args_size_and_tile(built):
    from glow_tts_amd import _lib
    L = _lib.lib()
    assert L.gt_voc_snake_args_size() == ctypes.sizeof(_lib.VocSnakeArgs) == 72
    assert L.gt_voc_snake_tile_positions() == 256
    assert _lib.C_STRUCTS[_lib.VocSnakeArgs] == "gt_voc_snake_args"


def test_voc_snake_statuses_before_any_launch(built):
    from glow_tts_amd import _lib
    L = _lib.lib()
    assert L.gt_voc_snake(None, None) == INVAL
    for kw in ({"X": None}, {"Y": None}, {"P": None}, {"n_frames": None}, {"B": 0}, {"B": -1}, {"L_cap": 0}, {"L_cap": -5}, {"C": 0},
               {"C": -16}, {"len_mul": 0}, {"len_mul": -1}, {"x_stride_b": 200 * 32 - 8}, {"y_stride_b": 200 * 32 - 8}, {"Y": P}):
        assert snake(L, **kw) == INVAL, kw
    for kw in ({"C": 24, "x_stride_b": 200 * 24, "y_stride_b": 200 * 24}, {"C": 8}, {"B": 65536},
               {"B": 64, "L_cap": 1 << 20, "x_stride_b": 32 << 20, "y_stride_b": 32 << 20}):           # 64 * 2^20 * 32 = 2^31
        assert snake(L, **kw) == UNSUPPORTED, kw
    assert snake(L, B=63, L_cap=1 << 20, x_stride_b=32 << 20, y_stride_b=32 << 20, X=P + 8) == ALIGN     # just below 2^31 passes on
    assert snake(L, C=24, B=0) == INVAL                                            # the argument checks come first
    assert snake(L, C=24, X=P + 8) == UNSUPPORTED                                  # refused before the alignment is looked at
    for kw in ({"X": P + 8}, {"X": P + 4}, {"Y": 2 * P + 4}, {"Y": 2 * P + 2}, {"P": 3 * P + 2}, {"n_frames": P + 2},
               {"x_stride_b": 200 * 32 + 4}, {"y_stride_b": 200 * 32 + 4}):
        assert snake(L, **kw) == ALIGN, kw
