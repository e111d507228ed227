"""CPU tests of the WaveGlow kernels' C-ABI (csrc/waveglow.hip: gt_wg_gate, gt_wg_boundary and their helpers): every status returned
before any launch, in the order include/glowtts_hip.h declares — NULL / range errors GT_E_INVAL, then GT_E_UNSUPPORTED, then GT_E_ALIGN
— with pointers that are never read (the pattern of tests/test_hifigan_cabi.py), the argument blocks' sizes against the ctypes
mirrors, and the documented values of the helper functions."""
import ctypes

INVAL, UNSUPPORTED, ALIGN = -1, -2, -3
P = 4096                                                                          # a non-NULL, 16-byte aligned "pointer" that is never read


def test_helpers_and_args_sizes(built):
    from glow_tts_amd import _lib
    L = _lib.lib()
    assert L.gt_wg_gate_args_size() == ctypes.sizeof(_lib.WgGateArgs) == 128
    assert L.gt_wg_boundary_args_size() == ctypes.sizeof(_lib.WgBoundaryArgs) == 128
    assert _lib.C_STRUCTS[_lib.WgGateArgs] == "gt_wg_gate_args" and _lib.C_STRUCTS[_lib.WgBoundaryArgs] == "gt_wg_boundary_args"
    M = L.gt_wg_tile_positions()
    assert M == L.gt_voc_tile_positions() == 128
    for C in (64, 256, 512):
        for dil in (1, 4, 128):
            assert L.gt_wg_gate_lds_bytes(C, 3, dil) == (M + 2 * dil) * 144 == L.gt_voc_lds_bytes(C, 3, dil)
    assert L.gt_wg_gate_lds_bytes(256, 3, 128) == 55296 <= 64 * 1024
    for args in ((256, 3, 256), (96, 3, 1), (0, 3, 1), (256, 2, 1), (256, 13, 1), (256, 3, 0), (256, 0, 1)):
        assert L.gt_wg_gate_lds_bytes(*args) == 0, args
    assert (_lib.WG_NOISE_STREAM, _lib.WG_MAX_C) == (5, 512)


def gate(L, **kw):
    from glow_tts_amd import _lib
    C, Lc = 128, 200
    base = dict(X=P, x_stride_b=Lc * 2 * C, ldx=2 * C, Cs=640, S=2 * P, s_stride_b=Lc * 640, W_in=3 * P, W_cond=4 * P, b_in=5 * P,
                b_cond=6 * P, G=7 * P, g_stride_b=Lc * C, len_mul=32, n_frames=8 * P, B=2, L_cap=Lc, C=C, taps=3, dil=4)
    base.update(kw)
    return L.gt_wg_gate(_lib.fill_args(_lib.WgGateArgs, **base), None)


def test_gate_statuses_before_any_launch(built):
    from glow_tts_amd import _lib
    L = _lib.lib()
    assert L.gt_wg_gate(None, None) == INVAL
    for kw in ({"X": None}, {"S": None}, {"W_in": None}, {"W_cond": None}, {"b_in": None}, {"b_cond": None}, {"G": None},
               {"n_frames": None}, {"B": 0}, {"L_cap": 0}, {"C": 0}, {"Cs": -64}, {"dil": 0}, {"len_mul": 0}, {"taps": 0}, {"taps": 4},
               {"ldx": 127}, {"x_stride_b": 200 * 256 - 4}, {"s_stride_b": 200 * 640 - 8}, {"g_stride_b": 200 * 128 - 1}, {"G": P},
               {"G": 2 * P}):
        assert gate(L, **kw) == INVAL, kw
    for kw in ({"taps": 13}, {"C": 96, "ldx": 192, "x_stride_b": 200 * 192}, {"Cs": 80, "s_stride_b": 200 * 80}, {"B": 65536},
               {"B": 16, "L_cap": 1 << 18, "Cs": 512, "x_stride_b": 256 << 18, "s_stride_b": 512 << 18, "g_stride_b": 128 << 18},   # 2^31
               {"dil": 256}):
        assert gate(L, **kw) == UNSUPPORTED, kw
    assert gate(L, taps=13, B=0) == INVAL and gate(L, taps=13, X=P + 4) == UNSUPPORTED   # the order of the classes
    for kw in ({"X": P + 4}, {"S": 2 * P + 8}, {"W_in": 3 * P + 8}, {"W_cond": 4 * P + 4}, {"b_in": 5 * P + 2}, {"b_cond": 6 * P + 2},
               {"G": 7 * P + 2}, {"n_frames": 8 * P + 2}, {"ldx": 258, "x_stride_b": 200 * 258}, {"x_stride_b": 200 * 256 + 2},
               {"s_stride_b": 200 * 640 + 4}):
        assert gate(L, **kw) == ALIGN, kw
    assert gate(L, B=15, L_cap=1 << 18, Cs=512, x_stride_b=256 << 18, s_stride_b=512 << 18, g_stride_b=128 << 18, X=P + 4) == ALIGN


def boundary(L, **kw):
    from glow_tts_amd import _lib
    C, Lc = 128, 200
    base = dict(state=P, st_stride_b=Lc * 2 * C, ld=2 * C, C=C, A=2 * P, a_stride_b=8 * Lc, w_end=3 * P, b_end=4 * P, w_inv=5 * P,
                w_start=6 * P, b_start=7 * P, n_frames=8 * P, seed_dev=None, seed=1, sigma=0.666, len_mul=32, B=2, L_cap=Lc, c_in=6,
                c_out=8)
    base.update(kw)
    return L.gt_wg_boundary(_lib.fill_args(_lib.WgBoundaryArgs, **base), None)


FIRST = dict(w_end=None, b_end=None, w_inv=None, c_in=0, c_out=4)
LAST = dict(w_start=None, b_start=None, c_in=8, c_out=8)


def test_boundary_statuses_before_any_launch(built):
    from glow_tts_amd import _lib
    L = _lib.lib()
    assert L.gt_wg_boundary(None, None) == INVAL
    for kw in ({"state": None}, {"A": None}, {"n_frames": None}, {"B": 0}, {"L_cap": -1}, {"C": 0}, {"len_mul": 0}, {"ld": 255},
               {"st_stride_b": 200 * 256 - 4}, {"a_stride_b": 1596}, {"c_in": 5}, {"c_out": 7}, {"c_in": -2}, {"c_in": 10, "c_out": 10},
               {"c_out": 10}, {"c_in": 0, "c_out": 0}, {"c_in": 8, "c_out": 6}, {"w_end": None}, {"b_end": None}, {"w_inv": None},
               {"c_in": 0}, dict(FIRST, c_in=2), {"w_start": None}, {"b_start": None}, dict(LAST, c_in=6, c_out=6), {"sigma": -0.5},
               {"sigma": float("nan")}):
        assert boundary(L, **kw) == INVAL, kw
    wide = lambda C: dict(C=C, ld=2 * C, st_stride_b=200 * 2 * C)  # noqa: E731
    for kw in (wide(96), wide(576), {"B": 65536}, {"B": 32, "L_cap": 1 << 18, "st_stride_b": 256 << 18, "a_stride_b": 8 << 18}):
        assert boundary(L, **kw) == UNSUPPORTED, kw
    assert boundary(L, B=0, **wide(96)) == INVAL and boundary(L, A=2 * P + 4, **wide(96)) == UNSUPPORTED
    for form in ({}, FIRST, LAST):
        for kw in ({"A": 2 * P + 4}, {"state": P + 2}, {"n_frames": 8 * P + 2}, {"seed_dev": 9 * P + 2}, {"ld": 258, "st_stride_b": 200 * 258},
                   {"st_stride_b": 200 * 256 + 2}, {"a_stride_b": 1602}):
            assert boundary(L, **dict(form, **kw)) == ALIGN, (form, kw)
    for kw in ({"w_end": 3 * P + 8}, {"b_end": 4 * P + 2}, {"w_inv": 5 * P + 8}, {"w_start": 6 * P + 4}, {"b_start": 7 * P + 2}):
        assert boundary(L, **kw) == ALIGN, kw
