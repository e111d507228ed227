"""CPU tests of the Vocos kernels' C-ABI (csrc/vocos.hip: gt_vocos_norm, gt_vocos_mlp, gt_vocos_polar and their helpers): every status
returned before any launch, in the order include/glowtts_hip.h declares — NULL / range errors GT_E_INVAL, then GT_E_UNSUPPORTED, then
GT_E_ALIGN — with pointers that are never read (the pattern of tests/test_hifigan_cabi.py), the argument blocks' sizes against the
ctypes mirrors, and the documented values of the helper functions."""
import ctypes

INVAL, UNSUPPORTED, ALIGN = -1, -2, -3
P = 4096                                                                          # a non-NULL, 16-byte aligned "pointer" that is never read


def test_helpers_and_args_sizes(built):
    from glow_tts_amd import _lib
    L = _lib.lib()
    assert L.gt_vocos_norm_args_size() == ctypes.sizeof(_lib.VocosNormArgs) == 96
    assert L.gt_vocos_mlp_args_size() == ctypes.sizeof(_lib.VocosMlpArgs) == 120
    assert L.gt_vocos_polar_args_size() == ctypes.sizeof(_lib.VocosPolarArgs) == 48
    assert _lib.C_STRUCTS[_lib.VocosNormArgs] == "gt_vocos_norm_args" and _lib.C_STRUCTS[_lib.VocosMlpArgs] == "gt_vocos_mlp_args"
    assert _lib.C_STRUCTS[_lib.VocosPolarArgs] == "gt_vocos_polar_args"
    M, HC = L.gt_vocos_tile_positions(), L.gt_vocos_hidden_chunk()
    assert (M, HC, L.gt_vocos_norm_tile_positions()) == (64, 128, 32)
    for C in (128, 256, 512):                                                      # the A tile and the double-buffered u chunk, 16-byte row pads
        assert L.gt_vocos_mlp_lds_bytes(C) == M * (2 * C + 16) + 2 * M * (2 * HC + 16)
    assert L.gt_vocos_mlp_lds_bytes(512) == 101376 <= 160 * 1024
    for C in (0, -128, 64, 192, 384, 1024):
        assert L.gt_vocos_mlp_lds_bytes(C) == 0


def norm(L, **kw):
    from glow_tts_amd import _lib
    base = dict(X=P, x_stride_b=200 * 128, wd=3 * P, bd=4 * P, g=5 * P, be=6 * P, Y=2 * P, y_stride_b=200 * 128, n_frames=7 * P, B=2,
                L_cap=200, C=128, y_bf16=0, eps=1e-6)
    base.update(kw)
    return L.gt_vocos_norm(_lib.fill_args(_lib.VocosNormArgs, **base), None)


def test_vocos_norm_statuses_before_any_launch(built):
    from glow_tts_amd import _lib
    L = _lib.lib()
    assert L.gt_vocos_norm(None, None) == INVAL
    for kw in ({"X": None}, {"g": None}, {"be": None}, {"Y": None}, {"n_frames": None}, {"wd": None}, {"bd": None}, {"B": 0}, {"B": -1},
               {"L_cap": 0}, {"C": 0}, {"C": -64}, {"eps": -1.0}, {"eps": float("nan")}, {"x_stride_b": 200 * 128 - 1},
               {"y_stride_b": 200 * 128 - 1}, {"Y": P}, {"Y": P, "wd": None, "bd": None, "y_bf16": 1}):
        assert norm(L, **kw) == INVAL, kw
    for kw in ({"C": 96, "x_stride_b": 200 * 96, "y_stride_b": 200 * 96}, {"C": 576, "x_stride_b": 200 * 576, "y_stride_b": 200 * 576},
               {"B": 65536}, {"B": 16, "L_cap": 1 << 20, "x_stride_b": 128 << 20, "y_stride_b": 128 << 20}):   # 16 * 2^20 * 128 = 2^31
        assert norm(L, **kw) == UNSUPPORTED, kw
    assert norm(L, C=96, x_stride_b=200 * 96, y_stride_b=200 * 96, B=0) == INVAL   # the argument checks come first
    assert norm(L, C=96, x_stride_b=200 * 96, y_stride_b=200 * 96, X=P + 2) == UNSUPPORTED
    for kw in ({"X": P + 2}, {"wd": 3 * P + 2}, {"bd": 4 * P + 1}, {"g": 5 * P + 2}, {"be": 6 * P + 2}, {"n_frames": 7 * P + 2},
               {"Y": 2 * P + 2}, {"Y": 2 * P + 1, "y_bf16": 1}):
        assert norm(L, **kw) == ALIGN, kw
    assert norm(L, B=15, L_cap=1 << 20, x_stride_b=128 << 20, y_stride_b=128 << 20, X=P + 2) == ALIGN   # below 2^31: passes on


def mlp(L, **kw):
    from glow_tts_amd import _lib
    base = dict(A=P, a_stride_b=200 * 128, W1=2 * P, b1=3 * P, W2=4 * P, b2=5 * P, R=6 * P, r_stride_b=200 * 128, Y=6 * P,
                y_stride_b=200 * 128, U=None, u_stride_b=0, n_frames=7 * P, B=2, L_cap=200, C=128, H=256)
    base.update(kw)
    return L.gt_vocos_mlp(_lib.fill_args(_lib.VocosMlpArgs, **base), None)


def test_vocos_mlp_statuses_before_any_launch(built):
    from glow_tts_amd import _lib
    L = _lib.lib()
    assert L.gt_vocos_mlp(None, None) == INVAL
    for kw in ({"A": None}, {"W1": None}, {"b1": None}, {"W2": None}, {"b2": None}, {"R": None}, {"Y": None}, {"n_frames": None},
               {"B": 0}, {"L_cap": -1}, {"C": 0}, {"H": 0}, {"H": -128}, {"a_stride_b": 200 * 128 - 8}, {"r_stride_b": 200 * 128 - 1},
               {"y_stride_b": 200 * 128 - 1}, {"U": 8 * P, "u_stride_b": 200 * 256 - 4}, {"Y": P}, {"U": 6 * P, "u_stride_b": 200 * 256},
               {"U": P, "u_stride_b": 200 * 256}):
        assert mlp(L, **kw) == INVAL, kw
    big = dict(a_stride_b=512 << 20, r_stride_b=512 << 20, y_stride_b=512 << 20)
    wide = lambda C: dict(C=C, a_stride_b=200 * C, r_stride_b=200 * C, y_stride_b=200 * C)  # noqa: E731
    for kw in (wide(64), wide(192), wide(384), wide(1024), {"H": 192}, {"H": 2048 + 128}, {"B": 65536},
               dict(big, B=4, L_cap=1 << 20, C=512, H=512), {"B": 8, "L_cap": 1 << 20, "C": 128, "H": 256,
                                                                "a_stride_b": 128 << 20, "r_stride_b": 128 << 20, "y_stride_b": 128 << 20}):
        assert mlp(L, **kw) == UNSUPPORTED, kw
    assert mlp(L, B=0, **wide(192)) == INVAL and mlp(L, A=P + 8, **wide(192)) == UNSUPPORTED   # the order of the classes
    for kw in ({"A": P + 8}, {"W1": 2 * P + 8}, {"W2": 4 * P + 4}, {"a_stride_b": 200 * 128 + 4}, {"b1": 3 * P + 2}, {"b2": 5 * P + 2},
               {"R": 6 * P + 2}, {"Y": 9 * P + 2}, {"n_frames": 7 * P + 2}, {"U": 8 * P + 4, "u_stride_b": 200 * 256},
               {"U": 8 * P, "u_stride_b": 200 * 256 + 2}):
        assert mlp(L, **kw) == ALIGN, kw
    assert mlp(L, H=2048, A=P + 8) == ALIGN and mlp(L, A=P + 8, **wide(512)) == ALIGN


def polar(L, **kw):
    from glow_tts_amd import _lib
    base = dict(O=P, o_stride_b=70 * 1026, n_frames=2 * P, spec=3 * P, B=2, F_max=70, n_fft=1024)
    base.update(kw)
    return L.gt_vocos_polar(_lib.fill_args(_lib.VocosPolarArgs, **base), None)


def test_vocos_polar_statuses_before_any_launch(built):
    from glow_tts_amd import _lib
    L = _lib.lib()
    assert L.gt_vocos_polar(None, None) == INVAL
    for kw in ({"O": None}, {"n_frames": None}, {"spec": None}, {"B": 0}, {"B": 65536}, {"F_max": 0}, {"F_max": (1 << 20) + 1},
               {"o_stride_b": 70 * 1026 - 1}):
        assert polar(L, **kw) == INVAL, kw
    for kw in ({"n_fft": 2048}, {"n_fft": 512}, {"n_fft": 0}):
        assert polar(L, **kw) == UNSUPPORTED, kw
    assert polar(L, n_fft=2048, B=0) == INVAL and polar(L, n_fft=2048, spec=3 * P + 8) == UNSUPPORTED
    for kw in ({"O": P + 2}, {"n_frames": 2 * P + 2}, {"spec": 3 * P + 8}, {"spec": 3 * P + 4}):
        assert polar(L, **kw) == ALIGN, kw
