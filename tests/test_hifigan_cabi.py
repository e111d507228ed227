"""CPU tests of the vocoder kernel's C-ABI (csrc/hifigan.hip: gt_voc_conv and its helpers): every status returned before any launch, in
the order include/glowtts_hip.h declares — NULL / range errors GT_E_INVAL, then GT_E_UNSUPPORTED, then GT_E_ALIGN — with pointers that
are never read (the pattern of tests/test_resample_cabi.py), and the argument block's size against the ctypes mirror.  (That the
binding table and the mirror's field offsets match the header is tests/test_cabi.py's.)"""
import ctypes

INVAL, UNSUPPORTED, ALIGN = -1, -2, -3
P = 4096                                                                          # a non-NULL, 16-byte aligned "pointer" that is never read


def args(**kw):
    from glow_tts_amd import _lib
    base = dict(X=P, x_stride_b=200 * 32, x_stride_c=0, W=P, bias=P, res=None, acc=None, Y=2 * P, y_stride_b=200 * 32, ldy=32, len_mul=1,
                n_frames=P, B=2, L_cap=200, Cin=32, N=32, taps=7, dil=3, x_bf16=0, x_mel=0, y_bf16=0, tanh_out=0, slope=0.1, scale=1.0)
    base.update(kw)
    return _lib.fill_args(_lib.VocConvArgs, **base)


def voc(L, **kw):
    return L.gt_voc_conv(args(**kw), None)


MEL = dict(x_mel=1, Cin=80, x_stride_c=208, x_stride_b=80 * 208)


def test_args_size_tile_and_lds_bytes(built):
    from glow_tts_amd import _lib
    L = _lib.lib()
    assert L.gt_voc_conv_args_size() == ctypes.sizeof(_lib.VocConvArgs) == 136
    M = L.gt_voc_tile_positions()
    assert M == 128
    for Cin, taps, dil in ((32, 11, 5), (512, 11, 5), (80, 7, 1), (64, 3, 1), (16, 1, 1)):
        kc = L.gt_voc_k_chunk(Cin)
        assert kc == (64 if Cin % 64 == 0 else 32)
        assert L.gt_voc_lds_bytes(Cin, taps, dil) == (M + (taps - 1) * dil) * (2 * kc + 16), (Cin, taps, dil)
    assert L.gt_voc_lds_bytes(512, 11, 5) == 25632 and L.gt_voc_lds_bytes(32, 11, 5) == 14240
    for Cin, taps, dil in ((24, 3, 1), (0, 3, 1), (32, 4, 1), (32, 13, 1), (32, 0, 1), (32, 3, 0), (64, 11, 33), (32, 11, 70)):
        assert L.gt_voc_lds_bytes(Cin, taps, dil) == 0, (Cin, taps, dil)          # 64 KB: 455 rows of 144 bytes, 819 of 80
    assert L.gt_voc_lds_bytes(64, 11, 32) == 448 * 144 and L.gt_voc_lds_bytes(32, 11, 69) == 818 * 80


def test_voc_conv_statuses_before_any_launch(built):
    from glow_tts_amd import _lib
    L = _lib.lib()
    assert L.gt_voc_conv(None, None) == INVAL
    for kw in ({"X": None}, {"W": None}, {"bias": None}, {"Y": None}, {"n_frames": None}, {"B": 0}, {"B": -1}, {"L_cap": 0}, {"Cin": 0},
               {"Cin": -16}, {"N": 0}, {"taps": 0}, {"taps": -3}, {"taps": 4}, {"dil": 0}, {"dil": -1}, {"len_mul": 0}, {"ldy": 31},
               {"ldy": 0}, {"y_stride_b": 200 * 32 - 1}, {"x_stride_b": 200 * 32 - 8}, {"Y": P},
               dict(MEL, x_stride_c=199), dict(MEL, x_stride_b=199), dict(MEL, x_bf16=1)):
        assert voc(L, **kw) == INVAL, kw
    for kw in ({"taps": 13}, {"Cin": 24, "x_stride_b": 200 * 24}, {"B": 65536}, {"taps": 11, "dil": 70},
               {"B": 64, "L_cap": 1 << 20, "x_stride_b": 32 << 20, "y_stride_b": 32 << 20},              # 64 * 2^20 * 32 = 2^31
               {"N": 2048, "ldy": 2048, "L_cap": 1 << 19, "B": 2, "y_stride_b": 1 << 30, "x_stride_b": 32 << 19}):
        assert voc(L, **kw) == UNSUPPORTED, kw
    assert voc(L, B=63, L_cap=1 << 20, x_stride_b=32 << 20, y_stride_b=32 << 20, W=P + 8) == ALIGN      # just below 2^31 passes on
    assert voc(L, taps=13, B=0) == INVAL                                           # the argument checks come first
    assert voc(L, taps=13, W=P + 8) == UNSUPPORTED                                 # refused before the alignment is looked at
    for kw in ({"W": P + 8}, {"bias": P + 2}, {"n_frames": P + 2}, {"Y": 2 * P + 2}, {"res": P + 2}, {"acc": P + 1}, {"X": P + 8},
               {"X": P + 4}, {"x_stride_b": 200 * 32 + 4}, dict(MEL, X=P + 2)):
        assert voc(L, **kw) == ALIGN, kw
