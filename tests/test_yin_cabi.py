"""CPU tests of the pitch front end's C-ABI (csrc/yin_front.hip: gt_yin_f0, gt_yin_tile_frames): every status returned before any
launch, in the order include/glowtts_hip.h declares — NULL / out-of-range arguments GT_E_INVAL, then a geometry the kernel does not take
GT_E_UNSUPPORTED, then alignment GT_E_ALIGN.  The pattern of tests/test_mel_front_cabi.py: pointers that are never read.  (That the
binding table mirrors the header's new declarations is tests/test_cabi.py's.)"""
INVAL, UNSUPPORTED, ALIGN = -1, -2, -3
P = 4096                                                                          # a non-NULL, 16-byte aligned "pointer" that is never read


def yin(L, wav=P, is_i16=0, ld=4096, wav_len=P, B=2, F_max=17, w_len=1024, hop=256, tau_min=36, tau_max=441, sr=22050.0, thresh=0.1,
        lead=2, f0=P, harm=None, argmin=None):
    return L.gt_yin_f0(wav, is_i16, ld, wav_len, B, F_max, w_len, hop, tau_min, tau_max, sr, thresh, lead, f0, harm, argmin, None)


def test_yin_f0_statuses_before_any_launch(built):
    from glow_tts_amd import _lib
    L = _lib.lib()
    assert L.gt_yin_tile_frames() == 16
    for kw in ({"wav": None}, {"wav_len": None}, {"f0": None}, {"B": 0}, {"B": -1}, {"B": 65536}, {"F_max": 0}, {"F_max": (1 << 20) + 1},
               {"ld": 0}, {"ld": -4}, {"lead": -1}, {"w_len": 0}, {"hop": 0}, {"hop": -256}, {"tau_min": 0}, {"tau_min": -1},
               {"tau_min": 441}, {"tau_min": 500, "tau_max": 441}, {"sr": 0.0}, {"sr": -1.0}, {"sr": float("nan")}):
        assert yin(L, **kw) == INVAL, kw
    # the reference's own defaults (512 / 256), other frames and hops, lags past the two hops the kernel shares
    for kw in ({"w_len": 512}, {"w_len": 2048}, {"hop": 128}, {"hop": 512}, {"w_len": 512, "hop": 128}, {"tau_max": 513}, {"tau_max": 1024}):
        assert yin(L, **kw) == UNSUPPORTED, kw
    assert yin(L, B=0, w_len=512) == INVAL                                        # the argument checks come first
    for kw in ({"f0": P + 4}, {"f0": P + 8}, {"harm": P + 4}, {"argmin": P + 8}, {"wav": P + 2, "is_i16": 1}, {"wav": P + 8},
               {"wav_len": P + 2}, {"ld": 4095}, {"ld": 4094}, {"ld": 4095, "is_i16": 1}):
        assert yin(L, **kw) == ALIGN, kw
    assert yin(L, w_len=512, f0=P + 4) == UNSUPPORTED                             # the geometry is refused before the alignment is looked at
    assert yin(L, tau_max=513, wav_len=P + 2) == UNSUPPORTED
