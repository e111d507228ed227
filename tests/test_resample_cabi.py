"""CPU tests of the resampler's C-ABI (csrc/resample.hip: gt_resample, gt_resample_taps, gt_resample_lds_bytes, gt_resample_tile_out):
every status returned before any launch, in the order include/glowtts_hip.h declares — NULL / out-of-range arguments GT_E_INVAL, then
taps that are not the pair's GT_E_INVAL, then a pair the kernel does not take GT_E_UNSUPPORTED, then alignment GT_E_ALIGN.  The pattern
of tests/test_yin_cabi.py: pointers that are never read.  (That the binding table mirrors the header's new declarations is
tests/test_cabi.py's.)"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import resample64 as R  # noqa: E402

INVAL, UNSUPPORTED, ALIGN = -1, -2, -3
P = 4096                                                                          # a non-NULL, 16-byte aligned "pointer" that is never read


def rs(L, wav=P, is_i16=0, ld=4096, wav_len=P, B=2, bank=P, up=147, down=320, taps=44, out=P, ld_out=2048, out_len=P):
    return L.gt_resample(wav, is_i16, ld, wav_len, B, bank, up, down, taps, out, ld_out, out_len, None)


def test_resample_taps_and_lds_bytes(built):
    from glow_tts_amd import _lib
    L = _lib.lib()
    tile = L.gt_resample_tile_out()
    assert tile == 512
    for pair in R.ALL_PAIRS:
        up, down = R.ratio(*pair)
        T = R.TAPS[pair]
        assert L.gt_resample_taps(up, down) == T == -(-(20 * max(up, down) + 1) // up)
        bank, span = up * (T | 1), (up - 1 + (tile - 1) * down) // up + T
        lds = 4 * ((bank + 3) // 4 * 4 + (span + 3) // 4 * 4)
        assert L.gt_resample_lds_bytes(up, down) == lds <= 64 * 1024, pair
    assert L.gt_resample_lds_bytes(147, 320) == 31104 and L.gt_resample_lds_bytes(441, 640) == 57776
    # not reduced, non-positive, a bank past the LDS (1000 phases of 21 taps), a span past it (40 : 1)
    for up, down in ((2, 4), (294, 640), (0, 1), (1, 0), (-147, 320), (1000, 999), (1, 40), (1 << 30, 3)):
        assert L.gt_resample_taps(up, down) == 0 and L.gt_resample_lds_bytes(up, down) == 0, (up, down)
    assert L.gt_resample_taps(1, 1) == 21 and L.gt_resample_taps(1, 24) == 481


def test_resample_statuses_before_any_launch(built):
    from glow_tts_amd import _lib
    L = _lib.lib()
    for kw in ({"wav": None}, {"wav_len": None}, {"bank": None}, {"out": None}, {"B": 0}, {"B": -1}, {"B": 65536}, {"ld": 0}, {"ld": -4},
               {"ld_out": 0}, {"ld_out": -4}, {"up": 0}, {"up": -147}, {"down": 0}, {"down": -1}, {"taps": 0}, {"taps": -44}):
        assert rs(L, **kw) == INVAL, kw
    for kw in ({"taps": 43}, {"taps": 45}, {"up": 441, "down": 320}, {"up": 1000, "down": 999, "taps": 20}, {"up": 2, "down": 4, "taps": 40}):
        assert rs(L, **kw) == INVAL, kw                                            # taps that are not ceil((20 max + 1) / up)
    for kw in ({"up": 1000, "down": 999, "taps": 21}, {"up": 1, "down": 40, "taps": 801}, {"up": 2, "down": 4, "taps": 41},
               {"up": 294, "down": 640, "taps": 44}, {"ld_out": (1 << 30) + 4}):
        assert rs(L, **kw) == UNSUPPORTED, kw
    assert rs(L, B=0, up=1000, down=999, taps=21) == INVAL                         # the argument checks come first
    assert rs(L, taps=43, out=P + 4) == INVAL
    for kw in ({"wav": P + 8}, {"wav": P + 2, "is_i16": 1}, {"bank": P + 4}, {"out": P + 4}, {"out": P + 8}, {"wav_len": P + 2},
               {"out_len": P + 2}, {"ld": 4095}, {"ld": 4094, "is_i16": 1}, {"ld_out": 2047}, {"ld_out": 2050}):
        assert rs(L, **kw) == ALIGN, kw
    assert rs(L, up=1000, down=999, taps=21, out=P + 4) == UNSUPPORTED             # the pair is refused before the alignment is looked at
    for pair in R.ALL_PAIRS:                                                       # the six pairs pass every check up to the alignment
        up, down = R.ratio(*pair)
        assert rs(L, up=up, down=down, taps=R.TAPS[pair], out=P + 4) == ALIGN, pair
