"""CPU tests of the loudness C-ABI (csrc/loudness.hip): every status of gt_loudness_measure and gt_loudness_apply returned before any
launch, in the order include/glowtts_hip.h declares — NULL / out-of-range arguments GT_E_INVAL, then a rate the kernels do not take (or
int16 rows for the scale pass) GT_E_UNSUPPORTED, then alignment GT_E_ALIGN — the chunk lengths, the workspace size and the argument
block's size.  The pattern of tests/test_denoise_cabi.py: pointers that are never read."""
import ctypes

INVAL, UNSUPPORTED, ALIGN = -1, -2, -3
P = 4096                                                                          # a non-NULL, 16-byte aligned "pointer" that is never read
RATES = {16000: 50, 22050: 49, 24000: 50, 44100: 49, 48000: 50}
BAD_RATES = (22051, 7990, 200000, 10090, 0, -22050)
SHAPES = ({"B": 0}, {"B": -1}, {"B": 65536}, {"L_cap": 0}, {"L_cap": -5}, {"ld": 9999}, {"hop": 0}, {"hop": -1}, {"lost": -1})


def _lib_():
    from glow_tts_amd import _lib
    return _lib.lib()


def block(**kw):
    from glow_tts_amd import _lib
    a = dict(wav=P, n_frames=P, params=P, stats=P, ws=P, out=None, ws_bytes=1 << 40, ld=10000, ld_out=0, is_i16=0, hop=1, lost=0, B=2,
             L_cap=10000, fs=22050)
    a.update(kw)
    return ctypes.byref(_lib.fill_args(_lib.LoudnessArgs, **a))


def measure(L, **kw):
    return L.gt_loudness_measure(block(**kw), None)


def apply(L, **kw):
    return L.gt_loudness_apply(block(**kw), None)


def test_statuses_before_any_launch(built):
    L = _lib_()
    assert L.gt_loudness_measure(None, None) == INVAL and L.gt_loudness_apply(None, None) == INVAL
    for entry in (measure, apply):
        for kw in SHAPES + tuple({p: None} for p in ("wav", "n_frames", "stats")):
            assert entry(L, **kw) == INVAL, (entry.__name__, kw)
            assert entry(L, fs=22051, **kw) == INVAL, (entry.__name__, kw)         # the argument checks come first
        for fs in BAD_RATES:
            assert entry(L, fs=fs) == UNSUPPORTED, (entry.__name__, fs)
            assert entry(L, fs=fs, wav=P + 2, stats=P + 2) == UNSUPPORTED          # the rate is refused before the alignment is looked at
        for fs in RATES:
            assert entry(L, fs=fs, wav=P + 2) == ALIGN and entry(L, fs=fs, n_frames=P + 2) == ALIGN and entry(L, fs=fs, stats=P + 1) == ALIGN
    # what only the measurement reads
    for p in ("params", "ws"):
        assert measure(L, **{p: None}) == INVAL
    need = L.gt_loudness_ws_bytes(2, 10000, 22050)
    assert measure(L, ws_bytes=need - 1) == INVAL and measure(L, ws_bytes=need - 1, fs=22051) == UNSUPPORTED
    assert measure(L, params=P + 4) == ALIGN and measure(L, ws=P + 8) == ALIGN and measure(L, is_i16=1, wav=P + 1) == ALIGN
    assert measure(L, B=4096, L_cap=1 << 24, ld=1 << 24) == UNSUPPORTED             # a capacity past 2^31 chunk-state elements
    # what only the scale pass looks at
    assert apply(L, params=None, ws=None, ws_bytes=0, stats=P + 2) == ALIGN         # neither is looked at: the block gets as far as the alignment
    assert apply(L, out=P, ld_out=9999) == INVAL and apply(L, out=P + 2, ld_out=10000) == ALIGN
    assert apply(L, is_i16=1) == UNSUPPORTED and apply(L, is_i16=1, wav=P + 1) == UNSUPPORTED


def test_chunk_lengths_and_workspace_size(built):
    L = _lib_()
    for fs, chunk in RATES.items():
        assert L.gt_loudness_chunk(fs) == chunk and (fs // 10) % chunk == 0
        Kc, Sc = -(-10001 // chunk), 10001 // (fs // 10) + 1
        want = 3 * (Kc * 4 * 8 + Kc * 8 + Sc * 8 + Kc * 4)
        assert L.gt_loudness_ws_bytes(3, 10001, fs) == (want + 15) // 16 * 16
    for fs in BAD_RATES:
        assert L.gt_loudness_chunk(fs) == 0 and L.gt_loudness_ws_bytes(2, 10000, fs) == 0
    for B, cap in ((0, 100), (-1, 100), (65536, 100), (2, 0), (2, -1), (4096, 1 << 24)):
        assert L.gt_loudness_ws_bytes(B, cap, 22050) == 0, (B, cap)


def test_args_size_matches_the_mirror(built):
    from glow_tts_amd import _lib
    assert _lib_().gt_loudness_args_size() == ctypes.sizeof(_lib.LoudnessArgs) == 6 * 8 + 8 + 8 * 4
    assert _lib.LOUD_STATS == 8 and _lib.LOUD_PARAMS == 64
