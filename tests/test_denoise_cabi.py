"""CPU tests of gt_denoise_spec's C-ABI (csrc/denoise.hip): every status returned before any launch, in the order
include/glowtts_hip.h declares — NULL / out-of-range arguments (lost outside {0, 1} among them) GT_E_INVAL, then a geometry the
kernel does not take GT_E_UNSUPPORTED, then alignment GT_E_ALIGN — and the argument block's size.  The pattern of
tests/test_griffin_lim_cabi.py: pointers that are never read."""
import ctypes

INVAL, UNSUPPORTED, ALIGN = -1, -2, -3
P = 4096                                                                          # a non-NULL, 16-byte aligned "pointer" that is never read
GEOMETRIES = ({"n_fft": 2048, "win": 2048}, {"n_fft": 800, "hop": 200, "win": 800}, {"hop": 128}, {"win": 800})
SHAPES = ({"B": 0}, {"B": -1}, {"B": 65536}, {"F_max": 0}, {"F_max": -2}, {"F_max": (1 << 20) + 1}, {"F_max": 1 << 20, "lost": 0},
          {"lost": -1}, {"lost": 2}, {"ld_wav": 0}, {"ld_wav": -4})
POINTERS = ("wav", "bias", "strength", "n_frames", "mel_packed", "spec", "frames_out")


def denoise(L, **kw):
    from glow_tts_amd import _lib
    a = dict(wav=P, bias=P, strength=P, n_frames=P, mel_packed=P, spec=P, frames_out=P, ld_wav=4096, lost=0, B=2, F_max=16, n_fft=1024,
             hop=256, win=1024)
    a.update(kw)
    return L.gt_denoise_spec(ctypes.byref(_lib.fill_args(_lib.DenoiseSpecArgs, **a)), None)


def _lib_():
    from glow_tts_amd import _lib
    return _lib.lib()


def test_statuses_before_any_launch(built):
    L = _lib_()
    assert L.gt_denoise_spec(None, None) == INVAL
    for kw in GEOMETRIES:
        assert denoise(L, **kw) == UNSUPPORTED, kw                                # every reference config is 1024 / 256 / 1024
    for kw in SHAPES + tuple({p: None} for p in POINTERS):
        assert denoise(L, **kw) == INVAL, kw
    assert denoise(L, B=0, hop=128) == INVAL and denoise(L, lost=2, hop=128) == INVAL   # the argument checks come first
    for p in ("wav", "mel_packed", "spec"):
        assert denoise(L, **{p: P + 4}) == ALIGN and denoise(L, **{p: P + 8}) == ALIGN, p
        assert denoise(L, hop=128, **{p: P + 4}) == UNSUPPORTED, p                # the geometry is refused before the alignment is looked at
    for p in ("bias", "strength", "n_frames", "frames_out"):
        assert denoise(L, **{p: P + 2}) == ALIGN, p
        assert denoise(L, hop=128, **{p: P + 2}) == UNSUPPORTED, p
    assert denoise(L, ld_wav=4095) == ALIGN and denoise(L, ld_wav=4094) == ALIGN and denoise(L, ld_wav=4095, hop=128) == UNSUPPORTED
    assert denoise(L, F_max=(1 << 20), lost=1, B=0) == INVAL


def test_args_size_matches_the_mirror(built):
    from glow_tts_amd import _lib
    assert _lib_().gt_denoise_spec_args_size() == ctypes.sizeof(_lib.DenoiseSpecArgs) == 7 * 8 + 7 * 4 + 4
