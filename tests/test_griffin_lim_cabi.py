"""CPU tests of the waveform back end's C-ABI (csrc/griffin_lim.hip: gt_gl_pack, gt_gl_polar, gt_gl_project, gt_istft): every status
returned before any launch, in the order include/glowtts_hip.h declares — NULL / out-of-range arguments GT_E_INVAL, then a geometry
the kernels do not take GT_E_UNSUPPORTED, then alignment GT_E_ALIGN — and the size formulas.  The pattern of
tests/test_mel_front_cabi.py: pointers that are never read."""
INVAL, UNSUPPORTED, ALIGN = -1, -2, -3
P = 4096                                                                          # a non-NULL, 16-byte aligned "pointer" that is never read
GEOMETRIES = ({"n_fft": 2048, "win": 2048}, {"n_fft": 800, "hop": 200, "win": 800}, {"hop": 128}, {"win": 800})
SHAPES = ({"B": 0}, {"B": -1}, {"B": 65536}, {"F_max": 0}, {"F_max": -2}, {"F_max": (1 << 20) + 1})


def polar(L, mag=P, phase=P, n_frames=P, B=2, F_max=17, n_fft=1024, hop=256, win=1024, spec=P):
    return L.gt_gl_polar(mag, phase, n_frames, B, F_max, n_fft, hop, win, spec, None)


def project(L, wav=P, ld=4096, mag=P, n_frames=P, B=2, F_max=17, packed=P, n_fft=1024, hop=256, win=1024, spec=P):
    return L.gt_gl_project(wav, ld, mag, n_frames, B, F_max, packed, n_fft, hop, win, spec, None)


def istft(L, spec=P, n_frames=P, B=2, F_max=17, packed=P, n_fft=1024, hop=256, win=1024, wav=P, ld=4096):
    return L.gt_istft(spec, n_frames, B, F_max, packed, n_fft, hop, win, wav, ld, None)


def _lib():
    from glow_tts_amd import _lib
    return _lib.lib()


def _common(L, fn, pointers, aligned16):
    for kw in GEOMETRIES:
        assert fn(L, **kw) == UNSUPPORTED, kw                                     # every reference config is 1024 / 256 / 1024
    for kw in SHAPES + tuple({p: None} for p in pointers):
        assert fn(L, **kw) == INVAL, kw
    assert fn(L, B=0, hop=128) == INVAL                                           # the argument checks come first
    for p in aligned16:
        assert fn(L, **{p: P + 4}) == ALIGN and fn(L, **{p: P + 8}) == ALIGN, p
    assert fn(L, n_frames=P + 2) == ALIGN and fn(L, n_frames=P + 4, hop=128) == UNSUPPORTED
    assert fn(L, hop=128, **{aligned16[0]: P + 4}) == UNSUPPORTED                 # the geometry is refused before the alignment is looked at


def test_polar_statuses_before_any_launch(built):
    _common(_lib(), polar, ("mag", "phase", "n_frames", "spec"), ("mag", "phase", "spec"))


def test_project_statuses_before_any_launch(built):
    L = _lib()
    _common(L, project, ("wav", "mag", "n_frames", "packed", "spec"), ("wav", "mag", "packed", "spec"))
    assert project(L, ld=0) == INVAL and project(L, ld=-4) == INVAL
    assert project(L, ld=4095) == ALIGN and project(L, ld=4094) == ALIGN
    assert project(L, ld=0, hop=128) == INVAL and project(L, ld=4095, hop=128) == UNSUPPORTED


def test_istft_statuses_before_any_launch(built):
    L = _lib()
    _common(L, istft, ("spec", "n_frames", "packed", "wav"), ("spec", "packed", "wav"))
    assert istft(L, ld=0) == INVAL and istft(L, ld=-4) == INVAL
    assert istft(L, ld=4092) == INVAL and istft(L, F_max=18, ld=4096) == INVAL    # the row must hold 256 (F_max - 1) samples
    assert istft(L, F_max=5, ld=1026) == ALIGN and istft(L, F_max=5, ld=1025) == ALIGN
    assert istft(L, F_max=5, ld=1020, hop=128) == INVAL
    assert istft(L, F_max=1, ld=4) == 0                                           # one frame has no hop: nothing to launch, nothing wrong


def test_pack_statuses_and_sizes(built):
    L = _lib()
    # basis image [16 column tiles][64 bin groups][64 lanes][cos 4 | sin 4], bin 512's row by tile and row, the squared window
    assert L.gt_gl_pack_bytes() == 4 * (16 * 64 * 64 * 8 + 512 + 1024)
    assert L.gt_gl_tile_frames() == 64 and L.gt_gl_tile_hops() == 61 == L.gt_gl_tile_frames() - 3
    assert L.gt_gl_pack(None, 1024, P, None) == INVAL and L.gt_gl_pack(P, 1024, None, None) == INVAL
    assert L.gt_gl_pack(P, 2048, P, None) == UNSUPPORTED and L.gt_gl_pack(None, 2048, P, None) == INVAL
    assert L.gt_gl_pack(P + 4, 1024, P, None) == ALIGN and L.gt_gl_pack(P, 1024, P + 8, None) == ALIGN
    assert L.gt_gl_pack(P + 4, 2048, P, None) == UNSUPPORTED


def test_spec_bytes_formula(built):
    L = _lib()
    for B, F in ((1, 1), (1, 64), (1, 65), (3, 66), (32, 800), (65535, 1), (2, 1 << 20)):
        Fp = (F + 63) // 64 * 64
        assert L.gt_gl_spec_bytes(B, F) == 4 * B * Fp * (2 * 512 + 1), (B, F)     # re and im of bins 0..511, re of bin 512
    assert L.gt_gl_spec_bytes(32, 800) == 32 * 832 * 1025 * 4                     # 109 MB for the bench batch
    for B, F in ((0, 5), (-1, 5), (65536, 5), (1, 0), (1, (1 << 20) + 1)):
        assert L.gt_gl_spec_bytes(B, F) == 0, (B, F)
