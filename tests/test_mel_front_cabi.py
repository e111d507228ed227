"""CPU tests of the mel front end's C-ABI (csrc/mel_front.hip: gt_mel_pack, gt_mel_spectrogram): every status returned before any
launch, in the order include/glowtts_hip.h declares — NULL / out-of-range arguments GT_E_INVAL, then shapes the kernel does not take
GT_E_UNSUPPORTED, then alignment GT_E_ALIGN.  The pattern of tests/test_attn_route_cabi.py: pointers that are never read.  (That the
binding table mirrors the header's new declarations is tests/test_cabi.py's.)"""
INVAL, UNSUPPORTED, ALIGN = -1, -2, -3
P = 4096                                                                          # a non-NULL, 16-byte aligned "pointer" that is never read


def spec(L, wav=P, is_i16=0, ld=4096, wav_len=P, B=2, F_max=17, packed=P, n_fft=1024, hop=256, win=1024, n_mel=80, mel=P, energy=P, mag=None):
    return L.gt_mel_spectrogram(wav, is_i16, ld, wav_len, B, F_max, packed, n_fft, hop, win, n_mel, 1e-5, mel, energy, mag, None)


def test_mel_spectrogram_statuses_before_any_launch(built):
    from glow_tts_amd import _lib
    L = _lib.lib()
    assert spec(L, n_mel=129) == UNSUPPORTED and spec(L, n_mel=0) == INVAL and spec(L, n_mel=-3) == INVAL
    for kw in ({"n_fft": 2048, "win": 2048}, {"n_fft": 800, "hop": 200, "win": 800}, {"hop": 128}, {"win": 800}):
        assert spec(L, **kw) == UNSUPPORTED, kw                                   # every reference config is 1024 / 256 / 1024
    for kw in ({"B": 0}, {"B": -1}, {"B": 65536}, {"F_max": 0}, {"F_max": (1 << 20) + 1}, {"ld": 0}, {"wav": None}, {"wav_len": None},
               {"packed": None}, {"mel": None}, {"energy": None}):
        assert spec(L, **kw) == INVAL, kw
    assert spec(L, B=0, n_mel=129) == INVAL                                       # the argument checks come first
    for kw in ({"mel": P + 4}, {"mel": P + 8}, {"energy": P + 4}, {"mag": P + 4}, {"wav": P + 2, "is_i16": 1}, {"wav": P + 8}, {"packed": P + 4},
               {"wav_len": P + 2}, {"ld": 4095}, {"ld": 4094}, {"ld": 4095, "is_i16": 1}):
        assert spec(L, **kw) == ALIGN, kw
    assert spec(L, n_mel=129, mel=P + 4) == UNSUPPORTED                           # the shape is refused before the alignment is looked at


def test_mel_pack_statuses_and_sizes(built):
    from glow_tts_amd import _lib
    L = _lib.lib()
    # basis image [16 bin tiles][64 step groups][64 lanes][cos 4 | sin 4], bin 512's row, mel image [16][4][64][16], mel_basis[:, 512]
    assert L.gt_mel_pack_bytes() == 4 * (16 * 64 * 64 * 8 + 512 + 16 * 4 * 64 * 16 + 128)
    assert L.gt_mel_tile_frames() == 64
    assert L.gt_mel_pack(None, P, 1024, 80, P, None) == INVAL and L.gt_mel_pack(P, None, 1024, 80, P, None) == INVAL
    assert L.gt_mel_pack(P, P, 1024, 80, None, None) == INVAL and L.gt_mel_pack(P, P, 1024, 0, P, None) == INVAL
    assert L.gt_mel_pack(P, P, 2048, 80, P, None) == UNSUPPORTED and L.gt_mel_pack(P, P, 1024, 129, P, None) == UNSUPPORTED
    assert L.gt_mel_pack(P + 4, P, 1024, 80, P, None) == ALIGN and L.gt_mel_pack(P, P, 1024, 80, P + 8, None) == ALIGN
