"""CPU tests of the mel-inversion entry's C-ABI (csrc/gl_mel.hip: gt_gl_from_mel): every status returned before any launch, in the order
include/glowtts_hip.h declares — a NULL pointer (other than seed_dev) or an out-of-range shape or stride GT_E_INVAL, then alignment
GT_E_ALIGN.  The pattern of tests/test_griffin_lim_cabi.py: pointers that are never read."""
INVAL, ALIGN = -1, -3
P = 4096                                                                          # a non-NULL, 16-byte aligned "pointer" that is never read


def from_mel(L, mel=P, stride_b=80 * 24, stride_c=24, n_frames=P, B=2, F_max=17, n_mel=80, pinv=P, seed=5, seed_dev=None, mag=P, spec=P):
    return L.gt_gl_from_mel(mel, stride_b, stride_c, n_frames, B, F_max, n_mel, pinv, seed, seed_dev, mag, spec, None)


def _lib():
    from glow_tts_amd import _lib
    return _lib.lib()


def test_from_mel_statuses_before_any_launch(built):
    L = _lib()
    for p in ("mel", "n_frames", "pinv", "mag", "spec"):
        assert from_mel(L, **{p: None}) == INVAL, p
    for kw in ({"B": 0}, {"B": -1}, {"B": 65536}, {"F_max": 0}, {"F_max": -2}, {"F_max": (1 << 20) + 1, "stride_b": 1 << 30, "stride_c": 1 << 21},
               {"n_mel": 0}, {"n_mel": -3}, {"n_mel": 129}):
        assert from_mel(L, **kw) == INVAL, kw
    for kw in ({"stride_b": 0}, {"stride_b": -1920}, {"stride_b": 16}, {"stride_c": 0}, {"stride_c": -24}, {"stride_c": 16}):
        assert from_mel(L, **kw) == INVAL, kw                                     # a row must hold F_max frames
    for p in ("mag", "spec", "pinv"):
        assert from_mel(L, **{p: P + 4}) == ALIGN and from_mel(L, **{p: P + 8}) == ALIGN, p
    for p in ("mel", "n_frames", "seed_dev"):
        assert from_mel(L, **{p: P + 2}) == ALIGN and from_mel(L, **{p: P + 1}) == ALIGN, p
    assert from_mel(L, B=0, mag=P + 4) == INVAL and from_mel(L, stride_c=16, mel=P + 2) == INVAL      # the argument checks come first
    assert from_mel(L, mel=None, seed_dev=P + 2) == INVAL


def test_from_mel_is_declared_and_bound(built):
    from glow_tts_amd import _lib
    res, args = _lib.PROTOTYPES["gt_gl_from_mel"]
    assert res is _lib.STATUS and len(args) == 13
    assert args[1] is _lib.c_i64 and args[2] is _lib.c_i64 and args[8] is _lib.c_u32   # strides in elements, the seed by value
