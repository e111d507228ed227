"""CPU tests of the synthesis metrics' C-ABI (csrc/dtw.hip: gt_mel_cepstrum, gt_dtw_f32, gt_dtw_f0_stats, gt_dtw_workspace_bytes,
gt_dtw_lds_bytes): every status returned before any launch, in the order include/glowtts_hip.h declares — NULL / out-of-range arguments
GT_E_INVAL, then a shape the kernel does not take GT_E_UNSUPPORTED, then alignment GT_E_ALIGN — and the two size helpers against
their formulas.  The pattern of tests/test_resample_cabi.py: pointers that are never read.  (That the binding table mirrors the
header's new declarations is tests/test_cabi.py's.)"""
INVAL, UNSUPPORTED, ALIGN = -1, -2, -3
P = 4096                                                                          # a non-NULL, 16-byte aligned "pointer" that is never read
CU_LDS = 160 * 1024


def nq(Fb):
    return (-(-Fb // 16) + 3) // 4 * 4


def workspace_bytes(B, Fa, Fb):
    return (4 * (B * Fa * nq(Fb) + B * ((Fa + Fb + 63) // 64 * 64)) + 255) // 256 * 256


def lds_bytes(Fa, Fb):
    fixed = 512 * min(-(-Fa // 64), 16) + ((4 * Fb + 15) // 16 * 16 if Fa > 1024 else 0)
    return fixed + 64 * Fb if fixed + 64 * Fb <= CU_LDS else fixed


def cep(L, mel=P, ld=800, length=P, dct=P, B=2, N=80, K=13, F=800, out=P):
    return L.gt_mel_cepstrum(mel, ld, length, dct, B, N, K, F, out, None)


def dtw(L, a=P, b=P, a_len=P, b_len=P, B=2, Fa=800, Fb=760, alpha=1.0, cost=P, path_len=P, path=P, ld=None, ws=P, ws_bytes=None, status=None):
    ld = Fa + Fb - 1 if ld is None else ld
    ws_bytes = workspace_bytes(B, Fa, Fb) if ws_bytes is None else ws_bytes
    return L.gt_dtw_f32(a, b, a_len, b_len, B, Fa, Fb, alpha, cost, path_len, path, ld, ws, ws_bytes, status, None)


def f0(L, path=P, ld=1559, path_len=P, fa=P, ld_a=800, fb=P, ld_b=760, B=2, counts=P, sums=P):
    return L.gt_dtw_f0_stats(path, ld, path_len, fa, ld_a, fb, ld_b, B, counts, sums, None)


def test_dtw_workspace_and_lds_bytes(built):
    from glow_tts_amd import _lib
    L = _lib.lib()
    for B, Fa, Fb in ((1, 1, 1), (32, 800, 760), (3, 17, 16), (3, 16, 17), (2, 4096, 4096), (7, 1025, 33), (1, 64, 2500), (1, 64, 2600)):
        assert L.gt_dtw_workspace_bytes(B, Fa, Fb) == workspace_bytes(B, Fa, Fb), (B, Fa, Fb)
        assert L.gt_dtw_lds_bytes(Fa, Fb) == lds_bytes(Fa, Fb) <= CU_LDS, (Fa, Fb)
    assert L.gt_dtw_workspace_bytes(32, 800, 760) == 32 * (800 * 48 + 1600) * 4 == 5120000
    assert L.gt_dtw_lds_bytes(800, 760) == 13 * 512 + 64 * 760 == 55296             # the bench shape: rings + the image of b
    assert L.gt_dtw_lds_bytes(64, 2600) == 512 and L.gt_dtw_lds_bytes(4096, 4096) == 8192 + 16384    # b from global memory
    assert L.gt_dtw_lds_bytes(1024, 2432) == 8192 + 64 * 2432 == CU_LDS             # the largest image next to sixteen rings
    for shape in ((0, 8, 8), (2, 0, 8), (2, 8, 0), (-1, 8, 8), (2, 4097, 8), (2, 8, 4097)):
        assert L.gt_dtw_workspace_bytes(*shape) == 0, shape
    for shape in ((0, 8), (8, 0), (4097, 8), (8, 4097)):
        assert L.gt_dtw_lds_bytes(*shape) == 0, shape


def test_mel_cepstrum_statuses_before_any_launch(built):
    from glow_tts_amd import _lib
    L = _lib.lib()
    for kw in ({"mel": None}, {"length": None}, {"dct": None}, {"out": None}, {"B": 0}, {"B": -1}, {"B": 65536}, {"N": 0}, {"N": -80},
               {"K": 0}, {"K": -1}, {"F": 0}, {"F": -4}, {"F": (1 << 20) + 1, "ld": 1 << 21}, {"ld": 799}, {"ld": 0}):
        assert cep(L, **kw) == INVAL, kw
    for kw in ({"N": 129}, {"K": 17}, {"N": 1000, "K": 100}):
        assert cep(L, **kw) == UNSUPPORTED, kw
    assert cep(L, N=129, B=0) == INVAL and cep(L, K=17, ld=799) == INVAL            # the argument checks come first
    for kw in ({"out": P + 4}, {"out": P + 8}, {"mel": P + 2}, {"length": P + 2}, {"dct": P + 1}):
        assert cep(L, **kw) == ALIGN, kw
    assert cep(L, N=129, out=P + 4) == UNSUPPORTED                                  # refused before the alignment is looked at
    assert cep(L, N=128, K=16, out=P + 4) == ALIGN                                  # the limits themselves pass up to the alignment


def test_dtw_statuses_before_any_launch(built):
    from glow_tts_amd import _lib
    L = _lib.lib()
    for kw in ({"a": None}, {"b": None}, {"a_len": None}, {"b_len": None}, {"cost": None}, {"path_len": None}, {"path": None}, {"ws": None},
               {"B": 0}, {"B": -1}, {"B": 65536}, {"Fa": 0}, {"Fa": -8}, {"Fb": 0}, {"Fb": -8}, {"ld": 800 + 760 - 2}, {"ld": 0}, {"ld": -1},
               {"ws_bytes": workspace_bytes(2, 800, 760) - 1}, {"ws_bytes": 0}):
        assert dtw(L, **kw) == INVAL, kw
    for kw in ({"Fa": 4097}, {"Fb": 4097}, {"Fa": 1 << 30, "Fb": 1 << 30, "ld": (1 << 31) - 1}):
        assert dtw(L, ws_bytes=1 << 40, **kw) == UNSUPPORTED, kw
    assert dtw(L, Fa=4097, B=0) == INVAL and dtw(L, Fa=4097, ld=10) == INVAL        # the argument checks come first
    for kw in ({"a": P + 4}, {"b": P + 8}, {"path": P + 8}, {"ws": P + 4}, {"a_len": P + 2}, {"b_len": P + 2}, {"cost": P + 2},
               {"path_len": P + 1}, {"status": P + 2}):
        assert dtw(L, **kw) == ALIGN, kw
    assert dtw(L, Fa=4097, ws_bytes=1 << 40, a=P + 4) == UNSUPPORTED                # refused before the alignment is looked at
    assert dtw(L, Fa=4096, Fb=4096, a=P + 4) == ALIGN                               # 4096 is accepted up to the alignment check
    assert dtw(L, Fa=4096, Fb=4097, ws_bytes=1 << 40, a=P + 4) == UNSUPPORTED


def test_f0_stats_statuses_before_any_launch(built):
    from glow_tts_amd import _lib
    L = _lib.lib()
    for kw in ({"path": None}, {"path_len": None}, {"fa": None}, {"fb": None}, {"counts": None}, {"sums": None}, {"B": 0}, {"B": -1},
               {"B": 65536}, {"ld": 0}, {"ld": -1}, {"ld_a": 0}, {"ld_b": 0}, {"ld_b": -3}):
        assert f0(L, **kw) == INVAL, kw
    for kw in ({"path": P + 4}, {"path_len": P + 2}, {"fa": P + 2}, {"fb": P + 1}, {"counts": P + 2}, {"sums": P + 3}):
        assert f0(L, **kw) == ALIGN, kw
    assert f0(L, B=0, path=P + 4) == INVAL
