"""CPU tests of the denoiser's float64 restatement (tests/denoise64.py) and of the claims its error bound rests on: strength 0 is the
identity (to 1e-12 with the window's float64 envelope; gl64.inverse divides by the reference's float32 one), the form the kernel writes (Y = X max(|X| - c, 0) / |X|) IS the reference's polar route (digital silence included, where
atan2(0, 0) = 0), the geometry rule of the analysis behind a vocoder, and the shrinkage's non-expansiveness in X and in c."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import denoise64 as D  # noqa: E402
import gl64 as G  # noqa: E402
import mel64  # noqa: E402


def bias_for_tests(seed=7):
    return (np.random.default_rng(seed).uniform(0.0, 4.0, D.NBIN)).astype(np.float32)


def test_strength_zero_returns_the_signal():
    for name in mel64.SIGNALS:
        x = mel64.signal(name, 256 * 6).astype(np.float64)
        out = D.denoise64(x, bias_for_tests(), 0.0)
        assert np.array_equal(out["re"], out["X"][0]) and np.array_equal(out["im"][1:-1], out["X"][1][1:-1]), name
        # the inverse with the window's float64 envelope returns the signal to 1e-12; the reference's envelope is a float32 buffer
        # (window_sumsquare, gl64.envelope32), whose rounding alone moves a sample by up to 4 u |x| (gl64.C_RECON's term)
        F = out["re"].shape[1]
        raw = G.inverse(out["re"], out["im"], envelope=False) / G.SCALE
        env = np.zeros(D.N + D.HOP * (F - 1))
        for f in range(F):
            env[f * D.HOP:f * D.HOP + D.N] += mel64.window64() ** 2
        assert np.abs(raw / env[D.N // 2:-(D.N // 2)] * G.SCALE - x).max() <= 1e-12, name
        assert (np.abs(out["wav"] - x) <= 4 * D.U * np.abs(x) + 1e-12).all(), name


def test_the_kernels_form_is_the_polar_route():
    bias = bias_for_tests()
    for name in mel64.SIGNALS:
        x = mel64.signal(name, 256 * 7).astype(np.float64)
        x[256 * 2:256 * 6] = 0.0                                                            # frames 4 is digital silence: X = 0 exactly
        for strength in (0.0, 0.1, 10.0):
            a, b = D.denoise64(x, bias, strength), D.denoise64(x, bias, strength, route=D.polar)
            assert not np.hypot(*a["X"])[:, 4].any()
            for k in ("re", "im", "wav"):
                assert np.abs(a[k] - b[k]).max() <= 1e-12, (name, strength, k)
            assert not a["re"][:, 4].any() and not a["im"][:, 4].any()                      # (max(-c, 0), 0) = 0 for c >= 0


def test_geometry_rule():
    want = {(0, 0): 0, (0, 1): 2, (0, 2): 3, (0, 5): 6, (1, 0): 0, (1, 1): 0, (1, 2): 2, (1, 5): 5}
    for (lost, n), Fa in want.items():
        assert D.analysis_frames(n, lost) == Fa, (lost, n)
    assert D.analysis_frames(9, 0, F_max=5) == 6 and D.analysis_frames(9, 1, F_max=5) == 5   # the capacity clamps n first
    assert D.analysis_frames(-3, 0) == 0


def test_shrinkage_is_non_expansive():
    """|shrink(X, c) - shrink(X', c')| <= |X - X'| + |c - c'| for c, c' >= 0: what carries the DFT's error and c's rounding into Y"""
    rng = np.random.default_rng(11)
    n = 200000
    scale = 10.0 ** rng.uniform(-6, 2, n)
    X = (rng.standard_normal(n) + 1j * rng.standard_normal(n)) * scale
    X2 = X + (rng.standard_normal(n) + 1j * rng.standard_normal(n)) * scale * 10.0 ** rng.uniform(-8, 0.5, n)
    c = np.abs(X) * 10.0 ** rng.uniform(-3, 1, n)                                           # both sides of the clamp
    c2 = c * (1.0 + rng.uniform(-1, 1, n) * 10.0 ** rng.uniform(-8, 0, n))
    X[:100], c[100:200] = 0.0, 0.0

    def sh(z, cc):
        re, im = D.shrink(z.real, z.imag, cc)
        return re + 1j * im
    slack = 1e-14 * (np.abs(X) + np.abs(X2) + c)
    assert (np.abs(sh(X, c) - sh(X2, c)) <= np.abs(X - X2) + slack).all()
    assert (np.abs(sh(X, c) - sh(X, c2)) <= np.abs(c - c2) + slack).all()
    assert (np.abs(sh(X, c) - sh(X2, c2)) <= np.abs(X - X2) + np.abs(c - c2) + slack).all()
    assert ((np.abs(X) > c).mean() > 0.2) and ((np.abs(X) <= c).mean() > 0.2)
