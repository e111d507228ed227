"""CPU tests of the synthesis metrics' definitions (tests/dtw64.py, glow_tts_amd.metrics): the float64 oracle against
brute-force enumeration of every monotone path, the DCT matrix against scipy, the cepstrum's blindness to a gain, the tie rule on a
hand-made lattice, the path checker on broken paths, a float32 emulation of the kernel's arithmetic against the DTW bound, and
f0_errors' arithmetic against a direct NumPy restatement."""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dtw64 as R  # noqa: E402


def all_paths(Fa, Fb):
    """every path from (0, 0) to (Fa-1, Fb-1) by steps (1, 1), (1, 0), (0, 1)"""
    def walk(i, j):
        if (i, j) == (Fa - 1, Fb - 1):
            yield [(i, j)]
            return
        for di, dj in ((1, 1), (1, 0), (0, 1)):
            if i + di < Fa and j + dj < Fb:
                for rest in walk(i + di, j + dj):
                    yield [(i, j)] + rest
    return walk(0, 0)


def test_oracle_against_brute_force_enumeration():
    rng = np.random.RandomState(0)
    for Fa in range(1, 5):
        for Fb in range(1, 6):
            d = rng.rand(Fa, Fb)
            cost, path = R.dtw64(d)
            best = min(R.path_cost64(d, p) for p in all_paths(Fa, Fb))
            assert abs(cost - best) <= 1e-12 * max(best, 1.0), (Fa, Fb)
            assert abs(R.path_cost64(d, path) - cost) <= 1e-12 * max(cost, 1.0)
            rows = np.full((Fa + Fb + 1, 2), -1)
            rows[:len(path)] = path
            R.check_path(rows, len(path), Fa, Fb)
    assert R.dtw64(np.zeros((0, 3))) == (0.0, []) and R.dtw64(np.zeros((3, 0))) == (0.0, [])


def test_tie_rule_on_a_hand_made_lattice():
    """all distances equal: every predecessor ties and the diagonal wins until a border; then (i-1, j) or (i, j-1), the only one"""
    _, path = R.dtw64(np.ones((3, 5)))
    assert path == [(0, 0), (0, 1), (0, 2), (1, 3), (2, 4)]                     # back from the end: diagonal twice, then along row 0
    _, path = R.dtw64(np.ones((5, 3)))
    assert path == [(0, 0), (1, 0), (2, 0), (3, 1), (4, 2)]
    # D(1, 1): the diagonal 1 and (0, 1) = 1 tie -> the diagonal; D(2, 1): the diagonal D(1, 0) = 2 and (1, 1) = 2 tie -> the diagonal
    d = np.array([[1.0, 0.0], [1.0, 1.0], [5.0, 1.0]])
    cost, path = R.dtw64(d)
    assert cost == 3.0 and path == [(0, 0), (1, 0), (2, 1)]
    # (i-1, j) before (i, j-1): D(1, 1) with the diagonal 3, (0, 1) = 1 and (1, 0) = 1
    d = np.array([[3.0, -2.0], [-2.0, 1.0]])
    cost, path = R.dtw64(d)
    assert cost == 2.0 and path == [(0, 0), (0, 1), (1, 1)]


def test_path_checker_refuses_broken_paths():
    good = np.array([[0, 0], [1, 1], [1, 2], [-1, -1]])
    R.check_path(good, 3, 2, 3)
    for bad, n in ((np.array([[0, 0], [1, 2], [-1, -1], [-1, -1]]), 2), (np.array([[0, 1], [1, 1], [1, 2], [-1, -1]]), 3),
                   (np.array([[0, 0], [1, 1], [1, 2], [0, 0]]), 3), (np.array([[0, 0], [0, 0], [1, 1], [1, 2]]), 4),
                   (np.array([[0, 0], [1, 1], [0, 2], [1, 2]]), 4)):
        with pytest.raises(AssertionError):
            R.check_path(bad, n, 2, 3)


def test_dct_matrix_against_scipy_and_the_module():
    from scipy.fft import dct
    from glow_tts_amd import metrics
    for N, K in ((80, 13), (100, 16), (128, 1)):
        w = R.dct_matrix(N, K)
        m = np.random.RandomState(N).randn(N, 7)
        want = dct(m, type=2, norm="ortho", axis=0)[1:K + 1]
        assert np.abs(w @ m - want).max() < 1e-12
        assert np.array_equal(metrics.dct_matrix64(N, K), w)
        mod = metrics.MelCepstrum(N, K)
        assert [k for k, _ in mod.named_buffers()] == ["dct"] and not list(mod.parameters())
        assert mod.dct.dtype == torch.float32 and np.array_equal(mod.dct.numpy(), w.astype(np.float32))
    assert metrics.ALPHA_DB == R.ALPHA_DB == 10.0 * math.sqrt(2.0) / math.log(10.0)
    with pytest.raises(ValueError):
        metrics.MelCepstrum(129, 13)
    with pytest.raises(ValueError):
        metrics.MelCepstrum(80, 17)


def test_a_gain_in_the_log_domain_costs_nothing():
    w = R.dct_matrix(80, 13).astype(np.float32)
    mel = np.random.RandomState(1).randn(80, 9).astype(np.float32) * 2 - 5
    c, bound = R.cepstrum64(mel, w)
    c3, bound3 = R.cepstrum64(mel + np.float32(3.0), w)
    assert (np.abs(c - c3) <= 80 * 3.0 * 2.0 ** -24).all()                      # the fp32 rows sum to zero to their own rounding
    assert (bound > 0).all() and (bound3 >= bound * 0.1).all()


def test_float32_emulation_sits_inside_the_dtw_bound():
    """the kernel's arithmetic restated in float32 (dist32_along over the float64-optimal path) against D64: far inside delta"""
    for Fa, Fb, seed in ((65, 63, 1), (130, 65, 2)):
        a, b = R.warped_pair(Fa, Fb, 13, seed)
        d = R.dist64(a, b, R.ALPHA_DB)
        cost, path = R.dtw64(d)
        assert len(path) > max(Fa, Fb)                                           # the warp puts the path off the diagonal
        got = float(R.dist32_along(a, b, path, R.ALPHA_DB))
        assert abs(got - cost) <= R.dtw_delta(Fa, Fb) * cost


def test_f0_errors_arithmetic():
    from glow_tts_amd import metrics
    rng = np.random.RandomState(3)
    fa = np.where(rng.rand(40) < 0.7, rng.uniform(80, 300, 40), 0).astype(np.float32)
    fb = np.where(rng.rand(50) < 0.7, rng.uniform(80, 300, 50), 0).astype(np.float32)
    _, path = R.dtw64(rng.rand(40, 50))
    n_vv, n_vu, n_gross, s_hz, s_ct = R.f0_stats64(fa, fb, path)
    assert n_vv > 5 and n_vu > 5 and 0 < n_gross < n_vv
    counts = torch.tensor([[n_vv, n_vu, n_gross], [0, 4, 0], [0, 0, 0]], dtype=torch.int32)
    sums = torch.tensor([[s_hz, s_ct], [0.0, 0.0], [0.0, 0.0]], dtype=torch.float32)
    plen = torch.tensor([len(path), 9, 0], dtype=torch.int32)
    m = metrics.f0_metrics_from_stats(counts, sums, plen)
    assert abs(m["rmse_hz"][0].item() - math.sqrt(s_hz / n_vv)) < 1e-4 * math.sqrt(s_hz / n_vv)
    assert abs(m["rmse_cents"][0].item() - math.sqrt(s_ct / n_vv)) < 1e-4 * math.sqrt(s_ct / n_vv)
    assert abs(m["vde"][0].item() - n_vu / len(path)) < 1e-6 and abs(m["gpe"][0].item() - n_gross / n_vv) < 1e-6
    assert m["n_voiced"].tolist() == [n_vv, 0, 0]
    for k in ("rmse_hz", "rmse_cents", "gpe"):                                   # n_vv = 0: NaN
        assert math.isnan(m[k][1].item()) and math.isnan(m[k][2].item())
    assert abs(m["vde"][1].item() - 4 / 9) < 1e-6 and math.isnan(m["vde"][2].item())
    # the restatement itself on a case done by hand: steps (100, 100), (120, 100), (0, 100), (0, 0)
    got = R.f0_stats64(np.array([100, 120, 0, 0], np.float32), np.array([100, 100, 100, 0], np.float32), [(0, 0), (1, 1), (2, 2), (3, 3)])
    assert got[:3] == (2, 1, 0) and got[3] == 400.0 and abs(got[4] - (1200 * math.log2(1.2)) ** 2) < 1e-9
    assert R.f0_stats64(np.array([121], np.float32), np.array([100], np.float32), [(0, 0)])[2] == 1


def test_cpu_tensors_raise():
    from glow_tts_amd import _lib, metrics
    x = torch.zeros(1, 4, 16)
    with pytest.raises(_lib.CpuTensorError):
        metrics.dtw(x, None, x, None)
    with pytest.raises(_lib.CpuTensorError):
        metrics.MelCepstrum()(torch.zeros(1, 80, 4))
    with pytest.raises(_lib.CpuTensorError):
        metrics.mcd_dtw(torch.zeros(1, 80, 4), None, torch.zeros(1, 80, 4), None)
