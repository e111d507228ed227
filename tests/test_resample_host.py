"""CPU tests of the resampler's definition (glow_tts_amd.audio.resample_filter64 / resample_bank64, tests/resample64.py).

  * the float64 direct form equals scipy.signal.resample_poly's recorded outputs (tests/golden/resample_poly_scipy.npz: five rate
    pairs, L in {1, 5, down + 1, 700}) to 1e-12, and a live resample_poly call where scipy imports;
  * audio.resample_filter64 equals scipy's firwin(...) * up (recorded, and live where scipy imports) to 1e-15 of the filter's largest
    tap — per tap a relative figure means nothing at the sinc's zero crossings, where both hold rounding noise around 0 — and the
    restatement in tests/resample64.py to the same;
  * a float32 evaluation in tap order (resample64.twin32) stays inside the bound the GPU test uses;
  * four planted defects leave it, on 1531 noise samples per pair.  Worst err / bound per pair, the smallest .. the
    largest of the five pairs' figures:
        float32 twin                        0.07 .. 0.20
        bank index + 1 upsampled sample     3.2e3 .. 6.1e5
        no * up gain                        3.3e5 .. 7.3e5   (44 100 -> 22 050 Hz has up = 1: nothing to plant)
        clamped instead of zero edges       7.0e4 .. 2.6e5
        floor instead of ceil in n_out      1.1e4 .. 6.3e5   (the missing last output counted as 0; L up / down is no integer)"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import resample64 as R  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "resample_poly_scipy.npz")
L_DEFECT = 1531

try:
    from scipy import signal as sp_signal
except ImportError:                                                                # the recorded outputs stand in
    sp_signal = None


@pytest.fixture(scope="module")
def golden():
    g = np.load(GOLDEN)
    return {k: g[k] for k in g.files}


def operands(orig, new):
    """(up, down, fp32 bank as the module carries it, fp32 noise) for the defect tests"""
    from glow_tts_amd import audio
    up, down = R.ratio(orig, new)
    return up, down, audio.resample_bank64(up, down).astype(np.float32), R.signal("noise", L_DEFECT, orig, new)


def worst(err, mag, T):
    return float((err / R.bound(mag, T)).max())


def test_direct_form_equals_scipy(golden):
    from glow_tts_amd import audio
    for orig, new in R.PAIRS:
        up, down = R.ratio(orig, new)
        bank = audio.resample_bank64(up, down)
        assert bank.shape == (up, R.TAPS[(orig, new)])
        for tag in R.GOLDEN_LENGTHS:
            x, want = golden[f"{orig}_{new}_{tag}_x"], golden[f"{orig}_{new}_{tag}_y"]
            assert len(x) == R.golden_length(tag, down) and len(want) == R.n_out(len(x), up, down)
            got, _ = R.direct(x, bank, up, down)
            assert np.abs(got - want).max() <= 1e-12, (orig, new, tag)
            if sp_signal is not None:
                assert np.abs(got - sp_signal.resample_poly(x, up, down)).max() <= 1e-12, (orig, new, tag)


def test_filter_equals_firwin(golden):
    from glow_tts_amd import audio
    for orig, new in R.ALL_PAIRS:
        up, down = R.ratio(orig, new)
        h = audio.resample_filter64(up, down)
        m = max(up, down)
        assert h.dtype == np.float64 and h.shape == (20 * m + 1,) and abs(h.sum() - up) <= 1e-12 * up
        assert np.array_equal(audio.resample_filter64(new, orig), h)               # reduced first
        refs = [R.filter64(up, down)]
        if (orig, new) in R.PAIRS:
            refs.append(golden[f"{orig}_{new}_h"])
        if sp_signal is not None:
            refs.append(sp_signal.firwin(20 * m + 1, 1.0 / m, window=("kaiser", 5.0)) * up)
        for ref in refs:
            assert np.abs(h - ref).max() <= 1e-15 * np.abs(ref).max(), (orig, new)
        bank = audio.resample_bank64(up, down)
        T = bank.shape[1]
        assert T == -(-len(h) // up) == R.TAPS[(orig, new)] and np.array_equal(bank, R.bank64(h, up))
        flat = bank.T.reshape(-1)
        assert np.array_equal(flat[:len(h)], h) and not flat[len(h):].any()


def test_out_len_and_length_for():
    from glow_tts_amd import audio
    for orig, new in R.ALL_PAIRS:
        up, down = R.ratio(orig, new)
        for L in (0, 1, 5, down - 1, down, down + 1, 700, 1531, 1 << 28):
            assert audio.resample_out_len(L, up, down) == R.n_out(L, up, down) == (L * up + down - 1) // down
        for m in (1, 5, 511, 512, 513, 1027):
            L = R.length_for(m, up, down)
            assert R.n_out(L, up, down) >= m and (L == 1 or R.n_out(L - 1, up, down) < m)
            if up <= down:
                assert R.n_out(L, up, down) == m


def test_float32_twin_is_inside_the_bound():
    for orig, new in R.PAIRS:
        up, down, bank, x = operands(orig, new)
        y64, mag = R.direct(x, bank, up, down)
        w = worst(np.abs(R.twin32(x, bank, up, down).astype(np.float64) - y64), mag, bank.shape[1])
        print(f"{orig}->{new}: float32 twin worst err / bound {w:.3f}")
        assert w <= 1.0, (orig, new, w)


def test_planted_defects_are_outside_the_bound():
    for orig, new in R.PAIRS:
        up, down, bank, x = operands(orig, new)
        T = bank.shape[1]
        y64, mag = R.direct(x, bank, up, down)
        assert (L_DEFECT * up) % down                                               # n_out is a true ceiling here
        short = np.append(R.direct(x, bank, up, down, count=L_DEFECT * up // down)[0], 0.0)
        defects = {"bank index + 1": R.direct(x, bank, up, down, index_shift=1)[0],
                   "no * up gain": R.direct(x, bank / np.float32(up), up, down)[0],
                   "clamped edges": R.direct(x, bank, up, down, edges="clamp")[0],
                   "floor in n_out": short}
        for name, y in defects.items():
            if name == "no * up gain" and up == 1:
                continue                                                            # the gain is 1: nothing to plant
            w = worst(np.abs(y - y64), mag, T)
            print(f"{orig}->{new}: {name}: worst err / bound {w:.3g}")
            assert w > 1.0, (orig, new, name, w)
