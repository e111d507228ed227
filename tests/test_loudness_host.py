"""CPU tests of the BS.1770-4 definition the loudness kernels are held to (tests/loudness64.py) and of the float64
images audio.py hands them: the K-weighting coefficients against the recommendation's 48 kHz table, the oracle's filter against
scipy.signal.lfilter, the recommendation's own calibration (a full-scale 997 Hz sine reads -3.01 LKFS), the scale law, the chunked
decomposition (zero-state pass, transition scan, second pass) against the serial filter for three chunk lengths, the two gates on a
constructed signal, the one-block rule below 400 ms, silence, and the peak rule."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import loudness64 as L  # noqa: E402

RATES = (16000, 22050, 24000, 44100, 48000)


def test_kweighting64_equals_the_recommendations_table(built):
    from glow_tts_amd import audio
    (b, a), (c, d) = audio.kweighting64(48000)
    assert np.abs(b - np.array(L.TABLE_48K[0])).max() <= 1e-10 and np.abs(a[1:] - np.array(L.TABLE_48K[1])).max() <= 1e-10
    assert np.abs(d[1:] - np.array(L.TABLE_48K[2])).max() <= 1e-10 and a[0] == d[0] == 1.0 and c.tolist() == [1.0, -2.0, 1.0]
    for fs in RATES:                                       # the package's images are the oracle's own restatement of the formulas
        for got, want in zip(audio.kweighting64(fs), L.kweighting(fs)):
            assert np.allclose(got[0], want[0], rtol=1e-14, atol=0) and np.allclose(got[1], want[1], rtol=1e-14, atol=0)


def test_transition_matrix_is_the_filters_own(built):
    from glow_tts_amd import audio
    for fs, chunk in zip(RATES, (50, 49, 50, 49, 50)):
        assert audio.loudness_chunk(fs) == chunk and (fs // 10) % chunk == 0
        for n in (1, chunk, 16 * chunk):
            # the oracle's is a float64 product of n factors: its own roundings, amplified by the cancellation in the high-pass's
            # near-double pole, reach 1e-10 of the largest entry by n = 800; the package's is the exact power rounded once
            M, want = audio.kweighting_transition64(fs, n), L.transition(fs, n)
            assert np.abs(M - want).max() <= 1e-9 * np.abs(want).max(), (fs, n)
        one = audio.kweighting_transition64(fs, 1)
        assert np.array_equal(one, L.transition(fs, 1))                            # one step: the coefficients themselves
        M, M2 = audio.kweighting_transition64(fs, chunk), audio.kweighting_transition64(fs, 2 * chunk)
        assert np.abs(M @ M - M2).max() <= 1e-13 * np.abs(M2).max()
    assert audio.kweighting_transition64(22050, 0).tolist() == np.eye(4).tolist()
    for fs in (22051, 7990, 200000, 10 * 1009, 44100.5):   # no multiple of 10, out of range, a prime tenth
        assert audio.loudness_chunk(fs) == 0
        with pytest.raises(ValueError):
            audio.Loudness(fs)


def test_oracle_filter_equals_scipy_lfilter():
    signal = pytest.importorskip("scipy.signal")
    for fs in (22050, 48000):
        x = L.burst(3 * fs // 10 + 17, fs, 1).astype(np.float64)
        (b, a), (c, d) = L.kweighting(fs)
        want = signal.lfilter(c, d, signal.lfilter(b, a, x))
        assert np.abs(L.kfilter(x, fs) - want).max() <= 1e-12 * np.abs(want).max()


def test_full_scale_997_hz_sine_reads_minus_3_01_lkfs():
    fs = 48000
    x = np.sin(2.0 * np.pi * 997.0 * np.arange(5 * fs) / fs)
    assert abs(L.loudness64(x, fs)["L"] - (-3.01)) <= 0.01


def test_scaling_the_input_moves_L_by_exactly_the_gain():
    for fs, N in ((22050, 30000), (16000, 9000), (22050, 3000)):
        x = L.burst(N, fs, 2).astype(np.float64)
        z = L.kfilter(x, fs)
        base = L.loudness64(x, fs, z=z)["L"]
        for d in (-17.5, 6.0):
            k = 10.0 ** (d / 20.0)
            assert abs(L.loudness64(k * x, fs, z=k * z)["L"] - (base + d)) <= 1e-9      # the filter is linear: z scales with x
            assert abs(L.loudness64(k * x, fs)["L"] - (base + d)) <= 1e-9              # and filtered anew


@pytest.mark.parametrize("fs,N", ((22050, 3 * 2205 + 1234), (48000, 5017)))
def test_chunked_decomposition_equals_the_serial_filter(built, fs, N):
    from glow_tts_amd import audio
    x = L.burst(N, fs, 3).astype(np.float64)
    z = L.kfilter(x, fs)
    own = audio.loudness_chunk(fs)
    assert N % own and N > 16 * own
    for Lc in (own, 1, N + 7):
        assert np.abs(L.chunked(x, fs, Lc) - z).max() <= 1e-12 * np.abs(z).max(), Lc
    assert np.abs(L.chunked(x, fs, own, drop_state=True) - z).max() > 1e-3 * np.abs(z).max()       # the scan matters
    # the same with the matrices the kernels read: M over the chunk, and M^16 over a run of 16 chunks.  STATES are compared here, the
    # high-pass's pair nearly cancels (t1 = -t2 to three digits) and the serial filter's own rounding noise on them is its noise gain
    # (1e4 - 1e5) times 2^-53: 1e-10 of the largest state is what float64 can promise
    M, M16 = audio.kweighting_transition64(fs, own), audio.kweighting_transition64(fs, 16 * own)
    _, s = L.kfilter(x[:16 * own], fs, want_state=True)
    e, acc = [L.kfilter(x[k * own:(k + 1) * own], fs, want_state=True)[1] for k in range(16)], np.zeros(4)
    for k in range(16):
        acc = M @ acc + np.array(e[k])
    assert np.abs(acc - np.array(s)).max() <= 1e-10 * np.abs(s).max()
    _, s32 = L.kfilter(x[:32 * own], fs, want_state=True)
    _, r = L.kfilter(x[16 * own:32 * own], fs, want_state=True)
    assert np.abs(M16 @ np.array(s) + np.array(r) - np.array(s32)).max() <= 1e-10 * np.abs(s32).max()


def tone(fs, seconds, dbfs, hz=1000.0):
    return 10.0 ** (dbfs / 20.0) * np.sin(2.0 * np.pi * hz * np.arange(int(seconds * fs)) / fs)


def test_the_gates_drop_the_quiet_parts():
    fs = 22050
    loud, mid, faint = tone(fs, 2.0, -20.0), tone(fs, 2.0, -50.0), tone(fs, 2.0, -80.0)
    alone = L.loudness64(loud, fs)
    assert abs(alone["L"] - (-20.0 - 3.01)) < 0.1 and L.loudness64(faint, fs)["L"] == -np.inf
    ref = L.loudness64(np.concatenate([loud, mid, faint]), fs)
    l = L.lk(ref["zj"])
    assert ref["J"] == 57 and (l[44:] < -70.0).all() and not ref["A"][44:].any()                    # the absolute gate drops the last
    assert ref["A"][:40].all() and (l[24:40] < ref["gamma"]).all() and not ref["R"][20:].any()     # the relative gate the middle one
    # L is the loud part's level: R is the 17 loud blocks and the three that slide into the middle tone (3/4, 1/2, 1/4 loud)
    assert ref["R"][:20].all() and ref["nR"] == 20 and abs(ref["L"] - (alone["L"] + 10.0 * np.log10(18.5 / 20.0))) < 0.02
    assert abs(L.lk(ref["zj"][:17].mean()) - alone["L"]) < 0.02
    ungated = L.loudness64(np.concatenate([loud, mid, faint]), fs, relative=False)
    assert ungated["L"] < ref["L"] - 2.5


def test_short_utterances_silence_and_the_peak_rule():
    fs = 22050
    x = L.burst(8819, fs, 4).astype(np.float64)
    ref = L.loudness64(x, fs)
    z = L.kfilter(x, fs)
    assert ref["J"] == 1 and len(ref["E"]) == 0 and ref["zj"][0] == np.sum(z * z) / 8819            # one block over all of it
    assert L.loudness64(L.burst(8820, fs, 4), fs)["J"] == 1 and L.loudness64(L.burst(11025, fs, 4), fs)["J"] == 2
    for quiet in (np.zeros(0), np.zeros(5000), np.zeros(30000)):
        ref = L.loudness64(quiet, fs)
        assert ref["L"] == -np.inf and ref["g"] == 1.0 and ref["nA"] == 0 and not ref["engaged"]
    # the peak rule engages exactly when g * peak exceeds the ceiling
    ceil = 10.0 ** (-1.0 / 20.0)
    for Lv, peak in ((-23.0, 0.5), (-30.0, 0.3), (-40.0, 0.2), (-16.0, 0.99)):
        for target in (-23.0, -16.0, -5.0):
            g, engaged = L.gain(Lv, peak, target, -1.0)
            free = 10.0 ** ((target - Lv) / 20.0)
            assert engaged == (free * peak > ceil)
            assert g == (ceil / peak if engaged else free) and g * peak <= ceil * (1 + 1e-15)
    assert L.gain(-23.0, 0.0, -5.0, -1.0) == (10.0 ** (18.0 / 20.0), False)                         # no peak to hold: the rule is off
