"""CPU tests of tests/gl_mel64.py, the float64 restatement the GPU tests of the mel-inversion kernel (csrc/gl_mel.hip, DESIGN.md
4.21) rely on: the restated phase generator, an fp32 emulation of the kernel's chain inside the counted bound, and three classic
mistakes that each break it — so the bound is neither violated by a correct fp32 kernel nor wide enough to hide a wrong one."""
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gl_mel64 as G  # noqa: E402
import mel64 as M  # noqa: E402


@functools.lru_cache(maxsize=None)
def operands():
    """(pinv32 [513, 80], mel32 [80, 40]): the float64 pseudo-inverse of the Slaney bank rounded once, and the log-mel of 20 frames
    of the chirp and 20 of loud_quiet as the mel front end defines it, rounded to fp32"""
    from glow_tts_amd import audio
    mb = audio.mel_filterbank(22050, 1024, 80, 0.0, 8000.0)
    pinv = np.linalg.pinv(mb.astype(np.float64)).astype(np.float32)
    mel = np.concatenate([M.mel64(M.signal(n, M.HOP * 19), mb)["mel"] for n in ("chirp", "loud_quiet")], axis=1).astype(np.float32)
    assert pinv.shape == (513, 80) and mel.shape == (80, 40)
    return pinv, mel


def test_counts():
    assert (G.c_mag(80), G.c_spec(80), G.c_mag(37), G.c_spec(37)) == (85, 90, 42, 47)
    assert G.PHASE_STREAM == 4 and G.U == 2.0 ** -24


def test_phase_generator_restated():
    t = G.phase_t(5, 0, 70)
    u = G.phase_u(G.phase_hash(5, 0, np.arange(70)[None, :], np.arange(513)[:, None]))
    assert t.shape == (513, 70) and u.min() > 0.0 and u.max() < 1.0
    assert np.array_equal(t, 2.0 * u - 1.0)
    t32 = t.astype(np.float32)
    assert np.array_equal(t32.astype(np.float64), t)                          # exact in fp32 ...
    u32 = ((G.phase_hash(5, 0, np.arange(70)[None, :], np.arange(513)[:, None]) >> np.uint32(9)).astype(np.float32) + np.float32(0.5)) \
        * np.float32(2.0 ** -23)
    assert np.array_equal(np.float32(2.0) * u32 - np.float32(1.0), t32)       # ... and what the kernel's fp32 expression gives
    assert np.abs(t).max() < 1.0 and np.abs(t).min() >= 2.0 ** -23            # an odd integer over 2^23: never 0, never +-1
    # streams 0..4, utterances and seeds give different draws
    draws = [G.phase_t(5, 0, 8, stream=s) for s in range(5)] + [G.phase_t(5, 1, 8), G.phase_t(6, 0, 8)]
    for i in range(len(draws)):
        for k in range(i + 1, len(draws)):
            assert (draws[i] != draws[k]).mean() > 0.99, (i, k)
    assert np.array_equal(G.phase_t(5, 0, 8), draws[4]) and np.array_equal(G.phase_t(5, 0, 70)[:, :8], draws[4])


def test_phase_generator_is_uniform():
    n = 100000
    u = G.phase_u(G.phase_hash(11, 3, np.arange(n // 500)[None, :], np.arange(500)[:, None])).reshape(-1)
    assert u.size == n
    # a uniform on (0, 1): mean 1/2 with sigma sqrt(1 / 12 n), variance 1/12 with sigma sqrt(1 / 180 n)
    assert abs(u.mean() - 0.5) < 4.0 * np.sqrt(1.0 / (12.0 * n))
    assert abs(u.var() - 1.0 / 12.0) < 4.0 * np.sqrt(1.0 / (180.0 * n))


def test_fp32_chain_is_inside_the_bound():
    pinv, mel = operands()
    e32 = np.exp(mel.astype(np.float64)).astype(np.float32)                   # a correctly rounded expf: inside its 2 ulp
    got = G.chain32(pinv, e32).astype(np.float64)
    err, bound = np.abs(got - G.mag64(pinv, mel)), G.mag_bound(pinv, mel)
    print(f"fp32 chain: worst share of the bound {(err / np.maximum(bound, 1e-300)).max():.4f}")
    assert (err <= bound).all()                                               # bins above the bank's last filter: 0 <= 0
    t = G.phase_t(7, 0, mel.shape[1])
    t32 = t.astype(np.float32)
    cs, sn = np.cos(np.pi * t32.astype(np.float64)).astype(np.float32), np.sin(np.pi * t32.astype(np.float64)).astype(np.float32)
    re, im = (got.astype(np.float32) * cs).astype(np.float64), (got.astype(np.float32) * sn).astype(np.float64)
    im[512] = 0.0
    rre, rim = G.spectrum64(G.mag64(pinv, mel), t)
    sb = G.spec_bound(pinv, mel)
    assert (np.abs(re - rre) <= sb).all() and (np.abs(im - rim) <= sb).all()


def test_three_mistakes_break_the_bound():
    pinv, mel = operands()
    ref, bound = G.mag64(pinv, mel), G.mag_bound(pinv, mel)
    e32 = np.exp(mel.astype(np.float64)).astype(np.float32)
    # exp omitted
    assert (np.abs(G.chain32(pinv, mel).astype(np.float64) - ref) > bound).mean() >= 0.5
    # the clamp omitted: counted where the sum is negative — and the test signal has such entries (about 3 %)
    raw = G.chain32(pinv, e32, clamp=False).astype(np.float64)
    neg = pinv.astype(np.float64) @ np.exp(mel.astype(np.float64)) < 0
    print(f"negative least-squares magnitudes: {neg.mean():.4f} of the entries")
    assert neg.mean() >= 0.01
    assert (np.abs(raw - ref) > bound)[neg].mean() >= 0.5
    # mel_pinv read with the wrong stride ([n_mel, 513] taken for [513, n_mel])
    wrong = np.ascontiguousarray(pinv.reshape(-1).reshape(80, 513).T)
    assert (np.abs(G.chain32(wrong, e32).astype(np.float64) - ref) > bound).mean() >= 0.5
    # ... and transposed products (the chain over the bins' axis cannot even be formed): the first 80 rows stand for it
    assert (np.abs(G.chain32(np.ascontiguousarray(pinv[:80].T), e32).astype(np.float64) - ref[:80]) > bound[:80]).mean() >= 0.5
