"""CPU tests of the waveform back end's host side (glow_tts_amd.audio.InverseSTFT) and of its float64 oracle
tests/gl64.py: the inverse basis is the reference's pinv(4 fourier_basis).T times the window, the module's buffer is that matrix
rounded once and exactly mirror-symmetric (the kernel's fold relies on it), the oracle's round trip reproduces a signal to the rounding
of the reference's float32 envelope, the oracle tells the three classic mistakes apart at the GPU test's own bound, and the STFT /
TacotronSTFT buffer sets are what they were."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gl64 as G  # noqa: E402
import mel64 as M  # noqa: E402


def test_gl64_inverse_basis_is_the_pseudo_inverse_times_the_window():
    closed, pinv = G.inverse_basis64(), G.pinv_basis64()
    assert closed.shape == pinv.shape == (1026, 1024)
    err = np.abs(closed - pinv).max()
    print(f"closed form vs float64 pinv: max |diff| {err:.3e} (largest entry {np.abs(closed).max():.3e})")
    assert err <= 1e-15                                    # entries are at most 2 / 4096 = 4.9e-4: 2e-12 of that


def test_inverse_stft_buffer_is_that_matrix_rounded_once_and_mirror_symmetric():
    from glow_tts_amd import audio
    mod = audio.InverseSTFT()
    assert [n for n, _ in mod.named_buffers()] == ["inverse_basis"] and not list(mod.parameters())
    ib = mod.inverse_basis
    assert ib.shape == (1026, 1, 1024) and ib.dtype == torch.float32
    b = ib[:, 0].numpy()
    assert np.array_equal(b, G.inverse_basis64().astype(np.float32))
    assert np.array_equal(b[:513, 1:], b[:513, :0:-1])     # cos rows even about sample 512
    assert np.array_equal(b[513:, 1:], -b[513:, :0:-1])    # sin rows odd
    assert not b[:, 0].any() and not b[513].any() and not b[1025].any() and not b[513:, 512].any()
    assert np.array_equal(b[0] * 4096.0, M.window64().astype(np.float32))   # the kernel takes the envelope's window from row 0


def test_gl64_round_trip_reproduces_every_kept_sample():
    worst = 0.0
    for name, L in zip(M.SIGNALS, (768, 1024, 4864, 256 * 63, 256 * 65)):
        x = M.signal(name, L).astype(np.float64)
        y = G.inverse(*G.transform(x))
        assert y.shape == x.shape
        # only the float32 envelope is inexact: 4 roundings of a value in [1.25, 1.5] = 4 u relative, plus float64 dust
        err = np.abs(y - x)
        worst = max(worst, (err / np.maximum(np.abs(x), 1e-3)).max())
        assert (err <= 4 * G.U * np.abs(x) + 1e-12).all(), name
    print(f"round trip: worst relative error {worst:.2e}")


def test_gl64_tells_the_three_classic_mistakes_apart():
    """each of them breaks the per-sample bound the GPU test holds the kernel to, on every signal"""
    for name in M.SIGNALS:
        x = M.signal(name, 4864)
        re, im = G.transform(x)
        re, im = re.astype(np.float32).astype(np.float64), im.astype(np.float32).astype(np.float64)
        good, bound = G.inverse(re, im), G.istft_bound(re, im)
        wrong = {"no envelope division": G.inverse(re, im, envelope=False),
                 "bins 1..511 weighted like 0 and 512": G.inverse(re, im, basis=G.flat_weight_basis()),
                 "imaginary sign flipped": G.inverse(re, im, imag_sign=-1.0)}
        if name == "dc_nyquist":                              # w x is even about every frame's centre: the spectrum is real, and
            assert np.abs(im).max() < 1e-12                   # a flipped sign of nothing is no mistake
            del wrong["imaginary sign flipped"]
        for what, y in wrong.items():
            assert (np.abs(y - good) > bound).mean() >= 0.5, (name, what)      # dc_nyquist is 0 at every other sample: exactly half


def test_stft_and_tacotron_buffers_are_unchanged():
    from glow_tts_amd import audio
    assert [n for n, _ in audio.STFT().named_buffers()] == ["forward_basis"]
    assert sorted(n for n, _ in audio.TacotronSTFT().named_buffers()) == ["mel_basis", "stft_fn.forward_basis"]
    gl = audio.GriffinLim(audio.TacotronSTFT())
    assert sorted(n for n, _ in gl.named_buffers()) == ["istft.inverse_basis", "stft.mel_basis", "stft.stft_fn.forward_basis"]
    assert sorted(n for n, _ in gl.stft.named_buffers()) == ["mel_basis", "stft_fn.forward_basis"]
