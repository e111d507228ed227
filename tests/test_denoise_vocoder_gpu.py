"""GPU tests of audio.Denoised, a vocoder with the spectral-subtraction denoiser behind it, and of Denoiser.from_vocoder (DESIGN.md
4.30), on the TINY WaveGlow of tests/waveglow64.py at frames (0, 1, 2, 3, 5), a small HiFi-GAN and the TINY Vocos (which loses a frame).

The kernels are deterministic and an utterance's samples depend on its own row alone, so the composition is a question of plumbing
(frame counts, `lost`, buffers, the seed), not of tolerance: Denoised(voc)(mel, lengths) must be BIT-IDENTICAL to voc(mel, lengths)
followed by Denoiser.denoise on its output.

The bias.  from_vocoder's bias_spec is frame 0 of |STFT| of the vocoder's own output for a zero mel at sigma = 0; against float64 it is
held in two steps, both derived: (1) within the mel front end's magnitude bound (tests/mel64.py: sqrt(2) d_f + 4 u mag) of the float64
|STFT| of that very output; (2) within that bound plus sqrt(2) ||row_k||_2 * 2 E_emul ||x64||_2 of the float64 |STFT| of the float64 generator's
sigma = 0 output x64 (waveglow64.generator64), the second term being what the bf16 operands may move the samples by — the criterion of
tests/test_waveglow_gpu.py (device error <= 2 E_emul in the 2-norm, E_emul the float64 emulation of the kernels' roundings) carried
through bin k's windowed basis row by Cauchy-Schwarz (sqrt(2): frame 0 holds samples 1 .. 512 twice, reflected)."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "golden"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gl64 as G  # noqa: E402
import mel64  # noqa: E402
import vocos64 as V  # noqa: E402
import waveglow64 as W  # noqa: E402

pytestmark = pytest.mark.gpu
FRAMES = W.TINY_FRAMES
BIAS_FRAMES = 88


def dev():
    return torch.device("cuda:0")


def bits(t):
    return t.contiguous().view(torch.int32)


@functools.lru_cache(maxsize=None)
def waveglow():
    from glow_tts_amd import audio
    return W.init_for_tests(audio.WaveGlow(**W.TINY), 41).to(dev())


@functools.lru_cache(maxsize=None)
def denoised_waveglow():
    from glow_tts_amd import audio
    return audio.Denoised(waveglow())


def composition(voc, den, frames, seed=None, min_frames=1):
    """Denoised(voc) in one call against voc followed by Denoiser.denoise; -> the denoised samples and the plain ones"""
    rng = np.random.default_rng(3)
    C = voc.mel_channels - voc.mel_padding
    mel = torch.from_numpy(np.stack([W.random_mel(rng, C, max(frames)) for _ in frames])).to(dev())
    lengths = torch.tensor(frames, dtype=torch.int32, device=dev())
    kw = {} if seed is None else dict(seed=seed)
    got, got_len = den(mel, lengths, mel_lengths_host=list(frames), **kw)
    plain, plain_len = voc(mel, lengths, mel_lengths_host=list(frames), **kw)
    want, want_len = den.denoiser.denoise(plain, plain_len)
    torch.cuda.synchronize()
    lost = min_frames - 1
    assert got_len.tolist() == plain_len.tolist() == want_len.tolist() == [256 * max(n - lost, 0) for n in frames]
    assert got.shape == plain.shape == want.shape == (len(frames), 256 * (max(frames) - lost))
    assert torch.equal(bits(got), bits(want))
    for b, n in enumerate(got_len.tolist()):
        assert not bool(got[b, n:].any()), b
        if n:
            assert float(got[b, :n].abs().max()) > 0 and not torch.equal(got[b, :n], plain[b, :n]), b   # and the stage does something
    return got, plain


def test_denoised_waveglow_is_the_vocoder_followed_by_the_denoiser(built):
    from glow_tts_amd import _lib
    voc, den = waveglow(), denoised_waveglow()
    assert den.seeded and den.launches == voc.launches + 2 and (den.hop_length, den.min_frames, den.mel_channels) == (256, 1, 80)
    got, _ = composition(voc, den, FRAMES, seed=3)
    assert den(torch.zeros(1, 80, 5, device=dev()), seed=3).shape == (1, 256 * 5)            # no lengths: the samples alone
    with _lib.record_calls() as names:
        den(torch.zeros(2, 80, 5, device=dev()), seed=4)
    names = [n for n in names if not n.endswith("_bytes")]                                  # buffer_spec's size query is no launch
    assert len(names) == den.launches and names[-2:] == ["gt_denoise_spec", "gt_istft"]
    with pytest.raises(ValueError):
        den.set_strength(-0.1)
    with pytest.raises(ValueError):
        den.set_strength(float("nan"))
    from glow_tts_amd.audio import CpuWaveError
    with pytest.raises(CpuWaveError):
        den.denoiser.denoise(torch.zeros(1, 1024))


def test_denoised_hifigan_and_vocos(built):
    from glow_tts_amd import audio
    torch.manual_seed(43)
    hifi = audio.HiFiGAN(upsample_initial_channel=256).to(dev())
    composition(hifi, audio.Denoised(hifi, strength=0.05), (0, 1, 2, 3, 5))
    vocos = V.init_for_tests(audio.Vocos(**V.TINY), 8).to(dev())
    den = audio.Denoised(vocos)
    assert den.min_frames == 2 and not den.seeded
    composition(vocos, den, (0, 1, 2, 3, 5, 70), min_frames=2)                             # lost = 1; 70 frames: a second tile
    with pytest.raises(ValueError):
        den(torch.zeros(1, 80, 4, device=dev()), seed=3)                                    # the inner vocoder draws no latent


def test_a_128_hop_vocoder_is_refused(built):
    from glow_tts_amd import audio
    half = audio.HiFiGAN(upsample_rates=(8, 8, 2), upsample_kernel_sizes=(16, 16, 4), upsample_initial_channel=128).to(dev())
    assert half.hop_length == 128
    with pytest.raises(ValueError):
        audio.Denoised(half)
    with pytest.raises(ValueError):
        audio.Denoised(half, denoiser=audio.Denoiser().to(dev()))
    with pytest.raises(ValueError):
        audio.Denoiser.from_vocoder(half)


def test_from_vocoder_bias_against_float64(built):
    from glow_tts_amd import audio
    voc = waveglow()
    sigma = voc.sigma
    den = audio.Denoiser.from_vocoder(voc, frames=BIAS_FRAMES)
    assert voc.sigma == sigma == W.SIGMA                                                    # restored
    bias = den.bias_spec.double().cpu().numpy()
    assert bias.shape == (G.NBIN,) and np.isfinite(bias).all() and bias.max() > 0
    again = audio.Denoiser.from_vocoder(voc, frames=BIAS_FRAMES)
    assert torch.equal(bits(again.bias_spec), bits(den.bias_spec))
    # (1) the STFT's frame 0 of the vocoder's own sigma = 0 output
    try:
        voc.sigma = 0.0
        own = voc(torch.zeros(1, 80, BIAS_FRAMES, device=dev()))[0].double().cpu().numpy()
    finally:
        voc.sigma = sigma
    ref = mel64.mel64(own, np.zeros((1, G.NBIN)))
    bound = mel64.bounds(ref, np.zeros((1, G.NBIN)))["mag"][:, 0]
    share = (np.abs(bias - ref["mag"][:, 0]) / bound).max()
    print(f"from_vocoder: bias vs float64 |STFT| of the device's own output, worst share of the magnitude bound {share:.4f}")
    assert share <= 1.0
    # (2) the float64 generator's sigma = 0 output
    sd = {k: v.cpu() for k, v in voc.state_dict().items()}
    zero = np.zeros((80, BIAS_FRAMES))
    x64 = W.generator64(sd, W.TINY, zero, 0, 0, sigma=0.0)
    emul = W.generator64(sd, W.TINY, zero, 0, 0, emul=True, sigma=0.0)
    e_emul, e_dev = W.rel_l2(emul, x64), W.rel_l2(own, x64)
    assert 0 < e_emul < 0.05 and e_dev <= 2 * e_emul, (e_dev, e_emul)
    ref64 = mel64.mel64(x64, np.zeros((1, G.NBIN)))
    basis = mel64.basis64()
    row_norm = np.sqrt((basis[:G.NBIN] ** 2).sum(1) + (basis[G.NBIN:] ** 2).sum(1))       # of bin k's complex row
    bound64 = mel64.bounds(ref64, np.zeros((1, G.NBIN)))["mag"][:, 0] + np.sqrt(2.0) * row_norm * 2 * e_emul * np.linalg.norm(x64)
    share64 = (np.abs(bias - ref64["mag"][:, 0]) / bound64).max()
    print(f"from_vocoder: bias vs float64 |STFT| of generator64(sigma=0): E_emul {e_emul:.3e}, device {e_dev:.3e}, worst share {share64:.4f}")
    assert share64 <= 1.0 and np.abs(ref64["mag"][:, 0]).max() > 1e-3


def test_the_bias_follows_the_vocoders_parameters(built):
    from glow_tts_amd import audio
    voc = W.init_for_tests(audio.WaveGlow(**W.TINY), 5).to(dev())
    den = audio.Denoiser.from_vocoder(voc, frames=8)
    before = den.bias().clone()
    assert den.bias() is den.bias_spec and torch.equal(before, den.bias_spec)
    with torch.no_grad():
        voc.WN[0].end.bias.add_(0.05)
    after = den.bias()
    assert after is den.bias_spec and not torch.equal(before, after)                       # rebuilt in place
