"""GPU tests of audio.Normalized, a vocoder with the BS.1770 loudness stage behind it, on the TINY WaveGlow of
tests/waveglow64.py at frames (0, 1, 2, 3, 5), a small HiFi-GAN, the TINY Vocos (which loses a frame), a 128-hop HiFi-GAN and around
audio.Denoised; and of metrics.Evaluator's loudness fields.

The kernels are deterministic and an utterance's samples depend on its own row alone, so the composition is a question of plumbing
(frame counts, hop, `lost`, buffers, the seed), not of tolerance: Normalized(voc)(mel, lengths) must be BIT-IDENTICAL to
voc(mel, lengths) followed by Loudness.normalize on its output.

The level.  The normalised samples y, measured by the float64 oracle tests/loudness64.py, sit at the target within

    loudness64.bounds' dL_double of the vocoder's samples x     the device's own L, in double, from which g is taken
  + 10 / ln 10 * 2^-24                                          g rounded to fp32: one relative error on every sample alike
  + 10 / ln 10 * rho_y                                          y = fl(g x): |dy| <= 2^-24 |y| per sample, through the K filter's l1
                                                                gain H1 (|dz| <= 2^-24 H1 max |y|), then loudness64.sum_bound / sum z^2

or, where the oracle says the peak rule engages for x, below the target with max |y| within 3 * 2^-24 of the ceiling.  Both cases are
exercised: the targets are -23 LUFS and +20 LUFS (g max |x| is then at least 10 times the crest factor: the ceiling always holds)."""
import functools
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "golden"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import loudness64 as L  # noqa: E402
import vocos64 as V  # noqa: E402
import waveglow64 as W  # noqa: E402

pytestmark = pytest.mark.gpu
FRAMES = W.TINY_FRAMES
FS, PEAK_DBFS = 22050, -1.0
TARGETS = (-23.0, 20.0)


def dev():
    return torch.device("cuda:0")


def bits(t):
    return t.contiguous().view(torch.int32)


@functools.lru_cache(maxsize=None)
def waveglow():
    from glow_tts_amd import audio
    return W.init_for_tests(audio.WaveGlow(**W.TINY), 41).to(dev())


@functools.lru_cache(maxsize=None)
def k_filter_l1():
    imp = np.zeros(FS // 2)
    imp[0] = 1.0
    return float(np.abs(L.kfilter(imp, FS)).sum())


def at_target_or_ceiling(x, y, target, chunk):
    """the oracle's verdict on one utterance: x the vocoder's samples, y the normalised ones (fp32 values in float64)"""
    ref = L.loudness64(x, FS, target, PEAK_DBFS)
    if ref["L"] == -np.inf:
        assert np.array_equal(y, x)
        return None
    assert L.gate_margin(ref) >= L.GATE_MARGIN
    got = L.loudness64(y, FS)
    if ref["engaged"]:
        assert got["L"] < target and abs(np.abs(y).max() - 10.0 ** (PEAK_DBFS / 20.0)) <= 3 * L.U32
        return True
    bd = L.bounds(x, FS, ref, chunk)
    rho_y = L.sum_bound(got["z"], L.U32 * k_filter_l1() * np.abs(y).max(), len(y)) / np.sum(got["z"] ** 2)
    bound = bd["dL_double"] + 10.0 / math.log(10.0) * (L.U32 + rho_y)
    assert abs(got["L"] - target) <= bound, (got["L"], target, bound)
    return False


def composition(voc, norm, frames, seed=None):
    """Normalized(voc) in one call against voc followed by Loudness.normalize, at both targets; -> how many utterances sat at the
    target and how many at the ceiling"""
    rng = np.random.default_rng(3)
    C = voc.mel_channels - voc.mel_padding
    mel = torch.from_numpy(np.stack([W.random_mel(rng, C, max(frames)) for _ in frames])).to(dev())
    lengths = torch.tensor(frames, dtype=torch.int32, device=dev())
    kw = {} if seed is None else dict(seed=seed)
    lost, hop = voc.min_frames - 1, voc.hop_length
    verdicts = []
    for target in TARGETS:
        norm.set_target(target, PEAK_DBFS)
        got, got_len = norm(mel, lengths, mel_lengths_host=list(frames), **kw)
        plain, plain_len = voc(mel, lengths, mel_lengths_host=list(frames), **kw)
        want, want_len = norm.loudness.normalize(plain, plain_len)
        torch.cuda.synchronize()
        assert got_len.tolist() == plain_len.tolist() == want_len.tolist() == [hop * max(n - lost, 0) for n in frames]
        assert got.shape == plain.shape == want.shape == (len(frames), hop * (max(frames) - lost))
        assert torch.equal(bits(got), bits(want))
        x, y = plain.double().cpu().numpy(), got.double().cpu().numpy()
        for b, n in enumerate(got_len.tolist()):
            assert not bool(got[b, n:].any()), b
            if n:
                assert float(got[b, :n].abs().max()) > 0, b
                verdicts.append(at_target_or_ceiling(x[b, :n], y[b, :n], target, norm.loudness.chunk))
    return verdicts.count(False), verdicts.count(True)


def test_normalized_waveglow_is_the_vocoder_followed_by_the_stage(built):
    from glow_tts_amd import _lib, audio
    voc = waveglow()
    norm = audio.Normalized(voc)
    assert norm.seeded and norm.launches == voc.launches + 2 and (norm.hop_length, norm.min_frames, norm.mel_channels) == (256, 1, 80)
    assert (norm.loudness.sampling_rate, norm.loudness.target_lufs, norm.loudness.peak_dbfs) == (22050, -23.0, -1.0)
    at_target, at_ceiling = composition(voc, norm, FRAMES, seed=3)
    print(f"normalized waveglow: {at_target} utterances at the target, {at_ceiling} at the ceiling")
    assert at_target > 0 and at_ceiling > 0
    assert norm(torch.zeros(1, 80, 5, device=dev()), seed=3).shape == (1, 256 * 5)           # no lengths: the samples alone
    with _lib.record_calls() as names:
        norm(torch.zeros(2, 80, 5, device=dev()), seed=4)
    names = [n for n in names if not n.endswith("_bytes")]                                  # buffer_spec's size query is no launch
    assert len(names) == norm.launches and names[-2:] == ["gt_loudness_measure", "gt_loudness_apply"]
    with pytest.raises(TypeError):
        audio.Normalized(voc, loudness=audio.Denoiser())
    with pytest.raises(TypeError):
        audio.Normalized(torch.nn.Linear(2, 2))


def test_normalized_hifigan_vocos_and_a_128_hop_vocoder(built):
    from glow_tts_amd import audio
    torch.manual_seed(43)
    hifi = audio.HiFiGAN(upsample_initial_channel=256).to(dev())
    assert sum(composition(hifi, audio.Normalized(hifi, target_lufs=-16.0), (0, 1, 2, 3, 5))) == 8
    vocos = V.init_for_tests(audio.Vocos(**V.TINY), 8).to(dev())
    norm = audio.Normalized(vocos)
    assert norm.min_frames == 2 and not norm.seeded
    assert sum(composition(vocos, norm, (0, 1, 2, 3, 5, 70))) == 8                           # lost = 1: frames 0 and 1 give no sample
    with pytest.raises(ValueError):
        norm(torch.zeros(1, 80, 4, device=dev()), seed=3)                                   # the inner vocoder draws no latent
    half = audio.HiFiGAN(upsample_rates=(8, 8, 2), upsample_kernel_sizes=(16, 16, 4), upsample_initial_channel=128).to(dev())
    assert half.hop_length == 128
    assert sum(composition(half, audio.Normalized(half), (0, 1, 3, 40))) == 6                # any hop: 40 frames are 5120 samples


def test_normalized_around_denoised(built):
    from glow_tts_amd import _lib, audio
    den = audio.Denoised(waveglow(), strength=0.1)
    norm = audio.Normalized(den, loudness=audio.Loudness(22050, -20.0, -3.0).to(dev()))
    assert norm.launches == waveglow().launches + 4 and norm.seeded
    mel = torch.from_numpy(np.stack([W.random_mel(np.random.default_rng(5), 80, 5) for _ in range(3)])).to(dev())
    lengths = torch.tensor([5, 0, 3], dtype=torch.int32, device=dev())
    got, got_len = norm(mel, lengths, mel_lengths_host=[5, 0, 3], seed=9)
    inner, inner_len = den(mel, lengths, mel_lengths_host=[5, 0, 3], seed=9)
    want, _ = norm.loudness.normalize(inner, inner_len)
    torch.cuda.synchronize()
    assert got_len.tolist() == [1280, 0, 768] and torch.equal(bits(got), bits(want)) and not torch.equal(got, inner)
    with _lib.record_calls() as names:
        norm(mel, lengths, mel_lengths_host=[5, 0, 3], seed=9)
    assert [n for n in names if not n.endswith("_bytes")][-4:] == ["gt_denoise_spec", "gt_istft", "gt_loudness_measure", "gt_loudness_apply"]


def test_evaluator_scores_the_loudness_of_both_waveforms(built):
    """the sweep of tests/test_dtw_gpu.py's end-to-end test, the synthesised side 6 dB quieter: lufs_syn - lufs_ref reads it; every
    output the Evaluator had is bit-identical with and without the new fields, and so are its launches"""
    from glow_tts_amd import _lib, audio, metrics
    sr = 22050
    t = torch.arange(sr, dtype=torch.float64) / sr
    phase = 2 * math.pi * 100.0 * (2.0 ** (2.0 * t) - 1.0) / (2.0 * math.log(2.0))
    x = sum(torch.sin(h * phase) / h for h in range(1, 6)).float().mul(0.3)[None, :].to(dev())
    z, z_len = audio.Resample(5, 4).to(dev())(x)
    x = x * 0.5
    x_len = torch.tensor([sr], dtype=torch.int32, device=dev())
    stft, yin = audio.TacotronSTFT().to(dev()), audio.YIN().to(dev())
    mel_x, mel_x_len, _ = stft.mel_spectrogram(x, x_len)
    plain = metrics.Evaluator(stft, yin)
    loud = metrics.Evaluator(stft, yin, loudness=audio.Loudness(sr).to(dev()))
    plain.score(mel_x, mel_x_len, z, z_len, x, x_len)
    loud.score(mel_x, mel_x_len, z, z_len, x, x_len)                                       # images and workspaces exist from here on
    with _lib.record_calls() as before:
        a = plain.score(mel_x, mel_x_len, z, z_len, x, x_len)
    with _lib.record_calls() as after:
        b = loud.score(mel_x, mel_x_len, z, z_len, x, x_len)
    torch.cuda.synchronize()
    after = [n for n in after if not n.endswith("_bytes")]
    assert after[:len(before)] == before and after[len(before):] == ["gt_loudness_measure", "gt_loudness_measure"]
    assert set(b) == set(a) | {"lufs_ref", "lufs_syn", "lufs_diff"}
    for k, v in a.items():
        assert v.dtype == b[k].dtype and v.shape == b[k].shape and v.cpu().numpy().tobytes() == b[k].cpu().numpy().tobytes(), k
    want_ref = L.loudness64(z[0, :int(z_len[0])].double().cpu().numpy(), sr)["L"]
    want_syn = L.loudness64(x[0].double().cpu().numpy(), sr)["L"]
    print(f"evaluator: lufs_ref {b['lufs_ref'].item():.4f} ({want_ref:.4f}), lufs_syn {b['lufs_syn'].item():.4f} ({want_syn:.4f})")
    assert abs(b["lufs_ref"].item() - want_ref) <= 1e-5 and abs(b["lufs_syn"].item() - want_syn) <= 1e-5
    # 6.02 dB quieter, and the reference is the sweep a major third up (more of it under the shelf): about a decibel either way
    assert torch.equal(b["lufs_diff"], b["lufs_syn"] - b["lufs_ref"]) and -7.5 < b["lufs_diff"].item() < -4.5
    # a reference at another rate is measured at its own rate
    c = loud.score(mel_x, mel_x_len, z, z_len, x, x_len, sampling_rate=22050)
    assert torch.equal(c["lufs_ref"], b["lufs_ref"])
