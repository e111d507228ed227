"""CPU tests of the mel front end's host side (glow_tts_amd.audio, data.TextAudioCollate) and of the float64 helper the
GPU tests measure against (tests/mel64.py).  No device is needed."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mel64 as M  # noqa: E402


@pytest.mark.parametrize("name,L", list(zip(M.SIGNALS, M.LENGTHS)))
def test_mel64_against_the_reference_formulation_in_fp32(name, L):
    """tests/mel64.py against the reference's CUDA-branch formulation evaluated by torch in fp32 on the CPU: F.pad(reflect), F.conv1d with
    STFT.forward_basis at stride 256, sqrt(re^2 + im^2), matmul, log(clamp) — held to the per-frame bound of the GPU tests (an fp32
    evaluation in any summation order keeps it), every element included."""
    from glow_tts_amd import audio
    mod = audio.TacotronSTFT()
    x = M.signal(name, L)
    mb = mod.mel_basis.double().numpy()
    ref = M.mel64(x, mb)
    bnd = M.bounds(ref, mb)
    xp = F.pad(torch.from_numpy(x)[None, None, None], (512, 512, 0, 0), mode="reflect").squeeze(1)
    ft = F.conv1d(xp, mod.stft_fn.forward_basis, stride=256)
    mag = torch.sqrt(ft[:, :513] ** 2 + ft[:, 513:] ** 2)
    mel = torch.log(torch.clamp(torch.matmul(mod.mel_basis, mag), min=audio.CLIP_VAL))
    got = {"mag": mag[0], "energy": torch.norm(mag, dim=1)[0], "mel": mel[0]}
    assert mag.shape == (1, 513, 1 + L // 256)
    for k, v in got.items():
        err = np.abs(v.double().numpy() - ref[k])
        assert (err <= bnd[k]).all(), (k, float((err / bnd[k]).max()))


def test_mel64_tells_the_two_classic_mistakes_apart():
    """a symmetric Hann window and zero padding, evaluated in float64, both leave the bound (otherwise the GPU test could not see them)"""
    x = M.signal("noise", 1061)
    mb = np.ones((1, 513))
    ref = M.mel64(x, mb)
    bnd = M.bounds(ref, mb)
    sym = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(M.N) / (M.N - 1))
    wrong_window = M.mel64(x, mb, basis=M.basis64(sym))
    assert (np.abs(wrong_window["mag"] - ref["mag"]) > bnd["mag"]).any()
    fr = np.stack([np.pad(x.astype(np.float64), (512, 512))[f * 256:f * 256 + 1024] for f in range(1 + len(x) // 256)])
    spec = fr @ M.basis64().T
    assert (np.abs(np.hypot(spec[:, :513], spec[:, 513:]).T - ref["mag"]) > bnd["mag"]).any()


def test_forward_basis_is_the_float64_basis_rounded_once():
    from glow_tts_amd import audio
    fb = audio.STFT(1024, 256, 1024).forward_basis
    assert fb.shape == (1026, 1, 1024) and fb.dtype == torch.float32
    fourier = np.fft.fft(np.eye(1024))
    want = np.vstack([fourier[:513].real, fourier[:513].imag]) * M.window64()[None, :]
    assert np.array_equal(fb[:, 0].numpy(), want.astype(np.float32))
    assert np.abs(fb[:, 0].double().numpy() - M.basis64()).max() < 1e-7                 # and it is the exact cos / -sin basis
    sym = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(1024) / 1023.0)                     # a symmetric Hann window must not pass
    assert not np.array_equal(fb[:, 0].numpy(), (np.vstack([fourier[:513].real, fourier[:513].imag]) * sym[None, :]).astype(np.float32))
    assert fb[:, 0, 0].abs().max().item() == 0.0                                        # w[0] = 0: the kernel's fold drops sample 0


def slaney_points(n_mels, fmin, fmax):
    """independent float64 restatement of the Slaney mel scale: n_mels + 2 band edges in Hz"""
    def to_mel(f):
        return f / (200.0 / 3.0) if f < 1000.0 else 15.0 + 27.0 * np.log(f / 1000.0) / np.log(6.4)

    def to_hz(m):
        return m * 200.0 / 3.0 if m < 15.0 else 1000.0 * 6.4 ** ((m - 15.0) / 27.0)
    lo, hi = to_mel(fmin), to_mel(fmax)
    return np.array([to_hz(lo + (hi - lo) * i / (n_mels + 1)) for i in range(n_mels + 2)])


@pytest.mark.parametrize("sr,n_fft,n_mels,fmin,fmax", [(22050, 1024, 80, 0.0, 8000.0), (22050, 1024, 128, 0.0, 11025.0), (16000, 1024, 40, 50.0, 7600.0)])
def test_mel_filterbank(sr, n_fft, n_mels, fmin, fmax):
    """against the restatement written here (element by element, scalar arithmetic), and the properties of librosa's default bank.
    The Slaney normalisation: filter i is a unit-peak triangle times 2 / (f[i + 2] - f[i]).  With W_i = (f[i + 2] - f[i]) n_fft / sr its
    width in bins and T_i the sum of the unit-peak triangle over the bins, the row sums to (2 n_fft / sr) (T_i / W_i) — T_i / W_i is
    the row's own width factor, 1/2 for a wide triangle (area = half base times height)."""
    from glow_tts_amd import audio
    w = audio.mel_filterbank(sr, n_fft, n_mels, fmin, fmax)
    assert w.shape == (n_mels, 1 + n_fft // 2) and w.dtype == np.float32
    pts = slaney_points(n_mels, fmin, fmax)
    freqs = np.arange(1 + n_fft // 2) * (sr / n_fft)
    want = np.zeros((n_mels, 1 + n_fft // 2))
    tri = np.zeros_like(want)
    for i in range(n_mels):
        for k, f in enumerate(freqs):
            tri[i, k] = max(0.0, min((f - pts[i]) / (pts[i + 1] - pts[i]), (pts[i + 2] - f) / (pts[i + 2] - pts[i + 1])))
        want[i] = tri[i] * 2.0 / (pts[i + 2] - pts[i])
    assert np.abs(w - want).max() <= 1e-6 * want.max()
    assert (w >= 0).all()
    assert (w[:, freqs > fmax] == 0).all()
    if fmin == 0.0:
        assert (w[:, 0] == 0).all()
    for i in range(n_mels):
        peak = int(np.argmax(w[i]))
        assert (np.diff(w[i, :peak + 1]) >= 0).all() and (np.diff(w[i, peak:]) <= 0).all()
        width_bins = (pts[i + 2] - pts[i]) * n_fft / sr
        assert abs(float(w[i].astype(np.float64).sum()) - (2.0 * n_fft / sr) * (tri[i].sum() / width_bins)) <= 1e-6
    assert int((w > 0).sum(0).max()) <= 2                                               # at most two filters meet in a bin


def test_tacotron_stft_buffers_and_host_refusals():
    from glow_tts_amd import audio
    mod = audio.TacotronSTFT()
    assert set(dict(mod.named_buffers())) == {"mel_basis", "stft_fn.forward_basis"}
    assert np.array_equal(mod.mel_basis.numpy(), audio.mel_filterbank(22050, 1024, 80, 0.0, 8000.0))
    other = torch.rand(80, 513)
    mod.load_state_dict({"mel_basis": other, "stft_fn.forward_basis": mod.stft_fn.forward_basis.clone()})   # a checkpoint's matrix loads over it
    assert torch.equal(mod.mel_basis, other)
    with pytest.raises(ValueError):
        mod.mel_spectrogram(torch.zeros(2, 4096))
    with pytest.raises(ValueError):
        mod.mel_spectrogram(torch.zeros(2, 4096, dtype=torch.int16), torch.tensor([4096, 2000]))


def items(n, full, rng):
    out = []
    for i in range(n):
        t, L = int(rng.integers(3, 40)), int(rng.integers(513, 9000))
        Fr = 1 + L // 256
        text = torch.from_numpy(rng.integers(1, 100, t))
        wave = torch.from_numpy(rng.integers(-32768, 32767, L).astype(np.int16))
        mel = torch.from_numpy(rng.standard_normal((80, Fr)).astype(np.float32))
        rest = (torch.rand(512), i % 5, torch.rand(3), torch.rand(1, Fr), torch.rand(1, Fr), i % 3) if full else ()
        out.append(((text, wave) + rest, (text, mel) + rest))
    return [a for a, _ in out], [m for _, m in out]


@pytest.mark.parametrize("full", [False, True])
def test_text_audio_collate_is_text_mel_collate_with_waves(full):
    from glow_tts_amd import data
    audio_items, mel_items = items(7, full, np.random.default_rng(3))
    a = data.TextAudioCollate()(audio_items)
    m = data.TextMelCollate()(mel_items)
    assert len(a) == len(m) == (10 if full else 4)
    assert torch.equal(a[0], m[0]) and torch.equal(a[1], m[1])                          # same order: texts and their lengths
    wav, wav_len = a[2], a[3]
    assert wav.dtype == torch.int16 and wav_len.dtype == torch.long and wav.shape[0] == 7 and wav.shape[1] % 4 == 0
    assert wav.shape[1] - max(x[1].numel() for x in audio_items) in range(4)
    assert torch.equal(1 + wav_len // 256, m[3])                                         # lengths in samples, the mel's in frames
    order = torch.sort(torch.LongTensor([len(x[0]) for x in audio_items]), descending=True)[1].tolist()
    for i, k in enumerate(order):
        L = audio_items[k][1].numel()
        assert wav_len[i] == L and torch.equal(wav[i, :L], audio_items[k][1]) and not wav[i, L:].any()
    for j in range(4, len(a)):
        assert a[j].shape == m[j].shape and torch.equal(a[j], m[j])
    if full:
        none_energy = [x[:6] + (None,) + x[7:] for x in audio_items]
        assert data.TextAudioCollate()(none_energy)[8] is None
    with pytest.raises(ValueError):
        data.TextAudioCollate()([(audio_items[0][0], audio_items[0][1].float())])
