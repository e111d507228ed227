"""GPU tests of mel inversion with counter phases as a whole (glow_tts_amd.audio.GriffinLim.from_mel(phases="counter") /
mel_workspace / run_from_mel, csrc/gl_mel.hip): batch, capacity and pitch invariance bit for bit, the seed by value
and from a device word, the Python path against hand-composed kernel calls, the default path against what it was, the refusal, and
convergence from counter phases against the float64 loop of tests/gl64.py."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gl64 as G  # noqa: E402
import gl_mel64 as GM  # noqa: E402
import mel64 as M  # noqa: E402

pytestmark = pytest.mark.gpu
HOP = 256
FRAMES = (33, 20, 65)                                                      # more than one 32-frame group, more than one 64-frame tile


def dev():
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def gl_mel():
    from glow_tts_amd import audio
    return audio.GriffinLim(audio.TacotronSTFT()).to(dev())


@functools.lru_cache(maxsize=None)
def batch():
    """log-mel [3, 80, 65] of three of mel64's signals (7.0 behind each utterance) and their frame counts on the device"""
    gl = gl_mel()
    mel = torch.full((len(FRAMES), 80, max(FRAMES)), 7.0, device=dev())
    for i, F in enumerate(FRAMES):
        x = M.signal(M.SIGNALS[(i + 2) % len(M.SIGNALS)], HOP * (F - 1))
        mel[i, :, :F] = gl.stft.mel_spectrogram(torch.from_numpy(x).to(dev()).view(1, -1))[0][0]
    return mel, torch.tensor(FRAMES, dtype=torch.int32, device=dev())


@functools.lru_cache(maxsize=None)
def reference():
    """the batch through from_mel(phases="counter"), n_iters = 2, seed 5 — computed once, left unchanged"""
    mel, fr = batch()
    wav, lengths = gl_mel().from_mel(mel, fr, mel_lengths_host=list(FRAMES), n_iters=2, seed=5, phases="counter")
    torch.cuda.synchronize()
    return wav, lengths


def test_batch_row_equals_the_utterance_alone_and_a_larger_capacity(built):
    mel, fr = batch()
    gl = gl_mel()
    wav, lengths = reference()
    assert wav.shape == (3, HOP * (max(FRAMES) - 1)) and lengths.tolist() == [HOP * (F - 1) for F in FRAMES]
    for i, F in enumerate(FRAMES):
        assert not bool(wav[i, HOP * (F - 1):].any()) and bool(torch.isfinite(wav[i]).all()) and float(wav[i].abs().max()) > 0
    # the same batch at a larger F_max and another mel pitch, NaN behind every utterance
    F_big, pitch = max(FRAMES) + 30, max(FRAMES) + 41
    wide = torch.full((3, 80, pitch), float("nan"), device=dev())
    for i, F in enumerate(FRAMES):
        wide[i, :, :F] = mel[i, :, :F]
    bufs = gl.mel_workspace(3, F_big, dev())
    big = gl.run_from_mel(wide, fr, bufs, n_iters=2, seed=5)
    assert big.shape == (3, HOP * (F_big - 1))
    assert torch.equal(big[:, :wav.shape[1]], wav) and not bool(big[:, wav.shape[1]:].any())
    # an utterance alone differs from its batch row only by its index b in the phase key: utterance 0 alone is row 0
    alone = gl.from_mel(mel[:1, :, :FRAMES[0]].contiguous(), n_iters=2, seed=5, phases="counter")
    assert alone.shape == (1, HOP * (FRAMES[0] - 1)) and torch.equal(alone[0], wav[0, :HOP * (FRAMES[0] - 1)])
    # row 1 between other neighbours (rows 0 and 2 swapped) keeps its samples
    swapped, _ = gl.from_mel(mel[[2, 1, 0]].contiguous(), fr[[2, 1, 0]].contiguous(), n_iters=2, seed=5, phases="counter")
    assert torch.equal(swapped[1], wav[1]) and not torch.equal(swapped[0], wav[0])
    # ... and the magnitudes of every utterance do not depend on the batch at all
    full = gl.mel_workspace(3, max(FRAMES), dev())
    gl.run_from_mel(mel, fr, full, n_iters=0, seed=5)
    for i, F in enumerate(FRAMES):
        one = gl.mel_workspace(1, F, dev())
        gl.run_from_mel(mel[i:i + 1, :, :F], torch.tensor([F], dtype=torch.int32, device=dev()), one, n_iters=0, seed=5)
        assert torch.equal(one["mag"][0], full["mag"][i, :, :F]), i


def test_seed_by_value_equals_the_seed_word_and_seeds_differ(built):
    mel, fr = batch()
    gl = gl_mel()
    wav, _ = reference()
    bufs = gl.mel_workspace(3, max(FRAMES), dev())
    word = torch.tensor([5, 99], dtype=torch.int32, device=dev())
    by_word = gl.run_from_mel(mel, fr, bufs, n_iters=2, seed=1234, seed_dev=word[:1]).clone()       # the word wins over the value
    assert torch.equal(by_word, wav)
    word[0] = 6
    other = gl.run_from_mel(mel, fr, bufs, n_iters=2, seed=1234, seed_dev=word[:1]).clone()
    six, _ = gl.from_mel(mel, fr, mel_lengths_host=list(FRAMES), n_iters=2, seed=6, phases="counter")
    assert torch.equal(other, six) and not torch.equal(other, wav)
    # the first spectrum carries the restated generator's phases: utterance 2 (65 frames of noise), wherever the magnitude is not tiny
    from glow_tts_amd import audio
    gl.run_from_mel(mel, fr, bufs, n_iters=0, seed=5)
    re, im = audio.spec_unpack(bufs["spec"], 3, max(FRAMES))
    F = FRAMES[2]
    t = torch.from_numpy(GM.phase_t(5, 2, F)).to(dev())
    m = bufs["mag"][2, :512, :F].double()
    got = torch.atan2(im[2, :512, :F].double(), re[2, :512, :F].double()) / np.pi
    live = m > 1e-6 * m.max()
    d = (got - t[:512])[live].abs()
    assert int(live.sum()) > 1000 and float(torch.minimum(d, 2.0 - d).max()) < 1e-5


def test_from_mel_counter_equals_the_hand_composed_kernel_calls(built):
    from glow_tts_amd import _lib
    mel, fr = batch()
    gl, B, F_max = gl_mel(), 3, max(FRAMES)
    gl.istft._image(), gl.stft._image(), gl.mel_pinv()                     # packed once, before the launches that are counted
    with _lib.record_calls() as names:
        wav, _ = gl.from_mel(mel, fr, mel_lengths_host=list(FRAMES), n_iters=3, seed=5, phases="counter")
    launches = [n for n in names if not n.endswith("_bytes")]
    assert launches == ["gt_gl_from_mel", "gt_istft"] + ["gt_gl_project", "gt_istft"] * 3                    # 1 + 1 + 2 n launches
    L, st = _lib.lib(), _lib.current_stream(dev())
    mag = torch.empty(B, 513, F_max, dtype=torch.float32, device=dev())
    spec = torch.empty(L.gt_gl_spec_bytes(B, F_max) // 4, dtype=torch.float32, device=dev())
    out = torch.empty(B, HOP * (F_max - 1), dtype=torch.float32, device=dev())
    p = lambda t: t.data_ptr()  # noqa: E731
    inv_img, fwd_img, pinv = gl.istft._image(), gl.stft._image(), gl.mel_pinv()
    assert L.gt_gl_from_mel(p(mel), mel.stride(0), mel.stride(1), p(fr), B, F_max, 80, p(pinv), 5, None, p(mag), p(spec), st) == 0
    assert L.gt_istft(p(spec), p(fr), B, F_max, p(inv_img), 1024, 256, 1024, p(out), out.stride(0), st) == 0
    for _ in range(3):
        assert L.gt_gl_project(p(out), out.stride(0), p(mag), p(fr), B, F_max, p(fwd_img), 1024, 256, 1024, p(spec), st) == 0
        assert L.gt_istft(p(spec), p(fr), B, F_max, p(inv_img), 1024, 256, 1024, p(out), out.stride(0), st) == 0
    torch.cuda.synchronize()
    assert torch.equal(wav, out)


def test_default_from_mel_is_what_it_was(built):
    """phases="torch" (the default): today's ops composed by hand — matmul / exp / clamp, a device generator's uniform_, the loop"""
    mel, fr = batch()
    gl = gl_mel()
    got, got_len = gl.from_mel(mel, fr, mel_lengths_host=list(FRAMES), n_iters=2, seed=3)
    same, _ = gl.from_mel(mel, fr, mel_lengths_host=list(FRAMES), n_iters=2, seed=3, phases="torch")
    magnitudes = torch.clamp(torch.matmul(gl.mel_pinv(), torch.exp(mel.float())), min=0.0)
    gen = torch.Generator(device=dev())
    gen.manual_seed(3)
    angles = torch.empty_like(magnitudes).uniform_(-np.pi, np.pi, generator=gen)
    want, want_len = gl(magnitudes, frames=fr, frames_host=list(FRAMES), n_iters=2, angles=angles)
    assert torch.equal(got, want) and torch.equal(same, want) and torch.equal(got_len, want_len)
    assert not torch.equal(got, reference()[0])


def test_refusals(built):
    from glow_tts_amd import audio
    mel, fr = batch()
    gl = gl_mel()
    with pytest.raises(ValueError, match="angles"):
        gl.from_mel(mel, fr, n_iters=1, angles=torch.zeros(3, 513, max(FRAMES), device=dev()), phases="counter")
    with pytest.raises(ValueError):
        gl.from_mel(mel, fr, n_iters=1, phases="philox")
    with pytest.raises(ValueError):
        gl.from_mel(mel[:, :, :3].contiguous(), n_iters=1, phases="counter")                    # 3 frames: the host knows
    with pytest.raises(ValueError):
        gl.from_mel(mel, fr, mel_lengths_host=[33, 3, 65], n_iters=1, phases="counter")
    with pytest.raises(ValueError):
        gl.from_mel(mel[:, :40].contiguous(), fr, n_iters=1, phases="counter")                  # 40 channels for an 80-channel bank
    with pytest.raises(audio.CpuWaveError):
        gl.from_mel(mel.cpu(), n_iters=1, phases="counter")
    with pytest.raises(ValueError):
        gl.mel_workspace(1, 1, dev())


def test_convergence_from_counter_phases_matches_the_float64_loop(built):
    """c_i = || |STFT(x_i)| - M || / || M || as tests/test_griffin_lim_gpu.py::test_convergence_matches_the_float64_loop states it, on
    the 20-frame chirp: M is the kernel's own inversion of the chirp's log-mel (read back, so both loops see the same fp32
    magnitudes), the device loop starts from the counter phases of seed 11, gl64's float64 loop from the restated phases of seeds
    11, 12, 13.  c_0 agrees (the first inverse is the same linear map of the same phases); c_30 lies inside the float64 ends'
    [min, max] widened on each side by their own spread, and below c_0."""
    F = 20
    gl = gl_mel()
    x = M.signal("chirp", HOP * (F - 1))
    mel = gl.stft.mel_spectrogram(torch.from_numpy(x).to(dev()).view(1, -1))[0]
    fr = torch.tensor([F], dtype=torch.int32, device=dev())
    bufs = gl.mel_workspace(1, F, dev())
    w0 = gl.run_from_mel(mel, fr, bufs, n_iters=0, seed=11)[0].double().cpu().numpy()
    mag32 = bufs["mag"][0].cpu().numpy()
    w30 = gl.run_from_mel(mel, fr, bufs, n_iters=30, seed=11)[0].double().cpu().numpy()
    assert np.array_equal(bufs["mag"][0].cpu().numpy(), mag32) and float(mag32.max()) > 0
    ends, starts = [], []
    for seed in (11, 12, 13):
        x0, xn = G.griffin_lim64(mag32, np.pi * GM.phase_t(seed, 0, F), 30)
        starts.append(G.convergence(x0, mag32)); ends.append(G.convergence(xn, mag32))
    c0, c30 = G.convergence(w0, mag32), G.convergence(w30, mag32)
    lo, hi = min(ends), max(ends)
    spread = hi - lo
    print(f"chirp from counter phases: device c_0 {c0:.4f} c_30 {c30:.4f}; float64 c_0 {min(starts):.4f}..{max(starts):.4f}, c_30 {lo:.4f}..{hi:.4f}")
    assert abs(c0 - starts[0]) < 1e-4
    assert lo - spread <= c30 <= hi + spread
    assert c30 < c0
