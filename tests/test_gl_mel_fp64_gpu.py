"""GPU test of the mel-inversion kernel (csrc/gl_mel.hip: gt_gl_from_mel) against the float64 oracle
tests/gl_mel64.py, with bounds that are counted there, not fitted.  A ragged batch with frame counts at the layout's edges (4, 5, the
32-frame group at 31 / 32 / 33, the Griffin-Lim tile T and T + 1), F_max no multiple of 32, a mel pitch larger than F_max, and NaN in
every mel frame from F_b on (nothing there may reach an output):

  n_mel = 80   real log-mels (TacotronSTFT.mel_spectrogram of mel64's signals) with GriffinLim.mel_pinv()
  n_mel = 37   an odd K with a random matrix and random log-mels
Every element of mag and of the unpacked spectrum is inside its bound, the outputs are exact zeros from F_b on (to the padded end of
the workspace), nothing is NaN, and the canaries around mag and spec are intact.  Prints the worst error as a share of the bound
(DESIGN.md 4.21 quotes it)."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gl_mel64 as G  # noqa: E402

pytestmark = pytest.mark.gpu
SEED = 20240611


def dev():
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def vocoder():
    from glow_tts_amd import audio
    return audio.GriffinLim(audio.TacotronSTFT()).to(dev())


@functools.lru_cache(maxsize=None)
def operands(n_mel):
    """(frames, F_max, pitch, pinv32 [513, n_mel], mel32 [B, n_mel, pitch] with NaN from F_b on) as host arrays"""
    from glow_tts_amd import _lib
    frames = G.ragged_frames(_lib.lib().gt_gl_tile_frames())
    B, F_max = len(frames), max(frames) + 2
    pitch = F_max + 5
    assert F_max % 32 and frames[-2] % 64 == 0
    mel = np.full((B, n_mel, pitch), np.nan, dtype=np.float32)
    if n_mel == 80:
        gl = vocoder()
        pinv = gl.mel_pinv().cpu().numpy()
        for i, (x, F) in enumerate(zip(G.ragged_signals(frames), frames)):
            m, _ = gl.stft.mel_spectrogram(torch.from_numpy(x).to(dev()).view(1, -1))
            assert m.shape == (1, 80, F)
            mel[i, :, :F] = m[0].cpu().numpy()
    else:
        rng = np.random.default_rng(n_mel)
        pinv = rng.standard_normal((513, n_mel)).astype(np.float32)
        for i, F in enumerate(frames):
            mel[i, :, :F] = rng.uniform(-8.0, 2.0, (n_mel, F)).astype(np.float32)
    return frames, F_max, pitch, pinv, mel


@pytest.mark.parametrize("n_mel", [80, 37])
def test_from_mel_within_the_float64_bound(built, n_mel):
    from glow_tts_amd import _lib, audio
    from oracle.guards import Guards
    frames, F_max, pitch, pinv, mel = operands(n_mel)
    B = len(frames)
    g = Guards(dev())
    mel_d = g.inp(torch.from_numpy(mel).to(dev()))
    pinv_d = g.inp(torch.from_numpy(pinv).to(dev()))
    fr = torch.tensor(frames, dtype=torch.int32, device=dev())
    words = _lib.lib().gt_gl_spec_bytes(B, F_max) // 4
    Fp = (F_max + 63) // 64 * 64
    assert words == B * Fp * 1025
    mag = g.out("mag", (B, 513, F_max))
    spec = g.out("spec", (words,))
    _lib.call.gt_gl_from_mel(mel_d, mel_d.stride(0), mel_d.stride(1), fr, B, F_max, n_mel, pinv_d, SEED, None, mag, spec,
                             _lib.current_stream(dev()))
    g.verify()                                               # canaries intact, every element written, no NaN
    assert bool(torch.isfinite(mag).all()) and bool(torch.isfinite(spec).all())
    re, im = (t.double().cpu().numpy() for t in audio.spec_unpack(spec, B, Fp))       # to the padded end of the workspace
    got = mag.double().cpu().numpy()
    worst_m, worst_s, failures = 0.0, 0.0, []
    for i, F in enumerate(frames):
        m32 = mel[i, :, :F]
        ref, mb, sb = G.mag64(pinv, m32), G.mag_bound(pinv, m32), G.spec_bound(pinv, m32)
        rre, rim = G.spectrum64(ref, G.phase_t(SEED, i, F))
        em = np.abs(got[i, :, :F] - ref)
        es = np.maximum(np.abs(re[i, :, :F] - rre), np.abs(im[i, :, :F] - rim))
        sm, ss = (em / np.maximum(mb, 1e-300)).max(), (es / np.maximum(sb, 1e-300)).max()
        worst_m, worst_s = max(worst_m, sm), max(worst_s, ss)
        print(f"from_mel n_mel={n_mel} utt {i} F={F}: mag err {em.max():.3e} = {sm:.4f} of the bound, spectrum err {es.max():.3e} = {ss:.4f}")
        if not (em <= mb).all() or not (es <= sb).all():
            failures.append((i, F, sm, ss))
        assert not got[i, :, F:].any() and not re[i, :, F:].any() and not im[i, :, F:].any(), i      # exact zeros from F_b on
        assert float(np.abs(ref).max()) > 0 and float(np.abs(rim).max()) > 0
    print(f"from_mel n_mel={n_mel}: worst share of the bound {worst_m:.4f} (magnitudes), {worst_s:.4f} (spectrum)")
    assert not failures, failures
