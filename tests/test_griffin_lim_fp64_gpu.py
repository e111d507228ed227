"""GPU tests of the waveform back end's two MFMA kernels (csrc/griffin_lim.hip) against the float64 oracle
tests/gl64.py, with bounds that are derived there, not fitted.  The ragged batch: mel64's five signals in turn at 4 and 5 frames and
at T, T + 1, T + 2 frames around the frame tile and around the hop tile the library reports; spectrogram rows are padded with 7.0
behind each utterance (nothing there may be read).

  gt_istft       on fp32 (mag, phase) of the float64 transform: every kept sample within C_ISTFT u sum |ib| |Y| of gl64.inverse on
                 the same fp32 operands, and within that plus the reconstruction term of the ORIGINAL signal.
  gt_gl_project  on the signals and their own fp32 magnitudes: every component of every Y[k][f] within
                 M min(2, c' d_f / |X64|) + c'' u M of M X64 / |X64|; no element is excluded.
Each test prints its worst error as a share of the bound (DESIGN.md 4.20 quotes them)."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gl64 as G  # noqa: E402

pytestmark = pytest.mark.gpu


def dev():
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def modules():
    from glow_tts_amd import audio
    return audio.GriffinLim(audio.STFT()).to(dev())


@functools.lru_cache(maxsize=None)
def batch():
    """frames, signals, the float64 transforms, and fp32 (mag, phase) [B, 513, F_max] padded with 7.0"""
    from glow_tts_amd import _lib
    frames = G.ragged_frames(_lib.lib().gt_gl_tile_frames(), _lib.lib().gt_gl_tile_hops())
    waves = G.ragged_signals(frames)
    F_max = max(frames)
    mag = np.full((len(frames), G.NBIN, F_max), 7.0, dtype=np.float32)
    phase = np.full_like(mag, 7.0)
    for i, (x, F) in enumerate(zip(waves, frames)):
        re, im = G.transform(x)
        assert re.shape[1] == F
        mag[i, :, :F] = np.hypot(re, im)
        phase[i, :, :F] = np.arctan2(im, re)
    return frames, waves, mag, phase


def test_istft_within_the_float64_bound(built):
    frames, waves, mag, phase = batch()
    gl = modules()
    out = gl.istft.inverse(torch.from_numpy(mag).to(dev()), torch.from_numpy(phase).to(dev()),
                           frames=torch.tensor(frames, dtype=torch.int32, device=dev()))
    torch.cuda.synchronize()
    out = out.double().cpu().numpy()
    assert out.shape == (len(frames), G.HOP * (max(frames) - 1))
    worst, worst_orig, failures = 0.0, 0.0, []
    for i, (x, F) in enumerate(zip(waves, frames)):
        L = G.HOP * (F - 1)
        m, p = mag[i, :, :F].astype(np.float64), phase[i, :, :F].astype(np.float64)
        re, im = m * np.cos(p), m * np.sin(p)
        ref, bound, bound_orig = G.inverse(re, im), G.istft_bound(re, im), G.recon_bound(re, im)
        err, err_orig = np.abs(out[i, :L] - ref), np.abs(out[i, :L] - x.astype(np.float64))
        share, share_orig = (err / bound).max(), (err_orig / bound_orig).max()
        worst, worst_orig = max(worst, share), max(worst_orig, share_orig)
        print(f"istft utt {i} F={F}: max err {err.max():.3e} = {share:.4f} of the bound; vs the signal {err_orig.max():.3e} = {share_orig:.4f}")
        if not (err <= bound).all() or not (err_orig <= bound_orig).all():
            failures.append((i, F, share, share_orig))
        assert not out[i, L:].any(), i
    print(f"istft: worst share of the bound {worst:.4f} (vs gl64.inverse), {worst_orig:.4f} (vs the original signal)")
    assert not failures, failures


def test_project_within_the_float64_bound(built):
    from glow_tts_amd import audio
    frames, waves, mag, _ = batch()
    gl = modules()
    B, F_max = len(frames), max(frames)
    wav = np.zeros((B, G.HOP * (F_max - 1)), dtype=np.float32)
    for i, x in enumerate(waves):
        wav[i, :len(x)] = x
        wav[i, len(x):] = 7.0                                  # behind the utterance: not to be read
    n_frames = torch.tensor(frames, dtype=torch.int32, device=dev())
    spec = gl.istft.workspace(B, F_max, dev())
    spec.fill_(float("nan"))                                   # all of it must be written
    gl.project(torch.from_numpy(wav).to(dev()), torch.from_numpy(mag).to(dev()), n_frames, spec)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(spec).all())
    yre, yim = (t.double().cpu().numpy() for t in audio.spec_unpack(spec, B, F_max))
    worst, worst_settled, failures = 0.0, 0.0, []
    for i, (x, F) in enumerate(zip(waves, frames)):
        M = mag[i, :, :F].astype(np.float64)
        rre, rim, mag64, S = G.project64(x, M)
        bound = G.project_bound(M, mag64, S)
        err = np.maximum(np.abs(yre[i, :, :F] - rre), np.abs(yim[i, :, :F] - rim))
        shares = err / np.maximum(bound, 1e-300)
        share, settled = shares.max(), bound < 2 * M            # settled: the phase term is below its cap of 2 M
        worst = max(worst, share)
        worst_settled = max(worst_settled, shares[settled].max() if settled.any() else 0.0)
        print(f"project utt {i} F={F}: max err {err.max():.3e}, worst share of the bound {share:.4f} "
              f"({shares[settled].max() if settled.any() else 0.0:.4f} where the phase is determined, {settled.mean():.3f} of the bins)")
        if not (err <= bound).all():
            failures.append((i, F, share))
        assert not yre[i, :, F:].any() and not yim[i, :, F:].any(), i
    print(f"project: worst share of the bound {worst:.4f}; {worst_settled:.4f} where the phase is determined")
    assert not failures, failures
