"""GPU tests of the Vocos module (glow_tts_amd.audio.Vocos on csrc/vocos.hip, gt_voc_conv and gt_istft).

The tolerance is measured, not fixed, as in tests/test_hifigan_gpu.py: tests/vocos64.py has the exact float64 generator and a CPU
EMULATION of the device's rounding (bf16 where the kernels round to bf16, float64 elsewhere).  E_emul = ||emul - exact|| / ||exact|| is
computed here, on the CPU, for the same weights and mel, and the device must satisfy ||gpu - exact|| / ||exact|| <= 2 E_emul per
utterance and over the batch; 0 < E_emul < 0.05 is a condition, so that the test cannot pass on noise.  Weights: torch's default
initialisation, gamma ~ U(0.1, 1), the head's weight x 4 (phases of a few radians, magnitudes over e^+-2).  Each test prints E_emul
and the measured ratio.

Measured on an MI355X (ratio = device error / E_emul over the batch; the bound is 2):
  tiny (128 / 256 / 2 layers, frames 0, 1, 2, 3, 9, 65)   E_emul 9.25e-03, device 9.25e-03, ratio 1.000 (per utterance 1.000)
  published shape (512 / 1536 / 8 layers, frames 5, 9)    E_emul 1.11e-02, device 1.09e-02, ratio 0.989 (per utterance 1.003, 0.982)
  100 bands padded to 112 (tiny, 7 frames)                E_emul 9.75e-03, device 9.75e-03, ratio 1.000
"""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import vocos64 as V  # noqa: E402

pytestmark = pytest.mark.gpu


def dev():
    return torch.device("cuda:0")


def tile():
    from glow_tts_amd import _lib
    return _lib.lib().gt_vocos_tile_positions()


@functools.lru_cache(maxsize=None)
def tiny():
    from glow_tts_amd import _lib, audio
    assert V.TINY["intermediate_dim"] == 2 * _lib.lib().gt_vocos_hidden_chunk()
    torch.manual_seed(7)
    return V.init_for_tests(audio.Vocos(**V.TINY), 8).to(dev())


@functools.lru_cache(maxsize=None)
def tiny_batch():
    """(mel [B, 80, F_max] with NaN behind every utterance's frames, the frame counts)"""
    rng = np.random.default_rng(17)
    frames = (0, 1, 2, 3, 9, tile() + 1)
    mel = np.full((len(frames), 80, max(frames)), np.nan, dtype=np.float32)
    for b, n in enumerate(frames):
        mel[b, :, :n] = V.random_mel(rng, 80, n)
    return mel, frames


@functools.lru_cache(maxsize=None)
def tiny_wav():
    """forward of the tiny batch, computed once and shared"""
    mel, frames = tiny_batch()
    wav, wav_lengths = tiny()(torch.from_numpy(mel).to(dev()), torch.tensor(frames, dtype=torch.int32, device=dev()),
                              mel_lengths_host=list(frames))
    torch.cuda.synchronize()
    return wav, wav_lengths


def check_against_float64(name, voc, cfg, mel, frames, wav):
    """every utterance against the exact float64 generator on the module's fp32 weights, the bound from the emulation"""
    sd = {k: v.cpu() for k, v in voc.state_dict().items()}
    got = wav.double().cpu().numpy()
    assert got.shape == (len(frames), 256 * (mel.shape[2] - 1)) and np.isfinite(got).all()
    exact, emul, dev_ = [], [], []
    for b, n in enumerate(frames):
        L = 256 * max(n - 1, 0)
        assert not got[b, L:].any(), (name, b)                                     # exact zeros behind the utterance (no sample below 2 frames)
        ex, em = V.generator64(sd, cfg, mel[b, :, :n]), V.generator64(sd, cfg, mel[b, :, :n], emul=True)
        assert ex.shape == (L,)
        if L:
            eb, db = V.rel_l2(em, ex), V.rel_l2(got[b, :L], ex)
            print(f"{name} utt {b} F={n}: emulation {eb:.3e}, device {db:.3e}, ratio {db / eb:.3f}")
            assert 0 < eb and db <= 2 * eb, (name, b, db, eb)
        exact.append(ex); emul.append(em); dev_.append(got[b, :L])
    exact, emul, dev_ = (np.concatenate(v) for v in (exact, emul, dev_))
    e_emul, e_dev = V.rel_l2(emul, exact), V.rel_l2(dev_, exact)
    print(f"{name}: E_emul {e_emul:.3e}, device error {e_dev:.3e}, ratio {e_dev / e_emul:.3f} (bound 2)")
    assert 0 < e_emul < 0.05 and float(np.abs(exact).max()) > 1e-3
    assert e_dev <= 2 * e_emul, (e_dev, e_emul)


def test_tiny_config_ragged_batch(built):
    mel, frames = tiny_batch()
    wav, wav_lengths = tiny_wav()
    assert wav_lengths.tolist() == [256 * max(n - 1, 0) for n in frames]
    check_against_float64("tiny", tiny(), V.TINY, mel, frames, wav)


def test_published_shape(built):
    """13.5 M random parameters at 512 / 1536 / 8 layers, B = 2, F = (5, 9): the only test that runs the whole model at C = 512"""
    from glow_tts_amd import _lib, audio
    torch.manual_seed(23)
    voc = V.init_for_tests(audio.Vocos(**V.PUBLISHED), 24).to(dev())
    rng = np.random.default_rng(29)
    frames = (5, 9)
    mel = np.full((2, 80, 9), np.nan, dtype=np.float32)
    for b, n in enumerate(frames):
        mel[b, :, :n] = V.random_mel(rng, 80, n)
    voc.images(), voc.istft._image()                                               # packed outside the launches that are counted
    with _lib.record_calls() as names:
        wav, _ = voc(torch.from_numpy(mel).to(dev()), torch.tensor(frames, dtype=torch.int32, device=dev()))
    launches = [n for n in names if n in ("gt_voc_conv", "gt_vocos_norm", "gt_vocos_mlp", "gt_vocos_polar", "gt_istft")]
    assert len(launches) == voc.launches == 22
    assert [launches.count(n) for n in ("gt_voc_conv", "gt_vocos_norm", "gt_vocos_mlp", "gt_vocos_polar", "gt_istft")] == [2, 10, 8, 1, 1]
    check_against_float64("published", voc, V.PUBLISHED, mel, frames, wav)


def test_batch_independence_and_capacity_form(built):
    """a batch row is bit-identical to the utterance vocoded alone; run() into a workspace of larger capacity (B + 1, F_max + 11), stale NaN
    patterns in every buffer, is bit-identical to forward()"""
    voc = tiny()
    mel, frames = tiny_batch()
    B, F_max = mel.shape[0], mel.shape[2]
    mel_d = torch.from_numpy(mel).to(dev())
    wav, _ = tiny_wav()
    for b, n in enumerate(frames):
        if n >= 2:
            alone = voc(mel_d[b:b + 1, :, :n].contiguous())
            assert alone.shape == (1, 256 * (n - 1))
            assert torch.equal(alone[0].view(torch.int32), wav[b, :256 * (n - 1)].view(torch.int32)), b
    bufs = voc.workspace(B + 1, F_max + 11, dev())
    assert sorted(bufs) == ["a", "o", "spec", "wav", "x"]
    for t in bufs.values():
        t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32).fill_(-1)             # NaN patterns: nothing stale may matter
    big = torch.full((B + 1, 80, F_max + 16), float("nan"), device=dev())
    big[:B, :, :F_max] = mel_d
    n_frames = torch.tensor(list(frames) + [0], dtype=torch.int32, device=dev())
    out = voc.run(big, n_frames, bufs)
    assert out.shape == (B + 1, 256 * (F_max + 10)) and out is bufs["wav"]
    assert torch.equal(out[:B, :256 * (F_max - 1)].view(torch.int32), wav.view(torch.int32))
    assert not bool(out[:B, 256 * (F_max - 1):].any()) and not bool(out[B].any())


def test_images_follow_the_weights_and_cpu_mel_raises(built):
    from glow_tts_amd import audio
    torch.manual_seed(31)
    voc = V.init_for_tests(audio.Vocos(**V.TINY), 32).to(dev())
    mel = torch.from_numpy(V.random_mel(np.random.default_rng(3), 80, 6)).to(dev())[None]
    w0 = voc(mel)
    assert w0.shape == (1, 256 * 5) and float(w0.abs().max()) > 0
    imgs = voc.images()
    assert voc.images() is imgs
    with torch.no_grad():
        voc.backbone.convnext[1].gamma.mul_(0.5)                                               # an in-place edit: _version moves
    assert voc.images() is not imgs
    assert not torch.equal(voc(mel), w0)
    with torch.no_grad():
        voc.backbone.convnext[1].gamma.mul_(2.0)                                               # exact: back to the first weights
    assert torch.equal(voc(mel), w0)
    imgs = voc.images()
    voc = voc.to("cpu").to(dev())                                                              # new storage: rebuilt
    assert voc.images() is not imgs and torch.equal(voc(mel), w0)
    with pytest.raises(audio.CpuWaveError):
        voc(mel.cpu())
    with pytest.raises(ValueError):
        voc(mel[:, :40])
    assert voc(mel[:, :, :1]).shape == (1, 0)                                                  # one frame: no sample


def test_padded_band_count(built):
    """a 100-band model: forward pads the mel to 112 channels, the result is that of the 112-band model with zero weights there"""
    from glow_tts_amd import audio
    torch.manual_seed(33)
    cfg = dict(V.TINY, input_channels=100)
    voc = V.init_for_tests(audio.Vocos(**cfg), 34).to(dev())
    rng = np.random.default_rng(35)
    mel = V.random_mel(rng, 100, 7)[None]
    wav = voc(torch.from_numpy(mel).to(dev()))
    check_against_float64("100 bands", voc, cfg, mel, (7,), wav)
