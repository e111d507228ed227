"""GPU tests of the vocoder module (glow_tts_amd.audio.HiFiGAN on csrc/hifigan.hip).

The tolerance is measured, not fixed: tests/hifigan64.py has the exact float64 generator and a CPU EMULATION of the kernel's numerics
(operands rounded to bf16 where the kernel rounds them, everything else float64).  E_emul = ||emul - exact|| / ||exact|| is computed
here, on the CPU, for the same weights and mel (over all samples of the batch), and the device must satisfy
||gpu - exact|| / ||exact|| <= 2 E_emul: the factor 2 covers different realisations of the same rounding model (fp32 accumulation
order flips individual bf16 roundings, the error model is the same).  Each test prints E_emul and the measured ratio.

Measured on an MI355X (ratio = device error / E_emul over the batch; the bound is 2; per utterance the ratio was 1.000 - 1.037):
  tiny, resblock "1"   E_emul 6.60e-03, device 6.67e-03, ratio 1.010
  tiny, resblock "2"   E_emul 5.78e-03, device 5.83e-03, ratio 1.009
  V1 at full width     E_emul 2.76e-03, device 2.78e-03, ratio 1.007
The same bound is asked of every utterance on its own samples.
"""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hifigan64 as H  # noqa: E402

pytestmark = pytest.mark.gpu


def dev():
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def tiny(resblock):
    from glow_tts_amd import audio
    torch.manual_seed(7 + int(resblock))
    return audio.HiFiGAN(resblock=resblock, **H.TINY).to(dev())


@functools.lru_cache(maxsize=None)
def tiny_batch():
    """(mel [B, 80, F_max] with NaN behind every utterance's frames, the frame counts)"""
    rng = np.random.default_rng(17)
    frames = H.TINY_FRAMES
    mel = np.full((len(frames), 80, max(frames)), np.nan, dtype=np.float32)
    for b, n in enumerate(frames):
        mel[b, :, :n] = H.random_mel(rng, 80, n)
    return mel, frames


def check_against_float64(name, voc, cfg, resblock, mel, frames, wav):
    """every utterance against the exact float64 generator on the module's fp32 weights, the bound from the emulation"""
    U = voc.hop_length
    sd = {k: v.cpu() for k, v in voc.state_dict().items()}
    got = wav.double().cpu().numpy()
    assert got.shape == (len(frames), U * mel.shape[2]) and np.isfinite(got).all()
    exact, emul, dev_ = [], [], []
    for b, n in enumerate(frames):
        assert not got[b, U * n:].any(), (name, b)                                  # exact zeros behind the utterance (all of row F_b = 0)
        ex = H.generator64(sd, cfg, mel[b, :, :n], resblock)
        em = H.generator64(sd, cfg, mel[b, :, :n], resblock, emul=True)
        assert ex.shape == (U * n,)
        if n:
            eb, db = H.rel_l2(em, ex), H.rel_l2(got[b, :U * n], ex)
            print(f"{name} utt {b} F={n}: emulation {eb:.3e}, device {db:.3e}, ratio {db / eb:.3f}")
            assert 0 < eb and db <= 2 * eb, (name, b, db, eb)
        exact.append(ex); emul.append(em); dev_.append(got[b, :U * n])
    exact, emul, dev_ = (np.concatenate(v) for v in (exact, emul, dev_))
    e_emul, e_dev = H.rel_l2(emul, exact), H.rel_l2(dev_, exact)
    print(f"{name}: E_emul {e_emul:.3e}, device error {e_dev:.3e}, ratio {e_dev / e_emul:.3f} (bound 2)")
    assert 0 < e_emul < 0.05 and float(np.abs(exact).max()) > 1e-3
    assert e_dev <= 2 * e_emul, (e_dev, e_emul)


@pytest.mark.parametrize("resblock", ["1", "2"])
def test_tiny_config_ragged_batch(built, resblock):
    voc = tiny(resblock)
    mel, frames = tiny_batch()
    lengths = torch.tensor(frames, dtype=torch.int32, device=dev())
    wav, wav_lengths = voc(torch.from_numpy(mel).to(dev()), lengths, mel_lengths_host=list(frames))
    assert wav_lengths.tolist() == [8 * n for n in frames]
    check_against_float64(f'tiny resblock "{resblock}"', voc, H.TINY, resblock, mel, frames, wav)


def test_v1_at_full_width(built):
    """13 926 017 random parameters, B = 2, F = (5, 9): the only test that sees 512-channel layers, N = 2048 and the 64 -> 2 * 32 stage"""
    from glow_tts_amd import _lib, audio
    torch.manual_seed(23)
    voc = audio.HiFiGAN().to(dev())
    assert sum(p.numel() for p in voc.parameters()) == 13926017
    rng = np.random.default_rng(29)
    frames = (5, 9)
    mel = np.full((2, 80, 9), np.nan, dtype=np.float32)
    for b, n in enumerate(frames):
        mel[b, :, :n] = H.random_mel(rng, 80, n)
    with _lib.record_calls() as names:
        wav, _ = voc(torch.from_numpy(mel).to(dev()), torch.tensor(frames, dtype=torch.int32, device=dev()))
    assert names.count("gt_voc_conv") == voc.launches == 78
    check_against_float64("V1", voc, H.V1, "1", mel, frames, wav)


def test_batch_independence_and_capacity_form(built):
    """a batch row is bit-identical to the utterance vocoded alone; run() into a workspace of larger capacity (B + 1, F_max + 11) is
    bit-identical to forward()"""
    voc = tiny("1")
    mel, frames = tiny_batch()
    B, F_max = mel.shape[0], mel.shape[2]
    mel_d = torch.from_numpy(mel).to(dev())
    wav, _ = voc(mel_d, torch.tensor(frames, dtype=torch.int32, device=dev()))
    for b, n in enumerate(frames):
        if n:
            alone = voc(mel_d[b:b + 1, :, :n].contiguous())
            assert alone.shape == (1, 8 * n)
            assert torch.equal(alone[0].view(torch.int32), wav[b, :8 * n].view(torch.int32)), b
    bufs = voc.workspace(B + 1, F_max + 11, dev())
    for t in bufs.values():
        t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32).fill_(-1)             # NaN patterns: nothing stale may matter
    big = torch.full((B + 1, 80, F_max + 16), float("nan"), device=dev())
    big[:B, :, :F_max] = mel_d
    n_frames = torch.tensor(list(frames) + [0], dtype=torch.int32, device=dev())
    out = voc.run(big, n_frames, bufs)
    assert out.shape == (B + 1, 8 * (F_max + 11)) and out is bufs["wav"]
    assert torch.equal(out[:B, :8 * F_max].view(torch.int32), wav.view(torch.int32))
    assert not bool(out[:B, 8 * F_max:].any()) and not bool(out[B].any())


def test_images_follow_the_weights_and_cpu_mel_raises(built):
    from glow_tts_amd import audio
    torch.manual_seed(31)
    voc = audio.HiFiGAN(resblock="2", **H.TINY).to(dev())
    mel = torch.from_numpy(H.random_mel(np.random.default_rng(3), 80, 6)).to(dev())[None]
    w0 = voc(mel)
    imgs = voc.images()
    assert voc.images() is imgs and len(imgs) == voc.launches
    with torch.no_grad():
        voc.conv_post.weight.mul_(0.5)                                                         # an in-place edit: _version moves
    assert voc.images() is not imgs
    w1 = voc(mel)
    assert not torch.equal(w0, w1)
    with torch.no_grad():
        voc.conv_post.weight.mul_(2.0)                                                         # exact: back to the first weights
    assert torch.equal(voc(mel), w0)
    imgs = voc.images()
    voc = voc.to("cpu").to(dev())                                                              # new storage: rebuilt
    assert voc.images() is not imgs and torch.equal(voc(mel), w0)
    with pytest.raises(audio.CpuWaveError):
        voc(mel.cpu())
    with pytest.raises(ValueError):
        voc(mel[:, :40])
