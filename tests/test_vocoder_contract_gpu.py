"""GPU test of the contract the three neural vocoders meet (glow_tts_amd.audio._MelVocoder), said once for all of them:
workspace(B, F_max) holds what buffer_spec names and wav [B, wav_len(F_max)]; run() into a workspace of larger capacity, stale NaN
patterns in every buffer and a mel of larger pitch, is bit-identical to forward() on the ragged batch TINY_FRAMES — whose 0-, 1- and
2-frame utterances are where the two length rules (U F and 256 (F - 1)) part — and exact zero behind every utterance and in the extra
row.  The modules are the tiny ones of tests/test_{hifigan,bigvgan,vocos}_gpu.py under those files' seeds.  A Vocos of 100 bands has no
run() (forward pads its mel): it is asked for the refusal and for forward's lengths and zeros."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bigvgan64 as G  # noqa: E402
import hifigan64 as H  # noqa: E402
import vocos64 as V  # noqa: E402

pytestmark = pytest.mark.gpu
FRAMES = H.TINY_FRAMES
CASES = ["hifigan1", "hifigan2", "bigvgan24", "bigvgan2", "vocos", "vocos100"]


def dev():
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def module(case):
    from glow_tts_amd import audio
    if case.startswith("hifigan"):
        torch.manual_seed(7 + int(case[-1]))
        return audio.HiFiGAN(resblock=case[-1], **H.TINY).to(dev())
    if case.startswith("bigvgan"):
        cfg, kw, seed = {"bigvgan24": (G.TINY24, dict(resblock="1", activation="snakebeta"), 9),
                         "bigvgan2": (G.TINY, dict(resblock="2", activation="snake"), 8)}[case]
        voc = audio.BigVGAN(n_mel_channels=16, **cfg, **kw)
        voc.load_generator_state(G.seeded(cfg, seed, n_mel=16, **kw).state_dict())
        return voc.to(dev())
    if case == "vocos":
        torch.manual_seed(7)
        return V.init_for_tests(audio.Vocos(**V.TINY), 8).to(dev())
    torch.manual_seed(33)
    return V.init_for_tests(audio.Vocos(**dict(V.TINY, input_channels=100)), 34).to(dev())


@pytest.mark.parametrize("case", CASES)
def test_capacity_form_equals_forward(built, case):
    voc = module(case)
    n_mel = voc.mel_channels - voc.mel_padding
    B, F_max = len(FRAMES), max(FRAMES)
    rng = np.random.default_rng(17)
    mel = np.full((B, n_mel, F_max), np.nan, dtype=np.float32)
    for b, n in enumerate(FRAMES):
        mel[b, :, :n] = H.random_mel(rng, n_mel, n)
    mel_d = torch.from_numpy(mel).to(dev())
    wav, wav_lengths = voc(mel_d, torch.tensor(FRAMES, dtype=torch.int32, device=dev()), mel_lengths_host=list(FRAMES))
    assert wav.shape == (B, voc.wav_len(F_max)) and wav_lengths.tolist() == [voc.wav_len(n) for n in FRAMES]
    assert bool(torch.isfinite(wav).all()) and bool(wav.abs().max() > 1e-3)
    for b, n in enumerate(FRAMES):
        assert not bool(wav[b, voc.wav_len(n):].any()), b                           # exact zeros behind the utterance
        assert not voc.wav_len(n) or bool(wav[b, :voc.wav_len(n)].any()), b

    Bc, Fc = B + 1, F_max + 11
    spec = voc.buffer_spec(Bc, Fc)
    bufs = voc.workspace(Bc, Fc, dev())
    assert list(bufs) == [name for name, _, _ in spec] + ["wav"]
    assert [(t.dtype, t.numel()) for t in bufs.values()] == [(dt, n) for _, dt, n in spec] + [(torch.float32, Bc * voc.wav_len(Fc))]
    assert bufs["wav"].shape == (Bc, voc.wav_len(Fc)) and all(t.device == wav.device for t in bufs.values())
    assert sum(t.numel() * t.element_size() for t in bufs.values()) == voc.workspace_bytes(Bc, Fc)
    for t in bufs.values():
        t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32).fill_(-1)             # NaN patterns: nothing stale may matter
    big = torch.full((Bc, n_mel, F_max + 16), float("nan"), device=dev())
    big[:B, :, :F_max] = mel_d
    n_frames = torch.tensor(list(FRAMES) + [0], dtype=torch.int32, device=dev())
    if voc.mel_padding:
        with pytest.raises(ValueError, match="forward pads"):
            voc.run(big, n_frames, bufs)
        return
    out = voc.run(big, n_frames, bufs)
    assert out is bufs["wav"]
    assert torch.equal(out[:B, :voc.wav_len(F_max)].view(torch.int32), wav.view(torch.int32))
    assert not bool(out[:B, voc.wav_len(F_max):].any()) and not bool(out[B].any())
