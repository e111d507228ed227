"""GPU tests of the BigVGAN module (glow_tts_amd.audio.BigVGAN: gt_voc_snake in front of gt_voc_conv).

The numeric rule is tests/test_hifigan_gpu.py's own: tests/bigvgan64.py has the exact float64 generator and a CPU EMULATION of the
device's numerics (bf16 where the device rounds: every activation's output, the packed weights, gt_voc_conv's rounding of the mel and
of a transposed convolution's input; everything else float64).  Per utterance and over the batch
    rel_l2(device, exact) <= 2 rel_l2(emul, exact),   0 < rel_l2(emul, exact) < 0.05,   max |exact| > 1e-3
— the last two are conditions on the seeded weights and alpha, met by the emulation alone on the CPU.  Each test prints the figures.

TINY24 (96 -> 48 -> 24 channels) exercises the host padding of a 24-channel stage to 32.  Its real channels are compared bit for bit
with the same weights run UNPADDED with a 32-channel last stage whose extra channels are zero.  That generator is 96 -> 48 -> 32: the
constructor only halves, so the test widens the last stage's modules of a TINY24 module by hand.  (128 -> 64 -> 32 is no such
comparison: 128 and 64 input channels put gt_voc_conv on its 64-channel chunk where 96 and 48 take the 32-channel one, a different
fp32 summation order in the FIRST stages, which no padding touches.)"""
import functools
import os
import sys

import numpy as np
import pytest
import torch
from torch import nn

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bigvgan64 as G  # noqa: E402

pytestmark = pytest.mark.gpu
N_MEL = 16
CASES = {"tiny1": (G.TINY, dict(resblock="1", activation="snakebeta")), "tiny2": (G.TINY, dict(resblock="2", activation="snake")),
         "tiny24": (G.TINY24, dict(resblock="1", activation="snakebeta"))}
SEEDS = {"tiny1": 7, "tiny2": 8, "tiny24": 9}


def dev():
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def source(case):
    """the seeded torch generator of a case (CPU, fp32): the source of its state dict"""
    cfg, kw = CASES[case]
    return G.seeded(cfg, SEEDS[case], n_mel=N_MEL, **kw)


@functools.lru_cache(maxsize=None)
def module(case):
    from glow_tts_amd import audio
    cfg, kw = CASES[case]
    voc = audio.BigVGAN(n_mel_channels=N_MEL, **cfg, **kw)
    voc.load_generator_state(source(case).state_dict())
    return voc.to(dev())


@functools.lru_cache(maxsize=None)
def tiny_batch():
    """(mel [B, 16, F_max] with NaN behind every utterance's frames, the frame counts)"""
    rng = np.random.default_rng(17)
    frames = G.TINY_FRAMES
    mel = np.full((len(frames), N_MEL, max(frames)), np.nan, dtype=np.float32)
    for b, n in enumerate(frames):
        mel[b, :, :n] = G.random_mel(rng, N_MEL, n)
    return mel, frames


@functools.lru_cache(maxsize=None)
def references(case):
    """[(exact, emul)] per utterance of the tiny batch: float64 on the CPU, computed once"""
    cfg, kw = CASES[case]
    sd = {k: v.cpu() for k, v in source(case).state_dict().items()}
    mel, frames = tiny_batch()
    full = dict(cfg, **kw)
    return [(G.generator64(sd, full, mel[b, :, :n]), G.generator64(sd, full, mel[b, :, :n], emul=True)) for b, n in enumerate(frames)]


def check_against_float64(name, U, frames, refs, wav):
    got = wav.double().cpu().numpy()
    assert got.shape[0] == len(frames) and np.isfinite(got).all()
    exact, emul, dev_ = [], [], []
    for b, n in enumerate(frames):
        assert not got[b, U * n:].any(), (name, b)                                  # exact zeros behind the utterance
        ex, em = refs[b]
        assert ex.shape == (U * n,)
        if n:
            eb, db = G.rel_l2(em, ex), G.rel_l2(got[b, :U * n], ex)
            print(f"{name} utt {b} F={n}: emulation {eb:.3e}, device {db:.3e}, ratio {db / eb:.3f}")
            assert 0 < eb < 0.05 and db <= 2 * eb, (name, b, db, eb)
        exact.append(ex); emul.append(em); dev_.append(got[b, :U * n])
    exact, emul, dev_ = (np.concatenate(v) for v in (exact, emul, dev_))
    e_emul, e_dev = G.rel_l2(emul, exact), G.rel_l2(dev_, exact)
    print(f"{name}: E_emul {e_emul:.3e}, device error {e_dev:.3e}, ratio {e_dev / e_emul:.3f} (bound 2)")
    assert 0 < e_emul < 0.05 and float(np.abs(exact).max()) > 1e-3
    assert e_dev <= 2 * e_emul, (e_dev, e_emul)


def vocode(voc, mel, frames):
    lengths = torch.tensor(frames, dtype=torch.int32, device=dev())
    return voc(torch.from_numpy(mel).to(dev()), lengths, mel_lengths_host=list(frames))


@pytest.mark.parametrize("case", list(CASES))
def test_tiny_configs_ragged_batch(built, case):
    from glow_tts_amd import _lib
    voc = module(case)
    mel, frames = tiny_batch()
    voc.held()                                                                      # packed outside the launches that are counted
    with _lib.record_calls() as names:
        wav, wav_lengths = vocode(voc, mel, frames)
    U = voc.hop_length
    assert wav_lengths.tolist() == [U * n for n in frames] and wav.shape == (len(frames), U * max(frames))
    assert names.count("gt_voc_conv") == voc.conv_launches and names.count("gt_voc_snake") == voc.snake_launches
    assert len(names) == voc.launches == voc.conv_launches + voc.snake_launches
    check_against_float64(case, U, frames, references(case), wav)


def test_padding_leaves_the_real_channels_bit_equal(built):
    """TINY24 against the same weights at 96 -> 48 -> 32 unpadded, the eight extra channels zero (module docstring)"""
    from glow_tts_amd import audio
    voc = module("tiny24")
    cfg, kw = CASES["tiny24"]
    wide = audio.BigVGAN(n_mel_channels=N_MEL, **cfg, **kw)
    wide.load_generator_state(source("tiny24").state_dict())
    K = len(cfg["resblock_kernel_sizes"])
    wide.ups[1] = nn.ModuleList([nn.ConvTranspose1d(48, 32, 4, 2, padding=1)])
    for j, (k, ds) in enumerate(zip(cfg["resblock_kernel_sizes"], cfg["resblock_dilation_sizes"])):
        wide.resblocks[K + j] = audio._AMPBlock("1", 32, k, ds, "snakebeta", True)
    wide.activation_post = audio._Activation1d(32, "snakebeta", True)
    wide.conv_post = nn.Conv1d(32, 1, 7, padding=3)
    wide.channels, wide.padded_channels = [96, 48, 32], [96, 48, 32]
    narrow = voc.state_dict()
    with torch.no_grad():
        for name, p in wide.state_dict().items():
            src = narrow[name].cpu()
            p.zero_()                                                               # zero extra channels (log alpha 0, log beta 0)
            p[tuple(slice(0, n) for n in src.shape)] = src
    wide = wide.to(dev())
    assert wide.conv_post.weight.shape == (1, 32, 7) and not bool(wide.conv_post.weight[:, 24:].any())
    mel, frames = tiny_batch()
    a, _ = vocode(voc, mel, frames)
    b, _ = vocode(wide, mel, frames)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)) and bool(a.abs().max() > 1e-3)


def test_batch_independence_and_capacity_form(built):
    """a batch row is bit-identical to the utterance vocoded alone; run() into a workspace of larger capacity (B + 1, F_max + 11) is
    bit-identical to forward()"""
    voc = module("tiny24")
    mel, frames = tiny_batch()
    B, F_max, U = mel.shape[0], mel.shape[2], voc.hop_length
    mel_d = torch.from_numpy(mel).to(dev())
    wav, _ = voc(mel_d, torch.tensor(frames, dtype=torch.int32, device=dev()))
    for b, n in enumerate(frames):
        if n:
            alone = voc(mel_d[b:b + 1, :, :n].contiguous())
            assert alone.shape == (1, U * n)
            assert torch.equal(alone[0].view(torch.int32), wav[b, :U * n].view(torch.int32)), b
    bufs = voc.workspace(B + 1, F_max + 11, dev())
    assert set(bufs) == {"u", "r", "s", "t", "a", "wav"} and bufs["a"].dtype == torch.bfloat16 and bufs["t"].dtype == torch.float32
    assert sum(t.numel() * t.element_size() for t in bufs.values()) == voc.workspace_bytes(B + 1, F_max + 11)
    for t in bufs.values():
        t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32).fill_(-1)             # NaN patterns: nothing stale may matter
    big = torch.full((B + 1, N_MEL, F_max + 16), float("nan"), device=dev())
    big[:B, :, :F_max] = mel_d
    n_frames = torch.tensor(list(frames) + [0], dtype=torch.int32, device=dev())
    out = voc.run(big, n_frames, bufs)
    assert out.shape == (B + 1, U * (F_max + 11)) and out is bufs["wav"]
    assert torch.equal(out[:B, :U * F_max].view(torch.int32), wav.view(torch.int32))
    assert not bool(out[:B, U * F_max:].any()) and not bool(out[B].any())


def test_images_and_blocks_follow_alpha_and_cpu_mel_raises(built):
    from glow_tts_amd import audio
    cfg, kw = CASES["tiny2"]
    voc = audio.BigVGAN(n_mel_channels=N_MEL, **cfg, **kw)
    voc.load_generator_state(source("tiny2").state_dict())
    voc = voc.to(dev())
    mel = torch.from_numpy(G.random_mel(np.random.default_rng(3), N_MEL, 6)).to(dev())[None]
    w0 = voc(mel)
    held = voc.held()
    assert voc.held() is held and len(held[0]) == voc.conv_launches and len(held[1]) == voc.snake_launches
    with torch.no_grad():
        voc.activation_post.act.alpha.add_(0.5)                                                # an in-place edit: _version moves
    assert voc.held() is not held
    w1 = voc(mel)
    assert not torch.equal(w0, w1)
    with torch.no_grad():
        voc.activation_post.act.alpha.sub_(0.5)                                                # exact: back to the first alpha
    assert torch.equal(voc(mel), w0)
    with torch.no_grad():
        voc.resblocks[0].activations[0].upsample.filter.mul_(0.5)                              # a buffer counts too
    assert not torch.equal(voc(mel), w0)
    with pytest.raises(audio.CpuWaveError):
        voc(mel.cpu())
    with pytest.raises(ValueError):
        voc(mel[:, :8])


def test_without_tanh_the_samples_are_clamped(built):
    from glow_tts_amd import audio
    kw = dict(resblock="2", activation="snake", use_tanh_at_final=False, use_bias_at_final=False)
    src = G.seeded(G.TINY, 12, n_mel=N_MEL, **kw)
    with torch.no_grad():
        src.conv_post.weight.mul_(40.0)                                                        # drive samples past +-1
    voc = audio.BigVGAN(n_mel_channels=N_MEL, **G.TINY, **kw)
    voc.load_generator_state(src.state_dict())
    voc = voc.to(dev())
    assert voc.conv_post.bias is None
    mel = G.random_mel(np.random.default_rng(4), N_MEL, 9)
    wav = voc(torch.from_numpy(mel).to(dev())[None])[0].double().cpu().numpy()
    full = dict(G.TINY, **kw)
    ex, em = G.generator64(src.state_dict(), full, mel), G.generator64(src.state_dict(), full, mel, emul=True)
    assert float(np.abs(wav).max()) == 1.0 and float(np.abs(ex).max()) == 1.0 and 0 < (np.abs(ex) < 1).mean() < 1
    assert ((np.abs(wav) == 1) == (np.abs(ex) == 1)).mean() > 0.9
    eb, db = G.rel_l2(em, ex), G.rel_l2(wav, ex)
    print(f"clamped: emulation {eb:.3e}, device {db:.3e}")
    assert 0 < eb < 0.05 and db <= 2 * eb


def test_base_shape_at_full_width(built):
    """the published base shape with random parameters, B = 1, 8 frames: the 151 launches and finiteness only"""
    from glow_tts_amd import _lib, audio
    torch.manual_seed(23)
    voc = audio.BigVGAN().to(dev())
    mel = torch.from_numpy(G.random_mel(np.random.default_rng(29), 80, 8)).to(dev())[None]
    voc.held()                                                                      # packed outside the launches that are counted
    with _lib.record_calls() as names:
        wav = voc(mel)
    assert names.count("gt_voc_conv") == 78 and names.count("gt_voc_snake") == 73 and len(names) == voc.launches == 151
    assert wav.shape == (1, 256 * 8) and bool(torch.isfinite(wav).all()) and bool(wav.abs().max() > 0) and bool(wav.abs().max() <= 1)
