"""GPU tests of text to NORMALISED waveform inside the captured graph: FlowGenerator.compile_synthesis(vocoder=audio.Normalized(
audio.Denoised(audio.WaveGlow(...)))) on the small model, the TINY flow and the capacities of tests/test_denoise_synthesis_gpu.py
(DESIGN.md 4.31).  audio.Normalized speaks the vocoder contract, so glow-tts_amd/synthesis.py has no line for it.

h.wav() must be BIT-IDENTICAL to the eager Normalized call on h.mel() with the call's seed; the graph grows by the inner vocoder's
entries + 2; the target and the ceiling are words the kernel reads on the device: set_target between two replays changes the next
h.wav() with no new capture; and a replay with other lengths leaves zeros behind every utterance."""
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "golden"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import waveglow64 as W  # noqa: E402
from test_hifigan_synthesis_gpu import CALLS, MAX_FRAMES, U  # noqa: E402
from test_synthesis_graph_gpu import B, TX, build_generator, eager, rows_needed, texts  # noqa: E402

pytestmark = pytest.mark.gpu
TARGET = -23.0


def dev():
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def vocoder():
    from glow_tts_amd import audio
    inner = audio.Denoised(W.init_for_tests(audio.WaveGlow(**W.TINY), 41).to(dev()), strength=0.1)
    return audio.Normalized(inner, target_lufs=TARGET)


def eager_wav(y, lens, seed):
    frames = [2 * (v // 2) for v in lens]
    wav, wav_len = vocoder()(y, torch.tensor(frames, dtype=torch.int32, device=dev()), mel_lengths_host=frames, seed=seed)
    torch.cuda.synchronize()
    return wav, wav_len.tolist()


@functools.lru_cache(maxsize=None)
def setup():
    gen, _ = build_generator()
    tx = texts()
    probe = [eager(gen, ids, xl, *c)["lens"] for ids, xl in tx for c in CALLS]
    assert min(min(v) for v in probe) >= 2 and max(max(v) for v in probe) <= MAX_FRAMES, probe
    max_rows = -(-max(rows_needed(v) for v in probe) // 128) * 128
    gen.rows_cfg.row_round = max_rows
    plain = gen.compile_synthesis(B, TX, MAX_FRAMES, max_rows=max_rows)
    synth = gen.compile_synthesis(B, TX, MAX_FRAMES, max_rows=max_rows, vocoder=vocoder())
    return gen, tx, synth, plain


def test_wav_equals_the_eager_normalized_vocoder(built):
    gen, tx, synth, plain = setup()
    norm = vocoder()
    norm.set_target(TARGET)
    assert synth.wav_static.shape == (B, U * MAX_FRAMES)
    assert synth.captured_entries == plain.captured_entries + norm.vocoder.launches + 2 == plain.captured_entries + norm.launches
    assert norm.launches == norm.vocoder.vocoder.launches + 4
    ids, xl = tx[0]
    for seed, ns, ls in CALLS:
        h = synth(ids, xl, seed=seed, noise_scale=ns, length_scale=ls)
        assert h.status == 0
        wav, wav_len = h.wav()
        want, want_len = eager_wav(h.mel(), h.lengths(), seed)
        assert want_len == wav_len and wav.shape == want.shape and torch.equal(wav.view(torch.int32), want.view(torch.int32))
        frames = torch.tensor([2 * (v // 2) for v in h.lengths()], dtype=torch.int32, device=dev())
        inner, _ = norm.vocoder(h.mel(), frames, seed=seed)
        assert not torch.equal(inner, want)                                                   # the stage is in the graph
        for b, n in enumerate(wav_len):
            assert not bool(wav[b, n:].any()) and float(wav[b, :n].abs().max()) > 0, b
    assert synth.overflows == 0 and synth.guards_intact()


def test_set_target_reaches_the_next_replay_without_a_new_capture(built):
    gen, tx, synth, _ = setup()
    norm = vocoder()
    ids, xl = tx[0]
    seed, ns, ls = CALLS[0]
    graph, entries = synth.graph, synth.captured_entries
    seen = {}
    try:
        for target, peak in ((-23.0, -1.0), (-30.0, -1.0), (20.0, -6.0), (-23.0, -1.0)):
            norm.set_target(target, peak)
            h = synth(ids, xl, seed=seed, noise_scale=ns, length_scale=ls)
            assert h.status == 0
            wav, wav_len = h.wav(clone=True)
            want, _ = eager_wav(h.mel(), h.lengths(), seed)
            assert torch.equal(wav.view(torch.int32), want.view(torch.int32)), target
            if (target, peak) in seen:
                assert torch.equal(seen[target, peak], wav)
            seen[target, peak] = wav
            if target == 20.0:                                                                # the ceiling holds every utterance
                for b, n in enumerate(wav_len):
                    assert abs(float(wav[b, :n].abs().max()) - 10.0 ** (-6.0 / 20.0)) <= 1e-6, b
        quiet, loud = seen[-30.0, -1.0], seen[-23.0, -1.0]
        assert not torch.equal(quiet, loud)
        assert quiet.double().norm().item() < loud.double().norm().item()
    finally:
        norm.set_target(TARGET, -1.0)
    assert synth.graph is graph and synth.captured_entries == entries and synth.guards_intact()


def test_a_replay_with_other_lengths_leaves_zeros_behind_every_utterance(built):
    gen, tx, synth, _ = setup()
    vocoder().set_target(TARGET, -1.0)
    seen = []
    for (ids, xl), (seed, ns, ls) in ((tx[0], CALLS[0]), (tx[-1], CALLS[-1]), (tx[0], CALLS[0])):
        h = synth(ids, xl, seed=seed, noise_scale=ns, length_scale=ls)
        assert h.status == 0
        wav, wav_len = h.wav(clone=True)
        want, want_len = eager_wav(h.mel(), h.lengths(), seed)
        assert wav_len == want_len and torch.equal(wav.view(torch.int32), want.view(torch.int32))
        for b, n in enumerate(wav_len):
            assert not bool(wav[b, n:].any()), b
        seen.append((wav_len, wav))
    assert seen[0][0] != seen[1][0]                                                           # the lengths did change in between
    assert seen[0][0] == seen[2][0] and torch.equal(seen[0][1], seen[2][1])
    assert synth.guards_intact()
