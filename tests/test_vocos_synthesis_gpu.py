"""GPU tests of text to waveform through the Vocos vocoder inside the captured graph (FlowGenerator.compile_synthesis(vocoder=
audio.Vocos(...)), SynthesisHandle.wav(); glow-tts_amd/synthesis.py) on the small model of
tests/test_synthesis_graph_gpu.py with the tiny Vocos of tests/vocos64.py and max_frames = 64, modelled on
tests/test_hifigan_synthesis_gpu.py.

The kernels are deterministic and an utterance's samples depend on its own mel alone, at any capacity: h.wav() must be BIT-IDENTICAL
to vocoder(h.mel(), 2 (lengths // 2)), with Griffin-Lim's length rule 256 max(2 (len // 2) - 1, 0)."""
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "golden"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import vocos64 as V  # noqa: E402
from test_synthesis_graph_gpu import B, TX, build_generator, eager, rows_needed, texts  # noqa: E402

pytestmark = pytest.mark.gpu
MAX_FRAMES = 64
CALLS = ((5, 0.667, 10.0), (9, 0.3, 16.0))                                         # tests/test_hifigan_synthesis_gpu.py's
OVERFLOW = (7, 0.5, 65.0)


def dev():
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def vocoder():
    from glow_tts_amd import audio
    torch.manual_seed(41)
    return V.init_for_tests(audio.Vocos(**V.TINY), 42).to(dev())


def eager_wav(y, lens):
    frames = [2 * (v // 2) for v in lens]
    wav, wav_len = vocoder()(y, torch.tensor(frames, dtype=torch.int32, device=dev()), mel_lengths_host=frames)
    torch.cuda.synchronize()
    return wav, wav_len.tolist()


@functools.lru_cache(maxsize=None)
def setup():
    gen, _ = build_generator()
    tx = texts()
    probe = [eager(gen, ids, xl, *c)["lens"] for ids, xl in tx for c in CALLS]
    assert min(min(v) for v in probe) >= 2 and max(max(v) for v in probe) <= MAX_FRAMES, probe
    over = eager(gen, *tx[0], *OVERFLOW)["lens"]
    assert max(over) > MAX_FRAMES, over
    max_rows = -(-max(rows_needed(v) for v in probe + [over]) // 128) * 128
    gen.rows_cfg.row_round = max_rows
    refs = {}
    for i, (ids, xl) in enumerate(tx):
        for j, c in enumerate(CALLS):
            r = eager(gen, ids, xl, *c)
            r["wav"], r["wav_len"] = eager_wav(r["y"], r["lens"])
            refs[(i, j)] = r
    plain = gen.compile_synthesis(B, TX, MAX_FRAMES, max_rows=max_rows)
    synth = gen.compile_synthesis(B, TX, MAX_FRAMES, max_rows=max_rows, vocoder=vocoder(), vocoder_iters=3)    # iters: ignored
    return gen, tx, refs, synth, plain


def test_wav_equals_the_eager_vocoder(built):
    gen, tx, refs, synth, plain = setup()
    graph = synth.graph
    assert synth.wav_static.shape == (B, 256 * (MAX_FRAMES - 1))
    assert synth.captured_entries == plain.captured_entries + vocoder().launches == plain.captured_entries + 10
    for i, (ids, xl) in enumerate(tx):
        for j, (seed, ns, ls) in enumerate(CALLS):
            ref = refs[(i, j)]
            h = synth(ids, xl, seed=seed, noise_scale=ns, length_scale=ls)
            assert h.status == 0 and h.lengths() == ref["lens"]
            wav, wav_len = h.wav()
            T = max(ref["lens"]) // 2 * 2
            assert wav_len == ref["wav_len"] == [256 * max(2 * (v // 2) - 1, 0) for v in ref["lens"]]
            assert wav.shape == ref["wav"].shape == (B, 256 * (T - 1)) and wav.dtype == torch.float32
            y = h.mel()
            assert torch.equal(y, ref["y"])
            again, again_len = eager_wav(y, h.lengths())
            assert again_len == wav_len and torch.equal(wav.view(torch.int32), again.view(torch.int32))
            assert torch.equal(wav.view(torch.int32), ref["wav"].view(torch.int32))
            for b, n in enumerate(wav_len):
                assert not bool(wav[b, n:].any()) and float(wav[b, :n].abs().max()) > 0, b
            assert not bool(synth.wav_static[:, 256 * (T - 1):].any())
    assert synth.graph is graph and synth.overflows == 0 and synth.guards_intact()
    assert not torch.equal(refs[(0, 0)]["wav"][:, :256], refs[(1, 0)]["wav"][:, :256])


def test_overflow_falls_back_to_the_eager_waveform(built):
    from glow_tts_amd.synthesis import SynthesisOverflow
    gen, tx, refs, synth, plain = setup()
    ids, xl = tx[0]
    seed, ns, ls = OVERFLOW
    want = eager(gen, ids, xl, seed, ns, ls)
    want_wav, want_len = eager_wav(want["y"], want["lens"])
    before = synth.overflows
    h = synth(ids, xl, seed=seed, noise_scale=ns, length_scale=ls)
    assert h.status != 0 and h.lengths() == want["lens"]
    with pytest.raises(SynthesisOverflow):
        h.wav(fallback=False)
    wav, wav_len = h.wav()
    assert wav_len == want_len and wav.shape == want_wav.shape and torch.equal(wav, want_wav)
    assert torch.equal(h.mel(), want["y"]) and synth.overflows == before + 1 and synth.guards_intact()
    seed, ns, ls = CALLS[0]
    h = synth(ids, xl, seed=seed, noise_scale=ns, length_scale=ls)
    assert h.status == 0 and torch.equal(h.wav()[0], refs[(0, 0)]["wav"])


def test_vocoder_refusals(built):
    from glow_tts_amd import audio
    gen, tx, refs, synth, plain = setup()
    with pytest.raises(ValueError, match="mel channels, the model"):
        gen.compile_synthesis(B, TX, MAX_FRAMES, vocoder=audio.Vocos(**dict(V.TINY, input_channels=64)).to(dev()))
    with pytest.raises(ValueError, match="multiples of 16"):
        gen.compile_synthesis(B, TX, MAX_FRAMES, vocoder=audio.Vocos(**dict(V.TINY, input_channels=100)).to(dev()))
    with pytest.raises(ValueError, match="device"):
        gen.compile_synthesis(B, TX, MAX_FRAMES, vocoder=audio.Vocos(**V.TINY))
