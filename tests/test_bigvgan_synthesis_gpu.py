"""GPU tests of text to waveform through the BigVGAN vocoder inside the captured graph (FlowGenerator.compile_synthesis(vocoder=
audio.BigVGAN(...)), SynthesisHandle.wav(); glow-tts_amd/synthesis.py) on the small model of
tests/test_synthesis_graph_gpu.py, with the tiny generator of tests/bigvgan64.py whose last stage has 24 channels (TINY24: 96 -> 48 ->
24, run at 32; 4 samples per frame) and max_frames = 64: the buffers the vocoder describes (buffer_spec: u, r, s, t and the bf16 a)
at the padded width, and both of its kernels in the graph.

The kernel is deterministic and an utterance's samples depend on its own mel alone, at any capacity: h.wav() must be BIT-IDENTICAL to
vocoder(h.mel(), 2 (lengths // 2)) — a difference is a defect of the plumbing (frame counts, buffers, strides), not a tolerance
question."""
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "golden"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bigvgan64 as G  # noqa: E402
from test_synthesis_graph_gpu import B, TX, build_generator, eager, rows_needed, texts  # noqa: E402

pytestmark = pytest.mark.gpu
U, MAX_FRAMES = 4, 64
# (seed, noise_scale, length_scale): the small model predicts less than one frame per token; these scales keep every utterance inside
# 64 frames, OVERFLOW's does not
CALLS = ((5, 0.667, 10.0), (9, 0.3, 16.0))
OVERFLOW = (7, 0.5, 65.0)


def dev():
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def vocoder():
    from glow_tts_amd import audio
    voc = audio.BigVGAN(n_mel_channels=80, **G.TINY24)
    voc.load_generator_state(G.seeded(G.TINY24, 41, n_mel=80).state_dict())
    return voc.to(dev())


def eager_wav(y, lens):
    frames = [2 * (v // 2) for v in lens]
    wav, wav_len = vocoder()(y, torch.tensor(frames, dtype=torch.int32, device=dev()), mel_lengths_host=frames)
    torch.cuda.synchronize()
    return wav, wav_len.tolist()


@functools.lru_cache(maxsize=None)
def setup():
    """the model, the eager references (mel and samples) of every (text, call) — computed ONCE — and two synthesisers of 64 frames: one
    with the vocoder, one without"""
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
    """two texts and two calls through the SAME graph, each bit-identical to its eager result; the graph grew by the vocoder's launches"""
    gen, tx, refs, synth, plain = setup()
    graph = synth.graph
    assert synth.wav_static.shape == (B, U * MAX_FRAMES)
    assert {k: (v.dtype, v.numel()) for k, v in synth.voc_bufs.items() if k != "wav"} == \
        {name: (dtype, n) for name, dtype, n in vocoder().buffer_spec(B, MAX_FRAMES)} and "a" in synth.voc_bufs
    assert [(name, n) for name, _, n in vocoder().buffer_spec(B, MAX_FRAMES)] == [(name, B * MAX_FRAMES * 128) for name in "ursta"]
    assert synth.captured_entries == plain.captured_entries + vocoder().launches == plain.captured_entries + 40 + 37
    for i, (ids, xl) in enumerate(tx):
        for j, (seed, ns, ls) in enumerate(CALLS):
            ref = refs[(i, j)]
            h = synth(ids, xl, seed=seed, noise_scale=ns, length_scale=ls)
            assert h.status == 0 and h.lengths() == ref["lens"]
            wav, wav_len = h.wav()
            T = max(ref["lens"]) // 2 * 2
            assert wav_len == ref["wav_len"] == [U * 2 * (v // 2) for v in ref["lens"]]
            assert wav.shape == ref["wav"].shape == (B, U * T) and wav.dtype == torch.float32
            y = h.mel()
            assert torch.equal(y, ref["y"])                                                    # the mel is still infer(seed=)'s
            again, again_len = eager_wav(y, h.lengths())                                       # vocoder(h.mel(), 2 (lengths // 2))
            assert again_len == wav_len and torch.equal(wav.view(torch.int32), again.view(torch.int32))
            assert torch.equal(wav.view(torch.int32), ref["wav"].view(torch.int32))
            for b, n in enumerate(wav_len):
                assert not bool(wav[b, n:].any()) and float(wav[b, :n].abs().max()) > 0, b
            assert not bool(synth.wav_static[:, U * T:].any())                                 # ... and to the end of the static rows
    assert synth.graph is graph and synth.overflows == 0 and synth.guards_intact()
    assert not torch.equal(refs[(0, 0)]["wav"][:, :U], refs[(1, 0)]["wav"][:, :U])


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
    # the graph is intact behind it
    seed, ns, ls = CALLS[0]
    h = synth(ids, xl, seed=seed, noise_scale=ns, length_scale=ls)
    assert h.status == 0 and torch.equal(h.wav()[0], refs[(0, 0)]["wav"])


def test_vocoder_refusals(built):
    from glow_tts_amd import audio
    gen, tx, refs, synth, plain = setup()
    with pytest.raises(ValueError, match="mel channels"):
        gen.compile_synthesis(B, TX, MAX_FRAMES, vocoder=audio.BigVGAN(n_mel_channels=64, **G.TINY24).to(dev()))
    with pytest.raises(ValueError, match="device"):
        gen.compile_synthesis(B, TX, MAX_FRAMES, vocoder=audio.BigVGAN(n_mel_channels=80, **G.TINY24))
    with pytest.raises(RuntimeError):
        plain(*tx[0], seed=1).wav()
