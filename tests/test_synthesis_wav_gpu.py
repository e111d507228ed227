"""GPU tests of text to WAVEFORM as one captured graph (FlowGenerator.compile_synthesis(vocoder=), SynthesisHandle.wav();
glow-tts_amd/synthesis.py) on the small model of tests/test_synthesis_graph_gpu.py, two Griffin-Lim iterations.

The kernels are deterministic, an utterance's samples depend on its own mel, its index and the seed alone, and the graph runs the
launches of the eager path at capacity sizes: h.wav() must be BIT-IDENTICAL to GriffinLim.from_mel(h.mel(), 2 (lengths // 2),
n_iters=2, seed=seed, phases="counter") — a difference is a defect of the plumbing (frame counts, seed word, buffers), not a
tolerance question.  The mel stays bit-identical to infer(seed=)."""
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "golden"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_synthesis_graph_gpu import B, TX, TRIPLES, build_generator, eager, rows_needed, texts  # noqa: E402

pytestmark = pytest.mark.gpu
HOP, ITERS = 256, 2


def dev():
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def vocoder():
    from glow_tts_amd import audio
    return audio.GriffinLim(audio.TacotronSTFT(n_mel_channels=80)).to(dev())


def eager_wav(y, lens, seed):
    """the eager path the graph must reproduce: from_mel with counter phases on the mel's real frame counts (all >= 4: the host checks)"""
    frames = [2 * (v // 2) for v in lens]
    wav, wav_len = vocoder().from_mel(y, torch.tensor(frames, dtype=torch.int32, device=dev()), mel_lengths_host=frames, n_iters=ITERS,
                                      seed=seed, phases="counter")
    torch.cuda.synchronize()
    return wav, wav_len.tolist()


@functools.lru_cache(maxsize=None)
def setup():
    """the model, the eager references (mel and samples) of every (text, triple) — computed ONCE — and two synthesisers at the
    capacities that hold them: one with the vocoder, one without"""
    gen, _ = build_generator()
    tx = texts()
    probe = [eager(gen, ids, xl, *t)["lens"] for ids, xl in tx for t in TRIPLES]
    assert min(min(v) for v in probe) >= 4 and max(max(v) for v in probe) > 64
    max_frames = (max(max(v) for v in probe) + 1) // 2 * 2
    max_rows = -(-max(rows_needed(v) for v in probe) // 128) * 128
    gen.rows_cfg.row_round = max_rows
    refs = {}
    for i, (ids, xl) in enumerate(tx):
        for j, t in enumerate(TRIPLES):
            r = eager(gen, ids, xl, *t)
            r["wav"], r["wav_len"] = eager_wav(r["y"], r["lens"], t[0])
            refs[(i, j)] = r
    plain = gen.compile_synthesis(B, TX, max_frames, max_rows=max_rows)
    synth = gen.compile_synthesis(B, TX, max_frames, max_rows=max_rows, vocoder=vocoder(), vocoder_iters=ITERS)
    return gen, tx, refs, synth, plain


def check_wav(h, ref):
    assert h.status == 0 and h.lengths() == ref["lens"]
    wav, wav_len = h.wav()
    assert wav_len == ref["wav_len"] == [HOP * max(2 * (v // 2) - 1, 0) for v in ref["lens"]]
    assert wav.shape == ref["wav"].shape == (B, HOP * (max(ref["lens"]) // 2 * 2 - 1)) and wav.dtype == torch.float32
    assert torch.equal(wav, ref["wav"])                                                    # bit-identical
    for b, n in enumerate(wav_len):
        assert not bool(wav[b, n:].any()) and float(wav[b, :n].abs().max()) > 0, b        # zero behind each utterance
    y = h.mel()
    assert y.shape == ref["y"].shape and torch.equal(y, ref["y"])                          # the mel is still infer(seed=)'s


def test_wav_equals_the_eager_path(built):
    gen, tx, refs, synth, plain = setup()
    graph = synth.graph
    for i, (ids, xl) in enumerate(tx):
        for j, (seed, ns, ls) in enumerate(TRIPLES):
            h = synth(ids, xl, seed=seed, noise_scale=ns, length_scale=ls)
            check_wav(h, refs[(i, j)])
            full = synth.wav_static
            n = HOP * (max(h.lengths()) // 2 * 2 - 1)
            assert not bool(full[:, n:].any())                                             # ... and to the end of the static rows
    assert synth.graph is graph and synth.overflows == 0 and synth.guards_intact()
    # the call's seed decides the phases with no re-capture: same mel inputs, another seed's samples differ at the same noise scale 0
    a = synth(*tx[0], seed=1, noise_scale=0.0, length_scale=40.0)
    wa, ya = a.wav(clone=True)[0], a.mel(clone=True)
    b = synth(*tx[0], seed=2, noise_scale=0.0, length_scale=40.0)
    wb, yb = b.wav(clone=True)[0], b.mel(clone=True)
    assert torch.equal(ya, yb) and wa.shape == wb.shape and not torch.equal(wa, wb)
    assert synth.n_frames.tolist() == [2 * (v // 2) for v in b.lengths()]


def test_a_handle_read_after_the_next_call_returns_its_own_samples(built):
    gen, tx, refs, synth, plain = setup()
    torch.cuda.synchronize()
    hs = []
    for key in ((0, 0), (1, 1), (0, 1)):
        seed, ns, ls = TRIPLES[key[1]]
        hs.append((key, synth(*tx[key[0]], seed=seed, noise_scale=ns, length_scale=ls)))
    for key, h in hs:
        wav, wav_len = h.wav(clone=True)
        assert wav_len == refs[key]["wav_len"] and torch.equal(wav, refs[key]["wav"]), key
        assert torch.equal(h.mel(clone=True), refs[key]["y"]), key
    assert synth.guards_intact()


def test_wav_of_an_overwritten_call_raises(built):
    """wav() marks the call as read, like mel(): the next call overwrites the static buffers without a copy aside, and asking the
    first handle again raises instead of returning the later call's samples"""
    gen, tx, refs, synth, plain = setup()
    (s0, ns0, ls0), (s1, ns1, ls1) = TRIPLES
    h = synth(*tx[0], seed=s0, noise_scale=ns0, length_scale=ls0)
    wav = h.wav(clone=True)[0]
    assert torch.equal(wav, refs[(0, 0)]["wav"]) and torch.equal(h.wav()[0], wav)         # asked twice before the next call: the same
    h2 = synth(*tx[1], seed=s1, noise_scale=ns1, length_scale=ls1)
    assert h._saved is None                                                                # read already: nothing was moved aside
    with pytest.raises(RuntimeError, match="later call"):
        h.wav()
    assert torch.equal(h2.wav()[0], refs[(1, 1)]["wav"]) and torch.equal(wav, refs[(0, 0)]["wav"])
    assert synth._voc_images is not None and len(synth._voc_images) == 3 and plain._voc_images is None


def test_without_a_vocoder(built):
    gen, tx, refs, synth, plain = setup()
    assert plain.vocoder is None and plain.wav_static is None and plain.n_frames is None
    # the vocoder adds its 1 + 1 + 2 n launches to the graph and nothing else; without it the graph is the one it was
    assert synth.captured_entries == plain.captured_entries + 2 + 2 * ITERS
    seed, ns, ls = TRIPLES[0]
    h = plain(*tx[0], seed=seed, noise_scale=ns, length_scale=ls)
    assert torch.equal(h.mel(), refs[(0, 0)]["y"])
    with pytest.raises(RuntimeError, match="vocoder"):
        h.wav()


def test_vocoder_refusals(built):
    from glow_tts_amd import audio
    gen, tx, refs, synth, plain = setup()
    with pytest.raises(TypeError):
        gen.compile_synthesis(B, TX, 64, vocoder=audio.TacotronSTFT().to(dev()))
    with pytest.raises(TypeError):
        gen.compile_synthesis(B, TX, 64, vocoder=audio.GriffinLim(audio.STFT()).to(dev()))  # no mel basis
    with pytest.raises(ValueError, match="mel channels"):
        gen.compile_synthesis(B, TX, 64, vocoder=audio.GriffinLim(audio.TacotronSTFT(n_mel_channels=40)).to(dev()))
    with pytest.raises(ValueError, match="device"):
        gen.compile_synthesis(B, TX, 64, vocoder=audio.GriffinLim(audio.TacotronSTFT()))
    with pytest.raises(ValueError, match="vocoder_iters"):
        gen.compile_synthesis(B, TX, 64, vocoder=vocoder(), vocoder_iters=-1)


def test_overflow_falls_back_to_the_same_samples(built):
    from glow_tts_amd.synthesis import SynthesisOverflow
    gen, tx, refs, synth, plain = setup()
    ids, xl = tx[0]
    seed, ns, ls = TRIPLES[0]
    ref = refs[(0, 0)]
    lens = ref["lens"]
    keep = gen.rows_cfg.row_round
    try:
        small = gen.compile_synthesis(B, TX, (max(lens) - 2) // 2 * 2, max_rows=-(-rows_needed(lens) // 128) * 128, vocoder=vocoder(),
                                      vocoder_iters=ITERS)
        gen.rows_cfg.row_round = 128
        want = eager(gen, ids, xl, seed, ns, ls)
        want_wav, want_len = eager_wav(want["y"], want["lens"], seed)
        h = small(ids, xl, seed=seed, noise_scale=ns, length_scale=ls)
        assert h.status == 1 and h.lengths() == lens
        with pytest.raises(SynthesisOverflow):
            h.wav(fallback=False)
        wav, wav_len = h.wav()
        assert wav_len == want_len and wav.shape == want_wav.shape and torch.equal(wav, want_wav)
        assert torch.equal(h.mel(), want["y"]) and small.overflows == 1 and small.guards_intact()
    finally:
        gen.rows_cfg.row_round = keep


def test_utterances_of_two_frames(built):
    """a length scale that leaves one frame per token: utterances of 2 and 3 tokens have 2 frames (the squeeze drops the third).  The
    host cannot refuse what it has not read: the kernels' clamped reflection defines the samples — finite, the stated lengths, and
    nothing written outside the buffers."""
    gen, tx, refs, synth, plain = setup()
    g = torch.Generator().manual_seed(4)
    xl = torch.tensor([19, 2, 3])
    ids = torch.randint(1, 148, (B, TX), generator=g) * (torch.arange(TX)[None, :] < xl[:, None])
    h = synth(ids, xl, seed=3, noise_scale=0.5, length_scale=1e-3)
    assert h.status == 0 and h.lengths() == [19, 2, 3]
    wav, wav_len = h.wav()
    assert wav_len == [HOP * 17, HOP, HOP] and wav.shape == (B, HOP * 17)
    assert bool(torch.isfinite(wav).all()) and bool(torch.isfinite(synth.voc_bufs["spec"]).all())
    for b, n in enumerate(wav_len):
        assert not bool(wav[b, n:].any()), b
    assert float(wav[0].abs().max()) > 0 and synth.guards_intact()


def test_stochastic_synthesiser_with_a_vocoder(built):
    """one call of the full model (cfg 5 cut to 2 blocks / 2 layers, tests/test_synthesis_graph_cfg5_gpu.py)"""
    import test_synthesis_graph_cfg5_gpu as C5
    gen, _ = C5.build_cfg5()
    ids, xl, cond = C5.inputs()
    assert gen.set_synthesis_front(True, noise_key="frame") is True
    call = C5.CALLS[1]
    lens = C5.eager(gen, ids, xl, cond, **call)["lens"]
    assert min(lens) >= 4
    max_frames = (max(lens) // 2 + 1) * 2 + 8
    X = C5.round_up(C5.frame_rows_needed(lens), C5.ROUND)
    gen.rows_cfg.row_round = X
    ref = C5.eager(gen, ids, xl, cond, **call)
    want_wav, want_len = eager_wav(ref["y"], ref["lens"], call["seed"])
    synth = gen.compile_synthesis(C5.B, C5.TX, max_frames, max_rows=X, stochastic=True, max_frame_rows=X, vocoder=vocoder(),
                                  vocoder_iters=ITERS)
    h = synth(ids, xl, **cond, **call)
    assert h.status == 0 and h.lengths() == ref["lens"]
    wav, wav_len = h.wav()
    assert torch.equal(h.mel(), ref["y"])
    assert wav_len == want_len and wav.shape == want_wav.shape and torch.equal(wav, want_wav)
    assert synth.guards_intact()
