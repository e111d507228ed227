"""GPU tests of synthesis as one captured graph (FlowGenerator.compile_synthesis, glow-tts_amd/synthesis.py).

The replayed call against eager FlowGenerator.infer(seed=) on the same model: the eager call gets x padded to max_tokens (the encoder
sees the same shape) and the model's rows_cfg.row_round set to max_rows (its ragged context then has the same R and row0, so every
kernel picks the same row form).  The kernels are deterministic and see the same rows: the mel and every auxiliary output must be
BIT-IDENTICAL — a difference is a defect of the device-side geometry or of the scalar plumbing, not a tolerance question.  The one
tolerance here is the existing 3e-2 of max-abs of a mel against the float oracle's reverse decoder (tests/test_synthesis_front_gpu.py)."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "golden"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import synth_noise_host as H  # noqa: E402
from fill import fill_module  # noqa: E402
from oracle import glowtts_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
HALO = 2
B, TX = 3, 19
# (seed, noise_scale, length_scale): the small model predicts less than one frame per token, so the length scales stretch the
# utterances over more than one 64-frame tile of the prior kernel and more than one 128-row tile of the decoder
TRIPLES = ((5, 0.667, 40.0), (9, 0.3, 65.0))


def dev():
    return torch.device("cuda:0")


def relerr(a, b):
    return (a - b).abs().max().item() / max(1e-6, b.abs().max().item())


def texts():
    """two different batches of 3 texts, the second shorter than max_tokens (the synthesiser pads it)"""
    g = torch.Generator().manual_seed(21)
    out = []
    for Tx, xl in ((19, [19, 11, 7]), (15, [12, 15, 4])):
        xl = torch.tensor(xl)
        ids = torch.randint(1, 148, (B, Tx), generator=g) * (torch.arange(Tx)[None, :] < xl[:, None])
        out.append((ids, xl))
    return out


def padded(ids):
    out = torch.zeros(B, TX, dtype=ids.dtype)
    out[:, :ids.shape[1]] = ids
    return out


def build_generator(**extra):
    from glow_tts_amd import models
    gen = fill_module(models.FlowGenerator(148, 192, 768, 256, 80, use_sdp=False, kernel_size=3, n_heads=2, n_layers_enc=2, p_dropout=0.1,
                                           n_blocks_dec=2, kernel_size_dec=5, dilation_rate=1, n_block_layers=4, p_dropout_dec=0.05, n_sqz=2,
                                           window_size=4, mean_only=True, prenet=True, **extra), "").eval()
    P = {k: v.detach().cpu().float() for k, v in gen.state_dict().items()}
    gen = gen.to(dev())
    assert gen.store_inverse(fused_reverse=True, device_front=True) == (True, True)
    return gen, P


def eager(gen, ids, xl, seed, ns, ls, **cond):
    """infer(seed=) on x padded to max_tokens -> clones of what the replay is compared with"""
    (y, z_m, z_logs, _, z_mask), _, (attn, logw, logw_), _ = gen.infer(padded(ids).to(dev()), xl.to(dev()), noise_scale=ns, length_scale=ls,
                                                                         seed=seed, **{k: v.to(dev()) for k, v in cond.items()})
    torch.cuda.synchronize()
    return dict(y=y.clone(), z_m=z_m.clone(), z_logs=z_logs.clone(), attn=attn.clone(), logw=logw.clone(), logw_=logw_.clone(),
                lens=z_mask.squeeze(1).sum(1).long().tolist())


def rows_needed(lens):
    return sum(v // 2 + 2 * HALO for v in lens)


@functools.lru_cache(maxsize=None)
def setup():
    """the model, the eager references of every (text, triple) — computed ONCE, with the final row rounding — and the capacities that
    hold them: max_frames = the longest predicted utterance (even), max_rows = the rows of the largest batch, a multiple of 128"""
    gen, P = build_generator()
    tx = texts()
    probe = [eager(gen, ids, xl, *t)["lens"] for ids, xl in tx for t in TRIPLES]            # sizes from running the eager path once
    max_frames = (max(max(v) for v in probe) + 1) // 2 * 2
    max_rows = -(-max(rows_needed(v) for v in probe) // 128) * 128
    gen.rows_cfg.row_round = max_rows
    refs = {(i, j): eager(gen, ids, xl, *t) for i, (ids, xl) in enumerate(tx) for j, t in enumerate(TRIPLES)}
    print(f"predicted lengths {probe}: max_frames {max_frames}, max_rows {max_rows}")
    synth = gen.compile_synthesis(B, TX, max_frames, max_rows=max_rows, aux=True)
    return gen, P, tx, refs, synth


def check_call(h, ref, synth, aux=True):
    lens = h.lengths()
    assert h.status == 0
    assert lens == ref["lens"]
    y = h.mel()
    assert y.shape == ref["y"].shape and y.dtype == ref["y"].dtype
    assert torch.equal(y, ref["y"])                                                        # bit-identical
    for b in range(len(lens)):                                                             # frames past each utterance's length
        assert lens[b] >= y.shape[2] or y[b, :, lens[b]:].abs().max().item() == 0
    full = synth.mel_static
    assert y.shape[2] == max(lens) // 2 * 2                                                # the squeeze drops an odd trailing frame
    assert full[:, :, y.shape[2]:].numel() == 0 or full[:, :, y.shape[2]:].abs().max().item() == 0
    if aux:
        a = h.aux()
        for k in ("attn", "logw", "logw_", "z_m", "z_logs"):
            assert a[k].shape == ref[k].shape, k
            assert torch.equal(a[k], ref[k]), k


def test_replay_equals_eager(built):
    """two texts x two (seed, noise_scale, length_scale) triples through ONE captured graph: neither the seed, the scales nor the
    lengths are baked into it"""
    gen, P, tx, refs, synth = setup()
    graph = synth.graph
    lens_seen = set()
    for i, (ids, xl) in enumerate(tx):
        for j, (seed, ns, ls) in enumerate(TRIPLES):
            h = synth(ids, xl, seed=seed, noise_scale=ns, length_scale=ls)
            check_call(h, refs[(i, j)], synth)
            lens_seen.add(tuple(h.lengths()))
    assert synth.graph is graph and synth.overflows == 0
    assert len(lens_seen) == 4                                                             # four different geometries
    assert not torch.equal(refs[(0, 0)]["y"][:, :, :8], refs[(0, 1)]["y"][:, :, :8])
    assert synth.max_rows % 128 == 0 and synth.max_rows > 128 and synth.guards_intact()
    assert any(v & 1 for t in lens_seen for v in t)                                           # an odd length among them


def test_replay_against_the_oracle(built):
    gen, P, tx, refs, synth = setup()
    ids, xl = tx[0]
    ns, seed = 0.667, 1234
    h = synth(ids, xl, seed=seed, noise_scale=ns, length_scale=40.0)
    lens = h.lengths()
    assert max(lens) > 64
    y, a = h.mel(clone=True), h.aux()
    z_m, z_logs = a["z_m"].cpu(), a["z_logs"].cpu()
    C, Ty = z_m.shape[1], z_m.shape[2]
    z_mask = (torch.arange(Ty)[None, :] < torch.tensor(lens)[:, None]).unsqueeze(1).float()
    noise = np.stack([H.prior_noise(seed, b, C, Ty) for b in range(B)])
    z64 = (z_m.numpy().astype(np.float64) + np.exp(z_logs.numpy().astype(np.float64)) * noise * float(np.float32(ns))) * z_mask.numpy()
    y_want = R.decoder_rev(P, "decoder.", torch.from_numpy(z64).float(), z_mask, n_blocks=2)
    e = relerr(y.cpu(), y_want)
    print(f"replayed mel vs the float oracle: {e:.3e} of max-abs")
    assert y.shape == y_want.shape and torch.isfinite(y).all()
    assert e < 3e-2, e


def test_a_seed_reproduces_the_replay(built):
    gen, P, tx, refs, synth = setup()
    ids, xl = tx[0]
    call = lambda **kw: synth(ids, xl, noise_scale=0.667, length_scale=40.0, **kw).mel(clone=True)     # noqa: E731
    y1, y2, y3 = call(seed=77), call(seed=77), call(seed=78)
    assert torch.equal(y1, y2) and y1.shape == y3.shape and not torch.equal(y1, y3)
    torch.manual_seed(3)
    y4 = call()
    torch.manual_seed(3)
    y5 = call()
    torch.manual_seed(4)
    y6 = call()
    assert torch.equal(y4, y5) and not torch.equal(y4, y6)                                 # seed=None: torch.manual_seed governs the call
    torch.manual_seed(3)
    want = gen.infer(padded(ids).to(dev()), xl.to(dev()), noise_scale=0.667, length_scale=40.0)[0][0]   # ... and draws what infer draws
    assert torch.equal(y4, want)


def test_queued_calls(built):
    """four calls with different inputs issued before any synchronisation (the staging ring, and the outputs of a call that has not
    been read moved aside before the next replay overwrites them), then read in order"""
    gen, P, tx, refs, synth = setup()
    torch.cuda.synchronize()
    hs = []
    for i, (ids, xl) in enumerate(tx):
        for j, (seed, ns, ls) in enumerate(TRIPLES):
            hs.append(((i, j), synth(ids, xl, seed=seed, noise_scale=ns, length_scale=ls)))
    for key, h in hs:
        y = h.mel(clone=True)
        assert h.lengths() == refs[key]["lens"]
        assert y.shape == refs[key]["y"].shape and torch.equal(y, refs[key]["y"]), key
        a = h.aux()
        assert torch.equal(a["attn"], refs[key]["attn"]) and torch.equal(a["z_m"], refs[key]["z_m"]), key
    assert synth.guards_intact()


def test_more_calls_in_flight_than_the_ring_holds(built):
    """11 calls (the staging ring has 8 slots) issued before any is read, one of them an overflow, then read in order: a slot that is
    taken again first hands its call's lengths and status to that call's handle, so every handle returns ITS call's."""
    gen, P, tx, refs, synth = setup()
    assert synth.RING == 8
    torch.cuda.synchronize()
    count = synth.overflows
    keys = [(i % 2, (i // 2) % 2) for i in range(11)]
    hs = []
    for n, (i, j) in enumerate(keys):
        seed, ns, ls = TRIPLES[j]
        hs.append(synth(*tx[i], seed=seed, noise_scale=ns, length_scale=ls * (4.0 if n == 1 else 1.0)))      # call 1 does not fit
    assert hs[0]._read is not None and hs[2]._read is not None and hs[3]._read is None        # slots 0-2 were taken again
    for n, (key, h) in enumerate(zip(keys, hs)):
        if n == 1:
            assert h.status != 0 and max(h.lengths()) > synth.max_frames
            continue
        assert h.status == 0 and h.lengths() == refs[key]["lens"], n
        y = h.mel(clone=True)
        assert y.shape == refs[key]["y"].shape and torch.equal(y, refs[key]["y"]), n
    assert synth.overflows == count + 1 and synth.guards_intact()
    dropped = synth(*tx[0], seed=1, length_scale=TRIPLES[0][2] * 4.0)                         # an overflow whose handle is dropped
    del dropped
    for _ in range(synth.RING):
        synth(*tx[0], seed=1).mel()
    assert synth.overflows == count + 2                                                        # ... is counted when its slot is taken again


def test_the_next_replay_waits_for_the_readers_of_a_view(built):
    """mel() hands out a view of the static buffer; a consumer stream with a backlog (a device-side spin of a few ms stands for the
    vocoder of the previous utterance) copies it, then the next call is issued: its replay must not overwrite the view before that
    copy has run.  The same for mel(clone=True), which must not depend on the caller's stream at all."""
    gen, P, tx, refs, synth = setup()
    (s0, ns0, ls0), (s1, ns1, ls1) = TRIPLES
    consumer = torch.cuda.Stream()
    for clone in (False, True):
        h = synth(*tx[0], seed=s0, noise_scale=ns0, length_scale=ls0)
        h.lengths()
        with torch.cuda.stream(consumer):
            torch.cuda._sleep(2_000_000)                                                       # 1-20 ms by the counter's rate: several replays long
            got = h.mel(clone=clone)
            got = got if clone else got.clone()
        h2 = synth(*tx[1], seed=s1, noise_scale=ns1, length_scale=ls1)                         # overwrites the static buffers
        y2 = h2.mel(clone=True)
        torch.cuda.synchronize()
        assert torch.equal(got, refs[(0, 0)]["y"]), clone
        assert torch.equal(y2, refs[(1, 1)]["y"]), clone


def test_max_rows_granularity(built):
    gen, P, tx, refs, synth = setup()
    with pytest.raises(ValueError, match="multiple of 8"):
        gen.compile_synthesis(B, TX, 64, max_rows=260)


def test_speaker_and_language_vectors(built):
    """cfg 4's speaker vector g and the language id l: static inputs of the graph like the text"""
    gen, P = build_generator(gin_channels=256, lin_channels=4, n_lang=10)
    ids, xl = texts()[0]
    g = torch.Generator().manual_seed(8)
    conds = [dict(g=torch.randn(B, 256, generator=g), l=torch.randint(0, 10, (B,), generator=g)) for _ in range(2)]
    seed, ns, ls = TRIPLES[0]
    probe = [eager(gen, ids, xl, seed, ns, ls, **c)["lens"] for c in conds]
    max_frames = (max(max(v) for v in probe) + 1) // 2 * 2
    max_rows = -(-max(rows_needed(v) for v in probe) // 128) * 128
    gen.rows_cfg.row_round = max_rows
    synth = gen.compile_synthesis(B, TX, max_frames, max_rows=max_rows, aux=True)
    ys = []
    for c in conds:
        ref = eager(gen, ids, xl, seed, ns, ls, **c)
        h = synth(ids, xl, seed=seed, noise_scale=ns, length_scale=ls, **c)
        check_call(h, ref, synth)
        ys.append(ref["y"])
    assert ys[0].shape != ys[1].shape or not torch.equal(ys[0], ys[1])                      # the two speakers differ
    with pytest.raises(ValueError):
        synth(ids, xl, seed=seed)                                                          # g / l missing: nothing is launched


@pytest.mark.parametrize("which", ["frames", "rows"])
def test_overflow_is_a_handled_outcome(built, which):
    from glow_tts_amd.synthesis import SynthesisOverflow
    gen, P, tx, refs, _ = setup()
    ids, xl = tx[0]
    seed, ns, ls = TRIPLES[0]
    lens = refs[(0, 0)]["lens"]
    keep = gen.rows_cfg.row_round
    try:
        if which == "frames":                              # max_frames below the longest predicted utterance: bit 0
            max_frames, max_rows, bit = (max(lens) - 2) // 2 * 2, -(-rows_needed(lens) // 128) * 128, 1
        else:                                              # max_rows below the rows the batch needs: bit 1
            max_frames, max_rows, bit = (max(lens) + 1) // 2 * 2, (rows_needed(lens) - 1) // 8 * 8, 2
        synth = gen.compile_synthesis(B, TX, max_frames, max_rows=max_rows)
        gen.rows_cfg.row_round = 128
        want = eager(gen, ids, xl, seed, ns, ls)
        h = synth(ids, xl, seed=seed, noise_scale=ns, length_scale=ls)
        assert h.status == bit and h.lengths() == lens                                     # the unclipped predicted lengths
        assert synth.overflows == 1
        with pytest.raises(SynthesisOverflow) as e:
            h.mel(fallback=False)
        assert e.value.lengths == lens and e.value.status == bit
        y = h.mel()                                                                        # the default handle: the eager mel
        assert y.shape == want["y"].shape and torch.equal(y, want["y"])
        assert synth.overflows == 1 and synth.guards_intact()
        # a following call that fits (a quarter of the length) is correct again
        gen.rows_cfg.row_round = max_rows
        fit = eager(gen, ids, xl, seed, ns, 1.0)
        assert max(fit["lens"]) <= max_frames and rows_needed(fit["lens"]) <= max_rows
        h2 = synth(ids, xl, seed=seed, noise_scale=ns, length_scale=1.0)
        check_call(h2, fit, synth, aux=False)
        assert synth.overflows == 1 and synth.guards_intact()
        # the fallback on a consumer stream with a backlog, from a device-resident text shorter than max_tokens: the padded text is
        # built on the stream the eager call runs on, behind what the caller's stream has queued (the encoder must not read it earlier)
        ids1, xl1 = tx[1]
        gen.rows_cfg.row_round = 128
        want1 = eager(gen, ids1, xl1, seed, ns, 4 * ls)
        consumer = torch.cuda.Stream()
        with torch.cuda.stream(consumer):
            x_dev = ids1.to(dev()) + 0
            h3 = synth(x_dev, xl1, seed=seed, noise_scale=ns, length_scale=4 * ls)
            assert h3.status != 0
            torch.cuda._sleep(2_000_000)
            y3 = h3.mel()
        torch.cuda.synchronize()
        assert y3.shape == want1["y"].shape and torch.equal(y3, want1["y"])
        assert synth.overflows == 2 and synth.guards_intact()
    finally:
        gen.rows_cfg.row_round = keep


def test_refusals(built):
    from glow_tts_amd import models
    from test_synthesis_fused_gpu import CFG5
    gen, P, tx, refs, synth = setup()
    ids, xl = tx[0]
    before = synth._ring_i
    with pytest.raises(ValueError, match="max_tokens"):
        synth(torch.ones(B, TX + 1, dtype=torch.long), xl)                                 # oversize x: before any launch
    with pytest.raises(ValueError, match="batch"):
        synth(ids[:2], xl[:2])
    assert synth._ring_i == before
    plain, _ = build_generator()
    plain.store_inverse(fused_reverse=True, device_front=False)
    with pytest.raises(RuntimeError, match="store_inverse"):
        plain.compile_synthesis(B, TX, 64)
    plain.store_inverse(fused_reverse=False, device_front=True)
    with pytest.raises(RuntimeError, match="store_inverse"):
        plain.compile_synthesis(B, TX, 64)
    cfg5 = fill_module(models.FlowGenerator(n_vocab=187, out_channels=80, n_lang=10, **dict(CFG5, n_blocks_dec=2, n_layers_enc=2)), "").eval().to(dev())
    cfg5.store_inverse(fused_reverse=True, device_front=True)
    with pytest.raises(NotImplementedError):
        cfg5.compile_synthesis(2, 15, 64)
