"""GPU tests of full-model synthesis as one captured graph (FlowGenerator.compile_synthesis(stochastic=True),
glow-tts_amd/synthesis.py): cfg 5 — emotion front end, stochastic duration predictor in reverse, stochastic pitch /
energy predictors at the frame rate — cut to 2 decoder blocks / 2 encoder layers.

The replayed call against eager FlowGenerator.infer(seed=) under set_synthesis_front(noise_key="frame"): the capacities are chosen so
that the eager call's two ragged contexts (squeezed axis, frame rate) have the row counts of the graph's (see setup),
the noise is keyed by (utterance, token / frame), the kernels are deterministic and see the same rows: lengths, mel, pitch, energy and
every auxiliary output must be BIT-IDENTICAL.  Tolerances exist only against the float oracle: 3e-2 relative on the valid positions
for the predictors' reverse passes (tests/test_predictors_gpu.py::test_stochastic_predictors_reverse) and 3e-2 of max-abs for the mel
against the oracle's reverse decoder (tests/test_synthesis_front_gpu.py::test_infer_with_noise_against_the_oracle)."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "golden"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import synth_noise_host as H  # noqa: E402
import synth_prosody_host as PH  # noqa: E402
from fill import fill_module  # noqa: E402
from oracle import glowtts_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
HALO = 2
B, TX = 2, 15
ROUND = 128
# every scale of the call differs from its default: nothing may be baked into the graph
CALLS = (dict(seed=7, noise_scale=0.5, noise_scale_w=0.4, f0_noise_scale=0.6, energy_noise_scale=0.7, length_scale=1.0, pitch_scale=1.25,
              energy_scale=0.75),
         dict(seed=8, noise_scale=0.667, noise_scale_w=0.8, f0_noise_scale=0.3, energy_noise_scale=0.9, length_scale=1.3, pitch_scale=0.9,
              energy_scale=1.1))


def dev():
    return torch.device("cuda:0")


def relerr(a, b):
    return (a - b).abs().max().item() / max(1e-6, b.abs().max().item())


def inputs():
    """as tests/test_synthesis_front_gpu.py::test_cfg5_infer_with_the_front_on"""
    g = torch.Generator().manual_seed(2)
    xl = torch.tensor([15, 9])
    ids = torch.randint(1, 187, (B, TX), generator=g) * (torch.arange(TX)[None, :] < xl[:, None])
    graw, emo = torch.randn(B, 512, generator=g), torch.randint(0, 5, (B,), generator=g)
    cart = torch.rand(B, 3, generator=g) * torch.tensor([1.5, 3.1, 4.6]) + torch.tensor([0.0, 0.0, -1.55])
    lid = torch.randint(0, 3, (B,), generator=g)
    return ids, xl, dict(g=graw, emo=emo, emo_cartesian=cart, l=lid)


def build_cfg5():
    from glow_tts_amd import models
    from test_synthesis_fused_gpu import CFG5
    gen = fill_module(models.FlowGenerator(n_vocab=187, out_channels=80, n_lang=10, **dict(CFG5, n_blocks_dec=2, n_layers_enc=2)), "").eval()
    P = {k: v.detach().cpu().float() for k, v in gen.state_dict().items()}
    gen = gen.to(dev())
    assert gen.store_inverse(fused_reverse=True, device_front=True) == (True, True)
    assert gen.noise_key == "row"                                                  # what store_inverse(device_front=True) sets
    return gen, P


def eager(gen, ids, xl, cond, **call):
    """infer(seed=) -> clones of what the replay is compared with"""
    (y, z_m, z_logs, _, z_mask), _, (attn, logw, logw_), (pitch, energy) = \
        gen.infer(ids.to(dev()), xl.to(dev()), **{k: v.to(dev()) for k, v in cond.items()}, **call)
    torch.cuda.synchronize()
    return dict(y=y.clone(), z_m=z_m.clone(), z_logs=z_logs.clone(), attn=attn.clone(), logw=logw.clone(), logw_=logw_.clone(),
                pitch=pitch.clone(), energy=energy.clone(), lens=z_mask.squeeze(1).sum(1).long().tolist())


def rows_needed(lens):
    return sum(v // 2 + 2 * HALO for v in lens)


def frame_rows_needed(lens):
    return sum(v + 2 * HALO for v in lens)


def round_up(n, m):
    return -(-n // m) * m


@functools.lru_cache(maxsize=None)
def setup():
    """the model, the capacities, and the eager references — computed ONCE.  The eager path is run first to learn the lengths:
    max_frames = the next even number above the longest predicted utterance plus a margin; ONE row count X (a multiple of 128 that
    holds the frame rows of the largest batch) serves as rows_cfg.row_round, max_rows and max_frame_rows, so the eager call's two
    ragged contexts and the graph's two capacity contexts all have X rows, whatever the lengths of a call.  Then one eager call under
    the row keying (the parent's behaviour) and the references of both calls under the frame keying."""
    gen, P = build_cfg5()
    ids, xl, cond = inputs()
    assert gen.set_synthesis_front(True, noise_key="frame") is True and gen.noise_key == "frame"
    probe = [eager(gen, ids, xl, cond, **c)["lens"] for c in CALLS]
    max_frames = (max(max(v) for v in probe) // 2 + 1) * 2 + 8
    X = round_up(max(frame_rows_needed(v) for v in probe), ROUND)
    assert X >= max(rows_needed(v) for v in probe)
    gen.rows_cfg.row_round = X
    gen.set_synthesis_front(True, noise_key="row")
    row_keyed = eager(gen, ids, xl, cond, **CALLS[0])
    gen.set_synthesis_front(True, noise_key="frame")
    refs = [eager(gen, ids, xl, cond, **c) for c in CALLS]
    assert [r["lens"] for r in refs] == probe                                      # a draw does not depend on the rounding
    print(f"predicted lengths {probe}: max_frames {max_frames}, max_rows = max_frame_rows = {X}")
    synth = gen.compile_synthesis(B, TX, max_frames, max_rows=X, aux=True, stochastic=True, max_frame_rows=X)
    return gen, P, (ids, xl, cond), refs, synth, row_keyed


def check_call(h, ref, synth):
    lens = h.lengths()
    assert h.status == 0                                                           # a fallback must not hide a broken replay
    assert lens == ref["lens"]
    y = h.mel()
    assert y.shape == ref["y"].shape and y.dtype == ref["y"].dtype
    assert torch.equal(y, ref["y"])                                                # bit-identical
    pitch, energy = h.prosody()
    for got, k in ((pitch, "pitch"), (energy, "energy")):
        assert got.shape == ref[k].shape and got.dtype == ref[k].dtype, k
        assert torch.equal(got, ref[k]), k
        for b in range(len(lens)):
            assert lens[b] >= got.shape[1] or got[b, lens[b]:].abs().max().item() == 0
    a = h.aux()
    for k in ("logw", "attn", "z_m", "z_logs", "logw_"):
        assert a[k].shape == ref[k].shape, k
        assert torch.equal(a[k], ref[k]), k


def test_replay_equals_eager(built):
    """two calls that differ in the seed and in all seven scalars through ONE captured graph"""
    gen, P, (ids, xl, cond), refs, synth, _ = setup()
    graph = synth.graph
    for call, ref in zip(CALLS, refs):
        check_call(synth(ids, xl, **cond, **call), ref, synth)
    assert synth.graph is graph and synth.overflows == 0 and synth.guards_intact()
    assert refs[0]["pitch"].abs().max().item() > 0 and refs[0]["energy"].abs().max().item() > 0
    assert not torch.equal(refs[0]["pitch"][:, :4], refs[1]["pitch"][:, :4])       # the two calls differ
    print(f"C-ABI entries inside the cfg 5 graph: {synth.captured_entries}; lengths {refs[0]['lens']} and {refs[1]['lens']}")


def test_seed_and_scales(built):
    gen, P, (ids, xl, cond), refs, synth, _ = setup()
    base = dict(CALLS[0])

    def run(**kw):
        h = synth(ids, xl, **cond, **dict(base, **kw))
        assert h.status == 0
        p, e = h.prosody()
        return h.lengths(), h.mel(clone=True), p.clone(), e.clone()

    l1, y1, p1, e1 = run()
    l2, y2, p2, e2 = run()
    assert l1 == l2 and torch.equal(y1, y2) and torch.equal(p1, p2) and torch.equal(e1, e2)      # the seed reproduces the replay
    l3, y3, p3, e3 = run(seed=base["seed"] + 1)
    assert l3 != l1 or not torch.equal(p3, p1)                                     # another seed: other durations or another pitch
    # pitch_scale is read at replay: with 1.0 and 2.0 the pitch differs by exactly that factor, nothing else of the front moves
    l4, y4, p4, e4 = run(pitch_scale=1.0)
    l5, y5, p5, e5 = run(pitch_scale=2.0)
    assert l4 == l5 == l1 and torch.equal(e4, e5) and torch.equal(e4, e1)
    assert torch.equal(p5, p4 * 2.0) and p4.abs().max().item() > 0
    assert y4.shape == y5.shape and not torch.equal(y4, y5)                        # ... and the decoder saw it
    assert synth.overflows == 0 and synth.guards_intact()


def test_against_the_oracle(built):
    """logw, pitch and energy against the oracle's stochastic predictors in reverse, with the noise restated on the host under the
    (utterance, token / frame) keying; the mel against the oracle's reverse decoder on the device's own latent rows and contours"""
    import torch.nn.functional as F
    gen, P, (ids, xl, cond), refs, synth, _ = setup()
    call = CALLS[0]
    seed = call["seed"]
    # the text-side features the predictors read: the encoder's bf16 rows of the eager call (the replay's are bit-identical)
    eager(gen, ids, xl, cond, **call)
    rcx, xb = gen.encoder._last_rows
    x_feat = rcx.from_rows(xb).float().cpu()                                       # [B, 192, Tx]
    h = synth(ids, xl, **cond, **call)
    assert h.status == 0
    lens = h.lengths()
    y, a = h.mel(clone=True).cpu(), {k: v.clone().cpu() for k, v in h.aux().items()}
    pitch, energy = (t.clone().cpu() for t in h.prosody())
    Ty = max(lens)
    x_mask = (torch.arange(TX)[None, :] < xl[:, None]).unsqueeze(1).float()
    y_mask = (torch.arange(Ty)[None, :] < torch.tensor(lens)[:, None]).unsqueeze(1).float()
    g_o = R.emotion_speaker_vector(P, cond["g"], cond["emo"], cond["emo_cartesian"])
    l_o = F.embedding(cond["l"], P["emb_l.weight"]).unsqueeze(-1)
    f32 = lambda v: float(np.float32(v))                                          # noqa: E731
    nz = torch.from_numpy(PH.keyed_bct(xl.tolist(), TX, seed, H.DURATION, f32(call["noise_scale_w"]))).float()
    logw_o = R.predictor_reverse(P, "encoder.proj_w.", x_feat, x_mask, nz, g=g_o, l=l_o)
    m = x_mask.bool()
    e_w = relerr(a["logw"][m], logw_o[m])
    x_frames = torch.matmul(x_feat, a["attn"].squeeze(1))                          # models.py:1094 on the device's own path
    errs = {}
    for name, got, stream, ns, sc in (("pitch", pitch, H.PITCH, call["f0_noise_scale"], call["pitch_scale"]),
                                      ("energy", energy, H.ENERGY, call["energy_noise_scale"], call["energy_scale"])):
        nz = torch.from_numpy(PH.keyed_bct(lens, Ty, seed, stream, f32(ns))).float()
        want = R.predictor_reverse(P, f"proj_{name}.", x_frames, y_mask, nz, g=g_o).squeeze(1) * sc
        fm = y_mask.squeeze(1).bool()
        errs[name] = relerr(got[fm], want[fm])
    # the mel: the device's latent rows unsqueezed, the device's contours, the oracle's reverse decoder
    C, T2 = y.shape[1], Ty // 2
    rows, row0 = synth.rows.cpu(), synth.rc.row0.cpu().tolist()
    z = torch.zeros(B, C, 2 * T2)
    for b in range(B):
        n = lens[b] // 2
        blk = rows[row0[b] + HALO:row0[b] + HALO + n].view(n, 2, C)                # [s, parity, c]
        z[b, :, :2 * n] = blk.permute(2, 0, 1).reshape(C, 2 * n)
    zm = (torch.arange(2 * T2)[None, :] < (torch.tensor(lens) // 2 * 2)[:, None]).unsqueeze(1).float()
    y_want = R.decoder_rev(P, "decoder.", z, zm, g_o, n_blocks=2, pitch=(pitch[:, None, :2 * T2] * zm), energy=(energy[:, None, :2 * T2] * zm))
    e_y = relerr(y, y_want)
    print(f"replay vs the float oracle: logw {e_w:.3e}, pitch {errs['pitch']:.3e}, energy {errs['energy']:.3e} (relative, valid positions); "
          f"mel {e_y:.3e} of max-abs")
    assert e_w < 3e-2, e_w
    assert errs["pitch"] < 3e-2 and errs["energy"] < 3e-2, errs
    assert y.shape == y_want.shape and torch.isfinite(y).all()
    assert e_y < 3e-2, e_y


def test_frame_rows_overflow_is_a_handled_outcome(built):
    from glow_tts_amd.synthesis import SynthesisOverflow
    gen, P, (ids, xl, cond), refs, full, _ = setup()
    call, ref = CALLS[0], refs[0]
    lens = ref["lens"]
    # frame rows one short of what the batch needs (bit 2); the squeezed rows and the frames fit
    short = (frame_rows_needed(lens) - 1) // 8 * 8
    synth = gen.compile_synthesis(B, TX, full.max_frames, max_rows=full.max_rows, stochastic=True, max_frame_rows=short)
    assert synth.max_frame_rows == short < frame_rows_needed(lens)
    h = synth(ids, xl, **cond, **call)
    assert h.status == 4 and h.lengths() == lens                                   # the unclipped predicted lengths
    assert synth.overflows == 1
    with pytest.raises(SynthesisOverflow) as e:
        h.mel(fallback=False)
    assert e.value.status == 4 and e.value.lengths == lens
    y = h.mel()                                                                    # the default: eager infer of the same call and seed
    assert y.shape == ref["y"].shape and torch.equal(y, ref["y"])
    p, en = h.prosody()
    assert torch.equal(p, ref["pitch"]) and torch.equal(en, ref["energy"])
    assert synth.overflows == 1 and synth.guards_intact()


def test_refusals(built):
    gen, P, (ids, xl, cond), refs, synth, _ = setup()
    before = synth._ring_i
    for drop in ("emo", "emo_cartesian"):
        with pytest.raises(ValueError, match="emo"):
            synth(ids, xl, **{k: v for k, v in cond.items() if k != drop}, **CALLS[0])
    with pytest.raises(ValueError, match="emo"):
        synth(ids, xl, **dict(cond, emo=cond["emo"][:1]), **CALLS[0])
    assert synth._ring_i == before                                                 # nothing was staged, nothing launched
    with pytest.raises(ValueError, match="multiple of 8"):
        gen.compile_synthesis(B, TX, 64, stochastic=True, max_frame_rows=260)
    with pytest.raises(NotImplementedError, match="stochastic=True"):
        gen.compile_synthesis(B, TX, 64)                                           # the default still refuses cfg 5, and names the keyword
    other, _ = build_cfg5()                                                        # the row keying cannot be reproduced at capacity sizes
    with pytest.raises(RuntimeError, match="noise_key"):
        other.compile_synthesis(B, TX, 64, stochastic=True)
    with pytest.raises(ValueError, match="noise_key"):
        other.set_synthesis_front(True, noise_key="token")


def test_a_plain_model_under_stochastic_equals_its_plain_synthesiser(built):
    """cfg 2 (deterministic duration predictor, no conditioning): stochastic=True is the same graph with the longer call block"""
    from test_synthesis_graph_gpu import build_generator, texts
    gen, _ = build_generator()
    ids, xl = texts()[0]
    kw = dict(seed=5, noise_scale=0.667, length_scale=40.0)
    want = gen.infer(ids.to(dev()), xl.to(dev()), **kw)
    longest = int(want[0][4].sum(-1).max().item())
    max_frames = (longest // 2 + 1) * 2 + 8                                        # capacities from the eager call: a fit
    plain = gen.compile_synthesis(3, 19, max_frames)
    with pytest.raises(ValueError, match="stochastic=True"):
        plain(ids, xl, seed=5, pitch_scale=2.0)                                    # a scalar the plain call block does not hold
    gen.set_synthesis_front(True, noise_key="frame")
    full = gen.compile_synthesis(3, 19, max_frames, stochastic=True)
    assert full.rcf is None and full.max_frame_rows is None
    h1 = plain(ids, xl, **kw)
    y1, l1 = h1.mel(clone=True), h1.lengths()
    h2 = full(ids, xl, **kw)
    assert h1.status == 0 and h2.status == 0 and h2.lengths() == l1
    assert torch.equal(h2.mel(), y1) and h2.prosody() == (None, None)
    assert plain.overflows == 0 and full.overflows == 0


def test_the_eager_switch_goes_back(built):
    """noise_key="row" after "frame": the parent's behaviour, bit for bit; the two keyings draw different noise"""
    gen, P, (ids, xl, cond), refs, synth, before = setup()
    try:
        assert gen.set_synthesis_front(True, noise_key="row") is True and gen.noise_key == "row"
        again = eager(gen, ids, xl, cond, **CALLS[0])
        assert gen._front_last["rc_frames"].ragged is False                        # uniform frame rows, as before
    finally:
        gen.set_synthesis_front(True, noise_key="frame")
    for k in ("y", "logw", "attn", "pitch", "energy", "z_m"):
        assert again[k].shape == before[k].shape and torch.equal(again[k], before[k]), k
    assert again["lens"] == before["lens"]
    frame = refs[0]
    assert frame["lens"] != before["lens"] or not torch.equal(frame["pitch"], before["pitch"])
    eager(gen, ids, xl, cond, **CALLS[0])
    assert gen._front_last["rc_frames"].ragged is True and gen._front_last["rc_frames"].R == synth.max_frame_rows
