"""GPU tests of the device pitch front end (csrc/yin_front.hip, glow_tts_amd.audio.YIN).

The ragged batch: six utterances cut from the signals of tests/golden/yin_golden.npz at 1024, 1025, 4864 (= 19 * 256), 4865, 5276 and
9435 samples = 0, 1, 15, 16, 17 and 33 analysis frames: none, one, and one less than, exactly, one more than and two tiles plus one of
the kernel's 16-frame tile (gt_yin_tile_frames), one length a multiple of 256 and one a multiple plus 1.  Output rows have
1 + 9435 // 256 = 37 positions, frames from position lead = 2.

The float64 reference is tests/yin64.py (the direct sum).  A frame is compared unless a comparison the float64 walk consulted is within
eps_c = (2 * 1024 + 441 + 8) 2^-24 = 1.5e-4 relative (derived there from the fp32 format; tests/test_yin64.py checks that an fp32
evaluation in the kernel's order stays within it): on every other frame the lag is exact, f0 within 1 ulp of fl32(sr / tau) (one
correctly rounded division), harm within eps_c relative and argmin_f0 exact, and at most 2 % of the frames may be set aside."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import yin64 as Y  # noqa: E402

gpu = pytest.mark.gpu
P = Y.GET_F0
SR, HOP, WLEN, LEAD = P["sr"], P["hop"], P["w_len"], 2
TAU_MIN, TAU_MAX = Y.taus(P["sr"], P["f0_min"], P["f0_max"])
EPS = Y.eps_c(WLEN, TAU_MAX)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "yin_golden.npz")
CUTS = (("noise", 1024), ("vibrato", 1025), ("gated", 4864), ("vibrato", 4865), ("silence", 5276), ("glide", 9435))


def dev():
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def golden():
    g = np.load(GOLDEN)
    return {k: g[k] for k in g.files}


@functools.lru_cache(maxsize=None)
def module():
    from glow_tts_amd import audio
    return audio.YIN().to(dev())


def pad_rows(waves, fill=0):
    width = (max(len(x) for x in waves) + 3) // 4 * 4
    out = np.full((len(waves), width), fill, dtype=waves[0].dtype)
    for i, x in enumerate(waves):
        out[i, :len(x)] = x
    return out


@functools.lru_cache(maxsize=None)
def batch():
    """(int16 utterances, lengths, int16 rows on the device, int32 lengths on the device, F_max)"""
    waves = [golden()[f"{name}_wav"][:L] for name, L in CUTS]
    lengths = [len(x) for x in waves]
    return (waves, lengths, torch.from_numpy(pad_rows(waves)).to(dev()), torch.tensor(lengths, dtype=torch.int32, device=dev()),
            1 + max(lengths) // HOP)


@functools.lru_cache(maxsize=None)
def reference():
    """per utterance the float64 restatement on x / 32768, computed once"""
    return [Y.yin64(x.astype(np.float64) / 32768.0, SR, WLEN, HOP, P["f0_min"], P["f0_max"], P["thresh"]) for x in batch()[0]]


@functools.lru_cache(maxsize=None)
def batch_outputs():
    _, _, y, ln, F_max = batch()
    out = module().transform(y, ln, F_max, aux=True)
    torch.cuda.synchronize()
    return out


def compare(f0, harm, amin, ref, label):
    """one utterance's frames (numpy rows of n entries) against decide()'s dict -> number of frames set aside"""
    n = len(ref["tau"])
    assert f0.shape == (n,) and np.isfinite(f0).all() and np.isfinite(harm).all() and np.isfinite(amin).all(), label
    keep_t, keep_a = ~ref["amb_tau"], ~ref["amb_argmin"]
    got_tau = np.where(f0 > 0, np.round(SR / np.where(f0 > 0, f0, 1.0).astype(np.float64)), 0).astype(np.int64)
    assert (got_tau[keep_t] == ref["tau"][keep_t]).all(), (label, got_tau, ref["tau"])
    want = Y.contour(ref["tau"], SR).astype(np.float32)
    assert (np.abs(f0 - want)[keep_t] <= np.spacing(want)[keep_t]).all(), label
    rel = np.abs(harm.astype(np.float64) - ref["harm"]) / np.abs(ref["harm"])
    assert (rel[keep_t] <= EPS).all(), (label, float(rel[keep_t].max()))
    want_a = Y.argmin_contour(ref["argmin"], TAU_MIN, SR).astype(np.float32)
    assert (amin[keep_a] == want_a[keep_a]).all(), label
    return int((~keep_t | ~keep_a).sum()), float(rel[keep_t].max()) if keep_t.any() else 0.0


@gpu
def test_batch_against_float64(built):
    from glow_tts_amd import _lib
    t = _lib.lib().gt_yin_tile_frames()
    _, lengths, _, _, F_max = batch()
    assert [Y.n_frames(L, WLEN, HOP) for L in lengths] == [0, 1, t - 1, t, t + 1, 2 * t + 1] and F_max == 37
    assert lengths[2] % 256 == 0 and lengths[3] % 256 == 1
    f0, harm, amin = (v.cpu().numpy() for v in batch_outputs())
    aside = total = 0
    for i, (ref, (name, L)) in enumerate(zip(reference(), CUTS)):
        n = len(ref["tau"])
        a, worst = compare(f0[i, LEAD:LEAD + n], harm[i, LEAD:LEAD + n], amin[i, LEAD:LEAD + n], ref, (name, L))
        print(f"{name}[:{L}]: {n} frames, {a} set aside, voiced {int((ref['tau'] > 0).sum())}, worst harm error {worst:.2e} (eps_c {EPS:.2e})")
        aside += a
        total += n
    assert total == 82 and aside <= 0.02 * total, (aside, total)


@gpu
def test_golden_signals_against_the_reference(built):
    """the recorded outputs of the reference's compute_yin itself, int16 in"""
    g = golden()
    names = [str(s) for s in g["signals"]]
    waves = [g[f"{n}_wav"] for n in names]
    y = torch.from_numpy(pad_rows(waves)).to(dev())
    ln = torch.tensor([len(x) for x in waves], dtype=torch.int32, device=dev())
    F_max = 1 + max(len(x) for x in waves) // HOP
    f0, harm, amin = (v.cpu().numpy() for v in module().transform(y, ln, F_max, aux=True))
    aside = total = 0
    for i, name in enumerate(names):
        pit, hr, am = (g[f"{name}_{k}_f0"] for k in ("pitches", "harmonic_rates", "argmins"))
        assert not (np.isnan(pit) | np.isnan(hr) | np.isnan(am)).any()
        amb = Y.yin64(waves[i].astype(np.float64) / 32768.0, SR, WLEN, HOP, P["f0_min"], P["f0_max"], P["thresh"])
        ref = dict(tau=np.where(pit > 0, np.round(SR / np.where(pit > 0, pit, 1.0)), 0).astype(np.int64), harm=hr,
                   argmin=np.where(am > 0, np.round(SR / np.where(am > 0, am, 1.0)), 0).astype(np.int64),
                   amb_tau=amb["amb_tau"], amb_argmin=amb["amb_argmin"])
        n = len(pit)
        a, _ = compare(f0[i, LEAD:LEAD + n], harm[i, LEAD:LEAD + n], amin[i, LEAD:LEAD + n], ref, name)
        assert (f0[i, :LEAD] == 0).all() and (f0[i, LEAD + n:] == 0).all()
        aside += a
        total += n
    assert total == 200 and aside <= 0.02 * total, (aside, total)


@gpu
def test_nan_behind_the_utterances_and_zeros_outside_the_frames(built):
    waves, lengths, _, ln, F_max = batch()
    rows = pad_rows([x.astype(np.float32) / np.float32(32768.0) for x in waves], fill=np.nan)
    rows = np.concatenate([rows, np.full((len(waves), 1024), np.nan, dtype=np.float32)], axis=1)   # also behind the longest one
    out = module().transform(torch.from_numpy(rows).to(dev()), ln, F_max, aux=True)
    for got, want in zip(out, batch_outputs()):
        assert torch.isfinite(got).all()                         # a read past an utterance's own samples would poison an output
        assert torch.equal(got, want)
    for v in out:
        v = v.cpu().numpy()
        for i, L in enumerate(lengths):
            n = Y.n_frames(L, WLEN, HOP)
            assert (v[i, :LEAD] == 0).all() and (v[i, LEAD + n:] == 0).all(), (i, L)
    assert (out[1].cpu().numpy()[5, LEAD:LEAD + 33] > 0).all()    # harm is positive on every frame


@gpu
def test_batch_row_equals_the_utterance_alone(built):
    waves, lengths, _, _, _ = batch()
    f0, harm, amin = batch_outputs()
    for i, (x, L) in enumerate(zip(waves, lengths)):
        n = Y.n_frames(L, WLEN, HOP)
        F1 = 1 + L // HOP
        y1 = torch.from_numpy(pad_rows([x])).to(dev())
        a, b, c = module().transform(y1, torch.tensor([L], dtype=torch.int32, device=dev()), F1, aux=True)
        assert a.shape == (1, F1) and F1 >= LEAD + n
        for one, row in ((a, f0), (b, harm), (c, amin)):
            assert torch.equal(one[0], row[i, :F1]), (i, L)
        # another lead and another row width move the frames, not their bits
        a0, _, _ = module().transform(y1, torch.tensor([L], dtype=torch.int32, device=dev()), max(n, 1), lead=0)
        assert torch.equal(a0[0, :n], f0[i, LEAD:LEAD + n]), (i, L)


@gpu
def test_int16_equals_fp32_of_the_same_samples(built):
    _, _, y, ln, F_max = batch()
    got = module().transform(y.float() / 32768.0, ln, F_max, aux=True)
    for p, q in zip(got, batch_outputs()):
        assert torch.equal(p, q)
    assert batch_outputs()[0].max().item() > 100.0


@gpu
def test_aux_outputs_are_optional(built):
    _, _, y, ln, F_max = batch()
    f0, harm, amin = module().transform(y, ln, F_max, aux=False)
    assert harm is None and amin is None and torch.equal(f0, batch_outputs()[0])


@gpu
def test_silent_utterance(built):
    y = torch.zeros(2, 5000, dtype=torch.int16, device=dev())
    f0, harm, amin = module().transform(y, torch.tensor([5000, 4000], dtype=torch.int32, device=dev()), 1 + 5000 // HOP, aux=True)
    assert (f0 == 0).all() and (amin == 0).all()
    n0, n1 = Y.n_frames(5000, WLEN, HOP), Y.n_frames(4000, WLEN, HOP)
    assert (harm[0, LEAD:LEAD + n0] == 1).all() and (harm[1, LEAD:LEAD + n1] == 1).all()
    assert (harm[0, :LEAD] == 0).all() and (harm[0, LEAD + n0:] == 0).all() and (harm[1, LEAD + n1:] == 0).all()


@gpu
def test_widest_lag_range_and_a_short_output_row(built):
    """tau_min = 2, tau_max = 512 (every lag the kernel computes is used; eps_c for that range), and F_max = 10 positions for 16 frames:
    the frames that fit are the same"""
    from glow_tts_amd import audio
    mod = audio.YIN(f0_min=43, f0_max=11025).to(dev())
    assert (mod.tau_min, mod.tau_max) == (2, 512)
    eps = Y.eps_c(WLEN, 512)
    waves = [golden()[f"{name}_wav"][:4865] for name in ("vibrato", "gated")]
    y = torch.from_numpy(pad_rows(waves)).to(dev())
    ln = torch.tensor([4865, 4865], dtype=torch.int32, device=dev())
    f0, harm, amin = (v.cpu().numpy() for v in mod.transform(y, ln, 40, aux=True))
    short = mod.transform(y, ln, 10)[0]
    assert torch.equal(short, torch.from_numpy(f0[:, :10]).to(dev()))
    for i, x in enumerate(waves):
        ref = Y.yin64(x.astype(np.float64) / 32768.0, SR, WLEN, HOP, 43, 11025, P["thresh"])
        n = len(ref["tau"])
        assert n == 16 and (f0[i, LEAD + n:] == 0).all()
        keep_t, keep_a = ~ref["amb_tau"], ~ref["amb_argmin"]
        assert (~keep_t | ~keep_a).sum() <= 0.02 * n
        got = np.where(f0[i] > 0, np.round(SR / np.where(f0[i] > 0, f0[i], 1.0).astype(np.float64)), 0)[LEAD:LEAD + n]
        assert (got[keep_t] == ref["tau"][keep_t]).all(), (i, got, ref["tau"])
        rel = np.abs(harm[i, LEAD:LEAD + n] - ref["harm"]) / np.abs(ref["harm"])
        assert (rel[keep_t] <= eps).all()
        assert (amin[i, LEAD:LEAD + n][keep_a] == Y.argmin_contour(ref["argmin"], 2, SR).astype(np.float32)[keep_a]).all()


@gpu
def test_graph_replay_equals_the_eager_call(built):
    _, _, y, ln, F_max = batch()
    mod = module()
    ys, ls = y.clone(), ln.clone()
    torch.cuda.synchronize()
    side, graph = torch.cuda.Stream(), torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        out = mod.transform(ys, ls, F_max, aux=True)
    y2, l2 = torch.roll(y, 1, 0).contiguous(), torch.roll(ln, 1, 0).contiguous()      # every row: other samples, another length
    ys.copy_(y2); ls.copy_(l2)
    graph.replay()
    torch.cuda.synchronize()
    want = mod.transform(y2, l2, F_max, aux=True)
    for p, q, r in zip(out, want, batch_outputs()):
        assert torch.equal(p, q) and torch.equal(p, torch.roll(r, 1, 0))


@gpu
def test_module_contract(built):
    from glow_tts_amd import audio
    waves, lengths, y, ln, F_max = batch()
    mod = module()
    assert (mod.tau_min, mod.tau_max, mod.pad_frames) == (36, 441, 2) and not list(mod.parameters()) and not list(mod.buffers())
    stft = audio.TacotronSTFT().to(dev())
    for lens in (ln, ln.cpu(), ln.long()):
        f0 = mod.f0(y, lens)
        m, _, _ = stft.mel_spectrogram(y, lens)
        assert f0.shape == (len(waves), 1, m.shape[2]) and f0.dtype == torch.float32  # the same F_max as the mel of the same call
        assert torch.equal(f0[:, 0, :F_max], batch_outputs()[0]) and (f0[:, 0, F_max:] == 0).all()
    f0, harm, amin = mod.f0(y, ln, lengths_host=lengths, aux=True)
    m, _, e = stft.mel_spectrogram(y, ln, lengths_host=lengths)
    assert f0.shape == e.shape == (len(waves), 1, F_max) and m.shape[2] == F_max and harm.shape == amin.shape == f0.shape
    assert torch.equal(harm[:, 0], batch_outputs()[1])
    one = mod.f0(y[5:6, :9435])
    assert one.shape == (1, 1, 1 + 9435 // HOP) and torch.equal(one[0, 0], batch_outputs()[0][5])
    with pytest.raises(ValueError):
        mod.f0(y.cpu())
    with pytest.raises(audio.CpuWaveError):
        mod.f0(y.cpu(), ln.cpu())
    with pytest.raises(ValueError):
        mod.f0(y, ln, lengths_host=[20000] + lengths[1:])
    # compute_yin: the reference's signature for one device waveform, unpadded; its own defaults are a geometry the kernel refuses
    x = y[5, :9435]
    pit, hr, am, times = audio.compute_yin(x, SR, w_len=1024, w_step=256, f0_min=50, f0_max=600, harmo_thresh=0.1)
    n = Y.n_frames(9435, WLEN, HOP)
    assert pit.shape == hr.shape == am.shape == times.shape == (n,)
    assert torch.equal(pit, batch_outputs()[0][5, LEAD:LEAD + n]) and torch.equal(hr, batch_outputs()[1][5, LEAD:LEAD + n])
    assert torch.equal(am, batch_outputs()[2][5, LEAD:LEAD + n])
    assert np.allclose(times.cpu().numpy(), np.arange(n) * 256 / 22050.0, rtol=1e-6, atol=0)
    with pytest.raises(Exception):
        audio.compute_yin(x, SR)


def test_collate_leaves_f0_to_the_device():
    """no GPU: TextAudioCollate with items whose f0 is None returns f0_padded = None (as for energy); items that carry f0 as before"""
    from glow_tts_amd import data
    def item(t, L, f0, en):
        return (torch.arange(t), torch.zeros(L, dtype=torch.int16), torch.zeros(512), 1, torch.zeros(3), f0, en, 0)
    out = data.TextAudioCollate()([item(3, 2000, None, None), item(5, 3000, None, None)])
    assert out[7] is None and out[8] is None and out[2].shape == (2, 3000) and out[3].tolist() == [3000, 2000]
    out = data.TextAudioCollate()([item(3, 2000, None, torch.ones(1, 8)), item(5, 3000, None, torch.ones(1, 12))])
    assert out[7] is None and out[8].shape == (2, 1, 12)
    out = data.TextAudioCollate()([item(3, 2000, torch.ones(1, 8), None), item(5, 3000, torch.ones(1, 12), None)])
    assert out[7].shape == (2, 1, 12) and out[7][1, 0].tolist() == [1.0] * 8 + [0.0] * 4 and out[8] is None
