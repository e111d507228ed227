"""GPU tests of the device mel front end (csrc/mel_front.hip, glow_tts_amd.audio) on the ragged batch of tests/mel64.py:
five signals (uniform noise, a sine on bin 40, a loud off-bin sine over 1e-4 noise, DC + Nyquist, a linear chirp) at 513, 1061,
256 * 64 - 1, 256 * 64 and 256 * 65 + 255 samples = 3, 5, 64, 65 and 66 frames, the last three on, one past and two past the kernel's
64-frame tile.

The float64 reference is tests/mel64.py (reflect padding per utterance, the exact windowed basis, the module's own mel_basis).  The
bound is derived, not fitted: a k-ordered fp32 chain of N = 1024 products has N roundings, the operands are rounded once each and the
centre fold adds one, so with u = 2^-24 and S_f = sum |w x_f| every DFT component is within d_f = (N + 4) u S_f = 6.1e-5 S_f, and
  |mag - mag64| <= sqrt(2) d_f + 4 u mag64,   |energy - energy64| <= sqrt(513) sqrt(2) d_f + 520 u energy64,
  |mel - log m| <= log1p(dmel / m) + 4 * 2^-23 * max(1, |log m|),  dmel = mel_basis (sqrt(2) d_f) + 520 u lin64,  m = max(lin64, clip)
with no element excluded.  A symmetric window is off by 2.7e-4 .. 1e-3 S_f and zero padding by >= 6e-2 S_f: both fail it."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mel64 as M  # noqa: E402

pytestmark = pytest.mark.gpu
HOP = 256


def dev():
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def module():
    from glow_tts_amd import audio
    return audio.TacotronSTFT().to(dev())


@functools.lru_cache(maxsize=None)
def batch():
    """(waves, lengths, padded fp32 [5, L_pad] on the device, int32 lengths on the device, F_max)"""
    waves, lengths = M.ragged_batch()
    pad = np.zeros((len(waves), (max(lengths) + 3) // 4 * 4), dtype=np.float32)
    for i, x in enumerate(waves):
        pad[i, :len(x)] = x
    return waves, lengths, torch.from_numpy(pad).to(dev()), torch.tensor(lengths, dtype=torch.int32, device=dev()), 1 + max(lengths) // HOP


@functools.lru_cache(maxsize=None)
def reference():
    """per utterance: (mel64 dict, bounds dict), computed once"""
    waves, _ = M.ragged_batch()
    mb = module().mel_basis.double().cpu().numpy()
    basis = M.basis64()
    refs = [M.mel64(x, mb, basis=basis) for x in waves]
    return [(r, M.bounds(r, mb)) for r in refs]


@functools.lru_cache(maxsize=None)
def batch_outputs():
    _, _, y, ln, F_max = batch()
    mel, energy, mag = module().transform(y, ln, F_max, magnitudes=True)
    torch.cuda.synchronize()
    return mel, energy, mag


def test_outputs_within_the_float64_bound(built):
    _, lengths, _, _, _ = batch()
    mel, energy, mag = (t.double().cpu().numpy() for t in batch_outputs())
    worst = {"mag": 0.0, "energy": 0.0, "mel": 0.0}
    worst_share = dict(worst)
    failures = []
    for i, ((ref, bnd), L) in enumerate(zip(reference(), lengths)):
        F = 1 + L // HOP
        got = {"mag": mag[i, :, :F], "energy": energy[i, :F], "mel": mel[i, :, :F]}
        for k in worst:
            err = np.abs(got[k] - ref[k])
            assert np.isfinite(got[k]).all()
            worst[k] = max(worst[k], float((err / ref["S"]).max()))
            worst_share[k] = max(worst_share[k], float((err / bnd[k]).max()))
            if not (err <= bnd[k]).all():
                failures.append((M.SIGNALS[i], k, float((err / bnd[k]).max())))
    print("mel front end, worst err / S_f:", {k: f"{v:.3e}" for k, v in worst.items()},
          " worst err / bound:", {k: f"{v:.3e}" for k, v in worst_share.items()}, " (d_f = 6.13e-5 S_f)")
    assert not failures, failures


def test_batch_row_equals_the_utterance_alone(built):
    waves, lengths, _, _, F_max = batch()
    mel, energy, mag = batch_outputs()
    for i, (x, L) in enumerate(zip(waves, lengths)):
        F = 1 + L // HOP
        y1 = torch.zeros(1, (L + 3) // 4 * 4, device=dev())
        y1[0, :L] = torch.from_numpy(x).to(dev())
        m1, e1, g1 = module().transform(y1, torch.tensor([L], dtype=torch.int32, device=dev()), F, magnitudes=True)
        assert m1.shape == (1, 80, F) and e1.shape == (1, F) and g1.shape == (1, 513, F)
        assert torch.equal(m1[0], mel[i, :, :F]) and torch.equal(e1[0], energy[i, :F]) and torch.equal(g1[0], mag[i, :, :F]), M.SIGNALS[i]
        assert F == F_max or (mel[i, :, F:].abs().max().item() == 0.0 and energy[i, F:].abs().max().item() == 0.0
                              and mag[i, :, F:].abs().max().item() == 0.0), M.SIGNALS[i]
        assert energy[i, :F].min().item() > 0.0


def test_int16_input_equals_fp32_of_the_same_samples(built):
    waves, lengths, y, ln, F_max = batch()
    yi = torch.round(y * 32767.0).to(torch.int16)
    a = module().transform(yi, ln, F_max, magnitudes=True)
    b = module().transform(yi.float() / 32768.0, ln, F_max, magnitudes=True)
    for p, q in zip(a, b):
        assert torch.equal(p, q)
    assert a[1].abs().max().item() > 1.0


def test_mag_is_optional(built):
    _, _, y, ln, F_max = batch()
    mel, energy, _ = batch_outputs()
    m2, e2, g2 = module().transform(y, ln, F_max, magnitudes=False)
    assert g2 is None and torch.equal(m2, mel) and torch.equal(e2, energy)


def test_module_contract(built):
    from glow_tts_amd import audio
    waves, lengths, y, ln, F_max = batch()
    T = 256 * 9 + 17
    mel, energy = module().mel_spectrogram(y[:2, :T])
    assert mel.shape == (2, 80, 1 + T // HOP) and energy.shape == (2, 1 + T // HOP) and mel.dtype == torch.float32
    mb = module().mel_basis.double().cpu().numpy()
    ref = M.mel64(y[1, :T].cpu().numpy(), mb)                                         # the unbatched call reflects about T, not the row
    assert (np.abs(mel[1].double().cpu().numpy() - ref["mel"]) <= M.bounds(ref, mb)["mel"]).all()
    for lens in (ln, ln.cpu(), ln.long()):
        m, ml, e = module().mel_spectrogram(y, lens)
        assert m.shape == (5, 80, m.shape[2]) and e.shape == (5, 1, m.shape[2]) and m.shape[2] >= F_max
        assert ml.cpu().tolist() == [1 + L // HOP for L in lengths]
        assert torch.equal(m[:, :, :F_max], batch_outputs()[0]) and torch.equal(e[:, 0, :F_max], batch_outputs()[1])
    m, ml, e = module().mel_spectrogram(y, ln, lengths_host=lengths)
    assert m.shape == (5, 80, F_max) and e.shape == (5, 1, F_max)
    with pytest.raises(ValueError):
        module().mel_spectrogram(y.cpu())
    with pytest.raises(ValueError):
        module().mel_spectrogram(y, ln, lengths_host=[512] + lengths[1:])
    with pytest.raises(ValueError):
        module().mel_spectrogram(y, torch.tensor([512] + lengths[1:]))
    with pytest.raises(ValueError):
        module().mel_spectrogram(y[:, :512])
    assert isinstance(module().stft_fn, audio.STFT) and module().mel_basis.shape == (80, 513)


def test_graph_replay_equals_the_eager_call(built):
    _, lengths, y, ln, F_max = batch()
    mod = module()
    ys, ls = y.clone(), ln.clone()
    mod.transform(ys, ls, F_max, magnitudes=True)                                     # the packed image exists before the capture
    torch.cuda.synchronize()
    side, graph = torch.cuda.Stream(), torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        out = mod.transform(ys, ls, F_max, magnitudes=True)
    y2, l2 = torch.roll(y, 1, 0).contiguous(), torch.roll(ln, 1, 0).contiguous()      # every row: other samples, another length
    ys.copy_(y2); ls.copy_(l2)
    graph.replay()
    torch.cuda.synchronize()
    want = mod.transform(y2, l2, F_max, magnitudes=True)
    for p, q, r in zip(out, want, batch_outputs()):
        assert torch.equal(p, q) and torch.equal(p, torch.roll(r, 1, 0))
