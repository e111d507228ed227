"""GPU tests of the denoiser's analysis kernel and of the pair gt_denoise_spec + gt_istft (csrc/denoise.hip, audio.Denoiser; DESIGN.md
4.30) against the float64 restatement tests/denoise64.py, with the bounds derived there, not fitted.

The ragged batch is gl64's: mel64's five signals in turn at 4 and 5 analysis frames and at T, T + 1, T + 2 frames around the frame tile
and around the hop tile the library reports, plus a row of no sample; rows are filled with 7.0 behind each utterance (nothing there may
be read) and the spectrum workspace with NaN (all of it must be written).  Both values of `lost` (the mel frame counts the kernel takes
are the analysis frames - 1 + lost), a random non-negative bias, and strengths 0, 0.1 and HALF.  HALF is the float64 median of
|X| / bias over the batch's broadband (noise) utterances, so that half of THEIR (bin, frame) elements clamp to zero (asserted on the
CPU): the other signals' spectra are sparse — 41 % of the whole batch's elements clamp at a strength of 1e-7 already, 79 % at 0.1 —
so a median over the whole batch would be a strength of 3.6e-6 that subtracts nothing.  At HALF 88 % of the batch clamps.

  spectrum   every component of every Y[k][f] within denoise64.spec_bound; no element is excluded
  waveform   every sample within denoise64.wav_bound; at strength 0 also within gl64.recon_bound of the input signal
  control    two known wrong variants, measured in float64 against the same bound: the bias of bin k + 1 misses it by 228 x (strength
             0.1) and 903 x (HALF = 0.409), the clamp left out by 232 x and 950 x; a test asserts at least CONTROL_MARGIN = 100 x
  also       frames_out equal to the rule, zeros behind each utterance, a batch row bit-identical to the utterance alone
Each test prints its worst error as a share of the bound (DESIGN.md 4.30 quotes them).  Measured on an MI355X: spectrum 0.0040 / 0.0039 /
0.0038 of the bound at strengths 0 / 0.1 / HALF, waveform 2.9e-5 / 2.2e-5 / 1.2e-5 (that bound adds 513 worst-case bin errors with one
sign), strength 0 against the input signal 0.037 of gl64.recon_bound; the same for both values of `lost`."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import denoise64 as D  # noqa: E402
import gl64 as G  # noqa: E402
import mel64  # noqa: E402

pytestmark = pytest.mark.gpu

STRENGTHS = ("zero", "tenth", "half")
CONTROL_MARGIN = 100.0                                     # a wrong variant misses the bound by at least this factor


def dev():
    return torch.device("cuda:0")


def bias32():
    return np.random.default_rng(5).uniform(0.0, 50.0, D.NBIN).astype(np.float32)


@functools.lru_cache(maxsize=None)
def batch():
    """analysis frame counts (the last row has no sample) and the signals"""
    from glow_tts_amd import _lib
    frames = G.ragged_frames(_lib.lib().gt_gl_tile_frames(), _lib.lib().gt_gl_tile_hops())
    return tuple(frames) + (0,), G.ragged_signals(frames)


@functools.lru_cache(maxsize=None)
def strength(name):
    if name == "zero":
        return 0.0
    if name == "tenth":
        return float(np.float32(0.1))
    _, waves = batch()
    noise = [x for i, x in enumerate(waves) if mel64.SIGNALS[i % len(mel64.SIGNALS)] == "noise"]
    ratios = np.concatenate([(np.hypot(*G.transform(x)) / bias32().astype(np.float64)[:, None]).reshape(-1) for x in noise])
    s = float(np.float32(np.median(ratios)))
    share = np.average([D.clamped_share(x, bias32(), s) for x in noise], weights=[len(x) // G.HOP + 1 for x in noise])
    assert 0.4 < share < 0.6, share                        # about half of the broadband rows' bins clamp to zero
    whole = np.average([D.clamped_share(x, bias32(), s) for x in waves], weights=[len(x) // G.HOP + 1 for x in waves])
    assert share < whole < 0.95, whole                     # the sparse rows clamp more, and not everything
    return s


@functools.lru_cache(maxsize=None)
def reference(name):
    """per utterance: denoise64's dict, computed once per strength and shared by the tests"""
    _, waves = batch()
    return [D.denoise64(x, bias32(), strength(name)) for x in waves]


@functools.lru_cache(maxsize=None)
def denoiser():
    from glow_tts_amd import audio
    return audio.Denoiser(bias_spec=torch.from_numpy(bias32())).to(dev())


def device_run(name, lost, rows=None):
    """the kernel pair on the batch (rows: a subset of it) -> (spec re, im [B, 513, Fa_max], frames_out, wav [B, 256 (Fa_max - 1)])"""
    from glow_tts_amd import audio
    frames, waves = batch()
    rows = list(range(len(frames))) if rows is None else rows
    fa = [frames[i] for i in rows]
    n_mel = [max(F - 1, 0) + lost for F in fa]             # the vocoder's mel frames: F - 1 hops of samples, `lost` frames lost
    F_max = max(n_mel)
    Fa_max = F_max - lost + 1
    wav = np.full((len(rows), G.HOP * (F_max - lost)), 7.0, dtype=np.float32)
    for r, i in enumerate(rows):
        if frames[i]:
            wav[r, :len(waves[i])] = waves[i]
    den = denoiser().set_strength(strength(name))
    bufs = den.workspace(len(rows), F_max, dev(), lost)
    bufs["dn_spec"].fill_(float("nan"))
    bufs["dn_frames"].fill_(-7)
    w = torch.from_numpy(wav).to(dev())
    n = torch.tensor(n_mel, dtype=torch.int32, device=dev())
    assert den.analyse(w, n, lost, bufs) == Fa_max
    torch.cuda.synchronize()
    assert torch.equal(w.cpu(), torch.from_numpy(wav))     # the analysis reads only
    assert bool(torch.isfinite(bufs["dn_spec"]).all())
    re, im = (t.clone() for t in audio.spec_unpack(bufs["dn_spec"], len(rows), Fa_max))
    out = den.run(w, n, lost, bufs)
    torch.cuda.synchronize()
    assert out is w and bufs["dn_frames"].tolist() == fa == [D.analysis_frames(v, lost, F_max) for v in n_mel]
    return re, im, fa, out


@pytest.mark.parametrize("lost", (0, 1))
@pytest.mark.parametrize("name", STRENGTHS)
def test_spectrum_and_waveform_within_the_float64_bounds(built, name, lost):
    frames, waves = batch()
    re, im, _, out = device_run(name, lost)
    yre, yim, out = re.double().cpu().numpy(), im.double().cpu().numpy(), out.double().cpu().numpy()
    worst_s, worst_w, worst_o, failures = 0.0, 0.0, 0.0, []
    for i, (x, F, ref) in enumerate(zip(waves, frames, reference(name))):
        L = G.HOP * (F - 1)
        sb, wb = D.spec_bound(ref, bias32(), strength(name)), D.wav_bound(ref, bias32(), strength(name))
        es = np.maximum(np.abs(yre[i, :, :F] - ref["re"]), np.abs(yim[i, :, :F] - ref["im"])) / sb
        ew = np.abs(out[i, :L] - ref["wav"]) / wb
        worst_s, worst_w = max(worst_s, es.max()), max(worst_w, ew.max())
        line = f"denoise {name} lost={lost} utt {i} F={F}: spectrum {es.max():.4f} of the bound, waveform {ew.max():.3e}"
        ok = (es <= 1.0).all() and (ew <= 1.0).all()
        if name == "zero":
            eo = np.abs(out[i, :L] - x.astype(np.float64)) / G.recon_bound(*ref["X"])
            worst_o = max(worst_o, eo.max())
            line += f", vs the input signal {eo.max():.4f} of gl64.recon_bound"
            ok = ok and (eo <= 1.0).all()
        print(line)
        if not ok:
            failures.append((i, F))
        assert not yre[i, :, F:].any() and not yim[i, :, F:].any() and not out[i, L:].any(), i
    assert not yre[-1].any() and not yim[-1].any() and not out[-1].any()                     # the row of no sample
    print(f"denoise {name} lost={lost}: worst share of the bound {worst_s:.4f} (spectrum), {worst_w:.3e} (waveform)"
          + (f", {worst_o:.4f} (strength 0 vs the input signal)" if name == "zero" else ""))
    assert not failures, failures


@pytest.mark.parametrize("name", ("tenth", "half"))
def test_known_wrong_variants_miss_the_bound_by_a_wide_margin(built, name):
    """float64 on both sides: what the bound tells apart (the figures of the module's docstring)"""
    _, waves = batch()
    for wrong in (D.wrong_next_bin, D.wrong_no_clamp):
        miss = 0.0
        for x, ref in zip(waves, reference(name)):
            bad = wrong(x, bias32(), strength(name))
            sb = D.spec_bound(ref, bias32(), strength(name))
            miss = max(miss, (np.maximum(np.abs(bad["re"] - ref["re"]), np.abs(bad["im"] - ref["im"])) / sb).max())
        print(f"denoise control {wrong.__name__} at {name}: misses the spectrum bound by {miss:.3g} x")
        assert miss > CONTROL_MARGIN, (wrong.__name__, miss)


@pytest.mark.parametrize("lost", (0, 1))
def test_a_batch_row_is_bit_identical_to_the_utterance_alone(built, lost):
    frames, _ = batch()
    re, im, _, out = device_run("half", lost)
    re, im, out = re.clone(), im.clone(), out.clone()
    bits = lambda t: t.contiguous().view(torch.int32)  # noqa: E731
    for i in (0, 3, len(frames) - 2):                      # 4 frames, T + 1 frames (two tiles), the hop tile's T + 2
        F, L = frames[i], G.HOP * (frames[i] - 1)
        r1, i1, fa, o1 = device_run("half", lost, rows=[i])
        assert fa == [F] and o1.shape == (1, L)
        assert torch.equal(bits(r1[0]), bits(re[i, :, :F])) and torch.equal(bits(i1[0]), bits(im[i, :, :F])), i
        assert torch.equal(bits(o1[0]), bits(out[i, :L])), i
