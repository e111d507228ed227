"""GPU tests of the loudness kernels (csrc/loudness.hip, audio.Loudness) against the float64 restatement
tests/loudness64.py, with the bounds derived there, not fitted.

Cases.  Seeded noise bursts, one level per 100 ms segment in the pattern LLLLMMMMTTTTTLLLL (L = 0.3, M 30 dB below it, T 75 dB below
it), so that blocks of every mixture occur and both gates bite; at 22 050 Hz (Ns = 2205, Nb = 8820, chunk 49) the lengths 0, 1, 2204,
2205, 8819, 8820, 8821, 11024, 11025, then 38 866 = 3 workgroups of 256 chunks and 1234 samples more (no multiple of 49) and 201 481 =
one full round of the state scan (4096 chunks) and 777 samples more; one case each at 16 000 and 48 000 Hz.  All of a rate's utterances
form ONE batch whose rows are longer than every utterance, NaN behind each utterance up to the capacity and guard values behind the
capacity and around the buffer.  loudness64.cases asserts, in float64, that every block of every case lies at least 1e-3 LU from both
gates and that the peak rule is decided by a relative margin of 1e-6.  Targets -23 LUFS (no row reaches the -1 dBFS ceiling) and
-2 LUFS (every row of 100 ms or more does; the row of one sample does not).

  stats      L within loudness64.bounds' dL (and within 0.1 LU, EBU Tech 3341's tolerance, whatever the bound says), J, |A|, |R| equal,
             the peak exact, g within 2^-24 and its own error, Gamma within its bound
  sums       every 100 ms segment's sum of z^2 (the workspace's chunk sums, a segment's added up) within the bound on it
  samples    y = fp32(g) x within loudness64.sample_bound of g64 x, exactly zero from the utterance's end to the capacity, every guard
             value intact; normalize() returns the same bits in a new tensor and leaves its input as it was
  bits       a batch row — stats, chunk sums, samples — bit-identical to the utterance alone; int16 input to its fp32 image
  control    four wrong variants, float64 on both sides, against the SAME bound on L.  Worst over the cases (measured here in
             float64): the start state dropped at chunk boundaries misses it by 3.9e4 x, no relative gate by 1.7e6 x, no -0.691 offset
             by 9.5e5 x, a 50 % block overlap by 7.6e5 x; the test asserts at least CONTROL_MARGIN = 100 x for each
Each test prints its worst error as a share of the bound (DESIGN.md 4.31 quotes them)."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import loudness64 as L  # noqa: E402

pytestmark = pytest.mark.gpu

LONG, ROUND = 3 * 256 * 49 + 1234, 4096 * 49 + 777
LENGTHS = {22050: (0, 1, 2204, 2205, 8819, 8820, 8821, 11024, 11025, LONG, ROUND), 16000: (16000 * 13 // 10 + 3,), 48000: (48000 * 9 // 10 + 17,)}
TARGETS = (-23.0, -2.0)
PEAK_DBFS = -1.0
CONTROL_MARGIN = 100.0
GUARD, GUARD_VALUE = 64, 7.0


def dev():
    return torch.device("cuda:0")


def bits(t):
    return t.contiguous().view(torch.int32)


@functools.lru_cache(maxsize=None)
def meter(fs):
    from glow_tts_amd import audio
    return audio.Loudness(fs, TARGETS[0], PEAK_DBFS).to(dev())


@functools.lru_cache(maxsize=None)
def reference(fs):
    """[(x fp32, {target: loudness64's dict}, loudness64.bounds' dict)] — computed once, shared by the tests"""
    chunk = meter(fs).chunk
    return [(x, refs, L.bounds(x, fs, refs[TARGETS[0]], chunk)) for x, refs in L.cases(fs, LENGTHS[fs], seed=fs, targets=TARGETS, peak_dbfs=PEAK_DBFS)]


def device_run(fs, target, rows=None, int16=False):
    """Loudness.run on the batch (rows: a subset) inside a guarded buffer -> (stats [B, 8], chunk sums float64 [B, Kc], wav [B, L_cap],
    the flat buffer, B, L_cap, ld)"""
    ref = reference(fs)
    rows = list(range(len(ref))) if rows is None else rows
    xs = [ref[i][0] for i in rows]
    B, L_cap = len(xs), max(max(len(x) for x in xs), 1) + 11
    ld = L_cap + 13
    host = np.full((B, ld), GUARD_VALUE, dtype=np.float32)
    for r, x in enumerate(xs):
        host[r, :len(x)] = x
        host[r, len(x):L_cap] = np.nan                     # nothing behind an utterance may be read
    flat = torch.full((GUARD + B * ld + GUARD,), GUARD_VALUE, dtype=torch.float32, device=dev())
    flat[GUARD:GUARD + B * ld] = torch.from_numpy(host).reshape(-1).to(dev())
    wav = flat[GUARD:GUARD + B * ld].view(B, ld)[:, :L_cap]
    n = torch.tensor([len(x) for x in xs], dtype=torch.int32, device=dev())
    loud = meter(fs).set_target(target)
    bufs = loud.workspace(B, L_cap, dev())
    bufs["ld_stats"].fill_(float("nan"))
    out = loud.run(wav, n, 1, 0, bufs)
    torch.cuda.synchronize()
    assert out is wav
    return bufs["ld_stats"].view(B, 8).clone(), loud.chunk_sums(bufs, B, L_cap).clone(), wav, flat, B, L_cap, ld


@pytest.mark.parametrize("fs", sorted(LENGTHS))
def test_stats_and_segment_sums_within_the_float64_bounds(built, fs):
    stats, sums, *_ = device_run(fs, TARGETS[0])
    stats, sums = stats.double().cpu().numpy(), sums.cpu().numpy()
    Ns, cps = fs // 10, (fs // 10) // meter(fs).chunk
    worst_L, worst_E, worst_g, gated = 0.0, 0.0, 0.0, [0, 0]
    for i, (x, refs, bd) in enumerate(reference(fs)):
        ref, N = refs[TARGETS[0]], len(x)
        got = dict(zip(meter(fs).STATS, stats[i]))
        print(f"loudness {fs} Hz N={N}: L {got['lufs']:.6f} vs {ref['L']:.6f} (bound {bd['dL']:.3e}), J {ref['J']}, |A| {ref['nA']}, |R| {ref['nR']}")
        assert (got["blocks"], got["gated_abs"], got["gated_rel"], got["samples"]) == (ref["J"], ref["nA"], ref["nR"], N), i
        assert got["peak"] == np.float64(np.float32(ref["peak"])), i
        gated[0] += ref["J"] - ref["nA"]
        gated[1] += ref["nA"] - ref["nR"]
        if ref["L"] == -np.inf:
            assert got["lufs"] == -np.inf and got["gain"] == 1.0 and got["gamma"] == -np.inf, i
            continue
        eL = abs(got["lufs"] - ref["L"])
        assert eL <= bd["dL"] and eL <= 0.1, (i, eL, bd["dL"])
        assert abs(got["gamma"] - ref["gamma"]) <= bd["dL_double"] + L.U32 * abs(ref["gamma"]), i
        dg = ref["g"] * (L.U32 + np.log(10.0) / 20.0 * bd["dL_double"] + 4 * L.U64)
        assert abs(got["gain"] - ref["g"]) <= dg and not ref["engaged"], i
        worst_L, worst_g = max(worst_L, eL / bd["dL"]), max(worst_g, abs(got["gain"] - ref["g"]) / dg)
        for s in range(len(ref["E"])):
            E = sums[i, s * cps:(s + 1) * cps].sum()
            share = abs(E - ref["E"][s]) / (bd["dE"][s] + cps * L.U64 * ref["E"][s])
            worst_E = max(worst_E, share)
            assert share <= 1.0, (i, s, share)
    print(f"loudness {fs} Hz: worst share of the bound {worst_L:.4f} (L), {worst_E:.3e} (segment sums), {worst_g:.4f} (g)")
    if fs == 22050:
        assert gated[0] > 0 and gated[1] > 0                # both gates bite


def test_known_wrong_variants_miss_the_bound_by_a_wide_margin(built):
    """float64 on both sides: what the bound on L tells apart (the figures of the module's docstring)"""
    chunk = meter(22050).chunk
    for wrong in L.WRONG:
        miss = 0.0
        for x, refs, bd in reference(22050):
            ref = refs[TARGETS[0]]
            if ref["L"] > -np.inf:
                miss = max(miss, abs(wrong(x, 22050, chunk)["L"] - ref["L"]) / bd["dL"])
        print(f"loudness control {wrong.__name__}: misses the bound on L by {miss:.3g} x")
        assert miss > CONTROL_MARGIN, (wrong.__name__, miss)


@pytest.mark.parametrize("target", TARGETS)
def test_samples_within_the_bound_zero_behind_and_guards_intact(built, target):
    fs = 22050
    ref = reference(fs)
    stats, _, wav, flat, B, L_cap, ld = device_run(fs, target)
    y, whole = wav.double().cpu().numpy(), flat.cpu().numpy()
    worst, engaged = 0.0, 0
    for i, (x, refs, bd) in enumerate(ref):
        r, N = refs[target], len(x)
        engaged += r["engaged"]
        if N:
            share = (np.abs(y[i, :N] - r["g"] * x.astype(np.float64)) / L.sample_bound(x, r, bd["dL_double"])).max()
            worst = max(worst, share)
            assert share <= 1.0, (i, share)
            if r["engaged"]:
                assert abs(np.abs(y[i, :N]).max() - 10.0 ** (PEAK_DBFS / 20.0)) <= 3 * L.U32
        assert not y[i, N:].any(), i                       # exactly zero from the utterance's end to the capacity
    rows = whole[GUARD:GUARD + B * ld].reshape(B, ld)
    assert (whole[:GUARD] == GUARD_VALUE).all() and (whole[GUARD + B * ld:] == GUARD_VALUE).all() and (rows[:, L_cap:] == GUARD_VALUE).all()
    assert engaged == (0 if target == TARGETS[0] else len(ref) - 2)                   # all but the rows of no and of one sample
    print(f"loudness samples at {target} LUFS: worst share of the bound {worst:.4f}, peak rule engaged in {engaged} of {len(ref)} rows")
    # the stand-alone call: the same bits in a new tensor, the caller's rows untouched
    T = L_cap
    src = wav.new_full((B, T), float("nan"))
    for i, (x, _, _) in enumerate(ref):
        src[i, :len(x)] = torch.from_numpy(x).to(dev())
    keep = src.clone()
    n = torch.tensor([len(x) for x, _, _ in ref], dtype=torch.int32, device=dev())
    out, out_len = meter(fs).set_target(target).normalize(src, n)
    torch.cuda.synchronize()
    assert out.data_ptr() != src.data_ptr() and torch.equal(bits(src), bits(keep)) and out_len.tolist() == n.tolist()
    assert torch.equal(bits(out), bits(wav))
    m = meter(fs).measure(src, n)
    assert torch.equal(bits(m["stats"]), bits(stats)) and torch.equal(m["lufs"], stats[:, 0]) and torch.equal(m["gain"], stats[:, 2])


def test_a_batch_row_is_bit_identical_to_the_utterance_alone(built):
    fs = 22050
    cps_all = -(-max(LENGTHS[fs]) // meter(fs).chunk)
    stats, sums, wav, *_ = device_run(fs, TARGETS[1])
    for i, N in enumerate(LENGTHS[fs]):
        s1, c1, w1, *_ = device_run(fs, TARGETS[1], rows=[i])
        K = -(-N // meter(fs).chunk)
        assert K <= cps_all and torch.equal(bits(s1[0]), bits(stats[i])), (N, s1, stats[i])
        assert torch.equal(c1[0, :K].view(torch.int64), sums[i, :K].view(torch.int64)), N
        assert torch.equal(bits(w1[0, :N]), bits(wav[i, :N])), N


def test_int16_input_is_bit_identical_to_its_fp32_image(built):
    fs = 22050
    rng = np.random.default_rng(7)
    lengths = (0, 1, 8821, LONG)
    T = LONG + 5
    x16 = np.zeros((len(lengths), T), dtype=np.int16)
    for i, N in enumerate(lengths):
        x16[i, :N] = (L.burst(N, fs, 70 + i) * 32768.0).astype(np.int16)
        x16[i, N:] = rng.integers(-32768, 32767, T - N)    # int16 has no NaN: noise behind the utterances instead
    n = torch.tensor(lengths, dtype=torch.int32, device=dev())
    a = meter(fs).set_target(TARGETS[0]).measure(torch.from_numpy(x16).to(dev()), n)
    b = meter(fs).measure(torch.from_numpy(x16.astype(np.float32) / 32768.0).to(dev()), n)
    torch.cuda.synchronize()
    assert torch.equal(bits(a["stats"]), bits(b["stats"])) and a["blocks"].tolist() == [0.0, 1.0, 1.0, 14.0]
    ref = L.loudness64(x16[3, :LONG].astype(np.float64) / 32768.0, fs)
    assert abs(a["lufs"][3].item() - ref["L"]) <= 1e-5 and a["lufs"][0].item() == -np.inf


def test_arguments(built):
    from glow_tts_amd import audio
    loud = meter(22050)
    with pytest.raises(audio.CpuWaveError):
        loud.measure(torch.zeros(1, 100))
    with pytest.raises(audio.CpuWaveError):
        loud.normalize(torch.zeros(1, 100))
    with pytest.raises(ValueError):
        loud.normalize(torch.zeros(1, 100, dtype=torch.int16, device=dev()))          # normalize is fp32
    with pytest.raises(ValueError):
        loud.measure(torch.zeros(2, 100, device=dev()), torch.tensor([5, 101]))       # a length past the rows
    with pytest.raises(ValueError):
        loud.set_target(float("nan"))
    with pytest.raises(ValueError):
        loud.run(torch.zeros(1, 100, device=dev()), torch.tensor([100], dtype=torch.int64, device=dev()), 1, 0, loud.workspace(1, 100, dev()))
    assert loud.measure(torch.zeros(0, 100, device=dev()))["lufs"].shape == (0,)
    empty = loud.measure(torch.zeros(2, 0, device=dev()))
    assert empty["lufs"].tolist() == [-np.inf] * 2 and empty["gain"].tolist() == [1.0, 1.0]
    assert loud.normalize(torch.zeros(2, 0, device=dev())).shape == (2, 0)
    strided = torch.randn(2, 6000, device=dev())[:, ::2]                               # a strided view is made contiguous first
    assert torch.equal(bits(loud.measure(strided)["stats"]), bits(loud.measure(strided.contiguous())["stats"]))
