"""GPU tests of the device resampler (csrc/resample.hip, glow_tts_amd.audio.Resample).

Per rate pair of tests/resample64.py (48 000, 16 000, 44 100 and 24 000 -> 22 050 Hz, 22 050 -> 16 000 Hz) two ragged batches: the
four fp32 signals (noise, a sine at 0.45 of the lower rate, full-scale DC, impulses at both ends) and the int16 full-scale square wave,
each at seven lengths: 1, 5, the inputs whose n_out is tile - 1, tile, tile + 1 and 2 tile + 3 of the kernel's 512-output tile
(gt_resample_tile_out; where up > down n_out skips values and the shortest input with at least that many outputs is taken), and 0.
Output rows are 8 elements longer than the longest utterance's output, so every row has a zero tail.

The reference is the float64 direct form on the kernel's own fp32 operands and the bound
|y - y64| <= (T + 2) 2^-24 sum_j |bank[p, j] x[k0 - j]| + T 2^-126 (tests/resample64.py, derived there from the fp32 format; a
tap-ordered float32 evaluation uses 0.07 - 0.20 of it, tests/test_resample_host.py), no element excluded.
Measured on an MI355X, worst err / bound per pair: 0.100 (48 000), 0.210 (16 000), 0.088 (44 100), 0.176 (24 000) and 0.163
(22 050 -> 16 000)."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import resample64 as R  # noqa: E402
from oracle.guards import Guards  # noqa: E402

gpu = pytest.mark.gpu
TILE = 512
FP32_SIGNALS = R.SIGNALS[:4]
pairs = pytest.mark.parametrize("pair", R.PAIRS, ids=[f"{a}to{b}" for a, b in R.PAIRS])


def dev():
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def module(pair):
    from glow_tts_amd import audio
    return audio.Resample(*pair).to(dev())


def lengths_of(pair):
    up, down = R.ratio(*pair)
    return [1, 5] + [R.length_for(m, up, down) for m in (TILE - 1, TILE, TILE + 1, 2 * TILE + 3)] + [0]


def pad_rows(waves, fill):
    width = (max(len(x) for x in waves) + 3) // 4 * 4
    out = np.full((len(waves), width), fill, dtype=waves[0].dtype)
    for i, x in enumerate(waves):
        out[i, :len(x)] = x
    return out


@functools.lru_cache(maxsize=None)
def batch(pair, kind):
    """kind "fp32": the four fp32 signals x seven lengths, NaN behind every utterance; "i16": the square wave x seven lengths.
    -> (utterances, lengths, padded rows (numpy), ld_out)"""
    names = FP32_SIGNALS if kind == "fp32" else R.SIGNALS[4:]
    waves = [R.signal(name, L, *pair) for name in names for L in lengths_of(pair)]
    lengths = [len(x) for x in waves]
    up, down = R.ratio(*pair)
    ld_out = (max(R.n_out(L, up, down) for L in lengths) + 3) // 4 * 4 + 8
    return waves, lengths, pad_rows(waves, np.nan if kind == "fp32" else 12345), ld_out


@functools.lru_cache(maxsize=None)
def reference(pair, kind):
    """per utterance (y64, bound) on the fp32 operands, computed once"""
    up, down = R.ratio(*pair)
    bank = module(pair).bank.cpu().numpy()
    out = []
    for x in batch(pair, kind)[0]:
        y64, mag = R.direct(R.as_f32(x), bank, up, down)
        out.append((y64, R.bound(mag, bank.shape[1])))
    return out


@functools.lru_cache(maxsize=None)
def batch_outputs(pair, kind):
    """the kernel through its C-ABI on guarded buffers -> (out [B, ld_out], out_len [B]) on the device"""
    from glow_tts_amd import _lib
    _, lengths, rows, ld_out = batch(pair, kind)
    mod = module(pair)
    g = Guards(dev())
    wav = g.inp(torch.from_numpy(rows), fill=float("nan") if kind == "fp32" else 12345)
    ln = g.inp(torch.tensor(lengths, dtype=torch.int32), fill=1)
    out = g.out("out", (len(lengths), ld_out))
    out_len = g.out("out_len", (len(lengths),), dtype=torch.int32)
    _lib.call.gt_resample(wav, int(kind == "i16"), rows.shape[1], ln, len(lengths), mod.bank, mod.up, mod.down, mod.taps, out, ld_out,
                          out_len, _lib.current_stream(dev()))
    g.verify()                                                     # nothing outside the buffers written, every element written, no NaN read
    return out, out_len


@gpu
@pairs
def test_every_output_inside_the_bound(built, pair):
    from glow_tts_amd import _lib
    up, down = R.ratio(*pair)
    assert _lib.lib().gt_resample_tile_out() == TILE and module(pair).taps == R.TAPS[pair]
    want_n = [R.n_out(L, up, down) for L in lengths_of(pair)]
    assert want_n[:2] == [R.n_out(1, up, down), R.n_out(5, up, down)] and want_n[-1] == 0
    for got, m in zip(want_n[2:6], (TILE - 1, TILE, TILE + 1, 2 * TILE + 3)):
        assert got == m if up <= down else m <= got <= m + 1
    worst = 0.0
    for kind in ("fp32", "i16"):
        _, lengths, _, ld_out = batch(pair, kind)
        out, out_len = (v.cpu().numpy() for v in batch_outputs(pair, kind))
        assert out_len.tolist() == [R.n_out(L, up, down) for L in lengths]          # L = 0 included
        for i, ((y64, bnd), L) in enumerate(zip(reference(pair, kind), lengths)):
            n = len(y64)
            assert n == R.n_out(L, up, down) <= ld_out - 8
            assert not out[i, n:].any(), (kind, i, L)                                # zero from n_out_b to ld_out
            if n:
                ratio = np.abs(out[i, :n].astype(np.float64) - y64) / bnd
                worst = max(worst, float(ratio.max()))
                assert (ratio <= 1.0).all(), (kind, i, L, float(ratio.max()))
        assert np.abs(out).max() > 0.5
    print(f"{pair[0]} -> {pair[1]}: worst err / bound {worst:.3f}")


@gpu
@pairs
def test_batch_row_equals_the_utterance_alone(built, pair):
    """noise and the int16 square wave at every length: alone (B = 1, another ld_out, no NaN behind it) the same bits"""
    mod = module(pair)
    for kind in ("fp32", "i16"):
        waves, lengths, _, _ = batch(pair, kind)
        out, _ = batch_outputs(pair, kind)
        for i in range(7):                                                           # the first signal of the batch
            x, L = waves[i], lengths[i]
            if L == 0:
                continue
            n = mod.out_len(L)
            one, one_len = mod.transform(torch.from_numpy(pad_rows([x], 0)).to(dev()), torch.tensor([L], dtype=torch.int32, device=dev()), n)
            assert one.shape == (1, n) and one_len.tolist() == [n]
            assert torch.equal(one[0], out[i, :n]), (kind, L)


@gpu
@pairs
def test_int16_equals_fp32_of_the_same_samples(built, pair):
    _, lengths, rows, ld_out = batch(pair, "i16")
    mod = module(pair)
    ln = torch.tensor(lengths, dtype=torch.int32, device=dev())
    image = torch.from_numpy(rows).to(dev()).float() / 32768.0
    got, got_len = mod.transform(image, ln, ld_out)
    out, out_len = batch_outputs(pair, "i16")
    assert torch.equal(got, out) and torch.equal(got_len, out_len)
    assert out.abs().max().item() > 1.0                                              # the square wave overshoots: it is not clipped


@gpu
def test_long_rows_take_several_tiles_per_workgroup(built):
    """24 rows of 257 tiles: the host lets a workgroup take three tiles (the loop over tiles, the workgroup whose last tile does not
    exist, a row that ends inside a workgroup's second tile, an empty row).  Every row equals the utterance alone (one tile per
    workgroup), and a short row the float64 reference."""
    pair = (48000, 22050)
    mod = module(pair)
    ld_out = TILE * 256 + 4
    T_in = (ld_out * mod.down) // mod.up + 4 & ~3
    x = torch.randint(-32768, 32768, (T_in,), generator=torch.Generator().manual_seed(5), dtype=torch.int32).to(torch.int16)
    y = x.to(dev())[None, :].repeat(24, 1)
    lengths = [T_in] * 24
    lengths[1], lengths[2], lengths[3], lengths[4] = R.length_for(TILE * 4 + 100, mod.up, mod.down), 0, 700, R.length_for(TILE * 3, mod.up, mod.down)
    out, out_len = mod.transform(y, torch.tensor(lengths, dtype=torch.int32, device=dev()), ld_out)
    assert out_len.tolist() == [min(mod.out_len(L), ld_out) for L in lengths] and out_len[0].item() == ld_out
    alone = {}
    for i, L in enumerate(lengths):
        if L not in alone:
            alone[L] = mod.transform(y[:1], torch.tensor([L], dtype=torch.int32, device=dev()), ld_out)[0][0] if L else torch.zeros_like(out[0])
        assert torch.equal(out[i], alone[L]), (i, L)
    y64, mag = R.direct(R.as_f32(x[:700].numpy()), mod.bank.cpu().numpy(), mod.up, mod.down)
    got = out[3, :len(y64)].cpu().numpy().astype(np.float64)
    assert (np.abs(got - y64) <= R.bound(mag, mod.taps)).all() and not out[3, len(y64):].any().item()


@gpu
def test_graph_replay_equals_the_eager_call(built):
    pair = (48000, 22050)
    _, lengths, rows, ld_out = batch(pair, "i16")
    mod = module(pair)
    y, ln = torch.from_numpy(rows).to(dev()), torch.tensor(lengths, dtype=torch.int32, device=dev())
    ys, ls = y.clone(), ln.clone()
    torch.cuda.synchronize()
    side, graph = torch.cuda.Stream(), torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        out = mod.transform(ys, ls, ld_out)
    y2, l2 = torch.roll(y, 1, 0).contiguous(), torch.roll(ln, 1, 0).contiguous()     # every row: other samples, another length
    ys.copy_(y2); ls.copy_(l2)
    graph.replay()
    torch.cuda.synchronize()
    want = mod.transform(y2, l2, ld_out)
    for p, q, r in zip(out, want, batch_outputs(pair, "i16")):
        assert torch.equal(p, q) and torch.equal(p, torch.roll(r, 1, 0))


@gpu
def test_mel_and_f0_of_a_48k_batch(built):
    """sampling_rate=48000 is Resample(48000, 22050) in front of today's path: the same bits, the same frame counts, mel, energy and
    f0 of one batch lined up; None and the module's own rate are today's path"""
    from glow_tts_amd import audio
    stft, yin = audio.TacotronSTFT().to(dev()), audio.YIN().to(dev())
    rs = module((48000, 22050))
    lengths = [48000, 30011, 20000]
    t = torch.arange(48000, dtype=torch.float32)
    y = torch.stack([torch.sin(2 * np.pi * f / 48000.0 * t) * 0.5 for f in (110.0, 220.0, 330.0)]).to(dev())
    for lens, host in ((torch.tensor(lengths, device=dev()), None), (torch.tensor(lengths), None), (torch.tensor(lengths, device=dev()), lengths)):
        y22, l22 = rs(y, lens, host)
        host22 = None if host is None and lens.is_cuda else [rs.out_len(v) for v in lengths]
        assert l22.tolist() == [rs.out_len(v) for v in lengths] and y22.shape[1] == (rs.out_len(48000) if host22 is None else max(host22))
        mel, mel_len, energy = stft.mel_spectrogram(y, lens, host, sampling_rate=48000)
        mel2, mel_len2, energy2 = stft.mel_spectrogram(y22, l22, host22)
        assert mel.shape == mel2.shape and torch.equal(mel, mel2) and torch.equal(mel_len, mel_len2) and torch.equal(energy, energy2)
        assert mel_len.tolist() == [1 + rs.out_len(v) // 256 for v in lengths]
        f0 = yin.f0(y, lens, host, sampling_rate=48000)
        assert torch.equal(f0, yin.f0(y22, l22, host22)) and f0.shape == (3, 1, mel.shape[2])       # lined up with the mel
    voiced = f0[0, 0, 4:80]
    assert ((voiced - 110.0).abs() < 2.0).all()                                      # the pitch survives the conversion
    m1, e1 = stft.mel_spectrogram(y[:, :22052], sampling_rate=48000)                 # the reference's call
    m2, e2 = stft.mel_spectrogram(rs(y[:, :22052])[0])
    assert torch.equal(m1, m2) and torch.equal(e1, e2) and m1.shape[2] == 1 + rs.out_len(22052) // 256
    y1 = y[:, :22052].contiguous()
    for same in (None, 22050):
        a, b = stft.mel_spectrogram(y1, sampling_rate=same), stft.mel_spectrogram(y1)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
        assert torch.equal(yin.f0(y1, sampling_rate=same), yin.f0(y1))
    assert not list(yin.buffers()) and [k for k, _ in stft.named_buffers()] == ["mel_basis", "stft_fn.forward_basis"]


@gpu
def test_module_contract(built):
    from glow_tts_amd import _lib, audio
    pair = (48000, 22050)
    waves, lengths, rows, _ = batch(pair, "i16")
    mod = module(pair)
    out, out_len = batch_outputs(pair, "i16")
    assert (mod.up, mod.down, mod.taps) == (147, 320, 44) and [k for k, _ in mod.named_buffers()] == ["bank"] and not list(mod.parameters())
    assert mod.bank.dtype == torch.float32 and tuple(mod.bank.shape) == (147, 44)
    y, ln = torch.from_numpy(rows).to(dev()), torch.tensor(lengths, dtype=torch.int32, device=dev())
    n_max, n_cap = max(mod.out_len(L) for L in lengths), mod.out_len(rows.shape[1])
    for lens, host, cap in ((ln, None, n_cap), (ln.cpu(), None, n_max), (ln.long(), lengths, n_max)):
        got, got_len = mod(y, lens, host)
        assert got.shape == (len(lengths), cap) and got.dtype == torch.float32 and got_len.dtype == torch.int32 and got_len.is_cuda
        assert torch.equal(got_len, out_len) and torch.equal(got[:, :n_max], out[:, :n_max]) and not got[:, n_max:].any().item()
    assert n_max % 4 and n_cap > n_max                                               # a row length the kernel's pitch rounds up
    short, short_len = mod.transform(y, ln, 1001)                                    # a capacity below the longest output: clamped
    assert short.shape == (len(lengths), 1001) and torch.equal(short, out[:, :1001])
    assert short_len.tolist() == [min(mod.out_len(L), 1001) for L in lengths]
    whole, whole_len = mod(y[3:4, :lengths[3]])                                      # no lengths: every row whole
    assert whole_len.tolist() == [TILE] and torch.equal(whole[0], out[3, :TILE])
    one = audio.resample_poly(y[5, :lengths[5]], 22050, 48000)                       # scipy's signature, reduced here
    assert one.shape == (2 * TILE + 3,) and torch.equal(one, out[5, :2 * TILE + 3])
    assert audio.resample_poly(y[5, :0], 147, 320).shape == (0,)
    same = audio.Resample(22050, 22050).to(dev())
    with _lib.record_calls() as names:
        a, a_len = same(y, ln)
        b, b_len = same(a, ln.cpu())
    assert names == [] and torch.equal(a, y.float() / 32768.0) and b is a and torch.equal(a_len, ln) and torch.equal(b_len, ln)
    with pytest.raises(audio.CpuWaveError):
        mod(y.cpu(), ln.cpu())
    with pytest.raises(audio.CpuWaveError):
        audio.resample_poly(y[5].cpu(), 147, 320)
    with pytest.raises(audio.CpuWaveError):
        audio.TacotronSTFT().mel_spectrogram(y.cpu(), ln.cpu(), sampling_rate=48000)
    with pytest.raises(ValueError):
        mod(y, ln, lengths_host=[1 << 20] + lengths[1:])
    with pytest.raises(ValueError):
        audio.Resample(22050, 1000)                                                  # 20 : 441: an input span past the LDS
    with pytest.raises(ValueError):
        mod(y.double())
