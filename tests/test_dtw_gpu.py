"""GPU tests of the synthesis metrics (csrc/dtw.hip, glow_tts_amd.metrics).

The batch: twelve utterances (Fa, Fb) = (1,1), (1,17), (17,1), (15,16), (16,33), (64,64), (65,63), (63,130), (130,65), (200,77), (0,40),
(40,0) in ONE call on guarded buffers (capacities 200 x 130, NaN behind every utterance's rows): they cross the 64-row band, the
16-cell direction word, a second, third and fourth band, in both orientations, and the empty cases.  Features: a random sequence and a
randomly time-warped, lightly perturbed copy (tests/dtw64.py: warped_pair, K = 13, columns 13..15 zero), alpha = 10 sqrt(2) / ln 10.
The reference is the float64 recurrence on the kernel's own fp32 operands; the bounds are derived in tests/dtw64.py from the fp32
format: |cost - D64| <= 2 delta D64 and C64(kernel's path) - D64 <= 2 delta D64 with delta = 11 u + (Fa + Fb) u, no utterance excluded.
Measured on an MI355X, worst err / bound: cost 0.056, the path's float64 cost 0.000 (every path of the batch is float64-optimal),
cepstrum 0.072 (N = 80), 0.043 (100), 0.048 (128), F0 sums 0.035."""
import functools
import math
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dtw64 as R  # noqa: E402
from oracle.guards import Guards  # noqa: E402

gpu = pytest.mark.gpu
SHAPES = [(1, 1), (1, 17), (17, 1), (15, 16), (16, 33), (64, 64), (65, 63), (63, 130), (130, 65), (200, 77), (0, 40), (40, 0)]
FA_MAX, FB_MAX, K = 200, 130, 13
ALPHA = np.float32(R.ALPHA_DB)


def dev():
    return torch.device("cuda:0")


def rows16(x, cap, fill):
    """x [F, k] -> [cap, 16]: columns k..15 zero, rows F..cap `fill`"""
    out = np.full((cap, 16), fill, dtype=np.float32)
    out[:len(x)] = 0.0
    out[:len(x), :x.shape[1]] = x
    return out


@functools.lru_cache(maxsize=None)
def batch():
    """-> (pairs [(a [Fa, 13], b [Fb, 13])], a rows [B, FA_MAX, 16] and b rows [B, FB_MAX, 16] with NaN behind every utterance)"""
    pairs = [R.warped_pair(Fa, Fb, K, 100 + i) for i, (Fa, Fb) in enumerate(SHAPES)]
    a = np.stack([rows16(p[0], FA_MAX, np.nan) for p in pairs])
    b = np.stack([rows16(p[1], FB_MAX, np.nan) for p in pairs])
    return pairs, a, b


@functools.lru_cache(maxsize=None)
def reference():
    """per utterance (d64 [Fa, Fb], D64, the float64-optimal path), computed once"""
    out = []
    for a, b in batch()[0]:
        d = R.dist64(a, b, ALPHA)
        cost, path = R.dtw64(d)
        out.append((d, cost, path))
    return out


def call_dtw(a, b, a_len, b_len, alpha, guards=None):
    """gt_dtw_f32 through its C-ABI -> (cost, path_len, path, status) on the device; guards: outputs on guarded buffers"""
    from glow_tts_amd import _lib
    B, Fa, Fb = a.shape[0], a.shape[1], b.shape[1]
    ld = Fa + Fb - 1
    if guards is None:
        cost = torch.empty(B, device=dev())
        path_len = torch.empty(B, dtype=torch.int32, device=dev())
        path = torch.empty(B, ld, 2, dtype=torch.int32, device=dev())
    else:
        cost = guards.out("cost", (B,))
        path_len = guards.out("path_len", (B,), dtype=torch.int32)
        path = guards.out("path", (B, ld, 2), dtype=torch.int32)
    status = torch.zeros(1, dtype=torch.int32, device=dev())
    ws = torch.empty(_lib.call.gt_dtw_workspace_bytes(B, Fa, Fb), dtype=torch.uint8, device=dev())
    _lib.call.gt_dtw_f32(a, b, a_len, b_len, B, Fa, Fb, float(alpha), cost, path_len, path, ld, ws, ws.numel(), status,
                         _lib.current_stream(dev()))
    return cost, path_len, path, status


@functools.lru_cache(maxsize=None)
def batch_outputs():
    _, a, b = batch()
    g = Guards(dev())
    ta, tb = g.inp(torch.from_numpy(a)), g.inp(torch.from_numpy(b))
    la = g.inp(torch.tensor([s[0] for s in SHAPES], dtype=torch.int32), fill=1)
    lb = g.inp(torch.tensor([s[1] for s in SHAPES], dtype=torch.int32), fill=1)
    out = call_dtw(ta, tb, la, lb, ALPHA, guards=g)
    g.verify()                                                     # nothing outside the buffers written, every element written, no NaN read
    assert out[3].item() == 0
    return out


def kernel_path(path, path_len, i):
    n = int(path_len[i])
    return [tuple(r) for r in path[i, :n].tolist()]


@gpu
def test_batch_paths_are_valid_and_costs_inside_the_bound(built):
    """Measured on an MI355X: worst |cost - D64| / (2 delta D64) = 0.0564, worst (C64(path) - D64) / (2 delta D64) = 0.0000."""
    cost, path_len, path = (t.cpu().numpy() for t in batch_outputs()[:3])
    pairs = batch()[0]
    worst_cost = worst_path = 0.0
    for i, ((Fa, Fb), (d, D64, _)) in enumerate(zip(SHAPES, reference())):
        n = int(path_len[i])
        R.check_path(path[i], n, Fa, Fb)
        assert int((path[i, :, 0] >= 0).sum()) == n == int((path[i, :, 1] >= 0).sum())
        if Fa == 0 or Fb == 0:
            assert cost[i] == 0.0 and n == 0
            continue
        kp = kernel_path(path, path_len, i)
        bound = 2.0 * R.dtw_delta(Fa, Fb) * D64
        if D64 > 0:
            worst_cost = max(worst_cost, abs(float(cost[i]) - D64) / bound)
            worst_path = max(worst_path, (R.path_cost64(d, kp) - D64) / bound)
        assert abs(float(cost[i]) - D64) <= bound, (i, Fa, Fb, float(cost[i]), D64)
        assert -1e-9 * D64 <= R.path_cost64(d, kp) - D64 <= bound, (i, Fa, Fb)
        # cost is the DP's own last cell = the fp32 sum of d along the returned path, taken in path order
        assert np.float32(cost[i]) == R.dist32_along(rows16(pairs[i][0], Fa, 0), rows16(pairs[i][1], Fb, 0), kp, ALPHA), (i, Fa, Fb)
    p8 = np.array(kernel_path(path, path_len, 8), dtype=np.float64)  # (130, 65): the warp puts the path well off the diagonal
    assert np.abs(p8[:, 0] / 129.0 - p8[:, 1] / 64.0).max() > 0.1
    print(f"dtw batch: worst |cost - D64| / bound {worst_cost:.4f}, worst (C64(path) - D64) / bound {worst_path:.4f}")


def lattice(Fa, Fb, seed):
    rng = np.random.RandomState(seed)
    return rng.randint(0, 8, (Fa, 1)).astype(np.float32), rng.randint(0, 8, (Fb, 1)).astype(np.float32)


def run_metrics_dtw(pairs, scale=1.0, cap=None):
    """glow_tts_amd.metrics.dtw on a zero-padded batch of (a, b) pairs -> (cost, path_len, path) numpy"""
    from glow_tts_amd import metrics
    Fa = cap[0] if cap else max(len(p[0]) for p in pairs)
    Fb = cap[1] if cap else max(len(p[1]) for p in pairs)
    k = pairs[0][0].shape[1]
    a = np.zeros((len(pairs), Fa, k), np.float32)
    b = np.zeros((len(pairs), Fb, k), np.float32)
    for i, (x, y) in enumerate(pairs):
        a[i, :len(x)], b[i, :len(y)] = x, y
    la = torch.tensor([len(p[0]) for p in pairs], dtype=torch.int32, device=dev())
    lb = torch.tensor([len(p[1]) for p in pairs], dtype=torch.int32, device=dev())
    res = metrics.dtw(torch.from_numpy(a).to(dev()), la, torch.from_numpy(b).to(dev()), lb, scale=scale)
    assert res.status.item() == 0
    return res.cost.cpu().numpy(), res.path_len.cpu().numpy(), res.path.cpu().numpy()


def assert_equals_oracle(pairs, out):
    cost, path_len, path = out
    for i, (a, b) in enumerate(pairs):
        D64, p64 = R.dtw64(R.dist64(a, b))
        assert float(cost[i]) == D64, (i, float(cost[i]), D64)
        assert kernel_path(path, path_len, i) == p64, i
        R.check_path(path[i], int(path_len[i]), len(a), len(b))


@gpu
def test_integer_lattice_equals_the_oracle_step_for_step(built):
    """K = 1, features in 0..7: every d and every partial sum is exact in fp32, so cost equals the oracle's exactly and the path equals
    the oracle's: the tie rule and the direction bits"""
    pairs = [lattice(70, 50, 1), lattice(50, 70, 2)]
    assert_equals_oracle(pairs, run_metrics_dtw(pairs))
    for p in pairs:                                                 # ties do occur: some cell has two equal predecessors
        d = R.dist64(*p)
        assert (d == 0).sum() > 50


@gpu
def test_integer_lattices_on_the_kernels_other_paths(built):
    """past 1 024 rows the bands take several passes (the pass row in LDS, the rings used again); past what fits the LDS next to the
    rings b's features come from global memory: both exact against the oracle, next to a short utterance in the same call"""
    from glow_tts_amd import _lib
    pairs = [lattice(1030, 70, 3), lattice(64, 33, 4)]
    assert _lib.call.gt_dtw_lds_bytes(1030, 70) == 16 * 512 + 288 + 64 * 70
    assert_equals_oracle(pairs, run_metrics_dtw(pairs))
    pairs = [lattice(3, 2600, 5), lattice(130, 300, 6)]
    assert _lib.call.gt_dtw_lds_bytes(130, 2600) == 3 * 512                          # no image of b
    assert_equals_oracle(pairs, run_metrics_dtw(pairs))


@gpu
def test_identical_and_stretched_sequences(built):
    rng = np.random.RandomState(7)
    x = rng.randn(100, 13).astype(np.float32)
    y = rng.randn(70, 13).astype(np.float32)
    cost, path_len, path = run_metrics_dtw([(x, x), (np.repeat(y, 2, axis=0), y), (y, np.repeat(y, 2, axis=0))], scale=R.ALPHA_DB)
    assert cost.tolist() == [0.0, 0.0, 0.0]
    assert kernel_path(path, path_len, 0) == [(i, i) for i in range(100)]            # the pure diagonal
    assert path_len.tolist() == [100, 140, 140]
    R.check_path(path[1], 140, 140, 70)
    R.check_path(path[2], 140, 70, 140)


@gpu
def test_batch_row_equals_the_utterance_alone(built):
    """B = 1, the utterance's own lengths as capacities (another number of waves, another workspace pitch), zeros behind it"""
    cost, path_len, path, _ = batch_outputs()
    cost, path_len, path = cost.cpu().numpy(), path_len.cpu().numpy(), path.cpu().numpy()
    for i, ((Fa, Fb), (a, b)) in enumerate(zip(SHAPES, batch()[0])):
        c1, n1, p1 = run_metrics_dtw([(a, b)], scale=float(ALPHA))
        assert np.array_equal(c1.view(np.int32), cost[i:i + 1].view(np.int32)), (i, Fa, Fb)
        assert n1[0] == path_len[i] and np.array_equal(p1[0, :n1[0]], path[i, :n1[0]]), (i, Fa, Fb)
        assert (p1[0, n1[0]:] == -1).all()


@gpu
def test_graph_replay_equals_the_eager_call(built):
    from glow_tts_amd import metrics
    _, a, b = batch()
    a, b = torch.from_numpy(np.nan_to_num(a)).to(dev()), torch.from_numpy(np.nan_to_num(b)).to(dev())
    la = torch.tensor([s[0] for s in SHAPES], dtype=torch.int32, device=dev())
    lb = torch.tensor([s[1] for s in SHAPES], dtype=torch.int32, device=dev())
    first = metrics.dtw(a, la, b, lb, scale=float(ALPHA))                            # the workspace of the shape exists from here on
    sa, sb, sla, slb = a.clone(), b.clone(), la.clone(), lb.clone()
    torch.cuda.synchronize()
    side, graph = torch.cuda.Stream(), torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        res = metrics.dtw(sa, sla, sb, slb, scale=float(ALPHA))
    a2, b2 = torch.roll(a, 1, 0).contiguous(), torch.roll(b, 1, 0).contiguous()      # every row: other frames, other lengths
    la2, lb2 = torch.roll(la, 1, 0).contiguous(), torch.roll(lb, 1, 0).contiguous()
    sa.copy_(a2); sb.copy_(b2); sla.copy_(la2); slb.copy_(lb2)
    graph.replay()
    torch.cuda.synchronize()
    want = metrics.dtw(a2, la2, b2, lb2, scale=float(ALPHA))
    ref = batch_outputs()
    for got, eager, rolled in ((res.cost, want.cost, first.cost), (res.path_len, want.path_len, first.path_len), (res.path, want.path, first.path)):
        assert torch.equal(got, eager) and torch.equal(got, torch.roll(rolled, 1, 0))
    assert torch.equal(first.cost, ref[0]) and torch.equal(first.path, ref[2])       # and the eager call is the guarded batch


@gpu
def test_bad_lengths_set_the_status_bit_and_leave_an_empty_result(built):
    a = torch.randn(4, 20, 16, device=dev())
    b = torch.randn(4, 30, 16, device=dev())
    la = torch.tensor([21, 5, -1, 20], dtype=torch.int32, device=dev())
    lb = torch.tensor([5, 37, 5, 30], dtype=torch.int32, device=dev())
    cost, path_len, path, status = call_dtw(a, b, la, lb, 1.0)
    assert status.item() == 1                                                        # GT_DTW_ST_BAD_LEN
    assert cost[:3].tolist() == [0.0, 0.0, 0.0] and path_len.tolist()[:3] == [0, 0, 0] and (path[:3] == -1).all().item()
    n = int(path_len[3])
    R.check_path(path[3].cpu().numpy(), n, 20, 30)
    assert cost[3].item() > 0


# ---- gt_mel_cepstrum --------------------------------------------------------------------------------------------------------------
FRAMES = [1, 63, 64, 65, 130]


@gpu
@pytest.mark.parametrize("N", [80, 100, 128])
def test_mel_cepstrum_inside_its_bound(built, N):
    """|c - c64| <= gamma(N + 1) sum_n |w[k, n] m[n]| on the kernel's fp32 operands; NaN behind every utterance's frames and behind the
    matrix's K rows; zero tail; mel + 3 gives the same coefficients to the bound.  Measured on an MI355X, worst err / bound: 0.072
    (N = 80), 0.043 (N = 100), 0.048 (N = 128)."""
    from glow_tts_amd import _lib, metrics
    mod = metrics.MelCepstrum(N, K).to(dev())
    F_max, ld, B = 130, 132, len(FRAMES)
    w = mod.dct.cpu().numpy()
    outs = []
    for shift in (0.0, 3.0):
        mel = np.full((B, N, ld), np.nan, dtype=np.float32)
        rng2 = np.random.RandomState(N)
        for i, F in enumerate(FRAMES):
            mel[i, :, :F] = (rng2.randn(N, F) * 2.0 - 5.0).astype(np.float32) + np.float32(shift)
        g = Guards(dev())
        out = g.out("out", (B, F_max, 16))
        _lib.call.gt_mel_cepstrum(g.inp(torch.from_numpy(mel)), ld, g.inp(torch.tensor(FRAMES, dtype=torch.int32), fill=1), g.inp(mod.dct), B,
                                  N, K, F_max, out, _lib.current_stream(dev()))
        g.verify()
        outs.append((mel, out.cpu().numpy().astype(np.float64)))
    worst = 0.0
    bounds = []
    for mel, got in outs:
        per = []
        for i, F in enumerate(FRAMES):
            c64, bound = R.cepstrum64(mel[i, :, :F], w)
            ratio = np.abs(got[i, :F, :K] - c64) / bound
            worst = max(worst, float(ratio.max()))
            assert (ratio <= 1.0).all(), (N, F, float(ratio.max()))
            assert not got[i, F:].any() and not got[i, :, K:].any(), (N, F)             # zero tail: frames and coefficients
            per.append(bound)
        bounds.append(per)
    row_sum = np.abs(w.astype(np.float64).sum(1))                                      # the fp32 rows sum to zero only to their rounding
    for i, F in enumerate(FRAMES):
        diff = np.abs(outs[0][1][i, :F, :K] - outs[1][1][i, :F, :K])
        assert (diff <= bounds[0][i] + bounds[1][i] * (1.0 + 1.0 / (N + 1)) + 3.0 * row_sum[None, :]).all(), (N, F)   # + the rounding of mel + 3
    mel0 = torch.from_numpy(np.nan_to_num(outs[0][0][:, :, :F_max])).to(dev())
    via = mod(mel0, torch.tensor(FRAMES))                                              # the module is that call
    assert via.shape == (B, F_max, 16) and np.array_equal(via.cpu().numpy().astype(np.float64), outs[0][1])
    print(f"cepstrum N = {N}: worst err / bound {worst:.3f}")


# ---- gt_dtw_f0_stats --------------------------------------------------------------------------------------------------------------
def contours(seed, F):
    """voiced and unvoiced stretches: [B, F] Hz, 0 = unvoiced"""
    rng = np.random.RandomState(seed)
    f = np.zeros((len(SHAPES), F), np.float32)
    for i in range(len(SHAPES)):
        t = 0
        while t < F:
            n = rng.randint(3, 25)
            if rng.rand() < 0.65:
                f[i, t:t + n] = (rng.uniform(90, 280) * (1 + 0.15 * rng.randn(len(f[i, t:t + n])))).clip(60, 500)
            t += n
    return f


@gpu
def test_f0_stats_on_the_batchs_own_paths(built):
    """counts exact, sums within gamma(P + 3) of float64 on the kernel's operands, a row equals the utterance alone.  Measured on an
    MI355X: worst err / bound 0.035."""
    from glow_tts_amd import _lib, metrics
    _, path_len, path, _ = batch_outputs()
    fa, fb = contours(11, FA_MAX), contours(12, FB_MAX)
    B = len(SHAPES)
    g = Guards(dev())
    counts = g.out("counts", (B, 3), dtype=torch.int32)
    sums = g.out("sums", (B, 2))
    _lib.call.gt_dtw_f0_stats(path, path.shape[1], path_len, g.inp(torch.from_numpy(fa)), FA_MAX, g.inp(torch.from_numpy(fb)), FB_MAX, B,
                              counts, sums, _lib.current_stream(dev()))
    g.verify()
    pl, pt = path_len.cpu().numpy(), path.cpu().numpy()
    worst, total_vv, total_gross = 0.0, 0, 0
    for i, (Fa, Fb) in enumerate(SHAPES):
        kp = kernel_path(pt, pl, i)
        n_vv, n_vu, n_gross, s_hz, s_ct = R.f0_stats64(fa[i], fb[i], kp)
        assert counts[i].tolist() == [n_vv, n_vu, n_gross], (i, Fa, Fb)
        total_vv, total_gross = total_vv + n_vv, total_gross + n_gross
        for got, want in ((sums[i, 0].item(), s_hz), (sums[i, 1].item(), s_ct)):
            bound = R.gamma(len(kp) + 3) * want
            assert abs(got - want) <= bound, (i, got, want)
            if want > 0:
                worst = max(worst, abs(got - want) / bound)
        # alone: B = 1, the contours cut to the utterance (another pitch)
        if Fa and Fb:
            res = metrics.DTWResult(None, path_len[i:i + 1].clone(), path[i:i + 1].contiguous(), None)
            c1, s1 = metrics.f0_stats(torch.from_numpy(fa[i:i + 1, :Fa].copy()).to(dev()), torch.from_numpy(fb[i:i + 1, :Fb].copy()).to(dev())[:, None, :], res)
            assert torch.equal(c1[0], counts[i]) and torch.equal(s1[0].view(torch.int32), sums[i].view(torch.int32)), (i, Fa, Fb)
    assert total_vv > 100 and 0 < total_gross < total_vv
    errs = metrics.f0_errors(torch.from_numpy(fa).to(dev()), torch.from_numpy(fb).to(dev()), metrics.DTWResult(None, path_len, path, None))
    want = metrics.f0_metrics_from_stats(counts.cpu(), sums.cpu(), path_len.cpu())
    for k, v in want.items():
        assert torch.allclose(errs[k].cpu().float(), v.float(), rtol=1e-6, atol=0.0, equal_nan=True), k
    assert math.isnan(errs["vde"][10].item()) and math.isnan(errs["rmse_hz"][11].item())     # the empty utterances
    print(f"f0 stats: worst err / bound {worst:.3f}")


# ---- end to end, no model needed --------------------------------------------------------------------------------------------------
@gpu
def test_evaluator_end_to_end(built):
    """Two waveforms: a tone complex whose pitch rises two octaves in 1 s (x), and audio.Resample(5, 4) of it (z: 4 samples for every 5).
    At one playback rate x is z slowed by 1.25, so x plays the part of the synthesised, longer utterance and z the reference.  Only
    relations are asserted: MCD-DTW below the frame-by-frame MCD over the common length, the path's slope (frames of x per frame of
    z) between 1.1 and 1.4 in its middle half, rmse_cents along the path below the unaligned one; CPU tensors raise; the launches
    are the seven DESIGN.md 4.27 lists.  Measured on an MI355X: MCD-DTW 29.8 dB against 123.9 dB frame by frame, slope 1.263,
    110.6 cents along the path against 636.9 unaligned."""
    from glow_tts_amd import _lib, audio, metrics
    sr = 22050
    t = torch.arange(sr, dtype=torch.float64) / sr
    phase = 2 * math.pi * 100.0 * (2.0 ** (2.0 * t) - 1.0) / (2.0 * math.log(2.0))       # f(t) = 100 * 4^t Hz
    x = sum(torch.sin(h * phase) / h for h in range(1, 6)).float().mul(0.3)[None, :].to(dev())
    z, z_len = audio.Resample(5, 4).to(dev())(x)
    x_len = torch.tensor([sr], dtype=torch.int32, device=dev())
    stft, yin = audio.TacotronSTFT().to(dev()), audio.YIN().to(dev())
    mel_x, mel_x_len, _ = stft.mel_spectrogram(x, x_len)
    ev = metrics.Evaluator(stft, yin)
    ev.score(mel_x, mel_x_len, z, z_len, x, x_len)                                       # images and workspaces exist from here on
    with _lib.record_calls() as names:
        s = ev.score(mel_x, mel_x_len, z, z_len, x, x_len)
    assert names == ["gt_mel_spectrogram", "gt_mel_cepstrum", "gt_mel_cepstrum", "gt_dtw_f32", "gt_yin_f0", "gt_yin_f0", "gt_dtw_f0_stats"]
    Fa, Fb = int(mel_x_len[0]), 1 + int(z_len[0]) // 256
    assert Fa == 87 and Fb == 69 and s["status"].item() == 0
    n = int(s["path_len"][0])
    path = s["path"][0, :n].cpu().numpy()
    R.check_path(s["path"][0].cpu().numpy(), n, Fa, Fb)
    # the frame-by-frame MCD over the common length
    mel_z, _, _ = stft.mel_spectrogram(z, z_len)
    cep = metrics.MelCepstrum().to(dev())
    ca, cb = cep(mel_x, mel_x_len)[0, :Fb, :13], cep(mel_z)[0, :Fb, :13]
    plain = (R.ALPHA_DB * (ca - cb).pow(2).sum(1).sqrt()).mean().item()
    mcd = s["mcd"][0].item()
    print(f"end to end: MCD-DTW {mcd:.3f} dB, frame by frame {plain:.3f} dB, path_len {n}")
    assert 0 < mcd < plain
    q = path[n // 4: n - n // 4]
    slope = (q[-1, 0] - q[0, 0]) / max(q[-1, 1] - q[0, 1], 1)
    print(f"end to end: slope {slope:.3f}")
    assert 1.1 <= slope <= 1.4
    f0_x, f0_z = yin.f0(x, x_len)[0, 0], yin.f0(z, z_len)[0, 0]
    both = (f0_x[:Fb] > 0) & (f0_z[:Fb] > 0)
    assert both.sum().item() > 30 and s["n_voiced"][0].item() > 30
    unaligned = (1200.0 * torch.log2(f0_x[:Fb][both] / f0_z[:Fb][both])).pow(2).mean().sqrt().item()
    print(f"end to end: rmse_cents {s['rmse_cents'][0].item():.1f} along the path, {unaligned:.1f} unaligned")
    assert s["rmse_cents"][0].item() < unaligned
    assert 0.0 <= s["vde"][0].item() <= 1.0 and 0.0 <= s["gpe"][0].item() <= 1.0 and s["rmse_hz"][0].item() >= 0
    # mcd_dtw is the first half of score
    res = metrics.mcd_dtw(mel_x, mel_x_len, mel_z, torch.tensor([Fb], dtype=torch.int32, device=dev()))
    assert torch.equal(res.cost, s["cost"]) and torch.equal(res.path, s["path"]) and torch.equal(res.mean, s["mcd"])
    for bad in ((mel_x.cpu(), mel_x_len, z, z_len), (mel_x, mel_x_len, z.cpu(), z_len.cpu()), (mel_x, mel_x_len, z, z_len, x.cpu(), x_len.cpu())):
        with pytest.raises(_lib.CpuTensorError):
            ev.score(*bad)
