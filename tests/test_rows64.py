"""CPU tests of oracle/rows64.py, the float64 restatement the decoder kernels' fp64 tests compare with: the rows conv against
F.conv1d, the bf16 conversion against torch, the image decoder against a packer with the kernel's index formulas, and the
planted-defect controls of the checking rule on synthetic fp32-accumulated results."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import dropmask, rows64

HALO = 2


def _rows(x_bct, lengths, ragged):
    """[B, C, T] -> rows [R, C] float64 (zero outside the valid frames) and the row map"""
    B, C, T = x_bct.shape
    rm = dropmask.row_map(lengths, T, ragged=ragged)
    R = int(rm.max()) + 1 + HALO
    if ragged:
        from glow_tts_amd import ops
        _, R = ops.RowsCtx.row_starts(lengths, T, ops.DEFAULT_ROWS.row_round)
    X = torch.zeros(R, C, dtype=torch.float64)
    for b, L in enumerate(lengths):
        X[torch.from_numpy(rm[b, :L])] = x_bct[b, :, :L].T
    return X, rm


@pytest.mark.parametrize("ragged", [False, True])
@pytest.mark.parametrize("k", [1, 3, 5])
def test_rows_conv_matches_conv1d(ragged, k):
    g = torch.Generator().manual_seed(k + 10 * ragged)
    lengths, T, Cin, Cout = [9, 1, 2, 6], 9, 7, 5
    x = torch.randn(len(lengths), Cin, T, generator=g, dtype=torch.float64)
    mask = (torch.arange(T)[None, :] < torch.tensor(lengths)[:, None]).double().unsqueeze(1)
    x = x * mask
    w = torch.randn(Cout, Cin, k, generator=g, dtype=torch.float64)
    b = torch.randn(Cout, generator=g, dtype=torch.float64)
    X, rm = _rows(x, lengths, ragged)
    W = w.permute(2, 0, 1)
    Y, S = rows64.conv_rows(X, W, b)
    want = F.conv1d(x, w, b, padding=k // 2)
    Sw = F.conv1d(x.abs(), w.abs(), b.abs(), padding=k // 2)
    for bi, L in enumerate(lengths):
        r = torch.from_numpy(rm[bi, :L])
        assert torch.allclose(Y[r].T, want[bi, :, :L], rtol=1e-12, atol=1e-12)
        assert torch.allclose(S[r].T, Sw[bi, :, :L], rtol=1e-12, atol=1e-12)
    # weight gradient: sum over rows of dY x shifted X == conv1d's weight gradient on the valid frames
    dy = torch.randn(len(lengths), Cout, T, generator=g, dtype=torch.float64) * mask
    dY, _ = _rows(dy, lengths, ragged)
    dW, SW = rows64.conv_rows_wgrad(X, dY, k)
    ww = w.clone().requires_grad_(True)
    F.conv1d(x, ww, None, padding=k // 2).backward(dy)
    assert torch.allclose(dW.permute(1, 2, 0), ww.grad, rtol=1e-12, atol=1e-12)
    assert bool((SW >= dW.abs() - 1e-12).all())
    # per-utterance sums over rowutt
    rowutt = torch.zeros(X.shape[0], dtype=torch.int64)
    for bi in range(len(lengths)):
        rowutt[int(rm[bi, 0]) - HALO:] = bi
    s, _ = rows64.utt_sum(X, rowutt, len(lengths))
    assert torch.allclose(s, x.sum(2), rtol=1e-12, atol=1e-12)


def test_bf16_conversion_matches_torch():
    specials = np.array([0.0, -0.0, 1.0, 1.0 + 2 ** -8, 1.0 + 3 * 2 ** -8, 1.0 + 2 ** -8 + 2 ** -20, -(1.0 + 2 ** -8),
                         2 ** -126, 2 ** -130, 3 * 2 ** -140, 2 ** -149, 1.5 * 2 ** -133, 2.5 * 2 ** -133,
                         np.finfo(np.float32).max, -np.finfo(np.float32).max, np.inf, -np.inf, np.nan, -np.nan], dtype=np.float32)
    rnd = np.random.default_rng(0)
    u = rnd.integers(0, 2 ** 32, 200000, dtype=np.uint64).astype(np.uint32)
    vals = np.concatenate([specials, u.view(np.float32), (u & 0xFFFF8000).view(np.float32)])   # ...8000: exact ties
    mine = rows64.f2bf(vals)
    theirs = torch.from_numpy(vals).to(torch.bfloat16).view(torch.int16).numpy().astype(np.uint16)
    nan = np.isnan(vals)
    assert np.array_equal(mine[~nan], theirs[~nan])
    assert np.isnan(rows64.bf2f(mine[nan])).all() and np.isnan(rows64.bf2f(theirs[nan])).all()
    # round trip and spacing
    back = rows64.bf2f(mine[~nan])
    assert np.array_equal(rows64.f2bf(back), mine[~nan])
    x = np.array([1.0, 1.5, 2.0, 3.0, 0.1, 2 ** -126, 2 ** -130])
    assert np.array_equal(rows64.bf16_ulp(x), [2 ** -7, 2 ** -7, 2 ** -6, 2 ** -6, 2 ** -11, 2 ** -133, 2 ** -133])
    assert np.all(np.abs(rows64.bf16_round(x) - x) <= rows64.RHO["bf16"] * np.abs(x))


SHAPES = [(384, 192, 5), (160, 192, 1), (192, 80, 1), (64, 96, 3)]


# flags in use (ops.PackedConv.flags): 0 plain, 1 gate interleave, 6 fragment order, 22 fragment order + [16 | 16] interleave;
# the gate images need 2H % 64 == 0
@pytest.mark.parametrize("flags,Cout,Cin,taps", [(f, *s) for f in (0, 6) for s in SHAPES]
                         + [(f, *s) for f in (1, 22) for s in SHAPES if s[0] % 64 == 0])
def test_image_decoder_inverts_the_packer(flags, Cout, Cin, taps):
    rnd = np.random.default_rng(Cout + Cin + flags)
    W = rnd.standard_normal((taps, Cout, Cin)).astype(np.float32)
    Np_f, Kp_f = -(-Cout // 64) * 64, -(-Cin // 64) * 64
    Np_d, Kp_d = -(-Cin // 64) * 64, -(-Cout // 64) * 64
    fwd = rows64.pack_image_np(W, Np_f, Kp_f, flags)
    dgr = rows64.pack_image_np(W, Np_d, Kp_d, flags, dgrad=True)
    want = torch.from_numpy(rows64.bf16_round(W))
    assert torch.equal(rows64.decode_fwd(fwd, Cout, Cin, taps, Np_f, Kp_f, flags), want)
    assert torch.equal(rows64.decode_dgrad(dgr, Cout, Cin, taps, Np_d, Kp_d, flags), want)
    # every entry outside the weights is padding, and zero
    for img, Np, Kp, fr in ((fwd, Np_f, Kp_f, flags & 2), (dgr, Np_d, Kp_d, flags & 4)):
        full = rows64.decode_image(img, taps, Np, Kp, bool(fr))
        assert int((full != 0).sum()) == int((W != 0).sum())
        assert np.unique(rows64.pk_index(bool(fr), *np.meshgrid(np.arange(taps), np.arange(Np), np.arange(Kp), indexing="ij"),
                                         Np, Kp)).size == taps * Np * Kp


def test_packed_weights_restate_the_weight_norm_scale():
    rnd = np.random.default_rng(3)
    v = rnd.standard_normal((6, 5, 3)).astype(np.float32)
    g = rnd.uniform(0.5, 1.5, 6).astype(np.float32)
    inv = (1.0 / np.sqrt((v.astype(np.float64) ** 2).reshape(6, -1).sum(1))).astype(np.float32)
    W = rows64.packed_weights(v, g, inv)
    sc = (g * inv).astype(np.float32)
    assert torch.equal(W, torch.from_numpy(rows64.bf16_round((v * sc[:, None, None]).astype(np.float32))).permute(2, 0, 1))
    assert torch.equal(rows64.packed_weights(v), torch.from_numpy(rows64.bf16_round(v)).permute(2, 0, 1))


def _fp32_conv(X, W):
    """fp32 accumulation of the same products (a stand-in for a kernel)"""
    taps = W.shape[0]
    Y = torch.zeros(X.shape[0], W.shape[1], dtype=torch.float32)
    for t in range(taps):
        Y += rows64.shift_rows(X, t - taps // 2).float() @ W[t].float().T
    return Y.double()


def test_planted_defect_controls_trip_on_synthetic_data():
    g = torch.Generator().manual_seed(1)
    R, Cin, Cout, taps = 300, 192, 96, 5
    X = torch.from_numpy(rows64.bf16_round(torch.randn(R, Cin, generator=g).numpy()))
    W = torch.from_numpy(rows64.bf16_round((torch.randn(taps, Cout, Cin, generator=g) * 0.03).numpy()))
    got = _fp32_conv(X, W)
    ref, S = rows64.conv_rows(X, W)
    bound = rows64.gamma(taps * Cin) * S
    logs = []
    rows64.check_with_control("conv fp32", got, ref, bound, rows64.conv_rows(X, rows64.drop_weight_entry(W))[0], log=logs.append)
    rows64.check_with_control("conv fp32 row", got, ref, bound, rows64.conv_rows(rows64.drop_row(X, R // 2), W)[0], log=logs.append)
    # bf16 outputs: the mismatch share sees the defect
    gb = torch.from_numpy(rows64.bf16_round(got.numpy()))
    rows64.check_with_control("conv bf16", gb, ref, bound, rows64.conv_rows(X, rows64.drop_weight_entry(W))[0], kind="bf16",
                              log=logs.append)
    # a 2^-8 relative bias (a defect of that size in a shared helper) is seen in bf16 outputs
    assert not rows64.check("biased", torch.from_numpy(rows64.bf16_round((got * (1 - 2 ** -8)).numpy())), ref, bound, "bf16").ok
    # weight gradient: one dY row dropped
    dY = torch.from_numpy(rows64.bf16_round(torch.randn(R, Cout, generator=g).numpy()))
    dW, SW = rows64.conv_rows_wgrad(X, dY, taps)
    gotw = torch.stack([dY.float().T @ rows64.shift_rows(X, t - taps // 2).float() for t in range(taps)]).double()
    rows64.check_with_control("wgrad", gotw, dW, rows64.gamma(R) * SW, rows64.conv_rows_wgrad(X, rows64.drop_row(dY, 7), taps)[0],
                              log=logs.append)
    assert len(logs) == 4
    # an error just above the bound fails, one at it passes
    e = rows64.check("edge", ref + 1.01 * (bound + rows64.RHO["f32"] * ref.abs()), ref, bound)
    assert e.worst > 1.0 and not e.ok


def test_weightnorm_backward_restatement():
    torch.manual_seed(0)
    Cout, Cin, taps = 8, 6, 3
    v = torch.randn(Cout, Cin, taps, dtype=torch.float64, requires_grad=True)
    gg = (torch.rand(Cout, 1, 1, dtype=torch.float64) + 0.5).requires_grad_(True)
    w = gg * v / v.reshape(Cout, -1).norm(dim=1).reshape(Cout, 1, 1)
    dWc = torch.randn(Cout, Cin, taps, dtype=torch.float64)
    w.backward(dWc)
    inv = 1.0 / v.detach().reshape(Cout, -1).norm(dim=1)
    dv, dg, bdv, bdg = rows64.weightnorm_bwd(dWc.permute(2, 0, 1), dWc.abs().permute(2, 0, 1), 10, v.detach(), gg.detach(), inv)
    assert torch.allclose(dv, v.grad, rtol=1e-12, atol=1e-12)
    assert torch.allclose(dg, gg.grad.reshape(-1), rtol=1e-12, atol=1e-12)
    assert bool((bdv > 0).all()) and bool((bdg > 0).all())
