"""CPU tests of oracle/conv64.py, the float64 restatement tests/test_conv_gemm_fp64_gpu.py holds gt_conv_gemm_bf16 to: pinned to torch
float64 conv1d + autograd, to oracle/glowtts_ref.py (the gate, the FFN's relu -> dropout with an injected mask) and to the packer's
index formulas; its float32 twin must pass every bound and every planted defect must miss by >= CONTROL_MISS at exactly the shapes
the device test uses (oracle/conv_cases.py); the ReLU-ambiguity cap is checked here for every case."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import conv64 as C64
from oracle import conv_cases as CC
from oracle import dropmask as DM
from oracle import glowtts_ref as GR
from oracle import rows64 as R64

F64 = torch.float64
HALO = CC.HALO


def rows_of(x):
    """[1, C, T] -> rows [T + 2 HALO, C] with zero halos"""
    return F.pad(x[0].T, (0, 0, HALO, HALO))


def close(a, b, tol=1e-12):
    assert a.shape == b.shape
    assert float((a - b).abs().max()) <= tol * max(1.0, float(b.abs().max())), float((a - b).abs().max())


# ----------------------------------------------------------------------------- torch float64 conv1d + autograd
@pytest.mark.parametrize("Cin,N,k", [(8, 4, 1), (80, 12, 3), (24, 40, 5)])
def test_forward_and_data_gradient_equal_torch_float64(Cin, N, k):
    g = torch.Generator().manual_seed(Cin + N + k)
    T = 37
    x = torch.randn(1, Cin, T, generator=g, dtype=F64).requires_grad_(True)
    w = torch.randn(N, Cin, k, generator=g, dtype=F64)
    b = torch.randn(N, generator=g, dtype=F64)
    y = F.conv1d(x, w, b, padding=k // 2)
    W = w.permute(2, 0, 1).contiguous()                                             # [taps][N][Cin]
    for edge in ("zero", "clamp"):                                                  # zero halo rows: the two forms agree
        refs, _ = C64.run(dict(X=rows_of(x.detach()), W=W, bias=b, out="f32", edge=edge))
        close(refs["y"][0][HALO:-HALO], y[0].T.detach())
    dy = torch.randn(1, N, T, generator=g, dtype=F64)
    y.backward(dy)
    refs, _ = C64.run(dict(X=rows_of(dy), W=R64.conv_rows_dgrad_weights(W), out="f32"))
    close(refs["y"][0][HALO:-HALO], x.grad[0].T)


def test_clamped_end_rows_differ_from_zero_rows_only_in_the_first_and_last_half_kernel():
    g = torch.Generator().manual_seed(1)
    X = torch.randn(23, 16, generator=g, dtype=F64)                                 # non-zero end rows
    for k in (3, 5):
        W = torch.randn(k, 8, 16, generator=g, dtype=F64)
        z, c = C64.acc(X, W, "zero")[0], C64.acc(X, W, "clamp")[0]
        assert torch.equal(z[k // 2:-(k // 2)], c[k // 2:-(k // 2)])
        assert bool((z[:k // 2] != c[:k // 2]).any()) and bool((z[-(k // 2):] != c[-(k // 2):]).any())
        ref = sum(X[min(max(0 + t - k // 2, 0), 22)] @ W[t].T for t in range(k))      # row 0 by hand
        close(c[0], ref)


def test_row_utt_is_the_kernels_binary_search():
    row0 = [0, 5, 5 + 9, 30, 64, 70]
    B = 5

    def gt_row_batch(m):
        lo, hi = 0, B - 1
        while lo < hi:
            mid = (lo + hi + 1) >> 1
            lo, hi = (mid, hi) if row0[mid] <= m else (lo, mid - 1)
        return lo
    assert list(C64.row_utt(70, B, row0=row0)) == [gt_row_batch(m) for m in range(70)]
    assert list(C64.row_utt(26, 2, Tp=13)) == [m // 13 for m in range(26)]
    assert list(C64.row_utt(7, 0)) == list(range(7))


# ----------------------------------------------------------------------------- oracle/glowtts_ref.py
def test_gate_equals_the_reference_gate_with_an_injected_mask():
    g = torch.Generator().manual_seed(2)
    H, C, T, k, p = 64, 24, 29, 5, 0.25
    x = torch.randn(1, C, T, generator=g, dtype=F64)
    P = {"c.weight": torch.randn(2 * H, C, k, generator=g, dtype=F64) / 8, "c.bias": torch.randn(2 * H, generator=g, dtype=F64)}
    cond = torch.randn(1, 2 * H, generator=g, dtype=F64)
    R = T + 2 * HALO
    keep = DM.drop_keep_gate(77, np.arange(R)[:, None], np.arange(H)[None, :], DM.thresh16(p))
    scale = float(DM.scale(p))
    mask = torch.from_numpy(np.concatenate(keep, 1)[HALO:-HALO].T.copy()).to(F64)[None] * scale       # [1, 2H, T]
    x_in = GR._drop({"d": mask}, "d", GR.conv1d(P, "c", x, padding=k // 2))
    want = GR.gate(x_in, cond[:, :, None].expand(-1, -1, T), H)
    refs, _ = C64.run(dict(X=rows_of(x), W=P["c.weight"].permute(2, 0, 1), bias=P["c.bias"], cond=cond, utt=np.zeros(R, dtype=np.int64),
                           gate=1, keep=keep, scale=scale))
    close(refs["y"][0][HALO:-HALO], want[0].T)
    close(refs["t"][0][HALO:-HALO], torch.tanh((x_in + cond[:, :, None])[0, :H]).T)
    close(refs["s"][0][HALO:-HALO], torch.sigmoid((x_in + cond[:, :, None])[0, H:]).T)


def test_ffn_relu_then_dropout_equals_the_reference_ffn():
    g = torch.Generator().manual_seed(3)
    C, Fc, T, L, k, p = 16, 40, 31, 26, 3, 0.1
    x = torch.randn(1, C, T, generator=g, dtype=F64)
    x_mask = (torch.arange(T) < L).to(F64)[None, None]
    P = {"f.conv_1.weight": torch.randn(Fc, C, k, generator=g, dtype=F64) / 4, "f.conv_1.bias": torch.randn(Fc, generator=g, dtype=F64),
         "f.conv_2.weight": torch.randn(C, Fc, k, generator=g, dtype=F64) / 6, "f.conv_2.bias": torch.randn(C, generator=g, dtype=F64)}
    R = T + 2 * HALO
    keep = DM.drop_keep(5, np.arange(R)[:, None], np.arange(Fc)[None, :], DM.thresh32(p))
    scale = float(DM.scale(p))
    mask = torch.from_numpy(keep[HALO:-HALO].T.copy()).to(F64)[None] * scale
    want = GR.ffn_fwd(P, "f.", x, x_mask, k, drop={"f.drop:0": mask})
    rm = F.pad(x_mask[0, 0], (HALO, HALO))
    y1, _ = C64.run(dict(X=rows_of(x * x_mask), W=P["f.conv_1.weight"].permute(2, 0, 1), bias=P["f.conv_1.bias"], relu=True, keep=keep,
                         scale=scale, rowmask=rm, out="f32"))
    y2, _ = C64.run(dict(X=y1["y"][0], W=P["f.conv_2.weight"].permute(2, 0, 1), bias=P["f.conv_2.bias"], rowmask=rm, out="f32"))
    close(y2["y"][0][HALO:-HALO], want[0].T)


def test_gate_backward_and_relu_dropout_backward_equal_autograd():
    g = torch.Generator().manual_seed(4)
    R, N, K = 19, 8, 16
    X = torch.randn(R, K, generator=g, dtype=F64)
    W = torch.randn(1, N, K, generator=g, dtype=F64)
    add = torch.randn(R, N, generator=g, dtype=F64)
    pre = torch.randn(R, 2 * N, generator=g, dtype=F64).requires_grad_(True)
    T, S = torch.tanh(pre[:, :N]), torch.sigmoid(pre[:, N:])
    d = X @ W[0].T + add
    (T * S).backward(d)
    refs, _ = C64.run(dict(X=X, W=W, addend=add, gate=2, T=T.detach(), S=S.detach()))
    close(refs["y"][0], pre.grad)
    ys = R64.f2bf(np.maximum(np.random.default_rng(0).standard_normal((R, N)), 0).astype(np.float32))
    ys[0, :] = 0x8000                                                                # -0 is a zero
    refs, _ = C64.run(dict(X=X, W=W, addend=add, gate=3, ysaved=ys, scale=1.25))
    close(refs["y"][0], torch.where(torch.from_numpy(R64.bf2f(ys) != 0), d * 1.25, torch.zeros_like(d)))
    assert bool((refs["y"][0][0] == 0).all())


# ----------------------------------------------------------------------------- the packer's index formulas
@pytest.mark.parametrize("flags", [0, 1, 6, 16])
def test_images_round_trip_through_the_decoders(flags):
    g = np.random.default_rng(flags)
    taps, Cout, Cin = 3, 128, 80
    W = R64.bf16_round(g.standard_normal((taps, Cout, Cin)).astype(np.float32))
    Np, Kp = CC.np_of(Cout, bool(flags & 17)), CC.kp_of(Cin)
    img = R64.pack_image_np(W, Np, Kp, flags)
    assert np.array_equal(R64.decode_fwd(img, Cout, Cin, taps, Np, Kp, flags).numpy(), W)
    assert int((img != 0).sum()) <= W.size                                           # the padding stays zero
    Npd, Kpd = CC.np_of(Cin), CC.kp_of(Cout)
    imgd = R64.pack_image_np(W, Npd, Kpd, flags, dgrad=True)
    assert np.array_equal(R64.decode_dgrad(imgd, Cout, Cin, taps, Npd, Kpd, flags).numpy(), W)


def test_split_images_hold_hi_lo_hi_along_the_reduction_axis():
    """flag 8: the image a bf16x3 GEMM reads is a plain image of [w_hi | w_lo | w_hi]; conv_cases.host_weights builds it.
    rows64.pack_image_np has no flag-8 path, so the round trip here packs the already concatenated weights with flag 0; that the
    device packer's flag 8 writes exactly this image is pinned on the GPU by tests/test_pack_images_gpu.py."""
    c = CC.BY_NAME["epi x3 fwd 64x64"]
    raw = CC.operands(c)
    W = CC.host_weights(c, raw)                                                      # [1][N][3 Cin]
    ci = c["Cin"] // 3
    v = torch.from_numpy(raw["v"][:, :, 0]).double()
    assert torch.equal(W[0, :, :ci], W[0, :, 2 * ci:]) and torch.equal(W[0, :, :ci], torch.from_numpy(R64.bf16_round(raw["v"][:, :, 0])))
    assert float((W[0, :, :ci] + W[0, :, ci:2 * ci] - v).abs().max()) <= 2.0 ** -16 * float(v.abs().max())
    img = R64.pack_image_np(W.numpy(), CC.np_of(c["N"]), CC.kp_of(c["Cin"]), 0)
    assert torch.equal(R64.decode_fwd(img, c["N"], c["Cin"], 1, CC.np_of(c["N"]), CC.kp_of(c["Cin"]), 0), W)
    cd = CC.BY_NAME["epi x3 dgrad 64x64"]
    rawd = CC.operands(cd)
    Wd = CC.host_weights(cd, rawd)                                                   # [1][N][3 Cout]
    co = cd["Cin"] // 3
    assert torch.equal(Wd[0, :, :co], torch.from_numpy(R64.bf16_round(rawd["v"][:, :, 0])).T.contiguous())


# ----------------------------------------------------------------------------- the device test's cases, on the float32 twin
KEYS = sorted({c["key"] for c in CC.CASES})
FIRST = {k: next(c for c in CC.CASES if c["key"] == k) for k in KEYS}


@pytest.mark.parametrize("key", KEYS)
def test_twin_passes_and_every_planted_defect_is_seen(key):
    """at the device test's own shapes: the float32 twin is inside every bound, every planted defect misses by >= CONTROL_MISS, and
    the float64 reference alone keeps the ReLU-ambiguous share under the cap (conv64.rule asserts all three)"""
    c = FIRST[key]
    raw = CC.operands(c)
    op = CC.op_of(c, raw, CC.host_weights(c, raw))
    refs, amb, bads = C64.references(op, c["defects"], c["bm"])
    assert set(bads) == set(c["defects"]) and len(bads) >= 1
    twin, _ = C64.run(op, torch.float32)
    C64.rule(c["name"], op, twin, refs, amb, bads)


ROW_CASES = [k for k in KEYS if {"row_above", "row_below"} & set(FIRST[k]["defects"])]


@pytest.mark.parametrize("key", ROW_CASES)
def test_row_defects_zero_the_tile_edge_row_and_only_the_other_tile_shows_it(key):
    """row_above zeroes exactly row m0 - 1 (m0 = 2 bm), row_below exactly row m0 + bm = 2 bm of the tile [bm, 2 bm); the row holds
    data, an output row of the OTHER tile reads it through the taps, and the planted reference differs from the true one in that
    other tile only — on the float32 twin it is missed by >= CONTROL_MISS through those rows alone"""
    c = FIRST[key]
    bm, k2 = c["bm"], c["taps"] // 2
    assert k2 >= 1 and c["R"] > 2 * bm + 2
    raw = CC.operands(c)
    op = CC.op_of(c, raw, CC.host_weights(c, raw))
    refs, amb, bads = C64.references(op, c["defects"], bm)
    twin, _ = C64.run(op, torch.float32)
    X = torch.from_numpy(op["X"])
    for d in ("row_above", "row_below"):
        assert d in c["defects"]
        m = C64.edge_row(d, bm)
        assert m == (2 * bm - 1 if d == "row_above" else 2 * bm)
        Xd = C64.with_defect(op, d, bm)["X"]
        changed = torch.nonzero((Xd != X).any(1))[:, 0].tolist()
        assert changed == [m] and bool((X[m] != 0).any()) and not bool((Xd[m] != 0).any())
        other = slice(2 * bm, None) if d == "row_above" else slice(0, 2 * bm)
        own = slice(0, 2 * bm) if d == "row_above" else slice(2 * bm, None)
        for o, (r, b) in refs.items():
            bad = bads[d][o][0]
            assert torch.equal(bad[own], r[own])
            rows = torch.nonzero((bad[other] != r[other]).any(1))[:, 0] + (other.start or 0)
            want = list(range(2 * bm, 2 * bm + k2)) if d == "row_above" else list(range(2 * bm - k2, 2 * bm))
            assert rows.tolist() == want, (d, o, rows.tolist())
            kind = C64.kinds(op)[o]
            miss = R64.check(f"{key} {o} [{d}, other tile]", R64.t64(twin[o])[other], bad[other], b[other], kind).miss
            assert miss >= R64.CONTROL_MISS, (d, o, miss)
    # every tile that runs these operands has a tile edge at 2 bm
    for cc in CC.CASES:
        if cc["key"] == key:
            assert (2 * bm) % CC.TILE_BM[cc["tile"]] == 0 or cc["tile"] == CC.AUTO


def test_case_table_covers_what_the_kernel_can_take():
    names = [c["name"] for c in CC.CASES]
    assert len(set(names)) == len(names)
    assert {c["N"] for c in CC.CASES} >= {4, 8, 12, 80, 160, 192, 576, 768}
    assert {c["Cin"] for c in CC.CASES} >= {8, 80, 192, 768}
    for tile in (CC.T64x64, CC.T64x128, CC.T128x64, CC.T128x128, CC.T256x64, CC.TAPS):
        bm = CC.TILE_BM[tile]
        assert {c["R"] for c in CC.CASES if c["tile"] == tile} >= {bm - 1, bm, bm + 1, 8 * bm + 1, 5}, tile
    assert {c["taps"] for c in CC.CASES if c["tile"] == CC.TAPS} == {1, 3, 5}
    assert {(c["gate"], c["tile"]) for c in CC.CASES if c["gate"] == 1} == {(1, CC.T64x128), (1, CC.T128x128), (1, CC.T256x64)}
    # GT_TILE_AUTO's threshold, from the code's formula: 256 workgroups of 128 rows
    assert CC.auto_threshold_rows(192) == 85 * 128 and CC.auto_threshold_rows(768) == 42 * 128
    for Np in (192, 768):
        bn = 128 if Np % 128 == 0 else 64
        r = CC.auto_threshold_rows(Np)
        assert -(-r // 128) * (Np // bn) <= 256 < -(-(r + 1) // 128) * (Np // bn)
        assert -(-r // 64) * (Np // 64) <= 1024                                       # the all-taps threshold never binds first
    # ragged layouts: an utterance of one frame, one that ends on the first tile edge, every utterance at least one frame
    for R, bm in [(129, 64), (513, 64), (1025, 128), (2049, 256), (193, 64)]:
        row0 = CC.layout(R, bm)
        assert row0[0] == 0 and row0[-1] == R and row0[1] == 5 and bm in row0 and min(np.diff(row0)) >= 5
    assert CC.layout(5, 64) == [0, 5]
