"""The layout kernels every other GPU test's operands pass through (csrc/flow_ops.hip: gt_rows_from_bct, gt_bct_from_rows,
gt_squeeze_rows_f32, gt_unsqueeze_rows_f32, gt_rows_f32_to_bf16, gt_rows_add_bf16), bit for bit against the index-only restatements
of oracle/loss64.py (pinned to commons.squeeze / unsqueeze by tests/test_loss64.py).  Every launch runs between guards
(oracle/guards.py): outputs inside canaries and pre-filled with canaries (every element must be written, halo and rounding rows as
zero), inputs between NaN guards."""
import itertools

import numpy as np
import pytest
import torch

from oracle import loss64 as L64
from oracle import loss_cases as LC
from oracle.guards import Guards

pytestmark = pytest.mark.gpu
F32, BF16 = torch.float32, torch.bfloat16
GT_E_INVAL = -1


def dev():
    return torch.device("cuda:0")


def api():
    from glow_tts_amd import _lib
    return _lib.call, _lib.current_stream(dev()), _lib


def exact(name, got, want):
    got, want = got.detach().float().cpu().double().numpy(), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, name
    bad = int((got != want).sum())
    print(f"{name}: {got.size} elements, {bad} differ")
    assert bad == 0, name


def row0_of(G, lay):
    return None if lay.row0 is None else G.inp(torch.from_numpy(lay.row0), fill=int(lay.R))


def lens_of(G, lens):
    return G.inp(torch.tensor(lens, dtype=torch.int32), fill=0)


@pytest.mark.parametrize("C", LC.BCT_C)
@pytest.mark.parametrize("ragged", [True, False])
def test_rows_from_bct_and_bct_from_rows_are_exact(built, ragged, C):
    call, st, _ = api()
    lay = L64.Layout(LC.BCT_LENS, LC.BCT_T, ragged)
    assert lay.R % 64 != 0
    g = LC.gen(C, int(ragged), 31)
    x = torch.randn(lay.B, C, lay.T, generator=g)                                    # frames past a length hold data too: copied as they are
    rows = torch.randn(lay.R, C, generator=g)
    for src_f32, dst_f32 in itertools.product((True, False), repeat=2):
        sdt, ddt = (F32 if src_f32 else BF16), (F32 if dst_f32 else BF16)
        tag = f"ragged={ragged} C={C} {'fp32' if src_f32 else 'bf16'} -> {'fp32' if dst_f32 else 'bf16'}"
        G = Guards(dev())
        out = G.out("rows", (lay.R, C), dtype=ddt)
        call.gt_rows_from_bct(G.inp(x.to(sdt)), int(src_f32), out, int(dst_f32), row0_of(G, lay), lay.B, C, lay.T, lay.Tp, lay.R, st)
        G.verify()
        want = L64.cast(L64.rows_from_bct(x.to(sdt).double().numpy(), lay), dst_f32)
        exact("gt_rows_from_bct " + tag, out, want)
        assert (want[lay.rowframe < 0] == 0).all()
        G = Guards(dev())
        back = G.out("x", (lay.B, C, lay.T), dtype=ddt)
        rn = rows.to(sdt).clone()
        rn[~torch.from_numpy(lay.valid)] = float("nan")                              # rows past a length are not read
        call.gt_bct_from_rows(G.inp(rn), int(src_f32), back, int(dst_f32), lens_of(G, lay.lens), row0_of(G, lay), lay.B, C, lay.T, lay.Tp,
                              lay.R, st)
        G.verify()
        exact("gt_bct_from_rows " + tag, back, L64.cast(L64.bct_from_rows(rows.to(sdt).double().numpy(), lay), dst_f32))


@pytest.mark.parametrize("Ty", LC.SQZ_TY)
@pytest.mark.parametrize("C", LC.SQZ_C)
def test_squeeze_and_unsqueeze_rows_are_exact(built, C, Ty):
    call, st, _ = api()
    for ragged in (True, False):
        lay, len_sq, y, rows = LC.sqz_case(C, Ty, ragged)
        tag = f"C={C} Ty={Ty} ragged={ragged} len_sq={len_sq}"
        G = Guards(dev())
        d_len, d_row0 = lens_of(G, len_sq), row0_of(G, lay)
        sq = G.out("rows", (lay.R, 2 * C))
        call.gt_squeeze_rows_f32(G.inp(y), sq, d_len, lay.B, C, Ty, lay.Tp, d_row0, st)
        rn = rows.clone()
        rn[~torch.from_numpy(lay.valid)] = float("nan")                              # halo / padded rows are not read
        un = G.out("y", (lay.B, C, Ty))
        call.gt_unsqueeze_rows_f32(G.inp(rn), un, d_len, lay.B, C, Ty, lay.Tp, d_row0, st)
        G.verify()
        want_sq = L64.squeeze_rows(y.double().numpy(), len_sq, lay)
        want_un = L64.unsqueeze_rows(rows.double().numpy(), len_sq, lay, Ty)
        exact("gt_squeeze_rows_f32 " + tag, sq, want_sq)
        exact("gt_unsqueeze_rows_f32 " + tag, un, want_un)
        assert (want_sq[~lay.valid] == 0).all() and (Ty % 2 == 0 or (want_un[:, :, Ty - 1] == 0).all())
        # round trips, both ways: each is the other's backward
        G = Guards(dev())
        d_len, d_row0 = lens_of(G, len_sq), row0_of(G, lay)
        y2, r2 = G.out("y2", (lay.B, C, Ty)), G.out("rows2", (lay.R, 2 * C))
        call.gt_unsqueeze_rows_f32(sq, y2, d_len, lay.B, C, Ty, lay.Tp, d_row0, st)
        call.gt_squeeze_rows_f32(un, r2, d_len, lay.B, C, Ty, lay.Tp, d_row0, st)
        G.verify()
        on = (np.arange(Ty)[None, :] < 2 * np.minimum(np.asarray(len_sq), Ty // 2)[:, None])[:, None, :]
        exact("unsqueeze(squeeze(y)) " + tag, y2, y.double().numpy() * on)
        exact("squeeze(unsqueeze(rows)) " + tag, r2, rows.double().numpy() * lay.valid[:, None])


def test_squeeze_refuses_81_channels(built):
    call, st, _lib = api()
    t = torch.zeros(4096, device=dev())
    ln = torch.ones(1, dtype=torch.int32, device=dev())
    for entry in (call.gt_squeeze_rows_f32, call.gt_unsqueeze_rows_f32):
        with pytest.raises(_lib.GtError) as e:
            entry(t, t, ln, 1, 81, 8, 8, None, st)
        assert e.value.code == GT_E_INVAL


@pytest.mark.parametrize("ragged", [True, False])
def test_rows_f32_to_bf16_and_rows_add_bf16_are_exact(built, ragged):
    call, st, _ = api()
    lay = L64.Layout(LC.BCT_LENS, LC.BCT_T, ragged)
    n, ld = 80, 96
    g = LC.gen(int(ragged), 37)
    x, add, dx = torch.randn(lay.R, ld, generator=g), torch.randn(lay.R, ld, generator=g).to(BF16), torch.randn(lay.R, ld, generator=g)
    keep = (torch.arange(ld) >= n)[None, :]
    for masked in (True, False):
        G = Guards(dev())
        out = G.out("out", (lay.R, ld), dtype=BF16, keep=keep)
        call.gt_rows_f32_to_bf16(G.inp(x), ld, out, ld, G.inp(torch.from_numpy(lay.rowmask)) if masked else None, lay.R, n, st)
        G.verify()
        exact(f"gt_rows_f32_to_bf16 ragged={ragged} rowmask={'set' if masked else 'NULL'}", out[:, :n],
              L64.rows_f32_to_bf16(x.numpy(), lay.rowmask if masked else None, n))
    G = Guards(dev())
    start = dx.clone()
    start[:, n:] = 768.0
    acc = G.out("dx", (lay.R, ld), prior=start, keep=keep)
    call.gt_rows_add_bf16(acc, ld, G.inp(add), ld, lay.R, n, st)
    G.verify()
    exact(f"gt_rows_add_bf16 ragged={ragged}", acc[:, :n], L64.rows_add_bf16(dx.numpy(), add.float().numpy(), n))
