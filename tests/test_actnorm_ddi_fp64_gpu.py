"""gt_actnorm_ddi (csrc/flow_ops.hip: the stats and finish kernels of the ActNorm data-dependent initialisation) against float64 on
hand-made rows, under the bounds oracle/ddi64.py derives from the kernel's roundings; the cases, the condition on their inputs and the
planted defects are the ones tests/test_ddi64.py validates on the float32 twin.

The entry is called through _lib.call between guards (oracle/guards.py): the rows and the lengths between guards, logs / bias inside
canaries and pre-filled with canaries, the workspace pre-filled with NaN (the entry clears it).  Every element of logs and bias is
held to |got - ref| <= bound; each test prints its worst error / bound.  Then the decoder: what every block's ActNorm is handed on its
first forward is exactly zero outside the valid rows — the kernel sums ALL rows — and what it is given back is the float64
initialisation of those very rows to fp32 accuracy, block after block."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "golden"))
from fill import fill_module  # noqa: E402
from oracle import ddi64 as D  # noqa: E402
from oracle.guards import CAN, Guards  # noqa: E402

pytestmark = pytest.mark.gpu
GT_E_INVAL = -1


def dev():
    return torch.device("cuda:0")


def api():
    from glow_tts_amd import _lib
    return _lib.call, _lib.current_stream(dev()), _lib


@pytest.mark.parametrize("name", list(D.CASES))
def test_entry_against_float64(built, name):
    from glow_tts_amd import ops
    call, st, _ = api()
    x, lay, n = D.case(name)
    lens, T, ragged, rnd, C = D.CASES[name]
    assert ops.HALO == D.HALO == 2
    if ragged:                                               # the host side's own layout of these lengths
        starts, R = ops.RowsCtx.row_starts(lens, T, rnd)
        assert R == lay.R and starts == lay.row0.tolist()
    else:
        assert lay.R == len(lens) * (T + 2 * ops.HALO) and lay.base.tolist() == [b * (T + 2 * ops.HALO) for b in range(len(lens))]
    G = Guards(dev())
    logs, bias = G.out("logs", (C,)), G.out("bias", (C,))
    ws = G.out("workspace", (2 * C,), dtype=torch.float64, prior=torch.full((2 * C,), float("nan"), dtype=torch.float64))
    call.gt_actnorm_ddi(G.inp(torch.from_numpy(x)), G.inp(torch.tensor(lens, dtype=torch.int32), fill=1), len(lens), lay.R, C, ws, logs, bias, st)
    G.verify()
    D.compare(f"gt_actnorm_ddi {name}", logs.cpu().numpy(), bias.cpu().numpy(), x, lay.valid, n, geom=(lay.B, lay.Tp),
              defects=D.defects_for(name))
    # the workspace holds the two sums: fp64 sums of fp32 values, R + 1 roundings of 2^-53 at the most (and as many in numpy's sum)
    xs = x.astype(np.float64)
    w = ws.cpu().numpy()
    tol = 2 * (lay.R + 1) * D.U64
    assert (np.abs(w[:C] - xs.sum(0)) <= tol * np.abs(xs).sum(0)).all() and (np.abs(w[C:] - (xs * xs).sum(0)) <= tol * (xs * xs).sum(0)).all()


def test_entry_refuses_nulls_and_non_positive_sizes(built):
    call, st, _lib = api()
    G = Guards(dev())
    C, R, B = 8, 12, 2
    logs, bias = G.out("logs", (C,)), G.out("bias", (C,))
    x, ln, ws = torch.zeros(R, C, device=dev()), torch.tensor([4, 4], dtype=torch.int32, device=dev()), torch.zeros(2 * C, dtype=torch.float64, device=dev())
    good = dict(x=x, len=ln, B=B, R=R, C=C, ws=ws, logs=logs, bias=bias)
    order = ["x", "len", "B", "R", "C", "ws", "logs", "bias"]
    bads = [{k: None} for k in ("x", "len", "ws", "logs", "bias")] + [{k: v} for k in ("B", "R", "C") for v in (0, -1)]
    for bad in bads:
        a = dict(good, **bad)
        with pytest.raises(_lib.GtError) as e:
            call.gt_actnorm_ddi(*[a[k] for k in order], st)
        assert e.value.code == GT_E_INVAL, bad
    torch.cuda.synchronize()
    for name, buf, view, _, _ in G.outs:                     # nothing was launched: logs, bias and their guards hold the canary
        assert bool((buf == CAN).all()), name


@pytest.mark.parametrize("ragged", [False, True])
def test_decoder_hands_zero_rows_to_every_block(built, ragged, monkeypatch):
    """A 3-block decoder with set_ddi(True) on every ActNorm, one forward: every block's init sees rows that are exactly zero wherever
    rowmask is 0 (halo, padded, rounding and past-the-length rows), and writes the float64 initialisation of ITS OWN rows within the
    derived bound — blocks > 0 included, which tests/test_decoder_gpu.py can only hold to 2e-2 of the CPU oracle's."""
    from glow_tts_amd import flow_impl, models, modules, ops
    dec = fill_module(models.FlowSpecDecoder(80, 192, 5, 1, 3, 4, p_dropout=0.05), "decoder.").eval().to(dev())
    T = 44
    lens = [44, 31, 2, 18, 44]                               # full length first and last, an odd one (its last frame is dropped), 2 -> 1
    if ragged:
        dec.rows_cfg = ops.RowsConfig(ragged=True, row_round=64)
        dec.rows_cfg.host_lengths["y"] = list(lens)
    m = (torch.arange(T)[None, :] < torch.tensor(lens)[:, None]).unsqueeze(1).float()
    y = (torch.randn(len(lens), 80, T, generator=torch.Generator().manual_seed(4)) * 1.7 + 0.3) * m
    for f in dec.flows:
        if isinstance(f, modules.ActNorm):
            f.set_ddi(True)
    seen = []
    orig = flow_impl.actnorm_ddi

    def spy(rc, x, an):
        orig(rc, x, an)
        seen.append((rc, x.detach().clone(), rc.rowmask.detach().clone(), rc.lengths.detach().clone(), an.logs.detach().clone(),
                     an.bias.detach().clone()))
    monkeypatch.setattr(flow_impl, "actnorm_ddi", spy)
    with torch.no_grad():
        dec(y.to(dev()), m.to(dev()))
    torch.cuda.synchronize()
    assert len(seen) == 3
    for b, (rc, x, rowmask, lengths, logs, bias) in enumerate(seen):
        assert rc.ragged == ragged and x.dtype == torch.float32 and x.shape == (rc.R, 160) and lengths.tolist() == [v // 2 for v in lens]
        valid = (rowmask != 0).cpu().numpy()
        n = int(lengths.sum())
        assert int(valid.sum()) == n and n < rc.R
        xs = x.cpu().numpy()
        stray = np.nonzero(xs[~valid])
        assert stray[0].size == 0, (f"block {b}: {stray[0].size} non-zero elements in rows with rowmask == 0, first at row "
                                    f"{np.nonzero(~valid)[0][stray[0][0]]} channel {stray[1][0]}")
        D.condition(xs, valid, n)
        D.compare(f"decoder {'ragged' if ragged else 'uniform'} block {b}", logs.reshape(-1).cpu().numpy(), bias.reshape(-1).cpu().numpy(),
                  xs, valid, n, geom=(rc.B, rc.Tp), defects=("denom_R",))
