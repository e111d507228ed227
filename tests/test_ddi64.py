"""oracle/ddi64.py (the float64 restatement tests/test_actnorm_ddi_fp64_gpu.py holds gt_actnorm_ddi to) pinned to the reference's own
ActNorm.initialize through the committed fixtures (float_golden's ddi_y / ddi_mask -> ddi_logs0 / ddi_bias0), its float32 twin held to
its own bound on every case of the GPU test, every planted defect shown to leave that bound, and the condition on the cases' inputs
(every channel's V exactly 0 or >= 1e-2).  No GPU."""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "golden"))
import shards  # noqa: E402
from oracle import ddi64 as D  # noqa: E402
from oracle import glowtts_ref as R  # noqa: E402
from oracle.rows64 import CONTROL_MISS  # noqa: E402

G = shards.load(os.path.join(os.path.dirname(__file__), "golden", "float_golden"))


def test_restatement_reproduces_the_reference_fixture():
    """The fixture is the reference's fp32 evaluation: its two sums run over n <= 40 fp32 terms (one more rounding in x * x), so each
    is held to (n + 3) U relative to its absolute-value sum; everything behind the sums is the kernel's own chain of roundings."""
    y, mask = torch.from_numpy(G["ddi_y"]), torch.from_numpy(G["ddi_mask"])
    h, m = R.squeeze(y, mask)                                            # commons.squeeze: [3, 160, 22], [3, 1, 22]
    rows = h.permute(0, 2, 1).reshape(-1, h.shape[1]).numpy()
    valid = m.permute(0, 2, 1).reshape(-1).numpy() != 0
    n = int(valid.sum())
    assert rows.shape == (66, 160) and n == 22 + 15 + 3 and not rows[~valid].any()
    logs, bias, bl, bb = D.ddi(rows, valid, n, g=(n + 3) * D.U)
    r_logs, r_bias = D.ratio(G["ddi_logs0"].reshape(-1), logs, bl), D.ratio(G["ddi_bias0"].reshape(-1), bias, bb)
    print(f"fixture vs float64: worst err/bound logs {r_logs:.3g} bias {r_bias:.3g}; widest bound logs {bl.max():.3g} bias {bb.max():.3g}")
    assert r_logs <= 1.0 and r_bias <= 1.0
    assert bl.max() < 1e-4 and bb.max() < 1e-4                           # fp32 accuracy, not a tolerance that any number passes
    # ... and equals oracle/glowtts_ref.py's restatement in float64 to float64 accuracy
    lg, bs = R.actnorm_initialize(h.double(), m.double())
    assert np.abs(lg.reshape(-1).numpy() - logs).max() < 1e-13 and np.abs(bs.reshape(-1).numpy() - bias).max() < 1e-13


@pytest.mark.parametrize("name", list(D.CASES))
def test_condition_on_the_inputs(name):
    """Every channel of every case: V exactly 0 (the constant 0.5, whose expected values are closed forms) or V >= 1e-2; the layout
    leaves zeros in every invalid row and exercises what its name says."""
    x, lay, n = D.case(name)
    lens, T, ragged, rnd, C = D.CASES[name]
    assert x.dtype == np.float32 and x.shape == (lay.R, C) and n == sum(lens) and not x[~lay.valid].any() and n < lay.R
    V, exact = D.condition(x, lay.valid, n)
    const = [c for c, s in D.special_channels(C).items() if isinstance(s, float)]
    assert np.nonzero(exact)[0].tolist() == const and (V[~exact] >= D.V_MIN).all() and (V[exact] == 0).all()
    logs, bias, bl, bb = D.ddi(x, lay.valid, n)
    for c in const:
        want = -0.5 * math.log(1e-6)                                     # two float64 libraries: a few float64 ulps
        assert abs(logs[c] - want) <= 4e-16 * want and abs(bias[c] + 0.5 * math.exp(want)) <= 4e-16 * 0.5 * math.exp(want) * 8
    assert np.isfinite(bl).all() and np.isfinite(bb).all() and (bl > 0).all() and (bb > 0).all()
    # the cancelling channel's bound is wide because its error is: 100x the bound of a noise channel, and still below 1e-2
    c40 = [c for c, s in D.special_channels(C).items() if s == (40.0, 0.2)][0]
    assert 1e-4 < bl[c40] < 1e-2 and (C == 2 or bl[0] < 1e-5)
    if len(lens) == 33:
        assert 1 in lens and lens[0] == lens[-1] == T and lay.R >= 5 * 64 + 1


def test_cases_cover_the_kernels_paths():
    shapes = {(len(v[0]), v[4], v[2]) for v in D.CASES.values()}
    assert {c for _, c, _ in shapes} == {2, 160, 260} and {b for b, _, _ in shapes} == {1, 33} and {r for _, _, r in shapes} == {False, True}
    Rs = sorted({D.case(k)[1].R for k in D.CASES})
    assert Rs[0] <= 64 and 65 in Rs and 64 in Rs and Rs[-1] >= 5 * 64 + 1


@pytest.mark.parametrize("name", list(D.CASES))
def test_float32_twin_stays_inside_the_bound(name):
    x, lay, n = D.case(name)
    logs, bias, bl, bb = D.ddi(x, lay.valid, n)
    tl, tb, _, _ = D.ddi(x, lay.valid, n, dtype=np.float32)
    r_logs, r_bias = D.ratio(tl, logs, bl), D.ratio(tb, bias, bb)
    print(f"{name}: twin worst err/bound logs {r_logs:.3g} bias {r_bias:.3g}")
    assert r_logs <= 1.0 and r_bias <= 1.0


@pytest.mark.parametrize("name", list(D.CASES))
def test_every_planted_defect_leaves_the_bound(name):
    """... on the float32 twin's values, as the GPU test asks of the kernel's (ddi64.compare)."""
    x, lay, n = D.case(name)
    tl, tb, _, _ = D.ddi(x, lay.valid, n, dtype=np.float32)
    defects = D.defects_for(name)
    assert set(defects) >= set(D.DEFECTS) - {"wrap256"} and (("wrap256" in defects) == (D.CASES[name][4] > 256))
    worst = D.compare(name, tl, tb, x, lay.valid, n, geom=(lay.B, lay.Tp), defects=defects)
    assert worst <= 1.0
    # the float64 values of a defect are no rounding away from the twin's values of the same defect: the defect is what is seen
    for d in defects:
        dl, db, bl, bb = D.ddi(x, lay.valid, n, defect=d, geom=(lay.B, lay.Tp))
        assert max(D.ratio(tl, dl, bl), D.ratio(tb, db, bb)) >= CONTROL_MISS, d


def test_ratio_reports_non_finite_differences():
    one = np.ones(3)
    assert D.ratio(one, one, one) == 0.0 and D.ratio(one * 2, one, one) == 1.0
    assert D.ratio(np.array([1.0, np.nan, 1.0]), one, one) == math.inf and D.ratio(one, np.array([1.0, np.inf, 1.0]), one) == math.inf
