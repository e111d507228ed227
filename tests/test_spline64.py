"""CPU tests of oracle/spline64.py, the float64 restatement tests/test_predictor_rows_fp64_gpu.py holds the ConvFlow, spline and
likelihood row kernels to: it reproduces the golden's wide-parameter spline arrays (recorded from the reference's own transform) and
the ElementwiseAffine arrays to 1e-5 of max-abs, its spline gradients pass gradcheck in bin 0, bin 9 and a tail, and its rows-layout
operators agree with the [B, C, T] oracle (oracle/glowtts_ref.py) on a two-utterance layout with halo rows."""
import math
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "golden"))
from fill import filled_state  # noqa: E402
import shards  # noqa: E402
from oracle import glowtts_ref as R  # noqa: E402
from oracle import spline64 as S  # noqa: E402

G = shards.load(os.path.join(os.path.dirname(__file__), "golden", "float_golden"))
C = 192
F64 = torch.float64


def t(name):
    return torch.from_numpy(G[name])


def close(got, want, tol=1e-5):
    want = want.double()
    err = float((got.double() - want).abs().max())
    return err <= tol * float(want.abs().max()), err


def golden_rows():
    """the golden's [2, 1, 23] spline arrays as 46 rows, every row its own utterance (its log|det| has a cotangent of its own)"""
    n = t("sp_in").numel()
    par = torch.zeros(n, S.PW, dtype=F64)
    par[:, :10] = t("sp_uw").reshape(n, 10).double() * math.sqrt(C)
    par[:, 10:20] = t("sp_uh").reshape(n, 10).double() * math.sqrt(C)
    par[:, 20:29] = t("sp_ud").reshape(n, 9).double()
    z = torch.stack([torch.zeros(n), t("sp_in").reshape(n)], 1)
    return n, par, z, torch.ones(n), torch.arange(n)


def test_float64_reproduces_the_golden_spline():
    n, par, z, mk, utt = golden_rows()
    z_out, acc, info = S.convflow_spline_fwd(par, z, mk, utt, torch.zeros(n), 1.0, 0)
    assert info.inside.any() and (~info.inside).any()
    for got, name in ((z_out[:, 1], "sp_out"), (acc, "sp_lad")):
        ok, err = close(got, t(name).reshape(n))
        assert ok, (name, err)
    gy = torch.randn(t("sp_out").shape, generator=torch.Generator().manual_seed(22)).reshape(n)
    gl = torch.randn(t("sp_lad").shape, generator=torch.Generator().manual_seed(23)).reshape(n)
    h, Wp = torch.zeros(n, C), torch.zeros(S.NPAR, C)
    _, _, _, dz_in, gp = S.convflow_spline_bwd(h, Wp, par, z, torch.stack([torch.zeros(n), gy], 1), gl, mk, utt, torch.zeros(S.NPAR, C),
                                               torch.zeros(S.NPAR), 1.0, 0)
    s = math.sqrt(C)
    for got, name in ((dz_in[:, 1], "sp_gin"), (gp[:, :10] * s, "sp_guw"), (gp[:, 10:20] * s, "sp_guh"), (gp[:, 20:29], "sp_gud")):
        ok, err = close(got, t(name).reshape(got.shape))
        assert ok, (name, err)
    assert float(gp[:, 29:].abs().max()) == 0


def test_float64_reproduces_the_golden_inverse():
    """sp_inv is the golden's round trip: the reference's float32 inverse of its own float32 forward output.  The float64 run of that
    recipe, the inverse of the float64 forward output of sp_in, reproduces it to 1e-5 of max-abs (measured 1.34e-5 against 7.15e-5).
    Feeding the float64 inverse the golden's fp32-ROUNDED sp_out instead does not test the operator: at row 17 (bin 5, dy/dx = 0.006) one
    fp32 ulp of y moves x by 4.0e-5, and that run differs from sp_inv by 1.32e-4 through the golden's own rounding.  On the golden's
    sp_out the inverse is therefore judged as the GPU test judges it: by its residual, and by the float32 run, which is the same
    arithmetic as the golden's and reproduces it."""
    n, par, z, mk, utt = golden_rows()
    want = t("sp_inv").reshape(n).double()
    y64, _, _ = S.convflow_spline_fwd(par, z, mk, utt, torch.zeros(n), 1.0, 0)
    x, info = S.convflow_spline_inv(par, y64, mk)
    assert info.inside.any() and (~info.inside).any()
    ok, worst = close(x[:, 1], want)
    assert ok, ("sp_inv", worst)
    assert torch.equal(x[~info.inside][:, 1], want[~info.inside])
    # on the golden's own fp32 output
    zi = torch.stack([torch.zeros(n), t("sp_out").reshape(n)], 1)
    x, info = S.convflow_spline_inv(par, zi, mk)
    assert torch.equal(x[~info.inside][:, 1], want[~info.inside])
    assert float(S.inv_residual(par, x[:, 1], zi[:, 1]).max()) < 1e-12
    assert float(S.inv_residual(par, want, zi[:, 1]).max()) <= 1e-5 * float(zi[:, 1].abs().max())
    x32, _ = S.convflow_spline_inv(par, zi, mk, dtype=torch.float32)
    assert close(x32[:, 1], want)[0]


def _rows_of(x, Tp, lens):
    """[B, c, T] -> rows [B Tp, c]: utterance b's frames behind a 2-row halo"""
    B, c, _ = x.shape
    out = torch.zeros(B * Tp, c, dtype=x.dtype)
    for b, n in enumerate(lens):
        out[b * Tp + 2: b * Tp + 2 + n] = x[b, :, :n].T
    return out


def test_float64_reproduces_the_golden_elementwise_affine():
    P = filled_state({"log_scale": (2, 1), "translation": (2, 1)}, "ea.")
    mask = t("f1_mask")
    lens = [int(v) for v in mask.sum((1, 2))]
    Tp = mask.shape[2] + 4
    utt = torch.arange(2).repeat_interleave(Tp)
    y, acc = S.ea_fwd(_rows_of(t("ea_x"), Tp, lens), P["ea.log_scale"], P["ea.translation"], _rows_of(mask, Tp, lens)[:, 0], utt, torch.zeros(2), 1.0, 0)
    ok, err = close(y, _rows_of(t("ea_out"), Tp, lens))
    assert ok, err
    ok, err = close(acc, t("ea_logdet"))
    assert ok, err


def test_spline_gradients_pass_gradcheck_in_bin_0_bin_9_and_a_tail():
    g = torch.Generator().manual_seed(5)
    par = F.pad(torch.randn(3, S.NPAR, generator=g, dtype=F64) * torch.tensor([math.sqrt(C)] * 20 + [1.0] * 9, dtype=F64), (0, 3))
    z = torch.tensor([[0.3, -4.9], [-0.2, 4.9], [0.1, 5.5]], dtype=F64)
    mk, utt = torch.ones(3, dtype=F64), torch.tensor([0, 0, 1])
    _, _, info = S.convflow_spline_fwd(par, z, mk, utt, torch.zeros(2), -1.0, 1)
    assert info.bin.tolist() == [0, 9, S.NB] and info.inside.tolist() == [True, True, False]
    assert float(info.knot_dist[:2].min()) > 1e-3            # finite differences stay inside one bin

    def f(p, zz):
        return S._spline_fwd(p, zz, mk, utt, torch.zeros(2, dtype=F64), -1.0, 1, C, None)[:2]
    assert torch.autograd.gradcheck(f, (par.clone().requires_grad_(True), z.clone().requires_grad_(True)), eps=1e-6, atol=1e-7, rtol=1e-5)


def test_rows_operators_agree_with_the_bct_oracle():
    g = torch.Generator().manual_seed(9)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=F64)             # noqa: E731
    B, T, lens = 2, 9, [9, 5]
    Tp = T + 4
    mask = (torch.arange(T)[None, :] < torch.tensor(lens)[:, None]).double()[:, None]
    mk, utt = _rows_of(mask, Tp, lens)[:, 0], torch.arange(B).repeat_interleave(Tp)
    assert mk[:2].sum() == 0 and mk[Tp - 2: Tp + 2].sum() == 0          # halo rows at the border between the two utterances
    rows = lambda x: _rows_of(x, Tp, lens)                               # noqa: E731
    same = lambda a, b: float((a - b).abs().max()) <= 1e-12 * max(1.0, float(b.abs().max()))   # noqa: E731
    # ConvFlow: pre, proj + spline in both directions
    z, gcond, hh = rn(B, 2, T) * 3 * mask, rn(B, C, T), rn(B, C, T)
    w_pre, b_pre, Wp, bp = rn(C, 1, 1), rn(C), rn(S.NPAR, C, 1) * 0.1, rn(S.NPAR)
    x0 = (F.conv1d(z[:, :1], w_pre, b_pre) + gcond) * mask
    assert same(S.convflow_pre_fwd(rows(z)[:, 0], w_pre, b_pre, rows(gcond), None, mk), rows(x0))
    p = F.conv1d(hh, Wp, bp) * mask
    p = p.reshape(B, 1, -1, T).permute(0, 1, 3, 2)
    uw, uh, ud = p[..., :10] / math.sqrt(C), p[..., 10:20] / math.sqrt(C), p[..., 20:]
    y, lad = R.rq_spline_fwd(z[:, 1:], uw, uh, ud)
    par, _ = S.proj_params(rows(hh), Wp, bp, mk)
    acc0 = rn(B)
    z_out, acc, info = S.convflow_spline_fwd(par, rows(z), mk, utt, acc0, -1.0, 1)
    assert same(z_out, rows(torch.flip(torch.cat([z[:, :1], y], 1) * mask, [1])))
    assert same(acc, acc0 - torch.sum(lad * mask, [1, 2]))
    zi, _ = S.convflow_spline_inv(par, rows(z), mk)
    assert same(zi, rows(torch.cat([z[:, :1], R.rq_spline_inv(z[:, 1:], uw, uh, ud)], 1) * mask))
    assert float(S.inv_residual(par, zi[:, 1], rows(z)[:, 1])[info.inside & (mk != 0)].max()) < 1e-9
    # ElementwiseAffine, both directions
    P = {"ea.log_scale": rn(2, 1) * 0.5, "ea.translation": rn(2, 1)}
    ye, ld = R.elementwise_affine(P, "ea.", z, mask)
    yr, ar = S.ea_fwd(rows(z), P["ea.log_scale"], P["ea.translation"], mk, utt, acc0, 1.0, 0)
    assert same(yr, rows(ye)) and same(ar, acc0 + ld)
    xr, none = S.ea_fwd(yr, P["ea.log_scale"], P["ea.translation"], mk, utt, None, 1.0, 1)
    assert none is None and same(xr, rows(R.elementwise_affine(P, "ea.", ye, mask, reverse=True))) and float((xr - rows(z)).abs().max()) < 1e-12
    # the middle of the duration predictor (oracle.glowtts_ref.sdp_fwd: models.py:299-311) and the Gaussian likelihood (:321)
    w, e_q = torch.randint(0, 4, (B, 1, T), generator=g).double() * mask, rn(B, 2, T) * mask
    z_u, z_v = z[:, :1], z[:, 1:]
    z0 = (w - torch.sigmoid(z_u) * mask) * mask
    logdet_q = torch.sum((F.logsigmoid(z_u) + F.logsigmoid(-z_u)) * mask, [1, 2])
    nll_post = torch.sum(-0.5 * (math.log(2 * math.pi) + e_q ** 2) * mask, [1, 2]) - logdet_q
    z0 = torch.log(torch.clamp_min(z0, 1e-5)) * mask
    zm, am = S.sdp_mid_fwd(rows(z), rows(w)[:, 0], rows(e_q), mk, utt, acc0)
    assert same(zm, rows(torch.cat([z0, z_v], 1))) and same(am, acc0 + nll_post + torch.sum(z0, [1, 2]))
    assert (rows(w)[:, 0] == 0)[mk != 0].any()                                                        # the clamp is reached
    assert same(S.nll_gauss_fwd(rows(z), mk, utt, acc0), acc0 + torch.sum(0.5 * (math.log(2 * math.pi) + z ** 2) * mask, [1, 2]))


def test_float32_twin_and_planted_defects_differ_from_float64():
    """the fp32 twin is a different arithmetic (its error is not zero) and every planted defect moves what it is meant to move"""
    n, par, z, mk, utt = golden_rows()
    a64 = S.convflow_spline_fwd(par, z, mk, utt, torch.zeros(n), 1.0, 0)[1]
    a32 = S.convflow_spline_fwd(par, z, mk, utt, torch.zeros(n), 1.0, 0, dtype=torch.float32)[1]
    assert a32.dtype == torch.float32 and 0 < float((a32.double() - a64).norm() / a64.norm()) < 1e-4
    bad = S.convflow_spline_fwd(par, z, mk, utt, torch.zeros(n), 1.0, 0, defect="no_2_over_delta")[1]
    assert float((bad - a64).norm() / a64.norm()) > 0.1
    bad = S.convflow_spline_fwd(par, z, mk, utt, torch.zeros(n), 1.0, 0, defect="end_der_free")[1]
    assert float((bad - a64).norm() / a64.norm()) > 1e-3
    args = (torch.zeros(n, C), torch.zeros(S.NPAR, C), par, z, torch.ones(n, 2), torch.ones(n), mk, utt, torch.zeros(S.NPAR, C), torch.zeros(S.NPAR), 1.0, 0)
    gp, bad = S.convflow_spline_bwd(*args)[4], S.convflow_spline_bwd(*args, defect="far_bins_forgotten")[4]
    assert float((bad - gp).norm() / gp.norm()) > 1e-2
    u2 = S.credit_neighbour(torch.tensor([0, 0, 0, 1, 1, 1, 2]), torch.tensor([0., 1, 1, 0, 1, 1, 1]))
    assert u2.tolist() == [0, 0, 0, 1, 0, 1, 1]
