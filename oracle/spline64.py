"""TEST INFRASTRUCTURE ONLY — float64 restatement of the ConvFlow, spline and likelihood row kernels (the second half of
csrc/predictor_ops.hip: gt_convflow_pre_fwd/bwd, gt_convflow_spline_fwd/bwd/inv, gt_ea_fwd/bwd, gt_sdp_mid_fwd/bwd, gt_nll_gauss_fwd/bwd)
on the rows layout, for tests/test_spline64.py and tests/test_predictor_rows_fp64_gpu.py.

Every operator takes the kernel's own fp32 operands ([R, .] buffers, rowmask [R], utt [R]) and `dtype=`: at torch.float64 it is the
reference, at torch.float32 the "fp32 twin" (the same operator in torch's float32 arithmetic on the same data), whose own error against
float64 is what a kernel's error is held to.  The spline itself is oracle.glowtts_ref.rq_spline_fwd / rq_spline_inv (not restated here;
their `end_ud` / `bin_idx` keywords serve a planted defect and the check at a knot); every gradient is autograd's through the forward
operator.  Destinations the kernels ACCUMULATE into (acc, dWp, dbp, dw_pre, db_pre, dz / dg
of pre_bwd, dlog_scale, dtranslation) take the prior value and return prior + contribution; everything else is overwritten, masked
rows with zeros.

What a test needs to choose its cases comes back with the values (`SplineInfo`): the bin of every row (-1 / NB for the two tails), the
distance of the searched value to the nearest interior knot and the width of its bin (on the searched axis: widths forward, heights
inverse), `inside`, and the slope dy/dx.

Planted defects (`defect=`), for the negative controls of the GPU test:
  "no_2_over_delta"     log|det| without its 2 log(delta) term: the forward's acc moves, the backward loses 2 / delta in d/d delta
  "far_bins_forgotten"  the gradient at the raw widths / heights of bins j > k + 1 is zero: the cumulative sum reaches them only through
                        the softmax's normalisation, which such a backward forgets
  "end_der_free"        the derivative at the two end knots is min_der + softplus(0) instead of being pinned to 1
The other three (flip ignored, acc overwritten, a border row credited to the neighbouring utterance) are planted through the operands:
another `flip`, a zero prior, `credit_neighbour(utt, rowmask)`.
"""
import math
import types

import torch
import torch.nn.functional as F

from oracle import glowtts_ref as R

NB = 10
NPAR = 3 * NB - 1
PW = 32                        # width of the kernels' params buffer: 29 used, 3 zero
TAIL = 5.0
MIN_BIN = 1e-3
F64 = torch.float64


def _c(x, dtype):
    return None if x is None else torch.as_tensor(x).detach().cpu().to(dtype)


def _idx(utt):
    return torch.as_tensor(utt).detach().cpu().long()


def utt_add(prior, utt, v):
    """prior[b] + sum of v over the rows of utterance b"""
    return prior.index_add(0, _idx(utt), v)


def credit_neighbour(utt, rowmask):
    """planted defect: the first valid row of every utterance but the first one is credited to the utterance before it"""
    utt, on = _idx(utt).clone(), torch.as_tensor(rowmask).cpu() != 0
    for b in utt.unique().tolist()[1:]:
        rows = torch.nonzero((utt == b) & on)
        if rows.numel():
            utt[rows[0, 0]] = b - 1
    return utt


# ------------------------------------------------------------------------------------------------ the spline's knots and bins
def knots(u):
    """knots of one axis from its scaled raw parameters [..., NB] -> [..., NB + 1] (what rq_spline_* builds inside; here only to
    report bins and distances, and for the "no_2_over_delta" defect)"""
    w = MIN_BIN + (1 - MIN_BIN * NB) * F.softmax(u, dim=-1)
    c = F.pad(torch.cumsum(w, -1), (1, 0)) * (2 * TAIL) - TAIL
    return torch.cat([torch.full_like(c[..., :1], -TAIL), c[..., 1:-1], torch.full_like(c[..., :1], TAIL)], -1)


def _bin(x, c):
    loc = c.detach().clone()
    loc[..., -1] += 1e-6
    return (torch.sum(x.detach().clamp(-TAIL, TAIL)[..., None] >= loc, -1) - 1).clamp(0, NB - 1)


def _delta(x, uw, uh, searched_on_heights=False):
    cw, ch = knots(uw), knots(uh)
    k = _bin(x, ch if searched_on_heights else cw)[..., None]
    return ((ch[..., 1:] - ch[..., :-1]) / (cw[..., 1:] - cw[..., :-1])).gather(-1, k)[..., 0]


def spline_info(v, uw, uh, slope, inverse=False):
    """v: the searched values (forward: x on the width knots; inverse: y on the height knots)"""
    v, uw, uh = v.detach(), uw.detach(), uh.detach()
    c = knots(uh if inverse else uw)
    k = _bin(v, c)
    inside = (v >= -TAIL) & (v <= TAIL)
    return types.SimpleNamespace(
        bin=torch.where(inside, k, torch.where(v < 0, torch.full_like(k, -1), torch.full_like(k, NB))),
        knot_dist=(v[..., None] - c[..., 1:-1]).abs().min(-1).values,
        bin_width=(c[..., 1:] - c[..., :-1]).gather(-1, k[..., None])[..., 0],
        knots=c, inside=inside, slope=slope.detach())


def split_params(par, C):
    """params [R, 32] -> the spline's scaled (uw, uh, ud) (modules.py:801-803)"""
    s = 1.0 / math.sqrt(C)
    return par[:, :NB] * s, par[:, NB:2 * NB] * s, par[:, 2 * NB:NPAR]


# ------------------------------------------------------------------------------------------------ ConvFlow
def convflow_pre_fwd(z0, w_pre, b_pre, g1, g2, rowmask, dtype=F64):
    """x0 = (w_pre z0 + b_pre + g1 + g2) * mask; z0 [R] is column 0 of the kernel's z rows (ldz = 1 or 2)"""
    z0, w, b, g1, g2, mk = (_c(a, dtype) for a in (z0, w_pre, b_pre, g1, g2, rowmask))
    return _pre(z0, w.reshape(-1), b.reshape(-1), g1, g2, mk)


def _pre(z0, w, b, g1, g2, mk):
    x = z0[:, None] * w + b
    if g1 is not None:
        x = x + g1
    if g2 is not None:
        x = x + g2
    return x * mk[:, None]


def convflow_pre_bwd(dx0, z0, w_pre, rowmask, dw0, db0, dz0=None, dg0=None, dtype=F64):
    """-> (dw_pre, db_pre, dz[:, 0], dg): the priors plus autograd's gradients of sum(x0 dx0); dz0 / dg0 None: not asked for"""
    dx0, z0, w, mk, dw0, db0, dz0, dg0 = (_c(a, dtype) for a in (dx0, z0, w_pre, rowmask, dw0, db0, dz0, dg0))
    z0, w = z0.requires_grad_(True), w.reshape(-1).requires_grad_(True)
    b, g = torch.zeros_like(w, requires_grad=True), torch.zeros_like(dx0, requires_grad=True)
    gw, gb, gz, gg = torch.autograd.grad((_pre(z0, w, b, g, None, mk) * dx0).sum(), [w, b, z0, g])
    return (dw0.reshape(-1) + gw, db0.reshape(-1) + gb, None if dz0 is None else dz0 + gz, None if dg0 is None else dg0 + gg)


def proj_params(h, Wp, bp, rowmask, dtype=F64):
    """params = (Wp h + bp) * mask as [R, 32] (columns 29..31 zero), and the absolute-value twin S = |h| |Wp|^T + |bp|"""
    h, Wp, bp, mk = (_c(a, dtype) for a in (h, Wp, bp, rowmask))
    Wp, bp = Wp.reshape(NPAR, -1), bp.reshape(-1)
    par = F.pad((h @ Wp.T + bp) * mk[:, None], (0, PW - NPAR))
    return par, F.pad(h.abs() @ Wp.abs().T + bp.abs(), (0, PW - NPAR))


def across_the_knot(x, uw):
    """the bin on the other side of the interior knot nearest to x"""
    c = knots(uw.detach())
    k = _bin(x, c)
    j = (x.detach()[..., None] - c[..., 1:-1]).abs().argmin(-1) + 1
    return torch.where(k >= j, j - 1, j)


def _spline_fwd(par, z_in, mk, utt, acc0, sign, flip, C, defect, other_bin=False):
    uw, uh, ud = split_params(par, C)
    x1 = z_in[:, 1]
    y, lad = R.rq_spline_fwd(x1, uw, uh, ud, end_ud=0.0 if defect == "end_der_free" else None,
                             bin_idx=across_the_knot(x1, uw) if other_bin else None)
    if defect == "no_2_over_delta":
        inside = (x1 >= -TAIL) & (x1 <= TAIL)
        lad = torch.where(inside, lad - 2 * torch.log(_delta(x1, uw, uh)), lad)
    cols = [y, z_in[:, 0]] if flip else [z_in[:, 0], y]
    return torch.stack(cols, 1) * mk[:, None], utt_add(acc0, utt, sign * lad * mk), lad


def convflow_spline_fwd(par, z_in, rowmask, utt, acc0, sign, flip, C=192, dtype=F64, defect=None, other_bin=False):
    """z_out = [z0, RQS(z1)] * mask (columns swapped when flip), acc = acc0 + sign * sum of log|det| per utterance -> (z_out, acc, info).
    other_bin: every row is evaluated with the piece of the bin across its nearest interior knot.  The spline is C1 there, so for an x
    within an fp32 step of a knot that piece is as good an answer: an fp32 implementation's knots differ from these by such a step, and
    log|det| is only C0 at a knot (its slope y'' / y' jumps), so the two pieces differ by (jump) x (distance) a little off the knot."""
    par, z_in, mk, acc0 = (_c(a, dtype) for a in (par, z_in, rowmask, acc0))
    z_out, acc, lad = _spline_fwd(par, z_in, mk, utt, acc0, float(sign), flip, C, defect, other_bin)
    uw, uh, _ = split_params(par, C)
    inside = (z_in[:, 1] >= -TAIL) & (z_in[:, 1] <= TAIL)
    info = spline_info(z_in[:, 1], uw, uh, torch.where(inside, torch.exp(lad), torch.ones_like(lad)))
    info.lad = lad
    return z_out, acc, info


def convflow_spline_bwd(h, Wp, par, z_in, dz_out, gacc, rowmask, utt, dWp0, dbp0, sign, flip, C=192, dtype=F64, defect=None):
    """params (the buffer the forward wrote) is the leaf: gp = d/d params of sum(z_out dz_out) + sum(acc gacc) by autograd, then
    dh = gp Wp, dWp = dWp0 + gp^T h, dbp = dbp0 + sum_m gp, dz_in = [dz_out's pass-through column, d/d z1] * mask
    -> (dh, dWp, dbp, dz_in, gp [R, 32])"""
    h, Wp, par, z_in, dz_out, gacc, mk, dWp0, dbp0 = (_c(a, dtype) for a in (h, Wp, par, z_in, dz_out, gacc, rowmask, dWp0, dbp0))
    Wp = Wp.reshape(NPAR, -1)
    par, z_in = par.requires_grad_(True), z_in.requires_grad_(True)
    z_out, acc, _ = _spline_fwd(par, z_in, mk, utt, torch.zeros_like(gacc), float(sign), flip, C, defect)
    gp, dz_in = torch.autograd.grad((z_out * dz_out).sum() + (acc * gacc).sum(), [par, z_in])
    if defect == "far_bins_forgotten":
        uw, _, _ = split_params(par.detach(), C)
        far = torch.arange(NB)[None, :] > _bin(z_in.detach()[:, 1], knots(uw))[:, None] + 1
        gp = gp.clone()
        gp[:, :NB][far] = 0
        gp[:, NB:2 * NB][far] = 0
    g = gp[:, :NPAR]
    return g @ Wp, dWp0.reshape(NPAR, -1) + g.T @ h, dbp0.reshape(-1) + g.sum(0), dz_in, gp


def convflow_spline_inv(par, z_in, rowmask, C=192, dtype=F64):
    """z_out = [z0, RQS^-1(z1)] * mask -> (z_out, info); info.slope is dy/dx at the solution"""
    par, z_in, mk = (_c(a, dtype) for a in (par, z_in, rowmask))
    uw, uh, ud = split_params(par, C)
    y = z_in[:, 1]
    x = R.rq_spline_inv(y, uw, uh, ud)
    _, lad = R.rq_spline_fwd(x, uw, uh, ud)
    return torch.stack([z_in[:, 0], x], 1) * mk[:, None], spline_info(y, uw, uh, torch.exp(lad), inverse=True)


def inv_residual(par, x, y, C=192):
    """|RQS(x) - y| per row at float64, with x taken as the exact float64 value of what an inverse returned"""
    par, x, y = (_c(a, F64) for a in (par, x, y))
    uw, uh, ud = split_params(par, C)
    return (R.rq_spline_fwd(x, uw, uh, ud)[0] - y).abs()


# ------------------------------------------------------------------------------------------------ the small row operators on [R, 2]
def _ea(x, ls, tr, mk, utt, acc0, sign, reverse):
    if reverse:
        y = (x - tr) * torch.exp(-ls) * mk[:, None]
    else:
        y = (x * torch.exp(ls) + tr) * mk[:, None]
    return y, None if acc0 is None else utt_add(acc0, utt, sign * (ls[0] + ls[1]) * mk)


def ea_fwd(x, log_scale, translation, rowmask, utt, acc0, sign, reverse, dtype=F64):
    """ElementwiseAffine: y = (x exp(ls) + t) * mask, or its inverse; acc = acc0 + sign (ls_0 + ls_1) per valid row (acc0 None: no acc)"""
    x, ls, tr, mk, acc0 = (_c(a, dtype) for a in (x, log_scale, translation, rowmask, acc0))
    return _ea(x, ls.reshape(-1), tr.reshape(-1), mk, utt, acc0, float(sign), reverse)


def ea_bwd(x, log_scale, dy, gacc, rowmask, utt, dls0, dtr0, sign, dtype=F64):
    """-> (dx, dlog_scale, dtranslation): autograd through the forward direction, the priors added"""
    x, ls, dy, gacc, mk, dls0, dtr0 = (_c(a, dtype) for a in (x, log_scale, dy, gacc, rowmask, dls0, dtr0))
    x, ls = x.requires_grad_(True), ls.reshape(-1).requires_grad_(True)
    tr = torch.zeros_like(ls, requires_grad=True)
    y, acc = _ea(x, ls, tr, mk, utt, torch.zeros_like(gacc), float(sign), 0)
    dx, dls, dtr = torch.autograd.grad((y * dy).sum() + (acc * gacc).sum(), [x, ls, tr])
    return dx, dls0.reshape(-1) + dls, dtr0.reshape(-1) + dtr


def _sdp_mid(zq, w, eq, mk, utt, acc0):
    zu = zq[:, 0]
    z0l = torch.log(torch.clamp_min(w - torch.sigmoid(zu), 1e-5)) * mk
    a = -0.5 * (2 * math.log(2 * math.pi) + eq[:, 0] ** 2 + eq[:, 1] ** 2) - (F.logsigmoid(zu) + F.logsigmoid(-zu)) + z0l
    return torch.stack([z0l, zq[:, 1] * mk], 1), utt_add(acc0, utt, a * mk)


def sdp_mid_fwd(zq, w, eq, rowmask, utt, acc0, dtype=F64):
    """models.py:299-311: z = [log(max(w - sigmoid(z_u), 1e-5)), z_v] * mask, acc = acc0 + the posterior's likelihood terms"""
    zq, w, eq, mk, acc0 = (_c(a, dtype) for a in (zq, w, eq, rowmask, acc0))
    return _sdp_mid(zq, w.reshape(-1), eq, mk, utt, acc0)


def sdp_mid_bwd(zq, w, dz, gacc, rowmask, utt, dtype=F64):
    zq, w, dz, gacc, mk = (_c(a, dtype) for a in (zq, w, dz, gacc, rowmask))
    zq = zq.requires_grad_(True)
    z, acc = _sdp_mid(zq, w.reshape(-1), torch.zeros_like(zq), mk, utt, torch.zeros_like(gacc))
    return torch.autograd.grad((z * dz).sum() + (acc * gacc).sum(), [zq])[0]


def _nll(z, mk, utt, acc0):
    return utt_add(acc0, utt, 0.5 * (2 * math.log(2 * math.pi) + z[:, 0] ** 2 + z[:, 1] ** 2) * mk)


def nll_gauss_fwd(z, rowmask, utt, acc0, dtype=F64):
    z, mk, acc0 = (_c(a, dtype) for a in (z, rowmask, acc0))
    return _nll(z, mk, utt, acc0)


def nll_gauss_bwd(z, gacc, rowmask, utt, dtype=F64):
    z, gacc, mk = (_c(a, dtype) for a in (z, gacc, rowmask))
    z = z.requires_grad_(True)
    return torch.autograd.grad((_nll(z, mk, utt, torch.zeros_like(gacc)) * gacc).sum(), [z])[0]
