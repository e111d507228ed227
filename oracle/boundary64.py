"""TEST INFRASTRUCTURE ONLY — float64 restatement of the row-local chain between two WaveNets (csrc/wn_boundary.hip, and the
five-launch path's kernels in csrc/flow_ops.hip), in the style and under the rule of oracle/rows64.py:

    affine coupling (attentions.py:171-186) forward / backward / reverse, with sigmoid_scale (logs = log(1e-6 + sigmoid(raw + 2)));
    ActNorm + InvConvNear (modules.py:584-599, 635-665) forward / backward / reverse on the channel groups {2g, 2g+1, 80+2g, 80+2g+1};
    the pair's per-frame log-det (sum logs + C/4 logdet W) len[b] and gt_flow_scalars' 18 values.

Every operator works on rows [R, C] in the dtype of its arguments (float64: the reference; float32: the twin that the tests hold the
kernels to where the rule does not reach — sigmoid_scale's __logf, the 4x4 inverse) and returns its value with the bound the rule
allows the kernel, WITHOUT the output's own rounding (rows64.check adds rho_out |ref|).  The bounds are the fp32 roundings of the
kernels' formulas, written out term by term:

    U          2^-24: one fp32 rounding, relative.
    exp_rel(x) (2 + |x|) 2^-23: __expf(x) = v_exp_f32(x * log2 e).  The product is rounded once and log2 e itself is a rounded
               constant: the exponent is off by at most |x| log2 e 2^-23, the result by the factor 2^that = 1 + |x| 2^-23; the
               instruction adds one ulp (2^-23) and one more is allowed for the denormal-range scaling around it.
    gamma(K)   rows64: K fp32 products summed in any order.

A bound on an INPUT (e_*: what the previous stage of a chain may be off by) is carried through by the absolute values of the
partial derivatives.  tests/test_boundary64.py pins the operators to oracle/glowtts_ref.py in float64 and their gradients to
autograd, and runs the float32 twin against the bounds; tests/test_wn_boundary_fp64_gpu.py holds the kernels to them.
"""
import torch

from oracle.rows64 import RHO, gamma, t64

U = RHO["f32"]
F64 = torch.float64


def exp_rel(x):
    return (2.0 + x.abs()) * 2.0 ** -23


def group_index(C):
    """[C/4, 4]: the channels of group g in the order InvConvNear mixes them"""
    g = torch.arange(C // 4)
    return torch.stack([2 * g, 2 * g + 1, C // 2 + 2 * g, C // 2 + 2 * g + 1], 1)


def to_groups(X):
    return X[:, group_index(X.shape[1])]                      # [R, G, 4]


def from_groups(Xg):
    R, G, _ = Xg.shape
    out = torch.zeros(R, 4 * G, dtype=Xg.dtype)
    out[:, group_index(4 * G)] = Xg
    return out


def _z(x, like):
    return torch.zeros_like(like) if x is None else x


def scale_logs(raw, sigmoid_scale):
    """-> (logs, d logs / d raw): the identity, or log(1e-6 + sigmoid(raw + 2)) (attentions.py:172-173)"""
    if not sigmoid_scale:
        return raw, torch.ones_like(raw)
    sg = torch.sigmoid(raw + 2)
    return torch.log(1e-6 + sg), sg * (1 - sg) / (1e-6 + sg)


def fast_log_sigmoid_err(raw):
    """what the kernels' __logf(1e-6f + sigmoidf_(raw + 2)) may be off by: FAST_FN on the sigmoid (rows64) through the logarithm's
    derivative, the rounded sum (one U, as much in the logarithm), and v_log_f32 * ln 2 (an ulp of the result each, 2^-22 |logs|).
    Used only where a far wider input bound rides on the same term (the reverse chain): elsewhere sigmoid_scale goes to the twin."""
    from oracle.rows64 import FAST_FN
    sg = torch.sigmoid(raw + 2)
    return FAST_FN / (1e-6 + sg) + 2 * U + 2.0 ** -22 * torch.log(1e-6 + sg).abs()


def credit_neighbour(rowutt, mask):
    """planted defect: the first valid row of every utterance b > 0 counted for utterance b - 1"""
    ru = torch.as_tensor(rowutt).long().clone()
    valid = torch.as_tensor(mask) > 0
    for b in range(1, int(ru.max()) + 1):
        rows = torch.nonzero(valid & (ru == b))
        if len(rows):
            ru[int(rows[0])] = b - 1
    return ru


# ----------------------------------------------------------------------------- affine coupling
def coupling_fwd(out, x, mask, rowutt, B, sigmoid_scale=False, e_out=None):
    """out = [m | raw] [R, C], x = [x0 | x1] [R, C], mask [R] ->
        z = [x0 | (m + exp(logs) x1) mask], rowsum[r] = sum_c logs mask, logdet[b] = sum of its rows' rowsum.
    Returns {"z": (ref, bound), "rowsum": (ref, S), "logdet": (ref, S, n)}: S = the sum of absolute values, n[b] the addends."""
    h = out.shape[1] // 2
    m, raw, x0, x1, mk = out[:, :h], out[:, h:], x[:, :h], x[:, h:], mask[:, None]
    e_o = _z(e_out, out)
    lg, dl = scale_logs(raw, sigmoid_scale)
    e_lg = e_o[:, h:] * dl.abs()
    ex = torch.exp(lg)
    z1 = (m + ex * x1) * mk
    bz1 = (e_o[:, :h] + (ex * x1).abs() * (torch.expm1(e_lg) + exp_rel(lg) + U) + U * (m + ex * x1).abs()) * mk
    rs, rsS = (lg * mk).sum(1), (lg.abs() * mk).sum(1)
    idx = torch.as_tensor(rowutt).long()
    ld = torch.zeros(B, dtype=out.dtype).index_add_(0, idx, rs)
    ldS = torch.zeros(B, dtype=out.dtype).index_add_(0, idx, rsS)
    n = torch.zeros(B, dtype=out.dtype).index_add_(0, idx, (mask > 0).to(out.dtype) * h)
    return {"z": (torch.cat([x0, z1], 1), torch.cat([torch.zeros_like(x0), bz1], 1)), "rowsum": (rs, rsS), "logdet": (ld, ldS, n), "logs": lg}


def coupling_bwd(raw, x1, dz, dlogdet, mask, rowutt, sigmoid_scale=False, e_dz=None, scale_derivative=True):
    """raw [R, C/2] (the logs half of `out`), x1 [R, C/2], dz [R, C] ->
        dx = [dz0 | dz1 mask exp(logs)],  dout = [dz1 mask | (dz1 mask exp(logs) x1 + dlogdet[utt] mask) dlogs/draw].
    Returns {"dx": (ref, bound), "dout": (ref, bound)}; scale_derivative=False plants the omitted sigmoid_scale factor."""
    h = raw.shape[1]
    mk = mask[:, None]
    e = _z(e_dz, dz)
    lg, dl = scale_logs(raw, sigmoid_scale)
    if not scale_derivative:
        dl = torch.ones_like(dl)
    ex = torch.exp(lg)
    dz0, dz1, e1 = dz[:, :h], dz[:, h:] * mk, e[:, h:] * mk
    dld = dlogdet[torch.as_tensor(rowutt).long()][:, None] * mk
    dx1 = dz1 * ex
    bx1 = e1 * ex + dx1.abs() * (exp_rel(lg) + U)
    t = dx1 * x1
    dlg = (t + dld) * dl
    blg = (bx1 * x1.abs() + U * t.abs() + U * (t + dld).abs()) * dl.abs() + (4 * U * dlg.abs() if sigmoid_scale else 0)
    return {"dx": (torch.cat([dz0, dx1], 1), torch.cat([e[:, :h], bx1], 1)), "dout": (torch.cat([dz1, dlg], 1), torch.cat([e1, blg], 1))}


def coupling_rev(out, z, mask, sigmoid_scale=False, e_out=None):
    """x = [z0 | (z1 - m) exp(-logs) mask] (attentions.py:178-180) -> (ref, bound)"""
    h = out.shape[1] // 2
    m, raw, mk = out[:, :h], out[:, h:], mask[:, None]
    e_o = _z(e_out, out)
    lg, dl = scale_logs(raw, sigmoid_scale)
    e_lg = e_o[:, h:] * dl.abs()
    if sigmoid_scale:
        e_lg = e_lg + fast_log_sigmoid_err(raw)
    ex = torch.exp(-lg)
    d = z[:, h:] - m
    x1 = d * ex * mk
    # (z1 - m - dm) exp(-logs - dl): the error in m rides on the perturbed exponential too
    b1 = (e_o[:, :h] * ex * torch.exp(e_lg) + d.abs() * ex * (torch.expm1(e_lg) + exp_rel(lg) + 2 * U) + U * d.abs() * ex) * mk
    return torch.cat([z[:, :h], x1], 1), torch.cat([torch.zeros_like(x1), b1], 1)


# ----------------------------------------------------------------------------- ActNorm + InvConvNear
def actnorm_invconv_fwd(x, logs, bias, W, mask, e_x=None):
    """y[group g] = W (bias + exp(logs) x)[group g] * mask -> (y, bound), and the pre-mix a = bias + exp(logs) x with its bound"""
    el = torch.exp(logs)
    a = bias + el * x
    ba = el * _z(e_x, x) + (el * x).abs() * (exp_rel(logs) + U) + U * a.abs()
    ag, bag = to_groups(a), to_groups(ba)
    mk = mask[:, None, None]
    yg = (ag @ W.T) * mk
    byg = (bag @ W.abs().T + gamma(4) * (ag.abs() @ W.abs().T)) * mk
    return from_groups(yg), from_groups(byg), a, ba


def actnorm_invconv_rev(y, logs, bias, Winv, mask, e_y=None):
    """x = ((W^-1 y)[group] mask - bias) exp(-logs) mask (modules.py:647-652, 592-594) -> (x, bound)"""
    mk = mask[:, None, None]
    yg, eg = to_groups(y), to_groups(_z(e_y, y))
    ug = (yg @ Winv.T) * mk
    bug = (eg @ Winv.abs().T + gamma(4) * (yg.abs() @ Winv.abs().T)) * mk
    u, bu = from_groups(ug), from_groups(bug)
    el = torch.exp(-logs)
    x = (u - bias) * el * mask[:, None]
    bx = ((bu + U * (u - bias).abs()) * el + x.abs() * (exp_rel(logs) + 2 * U)) * mask[:, None]
    return x, bx


def actnorm_invconv_bwd(x, dy, logs, bias, W, WinvT, mask, dlogdet, lens, e_dy=None, drop_row=None, use_inverse=False,
                        bookkeeping=True, slabs=1):
    """Backward of the pair and of its log-det (sum logs + C/4 logdet W) len[b]:  with dym = dy mask, a = bias + exp(logs) x,
        d a = W^T dym (per group),  dx = d a exp(logs),
        d_an_bias[c] = sum_r d a,  d_an_logs[c] = sum_r d a x exp(logs) + s,  d_w_ic[o][i] = sum_{r, g} dym[o] a[i] + (C/4) s W^-T[o][i],
        s = sum_b dlogdet[b] len[b]   (the bookkeeping term).
    WinvT [4, 4]: the W^-T the kernel reads (gt_flow_scalars' scal[2:]).  slabs: how many partial sums a total is added up from
    (workgroups + reduction stages); every sum is bounded as gamma(addends + slabs) * (sum of absolute values) plus its terms'
    own bounds.  Planted defects: drop_row (a valid row left out of the three sums), use_inverse (W^-1 where W^-T belongs),
    bookkeeping=False (s omitted from d_an_logs).
    Returns {"dx", "d_an_logs", "d_an_bias", "d_w_ic": (ref, bound)}."""
    R, C = x.shape
    G = C // 4
    mk = mask[:, None]
    el = torch.exp(logs)
    a = bias + el * x
    ba = (el * x).abs() * (exp_rel(logs) + U) + U * a.abs()
    dym, e = dy * mk, _z(e_dy, dy) * mk
    dg, eg = to_groups(dym), to_groups(e)
    dag = dg @ W                                              # d a[i] = sum_o W[o][i] dym[o]
    bdag = eg @ W.abs() + gamma(4) * (dg.abs() @ W.abs())
    da, bda = from_groups(dag), from_groups(bdag)
    dx = da * el
    bdx = bda * el + dx.abs() * (exp_rel(logs) + U)
    keep = torch.ones(R, dtype=x.dtype)
    if drop_row is not None:
        keep[drop_row] = 0
    k1, k3 = keep[:, None], keep[:, None, None]
    n = R + slabs
    tL = dx * x
    dlogs = (tL * k1).sum(0)
    blogs = ((bdx * x.abs() + U * tL.abs()) * k1).sum(0) + gamma(n) * (tL.abs() * k1).sum(0)
    dbias = (da * k1).sum(0)
    bbias = (bda * k1).sum(0) + gamma(n) * (da.abs() * k1).sum(0)
    ag, bag = to_groups(a), to_groups(ba)
    tW = dg[:, :, :, None] * ag[:, :, None, :] * k3[..., None]                      # [R, G, o, i]
    dW = tW.sum((0, 1))
    bW = ((eg[:, :, :, None] * (ag.abs() + bag)[:, :, None, :] + dg.abs()[:, :, :, None] * bag[:, :, None, :]) * k3[..., None]).sum((0, 1)) \
        + (U + gamma(R * G + slabs)) * tW.abs().sum((0, 1))
    lens = lens.to(x.dtype)
    s = (dlogdet * lens).sum()
    bs = gamma(len(lens) + 4) * (dlogdet * lens).abs().sum()
    M = WinvT.T if use_inverse else WinvT
    if bookkeeping:
        dlogs = dlogs + s
        blogs = blogs + bs + U * (dlogs.abs() + s.abs())
    dW = dW + G * s * M
    bW = bW + G * (bs + 3 * U * s.abs()) * M.abs() + U * dW.abs()
    return {"dx": (dx, bdx), "d_an_logs": (dlogs, blogs), "d_an_bias": (dbias, bbias), "d_w_ic": (dW.reshape(-1), bW.reshape(-1))}


# ----------------------------------------------------------------------------- the pair's log-det, gt_flow_scalars
def flow_scalars(logs, W):
    """gt_flow_scalars' 18 values {sum logs, logdet W, W^-T row major} in the dtype of the arguments"""
    return torch.cat([logs.sum().reshape(1), torch.logdet(W).reshape(1), torch.linalg.inv(W).T.reshape(-1)])


def pair_logdet(scal, lens, C):
    """(sum logs + C/4 logdet W) len[b] from the 18 scalars -> (ref [B], bound): the kernel forms the per-frame value once in fp32
    (a product and a sum) and multiplies by the length"""
    lens = lens.to(scal.dtype)
    pf = scal[0] + (C // 4) * scal[1]
    return pf * lens, U * (scal[0].abs() + 2 * (C // 4) * scal[1].abs() + 2 * pf.abs()) * lens


def rows(x, dtype=F64):
    return t64(x).to(dtype)
