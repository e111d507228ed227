"""TEST INFRASTRUCTURE ONLY — float64 restatement of the channel LayerNorm kernels (csrc/encoder_ops.hip: gt_layernorm_fwd_kernel,
gt_layernorm_bwd_kernel in its atomics and partials forms, gt_param_partials_reduce_kernel), for the rule of oracle/rows64.py.

Operands are the kernel's own: a fp32 [R, C], y bf16 [R, C] (either may be absent), gamma / beta fp32, rowmask, the dropout keeps
of oracle/dropmask.py (drop_keep(seed, row, channel, thresh32(p)), scale fp32 1 / (1 - p)); the backward is TEACHER-FORCED on the
mean and rstd the forward stored.

  forward   s = a + y keep_in scale_in;  mean = sum_c s / C;  var = sum_c (s - mean)^2 / C;  rstd = 1 / sqrt(var + eps)
            n = (s - mean) rstd gamma + beta;  o = relu?(n) keep_out scale_out rowmask          (out_f32 and / or out_bf16)
  backward  xh = (s - mean) rstd;  d = (dout_f32 + dout_bf16) rowmask keep_out scale_out, zero where relu & 1 and xh gamma + beta <= 0
            dgamma += sum_m d xh;  dbeta += sum_m d;  dn = d gamma;  s1 = sum_c dn / C;  s2 = sum_c dn xh / C
            ds = rstd (dn - s1 - xh s2);  da = ds;  dy = bf16(ds keep_in scale_in), keep_in also false where relu & 2 and the bf16 y
            has zero magnitude bits (y is a ReLU's output: +0 and -0 alike)

Bounds (u = 2^-24; gamma(K) = (K + 4) 2^-23, rows64.gamma), every line one fp32 operation of the kernel carried to first order:
  e_s     u |y scale| (the product, only with p_in) + u |s| (the add, only with both a and y)
  mean    (sum_c e_s + gamma(C) sum_c |s|) / C + u |mean|                               C-term sum in any order, the division
  var     dd = s - mean: e_dd = e_s + e_mean + u |dd|;  (sum_c (2 |dd| e_dd + u dd^2) + gamma(C) sum_c dd^2) / C + u var
  rstd    rstd ((e_var + u (var + eps)) / (2 (var + eps)) + FAST_FN)                    the add of eps, rsqrtf (v_rsq_f32)
  n       |rstd gamma| e_dd + |dd gamma| e_rstd + 3 u |dd rstd gamma| + u |n|           two multiplies, the add (fma or not)
  o       e_n (ReLU is 1-Lipschitz) scaled by keep scale, + u |o| for that multiply
  xh      rstd (e_s + u |s - mean|) + u |xh|                                            mean and rstd are exact operands here
  d       u |d| for the add of the two dout forms (only with both) + u |d| for the multiply by scale_out (only with p_out)
  dn      |gamma| e_d + u |dn|
  s1      (sum_c e_dn + gamma(C) sum_c |dn|) / C + u |s1|
  s2      (sum_c (e_dn |xh| + |dn| e_xh + u |dn xh|) + gamma(C) sum_c |dn xh|) / C + u |s2|
  ds      rstd (e_dn + e_s1 + e_xh |s2| + |xh| e_s2 + 3 u (|dn| + |s1| + |xh s2|)) + u |ds|;   dy: keep scale e_ds + u |dy|
  dgamma  gamma(K) (|prior| + sum_m |d xh|) + sum_m |d| e_xh,  dbeta  gamma(K) (|prior| + sum_m |d|) + sum_m e_d, with K the number of
          additions in any order: R products (each rounds: 2 R for dgamma), the workgroups' atomics or partial rows, the prior value.
The ReLU gate (relu & 1) decides on an fp32 value: where the float64 pre-activation lies within its own bound e_pre = |gamma| e_xh +
2 u (|xh gamma| + |pre|) of zero the kernel may go either way (`ambiguous`).  Those elements are left out of the elementwise rule of
da / dy, and their possible contribution (present or absent) is ADDED to the bounds of what they feed: |dn| / C to s1, |dn xh| / C to
s2 of their row, |d xh| and |d| to dgamma / dbeta of their channel.
"""
import numpy as np
import torch

from oracle.rows64 import FAST_FN, RHO, gamma, t64

U = RHO["f32"]


def _ks(keep, scale, like):
    return torch.ones_like(like) if keep is None else t64(np.asarray(keep, dtype=np.float64)) * float(scale)


def _s(a, y, keep_in, scale_in):
    """s = a + y keep scale and its bound e_s"""
    if y is None:
        return t64(a), torch.zeros_like(t64(a))
    yy = t64(y)
    e = torch.zeros_like(yy)
    if keep_in is not None:
        yy = yy * _ks(keep_in, scale_in, yy)
        e = U * yy.abs()
    if a is None:
        return yy, e
    s = t64(a) + yy
    return s, e + U * s.abs()


def forward(a, y, gam, beta, rowmask, eps, keep_in=None, scale_in=1.0, keep_out=None, scale_out=1.0, relu=0, skip_mean_channel=None):
    """{"mean", "rstd" [R]; "out" [R, C]: (ref, bound)} plus "s": (s, e_s).  skip_mean_channel: planted defect, that channel left out
    of the mean's sum (still divided by C)."""
    s, e_s = _s(a, y, keep_in, scale_in)
    C = s.shape[1]
    gam, beta = t64(gam), t64(beta)
    sm = s
    if skip_mean_channel is not None:
        sm = s.clone()
        sm[:, skip_mean_channel] = 0
    mean = sm.sum(1, keepdim=True) / C
    e_mean = (e_s.sum(1, keepdim=True) + gamma(C) * s.abs().sum(1, keepdim=True)) / C + U * mean.abs()
    dd = s - mean
    e_dd = e_s + e_mean + U * dd.abs()
    var = (dd * dd).sum(1, keepdim=True) / C
    e_var = ((2 * dd.abs() * e_dd + U * dd * dd).sum(1, keepdim=True) + gamma(C) * (dd * dd).sum(1, keepdim=True)) / C + U * var
    rstd = 1.0 / torch.sqrt(var + eps)
    e_rstd = rstd * ((e_var + U * (var + eps)) / (2 * (var + eps)) + FAST_FN)
    n = dd * rstd * gam + beta
    e_n = (rstd * gam).abs() * e_dd + (dd * gam).abs() * e_rstd + 3 * U * (dd * rstd * gam).abs() + U * n.abs()
    o = torch.relu(n) if relu else n
    if keep_out is not None:
        ks = _ks(keep_out, scale_out, o)
        o, e_n = o * ks, e_n * ks + U * (o * ks).abs()
    rm = torch.ones(s.shape[0], 1, dtype=torch.float64) if rowmask is None else t64(rowmask).reshape(-1, 1)
    return {"s": (s, e_s), "mean": (mean[:, 0], e_mean[:, 0]), "rstd": (rstd[:, 0], e_rstd[:, 0]), "out": (o * rm, e_n * rm)}


def backward(a, y, gam, beta, rowmask, mean, rstd, dout_f32, dout_bf16, K_param, prior_gamma, prior_beta,
             keep_in=None, scale_in=1.0, keep_out=None, scale_out=1.0, relu=0, y_bits=None, dy_scale=True, skip_row=None):
    """{"da", "dy" [R, C]; "dgamma", "dbeta" [C]: (ref, bound)}, "ambiguous": bool [R, C].  mean / rstd: the kernel's own (fp32).
    y_bits: the raw bf16 bits of y (relu & 2).  Planted defects: dy_scale = False leaves p_in's scale out of dy; skip_row leaves that
    row out of dgamma (and dbeta)."""
    s, e_s = _s(a, y, keep_in, scale_in)
    R, C = s.shape
    gam, beta = t64(gam), t64(beta)
    mean, rstd = t64(mean).reshape(-1, 1), t64(rstd).reshape(-1, 1)
    xh = (s - mean) * rstd
    e_xh = rstd * (e_s + U * (s - mean).abs()) + U * xh.abs()
    rm = torch.ones(R, 1, dtype=torch.float64) if rowmask is None else t64(rowmask).reshape(-1, 1)
    d = torch.zeros_like(s)
    for t in (dout_f32, dout_bf16):
        if t is not None:
            d = d + t64(t)
    e_d = U * d.abs() if (dout_f32 is not None and dout_bf16 is not None) else torch.zeros_like(d)
    d, e_d = d * rm, e_d * rm
    if keep_out is not None:
        ks = _ks(keep_out, scale_out, d)
        d, e_d = d * ks, e_d * ks + U * (d * ks).abs()
    amb = torch.zeros_like(s, dtype=torch.bool)
    if relu & 1:
        pre = xh * gam + beta
        e_pre = gam.abs() * e_xh + 2 * U * ((xh * gam).abs() + pre.abs())
        amb = (pre.abs() <= e_pre) & (d != 0)
        gate = (pre > 0).double()
        d_amb = d * amb                                              # what the gate may let through or not
        d, e_d = d * gate * (~amb), e_d * gate
    else:
        d_amb = torch.zeros_like(d)
    dn = d * gam
    e_dn = gam.abs() * e_d + U * dn.abs()
    dn_amb = (d_amb * gam).abs()
    s1 = dn.sum(1, keepdim=True) / C
    e_s1 = (e_dn.sum(1, keepdim=True) + gamma(C) * dn.abs().sum(1, keepdim=True) + dn_amb.sum(1, keepdim=True)) / C + U * s1.abs()
    s2 = (dn * xh).sum(1, keepdim=True) / C
    e_s2 = ((e_dn * xh.abs() + dn.abs() * e_xh + U * (dn * xh).abs()).sum(1, keepdim=True) + gamma(C) * (dn * xh).abs().sum(1, keepdim=True)
            + (dn_amb * xh.abs()).sum(1, keepdim=True)) / C + U * s2.abs()
    ds = rstd * (dn - s1 - xh * s2)
    e_ds = rstd * (e_dn + e_s1 + e_xh * s2.abs() + xh.abs() * e_s2 + 3 * U * (dn.abs() + s1.abs() + (xh * s2).abs())) + U * ds.abs()
    dy, e_dy = ds, e_ds
    if keep_in is not None or (relu & 2):
        k = torch.ones_like(s) if keep_in is None else t64(np.asarray(keep_in, dtype=np.float64))
        if relu & 2:
            k = k * t64(((np.asarray(y_bits).astype(np.uint16) & 0x7fff) != 0).astype(np.float64))
        k = k * (float(scale_in) if dy_scale else 1.0)
        dy, e_dy = ds * k, e_ds * k + U * (ds * k).abs()
    dg_rows, db_rows = d * xh, d
    if skip_row is not None:
        dg_rows, db_rows = dg_rows.clone(), db_rows.clone()
        dg_rows[skip_row] = 0
        db_rows[skip_row] = 0
    pg, pb = t64(prior_gamma), t64(prior_beta)
    dgamma = pg + dg_rows.sum(0)
    b_dg = gamma(K_param + R) * (pg.abs() + (d * xh).abs().sum(0)) + (d.abs() * e_xh + e_d * xh.abs()).sum(0) + (d_amb * xh).abs().sum(0)
    dbeta = pb + db_rows.sum(0)
    b_db = gamma(K_param) * (pb.abs() + d.abs().sum(0)) + e_d.sum(0) + d_amb.abs().sum(0)
    return {"da": (ds, e_ds), "dy": (dy, e_dy), "dgamma": (dgamma, b_dg), "dbeta": (dbeta, b_db), "ambiguous": amb}


def param_terms(R, form, n_rows=None):
    """K of dbeta's sum (dgamma adds R for its products' own roundings): R rows + one addition per workgroup (atomics form: 32 rows per
    workgroup from R = 2048 on, else 16) or per partial row and the reduce kernel's 4 row slices (partials form) + the prior value."""
    if form == "atomics":
        return R + -(-R // (32 if R >= 2048 else 16)) + 1
    return R + n_rows + 4 + 1


def check_excluding(name, got, ref, bound, exclude, kind="f32"):
    """rows64.check with the `exclude`d elements taken out of every rule; returns (Report, share excluded)"""
    from oracle import rows64
    keep = ~exclude.reshape(-1)
    g, r, b = (t64(x).reshape(-1)[keep] for x in (got, ref, bound))
    return rows64.check(name, g, r, b, kind), float(exclude.double().mean())


# ----------------------------------------------------------------------------- the checks of one forward + backward call
def _keep(p, seed, R, C):
    from oracle import dropmask
    if not p:
        return None, 1.0
    return dropmask.drop_keep(seed, np.arange(R)[:, None], np.arange(C)[None, :], dropmask.thresh32(p)), dropmask.scale(p)


def check_case(tag, c, got, log=print, max_excluded=1e-4):
    """Every check of one gt_layernorm_fwd + backward call (either backward form; got["dgamma"] / got["dbeta"] are the destinations
    after the atomics or after gt_param_partials_reduce).
    c: namespace with a (fp32 [R, C] or None), y (bf16 tensor [R, C] or None), gamma, beta, rowmask, eps, p_in, seed_in, p_out, seed_out
       (the hashed seeds), relu, dout_f32, dout_bf16 (either None), prior_gamma, prior_beta, K_param (param_terms).
    got: mean, rstd, out_f32 / out_bf16 (either None), da / dy (either None), dgamma, dbeta.
    Returns ({check name: Report}, share of elements the ReLU gate's ambiguity excluded)."""
    from oracle import rows64
    R, C = (c.a if c.a is not None else c.y).shape
    ch = C // 3                                                       # the channel the planted defect leaves out of the mean
    ki, si = _keep(c.p_in, c.seed_in, R, C)
    ko, so = _keep(c.p_out, c.seed_out, R, C)
    y_bits = None if c.y is None else rows64.bits(c.y)
    fw = dict(keep_in=ki, scale_in=si, keep_out=ko, scale_out=so, relu=c.relu & 1)
    f = forward(c.a, c.y, c.gamma, c.beta, c.rowmask, c.eps, **fw)
    f_eps = forward(c.a, c.y, c.gamma, c.beta, c.rowmask, 1e-5, **fw)
    f_ch = forward(c.a, c.y, c.gamma, c.beta, c.rowmask, c.eps, skip_mean_channel=ch, **fw)
    rep = {}
    cc = rows64.check_with_control
    rep["mean"] = cc(f"{tag} mean <channel {ch} left out>", got["mean"], *f["mean"], f_ch["mean"][0], log=log)
    rep["rstd"] = cc(f"{tag} rstd <eps 1e-5>", got["rstd"], *f["rstd"], f_eps["rstd"][0], log=log)
    if got.get("out_f32") is not None:
        cc(f"{tag} out_f32 <eps 1e-5>", got["out_f32"], *f["out"], f_eps["out"][0], log=log)
        rep["out_f32"] = cc(f"{tag} out_f32 <channel {ch} left out of the mean>", got["out_f32"], *f["out"], f_ch["out"][0], log=log)
    if got.get("out_bf16") is not None:
        rep["out_bf16"] = cc(f"{tag} out_bf16 <channel {ch} left out of the mean>", got["out_bf16"], *f["out"], f_ch["out"][0], kind="bf16", log=log)
    bw = dict(keep_in=ki, scale_in=si, keep_out=ko, scale_out=so, relu=c.relu, y_bits=y_bits)
    args = (c.a, c.y, c.gamma, c.beta, c.rowmask)
    tail = (c.dout_f32, c.dout_bf16, c.K_param, c.prior_gamma, c.prior_beta)
    g = backward(*args, got["mean"], got["rstd"], *tail, **bw)
    g_ch = backward(*args, f_ch["mean"][0], f_ch["rstd"][0], *tail, **bw)
    d = torch.zeros(R, C, dtype=torch.float64)
    for t in (c.dout_f32, c.dout_bf16):
        if t is not None:
            d = d + t64(t)
    rm = torch.ones(R) if c.rowmask is None else t64(c.rowmask)
    row = int(((d.abs().sum(1)) * rm).argmax())                       # the row the planted defect leaves out of dgamma / dbeta
    g_row = backward(*args, got["mean"], got["rstd"], *tail, skip_row=row, **bw)
    amb = g["ambiguous"].reshape(-1)
    share = float(amb.double().mean())
    assert share <= max_excluded, f"{tag}: the ReLU gate is ambiguous on {share:.3g} of the elements"
    sel = lambda x: t64(x).reshape(-1)[~amb]                          # noqa: E731
    if got.get("da") is not None:
        rep["da"] = cc(f"{tag} da <channel {ch} left out of the mean>", sel(got["da"]), sel(g["da"][0]), sel(g["da"][1]), sel(g_ch["da"][0]), log=log)
    if got.get("dy") is not None:
        if c.p_in:
            bad, label = backward(*args, got["mean"], got["rstd"], *tail, dy_scale=False, **bw)["dy"][0], "p_in's scale left out"
        else:
            bad, label = g_ch["dy"][0], f"channel {ch} left out of the mean"
        rep["dy"] = cc(f"{tag} dy <{label}>", sel(got["dy"]), sel(g["dy"][0]), sel(g["dy"][1]), sel(bad), kind="bf16", log=log)
    for n in ("dgamma", "dbeta"):
        rep[n] = cc(f"{tag} {n} <row {row} left out>", got[n], *g[n], g_row[n][0], log=log)
    log(f"{tag}: ReLU gate ambiguous on {share:.3g} of the elements (limit {max_excluded:g})")
    return rep, share


def make_case(R_, C, form, seed=0):
    """The operand forms the product uses (CPU tensors; the tests' shared case builder): "a" (a only, dout_f32), "y" (bf16 y only,
    dout_bf16), "a+y" (p_in = 0.1, both dout forms: the post-attention residual), "relu1" (relu = 1, p_out = 0.5: the prenet), "relu2"
    (relu = 2, y a ReLU's output with exact +0 and -0 entries).  rowmask has zero rows at both ends and in the middle.
    Scales: a, y ~ 0.25 N(0,1), so var ~ 0.06 and the eps 1e-5 defect moves rstd by 7e-4 of its value (at var = 1 it would move it by
    4.5e-5, under 3x the fp32 bound gamma(C) / 2); the pre-activations are unit normal whatever the input's scale.  gamma ~ 1 + 0.1 N,
    beta ~ 0.1 N keep the ReLU gate's pre-activation xh gamma + beta a continuous variable of density <= 0.5 at zero: with a bound
    near 1e-6 the expected ambiguous share is about 1e-6."""
    import types
    from oracle import dropmask
    g = torch.Generator().manual_seed(seed + R_ + C)
    c = types.SimpleNamespace(a=None, y=None, eps=1e-4, p_in=0.0, p_out=0.0, seed_in=dropmask.word_seed(5, 1234), seed_out=dropmask.word_seed(5, 4321),
                              relu=0, dout_f32=None, dout_bf16=None)
    if form != "y":
        c.a = 0.25 * torch.randn(R_, C, generator=g)
    if form != "a":
        c.y = (torch.randn(R_, C, generator=g) * (0.1 if form == "a+y" else 0.25)).to(torch.bfloat16)
    if form == "a+y":
        c.p_in = 0.1
    if form == "relu1":
        c.relu, c.p_out = 1, 0.5
    if form == "relu2":
        y = torch.relu(c.y.float())
        y[::3, ::5] = -0.0
        c.y, c.relu = y.to(torch.bfloat16), 2
    c.gamma, c.beta = 1 + 0.1 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g)
    rm = torch.ones(R_)
    rm[:3] = 0; rm[R_ // 2:R_ // 2 + 4] = 0; rm[-5:] = 0
    c.rowmask = rm
    d = torch.randn(R_, C, generator=g)
    if form in ("a", "relu1"):
        c.dout_f32 = d
    elif form in ("y", "relu2"):
        c.dout_bf16 = d.to(torch.bfloat16)
    else:
        c.dout_f32, c.dout_bf16 = d, torch.randn(R_, C, generator=g).to(torch.bfloat16)
    c.prior_gamma, c.prior_beta = torch.randn(C, generator=g), torch.randn(C, generator=g)
    c.K_param = param_terms(R_, "atomics")
    return c
