"""TEST INFRASTRUCTURE ONLY — float64 restatement of the per-op DDSConv kernels (the first half of csrc/predictor_ops.hip: gt_dds_sep_fwd,
gt_dds_out_fwd, gt_dds_out_bwd, gt_dds_sep_bwd, gt_dds_dw_bwd) and of gt_rows_split3 on the rows layout, one operator per kernel, for
tests/test_dds64.py and tests/test_dds_ops_fp64_gpu.py.

Every operator takes the kernel's OWN operands (teacher forcing: sep_bwd a d a1, out_* an h2, dw_bwd a d h1 and a dy), so no GEMM sits
between a kernel and its check.  The four nonlinear operators take `dtype=`: at torch.float64 they are the reference, at torch.float32
the "fp32 twin" whose own error against float64 a kernel's error is held to.  dw_bwd is linear: it returns the absolute-value twin of
every sum and its term count, for the elementwise rule of rows64.check.  Both LayerNorm backwards are written by hand (ln_bwd_row of
csrc/dds_rows.h restated), so that defects can be planted in them; tests/test_dds64.py holds them to float64 autograd of the forwards.

Rows: x [R, C] is zero on rows with rowmask == 0 (the contract of the kernels); every other row operand may hold anything there.
Parameter gradients ACCUMULATE: every backward takes the prior values and returns prior + contribution.  Row outputs are overwritten,
masked rows with zeros.

Planted defects (`defect=` one name or a collection of names; they live here only, so none of them can fault):
  "ignore_utt"     the side taps ignore the utterance index (they still stop at [0, R) and at masked rows)
  "taps_swapped"   tap 0 reads row m + d and tap 2 row m - d
  "gelu_tanh"      the tanh approximation of GELU, and its derivative
  "var_cm1"        LayerNorm's variance divided by C - 1
  "no_drop_scale"  the backward replays the keep mask but leaves 1 / (1 - p) out
  "dw_3C"          d w laid out as [3][C] where [C][3] is read
  "overwrite"      a parameter gradient overwritten instead of accumulated into
The eighth, a keep mask of seed + 1, is planted through the operands (`keep_mask(seed + 1, ...)`).
"""
import math
import types

import numpy as np
import torch

from oracle import dropmask, rows64

C = 192
F64 = torch.float64
DEFECTS = ("ignore_utt", "taps_swapped", "gelu_tanh", "var_cm1", "no_drop_scale", "dw_3C", "overwrite")
_K0, _K1 = math.sqrt(2.0 / math.pi), 0.044715


def _c(x, dtype):
    """x as a CPU tensor of dtype; a tensor that requires grad stays in its graph (tests/test_dds64.py differentiates the forwards)"""
    if x is None:
        return None
    x = torch.as_tensor(x)
    return (x if x.requires_grad else x.detach()).cpu().to(dtype)


def _has(defect, name):
    return defect is not None and (defect == name or (not isinstance(defect, str) and name in defect))


def _on(rowmask):
    return torch.as_tensor(rowmask).detach().cpu() != 0


def _rows(t, on):
    """t with its masked rows zeroed (they may hold anything)"""
    return torch.where(on[:, None], t, torch.zeros_like(t))


# ------------------------------------------------------------------------------------------------ pieces
def tap_rows(utt, rowmask, d, defect=None):
    """{k: (row read by tap k of every row m, clamped into [0, R); whether the tap counts)} for the side taps k = 0, 2: the row
    m + (k - 1) d counts only inside [0, R), inside the same utterance and where rowmask != 0 (tap_ok of csrc/dds_rows.h)"""
    utt, on = torch.as_tensor(utt).detach().cpu().long(), _on(rowmask)
    R = utt.numel()
    m = torch.arange(R)
    taps = {}
    for k in (0, 2):
        mm = m + ((1 - k) if _has(defect, "taps_swapped") else (k - 1)) * d
        mc = mm.clamp(0, R - 1)
        ok = (mm >= 0) & (mm < R) & on[mc]
        if not _has(defect, "ignore_utt"):
            ok = ok & (utt[mc] == utt)
        taps[k] = (mc, ok)
    return taps


def gelu(u, defect=None):
    if _has(defect, "gelu_tanh"):
        return 0.5 * u * (1 + torch.tanh(_K0 * (u + _K1 * u ** 3)))
    return 0.5 * u * (1 + torch.erf(u * math.sqrt(0.5)))


def gelu_grad(u, defect=None):
    if _has(defect, "gelu_tanh"):
        t = torch.tanh(_K0 * (u + _K1 * u ** 3))
        return 0.5 * (1 + t) + 0.5 * u * (1 - t * t) * _K0 * (1 + 3 * _K1 * u * u)
    return 0.5 * (1 + torch.erf(u * math.sqrt(0.5))) + u * torch.exp(-0.5 * u * u) / math.sqrt(2 * math.pi)


def _ln(h, eps, defect=None):
    """(xhat, rstd) of every row"""
    n = h.shape[1]
    mean = h.mean(1, keepdim=True)
    var = ((h - mean) ** 2).sum(1, keepdim=True) / (n - 1 if _has(defect, "var_cm1") else n)
    rstd = (var + eps).rsqrt()
    return (h - mean) * rstd, rstd


def sep_h1(x, w, b, utt, rowmask, d, dtype=F64, defect=None):
    """h1[m] = b + sum_k w[:, k] x[m + (k - 1) d] over the taps that count (every row; the kernels use the valid ones)"""
    x, w, b = _c(x, dtype), _c(w, dtype).reshape(-1, 3), _c(b, dtype)
    h1 = b + w[:, 1] * x
    for k, (mc, ok) in tap_rows(utt, rowmask, d, defect).items():
        h1 = h1 + w[:, k] * x[mc] * ok[:, None].to(dtype)
    return h1


def ln_gelu_fwd(h, gamma, beta, rowmask, eps, dtype=F64, defect=None):
    """gelu_erf(LayerNorm(h)) on valid rows, 0 on masked rows"""
    on = _on(rowmask)
    xh, _ = _ln(_rows(_c(h, dtype), on), eps, defect)
    return _rows(gelu(xh * _c(gamma, dtype) + _c(beta, dtype), defect), on)


def ln_gelu_bwd(h, dA, gamma, beta, rowmask, eps, prior_dgamma, prior_dbeta, dtype=F64, defect=None):
    """the backward of ln_gelu_fwd by hand (ln_bwd_row): dA at the GELU's output -> (d h, d gamma, d beta)"""
    on = _on(rowmask)
    h, dA, gamma, beta = _rows(_c(h, dtype), on), _rows(_c(dA, dtype), on), _c(gamma, dtype), _c(beta, dtype)
    xh, rstd = _ln(h, eps, defect)
    du = _rows(dA * gelu_grad(xh * gamma + beta, defect), on)
    dgamma, dbeta = (du * xh).sum(0), du.sum(0)
    dxh = du * gamma
    s1, s2 = dxh.mean(1, keepdim=True), (dxh * xh).mean(1, keepdim=True)
    dh = _rows(rstd * (dxh - s1 - xh * s2), on)
    if not _has(defect, "overwrite"):
        dgamma, dbeta = dgamma + _c(prior_dgamma, dtype).reshape(-1), dbeta + _c(prior_dbeta, dtype).reshape(-1)
    return dh, dgamma, dbeta


# ------------------------------------------------------------------------------------------------ one operator per kernel
def sep_fwd(x, w, b, gamma1, beta1, utt, rowmask, d, eps, dtype=F64, defect=None):
    """gt_dds_sep_fwd: a1 [R, C] (the kernel stores it as the bf16 pair hi + lo)"""
    return ln_gelu_fwd(sep_h1(x, w, b, utt, rowmask, d, dtype, defect), gamma1, beta1, rowmask, eps, dtype, defect)


def out_fwd(h2, x, gamma2, beta2, rowmask, keep, scale, eps, dtype=F64, defect=None):
    """gt_dds_out_fwd: out = x + keep * scale * gelu(LN(h2)) on valid rows, 0 on masked rows; keep: 0 / 1 [R, C] or None"""
    y = ln_gelu_fwd(h2, gamma2, beta2, rowmask, eps, dtype, defect)
    if keep is not None:
        y = y * _c(keep, dtype) * _c(scale, dtype)
    return _rows(_c(x, dtype) + y, _on(rowmask))


def out_bwd(h2, dy, gamma2, beta2, rowmask, keep, scale, eps, prior_dgamma, prior_dbeta, dtype=F64, defect=None):
    """gt_dds_out_bwd: (d h2, d gamma2, d beta2)"""
    dA = _c(dy, dtype)
    if keep is not None:
        dA = torch.where(_c(keep, dtype) != 0, dA if _has(defect, "no_drop_scale") else dA * _c(scale, dtype), torch.zeros_like(dA))
    return ln_gelu_bwd(h2, dA, gamma2, beta2, rowmask, eps, prior_dgamma, prior_dbeta, dtype, defect)


def sep_bwd(x, w, b, gamma1, beta1, utt, rowmask, d, da1, eps, prior_dgamma, prior_dbeta, dtype=F64, defect=None):
    """gt_dds_sep_bwd: (d h1, d gamma1, d beta1), h1 recomputed from x"""
    return ln_gelu_bwd(sep_h1(x, w, b, utt, rowmask, d, dtype, defect), da1, gamma1, beta1, rowmask, eps, prior_dgamma, prior_dbeta, dtype, defect)


def dw_bwd(x, dh1, dy, w, utt, rowmask, d, prior_dw, prior_db, defect=None):
    """gt_dds_dw_bwd in float64: dx = dy + sum_k w[:, k] dh1[m - (k - 1) d] on valid rows (0 on masked rows),
    dw[c, k] = prior + sum_m dh1[m, c] x[m + (k - 1) d, c], db[c] = prior + sum_m dh1[m, c], the sums over valid rows m and the taps
    that count.  Returns a namespace: dx, dw [C, 3], db, their absolute-value twins S_dx, S_dw, S_db (priors included) and the term
    counts K_dx = 4, K_dw = K_db = valid rows + 1."""
    on = _on(rowmask)
    x, dh1, dy, w = _c(x, F64), _rows(_c(dh1, F64), on), _rows(_c(dy, F64), on), _c(w, F64).reshape(-1, 3)
    taps = tap_rows(utt, rowmask, d, defect)
    dx, S_dx = dy + w[:, 1] * dh1, dy.abs() + w[:, 1].abs() * dh1.abs()
    dw, S_dw = torch.zeros_like(w), torch.zeros_like(w)
    dw[:, 1], S_dw[:, 1] = (dh1 * x).sum(0), (dh1 * x).abs().sum(0)
    R = x.shape[0]
    for k, (mc, ok) in taps.items():
        okf = (ok & on)[:, None].double()
        dw[:, k], S_dw[:, k] = (dh1 * x[mc] * okf).sum(0), (dh1 * x[mc] * okf).abs().sum(0)
        # row m gives w[:, k] dh1[m] to dx[m + (k - 1) d]: the transpose of the gather above
        dx = dx.index_add(0, mc, w[:, k] * dh1 * okf)
        S_dx = S_dx.index_add(0, mc, (w[:, k] * dh1 * okf).abs())
    dx, S_dx = _rows(dx, on), _rows(S_dx, on)
    db, S_db = dh1.sum(0), dh1.abs().sum(0)
    if _has(defect, "dw_3C"):
        dw, S_dw = dw.t().contiguous().reshape(-1, 3), S_dw.t().contiguous().reshape(-1, 3)
    if not _has(defect, "overwrite"):
        pw, pb = _c(prior_dw, F64).reshape(-1, 3), _c(prior_db, F64).reshape(-1)
        dw, S_dw, db, S_db = dw + pw, S_dw + pw.abs(), db + pb, S_db + pb.abs()
    K = int(on.sum()) + 1
    return types.SimpleNamespace(dx=dx, dw=dw, db=db, S_dx=S_dx, S_dw=S_dw, S_db=S_db, K_dx=4, K_dw=K, K_db=K, R=R)


# ------------------------------------------------------------------------------------------------ gt_rows_split3
def split3(v, rowmask=None):
    """gt_rows_split3: the bf16 bits [R, 3 C'] = [hi | hi | lo] (uint16) of v [R, C'], fp32 values or a torch.bfloat16 tensor / uint16 bf16
    bits: hi = bf16(v * mask), lo = bf16(v * mask - hi) in fp32 arithmetic (for a bf16 input that is lo = 0)"""
    if isinstance(v, torch.Tensor) and v.dtype == torch.bfloat16 or isinstance(v, np.ndarray) and v.dtype == np.uint16:
        v = rows64.bf2f(v)
    v = np.asarray(v.detach().cpu() if isinstance(v, torch.Tensor) else v, dtype=np.float32)
    if rowmask is not None:
        v = (v * np.asarray(torch.as_tensor(rowmask).detach().cpu(), dtype=np.float32)[:, None]).astype(np.float32)
    hi = rows64.f2bf(v)
    lo = rows64.f2bf((v - rows64.bf2f(hi)).astype(np.float32))
    return np.concatenate([hi, hi, lo], 1)


def pair_value(bits3):
    """hi + lo of split3 bits [R, 3 C'] as float64 [R, C']"""
    n = bits3.shape[1] // 3
    b = np.asarray(bits3)
    return torch.from_numpy(rows64.bf2f(b[:, :n]).astype(np.float64) + rows64.bf2f(b[:, 2 * n:]).astype(np.float64))


def as_pair(v, rowmask=None):
    """v [R, C'] (any float dtype) rounded to fp32 and stored as the bf16 pair: what a kernel that computes v in fp32 can hand on"""
    return pair_value(split3(_c(v, torch.float32), rowmask))


# ------------------------------------------------------------------------------------------------ the dropout mask
def keep_mask(seed, word, R, p, n=C):
    """(keep 0 / 1 [R, n] float64, scale) of drop_keep(word ^ seed, row, channel) by oracle/dropmask.py; (None, 1) at p = 0"""
    if p <= 0:
        return None, 1.0
    m = dropmask.channel_mask(seed, word, np.arange(R, dtype=np.int64)[None, :], n, p)[0].t().contiguous()      # [R, n] keep * scale
    return (m != 0).double(), float(dropmask.scale(p))


# ------------------------------------------------------------------------------------------------ geometries and operands of the tests
def layout(R, utts):
    """utts: (first row, rows owned, first valid row, valid rows) per utterance, in row order; the last one owns the rest"""
    utt, mask = np.zeros(R, dtype=np.int32), np.zeros(R, dtype=np.float32)
    for b, (r0, n, v0, nv) in enumerate(utts):
        utt[r0:] = b
        mask[v0:v0 + nv] = 1
        assert r0 <= v0 and v0 + nv <= r0 + n <= R
    return torch.from_numpy(utt), torch.from_numpy(mask)


# a workgroup of the five kernels is 4 waves x 2 rows = 8 rows
WG = 8
GEOMS = {
    "r7": lambda: layout(7, [(0, 7, 0, 7)]),                                    # one utterance, all rows valid, no halo: only the range guard
                                                                                #   stops the taps at rows 0 and 6; wave 3 has one row
    "r8": lambda: layout(8, [(0, 3, 0, 3), (3, 1, 3, 1), (4, 4, 4, 4)]),        # one workgroup; 3, 1 and 4 frames back to back, no halo: at
                                                                                #   d = 1 and d = 3 only `utt` decides
    "r9": lambda: layout(9, [(0, 3, 0, 3), (3, 1, 3, 1), (4, 5, 4, 4)]),        # a second workgroup of a single masked row
    "r33": lambda: layout(33, [(0, 14, 2, 10), (14, 5, 16, 1), (19, 14, 21, 9)]),   # 2-row halos; 10, 1 and 9 frames: the d = 9 taps fall just
                                                                                #   inside utterance 0, onto the halo or outside for 2; a trailing row
    "r70": lambda: layout(70, [(0, 24, 2, 22), (24, 37, 24, 33), (61, 9, 61, 3)]),  # a border on a workgroup edge (row 24), valid on both sides;
                                                                                #   33 frames > 3 workgroups; the last workgroup (rows 64..69) masked
}
WIDE_X = ("r8", "r33", "r70")        # x is a column window of an [R, 256] buffer there
PADDED_A1 = "r33"                    # gt_dds_sep_fwd runs with lda = 3 C + 8 there


def geometry_claims():
    """asserts what the comments of GEOMS say"""
    u, m = GEOMS["r7"]()
    assert m.all() and len(set(u.tolist())) == 1 and m.numel() == 7
    for name in ("r8", "r9"):
        u, m = GEOMS[name]()
        assert u[:8].tolist() == [0, 0, 0, 1, 2, 2, 2, 2] and m[:8].all()
        for d in (1, 3):                                   # no tap of rows 0..7 is stopped by the mask: inside [0, 8) only `utt` decides
            for k, (mc, ok) in tap_rows(u, m, d, "ignore_utt").items():
                mm = torch.arange(8) + (k - 1) * d
                inside = (mm >= 0) & (mm < 8)
                assert bool(ok[:8][inside].all())
            free, true = tap_rows(u, m, d, "ignore_utt"), tap_rows(u, m, d)
            crossing = sum(int((free[k][1] & ~true[k][1])[:8].sum()) for k in (0, 2))       # ... and it stops at least four taps
            assert crossing >= 4, (name, d, crossing)
    u, m = GEOMS["r9"]()
    assert m.numel() == 9 and m[8] == 0
    u, m = GEOMS["r33"]()
    assert m.numel() == 33 and int(m.sum()) == 20 and m[32] == 0
    assert [int(m[r]) for r in (1, 2, 11, 12, 15, 16, 17, 20, 21, 29, 30)] == [0, 1, 1, 0, 0, 1, 0, 0, 1, 1, 0]
    t = tap_rows(u, m, 9)
    assert bool(t[2][1][2]) and bool(t[0][1][11]) and not bool(t[2][1][3])           # row 2 + 9 = 11: the last frame of utterance 0
    assert not bool(t[2][1][21]) and not bool(t[0][1][29]) and not bool(t[2][1][29])   # utterance 2: row 30 is halo, row 38 outside
    u, m = GEOMS["r70"]()
    assert m.numel() == 70 and u[23] == 0 and u[24] == 1 and m[23] == 1 and m[24] == 1 and 24 % WG == 0
    assert m[24:57].all() and 33 > 3 * WG and m[64:].sum() == 0 and m[56:64].sum() > 0 and 64 % WG == 0


def operands(gname, seed=0):
    """the fp32 CPU operands of every kernel for one geometry: x zero on masked rows; dy, da1, h2, dh1 with large finite values there;
    gamma = 1 + 0.1 N, beta = 0.1 N, w_sep = 0.5 N; non-zero priors for every parameter gradient"""
    utt, mask = GEOMS[gname]()
    R = mask.numel()
    gen = torch.Generator().manual_seed(5000 + seed + 13 * list(GEOMS).index(gname))
    rn = lambda *s: torch.randn(*s, generator=gen)                                  # noqa: E731
    on = mask != 0
    sign = torch.where(torch.arange(C) % 2 == 0, 1.0, -1.0)

    def rows():
        return torch.where(on[:, None], rn(R, C), 1e30 * sign.expand(R, C))
    O = types.SimpleNamespace(gname=gname, R=R, utt=utt, mask=mask, on=on, n_valid=int(on.sum()))
    O.x = rn(R, C) * mask[:, None]
    O.dy, O.da1, O.h2, O.dh1 = rows(), rows(), rows(), rows()
    O.w, O.b = rn(C, 3) * 0.5, rn(C) * 0.1
    O.gamma1, O.beta1, O.gamma2, O.beta2 = 1 + 0.1 * rn(C), 0.1 * rn(C), 1 + 0.1 * rn(C), 0.1 * rn(C)
    O.dg1_0, O.db1_0, O.dg2_0, O.db2_0, O.dw_0, O.db_0 = rn(C), rn(C), rn(C), rn(C), rn(C, 3), rn(C)
    return O


def reference(O, d, keep, scale, eps, dtype=F64, defect=None, pairs=True):
    """every compared output of the four nonlinear kernels on the operands O, by name; pairs: a1 and d h2 as the bf16 pair a kernel
    stores (the twin's form; the float64 reference stays exact)"""
    v = {}
    v["sep.a1"] = sep_fwd(O.x, O.w, O.b, O.gamma1, O.beta1, O.utt, O.mask, d, eps, dtype, defect)
    v["out.out"] = out_fwd(O.h2, O.x, O.gamma2, O.beta2, O.mask, keep, scale, eps, dtype, defect)
    v["outb.dh2"], v["outb.dgamma"], v["outb.dbeta"] = out_bwd(O.h2, O.dy, O.gamma2, O.beta2, O.mask, keep, scale, eps, O.dg2_0, O.db2_0, dtype, defect)
    v["sepb.dh1"], v["sepb.dgamma"], v["sepb.dbeta"] = sep_bwd(O.x, O.w, O.b, O.gamma1, O.beta1, O.utt, O.mask, d, O.da1, eps, O.dg1_0, O.db1_0,
                                                               dtype, defect)
    if dtype != F64 and pairs:
        v["sep.a1"], v["outb.dh2"] = as_pair(v["sep.a1"]), as_pair(v["outb.dh2"])
    return {k: t.double() for k, t in v.items()}
