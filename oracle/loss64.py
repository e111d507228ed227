"""TEST INFRASTRUCTURE ONLY — float64 restatement of the fp32 kernels between the decoder and the loss (csrc/align_loss.hip:
gt_logp_f32, gt_mle_sums / _finish / _bwd, gt_duration_loss_fwd / _bwd, gt_prior_expand / _bwd, gt_length_mask; csrc/encoder_ops.hip:
gt_embedding_fwd / _bwd, gt_rows_add_cond, gt_rows_utt_sum) and of the layout kernels (csrc/flow_ops.hip: gt_rows_from_bct, gt_bct_from_rows,
gt_squeeze_rows_f32, gt_unsqueeze_rows_f32, gt_rows_f32_to_bf16, gt_rows_add_bf16), each written from the comment above its kernel.

The rule, gamma, RHO, FAST_FN, check and check_with_control are oracle/rows64.py's.  Arithmetic operators return the float64
reference with what the rule needs next to it: the absolute-value twin S (bound = gamma(K) S) or, where the result is elementwise
fp32 work, the bound itself (a count of roundings, derived in the operator's docstring); rho_out |ref| is added by `check`.  They
take `dtype`: torch.float32 gives the float32 twin, the same formula on the same data, which must itself pass the rule
(tests/test_loss64.py).  `defect=` plants one of the defects the tests must see (rows64.CONTROL_MISS).  The data-movement operators
are exact and return the one array the kernel must equal bit for bit.

One fp32 rounding is U = 2^-24.  __expf(-2 s) is allowed FAST_FN = 2^-21 RELATIVE for |s| <= 2 (derived, not measured: the argument
scaling by log2 e costs |2 s| 2^-24 <= 2^-22 of the result, the hardware exp2 one ulp, 2^-23); the tests keep x_logs / logs inside
|s| <= 2.  __logf is outside the rule: the duration loss is held to its float32 twin (tests/test_loss_kernels_fp64_gpu.py).
"""
import math
import os
import re

import numpy as np
import torch

from .rows64 import FAST_FN, RHO, bf16_round, gamma

HALO = 2
U = RHO["f32"]
HALF_LOG_2PI = 0.5 * math.log(2 * math.pi)
F64 = torch.float64
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "glowtts_hip.h")


def header_constant(name):
    """integer value of `#define name value` in include/glowtts_hip.h"""
    with open(HEADER) as f:
        m = re.search(r"^#define\s+" + name + r"\s+(\d+)", f.read(), re.M)
    assert m, f"{name} is not defined in {HEADER}"
    return int(m.group(1))


def _t(x, dtype=F64):
    if isinstance(x, torch.Tensor):
        return x.detach().cpu().to(dtype)
    return torch.from_numpy(np.asarray(x, dtype=np.float64)).to(dtype)


def _i(x):
    return torch.as_tensor(np.asarray(x.detach().cpu() if isinstance(x, torch.Tensor) else x), dtype=torch.int64)


# ----------------------------------------------------------------------------- the rows layout (include/glowtts_hip.h, GT_HALO)
class Layout:
    """Rows of a batch with these lengths: uniform (utterance b owns rows [b Tp, (b + 1) Tp), Tp = T + 2 HALO) or ragged (row0[B + 1],
    utterance b owns its frames + 2 HALO rows, the last one also the rows that round R up to a multiple of `rnd`; Tp is then only an
    upper bound on the rows of one utterance).  Frame t of utterance b is row base(b) + HALO + t."""

    def __init__(self, lens, T, ragged, rnd=8):
        self.lens, self.B, self.T, self.ragged = [int(v) for v in lens], len(lens), int(T), bool(ragged)
        if ragged:
            starts = [0]
            for v in self.lens:
                starts.append(starts[-1] + max(0, min(v, T)) + 2 * HALO)
            self.R = -(-starts[-1] // rnd) * rnd
            starts[-1] = self.R
            self.row0 = np.asarray(starts, dtype=np.int32)
            self.Tp = T + 2 * HALO + rnd - 1
            self.base = self.row0[:-1].astype(np.int64)
        else:
            self.Tp = T + 2 * HALO
            self.R = self.B * self.Tp
            self.row0 = None
            self.base = np.arange(self.B, dtype=np.int64) * self.Tp
        m = np.arange(self.R)
        self.rowbatch = np.searchsorted(self.base, m, side="right") - 1                    # gt_row_batch
        self.rowframe = m - self.base[self.rowbatch] - HALO
        self.count = np.diff(np.append(self.base, self.R))                                   # gt_row_count
        ln = np.minimum(np.asarray(self.lens), T)
        self.valid = (self.rowframe >= 0) & (self.rowframe < ln[self.rowbatch])
        self.rowmask = self.valid.astype(np.float32)

    def frame_rows(self, b):
        """rows of the valid frames of utterance b"""
        return self.base[b] + HALO + np.arange(min(self.lens[b], self.T))


# ----------------------------------------------------------------------------- gt_logp_f32
def logp(x_m, x_logs, z, dtype=F64, defect=None):
    """logp[b,i,j] = sum_d (-0.5 log 2pi - s_id) + sum_d e^{-2 s_id} (-0.5 z_jd^2) + sum_d m_id e^{-2 s_id} z_jd + sum_d -0.5 m_id^2 e^{-2 s_id}
    x_m, x_logs (None = 0) [B, C, Tx], z [B, C, Ty].  Returns (ref [B, Tx, Ty], S, S_e): S the sum over d of the four |terms|, S_e the
    same over the three that hold e^{-2s}.  logp_bound gives the rule's bound from them.  Valid for |x_logs| <= 2 (FAST_FN).
    defect: "drop_channel" (channel C-1 left out of the z^2 term of lattice row Tx-1), "stale_column" (column Ty-1 computed from
    frame Ty-2), "batch_logs" (batch 1 reads batch 0's x_logs), "row_swap" (the row constant of row i given to row i^4)."""
    m, zz = _t(x_m, dtype), _t(z, dtype)
    s = torch.zeros_like(m) if x_logs is None else _t(x_logs, dtype)
    B, C, Tx = m.shape
    Ty = zz.shape[2]
    if defect == "batch_logs":
        s = s.clone()
        s[1] = s[0]
    if defect == "stale_column":
        zz = zz.clone()
        zz[:, :, Ty - 1] = zz[:, :, Ty - 2]
    e = torch.exp(-2 * s)
    t1 = -HALF_LOG_2PI - s
    t4 = -0.5 * m * m * e
    hz = -0.5 * zz * zz
    me = m * e
    rowc = (t1 + t4).sum(1)                                                              # [B, Tx]
    if defect == "row_swap":
        i = torch.arange(Tx)
        src = torch.where((i ^ 4) < Tx, i ^ 4, i)
        rowc = rowc[:, src]
    t2 = torch.einsum("bdi,bdj->bij", e, hz)
    t3 = torch.einsum("bdi,bdj->bij", me, zz)
    if defect == "drop_channel":
        t2 = t2.clone()
        t2[:, Tx - 1, :] -= e[:, C - 1, Tx - 1, None] * hz[:, C - 1, :]
    ref = rowc[:, :, None] + t2 + t3
    S_e = t4.abs().sum(1)[:, :, None] + torch.einsum("bdi,bdj->bij", e, hz.abs()) + torch.einsum("bdi,bdj->bij", me.abs(), zz.abs())
    S = t1.abs().sum(1)[:, :, None] + S_e
    return ref, S, S_e


def logp_bound(C, S, S_e, has_logs):
    """gamma(3 C) S + FAST_FN S_e: 2 C MFMA products and C row-constant terms per element (their own roundings inside gamma's + 4),
    __expf in every term that holds e^{-2s}; without x_logs the kernel uses 1.0f and the second part is gone."""
    return gamma(3 * C) * S + (FAST_FN * S_e if has_logs else 0.0)


# ----------------------------------------------------------------------------- gt_mle_sums + gt_mle_finish, gt_mle_bwd
def mle_depth(n):
    """Longest chain of fp32 additions behind one of gt_mle_sums / gt_mle_finish's sums of n terms: 8 per grid-stride trip of a
    thread (4 elements, 2 operations each; a trip of the grid is 4 * GT_MLE_PARTS * 256 elements), + 64 for the tail element, the
    wave fold (6), the workgroup fold (4), gt_mle_finish's chain (2), wave fold (6) and fold over 16 waves, rounded up generously.
    The sums are bounded by this depth, not by n."""
    parts = header_constant("GT_MLE_PARTS")
    return 8 * max(1, -(-int(n) // (4 * parts * 256))) + 64


def mle(z, m, logs, logdet, mask, C, dtype=F64):
    """commons.mle_loss as the kernels compute it: loss = (sum logs + 0.5 sum e^{-2 logs} (z - m)^2 - sum logdet) / denom + 0.5 log 2pi,
    denom = C sum(mask) (mask: the floats of z_mask [B, 1, T]); logs None = 0; z, m, logs flat, any n >= 0.
    Returns (loss, denom, bound) as 1-element tensors; bound (on loss): gamma(mle_depth(n)) on the absolute-value twins of the two
    big sums, FAST_FN on the e^{-2 logs} sum, gamma(ceil(B / 1024) + 22) on sum |logdet|, 2 U on the three-term numerator, U each
    for denom = sn * C, the division and the final add.  sum(mask) is a sum of 0 / 1 floats: exact below 2^24."""
    zz, mm = _t(z, dtype).reshape(-1), _t(m, dtype).reshape(-1)
    ll = torch.zeros_like(zz) if logs is None else _t(logs, dtype).reshape(-1)
    ld, mk = _t(logdet, dtype).reshape(-1), _t(mask, dtype).reshape(-1)
    d = zz - mm
    q = torch.exp(-2 * ll) * d * d
    a0, a1, sl = ll.sum(), q.sum(), ld.sum()
    denom = mk.sum() * C
    num = a0 + 0.5 * a1 - sl
    loss = num / denom + HALF_LOG_2PI
    e_num = (gamma(mle_depth(zz.numel())) * (ll.abs().sum() + 0.5 * a1) + (FAST_FN * 0.5 * a1 if logs is not None else 0.0)
             + gamma(-(-ld.numel() // 1024) + 22) * ld.abs().sum() + 2 * U * (a0.abs() + 0.5 * a1 + sl.abs()))
    bound = e_num / denom + 2 * U * (num / denom).abs() + U * loss.abs()
    return loss.reshape(1), denom.reshape(1), bound.reshape(1)


def mle_bwd(z, m, logs, gscale, gdenom, B, dtype=F64, defect=None):
    """dz = g e^{-2 logs} (z - m), dm = -dz, dlogs = g (1 - e^{-2 logs} (z - m)^2), dlogdet[b] = -g, g = gscale (/ gdenom when given).
    Returns {"dz" | "dm" | "dlogs" | "dlogdet": (ref, bound)}.  Bounds, elementwise: g one rounding (the division), z - m one, __expf
    FAST_FN relative (only with logs), each product one -> (FAST_FN + 4 U) |dz|; q = e d^2: (FAST_FN + 3 U) q, then 1 - q and the
    product with g: |g| (FAST_FN + 3 U) q + 3 U |dlogs|; dlogdet U |g|.
    defect: "dlogs_no_one" (dlogs without the `1 -` term), "dm_sign" (dm with dz's sign)."""
    zz, mm = _t(z, dtype).reshape(-1), _t(m, dtype).reshape(-1)
    ll = torch.zeros_like(zz) if logs is None else _t(logs, dtype).reshape(-1)
    g = _t(gscale, dtype).reshape(())
    if gdenom is not None:
        g = g / _t(gdenom, dtype).reshape(())
    fast = FAST_FN if logs is not None else 0.0
    e, d = torch.exp(-2 * ll), zz - mm
    v = g * e * d
    q = e * d * d
    dlogs = g * (1 - q)
    if defect == "dlogs_no_one":
        dlogs = -g * q
    bv = (fast + 4 * U) * v.abs()
    return {"dz": (v, bv), "dm": (v if defect == "dm_sign" else -v, bv),
            "dlogs": (dlogs, g.abs() * (fast + 3 * U) * q + 3 * U * dlogs.abs()),
            "dlogdet": ((-g).expand(B).clone(), (U * g.abs()).expand(B).clone())}


# ----------------------------------------------------------------------------- gt_duration_loss_fwd / _bwd
def _dur_parts(logw, w, lens, dtype, defect):
    lw, ww = _t(logw, dtype), _t(w, dtype)
    ln = _i(lens)
    B, Tx = lw.shape
    on = torch.arange(Tx)[None, :] < ln[:, None]
    ref = torch.log(ww if defect == "no_eps" else ww + 1e-8)
    ref = torch.where(on, ref, torch.zeros_like(ref))                 # w on padded tokens is never used
    tot = ln.to(dtype) if defect == "lens_b" else ln.sum().to(dtype).expand(B)
    return lw - ref, tot


def duration_loss(logw, w, lens, dtype=F64, defect=None):
    """l[b] = sum_{t < Tx} (logw[b,t] - log(w[b,t] + 1e-8) [t < lens[b]])^2 / sum(lens)   (models.py:1089-1092), logw, w [B, Tx].
    Contract: logw is ZERO on padded tokens (the predictor masks its output; a non-zero value there is squared into the sum, as in
    the reference), w on padded tokens is ignored (junk allowed).  Returns l [B].
    defect: "lens_b" (sum(lens) replaced by lens[b]), "no_eps" (the 1e-8 omitted: log 0 on a valid token with no frame)."""
    d, tot = _dur_parts(logw, w, lens, dtype, defect)
    return (d * d).sum(1) / tot


def duration_loss_bwd(logw, w, lens, g, dtype=F64, defect=None):
    """dlogw[b,t] = 2 g[b] (logw[b,t] - log(w[b,t] + 1e-8) [t < lens[b]]) / sum(lens), every t < Tx written (same contract)."""
    d, tot = _dur_parts(logw, w, lens, dtype, defect)
    return (2 * _t(g, dtype) / tot)[:, None] * d


# ----------------------------------------------------------------------------- gt_prior_expand / _bwd
def prior_expand(x_m, f2t):
    """z_m[b,c,j] = x_m[b,c,f2t[b,j]], 0 where f2t[b,j] < 0: a gather, exact.  x_m [B, C, Tx], f2t [B, Ty] -> [B, C, Ty]."""
    x = _t(x_m)
    t = _i(f2t)
    g = torch.gather(x, 2, t.clamp_min(0)[:, None, :].expand(-1, x.shape[1], -1))
    return torch.where((t >= 0)[:, None, :], g, torch.zeros_like(g))


def prior_expand_bwd(dz_m, f2t, Tx, dtype=F64, defect=None):
    """dx_m[b,c,i] = sum of dz_m[b,c,j] over the frames j with f2t[b,j] == i (np.add.at); every entry written, tokens without a
    frame get 0.  Returns (ref [B, C, Tx], S = the same sum over |dz_m|, run [B, Tx] = frames per token): bound = gamma(run) S.
    defect: "second_chunk" (of a run that crosses a 64-frame chunk boundary, the part inside the second chunk it touches dropped)."""
    dz = _t(dz_m, dtype)
    t = _i(f2t)
    B, C, Ty = dz.shape
    keep = t >= 0
    if defect == "second_chunk":
        keep = keep.clone()
        for b in range(B):
            for i in torch.unique(t[b][t[b] >= 0]).tolist():
                j = torch.nonzero(t[b] == i).reshape(-1)
                ch = torch.unique(j // 64)
                if ch.numel() >= 2:
                    keep[b, j[(j // 64) == ch[1]]] = False
    idx = t.clamp_min(0)[:, None, :].expand(-1, C, -1)
    src = dz * keep[:, None, :].to(dtype)
    ref = torch.zeros(B, C, Tx, dtype=dtype).scatter_add_(2, idx, src)
    S = torch.zeros(B, C, Tx, dtype=dtype).scatter_add_(2, idx, src.abs())
    run = torch.zeros(B, Tx, dtype=torch.int64).scatter_add_(1, t.clamp_min(0), (t >= 0).long())
    return ref, S, run


# ----------------------------------------------------------------------------- gt_embedding_fwd / _bwd
def embedding_fwd(ids, emb, L, scale, ld, prior=None):
    """rows[base(b) + HALO + t, c] = fp32(emb[ids[b,t], c] * scale) for t < lens[b], c < C; 0 on every other row; columns [C, ld) are
    not written (they keep `prior`, default 0).  One fp32 multiply: exact.  ids [B, T], emb [V, C] -> (fp32 rows [R, ld] as float64,
    the bf16 rows = f2bf of them)."""
    idt = _i(ids).numpy()
    e32 = np.asarray(emb.detach().cpu() if isinstance(emb, torch.Tensor) else emb, dtype=np.float32)
    C = e32.shape[1]
    out = np.zeros((L.R, ld), dtype=np.float32) if prior is None else np.array(prior, dtype=np.float32)
    out[:, :C] = 0
    for b in range(L.B):
        n = min(L.lens[b], L.T)
        out[L.frame_rows(b), :C] = e32[idt[b, :n]] * np.float32(scale)
    full = out.astype(np.float64)
    bf = full.copy()
    bf[:, :C] = bf16_round(out[:, :C])
    return torch.from_numpy(full), torch.from_numpy(bf)


def embedding_bwd(ids, dx, L, scale, V, prior, dtype=F64, defect=None):
    """demb[v, c] = prior[v, c] + sum over the valid tokens (b, t) with ids[b,t] == v of dx[row(b, t), c] * scale (atomics: any order).
    dx [R, ld] (only its first C columns are read), prior [V, C].  Returns (ref, S, count [V]): bound = gamma(count) S, S the sum of
    |dx scale| + |prior|.  defect: "no_scale" (scale omitted), "drop_last" (the last valid token of every utterance dropped)."""
    idt = _i(ids)
    p = _t(prior, dtype)
    C = p.shape[1]
    d = _t(dx, dtype)[:, :C] * (1.0 if defect == "no_scale" else float(np.float32(scale)))
    ref, S, cnt = p.clone(), p.abs().clone(), torch.zeros(V, dtype=torch.int64)
    for b in range(L.B):
        n = min(L.lens[b], L.T) - (1 if defect == "drop_last" else 0)
        rows = torch.from_numpy(L.frame_rows(b)[:n])
        ref.index_add_(0, idt[b, :n], d[rows])
        S.index_add_(0, idt[b, :n], d[rows].abs())
        cnt += torch.bincount(idt[b, :n], minlength=V)
    return ref, S, cnt


# ----------------------------------------------------------------------------- gt_rows_add_cond, gt_rows_utt_sum, gt_length_mask
def rows_add_cond(x, cond, L, rowmask, C):
    """out[m, c] = fp32(x[m, c] + cond[utterance(m), c]) where rowmask[m] != 0, else 0 (c < C): one fp32 add, exact; x holds fp32 or
    bf16 VALUES (rows where rowmask is 0 are not read: they may hold NaN).  Returns (fp32 result as float64 [R, C], its bf16 rounding)."""
    x32 = np.asarray(_t(x, torch.float32).numpy())[:, :C]
    c32 = np.asarray(_t(cond, torch.float32).numpy())
    on = np.asarray(rowmask) != 0
    out = np.zeros((L.R, C), dtype=np.float32)
    out[on] = x32[on] + c32[L.rowbatch[on]]
    return torch.from_numpy(out.astype(np.float64)), torch.from_numpy(bf16_round(out))


def rows_utt_sum(y, L, rowmask, C, prior=None, dtype=F64):
    """out[b, c] = (prior[b, c] +) sum over ALL rows m of utterance b (L.count[b] of them: halos, padding and the rows that round R up
    included) of y[m, c] * rowmask[m]; rowmask None = 1; a row whose rowmask is 0 is not read (it may hold NaN).  Returns (ref [B, C], S):
    bound = gamma(rows of the utterance) S (the fold over waves and the accumulate add are inside gamma's + 4 and rho_out)."""
    yy = _t(y, dtype)[:, :C]
    if rowmask is not None:
        k = _t(rowmask, dtype)[:, None]
        yy = torch.where(k != 0, yy * k, torch.zeros_like(yy))
    idx = torch.from_numpy(L.rowbatch)
    ref = torch.zeros(L.B, C, dtype=dtype).index_add_(0, idx, yy)
    S = torch.zeros(L.B, C, dtype=dtype).index_add_(0, idx, yy.abs())
    if prior is not None:
        ref, S = ref + _t(prior, dtype), S + _t(prior, dtype).abs()
    return ref, S


def length_mask(lengths, T):
    """mask[b, t] = 1 if t < lengths[b] else 0 (commons.sequence_mask as floats), exact"""
    return (torch.arange(T)[None, :] < _i(lengths)[:, None]).to(F64)


# ----------------------------------------------------------------------------- index-only restatements (csrc/flow_ops.hip), all exact
def cast(vals, dst_f32):
    """values a kernel stores through st_any: unchanged into fp32, rounded to nearest even into bf16 (float64 array of the values)"""
    v = np.asarray(vals, dtype=np.float64)
    return v if dst_f32 else bf16_round(v.astype(np.float32))


def rows_from_bct(x, L):
    """rows[m, c] = x[b(m), c, t(m)] for the rows with 0 <= t(m) < T, 0 on every other row (leading halos, and in the uniform layout the
    trailing ones).  Lengths play no part: frames past an utterance's length are copied as they are, so in the ragged layout the
    trailing halo rows and the rows that round R up carry x[b, :, lens[b] ...] — zero when x is zero there, which is what the callers
    pass.  x [B, C, T] float64 values -> [R, C]."""
    x = np.asarray(x, dtype=np.float64)
    out = np.zeros((L.R, x.shape[1]))
    on = (L.rowframe >= 0) & (L.rowframe < L.T)
    out[on] = x[L.rowbatch[on], :, L.rowframe[on]]
    return out


def bct_from_rows(rows, L, lengths=None):
    """x[b, c, t] = rows[base(b) + HALO + t, c] for t < min(lengths[b], T) (and a row < R), 0 beyond; every element written."""
    rows = np.asarray(rows, dtype=np.float64)
    lengths = L.lens if lengths is None else lengths
    out = np.zeros((L.B, rows.shape[1], L.T))
    for b in range(L.B):
        n = min(int(lengths[b]), L.T)
        r = L.base[b] + HALO + np.arange(n)
        r = r[r < L.R]
        out[b, :, :r.size] = rows[r].T
    return out


def squeeze_rows(y, len_sq, L):
    """rows[base(b) + r, p C + c] = y[b, c, 2 t' + p], t' = r - HALO, for 0 <= t' < min(len_sq[b], Ty // 2); 0 on every other row the
    utterance owns (halos, t' >= len_sq[b], the rows that round R up).  An odd trailing frame of y is never read.  y [B, C, Ty] ->
    [R, 2 C]; every row is written."""
    y = np.asarray(y, dtype=np.float64)
    B, C, Ty = y.shape
    out = np.zeros((L.R, 2 * C))
    for b in range(B):
        n = max(0, min(int(len_sq[b]), Ty // 2, int(L.count[b]) - HALO))
        blk = y[b, :, :2 * n].reshape(C, n, 2)                                        # [c, t', p]
        out[L.base[b] + HALO:L.base[b] + HALO + n] = blk.transpose(1, 2, 0).reshape(n, 2 * C)
    return out


def unsqueeze_rows(rows, len_sq, L, Ty):
    """y[b, c, 2 t' + p] = rows[base(b) + HALO + t', p C + c] for t' < min(len_sq[b], Ty // 2); 0 for the frames past 2 len_sq[b]
    and for an odd trailing frame; every element written.  rows [R, 2 C] -> [B, C, Ty]."""
    rows = np.asarray(rows, dtype=np.float64)
    C = rows.shape[1] // 2
    out = np.zeros((L.B, C, Ty))
    for b in range(L.B):
        n = max(0, min(int(len_sq[b]), Ty // 2))
        blk = rows[L.base[b] + HALO:L.base[b] + HALO + n].reshape(n, 2, C)            # [t', p, c]
        out[b, :, :2 * n] = blk.transpose(2, 0, 1).reshape(C, 2 * n)
    return out


def rows_f32_to_bf16(x, rowmask, n):
    """out[m, c] = bf16(fp32(x[m, c] * rowmask[m])), rowmask None = 1, c < n (values as float64)"""
    x32 = np.asarray(x, dtype=np.float32)[:, :n]
    if rowmask is not None:
        x32 = x32 * np.asarray(rowmask, dtype=np.float32)[:, None]
    return bf16_round(x32)


def rows_add_bf16(dx, add, n):
    """dx[m, c] = fp32(dx[m, c] + add[m, c]), add the VALUES of the bf16 rows, c < n: one fp32 add, exact"""
    return (np.asarray(dx, dtype=np.float32)[:, :n] + np.asarray(add, dtype=np.float32)[:, :n]).astype(np.float64)
