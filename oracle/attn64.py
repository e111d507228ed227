"""TEST INFRASTRUCTURE ONLY — float64 restatement of gt_attn_fwd / gt_attn_bwd (csrc/attn_mfma.hip, csrc/encoder_ops.hip), for the
checking rule of oracle/rows64.py:  |got - ref| <= bound + rho_out |ref|,  an aggregate limit, a planted defect that must miss.

Every operator works on ONE (utterance, head): q, k, v, dO are [T, D] float64 (the kernel's own bf16 rows, see `utt_rows`), Ek, Ev
[2 win + 1, D], P and everything derived from it [T, T] (query i, key j).  It returns (ref, S) with S the absolute-value twin of the
sum it restates, or (ref, bound) where the bound is not one plain sum.  The callers map utterances and heads.

The checks are TEACHER-FORCED: each one starts from what the kernel itself stored one step earlier (P; the workspace), so no
tolerance compounds.  The reference therefore has to use the kernel's own operands, and the two kernel families round differently:

  MFMA path (gt_attn_mfma_shape(T, D, win) == 1)                       generic path
    Ek, Ev are rounded to bf16 when staged in LDS                         Ek, Ev stay fp32
    P' = bf16(fp32(P keep scale)) feeds P' V and band(P') Ev              P' = fp32(P keep scale)
    bf16(dS) and bf16(P') leave pass 1 (the workspace: dS^T then P'^T,    dS is the fp32 [B,H,T,T] workspace; pass 2 rebuilds P'
    [B,H,T(j),TI(i)], TI = ceil(T/32) 32) and feed dQ, dK, dV, dEk, dEv   from P
  `operands(Ek, mfma)` and `drop(P, keep, scale, fmt)` restate these roundings exactly (bit for bit).

The operation (include/glowtts_hip.h), rel = j - i + win, band = [0 <= rel <= 2 win]:
  s[i,j]  = (q_i.k_j + band q_i.Ek[rel]) / sqrt(D);   -1e4 where j >= len or i >= len        scores
  P       = softmax_j(s)   (a padded query row: all scores -1e4, so 1/T over all T keys)       softmax_rows
  P'      = P keep scale,  keep = drop_keep(seed, (b H + h) T + i, j, thresh32(p))             drop / keep_mask
  out_i   = sum_j P'[i,j] v_j + sum_band P'[i,j] Ev[rel]                                       out
  dPd     = dO V^T + band(dO Ev^T);  dP = keep scale dPd;  Dsum_i = sum_j dP P                 ds
  dS      = P (dP - Dsum) / sqrt(D), zero where masked;   Pd_bwd = P' with rows i >= len zero  ds / pd_bwd
  dQ      = dS K + band(dS) Ek;   dK = dS^T Q;   dV = Pd_bwd^T dO                              dq / dk / dv
  dEk[r]  = sum_i dS[i, i+r-win] q_i;   dEv[r] = sum_i Pd_bwd[i, i+r-win] dO_i                 band_grad, summed over (b, h) and
                                                                                               added to the destination: accumulate

Bounds (derived, not fitted; u = 2^-24, gamma(K) = (K + 4) 2^-23 the fp32 accumulation of K terms in ANY order, rows64.gamma):
  every sum is bounded by gamma(K) S with K = the number of terms the kernel adds (`terms`):
    a product of two bf16 numbers is exact in fp32 (16 significant bits), so on the MFMA path K = the number of products; a product
    with an fp32 factor (fp32 Ek / Ev, fp32 P' / dS on the generic path) rounds once more, so K = twice the number of products.
    scores   q.k (D) + q.Ek (D) + the add of the two, rsqrtf(D) (1 ulp of the value + its own representation) and the multiply (4)
    out      T keys + 2 win + 1 band terms                      dPd     D + D + the add
    dQ       T + 2 win + 1            dK, dV   T (the MFMA kernel adds TI - T zeros more: no error)
    dEk, dEv every (utterance, head, query) contributes one product per diagonal; the MFMA kernel sums 32 queries in one MFMA chain,
             adds the waves' results into the workgroup's LDS table with atomics and the tables into the destination with atomics,
             the generic one adds products to the LDS table one by one: K = B H (T + waves + workgroups) + 1 (the prior value).
             The order of the atomics is arbitrary; gamma(K) S holds for every order.
  softmax  exp(s_l - m) as the kernel evaluates it = exp(s_l - m)(1 + d_l),
             d_l = e_s[l] (the score's own bound: exp turns an absolute error of its argument into a relative one of its value)
                   + 4 u |s_l - m| (the subtraction; __expf's multiply by its fp32 log2(e), twice u) + FAST_FN (v_exp_f32).
           The value of m cancels in the ratio.  P_j = w_j / sum_l w_l, so to first order
             |dP_j| <= P_j (d_j + sum_l P_l d_l + gamma(T) [the denominator's T-term sum] + resc (FAST_FN + 2 u) + FAST_FN + 2 u)
           with FAST_FN + 2 u for the reciprocal and the final multiply, and resc = the rescales exp(m_old - m_new) of the running
           denominator (the long forward's online pass: one per key tile + the merge of the two lane halves; 0 elsewhere).
           Masked keys of a valid query have exp(-1e4 - m) = 0 in fp32 and in float64 alike.
  dS       dP = keep scale dPd: e_dP = keep scale e_dPd + u |dP|;
           Dsum: products dP P rounded, T-term sum: e_D = sum_j e_dP P + gamma(2 T) sum_j |dP P|;
           t = dP - Dsum, P t, the multiply by rsqrtf(D): e_dS = (P (e_dP + e_D) + 5 u P (|dP| + |Dsum|)) / sqrt(D)
           (|t| <= |dP| + |Dsum| keeps the bound safe under cancellation).
rows64.check adds the output's own rho (2^-8 |ref| for bf16, 2^-24 |ref| for fp32).
"""
import math

import numpy as np
import torch

from oracle import dropmask
from oracle.rows64 import FAST_FN, RHO, bf16_round, gamma, t64

U = RHO["f32"]
MASKED = -1e4


# ----------------------------------------------------------------------------- operands as the kernel holds them
def utt_rows(X, rbase, n_own, T):
    """The kernel's [T, n] rows of one utterance from the rows matrix X [R, n]: frame t is row rbase + min(t, nv1), nv1 = n_own -
    HALO - 1 the trailing halo row (ragged layout: frames past the utterance's own rows read that zero row; rbase already holds
    the leading HALO).  n_own: rows the utterance owns (Tp, or row0[b + 1] - row0[b])."""
    from glow_tts_amd import ops
    nv1 = n_own - ops.HALO - 1
    idx = rbase + torch.clamp(torch.arange(T), max=nv1)
    return t64(X)[idx]


def operands(E, mfma):
    """Ek / Ev as the path reads them: bf16-rounded on the MFMA path, fp32 on the generic one"""
    E = t64(E)
    return torch.from_numpy(bf16_round(E.numpy())) if mfma else E


def keep_mask(seed, b, h, H, T, p, col_shift=0):
    """bool [T, T] keep of (utterance b, head h), or None for p == 0; col_shift = 1: the planted defect (column j + 1 hashed)"""
    if not p:
        return None
    rows = ((b * H + h) * T + np.arange(T))[:, None]
    return torch.from_numpy(dropmask.drop_keep(seed, rows, np.arange(T)[None, :] + col_shift, dropmask.thresh32(p)))


def drop(P, keep, scale, fmt="f64"):
    """P' = P keep scale [T, T] float64.  fmt "f64": exact; "f32": the fp32 product (generic path); "bf16": bf16(fp32 product) (MFMA
    path) — for the last two P must hold fp32 values (the kernel's saved P), and the result is the kernel's P' bit for bit."""
    P = t64(P)
    if fmt == "f64":
        return P if keep is None else P * keep * float(scale)
    x = P.numpy().astype(np.float32)
    if keep is not None:
        x = np.where(keep.numpy(), x * np.float32(scale), np.float32(0))
    return torch.from_numpy(bf16_round(x) if fmt == "bf16" else x.astype(np.float64))


# ----------------------------------------------------------------------------- the band
def _rel(T, win):
    i = torch.arange(T)
    rel = i[None, :] - i[:, None] + win
    return rel, (rel >= 0) & (rel <= 2 * win)


def band_gather(W, T, win, skip=None):
    """W [T, 2 win + 1] -> M [T, T], M[i, j] = W[i, j - i + win] inside the band, 0 outside; skip: that diagonal left out"""
    rel, inb = _rel(T, win)
    if skip is not None:
        inb = inb & (rel != skip)
    return torch.gather(W, 1, rel.clamp(0, 2 * win)) * inb


def band_scatter(M, win, skip=None):
    """M [T, T] -> W [T, 2 win + 1], W[i, r] = M[i, i + r - win] (0 where that key does not exist)"""
    T = M.shape[0]
    rel, inb = _rel(T, win)
    if skip is not None:
        inb = inb & (rel != skip)
    return torch.zeros(T, 2 * win + 1, dtype=M.dtype).scatter_add_(1, rel.clamp(0, 2 * win), M * inb)


def valid(length, T):
    """bool [T, T]: query i < len and key j < len"""
    ok = torch.arange(T) < length
    return ok[:, None] & ok[None, :]


# ----------------------------------------------------------------------------- term counts
def terms(mfma, T, D, win, B=1, H=1):
    """K of every sum (module docstring).  An fp32 factor doubles the count (the product itself rounds)."""
    NW = 2 * win + 1
    f = 1 if mfma else 2
    waves = -(-T // 32) if mfma else 0
    groups = -(-T // 128) if mfma else -(-T // 16)                  # upper bound for the 2-wave backward: ceil(T / 64) <= waves
    return {"scores": D + f * D + 4, "out": f * (T + NW), "dpd": D + f * D + 1, "dq": f * (T + NW), "dk": f * T, "dv": f * T,
            "dE": B * H * (f * T + 2 * waves + groups) + 1}


# ----------------------------------------------------------------------------- forward
def scores(q, k, Ek, length, T, win=4, drop_diag=None):
    """(s, S) [T, T]: masked, scaled scores and their |.| twin (0 where masked: -1e4 is exact).  drop_diag: planted defect, that
    diagonal of the Ek term left out."""
    q, k, Ek = t64(q), t64(k), t64(Ek)
    isq = 1.0 / math.sqrt(q.shape[1])
    s = (q @ k.T + band_gather(q @ Ek.T, T, win, drop_diag)) * isq
    S = (q.abs() @ k.abs().T + band_gather(q.abs() @ Ek.abs().T, T, win)) * isq
    ok = valid(length, T)
    return torch.where(ok, s, torch.full_like(s, MASKED)), S * ok


def softmax_rows(s, e_s, rescales=0):
    """(P, bound) from the scores and their bound e_s = gamma(K) S (module docstring, `softmax`)"""
    m = s.max(1, keepdim=True).values
    P = torch.softmax(s, 1)
    d = e_s + 4 * U * (s - m).abs().clamp(max=104.0) + FAST_FN     # fp32 exp is 0 below -104: larger arguments carry no error
    rel = d + (P * d).sum(1, keepdim=True) + gamma(s.shape[1]) + (rescales + 1) * (FAST_FN + 2 * U)
    return P, P * rel + 2.0 ** -126                                 # results below the smallest normal fp32 may be flushed to 0


def out(Pd, v, Ev, win=4, drop_diag=None):
    """(O, S) [T, D] from P' (drop()), v and Ev; drop_diag: that diagonal of the Ev term left out"""
    Pd, v, Ev = t64(Pd), t64(v), t64(Ev)
    O = Pd @ v + band_scatter(Pd, win, drop_diag) @ Ev
    S = Pd.abs() @ v.abs() + band_scatter(Pd.abs(), win) @ Ev.abs()
    return O, S


# ----------------------------------------------------------------------------- backward
def pd_bwd(Pd, length):
    """P' with the rows of padded queries zero: they carry no upstream gradient whatever dout holds"""
    Pd = t64(Pd)
    return Pd * (torch.arange(Pd.shape[0]) < length)[:, None]


def ds(P, dO, v, Ev, keep, scale, length, K_dpd, win=4, drop_diag=None):
    """(dS, bound) [T, T] from the saved P (module docstring, `dS`); K_dpd = terms()["dpd"].  drop_diag: that diagonal of the Ev
    term of dPd left out."""
    P, dO, v, Ev = t64(P), t64(dO), t64(v), t64(Ev)
    T, D = dO.shape
    dPd = dO @ v.T + band_gather(dO @ Ev.T, T, win, drop_diag)
    e = gamma(K_dpd) * (dO.abs() @ v.abs().T + band_gather(dO.abs() @ Ev.abs().T, T, win))
    ks = torch.ones_like(P) if keep is None else keep * float(scale)
    dP = dPd * ks
    e_dP = e * ks + U * dP.abs()
    Dsum = (dP * P).sum(1, keepdim=True)
    e_D = (e_dP * P).sum(1, keepdim=True) + gamma(2 * T) * (dP * P).abs().sum(1, keepdim=True)
    isq = 1.0 / math.sqrt(D)
    ok = valid(length, T)
    dS = P * (dP - Dsum) * isq * ok
    bound = (P * (e_dP + e_D) + 5 * U * P * (dP.abs() + Dsum.abs())) * isq * ok
    return dS, bound


def dq(dS, k, Ek, win=4, drop_diag=None):
    """(dQ, S) [T, D] from the workspace's dS; drop_diag: that diagonal of the Ek term left out"""
    dS, k, Ek = t64(dS), t64(k), t64(Ek)
    return dS @ k + band_scatter(dS, win, drop_diag) @ Ek, dS.abs() @ k.abs() + band_scatter(dS.abs(), win) @ Ek.abs()


def _without_row(M, i):
    if i is None:
        return M
    M = M.clone()
    M[i] = 0
    return M


def dk(dS, q, drop_query=None):
    """(dK, S) [T, D] = dS^T Q; drop_query: planted defect, that query row left out of the sum"""
    dS, q = _without_row(t64(dS), drop_query), t64(q)
    return dS.T @ q, dS.abs().T @ q.abs()


def dv(Pdb, dO, drop_query=None):
    """(dV, S) [T, D] = Pd_bwd^T dO"""
    return dk(Pdb, dO, drop_query)


def band_grad(M, x, win=4, drop_diag=None):
    """(dE, S) [2 win + 1, D] of one (utterance, head): dE[r] = sum_i M[i, i + r - win] x_i — dEk from (dS, q), dEv from (Pd_bwd, dO);
    drop_diag: that diagonal's row left out"""
    M, x = t64(M), t64(x)
    return band_scatter(M, win, drop_diag).T @ x, band_scatter(M.abs(), win).T @ x.abs()


def accumulate(parts, prior, K):
    """Sum of the per-(utterance, head) (dE, S) pairs onto the destination's prior contents -> (ref, bound)"""
    ref, S = t64(prior).clone(), t64(prior).abs()
    for r, s in parts:
        ref, S = ref + r, S + s
    return ref, gamma(K) * S


# ----------------------------------------------------------------------------- the checks of one gt_attn_fwd + gt_attn_bwd call
def _check(name, got, ref, bound, bads, kind, log):
    """rows64.check_with_control once per planted defect {label: bad reference}: the rule holds, every defect misses by >= 3x"""
    from oracle import rows64
    rep = None
    for label, bad in bads.items():
        rep = rows64.check_with_control(f"{name} <{label}>", got, ref, bound, bad, kind=kind, log=log)
    return rep


def check_case(tag, c, got, mfma, rescales=0, log=print):
    """Every teacher-forced check of one forward + backward call.
    c: namespace with B, H, T, D, win, lens [B], p, seed (the hashed seed: host seed XOR device word), q, k, v, dO ([B][H] lists of
       [T, D] float64: the kernel's own rows, utt_rows), Ek, Ev, prior_dEk, prior_dEv (fp32) and own [B] (query / key rows 0 .. own[b] - 1
       of utterance b are stored: min(T, rows behind rbase up to the trailing halo row)).
    got: P [B, H, T, T] fp32; out, dq, dk, dv [B, H, T, D] (bf16 values; rows >= own[b] are not looked at); dS [B, H, T(i), T(j)] the
       workspace's dS (bf16 values on the MFMA path, fp32 on the generic one); Pd the workspace's P' (MFMA path; None on the generic
       one, whose pass 2 rebuilds fp32 P' from P); dEk, dEv [2 win + 1, D] fp32.
    Returns {check name: rows64.Report}."""
    from oracle.rows64 import drop_row
    B, H, T, D, win = c.B, c.H, c.T, c.D, c.win
    K = terms(mfma, T, D, win, B, H)
    Ek, Ev = operands(c.Ek, mfma), operands(c.Ev, mfma)
    fmt = "bf16" if mfma else "f32"
    sc = dropmask.scale(c.p) if c.p else 1.0
    edge = (max(0, win - (T - 1)), min(2 * win, win + T - 1))         # the outermost diagonals that exist: 0 and 2 win from T = win + 1 on
    names = ("P", "out", "dS", "Pd", "dq", "dk", "dv")
    acc = {n: {"got": [], "ref": [], "bound": [], "bad": {}} for n in names}
    dE = {n: {"parts": [], "bad": [[] for _ in edge]} for n in ("dEk", "dEv")}

    def put(n, g, ref, bound, bads, rows=None):
        sel = (lambda x: x) if rows is None else (lambda x: x[:rows])
        a = acc[n]
        a["got"].append(sel(t64(g)).reshape(-1)); a["ref"].append(sel(ref).reshape(-1)); a["bound"].append(sel(bound).reshape(-1))
        for label, bad in bads.items():
            a["bad"].setdefault(label, []).append(sel(bad).reshape(-1))

    for b in range(B):
        n, own = int(c.lens[b]), int(c.own[b])
        for h in range(H):
            q, k, v, dO = c.q[b][h], c.k[b][h], c.v[b][h], c.dO[b][h]
            keep, keep1 = keep_mask(c.seed, b, h, H, T, c.p), keep_mask(c.seed, b, h, H, T, c.p, col_shift=1)
            # 1. P from the kernel's q, k, Ek
            s, S = scores(q, k, Ek, n, T, win)
            Pr, Pb = softmax_rows(s, gamma(K["scores"]) * S, rescales)
            put("P", got["P"][b, h], Pr, Pb, {f"Ek diagonal {r} dropped": torch.softmax(scores(q, k, Ek, n, T, win, drop_diag=r)[0], 1)
                                             for r in edge})
            # 2. out from the kernel's own P
            Pk = got["P"][b, h]
            Pd = drop(Pk, keep, sc, fmt)
            O, SO = out(Pd, v, Ev, win)
            v0 = drop_row(v, 0)
            bads = {f"Ev diagonal {r} dropped": out(Pd, v, Ev, win, drop_diag=r)[0] for r in edge}
            bads["V row 0 zeroed"] = out(Pd, v0, Ev, win)[0]
            if c.p:
                bads["dropout column + 1"] = out(drop(Pk, keep1, sc, fmt), v, Ev, win)[0]
            put("out", got["out"][b, h], O, gamma(K["out"]) * SO, bads, own)
            # 3. the workspace from the kernel's P, v, Ev, dO
            dSr, dSb = ds(Pk, dO, v, Ev, keep, sc, n, K["dpd"], win)
            bads = {f"Ev diagonal {edge[0]} dropped from dPd": ds(Pk, dO, v, Ev, keep, sc, n, K["dpd"], win, drop_diag=edge[0])[0],
                    "V row 0 zeroed": ds(Pk, dO, v0, Ev, keep, sc, n, K["dpd"], win)[0]}
            if c.p:
                bads["dropout column + 1"] = ds(Pk, dO, v, Ev, keep1, sc, n, K["dpd"], win)[0]
            put("dS", got["dS"][b, h], dSr, dSb, bads)
            Pdb = pd_bwd(Pd, n)
            if mfma:
                bad = pd_bwd(drop(Pk, keep1, sc, fmt), n) if c.p else drop_row(Pdb, 0)
                put("Pd", got["Pd"][b, h], Pdb, torch.zeros_like(Pdb), {"dropout column + 1" if c.p else "query row 0 dropped": bad})
            # 4. dq, dk, dv, dEk, dEv from the workspace's own values
            dSw = t64(got["dS"][b, h])
            Pdw = t64(got["Pd"][b, h]) if mfma else Pdb
            r_, s_ = dq(dSw, k, Ek, win)
            put("dq", got["dq"][b, h], r_, gamma(K["dq"]) * s_, {f"Ek diagonal {r} dropped": dq(dSw, k, Ek, win, drop_diag=r)[0] for r in edge}, own)
            r_, s_ = dk(dSw, q)
            put("dk", got["dk"][b, h], r_, gamma(K["dk"]) * s_, {"query row 0 dropped": dk(dSw, q, drop_query=0)[0]}, own)
            r_, s_ = dv(Pdw, dO)
            put("dv", got["dv"][b, h], r_, gamma(K["dv"]) * s_, {"query row 0 dropped": dv(Pdw, dO, drop_query=0)[0]}, own)
            for nm, M, x in (("dEk", dSw, q), ("dEv", Pdw, dO)):
                dE[nm]["parts"].append(band_grad(M, x, win))
                for e, r in enumerate(edge):
                    dE[nm]["bad"][e].append(band_grad(M, x, win, drop_diag=r))

    reports = {}
    kinds = {"P": "f32", "out": "bf16", "dS": "bf16" if mfma else "f32", "Pd": "bf16", "dq": "bf16", "dk": "bf16", "dv": "bf16"}
    for n in names:
        a = acc[n]
        if a["got"]:
            reports[n] = _check(f"{tag} {n}", torch.cat(a["got"]), torch.cat(a["ref"]), torch.cat(a["bound"]),
                                {label: torch.cat(v) for label, v in a["bad"].items()}, kinds[n], log)
    for nm, prior in (("dEk", c.prior_dEk), ("dEv", c.prior_dEv)):
        ref, bound = accumulate(dE[nm]["parts"], prior, K["dE"])
        reports[nm] = _check(f"{tag} {nm}", got[nm], ref, bound,
                             {f"diagonal {r} dropped": accumulate(dE[nm]["bad"][e], prior, K["dE"])[0] for e, r in enumerate(edge)}, "f32", log)
    return reports
