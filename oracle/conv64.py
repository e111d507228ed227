"""TEST INFRASTRUCTURE ONLY — float64 restatement of gt_conv_gemm_bf16 (csrc/conv_gemm.hip + csrc/conv_common.h), the whole entry
point in the order its epilogues apply it, under the rule of oracle/rows64.py:

    |got - ref| <= gamma_K * S + eps_epi + rho_out * |ref|        (rho_out * |ref| is added by rows64.check)

An operation is a dict `op` of CPU operands — the kernel's OWN operands: the bf16 rows it reads, the weights decoded from the image
it reads, the exact keep masks of oracle/dropmask.py:

    X [R, Cin], W [taps][N][Cin]   float64 values of the bf16 operands, W in the GEMM's convention with the gate interleave undone
                                   (a data gradient: rows64.conv_rows_dgrad_weights of the decoded image; bf16x3: the decoded
                                   [w_hi; w_lo; w_hi] image against [x_hi | x_hi | x_lo] rows, K = 3 Cin, operands taken as given)
    edge                           "zero": rows outside [0, R) read as zero (the definition of rows64.conv_rows);
                                   "clamp": the row index is clamped into [0, R-1] (what both kernels do: ldx1 / load_stage).
                                   They agree when the first and last taps/2 rows of X are zero — the precondition of the entry.
    bias [N], cond [B or R, >= N], utt [R] (row of `cond` every row reads: row_utt), relu, keep / scale (dropout), addend [R, N],
    rowmask [R], gate 0..3, T / S [R, N] (gate 2: the SAVED bf16 halves), ysaved [R, N] uint16 bits (gate 3), out "bf16" | "f32".

run(op) -> ({output: (ref, bound)}, amb);  run(op, torch.float32) -> the float32 twin's outputs (same order of operations, fp32
arithmetic, outputs rounded as the kernel rounds them): tests/test_conv64.py requires the twin to pass every bound.

Bounds (u = 2^-24, one fp32 rounding; K = taps * Cin products):

  acc     e = gamma_K * S, S = sum |x| |w| + |bias| + |cond|: K products accumulated in any order plus the two epilogue adds
          (gamma_K = (K + 4) u * 2 covers K + 4 roundings).
  relu    1-Lipschitz: e carries over.  An element whose float64 pre-activation lies within e of 0 may take either branch; with a
          later mask or scale its error is still inside the bound, but it is SET ASIDE (amb) so that no check depends on the
          branch.  At most AMB_CAP of a case's elements may be set aside (tests/test_conv64.py proves the cap for every case).
  drop    the keep mask is restated exactly (no ambiguity); v * scale rounds once: e = e * scale + u |v * scale|.
  addend  one add: e = e + u |v + addend|.  rowmask is 0 / 1: exact.
  gate 1  rows64.gate_fwd: cond is added AFTER the dropout, keep masks from drop_keep_gate (16-bit threshold).
  gate 2  d = (acc + addend) * rowmask with e_d as above, then rows64.gate_bwd with the saved T / S and the replayed keep masks.
  gate 3  (acc + addend) * rowmask * scale where the saved y is not +-0 (bits & 0x7fff), else exactly 0.

Aggregates and the control factor are the project's (rows64.AGG_F32, AGG_BF16, CONTROL_MISS)."""
import numpy as np
import torch

from oracle import rows64 as R64
from oracle.rows64 import RHO, gamma, t64

AMB_CAP = 0.005
F64 = torch.float64


def row_utt(R, B, Tp=1, row0=None):
    """csrc/common.h gt_row_batch for every row: the row of `cond` that row m reads (B == 0: per-row cond, m itself)."""
    m = np.arange(R, dtype=np.int64)
    if B == 0:
        return m
    if row0 is None:
        return m // Tp
    r0 = np.asarray(row0, dtype=np.int64)[:B]
    return np.clip(np.searchsorted(r0, m, side="right") - 1, 0, B - 1)


def shift_rows(X, s, edge):
    if edge == "zero":
        return R64.shift_rows(X, s)
    assert edge == "clamp", edge
    R = X.shape[0]
    return X[(torch.arange(R) + s).clamp(0, R - 1)]


def acc(X, W, edge="zero", dt=F64):
    """(Y, S): Y[m, n] = sum_tap sum_ci X[m + tap - k/2, ci] W[tap][n][ci] and its |.| twin (S only in float64)."""
    X, W = t64(X).to(dt), t64(W).to(dt)
    taps = W.shape[0]
    Y = torch.zeros(X.shape[0], W.shape[1], dtype=dt)
    S = torch.zeros_like(Y) if dt == F64 else None
    for t in range(taps):
        Xs = shift_rows(X, t - taps // 2, edge)
        Y += Xs @ W[t].T
        if S is not None:
            S += Xs.abs() @ W[t].abs().T
    return Y, S


def _round(v, kind, dt):
    """the twin's output rounding; the float64 reference stays exact"""
    if dt == F64:
        return v
    return torch.from_numpy(R64.bf16_round(v.numpy())) if kind == "bf16" else v.double()


def run(op, dt=F64):
    u = RHO["f32"]
    ref = dt == F64
    X, W = op["X"], op["W"]
    K = W.shape[0] * W.shape[2]
    N = W.shape[1]
    gate = op.get("gate", 0)
    kind = op.get("out", "bf16")
    c = lambda x: t64(x).to(dt)
    Y, S = acc(X, W, op.get("edge", "zero"), dt)
    if op.get("bias") is not None:
        b = c(op["bias"])
        Y = Y + b
        if ref:
            S = S + b.abs()
    cond = None
    if op.get("cond") is not None:
        cond = c(op["cond"])[torch.from_numpy(np.asarray(op["utt"], dtype=np.int64))][:, :N]
    scale = float(op.get("scale", 1.0))
    amb = torch.zeros(Y.shape[0], N, dtype=torch.bool)

    if gate == 1:
        H = N // 2
        keep = op.get("keep")
        if ref:
            outs, _ = R64.gate_fwd(Y, S, K, H, cond=cond, keep=keep, scale=scale)
            return {"y": outs["acts"], "t": outs["t"], "s": outs["s"]}, amb[:, :H]
        if keep is not None:
            Y = Y * (torch.cat([torch.from_numpy(keep[0]), torch.from_numpy(keep[1])], 1).to(dt) * np.float32(scale))
        if cond is not None:
            Y = Y + cond
        T, Sg = torch.tanh(Y[:, :H]), torch.sigmoid(Y[:, H:])
        return {"y": _round(T * Sg, "bf16", dt), "t": _round(T, "bf16", dt), "s": _round(Sg, "bf16", dt)}, amb[:, :H]

    if cond is not None:
        Y = Y + cond
        if ref:
            S = S + cond.abs()
    e = gamma(K) * S if ref else None
    if op.get("relu"):
        if ref:
            amb = Y.abs() <= e
        Y = torch.relu(Y)
    if op.get("keep") is not None and gate == 0:
        k = torch.from_numpy(np.asarray(op["keep"])).to(dt) * (scale if ref else np.float32(scale))
        Y = Y * k
        if ref:
            e = e * k + u * Y.abs()
    if op.get("addend") is not None:
        Y = Y + c(op["addend"])
        if ref:
            e = e + u * Y.abs()
    if op.get("rowmask") is not None:
        rm = c(op["rowmask"])[:, None]
        Y = Y * rm
        if ref:
            e = e * rm
    if gate == 3:
        nz = torch.from_numpy((np.asarray(op["ysaved"]).astype(np.uint16) & 0x7FFF) != 0)
        Y = torch.where(nz, Y * (scale if ref else np.float32(scale)), torch.zeros_like(Y))
        if ref:
            e = torch.where(nz, e * scale + u * Y.abs(), torch.zeros_like(e))
        return {"y": (Y, e) if ref else _round(Y, "bf16", dt)}, amb
    if gate == 2:
        keep = op.get("keep")
        if ref:
            _, _, d, bd = R64.gate_bwd(Y, e, op["T"], op["S"], keep=keep, scale=scale)
            return {"y": (d, bd)}, torch.cat([amb, amb], 1)
        T, Sg = c(op["T"]), c(op["S"])
        d = torch.cat([Y * Sg * (1 - T * T), Y * T * Sg * (1 - Sg)], 1)
        if keep is not None:
            d = d * (torch.cat([torch.from_numpy(keep[0]), torch.from_numpy(keep[1])], 1).to(dt) * np.float32(scale))
        return {"y": _round(d, "bf16", dt)}, torch.cat([amb, amb], 1)
    return {"y": (Y, e) if ref else _round(Y, kind, dt)}, amb


# ----------------------------------------------------------------------------- planted defects (they change numbers, never addresses)
def with_defect(op, name, bm=64):
    """A copy of `op` with one planted defect; `name`:
      weight_col   a zeroed weight column at an edge tap (tap 0, one input channel, every output)
      weight_mid   the same at the centre tap (a single one-frame utterance: its edge taps read halo rows only)
      row_above    a zeroed input row at m0 - 1 for the row tile that starts at m0 = 2 bm: the last row of the tile before it, which
                   the tile at m0 fetches through its taps.  Only output rows >= m0 of the planted reference carry the defect
      row_below    a zeroed input row at m0 + bm = 2 bm for the row tile [bm, 2 bm): the first row of the next tile, which this tile
                   fetches through its taps.  Only output rows < 2 bm of the planted reference carry the defect
                   (edge_row / splice_other_tile.  The edge is 2 bm because an utterance ends on the first edge bm, where the rows
                   are halo rows with nothing to zero; taps >= 3 and data at the row are asserted)
      cond_utt     cond taken from the neighbouring utterance
      keep_bit     one flipped keep bit per row
      no_addend    the addend dropped
    (`last_half`, the second 4-channel half of the last chunk left out, acts on the reference: drop_last_half)."""
    op = dict(op)
    R = op["X"].shape[0]
    if name in ("weight_col", "weight_mid"):
        W = t64(op["W"]).clone()
        W[0 if name == "weight_col" else W.shape[0] // 2, :, W.shape[2] // 5] = 0
        op["W"] = W
    elif name in ("row_above", "row_below"):
        m = edge_row(name, bm)
        X = t64(op["X"])
        assert m + 2 < R and bool((X[m] != 0).any()), f"row {m} holds no data: nothing to plant"
        assert t64(op["W"]).shape[0] >= 3, "a 1-tap conv reads no row of the neighbouring tile"
        op["X"] = R64.drop_row(X, m)
    elif name == "cond_utt":
        utt = np.asarray(op["utt"], dtype=np.int64)
        n = t64(op["cond"]).shape[0]
        op["utt"] = (utt + 1) % n
    elif name == "keep_bit":
        if isinstance(op["keep"], tuple):
            kt, ks = (np.array(k, copy=True) for k in op["keep"])
            j = np.arange(R) % kt.shape[1]
            kt[np.arange(R), j] ^= True
            ks[np.arange(R), j] ^= True
            op["keep"] = (kt, ks)
        else:
            k = np.array(op["keep"], copy=True)
            k[np.arange(R), np.arange(R) % k.shape[1]] ^= True
            op["keep"] = k
    elif name == "no_addend":
        op["addend"] = None
    else:
        raise KeyError(name)
    return op


def drop_last_half(refs):
    """the reference with the last four channels of every output left out (zero): what a skipped second half of the last 8-channel
    chunk (N % 8 == 0), or a skipped half chunk (N % 8 == 4), leaves behind"""
    out = {}
    for k, (r, b) in refs.items():
        r = r.clone()
        r[:, -4:] = 0
        out[k] = (r, b)
    return out


def edge_row(name, bm):
    """the input row a row defect zeroes: the last row of the tile [bm, 2 bm) (row_above) or the first row of the tile at 2 bm"""
    return 2 * bm - 1 if name == "row_above" else 2 * bm


def splice_other_tile(name, bm, refs, bad):
    """the planted reference of a row defect: the defect's values on the output rows of the OTHER tile only (the tile that does not
    own the zeroed row and reads it through its taps), the true reference elsewhere — the control is then missed only by a check that
    sees what a tile fetches across its edge"""
    out = {}
    for k, (r, b) in refs.items():
        r = r.clone()
        if name == "row_above":
            r[2 * bm:] = bad[k][0][2 * bm:]
        else:
            r[:2 * bm] = bad[k][0][:2 * bm]
        out[k] = (r, b)
    return out


def references(op, defects=(), bm=64):
    """-> (refs, amb, {defect: refs}) in float64"""
    refs, amb = run(op)
    bads = {}
    for d in defects:
        if d == "last_half":
            bads[d] = drop_last_half(refs)
        elif d in ("row_above", "row_below"):
            bads[d] = splice_other_tile(d, bm, refs, run(with_defect(op, d, bm))[0])
        else:
            bads[d] = run(with_defect(op, d, bm))[0]
    return refs, amb, bads


def kinds(op):
    return {"y": "bf16" if op.get("gate", 0) else op.get("out", "bf16"), "t": "bf16", "s": "bf16"}


def rule(name, op, got, refs, amb, bads, log=print):
    """rows64.check_with_control on every output of one case (ambiguous ReLU elements set aside, at most AMB_CAP of them): the rule
    must hold and every planted defect must miss it by >= CONTROL_MISS, on every output.  Returns {output: Report} and
    {defect: its smallest miss over the outputs}."""
    share = float(amb.double().mean()) if amb.numel() else 0.0
    assert share <= AMB_CAP, f"{name}: {100 * share:.3g} % of the elements are ReLU-ambiguous (cap {100 * AMB_CAP:g} %)"
    kd = kinds(op)

    def aside(x):
        x = t64(x).clone()
        if bool(amb.any()):
            x[amb] = 0
        return x

    reports = {}
    for k, (r, b) in refs.items():
        planted = {d: (aside(bad[k][0]), aside(bad[k][1])) for d, bad in bads.items()}
        reports[k] = R64.check_with_control(f"{name} {k}", aside(got[k]), aside(r), aside(b), planted, kind=kd[k], log=log)
    if bool(amb.any()):
        log(f"{name}: {int(amb.sum())} ReLU-ambiguous elements set aside")
    return reports, {d: min(rep.misses[d] for rep in reports.values()) for d in bads}
