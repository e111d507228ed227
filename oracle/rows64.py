"""TEST INFRASTRUCTURE ONLY — float64 restatement of the decoder kernels' contracts, and the one rule every fp64 test checks with.

The kernels round their operands to bf16 and accumulate in fp32.  A test here feeds this module the kernel's OWN bf16 operands
(decoded weight images, the rows it read) and compares the kernel's result with the exact float64 value of the same operation:

    elementwise, every row m < R (masked rows included):   |got - ref| <= gamma_K * S + eps_epi + rho_out * |ref|

  gamma_K = (K + 4) 2^-23    worst-case fp32 accumulation of K terms in any order (K products, plus the few sums a kernel adds
                             on top: slab partials, the bias, the cond term).
  S                          the absolute-value twin of the operation (sum |a| |b| + |bias| + ...), returned by every operator.
  rho_out                    the output's own rounding: 2^-8 for bf16 (8 significant bits: a round-to-nearest result is off by at
                             most 2^-8 of its value, e.g. 1 + 2^-8 -> 1), 2^-24 for fp32.
  eps_epi                    fp32 epilogue work: the accumulation bound carried through the nonlinearity by its derivative, plus
                             FAST_FN for the hardware exp / reciprocal of tanhf_ / sigmoidf_ (csrc/common.h).

  aggregate:  fp32 outputs ||got - ref||_2 / ||ref||_2 <= 2e-5;  bf16 outputs: at most 2 % of the elements differ from bf16(ref).

Every test also runs the same checks against a reference with one planted defect (a zeroed weight entry, a zeroed input row, a
dropped dY row) and requires at least one of them to miss by >= 3x (`check_with_control`): a check that cannot see the subtlest
plausible defect proves nothing.

Operators take and return torch float64 tensors on the CPU; rows are the product's rows layout (ops.RowsCtx): a k-tap conv reads
zero rows outside [0, R).  gt_conv_gemm_bf16 clamps the row index into [0, R-1] instead; the two agree because the first and last k/2
rows of every conv input are zero (halo rows) — the operands of these tests keep that precondition, oracle/conv64.py (edge=) restates
both forms.  bf16 tensors are raw bit patterns (int16 / uint16) or torch.bfloat16.
"""
import numpy as np
import torch

GAMMA_ULP = 2.0 ** -23
RHO = {"bf16": 2.0 ** -8, "f32": 2.0 ** -24}
FAST_FN = 2.0 ** -21           # __expf + v_rcp_f32 in tanhf_ / sigmoidf_, absolute on their (0, 1) / (-1, 1) results
AGG_F32 = 2e-5                 # ||got - ref|| / ||ref|| for fp32 outputs
AGG_BF16 = 0.02                # share of bf16 outputs that differ from bf16(ref)
CONTROL_MISS = 3.0             # a planted defect must miss some check by this factor


def gamma(K):
    return (K + 4) * GAMMA_ULP


# ----------------------------------------------------------------------------- bf16 (csrc/common.h f2bf / bf2f)
def f2bf(x):
    """fp32 -> bf16 bits (uint16), round to nearest even; NaN -> the quiet NaN 0x7FC0 (torch's conversion), +-inf stay."""
    a = np.ascontiguousarray(np.asarray(x, dtype=np.float32))
    u = a.view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)
    return np.where(np.isnan(a), np.uint16(0x7FC0), r)


def bf2f(h):
    """bf16 bits (any 16-bit integer array / tensor, or a torch.bfloat16 tensor) -> float32 numpy array."""
    if isinstance(h, torch.Tensor):
        h = h.detach().cpu()
        if h.dtype == torch.bfloat16:
            h = h.view(torch.int16)
        h = h.numpy()
    h = np.asarray(h).astype(np.uint16).astype(np.uint32)
    return (h << 16).view(np.float32)


def bf16_round(x):
    """value of bf16(fp32(x)) as float64"""
    return bf2f(f2bf(x)).astype(np.float64)


def bf16_ulp(x):
    """spacing of bf16 numbers at |x| (2^(e - 7) for |x| in [2^e, 2^(e+1)); the subnormal spacing 2^-133 below 2^-126)"""
    a = np.abs(np.asarray(x, dtype=np.float64))
    e = np.floor(np.log2(np.where(a > 0, a, 1.0)))
    return np.where(a >= 2.0 ** -126, 2.0 ** (e - 7), 2.0 ** -133)


def t64(x):
    """anything array-like (bf16 tensors as their values) -> float64 CPU tensor"""
    if isinstance(x, torch.Tensor):
        x = x.detach().cpu()
        if x.dtype == torch.bfloat16:
            return x.to(torch.float64)
        return x.to(torch.float64)
    return torch.from_numpy(np.asarray(x, dtype=np.float64))


def bits(x):
    """bf16 tensor -> uint16 numpy bits"""
    x = x.detach().cpu()
    if x.dtype == torch.bfloat16:
        x = x.view(torch.int16)
    return x.numpy().astype(np.uint16)


# ----------------------------------------------------------------------------- weight images (csrc/conv_gemm.hip)
def pk_index(frag, t, nrow, k, Np, Kp):
    """conv_gemm.hip pk_index: flat element index of (tap t, packed row nrow, reduction index k) in an image, broadcast."""
    t, nrow, k = (np.asarray(a, dtype=np.int64) for a in (t, nrow, k))
    if frag:
        return ((((t * (Np >> 5) + (nrow >> 5)) * (Kp >> 4) + (k >> 4)) * 64 + (nrow & 31) + 32 * ((k & 15) >> 3)) * 8 + (k & 7))
    return (t * Np + nrow) * Kp + k


def gate_row(co, Cout, flags):
    """packed forward row of output channel co: flag 1 [32 tanh | 32 sigmoid] per 64 rows, flag 16 [16 | 16] per 32, else co"""
    co = np.asarray(co, dtype=np.int64)
    half = Cout >> 1
    c = np.where(co < half, co, co - half)
    if flags & 1:
        return (c >> 5) * 64 + np.where(co < half, 0, 32) + (c & 31)
    if flags & 16:
        return (c >> 4) * 32 + np.where(co < half, 0, 16) + (c & 15)
    return co


def decode_image(img, taps, Np, Kp, frag):
    """A packed bf16 image (flat, raw bits) -> dense float64 [taps][Np][Kp] in packed-row order (gate interleave not undone)."""
    flat = bf2f(bits(img) if isinstance(img, torch.Tensor) else img).astype(np.float64)
    t, n, k = np.meshgrid(np.arange(taps), np.arange(Np), np.arange(Kp), indexing="ij")
    return torch.from_numpy(flat[pk_index(frag, t, n, k, Np, Kp)])


def _gather(img, idx):
    return torch.from_numpy(bf2f(bits(img) if isinstance(img, torch.Tensor) else np.asarray(img))[idx].astype(np.float64))


def decode_fwd(img, Cout, Cin, taps, Np, Kp, flags):
    """forward image (Pf[tap][pn(co)][ci]) -> dense W [taps][Cout][Cin] float64, gate interleave undone; reads only the weights'
    own entries, so `img` may be a window of a bigger image (ops.PackSlice)"""
    t, co, ci = np.meshgrid(np.arange(taps), np.arange(Cout), np.arange(Cin), indexing="ij")
    return _gather(img, pk_index(bool(flags & 2), t, gate_row(co, Cout, flags), ci, Np, Kp))


def decode_dgrad(img, Cout, Cin, taps, Np, Kp, flags):
    """data-gradient image (Pd[taps-1-tap][ci][co]: roles swapped, taps flipped) -> dense W [taps][Cout][Cin] float64 in the
    FORWARD convention"""
    t, co, ci = np.meshgrid(np.arange(taps), np.arange(Cout), np.arange(Cin), indexing="ij")
    return _gather(img, pk_index(bool(flags & 4), taps - 1 - t, ci, co, Np, Kp))


def packed_weights(v, g=None, inv_norm=None):
    """What pack_one_row / pack_rows8 write for weight v [Cout, Cin, taps] fp32: bf16(fp32(v * fp32(g * inv_norm))) with the
    kernel's own inv_norm [Cout] (or bf16(v) without g).  Returns float64 [taps][Cout][Cin]."""
    v = np.asarray(v.detach().cpu() if isinstance(v, torch.Tensor) else v, dtype=np.float32)
    if g is not None:
        g = np.asarray(g.detach().cpu() if isinstance(g, torch.Tensor) else g, dtype=np.float32).reshape(-1)
        inv = np.asarray(inv_norm.detach().cpu() if isinstance(inv_norm, torch.Tensor) else inv_norm, dtype=np.float32)
        sc = (g * inv).astype(np.float32)
        v = (v * sc[:, None, None]).astype(np.float32)
    return torch.from_numpy(bf16_round(v)).permute(2, 0, 1).contiguous()


def pack_image_np(W, Np, Kp, flags, dgrad=False):
    """numpy packer with the index formulas of pack_one_row (test of decode_*): W [taps][Cout][Cin] float -> flat bf16 bits"""
    W = np.asarray(W, dtype=np.float32)
    taps, Cout, Cin = W.shape
    out = np.zeros(taps * Np * Kp, dtype=np.uint16)
    tap, co, ci = np.meshgrid(np.arange(taps), np.arange(Cout), np.arange(Cin), indexing="ij")
    w = f2bf(W)
    if dgrad:
        out[pk_index(bool(flags & 4), taps - 1 - tap, ci, co, Np, Kp)] = w
    else:
        out[pk_index(bool(flags & 2), tap, gate_row(co, Cout, flags), ci, Np, Kp)] = w
    return out


# ----------------------------------------------------------------------------- rows-layout operators (float64, with |.| twins)
def shift_rows(X, s):
    """Xs[m] = X[m + s] for 0 <= m + s < R, else 0"""
    R = X.shape[0]
    out = torch.zeros_like(X)
    if s >= 0:
        if s < R:
            out[:R - s] = X[s:]
    elif -s < R:
        out[-s:] = X[:R + s]
    return out


def conv_rows(X, W, bias=None):
    """Y[m, n] = sum_tap sum_ci X[m + tap - k/2, ci] W[tap][n][ci] (+ bias[n]); X [R, Cin], W [taps][N][Cin].
    Returns (Y, S) with S the same sum over |X| |W| (+ |bias|)."""
    X, W = t64(X), t64(W)
    taps = W.shape[0]
    Y = torch.zeros(X.shape[0], W.shape[1], dtype=torch.float64)
    S = torch.zeros_like(Y)
    for t in range(taps):
        Xs = shift_rows(X, t - taps // 2)
        Y += Xs @ W[t].T
        S += Xs.abs() @ W[t].abs().T
    if bias is not None:
        b = t64(bias)
        Y += b
        S += b.abs()
    return Y, S


def conv_rows_wgrad(X, dY, taps):
    """dW[tap][co][ci] = sum_m dY[m, co] X[m + tap - k/2, ci] over ALL rows; returns (dW, S)."""
    X, dY = t64(X), t64(dY)
    dW = torch.stack([dY.T @ shift_rows(X, t - taps // 2) for t in range(taps)])
    S = torch.stack([dY.abs().T @ shift_rows(X, t - taps // 2).abs() for t in range(taps)])
    return dW, S


def utt_sum(Y, rowutt, B):
    """per-utterance sums over rows: out[b] = sum_{m: rowutt[m] == b} Y[m]; returns (out, sum of |Y|)"""
    Y = t64(Y)
    idx = torch.as_tensor(rowutt, dtype=torch.int64).cpu()
    out = torch.zeros(B, *Y.shape[1:], dtype=torch.float64).index_add_(0, idx, Y)
    S = torch.zeros_like(out).index_add_(0, idx, Y.abs())
    return out, S


def weightnorm_bwd(dW, S_dW, K_dW, v, g, inv_norm):
    """torch weight_norm (dim 0) backward, as the kernel maps it (conv_wgrad.hip weightnorm_bwd_row) with the kernel's inv_norm:
        dg = <dW, v> inv;   dv = g inv dW - g <dW, v> inv^3 v
    dW [taps][Cout][Cin] (float64 reference) with its |.| twin S_dW summed over K_dW terms; v [Cout, Cin, taps], g [Cout], inv [Cout].
    Returns (dv [Cout, Cin, taps], dg [Cout], bound_dv, bound_dg): the accumulation bound of dW carried through the linear map
    (absolute values of its coefficients) plus the fp32 rounding of each product / coefficient of the kernel's epilogue."""
    dWc = dW.permute(1, 2, 0)                               # [Cout, Cin, taps]
    BW = (gamma(K_dW) * S_dW).permute(1, 2, 0)
    v, g, inv = t64(v), t64(g).reshape(-1), t64(inv_norm)
    Cout = v.shape[0]
    n = v[0].numel()
    d = (dWc * v).reshape(Cout, -1).sum(1)
    Bd = (BW * v.abs()).reshape(Cout, -1).sum(1) + gamma(n + 6) * (dWc * v).abs().reshape(Cout, -1).sum(1)
    dg = d * inv
    a = (g * inv)[:, None, None]
    b = (g * d * inv ** 3)[:, None, None]
    dv = a * dWc - b * v
    u = RHO["f32"]
    bound_dv = a.abs() * BW + (g.abs() * inv ** 3 * Bd)[:, None, None] * v.abs() + u * (2 * (a * dWc).abs() + 5 * (b * v).abs())
    bound_dg = inv * Bd + u * dg.abs()
    return dv, dg, bound_dv, bound_dg


# ----------------------------------------------------------------------------- the checking rule
class Report:
    def __init__(self, name, worst, agg, agg_limit, kind):
        self.name, self.worst, self.agg, self.agg_limit, self.kind = name, worst, agg, agg_limit, kind

    @property
    def ok(self):
        return self.worst <= 1.0 and self.agg <= self.agg_limit

    @property
    def miss(self):
        """by how much the worse of the two checks is missed (<= 1: passes)"""
        return max(self.worst, self.agg / self.agg_limit)

    def __str__(self):
        return (f"{self.name}: worst err/bound {self.worst:.3g}, "
                + (f"rel L2 {self.agg:.3g}" if self.kind == "f32" else f"bf16 mismatches {100 * self.agg:.3g} %")
                + (f" (limit {self.agg_limit:g})" if self.kind == "f32" else f" (limit {100 * self.agg_limit:g} %)"))


def check(name, got, ref, bound, kind="f32"):
    """Evaluate the rule; `bound` = gamma_K * S + eps_epi (rho_out * |ref| is added here).  Returns a Report (asserts nothing)."""
    got, ref, bound = t64(got), t64(ref), t64(bound)
    assert got.shape == ref.shape == bound.shape, (name, got.shape, ref.shape, bound.shape)
    err = (got - ref).abs()
    lim = bound + RHO[kind] * ref.abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / lim)
    worst = float(ratio.max()) if ratio.numel() else 0.0
    if kind == "f32":
        agg = float((got - ref).norm() / ref.norm().clamp_min(1e-300))
        return Report(name, worst, agg, AGG_F32, kind)
    rb = t64(bf16_round(ref.numpy()))
    agg = float((got != rb).double().mean()) if got.numel() else 0.0
    return Report(name, worst, agg, AGG_BF16, kind)


def check_with_control(name, got, ref, bound, bad_ref, bad_bound=None, kind="f32", log=print):
    """The rule against the true reference must hold; against the planted-defect reference it must miss by >= CONTROL_MISS.
    bad_ref: one reference, or {defect name: reference or (reference, bound)} — every one of them must miss.
    Returns the passing report; its `misses` is {defect name: miss factor}."""
    r = check(name, got, ref, bound, kind)
    bads = bad_ref if isinstance(bad_ref, dict) else {"control": (bad_ref, bad_bound)}
    controls = {}
    for d, b in bads.items():
        b, bb = b if isinstance(b, tuple) else (b, None)
        controls[d] = check(f"{name} [planted defect: {d}]", got, b, bound if bb is None else bb, kind)
    r.misses = {d: c.miss for d, c in controls.items()}
    log(str(r) + "".join(f"; {d} misses by {c.miss:.3g}x" for d, c in controls.items()))
    assert r.ok, str(r)
    for c in controls.values():
        assert c.miss >= CONTROL_MISS, f"negative control not seen: {c}"
    return r


# ----------------------------------------------------------------------------- planted defects
def drop_weight_entry(W, tap=None, ci=None):
    """W [taps][N][K] with column (tap, ci) zeroed for every output: one product gone from every output element"""
    W = t64(W).clone()
    tap = W.shape[0] // 2 if tap is None else tap
    ci = W.shape[2] // 3 if ci is None else ci
    W[tap, :, ci] = 0
    return W


def drop_row(X, m):
    X = t64(X).clone()
    X[m] = 0
    return X


# ----------------------------------------------------------------------------- parameter gradients of one conv (flow_impl.conv_param_grads)
def conv_param_grads_ref(X, dY, taps, slabs, v, g=None, inv_norm=None, prior=None, drop_dy_row=None):
    """float64 reference of a conv's parameter gradients from its bf16 input rows X [R, Cin] and output-gradient rows dY [R, Cout]
    (gt_conv_wgrad_* -> slab partials -> gt_weightnorm_bwd*): {"v": (ref, bound), "g": ..., "b": ...} in the parameters' shapes
    (v [Cout, Cin, taps], g [Cout], b [Cout]).  The slab partials add `slabs` terms to every sum; prior: {"v", "g", "b"} the values
    the destinations held (accumulate = 1).  drop_dy_row: leave that row of dY out (the planted defect of the tests)."""
    X, dY = t64(X), t64(dY)
    if drop_dy_row is not None:
        dY = drop_row(dY, drop_dy_row)
    R = X.shape[0]
    K = R + slabs
    dW, SW = conv_rows_wgrad(X, dY, taps)
    out = {}
    if g is None:
        out["v"] = (dW.permute(1, 2, 0), gamma(K) * SW.permute(1, 2, 0))
    else:
        dv, dg, bdv, bdg = weightnorm_bwd(dW, SW, K, v, g, inv_norm)
        out["v"], out["g"] = (dv, bdv), (dg, bdg)
    out["b"] = (dY.sum(0), gamma(K) * dY.abs().sum(0))
    if prior is not None:
        for k, (ref, bnd) in list(out.items()):
            p = t64(prior[k]).reshape(ref.shape)
            out[k] = (ref + p, bnd + RHO["f32"] * (ref.abs() + p.abs()))        # one more fp32 add in the kernel
    return out


def check_conv_param_grads(name, conv, grads, X, dY, slabs, prior=None, log=print):
    """The rule on the gradients a ConvP / WNConvP got from flow_impl.conv_param_grads (grads: {param: tensor}) against
    conv_param_grads_ref with the kernel's inv_norm, with a dropped dY row (the one of largest |dY|) as the negative control.
    Returns {key: Report}."""
    wn = conv.weight_norm
    v = conv.weight_v if wn else conv.weight
    taps = v.shape[2]
    Cin, Cout = v.shape[1], v.shape[0]
    X, dY = t64(X)[:, :Cin], t64(dY)[:, :Cout]
    args = (X, dY, taps, slabs, v.detach().cpu(), conv.weight_g.detach().cpu() if wn else None,
            conv.pc.inv_norm.detach().cpu() if wn else None, prior)
    ref = conv_param_grads_ref(*args)
    bad = conv_param_grads_ref(*args, drop_dy_row=int(dY.abs().sum(1).argmax()))
    params = {"v": v, "b": conv.bias}
    if wn:
        params["g"] = conv.weight_g
    out = {}
    for k, p in params.items():
        got = t64(grads[p]).reshape(ref[k][0].shape)
        out[k] = check_with_control(f"{name} d{k}", got, ref[k][0], ref[k][1], bad[k][0], kind="f32", log=log)
    return out


# ----------------------------------------------------------------------------- the WaveNet gate (modules.py:151-170, csrc/wn_stack.hip)
def gate_fwd(Y, S_acc, K, H, cond=None, cond_bound=None, keep=None, scale=1.0):
    """One gated layer's epilogue from the float64 conv output Y = conv(x) + bias [R, 2H] (its |.| twin S_acc, K terms):
        pre = drop(Y) + cond;  T = tanh(pre[:, :H]), S = sigmoid(pre[:, H:]), acts = T * S   (the kernel: acts = bf16(T32 * S32))
    keep: (keep_t, keep_s) bool [R, H] or None; cond: float64 [R, 2H] or None with its own bound cond_bound.
    Returns {"t", "s", "acts": (ref, bound)} (bounds without the output's own rounding) and the pre-activation bound."""
    u = RHO["f32"]
    e = gamma(K) * S_acc
    if keep is not None:
        k = torch.cat([torch.from_numpy(keep[0]), torch.from_numpy(keep[1])], 1).double() * float(scale)
        Y, e = Y * k, e * k + u * (Y * k).abs()                                  # vt * drop_scale: one more rounding
    pre = Y if cond is None else Y + cond
    if cond is not None:
        e = e + u * pre.abs() + (0 if cond_bound is None else cond_bound)       # + cond: one rounding
    T, Sg = torch.tanh(pre[:, :H]), torch.sigmoid(pre[:, H:])
    bt = e[:, :H] + FAST_FN                                                      # |tanh'| <= 1
    bs = e[:, H:] / 4 + FAST_FN                                                  # |sigmoid'| <= 1/4
    acts = T * Sg
    ba = Sg.abs() * bt + T.abs() * bs + bt * bs + u * acts.abs()
    return {"t": (T, bt), "s": (Sg, bs), "acts": (acts, ba)}, e


def gate_bwd(dd, e_dd, T, Sg, keep=None, scale=1.0):
    """gate_bwd4 (csrc/wn_stack.hip) from d acts dd [R, H] (float64, accumulation bound e_dd) and the SAVED bf16 T, S:
        g_t = dd * S * (1 - T^2),  g_s = dd * T * S * (1 - S);  dpre_c = [g_t | g_s];  dpre = dpre_c * keep * scale
    Returns (dpre_c, bound_c, dpre, bound) (bounds without the output's own bf16 rounding)."""
    u = RHO["f32"]
    T, Sg = t64(T), t64(Sg)
    gt = dd * Sg * (1 - T * T)
    gs = dd * T * Sg * (1 - Sg)
    bt = e_dd * (Sg * (1 - T * T)).abs() + 4 * u * (dd * Sg).abs() * (1 + T * T)
    bs = e_dd * (T * Sg * (1 - Sg)).abs() + 5 * u * (dd * T * Sg).abs() * (1 + Sg.abs())
    c, bc = torch.cat([gt, gs], 1), torch.cat([bt, bs], 1)
    if keep is None:
        return c, bc, c, bc
    k = torch.cat([torch.from_numpy(keep[0]), torch.from_numpy(keep[1])], 1).double() * float(scale)
    return c, bc, c * k, bc * k + u * (c * k).abs()


def affine_cond(sig, w, b, H, n_layers):
    """COND == 2 (include/glowtts_hip.h): cond[m, 2H i + c] = b[off + c] + sig[m, par] * w[off + c], O = H n, par = 2H i // O,
    off = 2H i % O; returns (cond [R, 2H n] float64, bound) — the kernel's fp32 b + pv * w rounds at most twice."""
    sig, w, b = t64(sig), t64(w), t64(b)
    O = H * n_layers
    cols, bnds = [], []
    for i in range(n_layers):
        par, off = (2 * H * i) // O, (2 * H * i) % O
        pv = sig[:, par:par + 1]
        cols.append(b[off:off + 2 * H] + pv * w[off:off + 2 * H])
        bnds.append(2 * RHO["f32"] * (b[off:off + 2 * H].abs() + (pv * w[off:off + 2 * H]).abs()))
    return torch.cat(cols, 1), torch.cat(bnds, 1)


def conv_rows_dgrad_weights(W):
    """forward-convention W [taps][N][K] -> the weights of its data-gradient conv [taps][K][N] (roles swapped, taps flipped):
    conv_rows(dY, conv_rows_dgrad_weights(W)) = d/dX of conv_rows(X, W)"""
    return t64(W).flip(0).transpose(1, 2).contiguous()
