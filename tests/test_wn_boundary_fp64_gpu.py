"""The between-WaveNet kernels (csrc/wn_boundary.hip: gt_wn_boundary_fwd / _bwd / _rev, gt_boundary_param_reduce) and their
five-launch counterparts (csrc/flow_ops.hip: gt_coupling_*, gt_actnorm_invconv_*, gt_flow_scalars*) against float64 on their own
operands, under the rule of oracle/rows64.py with the operators of oracle/boundary64.py.

The launches of a real 3-block pass (train mode forward + backward, eval mode reverse) are recorded with flow_impl.BOUNDARY_TRACE and
re-issued one by one through _lib.fill_args, every stage teacher-forced from the kernel's own stored operands (decoded weight images,
the rows it read, the rows it wrote one stage earlier), so no bound grows with depth.  Where a tile never reaches HBM the reference
chains the stages and carries the bound (oracle/boundary64.py e_*): the backward's head -> tail tile (one K = 192 GEMM, then fp32
maps through the 4x4 mix and exp(logs)) and the reverse kernel's wn_out -> [m | logs] -> u -> x, whose composed bound is

    e_wn = gamma(768) S + 2^-8 |wn_out|  (bf16 in LDS)   ->   e_out = e_wn |Wend|^T + gamma(192) S   ->   coupling_rev, actnorm_invconv_rev

checked elementwise on every element.  That worst-case bound adds the 192 rounding errors of a row with one sign and is too wide to
see a zeroed weight column, so x is ALSO held, in relative L2, to the float64 chain whose wn_out is rounded to bf16 where the kernel
rounds it.  What is left between the two is fp32 error (AGG_F32) and the few roundings that fp32 accumulation sent the other way;
those are allowed as the rule allows them for a bf16 output: the limit is AGG_F32 plus the relative L2 distance to the same chain
with AGG_BF16 of wn_out's elements — the ones nearest a rounding midpoint, the only ones that can flip — moved to their other bf16
neighbour.  Against that limit the standard zeroed column of the skip GEMM and of the end conv must each miss by CONTROL_MISS.

Every re-issued launch runs between guards (reissue): outputs inside canaries and pre-filled with canaries (every row < R must be
written, masked rows must be zero), inputs exactly R rows long between NaN guards, logdet / dlogdet / len exactly B long between
guards with the guard rows of rowutt pointing into logdet's guard, accumulate-into outputs (logdet, d_an_logs, d_an_bias, d_w_ic)
pre-filled with non-zero values, pg_partial pre-filled with NaN.

Outside the rule — sigmoid_scale's __logf, the 4x4 inverse / log-det of gt_flow_scalars — the kernel is held to the float32 twin of
the float64 operator: rel-L2 err_kernel <= max(M err_twin, 2^-23), both against float64; 2^-23 is the fp32 spacing relative to the
output's scale.  M: twice the worst ratio measured on an MI355X, rounded up to a whole number (DESIGN.md 4.8.1 holds the table).

Planted defects, each required to miss by >= rows64.CONTROL_MISS: a zeroed (tap, k) weight column per GEMM, a valid row dropped from
the parameter-gradient sums, an utterance's first row credited to the previous utterance's log-det, W^-1 where W^-T belongs, the
sum dlogdet len term omitted from d_an_logs, the sigmoid_scale derivative omitted, W^T where W belongs in the 4x4 mix, the row
mask left out of the five-launch elementwise kernels, a neighbour's length in the pair's log-det."""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest
import torch

from oracle import boundary64 as B64
from oracle import rows64
from oracle.rows64 import RHO, check, check_with_control, conv_rows, drop_weight_entry, gamma, t64

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "golden"))
from fill import fill_module  # noqa: E402

pytestmark = pytest.mark.gpu
H, C, HALF, NL, NB = 192, 160, 80, 4, 3
GUARD, CAN, BCT_GUARD = 8, 768.0, 4096
U = RHO["f32"]
FLOOR = 2.0 ** -23
F32 = torch.float32
# err_kernel / err_twin allowed per output (module docstring; measured ratios in DESIGN.md 4.8.1)
M = {"fwd.z": 2, "fwd.logdet": 2, "bwd.dx_out": 3, "coupling_fwd.z": 2, "coupling_fwd.logdet": 2, "coupling_bwd.dx": 2,
     "coupling_rev.x": 2, "flow_scalars": 2}
# (name): squeezed lengths, squeezed T, ragged rows
LAYOUTS = {
    # 136 rows = 2 tiles + 8: tile 0 holds utterances 0, 1, 2 and the start of 3 (the segmented scan), R % 64 != 0
    "ragged": ([37, 1, 2, 60, 13], 60, True),
    # 5 x 144 rows: R % 64 = 16, the 1-frame utterance owns rows 144 .. 287 and tile 3 (rows 192 .. 255) holds masked rows only
    "uniform": ([37, 1, 2, 60, 13], 140, False),
    # 300 utterances of 1 and 2 frames, 1 656 rows: the per-utterance loops (b = threadIdx.x; b < B; b += 256) take a second trip
    "many": ([1 + (i % 2) for i in range(300)], 2, True),
}


def dev():
    return torch.device("cuda:0")


def rel_l2(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-300))


def hold_twin(key, name, got, ref, twin, bad=None):
    """err_kernel <= max(M err_twin, FLOOR); with `bad` (a planted-defect reference) the same limit must be missed by CONTROL_MISS"""
    ek, et = rel_l2(got, ref), rel_l2(twin, ref)
    lim = max(M[key] * et, FLOOR)
    msg = f"RATIO {key} {name}: err_kernel {ek:.3e} err_twin {et:.3e} ratio {ek / max(et, 1e-300):.3f} limit {lim:.3e}"
    if bad is not None:
        miss = rel_l2(got, bad) / lim
        msg += f"; control misses by {miss:.3g}x"
    print(msg)
    assert ek <= lim, msg
    if bad is not None:
        assert miss >= rows64.CONTROL_MISS, msg


def seen(name, got, ref, bound, bad, kind="f32"):
    """a further planted defect on a check that has already passed: it must miss by CONTROL_MISS"""
    c = check(name, got, bad, bound, kind)
    print(f"{name}: control misses by {c.miss:.3g}x")
    assert c.miss >= rows64.CONTROL_MISS, str(c)


# ----------------------------------------------------------------------------- one recorded pass per (layout, sigmoid_scale)
class Pass:
    pass


@functools.lru_cache(maxsize=None)
def record(layout, ss):
    from glow_tts_amd import flow_impl, models, modules, ops, wgrad
    from glow_tts_amd._lib import call
    lens, T, ragged = LAYOUTS[layout]
    P = Pass()
    P.tag, P.ss, P.lens, P.T, P.B, P.ragged = f"{layout} ss={int(ss)}", ss, lens, T, len(lens), ragged
    dec = fill_module(models.FlowSpecDecoder(80, H, 5, 1, NB, NL, p_dropout=0.05, sigmoid_scale=ss), "decoder.").to(dev()).train()
    assert dec.fused_boundary
    modules.prepare_all(dec)
    P.dec = dec
    rc = P.rc = ops.RowsCtx(torch.tensor(lens, dtype=torch.int32, device=dev()), T, lengths_host=lens if ragged else None, round_to=8)
    P.R, B = rc.R, P.B
    assert P.R % 64 != 0
    g = torch.Generator().manual_seed(17 + len(lens))
    fm = (torch.arange(2 * T)[None, :] < 2 * torch.tensor(lens)[:, None]).unsqueeze(1).float().to(dev())
    rn = lambda *s: torch.randn(*s, generator=g).to(dev())
    y, dz, zl = rn(B, HALF, 2 * T) * fm, rn(B, HALF, 2 * T) * fm, rn(B, HALF, 2 * T) * fm
    P.dlogdet = rn(B) * 0.1
    st = flow_impl._st(dev())

    def sq(t):
        r = torch.empty(P.R, C, device=dev())
        call.gt_squeeze_rows_f32(t, r, rc.lengths, B, HALF, 2 * T, rc.Tp, rc.row0, st)
        return r

    logdet = torch.zeros(B, device=dev())
    flow_impl.BOUNDARY_TRACE = trace = []
    try:
        if ragged:
            _, blocks = flow_impl.decoder_fwd_fused(rc, dec, None, [None] * NB, logdet, True, 5, y_bct=y, z_bct=torch.zeros_like(y))
            with wgrad.WgradQueue(dev(), site=dec):
                flow_impl.decoder_bwd_fused(rc, dec, blocks, None, P.dlogdet, False, dz_bct=dz, dx_bct=torch.zeros_like(y))
            dec.eval()
            flow_impl.decoder_rev_fused(rc, dec, None, [None] * NB, z_bct=zl, x_bct=torch.zeros_like(y))
        else:
            _, blocks = flow_impl.decoder_fwd_fused(rc, dec, sq(y), [None] * NB, logdet, True, 5)
            with wgrad.WgradQueue(dev(), site=dec):
                flow_impl.decoder_bwd_fused(rc, dec, blocks, sq(dz), P.dlogdet, False)
            dec.eval()
            flow_impl.decoder_rev_fused(rc, dec, sq(zl), [None] * NB)
    finally:
        flow_impl.BOUNDARY_TRACE = None
        dec.train()
    torch.cuda.synchronize()
    P.blocks = blocks
    P.fwd = [kw for n, _, kw in trace if n == "gt_wn_boundary_fwd"]
    P.bwd = [kw for n, _, kw in trace if n == "gt_wn_boundary_bwd"]
    P.rev = [kw for n, _, kw in trace if n == "gt_wn_boundary_rev"]
    # the variants this pass claims: head-only, both halves (twice), tail-only, in all three directions
    assert [(kw.get("acts") is not None, kw.get("y_next") is not None) for kw in P.fwd] == [(False, True), (True, True), (True, True), (True, False)]
    assert [(kw.get("dh") is not None, kw.get("dout") is not None) for kw in P.bwd] == [(False, True), (True, True), (True, True), (True, False)]
    assert [(kw.get("acts") is not None, kw.get("h_next") is not None) for kw in P.rev] == [(False, True), (True, True), (True, True), (True, False)]
    assert all(kw.get("pg_partial") is not None for kw in P.bwd[1:]) and all(kw.get("pf_ptr") is not None for kw in P.fwd[:3])
    for a, b, name in ((P.fwd[0], P.fwd[3], ("y_bct", "z_bct")), (P.bwd[0], P.bwd[3], ("dz_bct", "dx_bct")), (P.rev[0], P.rev[3], ("z_bct", "x_bct"))):
        assert (a.get(name[0]) is not None) == ragged and (b.get(name[1]) is not None) == ragged
    P.mask = t64(rc.rowmask)
    P.mk = P.mask[:, None]
    P.rowutt = rc.rowutt.long().cpu()
    P.lens64 = torch.tensor(lens, dtype=torch.float64)
    P.n_tiles = (P.R + 63) // 64
    if ragged:
        P.rowbatch, P.rowframe = rc.rowbatch.long().cpu(), rc.rowframe.long().cpu()
    P.max_utts_per_tile = max(len(set(P.rowutt[i * 64:(i + 1) * 64].tolist())) for i in range(P.n_tiles))
    P.masked_tiles = sum(int(P.mask[i * 64:(i + 1) * 64].sum() == 0) for i in range(P.n_tiles))
    return P


def squeeze_index(P, t):
    """commons.squeeze by plain indexing: [B, 80, 2T] -> rows [R, 160] (zero on masked rows)"""
    t = t.detach().cpu()
    out = torch.zeros(P.R, C, dtype=t.dtype)
    v = torch.nonzero(P.mask > 0).reshape(-1)
    b, f = P.rowbatch[v], P.rowframe[v]
    for p in range(2):
        out[v, p * HALF:(p + 1) * HALF] = t[b, :, 2 * f + p]
    return out


def unsqueeze_index(P, rows):
    rows = rows.detach().cpu()
    out = torch.zeros(P.B, HALF, 2 * P.T, dtype=rows.dtype)
    v = torch.nonzero(P.mask > 0).reshape(-1)
    b, f = P.rowbatch[v], P.rowframe[v]
    for p in range(2):
        out[b, :, 2 * f + p] = rows[v, p * HALF:(p + 1) * HALF]
    return out


# ----------------------------------------------------------------------------- re-issuing one launch between guards
ROW_IN = {"fwd": ("acts", "y", "x_in"), "bwd": ("dh", "dx_in", "x", "dz_in", "logs_raw", "y"), "rev": ("acts", "z", "x_in")}
ROW_OUT = {"fwd": ("wn_out", "logs_raw", "z", "y_next", "y0_bf16", "h_next"), "bwd": ("dx_out", "dout", "dwn_out", "via_skip"), "rev": ("x", "h_next")}
BCT_OUT = {"fwd": "z_bct", "bwd": "dx_bct", "rev": "x_bct"}
UNMASKED = ("logs_raw",)                     # the end conv's raw output carries its bias on masked rows too
ACC = ("d_an_logs", "d_an_bias", "d_w_ic")


class Result:
    pass


def guarded(t, fill, n=GUARD):
    buf = torch.full((t.shape[0] + 2 * n,) + tuple(t.shape[1:]), fill, dtype=t.dtype, device=t.device)
    buf[n:n + t.shape[0]] = t
    return buf, buf[n:n + t.shape[0]]


def prior_of(n, scale=1.0):
    return ((0.5 + 0.25 * (torch.arange(n) % 7)) * scale).float().to(dev())


def reissue(P, kind, kw, route="partials", **override):
    """One recorded launch again, between guards (module docstring) -> Result: .kw (what was launched), .out {name: view}, .prior.
    route (backward head): "partials" (pg_partial, then gt_boundary_param_reduce into the pre-filled accumulators) or "atomics"."""
    from glow_tts_amd import _lib
    from glow_tts_amd._lib import call
    L = _lib.lib()
    kw = dict(kw)
    kw.update(override)
    R, B, nan = P.R, P.B, float("nan")
    res = Result()
    res.out, res.prior, guards = {}, {}, []
    for k in ROW_IN[kind] + ("rowmask",):
        if kw.get(k) is not None:
            assert kw[k].shape[0] == R, k
            buf, kw[k] = guarded(kw[k], nan)
    if kw.get("acts") is not None:
        kw["ldacts"] = kw["acts"].stride(0)
    if kw.get("rowutt") is not None:
        buf, kw["rowutt"] = guarded(kw["rowutt"], B + 1)                 # a guard row's utterance lands in logdet's guard
    for k in ROW_OUT[kind]:
        if kw.get(k) is not None:
            buf, view = guarded(torch.full_like(kw[k], CAN), CAN)
            guards.append((k, buf, GUARD, R))
            kw[k] = res.out[k] = view
    if kw.get("via_skip") is not None:
        kw["ldvs"] = kw["via_skip"].stride(0)
    k = BCT_OUT[kind]
    if kw.get(k) is not None:
        n = kw[k].numel()
        flat = torch.full((n + 2 * BCT_GUARD,), CAN, device=dev())
        flat[BCT_GUARD:BCT_GUARD + n] = 0                                # pre-zeroed by the caller
        guards.append((k, flat, BCT_GUARD, n))
        kw[k] = res.out[k] = flat[BCT_GUARD:BCT_GUARD + n].view(kw[k].shape)
    if kw.get("len") is not None:
        buf, kw["len"] = guarded(kw["len"], 1 << 20)
    if kw.get("dlogdet") is not None:
        buf, kw["dlogdet"] = guarded(kw["dlogdet"], nan)
    if kind == "fwd":
        res.prior["logdet"] = prior_of(B)
        buf, view = guarded(res.prior["logdet"].clone(), CAN)
        guards.append(("logdet", buf, GUARD, B))
        kw["logdet"] = res.out["logdet"] = view
    tab = None
    if kind == "bwd" and kw.get("dh") is not None:
        for k, n in zip(ACC, (C, C, 16)):
            res.prior[k] = prior_of(n, 3.0)
            buf, view = guarded(res.prior[k].clone(), CAN)
            guards.append((k, buf, GUARD, n))
            kw[k] = res.out[k] = view
        if route == "partials":
            PG = L.gt_boundary_param_partials()
            buf, view = guarded(torch.full((P.n_tiles * PG,), nan, device=dev()), CAN, n=PG)
            guards.append(("pg_partial", buf, PG, P.n_tiles * PG))
            kw["pg_partial"] = res.out["pg_partial"] = view
            tab = torch.tensor([res.out[k].data_ptr() for k in ACC], dtype=torch.int64).to(dev())
        else:
            kw["pg_partial"] = None
    cls = {"fwd": _lib.BoundaryFwdArgs, "bwd": _lib.BoundaryBwdArgs, "rev": _lib.BoundaryRevArgs}[kind]
    args = _lib.fill_args(cls, **{k: v for k, v in kw.items() if v is not None})
    _lib.check(getattr(L, "gt_wn_boundary_" + kind)(ctypes.byref(args), _lib.current_stream(dev())), kind)
    torch.cuda.synchronize()
    if tab is not None:
        assert torch.isfinite(res.out["pg_partial"]).all(), "a float of pg_partial was not written"
        res.partials = res.out["pg_partial"].clone()
        call.gt_boundary_param_reduce(res.out["pg_partial"], P.n_tiles, 1, tab, _lib.current_stream(dev()))
        torch.cuda.synchronize()
    masked = (P.rc.rowmask == 0)
    for k, buf, n0, n in guards:
        g = torch.cat([buf[:n0].reshape(-1), buf[n0 + n:].reshape(-1)]).float()
        assert (g == CAN).all(), f"{kind} {k}: a guard was written"
    for k in ROW_OUT[kind]:
        if k in res.out:
            v = res.out[k].float()
            assert torch.isfinite(v).all(), f"{kind} {k}: a NaN guard was read"
            assert not (v == CAN).any(), f"{kind} {k}: a row < R was not written"
            if k not in UNMASKED:
                assert (v[masked] == 0).all(), f"{kind} {k}: a masked row is not zero"
    for k in ("logdet",) + ACC + (BCT_OUT[kind],):
        if k in res.out:
            assert torch.isfinite(res.out[k]).all(), f"{kind} {k}: a NaN guard was read"
    res.kw = kw
    return res


def Wf(pc, Cout, Cin):
    return rows64.decode_fwd(pc.fwd, Cout, Cin, 1, pc.Np_f, pc.Kp_f, pc.flags)


def Wd(pc, Cout, Cin):
    """the data-gradient image as the weights of its conv on rows: [1][Cin][Cout]"""
    return rows64.conv_rows_dgrad_weights(rows64.decode_dgrad(pc.dgrad, Cout, Cin, 1, pc.Np_d, pc.Kp_d, pc.flags))


def flat(t):
    return t64(t).reshape(-1)


# ----------------------------------------------------------------------------- forward
def check_fwd(P, b, res, tag=""):
    kw, out, ss, mk, B = res.kw, res.out, P.ss, P.mk, P.B
    tail, head = kw.get("acts") is not None, kw.get("y_next") is not None
    name = f"fwd[{b}] {P.tag}{tag}"
    prior = t64(res.prior["logdet"])
    ld_ref, ld_S, ld_n, ld_b, ld_bad, ld_twin = prior.clone(), prior.abs(), torch.zeros(B, dtype=torch.float64), 0, prior.clone(), prior.clone()
    if tail:
        cbp = P.dec.flows[3 * (b - 1) + 2]
        assert kw["w_skip"].data_ptr() == cbp.wn.pc_skipcat_frag.fwd.data_ptr() and kw["w_end"].data_ptr() == cbp.end.pc_frag.fwd.data_ptr()
        assert kw["sigmoid_scale"] == int(ss)
        Ws, We = Wf(cbp.wn.pc_skipcat_frag, H, NL * H), Wf(cbp.end.pc_frag, C, H)
        acts = t64(kw["acts"])[:, :NL * H]
        Y, S = conv_rows(acts, Ws, kw["b_skip"])
        Yb = conv_rows(acts, drop_weight_entry(Ws), kw["b_skip"])[0]
        check_with_control(name + " wn_out", t64(out["wn_out"]), Y * mk, gamma(NL * H) * S * mk, Yb * mk, kind="bf16")
        wn = t64(out["wn_out"])
        O, SO = conv_rows(wn, We, kw["b_end"])
        Ob = conv_rows(wn, drop_weight_entry(We), kw["b_end"])[0]
        raw = t64(out["logs_raw"])
        check_with_control(name + " logs_raw", raw, O[:, HALF:], gamma(H) * SO[:, HALF:], Ob[:, HALF:])
        e_out = torch.cat([gamma(H) * SO[:, :HALF], torch.zeros_like(raw)], 1)
        o, ob, y = torch.cat([O[:, :HALF], raw], 1), torch.cat([Ob[:, :HALF], raw], 1), t64(kw["y"])
        f = B64.coupling_fwd(o, y, P.mask, P.rowutt, B, ss, e_out)
        fb = B64.coupling_fwd(ob, y, P.mask, P.rowutt, B, ss, e_out)
        fu = B64.coupling_fwd(o, y, P.mask, B64.credit_neighbour(P.rowutt, P.mask), B, ss)
        zg = t64(out["z"]) if "z" in out else squeeze_index(P, out["z_bct"]).double()
        assert torch.equal(zg[:, :HALF], y[:, :HALF])                             # z0 is a copy
        if ss:
            f32 = B64.coupling_fwd(o.float(), y.float(), P.mask.float(), P.rowutt, B, True)
            hold_twin("fwd.z", name, zg[:, HALF:], f["z"][0][:, HALF:], f32["z"][0][:, HALF:], fb["z"][0][:, HALF:])
            ld_twin = ld_twin + f32["logdet"][0].double()
        else:
            check_with_control(name + " z", zg, f["z"][0], f["z"][1], fb["z"][0])
        ld_ref, ld_S, ld_n, ld_bad = ld_ref + f["logdet"][0], ld_S + f["logdet"][1], f["logdet"][2], ld_bad + fu["logdet"][0]
        xin = zg
    elif kw.get("y_bct") is not None:
        xin = t64(out["z"])                                                       # the squeezed rows the launch wrote
        assert torch.equal(out["z"].cpu(), squeeze_index(P, kw["y_bct"]))
    else:
        xin = t64(kw["x_in"])
    if head:
        cb = P.dec.flows[3 * b + 2]
        assert kw["w_start"].data_ptr() == cb.start.pc_frag.fwd.data_ptr() and kw["B"] == B
        lg, bs, W, scal = flat(kw["an_logs"]), flat(kw["an_bias"]), t64(kw["w_ic"]).reshape(4, 4), flat(kw["scal"])
        yr, yb, _, _ = B64.actnorm_invconv_fwd(xin, lg, bs, W, P.mask)
        check_with_control(name + " y_next", t64(out["y_next"]), yr, yb, B64.actnorm_invconv_fwd(xin, lg, bs, W.T, P.mask)[0])
        assert np.array_equal(rows64.bits(out["y0_bf16"]), rows64.f2bf(out["y_next"][:, :HALF].cpu().numpy())), name + " y0_bf16"
        Wst = Wf(cb.start.pc_frag, H, HALF)
        y0 = t64(out["y0_bf16"])
        Hh, Sh = conv_rows(y0, Wst, kw["b_start"])
        check_with_control(name + " h_next", t64(out["h_next"]), Hh * mk, gamma(HALF) * Sh * mk,
                           conv_rows(y0, drop_weight_entry(Wst), kw["b_start"])[0] * mk, kind="bf16")
        pl, pb = B64.pair_logdet(scal, P.lens64, C)
        ld_ref, ld_S, ld_b, ld_bad, ld_twin = ld_ref + pl, ld_S + pl.abs(), pb, ld_bad + pl, ld_twin + pl
    got = t64(out["logdet"])
    bound = gamma(ld_n + P.n_tiles + 8) * ld_S + ld_b
    if tail and ss:
        hold_twin("fwd.logdet", name, got, ld_ref, ld_twin.float(), ld_bad)
    elif tail:
        check_with_control(name + " logdet", got, ld_ref, bound, ld_bad)
    else:                                                                        # head only: the pair's term with the neighbour's length
        check_with_control(name + " logdet", got, ld_ref, bound, prior + pl.roll(1))


CASES = [("ragged", False), ("ragged", True), ("uniform", False), ("many", False)]


@pytest.mark.parametrize("layout,ss", CASES)
def test_forward_launches_against_float64(built, layout, ss):
    P = record(layout, ss)
    if layout == "ragged":
        assert P.max_utts_per_tile >= 3
    if layout == "uniform":
        assert P.masked_tiles >= 1
    if layout == "many":
        assert P.B > 256
    for b, kw in enumerate(P.fwd):
        check_fwd(P, b, reissue(P, "fwd", kw))


# ----------------------------------------------------------------------------- backward
def check_bwd(P, j, res, tag=""):
    kw, out, ss, mk, B = res.kw, res.out, P.ss, P.mk, P.B
    headb, tailb = kw.get("dh") is not None, kw.get("dout") is not None
    b = NB - j
    name = f"bwd[{j}] {P.tag}{tag}"
    dld = t64(P.dlogdet)
    dzb = None
    if headb:
        cb = P.dec.flows[3 * b + 2]
        assert kw["w_start_d"].data_ptr() == cb.start.pc_frag.dgrad.data_ptr() and kw["B"] == B
        Wsd = Wd(cb.start.pc_frag, H, HALF)                                      # [1][80][192]
        dh, dxi, x = t64(kw["dh"]), t64(kw["dx_in"]), t64(kw["x"])
        lg, bs, W, WinvT = flat(kw["an_logs"]), flat(kw["an_bias"]), t64(kw["w_ic"]).reshape(4, 4), flat(kw["scal"])[2:].reshape(4, 4)
        ds, S = conv_rows(dh, Wsd)

        def head_ref(ds_, **defect):
            top = dxi[:, :HALF] + ds_
            dy = torch.cat([top, dxi[:, HALF:]], 1)
            e = torch.cat([gamma(H) * S + U * top.abs(), torch.zeros_like(top)], 1)
            return B64.actnorm_invconv_bwd(x, dy, lg, bs, W, WinvT, P.mask, dld, P.lens64, e_dy=e, slabs=P.n_tiles + 16, **defect), dy

        ref, dy = head_ref(ds)
        bad_w = head_ref(conv_rows(dh, drop_weight_entry(Wsd))[0])[0]
        row = int(((dy.abs().sum(1)) * P.mask).argmax())
        bad_row, bad_inv, bad_book = head_ref(ds, drop_row=row)[0], head_ref(ds, use_inverse=True)[0], head_ref(ds, bookkeeping=False)[0]
        w_miss = []                                                              # the zeroed start-conv column: it sums away in d_an_bias, not in the others
        for k in ACC:
            pr = t64(res.prior[k])
            want = ref[k][0] + pr
            bound = ref[k][1] + U * (want.abs() + pr.abs())
            check_with_control(f"{name} {k}", t64(out[k]), want, bound, bad_row[k][0] + pr)
            w_miss.append(check(k, t64(out[k]), bad_w[k][0] + pr, bound).miss)
            if k == "d_w_ic":
                seen(f"{name} {k} [W^-1 for W^-T]", t64(out[k]), want, bound, bad_inv[k][0] + pr)
            if k == "d_an_logs":
                seen(f"{name} {k} [sum dlogdet len omitted]", t64(out[k]), want, bound, bad_book[k][0] + pr)
        print(f"{name} parameter gradients [zeroed start-conv column]: control misses by {max(w_miss):.3g}x")
        assert max(w_miss) >= rows64.CONTROL_MISS, w_miss
        dz, e_dz, dzb = ref["dx"][0], ref["dx"][1], bad_w["dx"][0]
        if not tailb:
            got = t64(out["dx_out"]) if "dx_out" in out else squeeze_index(P, out["dx_bct"]).double()
            check_with_control(name + " dx_out", got, dz, e_dz, dzb)
    else:
        dz = t64(kw["dz_in"]) if kw.get("dz_in") is not None else squeeze_index(P, kw["dz_bct"]).double()
        e_dz = torch.zeros_like(dz)
    if not tailb:
        return
    cbp = P.dec.flows[3 * (b - 1) + 2]
    assert kw["w_end_d"].data_ptr() == cbp.end.pc_frag.dgrad.data_ptr() and kw["w_skip_d"].data_ptr() == cbp.wn.pc_skipcat_frag.dgrad.data_ptr()
    assert kw["sigmoid_scale"] == int(ss)
    raw, y1 = t64(kw["logs_raw"]), t64(kw["y"])[:, HALF:]
    c = B64.coupling_bwd(raw, y1, dz, dld, P.mask, P.rowutt, ss, e_dz)
    if dzb is not None:                                                          # the zeroed start-conv column, through the whole chain
        cbad = B64.coupling_bwd(raw, y1, dzb, dld, P.mask, P.rowutt, ss, e_dz)
    else:                                                                        # tail only: d logdet of the neighbouring utterance
        cbad = B64.coupling_bwd(raw, y1, dz, dld, P.mask, B64.credit_neighbour(P.rowutt, P.mask), ss, e_dz)
    dxg = t64(out["dx_out"])
    if ss:
        r = check(name + " dx_out[:, :80]", dxg[:, :HALF], c["dx"][0][:, :HALF], c["dx"][1][:, :HALF])
        assert r.ok, str(r)
        t32 = B64.coupling_bwd(raw.float(), y1.float(), dz.float(), dld.float(), P.mask.float(), P.rowutt, True)
        hold_twin("bwd.dx_out", name, dxg[:, HALF:], c["dx"][0][:, HALF:], t32["dx"][0][:, HALF:], cbad["dx"][0][:, HALF:] if dzb is not None else None)
        nod = B64.coupling_bwd(raw, y1, dz, dld, P.mask, P.rowutt, True, e_dz, scale_derivative=False)
        check_with_control(name + " dout [sigmoid_scale derivative omitted]", t64(out["dout"]), c["dout"][0], c["dout"][1], nod["dout"][0], kind="bf16")
    elif dzb is not None:
        check_with_control(name + " dx_out", dxg, c["dx"][0], c["dx"][1], cbad["dx"][0])
    else:
        r = check(name + " dx_out", dxg, c["dx"][0], c["dx"][1])
        print(r)
        assert r.ok, str(r)
    check_with_control(name + " dout", t64(out["dout"]), c["dout"][0], c["dout"][1], cbad["dout"][0], kind="bf16")
    Wed, Wkd = Wd(cbp.end.pc_frag, C, H), Wd(cbp.wn.pc_skipcat_frag, H, NL * H)  # [1][192][160], [1][768][192]
    do = t64(out["dout"])
    dw, S = conv_rows(do, Wed)
    check_with_control(name + " dwn_out", t64(out["dwn_out"]), dw * mk, gamma(C) * S * mk, conv_rows(do, drop_weight_entry(Wed))[0] * mk, kind="bf16")
    dwk = t64(out["dwn_out"])
    v, S = conv_rows(dwk, Wkd)
    check_with_control(name + " via_skip", t64(out["via_skip"])[:, :NL * H], v, gamma(H) * S, conv_rows(dwk, drop_weight_entry(Wkd))[0], kind="bf16")


@pytest.mark.parametrize("layout,ss", CASES)
def test_backward_launches_against_float64_on_both_parameter_gradient_routes(built, layout, ss):
    P = record(layout, ss)
    for j, kw in enumerate(P.bwd):
        check_bwd(P, j, reissue(P, "bwd", kw, route="partials"), " partials")
        if kw.get("dh") is not None:
            check_bwd(P, j, reissue(P, "bwd", kw, route="atomics"), " atomics")


# ----------------------------------------------------------------------------- reverse
def rounded_and_flipped(wn):
    """float64 wn_out -> (bf16(wn), the same with the AGG_BF16 share of elements nearest a rounding midpoint moved to their other
    bf16 neighbour)"""
    a = wn.numpy()
    b = rows64.bf16_round(a)
    ulp = rows64.bf16_ulp(b)
    other = np.where(a >= b, b + ulp, b - ulp)
    d = np.abs(np.abs(a - b) - ulp / 2) / ulp                                   # distance to the midpoint, in ulps
    d[a == 0] = np.inf                                                           # masked rows are exactly zero in the kernel too
    n = int(np.ceil(rows64.AGG_BF16 * a.size))
    pick = np.argsort(d, axis=None)[:n]
    f = b.copy().reshape(-1)
    f[pick] = other.reshape(-1)[pick]
    return torch.from_numpy(b), torch.from_numpy(f.reshape(a.shape))


def check_rev(P, k, res, tag=""):
    kw, out, ss, mk = res.kw, res.out, P.ss, P.mk
    tail, head = kw.get("acts") is not None, kw.get("h_next") is not None
    bt, bh = NB - k, NB - 1 - k
    name = f"rev[{k}] {P.tag}{tag}"
    if tail:
        cb = P.dec.flows[3 * bt + 2]
        assert kw["w_skip"].data_ptr() == cb.wn.pc_skipcat_frag.fwd.data_ptr() and kw["sigmoid_scale"] == int(ss)
        Ws, We = Wf(cb.wn.pc_skipcat_frag, H, NL * H), Wf(cb.end.pc_frag, C, H)
        acts, z = t64(kw["acts"])[:, :NL * H], t64(kw["z"])
        lg, bs, Winv = flat(kw["an_logs"]), flat(kw["an_bias"]), flat(kw["scal"])[2:].reshape(4, 4).T

        def chain(wn, We_, e_wn):
            """x and its bound from a float64 wn_out that is off by at most e_wn"""
            O, SO = conv_rows(wn, We_, kw["b_end"])
            e_out = conv_rows(e_wn, We_.abs())[0] + gamma(H) * SO
            u, bu = B64.coupling_rev(O, z, P.mask, ss, e_out)
            return B64.actnorm_invconv_rev(u, lg, bs, Winv, P.mask, e_y=bu)

        Y, S = conv_rows(acts, Ws, kw["b_skip"])
        Yb = conv_rows(acts, drop_weight_entry(Ws), kw["b_skip"])[0]
        got = t64(out["x"]) if "x" in out else squeeze_index(P, out["x_bct"]).double()
        # (1) every element, from the exact wn_out: the composed worst-case bound (module docstring)
        x, bx = chain(Y * mk, We, (gamma(NL * H) * S + RHO["bf16"] * Y.abs()) * mk)
        r = check(name + " x", got, x, bx)
        print(f"{name} x: worst err/bound {r.worst:.3g} (composed bound, elementwise)")
        assert r.worst <= 1.0, str(r)
        # (2) in relative L2, from wn_out rounded to bf16 where the kernel rounds it: what is left is fp32 error (AGG_F32) and the
        # roundings that fell the other way, allowed as the rule allows them for a bf16 output — AGG_BF16 of the elements, the ones
        # nearest a rounding midpoint (the only ones fp32 accumulation error can flip), each moved to its other bf16 neighbour
        wn_b, wn_f = rounded_and_flipped(Y * mk)
        zero = torch.zeros_like(Y)
        xq = chain(wn_b, We, zero)[0]
        lim = rows64.AGG_F32 + rel_l2(chain(wn_f, We, zero)[0], xq)
        err = rel_l2(got, xq)
        bad = {"skip-GEMM": chain(rounded_and_flipped(Yb * mk)[0], We, zero)[0], "end-conv": chain(wn_b, drop_weight_entry(We), zero)[0]}
        miss = {k: rel_l2(got, v) / lim for k, v in bad.items()}
        print(f"{name} x: rel L2 against the bf16-rounded chain {err:.3e} (limit {lim:.3e}); zeroed column misses by "
              + ", ".join(f"{v:.3g}x ({k})" for k, v in miss.items()))
        assert err <= lim, (name, err, lim)
        assert min(miss.values()) >= rows64.CONTROL_MISS, (name, miss)
        x0 = got[:, :HALF]
    elif kw.get("z_bct") is not None:
        assert torch.equal(out["x"].cpu(), squeeze_index(P, kw["z_bct"]))
        x0 = t64(out["x"])[:, :HALF]
    else:
        x0 = t64(kw["x_in"])[:, :HALF]
    if head:
        cbh = P.dec.flows[3 * bh + 2]
        assert kw["w_start"].data_ptr() == cbh.start.pc_frag.fwd.data_ptr()
        Wst = Wf(cbh.start.pc_frag, H, HALF)
        x0 = torch.from_numpy(rows64.bf16_round(x0.float().numpy()))
        Hh, Sh = conv_rows(x0, Wst, kw["b_start"])
        check_with_control(name + " h_next", t64(out["h_next"]), Hh * mk, gamma(HALF) * Sh * mk,
                           conv_rows(x0, drop_weight_entry(Wst), kw["b_start"])[0] * mk, kind="bf16")


@pytest.mark.parametrize("layout,ss", CASES[:3])
def test_reverse_launches_against_float64(built, layout, ss):
    P = record(layout, ss)
    for k, kw in enumerate(P.rev):
        check_rev(P, k, reissue(P, "rev", kw))


# ----------------------------------------------------------------------------- folded squeeze / unsqueeze
def test_folded_squeeze_and_unsqueeze_are_data_movement(built):
    """y_bct / z_bct / dz_bct / dx_bct (and the reverse kernel's z_bct / x_bct): bit-equal to the rows variant composed with plain
    indexing and with gt_squeeze_rows_f32 / gt_unsqueeze_rows_f32; atomically accumulated outputs go through the bound (the tests above)."""
    from glow_tts_amd import flow_impl
    from glow_tts_amd._lib import call
    P = record("ragged", False)
    rc, st, B, T = P.rc, flow_impl._st(dev()), P.B, P.T
    drop = dict(T=None, rowbatch=None, rowframe=None)

    def sq_kernel(t):
        r = torch.empty(P.R, C, device=dev())
        call.gt_squeeze_rows_f32(t.contiguous(), r, rc.lengths, B, HALF, 2 * T, rc.Tp, rc.row0, st)
        return r

    def unsq_kernel(r):
        t = torch.zeros(B, HALF, 2 * T, device=dev())
        call.gt_unsqueeze_rows_f32(r.contiguous(), t, rc.lengths, B, HALF, 2 * T, rc.Tp, rc.row0, st)
        return t

    def same(a, b, names):
        for k in names:
            assert torch.equal(a.out[k], b.out[k]), k

    valid = (rc.rowmask > 0)
    # forward, first launch: y_bct -> the squeezed rows
    kw = P.fwd[0]
    rows = squeeze_index(P, kw["y_bct"]).to(dev())
    assert torch.equal(sq_kernel(kw["y_bct"])[valid], rows[valid])
    a, b = reissue(P, "fwd", kw), reissue(P, "fwd", kw, y_bct=None, z=None, x_in=rows, **drop)
    assert torch.equal(a.out["z"], rows)
    same(a, b, ("y_next", "y0_bf16", "h_next"))
    # forward, last launch: z rows -> z_bct
    kw = P.fwd[3]
    a, b = reissue(P, "fwd", kw), reissue(P, "fwd", kw, z_bct=None, z=torch.empty(P.R, C, device=dev()), len=None, **drop)
    same(a, b, ("wn_out", "logs_raw"))
    assert torch.equal(a.out["z_bct"].cpu(), unsqueeze_index(P, b.out["z"])) and torch.equal(a.out["z_bct"], unsq_kernel(b.out["z"]))
    assert a.out["z_bct"].abs().max().item() > 0
    # backward, first launch: dz_bct -> rows
    kw = P.bwd[0]
    rows = squeeze_index(P, kw["dz_bct"]).to(dev())
    a, b = reissue(P, "bwd", kw), reissue(P, "bwd", kw, dz_bct=None, dz_in=rows, len=None, **drop)
    same(a, b, ("dx_out", "dout", "dwn_out", "via_skip"))
    # backward, last launch: the input gradient's rows -> dx_bct; the partial rows are plain stores
    kw = P.bwd[3]
    a, b = reissue(P, "bwd", kw), reissue(P, "bwd", kw, dx_bct=None, dx_out=torch.empty(P.R, C, device=dev()), **drop)
    assert torch.equal(a.out["dx_bct"].cpu(), unsqueeze_index(P, b.out["dx_out"])) and torch.equal(a.out["dx_bct"], unsq_kernel(b.out["dx_out"]))
    assert torch.equal(a.partials, b.partials) and a.out["dx_bct"].abs().max().item() > 0
    # reverse, first and last launches
    kw = P.rev[0]
    rows = squeeze_index(P, kw["z_bct"]).to(dev())
    a, b = reissue(P, "rev", kw), reissue(P, "rev", kw, z_bct=None, x=None, x_in=rows, len=None, **drop)
    assert torch.equal(a.out["x"], rows)
    same(a, b, ("h_next",))
    kw = P.rev[3]
    a, b = reissue(P, "rev", kw), reissue(P, "rev", kw, x_bct=None, x=torch.empty(P.R, C, device=dev()), len=None, **drop)
    assert torch.equal(a.out["x_bct"].cpu(), unsqueeze_index(P, b.out["x"])) and torch.equal(a.out["x_bct"], unsq_kernel(b.out["x"]))


# ----------------------------------------------------------------------------- prefetch buffers are inert
MAGIC = 0x9E3779B9


def crafted_prefetch_lists():
    """256 KiB buffers, one 16-byte chunk per prefetch thread (64 workgroups x 256): the word 0x9E3779B9 in each of the chunk's four
    positions, all-zero chunks, all-ones chunks"""
    n = 64 * 256
    bufs = []
    for pos in range(4):
        a = np.zeros((n, 4), dtype=np.uint32)
        a[:, pos] = MAGIC
        bufs.append((f"0x9E3779B9 in word {pos}", a))
    bufs.append(("zeros", np.zeros((n, 4), dtype=np.uint32)))
    bufs.append(("ones", np.full((n, 4), 0xFFFFFFFF, dtype=np.uint32)))
    out = []
    for name, a in bufs:
        t = torch.from_numpy(a.view(np.int32)).to(dev())
        out.append((name, dict(pf_ptr=[t] + [None] * 15, pf_bytes=[n * 16] + [0] * 15)))
    return out


def test_prefetch_buffers_are_inert(built):
    """No output of a boundary launch depends on the bytes of the buffers in pf_ptr: one head + tail launch of each direction with
    its real prefetch list, with none, and with crafted buffers — every run inside the float64 bounds, logdet[0] (pre-filled, += )
    included.  (The forward kernel used to store the XOR of the prefetched words over logdet[0] when it equalled 0x9E3779B9: the
    first crafted buffer.)"""
    P = record("ragged", False)
    none = dict(pf_ptr=[None] * 16, pf_bytes=[0] * 16)
    lists = [("real list", {}), ("no list", none)] + crafted_prefetch_lists()
    for kind, kws, fn in (("fwd", P.fwd, check_fwd), ("bwd", P.bwd, check_bwd), ("rev", P.rev, check_rev)):
        kw = kws[1]
        assert kw.get("pf_ptr") is not None and kw["pf_ptr"][0] is not None and kw["pf_bytes"][0] > 0, kind
        for name, over in lists:
            fn(P, 1, reissue(P, kind, kw, **over), f" [prefetch: {name}]")


# ----------------------------------------------------------------------------- the five-launch path's kernels
@pytest.mark.parametrize("ss", [False, True])
def test_five_launch_kernels_against_float64(built, ss):
    """gt_coupling_fwd / _bwd / _rev and gt_actnorm_invconv_fwd / _bwd / _rev called directly on the operands of a recorded boundary
    launch, against the same float64 operators"""
    from glow_tts_amd import flow_impl
    from glow_tts_amd._lib import call
    P = record("ragged", ss)
    rc, st, B, R, mk = P.rc, flow_impl._st(dev()), P.B, P.R, P.mk
    kw = P.fwd[1]                                                                # tail of block 0 + head of block 1
    g = torch.Generator().manual_seed(3)
    f32 = dict(dtype=F32, device=dev())
    # [m | logs]: the end conv's m in fp32 beside the raw logs the boundary launch stored
    cbp = P.dec.flows[2]
    m = conv_rows(t64(kw["wn_out"]), Wf(cbp.end.pc_frag, C, H), kw["b_end"])[0][:, :HALF]
    outp = torch.cat([m.float().to(dev()), kw["logs_raw"]], 1).contiguous()
    o, y = t64(outp), t64(kw["y"])
    prior = prior_of(B)
    z, logdet = torch.full((R, C), CAN, **f32), prior.clone()
    call.gt_coupling_fwd(outp, kw["y"], z, rc.rowmask, logdet, B, R, C, rc.Tp, rc.row0, int(ss), st)
    dz = torch.randn(R, C, generator=g).to(dev()).contiguous()                   # unmasked: the kernel masks
    dx, dout = torch.full((R, C), CAN, **f32), torch.full((R, C), CAN, dtype=torch.bfloat16, device=dev())
    call.gt_coupling_bwd(outp, kw["y"], dz, P.dlogdet, rc.rowmask, dx, dout, B, R, C, rc.Tp, rc.row0, int(ss), st)
    xr = torch.full((R, C), CAN, **f32)
    call.gt_coupling_rev(outp, z, xr, rc.rowmask, R, C, int(ss), st)
    torch.cuda.synchronize()
    for t in (z, dx, dout, xr):
        assert not (t.float() == CAN).any()
    name = f"five-launch {P.tag}"
    f = B64.coupling_fwd(o, y, P.mask, P.rowutt, B, ss)
    fu = B64.coupling_fwd(o, y, P.mask, B64.credit_neighbour(P.rowutt, P.mask), B, ss)
    pr = t64(prior)
    dld = t64(P.dlogdet)
    c = B64.coupling_bwd(o[:, HALF:], y[:, HALF:], t64(dz), dld, P.mask, P.rowutt, ss)
    cu = B64.coupling_bwd(o[:, HALF:], y[:, HALF:], t64(dz), dld, P.mask, B64.credit_neighbour(P.rowutt, P.mask), ss)
    zq = t64(z)
    xv, bx = B64.coupling_rev(o, zq, P.mask, ss)
    ones = torch.ones_like(P.mask)                                               # planted: the row mask left out
    z_nm = B64.coupling_fwd(o, y, ones, P.rowutt, B, ss)["z"][0]
    dx_nm = B64.coupling_bwd(o[:, HALF:], y[:, HALF:], t64(dz), dld, ones, P.rowutt, ss)["dx"][0]
    x_nm = B64.coupling_rev(o, zq, ones, ss)[0]
    if ss:
        t = lambda a: a.float()
        f32t = B64.coupling_fwd(t(o), t(y), t(P.mask), P.rowutt, B, True)
        hold_twin("coupling_fwd.z", name, zq[:, HALF:], f["z"][0][:, HALF:], f32t["z"][0][:, HALF:], z_nm[:, HALF:])
        hold_twin("coupling_fwd.logdet", name, t64(logdet), pr + f["logdet"][0], (pr + f32t["logdet"][0].double()).float(), pr + fu["logdet"][0])
        c32 = B64.coupling_bwd(t(o[:, HALF:]), t(y[:, HALF:]), t(t64(dz)), t(dld), t(P.mask), P.rowutt, True)
        hold_twin("coupling_bwd.dx", name, t64(dx)[:, HALF:], c["dx"][0][:, HALF:], c32["dx"][0][:, HALF:], dx_nm[:, HALF:])
        nod = B64.coupling_bwd(o[:, HALF:], y[:, HALF:], t64(dz), dld, P.mask, P.rowutt, True, scale_derivative=False)
        check_with_control(name + " gt_coupling_bwd dout [sigmoid_scale derivative omitted]", t64(dout), c["dout"][0], c["dout"][1], nod["dout"][0], kind="bf16")
        hold_twin("coupling_rev.x", name, t64(xr)[:, HALF:], xv[:, HALF:], B64.coupling_rev(t(o), t(zq), t(P.mask), True)[0][:, HALF:],
                  x_nm[:, HALF:])
    else:
        check_with_control(name + " gt_coupling_fwd z", zq, f["z"][0], f["z"][1], z_nm)
        check_with_control(name + " gt_coupling_fwd logdet", t64(logdet), pr + f["logdet"][0], gamma(f["logdet"][2] + 16) * (pr.abs() + f["logdet"][1]),
                           pr + fu["logdet"][0])
        check_with_control(name + " gt_coupling_bwd dx", t64(dx), c["dx"][0], c["dx"][1], dx_nm)
        check_with_control(name + " gt_coupling_rev x", t64(xr), xv, bx, x_nm)
    check_with_control(name + " gt_coupling_bwd dout", t64(dout), c["dout"][0], c["dout"][1], cu["dout"][0], kind="bf16")
    assert torch.equal(z[:, :HALF], kw["y"][:, :HALF]) and torch.equal(dx[:, :HALF], dz[:, :HALF]) and torch.equal(xr[:, :HALF], z[:, :HALF])
    # ActNorm + InvConvNear
    lgd, bsd, Wdv = kw["an_logs"].detach().reshape(-1).contiguous(), kw["an_bias"].detach().reshape(-1).contiguous(), kw["w_ic"].detach().contiguous()
    scal = torch.empty(18, **f32)
    call.gt_flow_scalars(lgd, C, Wdv, scal, st)
    xin = kw["z"]
    yk, y0 = torch.full((R, C), CAN, **f32), torch.full((R, HALF), CAN, dtype=torch.bfloat16, device=dev())
    ld2 = prior.clone()
    call.gt_actnorm_invconv_fwd(xin, yk, y0, HALF, lgd, bsd, Wdv, scal, rc.rowmask, rc.lengths, ld2, B, R, C, st)
    xk, x0 = torch.full((R, C), CAN, **f32), torch.full((R, HALF), CAN, dtype=torch.bfloat16, device=dev())
    call.gt_actnorm_invconv_rev(yk, xk, x0, HALF, lgd, bsd, scal, rc.rowmask, R, C, st)
    dy = (torch.randn(R, C, generator=g).to(dev())).contiguous()                 # unmasked: the kernel masks
    dxk = torch.full((R, C), CAN, **f32)
    acc = {k: prior_of(n, 3.0) for k, n in zip(ACC, (C, C, 16))}
    got = {k: v.clone() for k, v in acc.items()}
    call.gt_actnorm_invconv_bwd(xin, dy, dxk, lgd, bsd, Wdv, scal, rc.rowmask, rc.lengths, P.dlogdet, got["d_an_logs"], got["d_an_bias"], got["d_w_ic"],
                                B, R, C, st)
    torch.cuda.synchronize()
    assert torch.equal(scal, kw["scal"])                                         # gt_flow_scalars_multi wrote the same 18 values
    for t in (yk, y0, xk, x0, dxk):
        assert not (t.float() == CAN).any()
    lg, bs, W, sc = flat(lgd), flat(bsd), t64(Wdv).reshape(4, 4), flat(scal)
    x64 = t64(xin)
    yr, yb, _, _ = B64.actnorm_invconv_fwd(x64, lg, bs, W, P.mask)
    check_with_control(name + " gt_actnorm_invconv_fwd y", t64(yk), yr, yb, B64.actnorm_invconv_fwd(x64, lg, bs, W.T, P.mask)[0])
    assert np.array_equal(rows64.bits(y0), rows64.f2bf(yk[:, :HALF].cpu().numpy()))
    pl, pb = B64.pair_logdet(sc, P.lens64, C)
    check_with_control(name + " gt_actnorm_invconv_fwd logdet", t64(ld2), pr + pl, pb + U * pr.abs(), pr + pl.roll(1))   # the neighbour's length
    Winv = sc[2:].reshape(4, 4).T
    xq, bxq = B64.actnorm_invconv_rev(t64(yk), lg, bs, Winv, P.mask)
    check_with_control(name + " gt_actnorm_invconv_rev x", t64(xk), xq, bxq, B64.actnorm_invconv_rev(t64(yk), lg, bs, Winv.T, P.mask)[0])
    assert np.array_equal(rows64.bits(x0), rows64.f2bf(xk[:, :HALF].cpu().numpy()))
    args = (x64, t64(dy), lg, bs, W, sc[2:].reshape(4, 4), P.mask, dld, P.lens64)
    ref = B64.actnorm_invconv_bwd(*args, slabs=(R + 127) // 128 + 8)
    row = int((t64(dy).abs().sum(1) * P.mask).argmax())
    bad_row, bad_inv, bad_book = (B64.actnorm_invconv_bwd(*args, **d) for d in (dict(drop_row=row), dict(use_inverse=True), dict(bookkeeping=False)))
    check_with_control(name + " gt_actnorm_invconv_bwd dx", t64(dxk), ref["dx"][0], ref["dx"][1],
                       B64.actnorm_invconv_bwd(*(args[:6] + (ones,) + args[7:]))["dx"][0])
    for k in ACC:
        p = t64(acc[k])
        want = ref[k][0] + p
        bound = ref[k][1] + U * (want.abs() + p.abs())
        check_with_control(f"{name} gt_actnorm_invconv_bwd {k}", t64(got[k]), want, bound, bad_row[k][0] + p)
        if k == "d_w_ic":
            seen(f"{name} {k} [W^-1 for W^-T]", t64(got[k]), want, bound, bad_inv[k][0] + p)
        if k == "d_an_logs":
            seen(f"{name} {k} [sum dlogdet len omitted]", t64(got[k]), want, bound, bad_book[k][0] + p)


def test_flow_scalars_against_float64(built):
    """gt_flow_scalars and gt_flow_scalars_multi: sum logs under the rule (160 addends); log det W and W^-T (outside it: a 4x4
    inverse) against the float32 twin.  Weights I + 0.3 randn as tests/test_decoder_gpu.py draws them, and one worse-conditioned
    matrix, I + 0.3 randn with its last row replaced by 0.98 row 0 + 0.02 row 3 (condition number printed: 252)."""
    from glow_tts_amd import flow_impl
    from glow_tts_amd._lib import call
    st = flow_impl._st(dev())
    g = torch.Generator().manual_seed(5)
    Ws = [torch.eye(4) + 0.3 * torch.randn(4, 4, generator=g) for _ in range(3)]
    bad = Ws[0].clone()
    bad[3] = 0.98 * bad[0] + 0.02 * bad[3]
    Ws.append(bad)
    Ws = [w if torch.det(w) > 0 else torch.cat([-w[:1], w[1:]]) for w in Ws]    # log det needs det > 0
    logs = [(torch.randn(C, generator=g) * 0.2) for _ in Ws]
    n = len(Ws)
    Wd_, lg_ = [w.contiguous().to(dev()) for w in Ws], [l.to(dev()) for l in logs]
    multi = torch.empty(n, 18, device=dev())
    lp = torch.tensor([l.data_ptr() for l in lg_], dtype=torch.int64).to(dev())
    wp = torch.tensor([w.data_ptr() for w in Wd_], dtype=torch.int64).to(dev())
    call.gt_flow_scalars_multi(lp, wp, C, multi, n, st)
    for i in range(n):
        one = torch.empty(18, device=dev())
        call.gt_flow_scalars(lg_[i], C, Wd_[i], one, st)
        torch.cuda.synchronize()
        assert torch.equal(one, multi[i])
        ref = B64.flow_scalars(logs[i].double(), Ws[i].double())
        twin = B64.flow_scalars(logs[i], Ws[i])
        cond = float(torch.linalg.cond(Ws[i].double()))
        name = f"gt_flow_scalars W[{i}] cond {cond:.3g}"
        r = check(name + " sum logs", t64(one[:1]), ref[:1], gamma(C) * logs[i].double().abs().sum().reshape(1))
        print(r)
        assert r.ok, str(r)
        swapped = torch.cat([ref[:2], ref[2:].reshape(4, 4).T.reshape(-1)])     # W^-1 where W^-T belongs
        hold_twin("flow_scalars", name, one.cpu()[1:], ref[1:], twin[1:], swapped[1:])
    assert cond > 50
