"""The whole-WaveNet kernels (gt_wn_stack_fwd / _bwd, and gt_wn_layer_fwd through set_stack(False)) against float64 on their own
bf16 operands, under the rule of oracle/rows64.py.  Teacher forcing: forward layer i is checked from the kernel's own x_i (x0 or
x_out[i-1]) and acts_i; the backward's dx[j] from the kernel's dpre_j and dx[j+1], dpre_{j-1} from the kernel's dx[j], the saved
T / S and via_skip — so no tolerance grows with depth.  Weights come from the decoded images (tests/test_pack_images_gpu.py ties
those to the parameters).  Every check runs a planted-defect control (one (tap, k) weight column zeroed: one product gone from every
output element) that must miss by >= 3x."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

from oracle import dropmask, rows64

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "golden"))
from fill import fill_module  # noqa: E402

pytestmark = pytest.mark.gpu
H = 192


def dev():
    return torch.device("cuda:0")


def small_rows():
    """ragged, with 1- and 2-frame utterances; R is no multiple of the rows a workgroup owns"""
    from glow_tts_amd import ops
    lens = [37, 1, 2, 60, 13]
    return ops.RowsCtx(torch.tensor(lens, dtype=torch.int32, device=dev()), 60, lengths_host=lens, round_to=8)


def cfg2_rows():
    """as tests/test_wn_stack_bwd_gpu.py: a cfg-2-shaped batch, about 9 k squeezed rows (the 64-row form)"""
    from glow_tts_amd import ops
    g = torch.Generator().manual_seed(1234)
    t_y = torch.randint(150, 401, (32,), generator=g) * 2
    t_y[0] = 800
    lens = [int(v) // 2 for v in t_y]
    return ops.RowsCtx(torch.tensor(lens, dtype=torch.int32, device=dev()), 400, lengths_host=lens, round_to=512)


def _keep(seed, R, p):
    if p <= 0:
        return None
    from glow_tts_amd import ops
    word = int(ops.seed_word(dev()).item()) & 0xFFFFFFFF
    return dropmask.drop_keep_gate(dropmask.word_seed(word, seed), np.arange(R)[:, None], np.arange(H)[None, :], dropmask.thresh16(p))


def _fwd_dispatch(kw):
    """(conditioning mode, dropout on) that gt_wn_stack_fwd instantiates for these arguments (COND = 2 with the affine pointers,
    1 with cond, per utterance when B > 0, per row when B == 0; DROP when drop_p > 0)"""
    if kw.get("aff_w") is not None:
        mode = "affine"
    elif kw["cond"] is None:
        mode = "none"
    else:
        mode = "speaker" if kw["B"] > 0 else "per_row"
    return mode, kw["drop_p"] > 0


def _run(rc, n, mode, p, monkeypatch, stack=True, seed=77, log=print):
    """Forward through flow_impl.wn_fwd (stack=False: set_stack(False, False); a long batch takes the per-layer kernels by itself)
    and check every layer's T, S, acts and x_out.  Returns what the backward check needs and which forward ran."""
    from glow_tts_amd import _lib, flow_impl, modules
    R = rc.R
    gin = 256 if mode == "speaker" else 0
    wn = fill_module(modules.WN(160, H, 5, 1, n, gin, p), "wn.").to(dev())
    modules.prepare_all(wn)
    L = _lib.lib()
    g = torch.Generator().manual_seed(10 * n + len(mode))
    rm = rc.rowmask
    h0 = (torch.randn(R, H, generator=g).to(dev()) * rm[:, None]).to(torch.bfloat16)
    cond, affine = None, None
    if mode == "speaker":
        cond = (torch.randn(rc.B, 2 * H * n, generator=g) * 0.3).to(dev())
    elif mode == "per_row":
        cond = (torch.randn(R, 2 * H * n, generator=g) * 0.3).to(dev())
    elif mode == "affine":
        affine = ((torch.randn(R, 2, generator=g)).to(dev()), (torch.randn(H * n, generator=g) * 0.3).to(dev()),
                  (torch.randn(H * n, generator=g) * 0.1).to(dev()))
    calls, fill = [], _lib.fill_args
    monkeypatch.setattr(_lib, "fill_args", lambda cls, **kw: calls.append((cls, kw)) or fill(cls, **kw))
    wn.set_stack(stack, stack)
    try:
        _, saved = flow_impl.wn_fwd(rc, wn, h0, cond, True, seed, cond_per_row=mode == "per_row", layers_only=True, affine=affine)
    finally:
        wn.set_stack(True, True)
        monkeypatch.setattr(_lib, "fill_args", fill)
    launched = [kw for cls, kw in calls if cls is _lib.WnStackFwdArgs]
    ran_stack = stack and flow_impl._stack_pays(R, n, dev())
    assert len(launched) == int(ran_stack)
    if ran_stack:                                              # the instantiation this case claims
        assert _fwd_dispatch(launched[0]) == (mode, p > 0)
    xs, ts, ss, acts_all, _, _ = saved
    torch.cuda.synchronize()
    tag = f"{'stack' if ran_stack else 'layer'} fwd R={R} form={L.gt_wn_stack_row_blocks(R, n, 1)} n={n} {mode} p={p}"
    # conditioning rows (float64) and their bound
    rowutt = rc.rowutt.long().cpu()
    if mode == "speaker":
        c64, cb = rows64.t64(cond)[rowutt], 0
    elif mode == "per_row":
        c64, cb = rows64.t64(cond), 0
    elif mode == "affine":
        c64, cb = rows64.affine_cond(affine[0], affine[1], affine[2], H, n)
    else:
        c64 = None
    scale = float(dropmask.scale(p)) if p > 0 else 1.0
    rm64 = rows64.t64(rm)[:, None]
    for i in range(n):
        il = wn.in_layers[i]
        W = rows64.decode_fwd(il.pc.fwd, 2 * H, H, 5, il.pc.Np_f, il.pc.Kp_f, il.pc.flags)
        x = rows64.t64(xs[i])
        Y, S = rows64.conv_rows(x, W, il.bias)
        Yb = rows64.conv_rows(x, rows64.drop_weight_entry(W), il.bias)[0]
        keep = _keep(seed + i, R, p)
        ci = None if c64 is None else c64[:, 2 * H * i:2 * H * (i + 1)]
        cbi = None if c64 is None or isinstance(cb, int) else cb[:, 2 * H * i:2 * H * (i + 1)]
        ref, _ = rows64.gate_fwd(Y, S, 5 * H + 1, H, ci, cbi, keep, scale)
        bad, _ = rows64.gate_fwd(Yb, S, 5 * H + 1, H, ci, cbi, keep, scale)
        got = {"t": ts[i], "s": ss[i], "acts": acts_all[:, H * i:H * (i + 1)]}
        for k in ("t", "s", "acts"):
            rows64.check_with_control(f"{tag} layer {i} {k}", rows64.t64(got[k]), ref[k][0], ref[k][1], bad[k][0], kind="bf16", log=log)
        if i < n - 1:                                          # x_out[i] from the kernel's acts_i and x_i
            rs = wn.res_skip_layers[i]
            Wr = rows64.decode_fwd(rs.pc_res.fwd, H, H, 1, rs.pc_res.Np_f, rs.pc_res.Kp_f, rs.pc_res.flags)
            a = rows64.t64(got["acts"])
            Yr, Sr = rows64.conv_rows(a, Wr, rs.bias[:H])
            want = (Yr + x) * rm64
            bound = rows64.gamma(H + 2) * (Sr + x.abs()) * rm64
            badr = (rows64.conv_rows(a, rows64.drop_weight_entry(Wr), rs.bias[:H])[0] + x) * rm64
            rows64.check_with_control(f"{tag} layer {i} x_out", rows64.t64(xs[i + 1]), want, bound, badr, kind="bf16", log=log)
    return wn, saved, affine, (lambda i: _keep(seed + i, R, p)), ran_stack


def _launch_stack_bwd(rc, wn, ts, ss, via, n, p, seed, need_c):
    from glow_tts_amd import _lib, flow_impl
    R = rc.R
    bf = dict(dtype=torch.bfloat16, device=dev())
    dpre = [torch.empty(R, 2 * H, **bf) for _ in range(n)]
    dpre_c = [torch.empty(R, 2 * H, **bf) if need_c else None for _ in range(n)]
    dxs = [torch.empty(R, H, **bf) for _ in range(n)]
    pad = [None] * (4 - n)
    args = _lib.fill_args(
        _lib.WnStackBwdArgs, via_skip=via, ldvs=via.stride(0), gate_t=list(ts) + pad, gate_s=list(ss) + pad,
        w_in_d=[il.pc.dgrad for il in wn.in_layers] + pad, w_res_d=[rs.pc_res.dgrad for rs in wn.res_skip_layers[:n - 1]] + [None] + pad,
        rowmask=rc.rowmask, dpre=dpre + pad, dpre_c=dpre_c + pad, dx=dxs + pad, R=R, H=H, taps=5, n_layers=n,
        drop_p=float(p), drop_seed=int(seed), seed_dev=flow_impl.seed_word(dev()) if p > 0 else None)
    _lib.check(_lib.lib().gt_wn_stack_bwd(ctypes.byref(args), flow_impl._st(dev())), "gt_wn_stack_bwd")
    return dpre, dpre_c, dxs


def _launch_layer_bwd(rc, wn, ts, ss, via, n, p, seed, need_c):
    """the per-layer launches of flow_impl._wn_bwd_fused with the stack off: gt_gate_bwd for the top layer, gt_wn_layer_bwd per layer
    boundary, and gt_wn_layer_bwd without its second stage for d x0"""
    from glow_tts_amd import _lib, flow_impl
    L, R, ptr = _lib.lib(), rc.R, _lib.ptr
    st, sw = flow_impl._st(dev()), (flow_impl.seed_word(dev()) if p > 0 else None)
    bf = dict(dtype=torch.bfloat16, device=dev())
    dpre, dpre_c, dxs = [None] * n, [None] * n, [None] * n
    i = n - 1
    dpre[i] = torch.empty(R, 2 * H, **bf)
    dpre_c[i] = torch.empty(R, 2 * H, **bf) if need_c else None
    v = via[:, H * i:H * (i + 1)]
    _lib.check(L.gt_gate_bwd(ptr(v), v.stride(0), ptr(ts[i]), ptr(ss[i]), H, ptr(dpre[i]), 2 * H, ptr(dpre_c[i]), R, H, float(p),
                             int(seed + i), ptr(sw), st), "gt_gate_bwd")
    dX = None
    for i in reversed(range(n - 1)):
        rs, nxt = wn.res_skip_layers[i], wn.in_layers[i + 1]
        dxs[i + 1] = torch.empty(R, H, **bf)
        dpre[i] = torch.empty(R, 2 * H, **bf)
        dpre_c[i] = torch.empty(R, 2 * H, **bf) if need_c else None
        v = via[:, H * i:H * (i + 1)]
        _lib.check(L.gt_wn_layer_bwd(ptr(dpre[i + 1]), 2 * H, ptr(nxt.pc.dgrad), ptr(dX), H, ptr(rc.rowmask), ptr(dxs[i + 1]), H,
                                     ptr(rs.pc_res.dgrad), ptr(v), v.stride(0), ptr(ts[i]), ptr(ss[i]), H, ptr(dpre[i]), ptr(dpre_c[i]),
                                     2 * H, R, H, 5, float(p), int(seed + i), ptr(sw), None, 0, None, st), "gt_wn_layer_bwd")
        dX = dxs[i + 1]
    dxs[0] = torch.empty(R, H, **bf)
    _lib.check(L.gt_wn_layer_bwd(ptr(dpre[0]), 2 * H, ptr(wn.in_layers[0].pc.dgrad), ptr(dX), H, ptr(rc.rowmask), ptr(dxs[0]), H,
                                 None, None, 0, None, None, 0, None, None, 0, R, H, 5, 0.0, 0, None, None, 0, None, st), "gt_wn_layer_bwd")
    return dpre, dpre_c, dxs


def _bwd(rc, wn, saved, n, mode, p, affine, keeps, stack=True, log=print):
    """Backward of the same WaveNet from random (masked) skip-path gradients: the whole-WaveNet kernel or the per-layer ones, then
    every layer's dpre / dpre_c / dx teacher-forced, the speaker d cond sums and the affine parameters' gradients."""
    from glow_tts_amd import _lib, flow_impl
    R = rc.R
    L = _lib.lib()
    xs, ts, ss, acts_all, _, seed = saved
    g = torch.Generator().manual_seed(99 + n)
    rm = rc.rowmask
    via = (torch.randn(R, n * H, generator=g).to(dev()) * rm[:, None]).to(torch.bfloat16)
    need_c = p > 0 and mode != "none"                  # d cond differs from d pre only behind the dropout mask
    launch = _launch_stack_bwd if stack else _launch_layer_bwd
    dpre, dpre_c, dxs = launch(rc, wn, ts, ss, via, n, p, seed, need_c)
    torch.cuda.synchronize()
    tag = f"{'stack' if stack else 'layer'} bwd R={R} form={L.gt_wn_stack_row_blocks(R, n, 0)} n={n} {mode} p={p}"
    scale = float(dropmask.scale(p)) if p > 0 else 1.0
    rm64 = rows64.t64(rm)[:, None]
    v64 = rows64.t64(via)

    def check_dpre(j, dd, e_dd, dd_bad):
        keep = keeps(j)
        c, bc, d, bd = rows64.gate_bwd(dd, e_dd, ts[j], ss[j], keep, scale)
        cb, _, db, _ = rows64.gate_bwd(dd_bad, e_dd, ts[j], ss[j], keep, scale)
        rows64.check_with_control(f"{tag} dpre[{j}]", rows64.t64(dpre[j]), d, bd, db, kind="bf16", log=log)
        if dpre_c[j] is not None:
            rows64.check_with_control(f"{tag} dpre_c[{j}]", rows64.t64(dpre_c[j]), c, bc, cb, kind="bf16", log=log)

    top = v64[:, H * (n - 1):]
    bad_top = rows64.drop_row(top, int(top.abs().sum(1).argmax()))       # (no weights in the top gate: a dropped row instead)
    check_dpre(n - 1, top, torch.zeros_like(top), bad_top)
    for j in reversed(range(n)):
        il = wn.in_layers[j]
        Wd = rows64.conv_rows_dgrad_weights(rows64.decode_dgrad(il.pc.dgrad, 2 * H, H, 5, il.pc.Np_d, il.pc.Kp_d, il.pc.flags))
        dp = rows64.t64(dpre[j])
        Y, S = rows64.conv_rows(dp, Wd)
        Yb = rows64.conv_rows(dp, rows64.drop_weight_entry(Wd))[0]
        nxt = rows64.t64(dxs[j + 1]) if j < n - 1 else torch.zeros_like(Y)
        want, badw = (Y + nxt) * rm64, (Yb + nxt) * rm64
        rows64.check_with_control(f"{tag} dx[{j}]", rows64.t64(dxs[j]), want, rows64.gamma(10 * H + 1) * (S + nxt.abs()) * rm64,
                                  badw, kind="bf16", log=log)
        if j > 0:                                              # dpre_{j-1} from the kernel's dx[j]
            rs = wn.res_skip_layers[j - 1]
            Wr = rows64.decode_dgrad(rs.pc_res.dgrad, H, H, 1, rs.pc_res.Np_d, rs.pc_res.Kp_d, rs.pc_res.flags)[0]   # [co][ci]
            dx = rows64.t64(dxs[j])
            vs = v64[:, H * (j - 1):H * j]
            dd = dx @ Wr + vs
            e_dd = rows64.gamma(H + 1) * (dx.abs() @ Wr.abs() + vs.abs())
            Wb = Wr.clone()
            Wb[:, H // 3] = 0
            check_dpre(j - 1, dd, e_dd, dx @ Wb + vs)
    # d cond: per-utterance sums of dpre_c (speaker) and the affine parameters' gradients, from the kernel's rows
    src = dpre_c if need_c else dpre
    if mode == "speaker":
        for i in range(n):
            out = torch.zeros(rc.B, 2 * H, device=dev())
            rc.utt_sum(src[i], out)
            torch.cuda.synchronize()
            s = rows64.t64(src[i]) * rm64
            ref, S = rows64.utt_sum(s, rc.rowutt.long().cpu(), rc.B)
            bad = rows64.utt_sum(rows64.drop_row(s, int(s.abs().sum(1).argmax())), rc.rowutt.long().cpu(), rc.B)[0]
            rows64.check_with_control(f"{tag} dcond[{i}]", out, ref, rows64.gamma(R) * S, bad, log=log)
    if mode == "affine":
        O = H * n
        dw, db = torch.zeros(O, device=dev()), torch.zeros(O, device=dev())
        s4 = src + [None] * (4 - n)
        _lib.check(L.gt_cond_affine_grads(_lib.ptr(s4[0]), _lib.ptr(s4[1]), _lib.ptr(s4[2]), _lib.ptr(s4[3]), 2 * H, _lib.ptr(affine[0]),
                                          _lib.ptr(dw), _lib.ptr(db), R, H, n, flow_impl._st(dev())), "gt_cond_affine_grads")
        torch.cuda.synchronize()
        sig = rows64.t64(affine[0])
        rw, rb, Sw, Sb = (torch.zeros(O, dtype=torch.float64) for _ in range(4))
        bw = torch.zeros(O, dtype=torch.float64)
        m_bad = int(rows64.t64(src[0]).abs().sum(1).argmax())
        for i in range(n):
            par, off = (2 * H * i) // O, (2 * H * i) % O
            d = rows64.t64(src[i])
            rw[off:off + 2 * H] += (d * sig[:, par:par + 1]).sum(0)
            Sw[off:off + 2 * H] += (d * sig[:, par:par + 1]).abs().sum(0)
            rb[off:off + 2 * H] += d.sum(0)
            Sb[off:off + 2 * H] += d.abs().sum(0)
            bw[off:off + 2 * H] += (rows64.drop_row(d, m_bad) * sig[:, par:par + 1]).sum(0)
        K = R * n
        rows64.check_with_control(f"{tag} affine dw", dw, rw, rows64.gamma(K) * Sw, bw, log=log)
        rows64.check_with_control(f"{tag} affine db", db, rb, rows64.gamma(K) * Sb, _drop_bias(src, m_bad, n, O), log=log)


def _drop_bias(src, m, n, O):
    """the affine bias gradient with row m of every layer's d pre left out (the planted defect)"""
    out = torch.zeros(O, dtype=torch.float64)
    for i in range(n):
        off = (2 * H * i) % O
        d = rows64.t64(src[i])
        out[off:off + 2 * H] += d.sum(0) - d[m]
    return out


def _rows_exact(R):
    """a ragged batch of exactly R rows (no rounding rows): utterances of 400 frames and a shorter last one"""
    from glow_tts_amd import ops
    B = max(1, -(-R // 404))
    lens = [400] * (B - 1) + [R - 404 * (B - 1) - 4]
    if lens[-1] < 1:
        lens[0] -= 1 - lens[-1]
        lens[-1] = 1
    rc = ops.RowsCtx(torch.tensor(lens, dtype=torch.int32, device=dev()), max(lens), lengths_host=lens, round_to=1)
    assert rc.R == R
    return rc


def _switch(n, fwd):
    """the smallest R for which gt_wn_stack_fwd (fwd = 1) / _bwd (fwd = 0) takes the 64-row form"""
    from glow_tts_amd import _lib
    lo, hi = 1, 1 << 16
    assert _lib.lib().gt_wn_stack_row_blocks(hi, n, fwd) == 2
    while lo < hi:
        mid = (lo + hi) // 2
        if _lib.lib().gt_wn_stack_row_blocks(mid, n, fwd) == 2:
            hi = mid
        else:
            lo = mid + 1
    return lo


def _forms(R, n):
    from glow_tts_amd import _lib
    return _lib.lib().gt_wn_stack_row_blocks(R, n, 1), _lib.lib().gt_wn_stack_row_blocks(R, n, 0)


SMALL = [(n, "speaker", 0.05) for n in (1, 2, 3)] + [(4, m, p) for m in ("none", "speaker", "per_row") for p in (0.0, 0.05)] + \
        [(2, "affine", 0.05), (4, "affine", 0.05), (4, "affine", 0.0)]


@pytest.mark.parametrize("n,mode,p", SMALL)
def test_wn_stack_small_ragged_vs_float64(built, monkeypatch, n, mode, p):
    from glow_tts_amd import _lib
    rc = small_rows()
    own32 = _lib.lib().gt_wn_stack_rows_per_workgroup(n) - 32          # the 32-row form owns 32 - 4 (n - 1) rows per workgroup
    assert rc.R % own32 != 0
    assert _forms(rc.R, n) == (1, 1)                                     # 32-row form both ways
    wn, saved, affine, keeps, ran_stack = _run(rc, n, mode, p, monkeypatch)
    assert ran_stack
    _bwd(rc, wn, saved, n, mode, p, affine, keeps)


@pytest.mark.parametrize("mode,p", [(m, p) for m in ("none", "speaker", "per_row", "affine") for p in (0.0, 0.05)])
def test_wn_stack_64_row_form_vs_float64(built, monkeypatch, mode, p):
    rc = cfg2_rows()
    assert _forms(rc.R, 4) == (2, 2)
    wn, saved, affine, keeps, ran_stack = _run(rc, 4, mode, p, monkeypatch)
    assert ran_stack
    _bwd(rc, wn, saved, 4, mode, p, affine, keeps)


# one 64-row tile (64 - 4 (n - 1) owned rows) either side of each switch; between the two switches the forward runs the 32-row form
# and the backward the 64-row form
EDGES = [("bwd", -1, "none", 0.05, (1, 1)), ("bwd", 0, "speaker", 0.05, (1, 2)), ("fwd", -1, "per_row", 0.05, (1, 2)),
         ("fwd", 0, "affine", 0.05, (2, 2))]


@pytest.mark.parametrize("which,side,mode,p,forms", EDGES)
def test_wn_stack_around_the_row_form_switch_vs_float64(built, monkeypatch, which, side, mode, p, forms):
    from glow_tts_amd import _lib
    n = 4
    R = _switch(n, int(which == "fwd")) + side * _lib.lib().gt_wn_stack_rows_per_workgroup(n)
    assert _forms(R, n) == forms, (R, _forms(R, n))
    rc = _rows_exact(R)
    wn, saved, affine, keeps, ran_stack = _run(rc, n, mode, p, monkeypatch)
    assert ran_stack
    _bwd(rc, wn, saved, n, mode, p, affine, keeps)


@pytest.mark.parametrize("mode,p", [("speaker", 0.05), ("none", 0.0)])
def test_wn_layer_kernels_vs_float64(built, monkeypatch, mode, p):
    """gt_wn_layer_fwd / gt_wn_layer_bwd / gt_gate_bwd (one launch per layer, set_stack(False)) under the same checks"""
    rc = small_rows()
    wn, saved, affine, keeps, ran_stack = _run(rc, 4, mode, p, monkeypatch, stack=False)
    assert not ran_stack
    _bwd(rc, wn, saved, 4, mode, p, affine, keeps, stack=False)


def test_wn_long_batch_takes_the_layer_kernels_vs_float64(built, monkeypatch):
    """a cfg-3-sized batch, where one launch per WaveNet would cost an extra round of workgroups (flow_impl._stack_pays is false):
    the default dispatch runs the per-layer kernels"""
    from glow_tts_amd import flow_impl
    lens = [436] * 31 + [1]
    from glow_tts_amd import ops
    rc = ops.RowsCtx(torch.tensor(lens, dtype=torch.int32, device=dev()), 436, lengths_host=lens, round_to=512)
    assert not flow_impl._stack_pays(rc.R, 4, dev())
    wn, saved, affine, keeps, ran_stack = _run(rc, 4, "speaker", 0.05, monkeypatch)
    assert not ran_stack
    _bwd(rc, wn, saved, 4, "speaker", 0.05, affine, keeps, stack=False)
