"""oracle/boundary64.py (the float64 operators tests/test_wn_boundary_fp64_gpu.py holds the boundary kernels to) pinned to
oracle/glowtts_ref.py run in float64 — actnorm_fwd, invconv_fwd, the coupling block's elementwise tail and their inverses — and its
backward operators pinned to autograd, sigmoid_scale on and off, on ragged masks with 1- and 2-frame utterances.  No GPU.

"Equal" for two float64 evaluations that sum in different orders (einsum / matmul) is EQ = 2^-44 of the tensor's largest magnitude
(256 float64 ulps); gradients, whose sums run over every row, 2^-40.  The float32 twin of every operator must also stay inside the
operator's own bound: a bound that fp32 arithmetic on the CPU breaks would be no bound for the kernel."""
import numpy as np
import pytest
import torch

from oracle import boundary64 as B64
from oracle import glowtts_ref as R
from oracle import rows64

EQ, EQ_GRAD = 2.0 ** -44, 2.0 ** -40
C, F64, F32 = 160, torch.float64, torch.float32
LENS = [9, 1, 2, 6, 0, 4]


def close(a, b, tol):
    return float((a - b).abs().max()) <= tol * max(1e-300, float(b.abs().max()))


def q(t):
    return t.float().double()


def to_rows(x):
    return x.permute(0, 2, 1).reshape(-1, x.shape[1])


def setup(seed=0):
    g = torch.Generator().manual_seed(seed)
    Bn, T = len(LENS), max(LENS)
    mask3 = (torch.arange(T)[None, :] < torch.tensor(LENS)[:, None]).unsqueeze(1).to(F64)
    rn = lambda *s: q(torch.randn(*s, generator=g, dtype=F64))          # float32-representable: the twin reads the same inputs
    I = dict(B=Bn, T=T, mask3=mask3, mask=mask3.reshape(-1), rowutt=torch.arange(Bn).repeat_interleave(T),
             lens=torch.tensor(LENS, dtype=F64), x=rn(Bn, C, T) * mask3, logs=rn(1, C, 1) * 0.3, bias=rn(1, C, 1) * 0.3,
             W=q(torch.eye(4, dtype=F64) + 0.3 * rn(4, 4)), out=rn(Bn, C, T), rz=rn(Bn, C, T), rl=rn(Bn))
    return I


def test_group_index_is_invconv_nears_grouping():
    idx = B64.group_index(C)
    assert idx.shape == (40, 4) and sorted(idx.reshape(-1).tolist()) == list(range(C))
    assert idx[3].tolist() == [6, 7, 86, 87]
    X = torch.randn(5, C, dtype=F64)
    assert torch.equal(B64.from_groups(B64.to_groups(X)), X)


def test_actnorm_invconv_forward_reverse_and_logdet_equal_the_reference():
    I = setup(1)
    P = {"a.logs": I["logs"], "a.bias": I["bias"], "i.weight": I["W"]}
    z1, ld1 = R.actnorm_fwd(P, "a.", I["x"], I["mask3"])
    z, ld2 = R.invconv_fwd(P, "i.", z1, I["mask3"])
    lg, bs = I["logs"].reshape(-1), I["bias"].reshape(-1)
    y, by, _, _ = B64.actnorm_invconv_fwd(to_rows(I["x"]), lg, bs, I["W"], I["mask"])
    assert close(y, to_rows(z), EQ)
    scal = B64.flow_scalars(lg, I["W"])
    assert close(scal[2:].reshape(4, 4), torch.linalg.inv(I["W"]).T, EQ) and close(scal[1], torch.logdet(I["W"]), EQ)
    ld, _ = B64.pair_logdet(scal, I["lens"], C)
    assert close(ld, ld1 + ld2, EQ)
    # the inverse maps: the reference inverts W in float32 (invconv_rev), so it pins the operator at float32's precision and the
    # round trip pins it at float64's
    P32 = {k: v.float() for k, v in P.items()}
    back = R.actnorm_rev(P32, "a.", R.invconv_rev(P32, "i.", z.float(), I["mask3"].float()), I["mask3"].float())
    xr, bx = B64.actnorm_invconv_rev(y, lg, bs, scal[2:].reshape(4, 4).T, I["mask"])
    assert close(xr, to_rows(back).double(), 2.0 ** -18) and close(xr, to_rows(I["x"]), 2.0 ** -36)
    # the float32 twin stays inside the bounds
    f = lambda t: t.to(F32)
    y32 = B64.actnorm_invconv_fwd(f(to_rows(I["x"])), f(lg), f(bs), f(I["W"]), f(I["mask"]))[0]
    assert rows64.check("twin y", y32, y, by).ok
    yq, Wi = q(y), q(scal[2:].reshape(4, 4).T)
    xq, bxq = B64.actnorm_invconv_rev(yq, lg, bs, Wi, I["mask"])
    assert rows64.check("twin x", B64.actnorm_invconv_rev(f(yq), f(lg), f(bs), f(Wi), f(I["mask"]))[0], xq, bxq).ok


def test_actnorm_invconv_backward_equals_autograd_and_sees_its_planted_defects():
    I = setup(2)
    leaves = {k: I[k].clone().requires_grad_(True) for k in ("x", "logs", "bias", "W")}
    P = {"a.logs": leaves["logs"], "a.bias": leaves["bias"], "i.weight": leaves["W"]}
    z1, ld1 = R.actnorm_fwd(P, "a.", leaves["x"], I["mask3"])
    z, ld2 = R.invconv_fwd(P, "i.", z1, I["mask3"])
    ((z * I["rz"]).sum() + ((ld1 + ld2) * I["rl"]).sum()).backward()
    lg, bs = I["logs"].reshape(-1), I["bias"].reshape(-1)
    args = (to_rows(I["x"]), to_rows(I["rz"]), lg, bs, I["W"], torch.linalg.inv(I["W"]).T, I["mask"], I["rl"], I["lens"])
    got = B64.actnorm_invconv_bwd(*args)
    want = {"dx": to_rows(leaves["x"].grad), "d_an_logs": leaves["logs"].grad.reshape(-1), "d_an_bias": leaves["bias"].grad.reshape(-1),
            "d_w_ic": leaves["W"].grad.reshape(-1)}
    for k, w in want.items():
        assert close(got[k][0], w, EQ_GRAD), k
    valid = int(torch.nonzero(I["mask"])[3])
    for kw, key in ((dict(drop_row=valid), "d_an_bias"), (dict(use_inverse=True), "d_w_ic"), (dict(bookkeeping=False), "d_an_logs")):
        bad = B64.actnorm_invconv_bwd(*args, **kw)
        assert not close(bad[key][0], want[key], 1e-6), kw
    args = args[:5] + (q(args[5]),) + args[6:]                # the twin reads a float32 W^-T, as the kernels do (gt_flow_scalars)
    got = B64.actnorm_invconv_bwd(*args)
    twin = B64.actnorm_invconv_bwd(*[a.to(F32) for a in args])
    for k in want:
        assert rows64.check("twin " + k, twin[k][0], got[k][0], got[k][1]).ok, k


@pytest.mark.parametrize("sigmoid_scale", [False, True])
def test_coupling_equals_the_reference_and_autograd(sigmoid_scale, monkeypatch):
    I = setup(3 + sigmoid_scale)
    out = I["out"].clone().requires_grad_(True)
    x = I["x"].clone().requires_grad_(True)
    monkeypatch.setattr(R, "_coupling_net", lambda *a, **k: out)                 # the block's elementwise tail on a given [m | logs]
    z, ld = R.coupling_fwd({}, "c.", x, I["mask3"], sigmoid_scale=sigmoid_scale)
    ((z * I["rz"]).sum() + (ld * I["rl"]).sum()).backward()
    o, xr, mk = to_rows(I["out"]), to_rows(I["x"]), I["mask"]
    f = B64.coupling_fwd(o, xr, mk, I["rowutt"], I["B"], sigmoid_scale)
    assert close(f["z"][0], to_rows(z.detach()), EQ) and close(f["logdet"][0], ld.detach(), EQ)
    assert float(f["logdet"][0][LENS.index(0)]) == 0 and f["logdet"][2].tolist() == [80.0 * v for v in LENS]
    bad_utt = B64.credit_neighbour(I["rowutt"], mk)
    assert not close(B64.coupling_fwd(o, xr, mk, bad_utt, I["B"], sigmoid_scale)["logdet"][0], ld.detach(), 1e-6)
    b = B64.coupling_bwd(o[:, 80:], xr[:, 80:], to_rows(I["rz"]), I["rl"], mk, I["rowutt"], sigmoid_scale)
    assert close(b["dx"][0], to_rows(x.grad), EQ_GRAD)
    assert close(b["dout"][0], to_rows(out.grad), EQ_GRAD)
    if sigmoid_scale:
        nod = B64.coupling_bwd(o[:, 80:], xr[:, 80:], to_rows(I["rz"]), I["rl"], mk, I["rowutt"], True, scale_derivative=False)
        assert not close(nod["dout"][0], to_rows(out.grad), 1e-3)
    back = R.coupling_rev({}, "c.", z.detach(), I["mask3"], sigmoid_scale=sigmoid_scale)
    xv, bx = B64.coupling_rev(o, f["z"][0], mk, sigmoid_scale)
    assert close(xv, to_rows(back.detach()), EQ) and close(xv, xr, 2.0 ** -36)
    if not sigmoid_scale:                                                        # (with it the rule does not apply: module docstring)
        t = lambda a: a.to(F32)
        f32 = B64.coupling_fwd(t(o), t(xr), t(mk), I["rowutt"], I["B"], False)
        assert rows64.check("twin z", f32["z"][0], f["z"][0], f["z"][1]).ok
        ldb = rows64.gamma(f["logdet"][2] + 8) * f["logdet"][1]
        assert rows64.check("twin logdet", f32["logdet"][0], f["logdet"][0], ldb).ok
        b32 = B64.coupling_bwd(t(o[:, 80:]), t(xr[:, 80:]), t(to_rows(I["rz"])), t(I["rl"]), t(mk), I["rowutt"], False)
        for k in ("dx", "dout"):
            assert rows64.check("twin " + k, b32[k][0], b[k][0], b[k][1]).ok, k
        zq = q(f["z"][0])
        xq, bxq = B64.coupling_rev(o, zq, mk, False)
        assert rows64.check("twin x", B64.coupling_rev(t(o), t(zq), t(mk), False)[0], xq, bxq).ok


def test_input_bounds_are_carried_through():
    """an error planted in an input, as large as its stated bound, stays inside the output's bound"""
    I = setup(9)
    g = torch.Generator().manual_seed(1)
    o, xr, mk = to_rows(I["out"]), to_rows(I["x"]), I["mask"]
    e = torch.full_like(o, 1e-6)
    pert = o + e * torch.sign(torch.randn(o.shape, generator=g, dtype=F64))
    ref = B64.coupling_fwd(o, xr, mk, I["rowutt"], I["B"], False, e_out=e)["z"]
    assert rows64.check("z", B64.coupling_fwd(pert, xr, mk, I["rowutt"], I["B"])["z"][0], *ref).ok
    xv, bx = B64.coupling_rev(o, xr, mk, False, e_out=e)
    assert rows64.check("x", B64.coupling_rev(pert, xr, mk)[0], xv, bx).ok
    lg, bs = I["logs"].reshape(-1), I["bias"].reshape(-1)
    WinvT = torch.linalg.inv(I["W"]).T
    args = [xr, o, lg, bs, I["W"], WinvT, mk, I["rl"], I["lens"]]
    ref = B64.actnorm_invconv_bwd(*args, e_dy=e)
    got = B64.actnorm_invconv_bwd(*(args[:1] + [pert] + args[2:]))
    for k in ref:
        assert rows64.check(k, got[k][0], ref[k][0], ref[k][1]).ok, k
    y, by = B64.actnorm_invconv_rev(o, lg, bs, WinvT.T, mk, e_y=e)
    assert rows64.check("rev", B64.actnorm_invconv_rev(pert, lg, bs, WinvT.T, mk)[0], y, by).ok
    assert np.isfinite(float(by.max()))
