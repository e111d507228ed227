"""CPU tests of oracle/attn64.py and oracle/ln64.py, the float64 restatements the encoder kernels' fp64 tests compare with:
  * against the oracle (oracle/glowtts_ref.py's band formulation, torch.nn.functional.layer_norm) and torch.autograd in float64;
  * an fp32 emulation with the MFMA path's roundings stands in for the kernel: it passes every rule of oracle/rows64.py, every
    planted defect misses by >= rows64.CONTROL_MISS, and an emulation with a defect of its own fails the check that belongs to it —
    the reference alone stays inside the caps, and the checks can see what they are for."""
import math
import types

import pytest
import torch
import torch.nn.functional as F

from oracle import attn64, dropmask, glowtts_ref as R, ln64, rows64

WIN = 4


# ============================================================================= attention: float64 against the oracle + autograd
def _oracle_attention(q, k, v, Ek, Ev, lens, H, mask):
    """R.mha_fwd's inner attention on given q, k, v [B, T, H D]: the 1x1 convs select q | k | v from one input and conv_o is the
    identity.  Returns (out [B, T, H D], dropped P [B, H, T, T])."""
    B, T, d = q.shape
    x = torch.cat([q, k, v], 2).transpose(1, 2)                         # [B, 3d, T]
    eye = torch.eye(d, dtype=torch.float64)
    z = torch.zeros(d, d, dtype=torch.float64)
    P = {"a.conv_q.weight": torch.cat([eye, z, z], 1)[:, :, None], "a.conv_k.weight": torch.cat([z, eye, z], 1)[:, :, None],
         "a.conv_v.weight": torch.cat([z, z, eye], 1)[:, :, None], "a.conv_o.weight": eye[:, :, None],
         "a.emb_rel_k": Ek[None], "a.emb_rel_v": Ev[None]}
    ok = torch.arange(T)[None, :] < torch.tensor(lens)[:, None]
    am = (ok[:, None, :, None] & ok[:, None, None, :])
    o, p = R.mha_fwd(P, "a.", x, x, am, n_heads=H, window_size=WIN, drop=None if mask is None else {"a.drop:0": mask})
    return o.transpose(1, 2), p


@pytest.mark.parametrize("p", [0.0, 0.5])
@pytest.mark.parametrize("T,lens", [(3, [3, 1]), (5, [1, 5, 4]), (37, [37, 1, 33])])
def test_float64_restatement_equals_the_oracle_and_autograd(T, lens, p):
    B, H, D = len(lens), 2, 8
    g = torch.Generator().manual_seed(T + int(10 * p))
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)   # noqa: E731
    ok = (torch.arange(T)[None, :] < torch.tensor(lens)[:, None]).double()[:, :, None]
    q, k, v = (rnd(B, T, H * D) * ok).requires_grad_(True), (rnd(B, T, H * D) * ok).requires_grad_(True), (rnd(B, T, H * D) * ok).requires_grad_(True)
    dO = rnd(B, T, H * D) * ok                                           # padded queries carry no upstream gradient
    Ek, Ev = rnd(2 * WIN + 1, D).requires_grad_(True), rnd(2 * WIN + 1, D).requires_grad_(True)
    keep = (torch.rand(B, H, T, T, generator=g) >= p) if p else None
    scale = 1.0 / (1.0 - p)
    want_o, want_p = _oracle_attention(q, k, v, Ek, Ev, lens, H, None if keep is None else keep.double() * scale)
    (want_o * dO).sum().backward()
    dEk, dEv = [], []
    for b in range(B):
        for h in range(H):
            sl = slice(h * D, (h + 1) * D)
            qq, kk, vv, dd = (x[b, :, sl].detach() for x in (q, k, v, dO))
            kp = None if keep is None else keep[b, h]
            s, S = attn64.scores(qq, kk, Ek.detach(), lens[b], T, WIN)
            assert bool((S >= 0).all()) and bool(((s.abs() <= S * (1 + 1e-12) + 1e-300) | (s == attn64.MASKED)).all())
            P, _ = attn64.softmax_rows(s, torch.zeros_like(s))
            Pd = attn64.drop(P, kp, scale)
            O, _ = attn64.out(Pd, vv, Ev.detach(), WIN)
            assert torch.allclose(Pd, want_p[b, h].detach(), rtol=0, atol=1e-12)
            assert torch.allclose(O, want_o[b, :, sl].detach(), rtol=0, atol=1e-12)
            dS, _ = attn64.ds(P, dd, vv, Ev.detach(), kp, scale, lens[b], 2 * D + 1, WIN)
            Pdb = attn64.pd_bwd(Pd, lens[b])
            for mine, want in ((attn64.dq(dS, kk, Ek.detach(), WIN)[0], q.grad), (attn64.dk(dS, qq)[0], k.grad), (attn64.dv(Pdb, dd)[0], v.grad)):
                assert torch.allclose(mine, want[b, :, sl], rtol=0, atol=1e-10)
            dEk.append(attn64.band_grad(dS, qq, WIN))
            dEv.append(attn64.band_grad(Pdb, dd, WIN))
    zero = torch.zeros(2 * WIN + 1, D)
    assert torch.allclose(attn64.accumulate(dEk, zero, 1)[0], Ek.grad, rtol=0, atol=1e-10)
    assert torch.allclose(attn64.accumulate(dEv, zero, 1)[0], Ev.grad, rtol=0, atol=1e-10)


# ============================================================================= attention: the fp32 emulation under the rule
def _bf(x):
    return x.to(torch.bfloat16).to(torch.float32)


def _case(T, lens, p, seed=0, H=2, D=96):
    """operands at the scales of the GPU test: q, k, v ~ 0.5 N(0,1) and dO ~ N(0,1) in bf16 (padded rows zero), Ek, Ev ~ 0.1 N(0,1)"""
    g = torch.Generator().manual_seed(1000 * T + seed)
    B = len(lens)
    ok = (torch.arange(T)[None, :] < torch.tensor(lens)[:, None]).float()[:, :, None, None]
    mk = lambda s: [[x for x in ub] for ub in (_bf(torch.randn(B, T, H, D, generator=g) * s) * ok).permute(0, 2, 1, 3).double()]   # noqa: E731
    c = types.SimpleNamespace(B=B, H=H, T=T, D=D, win=WIN, lens=lens, p=p, seed=dropmask.word_seed(0x9E3779B9, 77), own=[T] * B)
    c.q, c.k, c.v, c.dO = mk(0.5), mk(0.5), mk(0.5), mk(1.0)
    c.Ek, c.Ev = torch.randn(2 * WIN + 1, D, generator=g) * 0.1, torch.randn(2 * WIN + 1, D, generator=g) * 0.1
    c.prior_dEk, c.prior_dEv = torch.randn(2 * WIN + 1, D, generator=g), torch.randn(2 * WIN + 1, D, generator=g)
    return c


def _emulate(c, defect=None):
    """gt_attn_fwd + gt_attn_bwd of the MFMA path in torch float32: bf16 Ek / Ev, P' = bf16(fp32(P keep scale)), bf16 dS and P' from
    pass 1 into dQ, dK, dV, dEk, dEv.  defect: a bug of the emulation's own (the sensitivity test)."""
    T, D, win, f = c.T, c.D, c.win, torch.float32
    Ek, Ev = _bf(c.Ek), _bf(c.Ev)
    i = torch.arange(T)
    rel = i[None, :] - i[:, None] + win
    inb = (rel >= 0) & ((rel < 2 * win) if defect == "band edge" else (rel <= 2 * win))
    relc = rel.clamp(0, 2 * win)
    relk = (rel + ((i[None, :] % 32 == 0) if defect == "Ek[rel + 1] at a tile edge" else 0)).clamp(0, 2 * win)
    gather = lambda W, r=relc: torch.gather(W, 1, r) * inb               # noqa: E731
    scatter = lambda M: torch.zeros(T, 2 * win + 1).scatter_add_(1, relc, M * inb)   # noqa: E731
    isq = torch.tensor(1.0 / math.sqrt(D), dtype=f)
    sc = torch.tensor(float(dropmask.scale(c.p)) if c.p else 1.0, dtype=f)
    got = {n: torch.zeros(c.B, c.H, T, T if n in ("P", "dS", "Pd") else D) for n in ("P", "out", "dS", "Pd", "dq", "dk", "dv")}
    got["dEk"], got["dEv"] = c.prior_dEk.clone(), c.prior_dEv.clone()
    for b in range(c.B):
        ok = i < c.lens[b]
        ok2 = ok[:, None] & ok[None, :]
        for h in range(c.H):
            q, k, v, dO = (x[b][h].to(f) for x in (c.q, c.k, c.v, c.dO))
            keep = attn64.keep_mask(c.seed, b, h, c.H, T, c.p)
            ks = torch.ones(T, T) if keep is None else keep.to(f) * sc
            s = (q @ k.T + gather(q @ Ek.T, relk)) * isq
            s = torch.where(ok2, s, torch.full_like(s, -1e4))
            e = torch.exp(s - s.max(1, keepdim=True).values)
            P = e * (1.0 / e.sum(1, keepdim=True))
            Pd = _bf(P * ks)
            got["P"][b, h], got["out"][b, h] = P, _bf(Pd @ v + scatter(Pd) @ Ev)
            dP = (dO @ v.T + gather(dO @ Ev.T)) * ks
            Dsum = (dP * P).sum(1, keepdim=True)
            dS = _bf(P * (dP - Dsum) * isq * ok2)
            Pdb = Pd * ok[:, None]
            got["dS"][b, h], got["Pd"][b, h] = dS, Pdb
            dSk = dS.clone()
            if defect == "query 128 lost from dK":
                dSk[128] = 0
            got["dq"][b, h], got["dk"][b, h], got["dv"][b, h] = _bf(dS @ k + scatter(dS) @ Ek), _bf(dSk.T @ q), _bf(Pdb.T @ dO)
            got["dEk"] += scatter(dS).T @ q
            got["dEv"] += scatter(Pdb).T @ dO
    return got


_CASES = {}


def _shared(T, p):
    if (T, p) not in _CASES:
        _CASES[T, p] = _case(T, [T, 1, 33], p)
    return _CASES[T, p]


@pytest.mark.parametrize("T,p", [(37, 0.1), (37, 0.0), (300, 0.1)])
def test_fp32_emulation_passes_every_rule_and_every_control_misses(T, p):
    c = _shared(T, p)
    lines = []
    rep = attn64.check_case(f"emulation T={T} p={p}", c, _emulate(c), mfma=True, log=lines.append)
    print("\n".join(lines))
    assert set(rep) == {"P", "out", "dS", "Pd", "dq", "dk", "dv", "dEk", "dEv"} and all(r.ok for r in rep.values())
    assert len(lines) >= 16 and all("control misses by" in ln for ln in lines)


@pytest.mark.parametrize("defect,check", [("band edge", " P <"), ("Ek[rel + 1] at a tile edge", " P <"), ("query 128 lost from dK", " dk <")])
def test_a_defect_in_the_emulation_fails_its_check(defect, check):
    c = _shared(300, 0.1)
    with pytest.raises(AssertionError) as e:
        attn64.check_case("defective emulation", c, _emulate(c, defect), mfma=True, log=lambda s: None)
    assert check in str(e.value) and "planted defect" not in str(e.value), str(e.value)


def test_generic_path_operands_pass_too():
    """the generic path's restatement (fp32 Ek / Ev, fp32 P' and dS) on an fp32 emulation without the bf16 roundings"""
    c = _case(40, [33, 1, 40], 0.1, D=64)
    T, D, win, f = c.T, c.D, c.win, torch.float32
    i = torch.arange(T)
    rel = i[None, :] - i[:, None] + win
    inb, relc = (rel >= 0) & (rel <= 2 * win), rel.clamp(0, 2 * win)
    gather = lambda W: torch.gather(W, 1, relc) * inb                    # noqa: E731
    scatter = lambda M: torch.zeros(T, 2 * win + 1).scatter_add_(1, relc, M * inb)   # noqa: E731
    isq, sc = torch.tensor(1.0 / math.sqrt(D), dtype=f), torch.tensor(float(dropmask.scale(c.p)), dtype=f)
    got = {n: torch.zeros(c.B, c.H, T, T if n in ("P", "dS") else D) for n in ("P", "out", "dS", "dq", "dk", "dv")}
    got["Pd"], got["dEk"], got["dEv"] = None, c.prior_dEk.clone(), c.prior_dEv.clone()
    for b in range(c.B):
        ok = i < c.lens[b]
        ok2 = ok[:, None] & ok[None, :]
        for h in range(c.H):
            q, k, v, dO = (x[b][h].to(f) for x in (c.q, c.k, c.v, c.dO))
            ks = attn64.keep_mask(c.seed, b, h, c.H, T, c.p).to(f) * sc
            s = torch.where(ok2, (q @ k.T + gather(q @ c.Ek.T)) * isq, torch.tensor(-1e4))
            P = torch.softmax(s, 1)
            Pd = P * ks
            dP = (dO @ v.T + gather(dO @ c.Ev.T)) * ks
            dS = P * (dP - (dP * P).sum(1, keepdim=True)) * isq * ok2
            Pdb = Pd * ok[:, None]
            got["P"][b, h], got["out"][b, h], got["dS"][b, h] = P, _bf(Pd @ v + scatter(Pd) @ c.Ev), dS
            got["dq"][b, h], got["dk"][b, h], got["dv"][b, h] = _bf(dS @ k + scatter(dS) @ c.Ek), _bf(dS.T @ q), _bf(Pdb.T @ dO)
            got["dEk"] += scatter(dS).T @ q
            got["dEv"] += scatter(Pdb).T @ dO
    rep = attn64.check_case("generic emulation T=40 D=64", c, got, mfma=False)
    assert "Pd" not in rep and all(r.ok for r in rep.values())


# ============================================================================= LayerNorm
def _ln_emulate(c):
    """the kernels' operations in torch float32"""
    f = torch.float32
    R_, C = (c.a if c.a is not None else c.y).shape
    ki, si = ln64._keep(c.p_in, c.seed_in, R_, C)
    ko, so = ln64._keep(c.p_out, c.seed_out, R_, C)
    s = torch.zeros(R_, C) if c.a is None else c.a.clone()
    kin = torch.ones(R_, C, dtype=torch.bool)
    if c.y is not None:
        yy = c.y.float()
        if ki is not None:
            kin = torch.from_numpy(ki)
            yy = torch.where(kin, yy * torch.tensor(float(si), dtype=f), torch.zeros(()))
        s = s + yy
    if c.relu & 2:
        kin = kin & torch.from_numpy((rows64.bits(c.y) & 0x7fff) != 0)
    mean = s.sum(1, keepdim=True) / C
    rstd = torch.rsqrt(((s - mean) ** 2).sum(1, keepdim=True) / C + torch.tensor(c.eps, dtype=f))
    xh = (s - mean) * rstd
    n = xh * c.gamma + c.beta
    kso = torch.ones(R_, C) if ko is None else torch.from_numpy(ko).float() * torch.tensor(float(so), dtype=f)
    o = (torch.relu(n) if c.relu & 1 else n) * kso * c.rowmask[:, None]
    d = torch.zeros(R_, C)
    for t in (c.dout_f32, c.dout_bf16):
        if t is not None:
            d = d + t.float()
    d = d * c.rowmask[:, None] * kso
    if c.relu & 1:
        d = d * (n > 0)
    dn = d * c.gamma
    ds = rstd * (dn - dn.sum(1, keepdim=True) / C - xh * ((dn * xh).sum(1, keepdim=True) / C))
    dy = ds * kin * torch.tensor(float(si), dtype=f) if (c.p_in or c.relu & 2) else ds
    return {"mean": mean[:, 0], "rstd": rstd[:, 0], "out_f32": o, "out_bf16": o.to(torch.bfloat16), "da": ds, "dy": dy.to(torch.bfloat16),
            "dgamma": c.prior_gamma + (d * xh).sum(0), "dbeta": c.prior_beta + d.sum(0)}


@pytest.mark.parametrize("form", ["a", "y", "a+y", "relu1", "relu2"])
def test_layernorm_float64_equals_torch_and_autograd(form):
    c = ln64.make_case(23, 100, form)
    R_, C = 23, 100
    ki, si = ln64._keep(c.p_in, c.seed_in, R_, C)
    ko, so = ln64._keep(c.p_out, c.seed_out, R_, C)
    a = None if c.a is None else c.a.double().requires_grad_(True)
    y = None if c.y is None else c.y.double().requires_grad_(True)     # relu & 2: y = relu(pre); the gradient wrt pre is dy where y != 0
    s = 0 if a is None else a
    if y is not None:
        s = s + (y if ki is None else y * torch.from_numpy(ki) * float(si))
    gam, beta = c.gamma.double().requires_grad_(True), c.beta.double().requires_grad_(True)
    n = F.layer_norm(s, (C,), gam, beta, eps=c.eps)
    o = torch.relu(n) if c.relu & 1 else n
    if ko is not None:
        o = o * torch.from_numpy(ko) * float(so)
    o = o * c.rowmask.double()[:, None]
    f = ln64.forward(c.a, c.y, c.gamma, c.beta, c.rowmask, c.eps, ki, si, ko, so, c.relu & 1)
    assert torch.allclose(f["out"][0], o.detach(), rtol=0, atol=1e-12)
    assert torch.allclose(f["mean"][0], s.detach().mean(1), rtol=0, atol=1e-12)
    assert torch.allclose(f["rstd"][0], 1 / torch.sqrt(s.detach().var(1, unbiased=False) + c.eps), rtol=0, atol=1e-12)
    d = sum(t.double() for t in (c.dout_f32, c.dout_bf16) if t is not None)
    (o * d).sum().backward()
    g = ln64.backward(c.a, c.y, c.gamma, c.beta, c.rowmask, f["mean"][0], f["rstd"][0], c.dout_f32, c.dout_bf16, c.K_param, c.prior_gamma, c.prior_beta,
                      keep_in=ki, scale_in=si, keep_out=ko, scale_out=so, relu=c.relu, y_bits=None if c.y is None else rows64.bits(c.y))
    if a is not None:
        assert torch.allclose(g["da"][0], a.grad, rtol=0, atol=1e-10)
    if y is not None:
        want = y.grad * (y.detach() != 0) if c.relu & 2 else y.grad
        assert torch.allclose(g["dy"][0], want, rtol=0, atol=1e-10)
    assert torch.allclose(g["dgamma"][0], gam.grad + c.prior_gamma.double(), rtol=0, atol=1e-10)
    assert torch.allclose(g["dbeta"][0], beta.grad + c.prior_beta.double(), rtol=0, atol=1e-10)
    assert not g["ambiguous"].any()


@pytest.mark.parametrize("form", ["a", "y", "a+y", "relu1", "relu2"])
@pytest.mark.parametrize("R_,C", [(70, 100), (2085, 256)])
def test_layernorm_fp32_emulation_passes_and_controls_miss(R_, C, form):
    c = ln64.make_case(R_, C, form)
    got = _ln_emulate(c)
    if c.a is None:
        got["da"] = None
    if c.y is None:
        got["dy"] = None
    rep, share = ln64.check_case(f"LN emulation {form} R={R_} C={C}", c, got)
    assert all(r.ok for r in rep.values()) and share <= 1e-4


def test_layernorm_defective_emulation_fails():
    c = ln64.make_case(70, 100, "a+y")
    got = _ln_emulate(c)
    got["dy"] = (got["dy"].float() / float(dropmask.scale(c.p_in))).to(torch.bfloat16)      # p_in's scale forgotten
    with pytest.raises(AssertionError) as e:
        ln64.check_case("defective LN emulation", c, got, log=lambda s: None)
    assert " dy <" in str(e.value) and "planted defect" not in str(e.value)
