"""oracle/chain64.py (the float64 reference of tests/test_encoder_chain_fp64_gpu.py) pinned to oracle/glowtts_ref.py, and through it to
the goldens of the reference project (tests/test_float_oracle.py): in exact mode with float64 parameters it reproduces encoder_fwd,
conv_relu_norm_fwd, duration_predictor_fwd and text_encoder_fwd — outputs, every parameter gradient and every input gradient — to 1e-10
relative L2 (both sides are float64 sums of at most a few thousand terms: 1e-10 is an error, not rounding), with dropout off and on, at
the hyper-parameters and length lists of the GPU test, with and without speaker vector, language vector and proj_s.

conv_k.bias has a mathematically zero gradient (the softmax is invariant to a per-query constant): both sides hold rounding noise
there, compared on the scale of the layer's conv_q.bias gradient.

The modes: forced mode fed chain64's own exact activations equals exact mode to 1e-12; twin mode fed the same differs from exact mode
in every gradient tensor (every one has a rounding site upstream)."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "golden"))
from fill import closed_form  # noqa: E402
from oracle import chain64 as C64  # noqa: E402
from oracle import dropmask as D  # noqa: E402
from oracle import glowtts_ref as R  # noqa: E402

HID, FILT, HEADS, WIN, FILT_DP, KS, OUT, LIN, VOCAB = 192, 768, 2, 4, 256, 3, 80, 4, 11
WORD, STEP = 0x2545F491, 6
LENS_A, LENS_B = [13, 1, 2, 9], [70, 37, 1]
TOL = 1e-10


def _conv(P, name, co, ci, k):
    P[name + ".weight"], P[name + ".bias"] = (co, ci, k), (co,)


def layer_shapes(pre, n_layers):
    S = {}
    for i in range(n_layers):
        for c in "qkvo":
            _conv(S, f"{pre}attn_layers.{i}.conv_{c}", HID, HID, 1)
        S[f"{pre}attn_layers.{i}.emb_rel_k"] = S[f"{pre}attn_layers.{i}.emb_rel_v"] = (1, 2 * WIN + 1, HID // HEADS)
        _conv(S, f"{pre}ffn_layers.{i}.conv_1", FILT, HID, KS)
        _conv(S, f"{pre}ffn_layers.{i}.conv_2", HID, FILT, KS)
        for n in ("norm_layers_1", "norm_layers_2"):
            S[f"{pre}{n}.{i}.gamma"] = S[f"{pre}{n}.{i}.beta"] = (HID,)
    return S


def prenet_shapes(pre):
    S = {}
    for i in range(3):
        _conv(S, f"{pre}conv_layers.{i}", HID, HID, 5)
        S[f"{pre}norm_layers.{i}.gamma"] = S[f"{pre}norm_layers.{i}.beta"] = (HID,)
    _conv(S, pre + "proj", HID, HID, 1)
    return S


def duration_shapes(pre):
    S = {}
    _conv(S, pre + "conv_1", FILT_DP, HID, KS)
    _conv(S, pre + "conv_2", FILT_DP, FILT_DP, KS)
    _conv(S, pre + "proj", 1, FILT_DP, 1)
    for n in ("norm_1", "norm_2"):
        S[f"{pre}{n}.gamma"] = S[f"{pre}{n}.beta"] = (FILT_DP,)
    return S


def text_shapes(pre, n_layers, lin, proj_s):
    S = {pre + "emb.weight": (VOCAB, HID - lin)}
    S.update(prenet_shapes(pre + "pre."))
    S.update(layer_shapes(pre + "encoder.", n_layers))
    _conv(S, pre + "proj_m", OUT, HID, 1)
    if proj_s:
        _conv(S, pre + "proj_s", OUT, HID, 1)
    return S


def filled(shapes):
    return {k: closed_form(k, s, torch.float64) for k, s in shapes.items()}


def rel(a, b, den=None):
    den = float(b.norm()) if den is None else den
    return float((a - b).norm()) / max(den, 1e-300)


def inputs(lens, seed):
    g = torch.Generator().manual_seed(seed)
    B, T = len(lens), max(lens)
    mask = (torch.arange(T)[None, :] < torch.tensor(lens)[:, None]).double()[:, None, :]
    return g, B, T, mask


def compare(what, outs_c, outs_o, leaves_c, leaves_o):
    """outputs, then the gradient of every leaf, chain64 against the oracle"""
    bad = []
    for n in outs_c:
        e = rel(outs_c[n].detach(), outs_o[n].detach())
        if not e <= TOL:
            bad.append((what, n, e))
    for n, lc in leaves_c.items():
        lo = leaves_o[n]
        assert (lc.grad is None) == (lo.grad is None), (what, n)
        if lc.grad is None:
            continue
        den = None
        if n.endswith("conv_k.bias"):
            den = float(leaves_o[n.replace("conv_k", "conv_q")].grad.norm())
        e = rel(lc.grad, lo.grad, den)
        if not e <= TOL:
            bad.append((what, n, e))
    assert not bad, bad


def two(P, extra):
    """two independent sets of leaves of the same values: one per side"""
    a = C64.leaves({**P, **extra})
    b = C64.leaves({**P, **extra})
    return a, b


@pytest.mark.parametrize("lens", [LENS_A, LENS_B])
@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("cond", [False, True])
def test_encoder_exact(lens, p, cond):
    g, B, T, mask = inputs(lens, 1)
    n_layers = 3
    P = filled(layer_shapes("enc.", n_layers))
    P["enc.cond_g.weight"], P["enc.cond_g.bias"] = closed_form("enc.cond_g.weight", (HID, 16), torch.float64), closed_form("enc.cond_g.bias", (HID,), torch.float64)
    extra = {"x": torch.randn(B, HID, T, generator=g, dtype=torch.float64), "g": torch.randn(B, 16, 1, generator=g, dtype=torch.float64)}
    r = torch.randn(B, HID, T, generator=g, dtype=torch.float64)
    drop = None
    if p:
        rows = D.row_map(lens, T)
        drop = {k: v for i in range(n_layers) for k, v in D.encoder_layer_masks(8 * i, WORD, rows, i, B, T, HID, FILT, HEADS, p, pre="enc.").items()}
    Lc, Lo = two(P, extra)
    vec = F.linear(Lc["g"].squeeze(-1), Lc["enc.cond_g.weight"], Lc["enc.cond_g.bias"]) if cond else None
    oc = C64.encoder(Lc, "enc.", Lc["x"], mask, C64.Hooks(), vec, n_layers, drop)
    oo = R.encoder_fwd(Lo, "enc.", Lo["x"], mask, Lo["g"] if cond else None, n_layers, HEADS, WIN, KS, drop)
    (oc * r).sum().backward()
    (oo * r).sum().backward()
    compare("encoder", {"out": oc}, {"out": oo}, Lc, Lo)


@pytest.mark.parametrize("lens", [LENS_A, LENS_B])
@pytest.mark.parametrize("p", [0.0, 0.5])
def test_prenet_exact(lens, p):
    g, B, T, mask = inputs(lens, 2)
    P = filled(prenet_shapes("pre."))
    extra = {"x": torch.randn(B, HID, T, generator=g, dtype=torch.float64) * mask}
    r = torch.randn(B, HID, T, generator=g, dtype=torch.float64)
    drop = None
    if p:
        rows = D.row_map(lens, T)
        drop = {f"pre.relu_drop.1:{i}": D.channel_mask(77 + i, WORD, rows, HID, p) for i in range(3)}
    Lc, Lo = two(P, extra)
    oc = C64.prenet(Lc, "pre.", Lc["x"], Lc["x"], mask, C64.Hooks(), drop)
    oo = R.conv_relu_norm_fwd(Lo, "pre.", Lo["x"], mask, drop=drop)
    (oc * r).sum().backward()
    (oo * r).sum().backward()
    compare("prenet", {"out": oc}, {"out": oo}, Lc, Lo)


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("cond", [False, True])
def test_duration_exact(p, cond):
    lens = LENS_A
    g, B, T, mask = inputs(lens, 3)
    P = filled(duration_shapes("dp."))
    P["dp.cond.weight"], P["dp.cond.bias"] = closed_form("dp.cond.weight", (HID, 16, 1), torch.float64), closed_form("dp.cond.bias", (HID,), torch.float64)
    extra = {"g": torch.randn(B, 16, 1, generator=g, dtype=torch.float64)}
    x = torch.randn(B, HID, T, generator=g, dtype=torch.float64) * mask
    r = torch.randn(B, 1, T, generator=g, dtype=torch.float64)
    drop = D.duration_masks(99, WORD, D.row_map(lens, T), FILT_DP, p, pre="dp.") if p else None
    Lc, Lo = two(P, extra)
    vec = F.conv1d(Lc["g"], Lc["dp.cond.weight"], Lc["dp.cond.bias"]).squeeze(-1) if cond else None
    oc = C64.duration(Lc, "dp.", x, mask, C64.Hooks(), drop, vec)
    oo = R.duration_predictor_fwd(Lo, "dp.", x, mask, KS, Lo["g"] if cond else None, drop=drop)
    (oc * r).sum().backward()
    (oo * r).sum().backward()
    if cond:                                       # the oracle detaches g (models.py:587-589); the runner's dvec is d cond(g)
        assert Lo["g"].grad is None
        Lc["g"].grad = None
    compare("duration", {"logw": oc}, {"logw": oo}, Lc, Lo)


def text_case(full, p_on, seed=4):
    """(leaves, forward of chain64 given hooks, oracle forward, upstream gradients): plain (mean_only, 2 layers) or full (speaker +
    language vector, proj_s, 3 layers)"""
    lens = LENS_A
    g, B, T, mask = inputs(lens, seed)
    n_layers, lin = (3, LIN) if full else (2, 0)
    P = filled(text_shapes("encoder.", n_layers, lin, full))
    extra = {}
    if full:
        P["encoder.encoder.cond_g.weight"] = closed_form("encoder.encoder.cond_g.weight", (HID, 16), torch.float64)
        P["encoder.encoder.cond_g.bias"] = closed_form("encoder.encoder.cond_g.bias", (HID,), torch.float64)
        extra = {"g": torch.randn(B, 16, 1, generator=g, dtype=torch.float64), "l": torch.randn(B, lin, 1, generator=g, dtype=torch.float64)}
    ids = torch.randint(0, VOCAB, (B, T), generator=g)
    xl = torch.tensor(lens)
    ups = [torch.randn(B, c, T, generator=g, dtype=torch.float64) for c in (HID, OUT, OUT)]
    drop = D.text_encoder_masks(STEP, WORD, D.row_map(lens, T), B, T, n_layers, HID, FILT, HEADS, 0.1, True, 0.5) if p_on else None

    def chain(L, hk):
        vec = F.linear(L["g"].squeeze(-1), L["encoder.encoder.cond_g.weight"], L["encoder.encoder.cond_g.bias"]) if full else None
        lvec = L["l"].squeeze(-1) if full else None
        xo, xm, xs, _ = C64.text_encoder(L, "encoder.", ids, xl, hk, vec, lvec, HID, n_layers, True, not full, drop)
        return {"x": xo, "x_m": xm, **({"x_logs": xs} if full else {})}

    def oracle(L):
        x, xm, xs, _ = R.text_encoder_fwd(L, "encoder.", ids, xl, L["g"] if full else None, HID, n_layers, HEADS, WIN, KS, True, not full,
                                          L["l"] if full else None, drop)
        return {"x": x, "x_m": xm, **({"x_logs": xs} if full else {})}

    def loss(o):
        return sum((o[k] * u).sum() for k, u in zip(("x", "x_m", "x_logs"), ups) if k in o)

    return P, extra, chain, oracle, loss


@pytest.mark.parametrize("full", [False, True])
@pytest.mark.parametrize("p_on", [False, True])
def test_text_encoder_exact(full, p_on):
    P, extra, chain, oracle, loss = text_case(full, p_on)
    Lc, Lo = two(P, extra)
    oc, oo = chain(Lc, C64.Hooks()), oracle(Lo)
    loss(oc).backward()
    loss(oo).backward()
    compare("text encoder", oc, oo, Lc, Lo)


def _grads(L):
    return {n: t.grad.clone() for n, t in L.items() if t.grad is not None}


def test_modes_on_own_activations():
    """forced mode fed exact mode's own activations is exact mode (1e-12); twin mode fed the same differs in every gradient tensor"""
    P, extra, chain, _, loss = text_case(True, True)
    runs = {}
    hk0 = C64.Hooks()
    for mode in ("exact", "forced", "twin"):
        L = C64.leaves({**P, **extra})
        hk = hk0 if mode == "exact" else C64.Hooks(mode, hk0.seen)
        loss(chain(L, hk)).backward()
        runs[mode] = _grads(L)
        if mode != "exact":
            assert hk.used == set(hk0.seen)
        if mode == "twin":
            assert len(hk.stored) > 40, sorted(hk.stored)
    assert set(runs["exact"]) == set(runs["forced"]) == set(runs["twin"])
    for n, ge in runs["exact"].items():
        den = float(runs["exact"][n.replace("conv_k", "conv_q")].norm()) if n.endswith("conv_k.bias") else None
        assert rel(runs["forced"][n], ge, den) <= 1e-12, n
        assert not torch.equal(runs["twin"][n], ge), f"{n}: no rounding site upstream of this gradient?"
        if not n.endswith("conv_k.bias"):
            assert 1e-9 < rel(runs["twin"][n], ge) < 3e-2, (n, rel(runs["twin"][n], ge))


def test_modes_duration_and_defects_change_gradients():
    """the duration predictor's twin, and every planted defect of chain64 moves some gradient of the forced reference by > 1 %"""
    lens = LENS_A
    g, B, T, mask = inputs(lens, 5)
    P = filled(duration_shapes("dp."))
    x = torch.randn(B, HID, T, generator=g, dtype=torch.float64) * mask
    r = torch.randn(B, 1, T, generator=g, dtype=torch.float64)
    drop = D.duration_masks(99, WORD, D.row_map(lens, T), FILT_DP, 0.1, pre="dp.")
    vec0 = torch.randn(B, HID, generator=g, dtype=torch.float64)

    def run(hk):
        L = C64.leaves({**P, "vec": vec0})
        (C64.duration(L, "dp.", x, mask, hk, drop, L["vec"]) * r).sum().backward()
        return _grads(L)

    hk0 = C64.Hooks()
    ge = run(hk0)
    gf, gt, gd = run(C64.Hooks("forced", hk0.seen)), run(C64.Hooks("twin", hk0.seen)), run(C64.Hooks("forced", hk0.seen, ["relu_in_norm_2"]))
    for n in ge:
        assert rel(gf[n], ge[n]) <= 1e-12, n
        assert not torch.equal(gt[n], ge[n]), n
    assert max(rel(gd[n], ge[n]) for n in ge) > 1e-2

    Pt, extra, chain, _, loss = text_case(True, True)
    def trun(hk):
        L = C64.leaves({**Pt, **extra})
        loss(chain(L, hk)).backward()
        return _grads(L)
    hk0 = C64.Hooks()
    ge = trun(hk0)
    for d in ("dx1_lost", "proj_s_addend", "prenet_dxb", "dvec_late", "lvec_shift", {"proj_s_scale": 0.05}):
        gd = trun(C64.Hooks("forced", hk0.seen, d if isinstance(d, dict) else [d]))
        assert max(rel(gd[n], ge[n]) for n in ge if not n.endswith("conv_k.bias")) > 1e-2, d
