"""The stochastic predictors with the fused DDSConv layer kernels switched on (DilatedDepthSeparableConv.set_fused /
FlowGenerator.set_fused_predictors; csrc/dds_layer.hip): the module-level cases of tests/test_predictors_gpu.py restated with the same
inputs, the same oracles (oracle/glowtts_ref.py, tests/golden/float_golden/) and the same tolerances — activations 2e-2 of max-abs,
input gradients 3e-2, nll 1e-2 relative, parameter gradients 8e-2 of max-abs —, the cfg-5 trainer eager and captured, and the launches
a module makes on either side of the switch."""
import collections
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "golden"))
from fill import fill_module  # noqa: E402
import shards  # noqa: E402
from oracle import glowtts_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
G = shards.load(os.path.join(os.path.dirname(__file__), "golden", "float_golden"))


def t(name):
    return torch.from_numpy(G[name])


def dev():
    return torch.device("cuda:0")


def relerr(a, b):
    return (a - b).abs().max().item() / max(1e-6, b.abs().max().item())


def cpu_state(mod, prefix=""):
    return {prefix + k: v.detach().cpu().float().clone() for k, v in mod.state_dict().items()}


def lens_mask(lengths, T):
    l = torch.tensor(lengths)
    return (torch.arange(T)[None, :] < l[:, None]).unsqueeze(1).float()


def fuse(mod):
    """switch every DDSConv of `mod` to the fused kernels; returns mod"""
    from glow_tts_amd import predictors
    n = 0
    for m in mod.modules():
        if isinstance(m, predictors.DilatedDepthSeparableConv):
            assert m.fused is False                                # the default
            assert m.set_fused(True) is True
            n += 1
    assert n > 0
    return mod


def _check_param_grads(mod, P, prefix, tol=8e-2):
    worst = ("", 0.0)
    n = 0
    for name, p in mod.named_parameters():
        ref = P[prefix + name].grad
        if ref is None:
            continue
        assert p.grad is not None, name
        if ref.abs().max().item() < 1e-7:
            assert p.grad.abs().max().item() < 1e-4, name
            continue
        e = relerr(p.grad.cpu(), ref)
        n += 1
        if e > worst[1]:
            worst = (name, e)
        assert e < tol, (name, e)
    assert n > 0
    return worst


def test_fused_dds_conv_module_fwd_bwd(built):
    """test_dds_conv_module_fwd_bwd with the switch on: output, input / cond gradients, every parameter gradient"""
    from glow_tts_amd import predictors
    dds = fill_module(predictors.DilatedDepthSeparableConv(192, 3, 3, 0.5), "dds.").eval()
    P = {k: v.requires_grad_(True) for k, v in cpu_state(dds, "dds.").items()}
    x, g, m = t("dds_x").clone().requires_grad_(True), t("dds_g").clone().requires_grad_(True), t("f1_mask")
    o = R.dds_conv(P, "dds.", x, m, g=g)
    r = torch.randn(o.shape, generator=torch.Generator().manual_seed(3)) * m
    (o * r).sum().backward()
    dds = fuse(dds.to(dev()))
    xd, gd = x.detach().to(dev()).requires_grad_(True), g.detach().to(dev()).requires_grad_(True)
    od = dds(xd, m.to(dev()), g=gd)
    assert relerr(od.detach().cpu(), t("dds_out")) < 2e-2 and relerr(od.detach().cpu(), o.detach()) < 2e-2
    (od * r.to(dev())).sum().backward()
    vm = m.bool().expand_as(x)
    assert relerr(xd.grad.cpu()[vm], x.grad[vm]) < 3e-2 and relerr(gd.grad.cpu()[vm], g.grad[vm]) < 3e-2
    _check_param_grads(dds, P, "dds.")


@pytest.mark.parametrize("which", ["sdp", "spp", "sep"])
def test_fused_stochastic_predictor_nll_and_grads(built, which):
    """test_stochastic_predictor_nll_and_grads with the switch on: nll per utterance (vs the reference's value in the golden and vs
    the oracle) and every parameter gradient"""
    from glow_tts_amd import predictors
    if which == "sdp":
        mod = fill_module(predictors.StochasticDurationPredictor(192, 192, 3, 0.5, 4, gin_channels=512, lin_channels=4), "sdp.").eval()
        x, m, dr, nz = t("p5_x"), t("f1_mask"), t("p5_w"), t("p5_ew")
        kw = dict(g=t("p5_g"), l=t("p5_l"))
    else:
        cls = predictors.StochasticPitchPredictor if which == "spp" else predictors.StochasticEnergyPredictor
        mod = fill_module(cls(192, 256, 3, 0.1, 4, gin_channels=512), which + ".").eval()
        x, m, nz = t("p5_xf"), t("p5_fmask"), t("p5_ep")
        dr = t("p5_pitch") if which == "spp" else t("p5_pitch").abs()
        kw = dict(g=t("p5_g"))
    P = {k: v.requires_grad_(True) for k, v in cpu_state(mod, which + ".").items()}
    nll = R.sdp_fwd(P, "sdp.", x, m, dr, nz, **kw) if which == "sdp" else R.spp_fwd(P, which + ".", x, m, dr, nz, **kw)
    w = torch.tensor([1.0, -0.7])
    (nll * w).sum().backward()
    mod = fuse(mod.to(dev()))
    out = mod(x.to(dev()), m.to(dev()), dr.to(dev()), noise=nz.to(dev()), **{k: v.to(dev()) for k, v in kw.items()})
    want = t(which + "_nll")
    assert relerr(out.detach().cpu(), want) < 1e-2, (out, want)
    assert relerr(out.detach().cpu(), nll.detach()) < 1e-2
    (out * w.to(dev())).sum().backward()
    worst = _check_param_grads(mod, P, which + ".")
    print(which, "fused: worst parameter-gradient error", worst)


def test_fused_stochastic_predictors_reverse(built):
    """test_stochastic_predictors_reverse with the switch on (the sampling direction reaches dds_fwd through _cond_fwd and _cf_rev)"""
    from glow_tts_amd import predictors
    sdp = fuse(fill_module(predictors.StochasticDurationPredictor(192, 192, 3, 0.5, 4, gin_channels=512, lin_channels=4), "sdp.").eval().to(dev()))
    out = sdp(t("p5_x").to(dev()), t("f1_mask").to(dev()), g=t("p5_g").to(dev()), l=t("p5_l").to(dev()), reverse=True, noise_scale=0.8,
              noise=t("p5_ew").to(dev()))
    m = t("f1_mask").bool()
    assert relerr(out.cpu()[m], t("sdp_rev")[m]) < 3e-2
    spp = fuse(fill_module(predictors.StochasticPitchPredictor(192, 256, 3, 0.1, 4, gin_channels=512), "spp.").eval().to(dev()))
    nz = torch.cat([t("p5_ep"), t("p5_ep").flip(2)], 1)
    out = spp(t("p5_xf").to(dev()), t("p5_fmask").to(dev()), g=t("p5_g").to(dev()), reverse=True, noise_scale=0.7, noise=nz.to(dev()))
    fm = t("p5_fmask").bool()
    assert relerr(out.cpu()[fm], t("spp_rev")[fm]) < 3e-2


CFG5 = dict(hidden_channels=192, filter_channels=768, filter_channels_dp=256, kernel_size=3, p_dropout=0.1, n_blocks_dec=12,
            n_layers_enc=10, n_heads=2, p_dropout_dec=0.05, dilation_rate=1, kernel_size_dec=5, n_block_layers=4, n_sqz=2,
            prenet=True, mean_only=True, hidden_channels_enc=192, hidden_channels_dec=192, window_size=4, gin_channels=512,
            use_sdp=True, use_spk_embeds=True, use_lang_embeds=True, use_emo_embeds=True, lin_channels=4, emoin_channels=1024,
            use_spp=True, use_sep=True)      # == configs/base_blank_emo_lang_pitch.json "model"


def _cfg5_inputs(B, Tx, Ty, seed):
    g = torch.Generator().manual_seed(seed)
    xl = torch.randint(max(2, Tx // 2), Tx + 1, (B,), generator=g); xl[0] = Tx
    yl = torch.maximum(torch.randint(Ty // 3, Ty // 2 + 1, (B,), generator=g) * 2, xl + xl % 2); yl[0] = Ty
    ids = torch.randint(1, 187, (B, Tx), generator=g) * (torch.arange(Tx)[None, :] < xl[:, None])
    ym = lens_mask(yl.tolist(), Ty)
    y = torch.randn(B, 80, Ty, generator=g) * ym
    graw = torch.randn(B, 512, generator=g)
    emo = torch.randint(0, 5, (B,), generator=g)
    cart = torch.rand(B, 3, generator=g) * torch.tensor([1.5, 3.1, 4.6]) + torch.tensor([0.0, 0.0, -1.55])
    pitch = ((80 + 200 * torch.rand(B, 1, Ty, generator=g)) * (torch.rand(B, 1, Ty, generator=g) > 0.3)) * ym
    energy = (1 + 10 * torch.rand(B, 1, Ty, generator=g)) * ym
    lid = torch.randint(0, 3, (B,), generator=g)
    return ids, xl, y, yl, graw, emo, cart, pitch, energy, lid


def test_fused_cfg5_trainer_eager_and_graph_steps(built):
    """test_cfg5_trainer_eager_and_graph_steps with FlowGenerator.set_fused_predictors on: the fused branch is capturable (no host
    synchronisation, torch.empty buffers only) and the captured steps reproduce the eager fused steps to that test's criterion —
    finite losses within 0.5 of each other (the noise is drawn inside the step), one Adam step per step(), every predictor /
    front-end parameter moves."""
    from glow_tts_amd import predictors, train
    cfg = dict(CFG5, n_blocks_dec=2, n_layers_enc=2, p_dropout=0.0, p_dropout_dec=0.0, n_lang=10)

    def make():
        torch.manual_seed(0)
        m = train.build_model(cfg, n_vocab=187, device=dev())
        fill_module(m, "")
        m.encoder.pre.p_dropout = 0.0
        m.encoder.proj_w.convs.dropout_p = m.encoder.proj_w.post_convs.dropout_p = 0.0
        m.proj_pitch.convs.dropout_p = m.proj_energy.convs.dropout_p = 0.0
        n = m.set_fused_predictors(True)
        assert n == sum(isinstance(x, predictors.DilatedDepthSeparableConv) for x in m.modules()) == 3 * 5 + 5
        assert all(x.fused for x in m.modules() if isinstance(x, predictors.DilatedDepthSeparableConv))
        return m
    m1, m2 = make(), make()
    before = {n: p.detach().clone() for n, p in m1.named_parameters()}
    ids, xl, y, yl, graw, emo, cart, pitch, energy, lid = _cfg5_inputs(4, 30, 80, seed=4)
    d = lambda v: v.to(dev())                                         # noqa: E731
    kw = dict(g=d(graw), emo=d(emo), emo_cartesian=d(cart), pitch=d(pitch), energy=d(energy), l=d(lid))
    t1, t2 = train.Trainer(m1, graph=False), train.Trainer(m2, graph=True)
    torch.manual_seed(5)
    for _ in range(2):
        l1, _ = t1.step(d(ids), d(xl), d(y), d(yl), lengths_host=(xl.tolist(), yl.tolist()), **kw)
    torch.manual_seed(5)
    for _ in range(2):
        l2, _ = t2.step(d(ids), d(xl), d(y), d(yl), lengths_host=(xl.tolist(), yl.tolist()), **kw)
    torch.cuda.synchronize()
    assert t2.graph_mode and t2.n_captures == 1 and t2.adam_steps == 2
    assert torch.isfinite(l1).item() and torch.isfinite(l2).item()
    assert abs(l1.item() - l2.item()) < 0.5 * max(1.0, abs(l1.item()))          # same model, same batch, different noise draws
    for mm in (m1, m2):
        moved = {n for n, p in mm.named_parameters() if (p.detach() - before[n]).abs().max().item() > 0}
        for key in ("emb_g.weight", "emo_proj.bias", "emosty_layer_norm.weight", "encoder.proj_w.flows.3.proj.weight",
                    "encoder.proj_w.post_flows.0.log_scale", "proj_pitch.flows.1.convs.norms_1.0.gamma", "proj_energy.pre.weight",
                    "decoder.flows.2.wn_pitch.in_layers.0.weight_v"):
            assert key in moved, key


class _Counting:
    """predictors.call with every entry's name counted"""

    def __init__(self, inner):
        self._inner, self.counts = inner, collections.Counter()

    def __getattr__(self, name):
        fn = getattr(self._inner, name)

        def entry(*a):
            self.counts[name] += 1
            return fn(*a)
        return entry


def test_launches_on_either_side_of_the_switch(built, monkeypatch):
    """off: no gt_dds_layer_* entry is called and the per-op kernels run as before; on: a 3-layer module makes 3 gt_dds_layer_fwd,
    3 gt_dds_layer_bwd and 3 gt_dds_dw_bwd calls and no gt_dds_sep_* / gt_dds_out_* call.  Both give the same output and gradients
    to the module test's tolerances."""
    from glow_tts_amd import predictors
    dds = fill_module(predictors.DilatedDepthSeparableConv(192, 3, 3, 0.5), "dds.").eval().to(dev())
    x, g, m = t("dds_x").to(dev()), t("dds_g").to(dev()), t("f1_mask").to(dev())
    r = (torch.randn(x.shape, generator=torch.Generator().manual_seed(3)) * t("f1_mask")).to(dev())
    cnt = _Counting(predictors.call)
    monkeypatch.setattr(predictors, "call", cnt)
    res = {}
    for on in (False, True):
        dds.set_fused(on)
        dds.zero_grad()
        cnt.counts.clear()
        xd = x.clone().requires_grad_(True)
        od = dds(xd, m, g=g)
        (od * r).sum().backward()
        torch.cuda.synchronize()
        c = dict(cnt.counts)
        layer = {k: v for k, v in c.items() if k.startswith("gt_dds_layer_") and k not in ("gt_dds_layer_partial_rows", "gt_dds_layer_tile_rows")}
        perop = {k: v for k, v in c.items() if k.startswith("gt_dds_sep_") or k.startswith("gt_dds_out_")}
        if on:
            assert layer == {"gt_dds_layer_fwd": 3, "gt_dds_layer_bwd": 3} and not perop, c
        else:
            assert not layer and "gt_dds_layer_partial_rows" not in c, c
            assert perop == {"gt_dds_sep_fwd": 3, "gt_dds_out_fwd": 3, "gt_dds_out_bwd": 3, "gt_dds_sep_bwd": 3}, c
        assert c["gt_dds_dw_bwd"] == 3, c
        res[on] = (od.detach(), xd.grad.clone(), {n: p.grad.clone() for n, p in dds.named_parameters()})
    assert relerr(res[True][0], res[False][0]) < 2e-2 and relerr(res[True][1], res[False][1]) < 3e-2
    for n in res[True][2]:
        assert relerr(res[True][2][n], res[False][2][n]) < 8e-2, n
