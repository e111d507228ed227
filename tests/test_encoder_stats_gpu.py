"""The P-free attention path (gt_attn_fwd_stats / gt_attn_bwd_stats behind encoder_impl.mha_fwd(keep_p="stats")) at module and model
level past 505 tokens: MultiHeadAttention(keep_p=False) against the float oracle with the tolerances of
tests/test_encoder_long_gpu.py::test_mha_fwd_bwd_long, the memory a two-layer Encoder no longer takes, one whole training step at 513
tokens x 1040 frames with RowsConfig.attn_keep_p = False (the body of test_train_step_on_a_long_text_vs_oracle, its tolerances; the
forward is the same bits as with the switch on), and Trainer(attn_keep_p=False) eager against captured."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "golden"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from fill import fill_module  # noqa: E402
from oracle import glowtts_ref as R  # noqa: E402
from oracle import mas as omas  # noqa: E402
from test_encoder_long_gpu import HP, cpu_state, dev, grad_ok, lens_mask, relerr  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("T", [506, 513])
def test_mha_without_saved_p(built, T):
    from glow_tts_amd import _lib, attentions
    assert _lib.lib().gt_attn_long_shape(T, 96, 4) == 1
    att = fill_module(attentions.MultiHeadAttention(192, 192, 2, window_size=4, p_dropout=0.1), "mha.").eval()
    P = cpu_state(att, "mha.")
    lens = [T, max(1, T - 2)]
    xm = lens_mask(lens, T)
    g = torch.Generator().manual_seed(T)
    x = torch.randn(2, 192, T, generator=g) * xm
    xx = x.clone().requires_grad_(True)
    am = xm.unsqueeze(2) * xm.unsqueeze(-1)
    o, _ = R.mha_fwd(P, "mha.", xx, xx, am)
    r = torch.randn(o.shape, generator=g) * xm
    (o * r).sum().backward()
    att = att.to(dev())
    with torch.no_grad():
        xk = x.to(dev())
        od_keep = att(xk, xk, am.to(dev()))
    assert att.attn is not None and att.attn.shape == (2, 2, T, T)
    att.keep_p = False
    xd = x.to(dev()).requires_grad_(True)
    od = att(xd, xd, am.to(dev()))
    assert att.attn is None
    assert torch.equal(od.detach(), od_keep)
    (od * r.to(dev())).sum().backward()
    assert relerr(xd.grad.cpu(), xx.grad) < 4e-2
    for name, prm in att.named_parameters():
        assert grad_ok(prm.grad.cpu(), P["mha." + name].grad, 6e-2, name=name), name


def test_mha_keep_p_false_changes_nothing_at_short_shapes(built):
    from glow_tts_amd import attentions
    T = 100
    att = fill_module(attentions.MultiHeadAttention(192, 192, 2, window_size=4, p_dropout=0.1), "mha.").eval().to(dev())
    xm = lens_mask([T, T - 3], T).to(dev())
    x = torch.randn(2, 192, T, generator=torch.Generator().manual_seed(1)).to(dev()) * xm
    am = xm.unsqueeze(2) * xm.unsqueeze(-1)
    res = []
    for keep in (True, False):
        att.keep_p = keep
        att.zero_grad()
        xd = x.clone().requires_grad_(True)
        o = att(xd, xd, am)
        assert att.attn is not None                      # not a key-tiled shape: P is kept whatever the switch says
        o.square().sum().backward()
        assert bool(torch.isfinite(xd.grad).all()) and bool(torch.isfinite(att.emb_rel_k.grad).all())
        res.append(o.detach())
    assert torch.equal(res[0], res[1])                   # (the backward's atomics make its sums order-dependent: not compared bit for bit)


def test_encoder_memory_without_saved_p(built):
    """Two layers, B = 1, T = 1025: peak(on) - peak(off) >= n_layers 4 B H T^2 — the two saved P tensors are gone, the backward's
    T^2 workspace shrinks on top of that.  The workspaces are grow-only process-wide scratch (flow_impl._scratch), so what an
    earlier test left there would decide what this one measures: each measured step starts without them and allocates its own.
    Measured on an MI355X with both workspaces left in place instead (P alone): 15 202 304 B against the bound's 16 810 000 — the
    peak moves from a point where both P are live to the first layer's FFN (1.6 MB of activations more, one P fewer)."""
    from glow_tts_amd import attentions, devstate, ops
    n_layers, B, T, Hh = 2, 1, 1025, 2
    enc = fill_module(attentions.Encoder(192, 768, Hh, n_layers, kernel_size=3, p_dropout=0.1, window_size=4), "enc.").eval().to(dev())
    enc.rows_cfg = ops.RowsConfig()
    xm = lens_mask([T], T).to(dev())
    x = torch.randn(B, 192, T, generator=torch.Generator().manual_seed(3)).to(dev()) * xm

    def step(keep):
        enc.rows_cfg.attn_keep_p = keep
        enc.zero_grad(set_to_none=True)
        xd = x.clone().requires_grad_(True)
        for name in ("attn_bwd", "attn_bwd_stats"):
            devstate.get(xd.device).scratch_bufs.pop(name, None)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        out = enc(xd, xm)
        out.square().sum().backward()
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated(), out.detach(), xd.grad

    step(True); step(False)                              # every other grow-only scratch exists before anything is measured
    on, o_on, g_on = step(True)
    off, o_off, g_off = step(False)
    print(f"encoder peak memory: saved P {on} B, row statistics {off} B, difference {on - off} B (bound {n_layers * 4 * B * Hh * T * T})")
    assert torch.equal(o_on, o_off)
    assert relerr(g_off, g_on) < 4e-2
    assert on - off >= n_layers * 4 * B * Hh * T * T


def _long_step(gen, ids, xl, y, yl, keep):
    from glow_tts_amd import models
    gen.zero_grad(set_to_none=True)
    gen.rows_cfg.ragged = True
    gen.rows_cfg.attn_keep_p = keep
    try:
        outs = gen(ids.to(dev()), xl.to(dev()), y.to(dev()), yl.to(dev()))
    finally:
        gen.rows_cfg.ragged = False
        gen.rows_cfg.attn_keep_p = True
    (z, z_m, z_logs, logdet, z_mask) = outs[0]
    l_mle = models.mle_loss(z, z_m, z_logs, logdet, z_mask)
    loss = l_mle + outs[2][1].sum()
    return outs, l_mle, loss


def test_train_step_on_a_long_text_without_saved_p(built):
    from glow_tts_amd import models
    Tx, Ty, xl, yl = 513, 1040, [513, 131], [1040, 402]
    gen = fill_module(models.FlowGenerator(148, 192, 768, 256, 80, use_sdp=False, kernel_size=3, n_heads=2, n_layers_enc=2, p_dropout=0.1,
                                           n_blocks_dec=2, kernel_size_dec=5, dilation_rate=1, n_block_layers=4,
                                           p_dropout_dec=0.05, n_sqz=2, window_size=4, mean_only=True, prenet=True), "").eval()
    P = cpu_state(gen)
    g = torch.Generator().manual_seed(7)
    B = 2
    ids = torch.randint(1, 148, (B, Tx), generator=g); xl = torch.tensor(xl)
    yl = torch.tensor(yl)
    y = torch.randn(B, 80, Ty, generator=g) * lens_mask(yl.tolist(), Ty)
    ids = ids * (torch.arange(Tx)[None, :] < xl[:, None])

    gen = gen.to(dev())
    outs_on, l_mle_on, loss_on = _long_step(gen, ids, xl, y, yl, True)
    z_on, zm_on, loss_on = outs_on[0][0].detach().clone(), outs_on[0][1].detach().clone(), loss_on.detach().clone()
    del outs_on, l_mle_on
    outs, l_mle, loss = _long_step(gen, ids, xl, y, yl, False)
    (z, z_m, z_logs, logdet, z_mask), (x_m, x_logs, x_mask), (attn, l_length, _, _), _, _ = outs
    assert torch.equal(z, z_on) and torch.equal(z_m, zm_on) and torch.equal(loss.detach(), loss_on)      # the same forward, bit for bit
    loss.backward()

    amask = (x_mask.unsqueeze(-1) * z_mask.unsqueeze(2)).squeeze(1)
    p = omas.oracle_maximum_path(gen.last_logp.cpu().numpy(), amask.cpu().numpy())
    assert np.array_equal(attn.squeeze(1).cpu().numpy().astype(np.int32), p)

    out = R.train_forward(P, ids, xl, y, yl, lambda logp, mask: attn.squeeze(1).cpu().float(), HP)
    out["loss"].backward()
    assert relerr(gen.last_logp.cpu(), out["logp"]) < 3e-2
    assert relerr(z.detach().cpu(), out["z"].detach()) < 3e-2
    assert relerr(z_m.detach().cpu(), out["z_m"].detach()) < 3e-2
    assert abs(l_mle.item() - out["l_mle"].item()) < 2e-2 * max(1.0, abs(out["l_mle"].item()))
    assert relerr(l_length.detach().cpu(), out["l_length"].detach()) < 5e-2
    worst, bad = [], []
    for name, prm in gen.named_parameters():
        ref = P[name].grad
        if ref is None:
            assert prm.grad is None or prm.grad.abs().max().item() == 0, name
            continue
        assert prm.grad is not None, name
        e = relerr(prm.grad.cpu(), ref)
        worst.append((e, name))
        tol = 0.15 if ".pre.conv_layers." in name else (0.2 if "emb_rel_" in name else 0.1)     # test_train_step_on_a_long_text_vs_oracle's
        if not grad_ok(prm.grad.cpu(), ref, tol, name=name):
            bad.append((name, round(e, 3)))
    worst.sort(reverse=True)
    print("worst grad errors:", worst[:5])
    assert not bad, bad


def test_trainer_without_saved_p_graph_matches_eager(built):
    """Trainer(attn_keep_p=False) on one 513-token batch, four steps: the captured step's losses follow the eager trainer's with the
    tolerance of tests/test_train_gpu.py::test_graph_step_matches_eager_step."""
    from glow_tts_amd import train
    cfg = dict(train.BASE_MODEL, n_blocks_dec=2, n_layers_enc=2, p_dropout=0.0, p_dropout_dec=0.0)
    torch.manual_seed(0)
    m1 = train.build_model(cfg, device=dev())
    with torch.no_grad():
        for n, p in m1.named_parameters():
            if n.endswith("end.weight") or n.endswith("pre.proj.weight"):
                p.normal_(0, 0.02)
    m1.encoder.pre.p_dropout = 0.0
    m2 = train.build_model(cfg, device=dev())
    m2.load_state_dict(m1.state_dict())
    m2.encoder.pre.p_dropout = 0.0
    batch = train.synth_batch(2, 513, 1040, 0, dev())
    t1 = train.Trainer(m1, graph=False, attn_keep_p=False)
    t2 = train.Trainer(m2, graph=True, capture_after=2, attn_keep_p=False)
    assert m1.rows_cfg.attn_keep_p is False and m2.rows_cfg.attn_keep_p is False and m2.encoder.rows_cfg is m2.rows_cfg
    le, lg = [], []
    for _ in range(4):
        le.append(t1.step(*batch)[0].detach().clone())
        lg.append(t2.step(*batch)[0].detach().clone())       # a replay returns the graph's static loss tensor: copy it per step
    torch.cuda.synchronize()
    assert t2.n_captures == 1 and t2.n_replays >= 1 and t2.adam_steps == t1.adam_steps == 4
    for a, b in zip(le, lg):
        assert torch.isfinite(a).all() and abs(a.item() - b.item()) <= 2e-2 * max(1.0, abs(a.item())), (a.item(), b.item())
    worst = max((a - b).abs().max().item() for a, b in zip(m1.parameters(), m2.parameters()))
    assert worst < 5e-3, worst
