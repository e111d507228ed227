"""GPU parity past 505 tokens (the key-tiled attention kernels of csrc/attn_long.hip) against the float oracle
(oracle/glowtts_ref.py): MultiHeadAttention forward + backward exactly as tests/test_encoder_gpu.py::test_mha_fwd_bwd does it, and
one whole training step on a text of 513 tokens (TextEncoder -> decoder -> logp -> MAS -> losses, forward and backward; the body of
test_train_forward_backward_vs_oracle).  That step runs gt_mas_long_f32: more than 512 tokens.

Tolerances are the existing ones for the bf16 attention path: output 3e-2, P 2e-2, input gradient 4e-2, parameter gradients
grad_ok(6e-2); whole step 0.1 (prenet 0.15, emb_rel_* 0.2).  The whole step uses the 2-encoder-layer, 2-block generator."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "golden"))
from fill import fill_module  # noqa: E402
from oracle import glowtts_ref as R  # noqa: E402
from oracle import mas as omas  # noqa: E402

pytestmark = pytest.mark.gpu

HP = dict(hidden_channels=192, n_layers_enc=2, n_heads=2, window_size=4, kernel_size=3, prenet=True, mean_only=True,
          n_blocks_dec=2, n_block_layers=4, kernel_size_dec=5, n_sqz=2)


def dev():
    return torch.device("cuda:0")


def relerr(a, b):
    return (a - b).abs().max().item() / max(1e-6, b.abs().max().item())


def grad_ok(a, b, tol, atol=2e-3, name=""):
    """Gradient agreement in relative L2 norm plus a loose max-abs bound (tests/test_encoder_gpu.py: grad_ok); the key bias of a
    softmax attention has a mathematically zero gradient: both sides hold rounding noise only."""
    if name.endswith("conv_k.bias"):
        return a.abs().max().item() < 5e-2 and b.abs().max().item() < 1e-4
    l2 = (a - b).norm().item() / max(1e-12, b.norm().item())
    mx = (a - b).abs().max().item()
    return l2 <= tol and mx <= 0.5 * b.abs().max().item() + atol


def lens_mask(lengths, T):
    l = torch.tensor(lengths)
    return (torch.arange(T)[None, :] < l[:, None]).unsqueeze(1).float()


def cpu_state(mod, prefix=""):
    P = {prefix + k: v.detach().cpu().float().clone() for k, v in mod.state_dict().items()}
    for v in P.values():
        v.requires_grad_(True)
    return P


@pytest.mark.parametrize("T", [506, 513])
def test_mha_fwd_bwd_long(built, T):
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
    o, p = R.mha_fwd(P, "mha.", xx, xx, am)
    r = torch.randn(o.shape, generator=g) * xm
    (o * r).sum().backward()
    att = att.to(dev())
    xd = x.to(dev()).requires_grad_(True)
    od = att(xd, xd, am.to(dev()))
    valid = xm.bool().expand_as(o)
    assert relerr(od.detach().cpu()[valid], o.detach()[valid]) < 3e-2
    pv = (xm.unsqueeze(-1) * xm.unsqueeze(2)).bool().expand_as(p)
    assert (att.attn.cpu()[pv] - p.detach()[pv]).abs().max() < 2e-2
    (od * r.to(dev())).sum().backward()
    assert relerr(xd.grad.cpu(), xx.grad) < 4e-2
    for name, prm in att.named_parameters():
        assert grad_ok(prm.grad.cpu(), P["mha." + name].grad, 6e-2, name=name), name


def test_train_step_on_a_long_text_vs_oracle(built):
    """Tx = 513 tokens, Ty = 1040 frames, ragged rows, no speaker: the alignment is compared on the HIP path's own lattice
    (bit-exact; gt_mas_long_f32), then injected into the oracle so that the remaining quantities are comparable."""
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
    gen.rows_cfg.ragged = True
    try:
        (z, z_m, z_logs, logdet, z_mask), (x_m, x_logs, x_mask), (attn, l_length, _, _), _, _ = \
            gen(ids.to(dev()), xl.to(dev()), y.to(dev()), yl.to(dev()))
    finally:
        gen.rows_cfg.ragged = False
    l_mle = models.mle_loss(z, z_m, z_logs, logdet, z_mask)
    loss = l_mle + l_length.sum()
    loss.backward()

    # alignment: bit-exact on the HIP lattice
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
        # the tolerances of test_train_forward_backward_vs_oracle: prenet convs under three conv -> LayerNorm -> ReLU stages (bf16
        # ReLU flips compound), emb_rel_* sums of signed band entries (heavy cancellation), everything else below 0.1
        tol = 0.15 if ".pre.conv_layers." in name else (0.2 if "emb_rel_" in name else 0.1)
        if not grad_ok(prm.grad.cpu(), ref, tol, name=name):
            bad.append((name, round(e, 3)))
    worst.sort(reverse=True)
    print("worst grad errors:", worst[:5])
    assert not bad, bad
