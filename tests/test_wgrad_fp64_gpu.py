"""The weight-gradient kernels (gt_conv_wgrad_bf16 + gt_weightnorm_bwd, gt_conv_wgrad_batched + gt_weightnorm_bwd_batched through
wgrad.WgradQueue) against float64 dW, dv, dg and dbias of their own bf16 operands, under the rule of oracle/rows64.py: elementwise
gamma_K * S (K = rows + slabs) carried through the weight-norm map, and a relative L2 error of at most 2e-5.  Every case runs on
enough rows for >= 2 slabs (asserted), and every check has a dropped-dY-row negative control that must miss by >= 3x."""
import pytest
import torch

from oracle import rows64

pytestmark = pytest.mark.gpu

# (Cin, Cout, taps, weight-normed): every tap count, the decoder's and encoder's channel counts, and counts that are no multiple of
# the 128 x gt_conv_wgrad_ci_tile(taps) tile (Cout 160 / 80, Cin 80 / 160 at k = 1 and 5)
CASES = [(192, 384, 5, True), (160, 80, 5, False), (80, 192, 1, True), (192, 160, 1, False), (384, 192, 1, True),
         (192, 768, 3, False), (768, 192, 3, True)]
LENS, T = [777, 640, 333, 2, 1, 100], 777


def dev():
    return torch.device("cuda:0")


def _operands(Cin, Cout, k, wn, seed):
    from glow_tts_amd import ops
    from glow_tts_amd.modules import ConvP, WNConvP
    g = torch.Generator().manual_seed(seed)
    ctx = ops.RowsCtx(torch.tensor(LENS, dtype=torch.int32, device=dev()), T, lengths_host=LENS)
    m = ctx.rowmask.unsqueeze(1)
    x = (torch.randn(ctx.R, Cin, generator=g).to(dev()) * m).to(torch.bfloat16)
    dy = (torch.randn(ctx.R, Cout, generator=g).to(dev()) * m).to(torch.bfloat16)
    torch.manual_seed(seed)
    conv = (WNConvP if wn else ConvP)(Cin, Cout, k).to(dev())
    conv.prepare()
    return ctx, x, dy, conv


def _set_prior(conv, seed):
    """accumulate = 1: the queue adds into the parameters' slices of a flat buffer that already holds these values"""
    params = [conv.weight_v, conv.weight_g, conv.bias] if conv.weight_norm else [conv.weight, conv.bias]
    n = sum(p.numel() for p in params)
    buf = torch.randn(n, generator=torch.Generator().manual_seed(seed)).to(dev())
    prior, off = {}, 0
    for key, p in zip(("v", "g", "b") if conv.weight_norm else ("v", "b"), params):
        p._gt_flat_grad = (buf, off)
        prior[key] = buf[off:off + p.numel()].clone().cpu()
        off += p.numel()
    return params, prior


@pytest.mark.parametrize("Cin,Cout,k,wn", CASES)
def test_wgrad_single_and_batched_vs_float64(built, Cin, Cout, k, wn):
    from glow_tts_amd import flow_impl, wgrad
    ctx, x, dy, conv = _operands(Cin, Cout, k, wn, seed=Cin + 3 * Cout + k)
    R = ctx.R
    tag = f"wgrad k={k} {Cin}->{Cout} {'wn' if wn else 'plain'}"
    # single-conv form
    S = wgrad.single_slabs(R, Cin, Cout, k)
    assert S >= 2, S
    g1 = flow_impl.conv_param_grads(conv, x, dy, R)
    torch.cuda.synchronize()
    rows64.check_conv_param_grads(f"{tag} single S={S}", conv, g1, x, dy, S)
    # batched form, dY in three column pieces
    with wgrad.WgradQueue(dev()) as q:
        c1, c2 = 32, Cout // 2 + 8
        g2 = flow_impl.conv_param_grads(conv, x, None, R, parts=[(dy[:, :c1], 0, c1), (dy[:, c1:c2], c1, c2 - c1),
                                                                   (dy[:, c2:], c2, Cout - c2)])
        (Sb, slab_rows), = q.slab_plan()
        assert Sb >= 2 and (Sb - 1) * slab_rows < R <= Sb * slab_rows, (Sb, slab_rows, R)
    torch.cuda.synchronize()
    rows64.check_conv_param_grads(f"{tag} batched S={Sb}", conv, g2, x, dy, Sb)
    # batched, accumulate = 1 into gradients that already hold values
    params, prior = _set_prior(conv, seed=k)
    try:
        with wgrad.WgradQueue(dev(), accumulate=True) as q:
            g3 = flow_impl.conv_param_grads(conv, x, dy, R)
            (Sa, _), = q.slab_plan()
        torch.cuda.synchronize()
        rows64.check_conv_param_grads(f"{tag} batched accumulate S={Sa}", conv, g3, x, dy, Sa, prior=prior)
    finally:
        for p in params:
            del p._gt_flat_grad


# the k = 1 shapes of CASES on fewer rows than the k = 1 ring holds (32-row stages, 3 deep): less than a stage, exactly one, two and a
# ragged third
SHORT_K1 = [c for c in CASES if c[2] == 1]
SHORT_R = [20, 32, 70]


@pytest.mark.parametrize("R", SHORT_R)
@pytest.mark.parametrize("Cin,Cout,k,wn", SHORT_K1)
def test_wgrad_k1_short_jobs_vs_float64(built, Cin, Cout, k, wn, R):
    """The k = 1 tile (3 channel groups, 32-row stages, 3-deep ring) on jobs shorter than its ring, through the single-conv form and
    through a WgradQueue, under the rule at one slab.  The queue plans one slab for each R, so 20 and 32 rows are one zero-filled stage
    and 70 rows two stages and a ragged third that is; the single-conv entry plans by ceil(R / 64) and cuts 70 rows into 64 + 6, which
    the one-slab bound (71 terms a sum, not 72) covers with room."""
    from glow_tts_amd import flow_impl, wgrad
    from glow_tts_amd.modules import ConvP, WNConvP
    torch.manual_seed(Cin + 3 * Cout + R)
    conv = (WNConvP if wn else ConvP)(Cin, Cout, k).to(dev())
    conv.prepare()
    g = torch.Generator().manual_seed(R + Cin)
    x = torch.randn(R, Cin, generator=g).to(dev()).to(torch.bfloat16)
    dy = torch.randn(R, Cout, generator=g).to(dev()).to(torch.bfloat16)
    tag = f"wgrad k=1 {Cin}->{Cout} {'wn' if wn else 'plain'} R={R}"
    assert wgrad.single_slabs(R, Cin, Cout, k) == (1 if R <= 64 else 2)
    g1 = flow_impl.conv_param_grads(conv, x, dy, R)
    torch.cuda.synchronize()
    rows64.check_conv_param_grads(f"{tag} single", conv, g1, x, dy, 1)
    with wgrad.WgradQueue(dev()) as q:
        g2 = flow_impl.conv_param_grads(conv, x, dy, R)
        assert q.slab_plan() == [(1, (R + 63) // 64 * 64)], q.slab_plan()
    torch.cuda.synchronize()
    rows64.check_conv_param_grads(f"{tag} batched", conv, g2, x, dy, 1)
