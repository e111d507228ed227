"""The paired weight-gradient launch (gt_conv_wgrad_paired through wgrad.WgradQueue: 512-thread workgroups that compute two tiles of a
(job, slab) from one staged copy of the rows they share) against float64 dv, dg and dbias / dw of its own bf16 operands, under the
rule of oracle/rows64.py with its dropped-dY-row negative control, and against the 4-wave form (wgrad.PAIRED = False) on identical
inputs, bit for bit: each accumulator sees the same fragments in the same ascending 16-row k-steps of the same slabs.

Shapes: an odd x odd tile grid (same-co pairs, a same-ci pair and a single), one pair, same-ci pairs only, channel counts that are no
multiple of the tile (clamped column chunks), and the encoder's k = 3 shapes.  Rows: less than one ring stage, exactly one, three
stages with a ragged end (all through the zero-filling edge path, fewer stages than the ring is deep), and a ragged batch cut into 2
and 3 forced slabs (LDS-DMA stages), with dY in three column pieces and with accumulation into non-zero gradients.  That batch has
1920 rows, which 2 and 3 slabs of 64-row multiples divide exactly, so every case also runs on its first 1893 rows: there the last slab
ends inside a stage."""
import pytest
import torch

from oracle import rows64

# (Cin, Cout, taps, weight-normed)
CASES = [(192, 384, 5, True), (128, 128, 5, False), (64, 256, 5, True), (80, 160, 5, True), (160, 80, 5, False),
         (192, 768, 3, False), (768, 192, 3, True)]
LENS, T = [777, 640, 333, 2, 1, 100], 777


def dev():
    return torch.device("cuda:0")


def _conv(Cin, Cout, k, wn, seed):
    from glow_tts_amd.modules import ConvP, WNConvP
    torch.manual_seed(seed)
    conv = (WNConvP if wn else ConvP)(Cin, Cout, k).to(dev())
    conv.prepare()
    return conv


def _rows(R, Cin, Cout, seed, mask=None):
    g = torch.Generator().manual_seed(seed)
    x, dy = torch.randn(R, Cin, generator=g).to(dev()), torch.randn(R, Cout, generator=g).to(dev())
    if mask is not None:
        x, dy = x * mask, dy * mask
    return x.to(torch.bfloat16), dy.to(torch.bfloat16)


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


def _flush(conv, x, dy, R, paired, slabs=0, pieces=False, prior_seed=None):
    """One queue flush of one conv -> ({param: grad}, slab count, names of the library entries called, prior)"""
    from glow_tts_amd import _lib, flow_impl, wgrad
    Cout = conv.pc.Cout
    saved = wgrad.PAIRED, wgrad.PAIR_MIN_WGS, wgrad.FORCE_SLABS
    wgrad.PAIRED, wgrad.PAIR_MIN_WGS, wgrad.FORCE_SLABS = paired, 0, slabs
    params, prior = _set_prior(conv, prior_seed) if prior_seed is not None else ([], None)
    try:
        with _lib.record_calls() as names:
            with wgrad.WgradQueue(dev(), accumulate=prior is not None) as q:
                if pieces:
                    c1, c2 = 32, Cout // 2 + 8
                    g = flow_impl.conv_param_grads(conv, x, None, R, parts=[(dy[:, :c1], 0, c1), (dy[:, c1:c2], c1, c2 - c1),
                                                                              (dy[:, c2:], c2, Cout - c2)])
                else:
                    g = flow_impl.conv_param_grads(conv, x, dy, R)
                (S, slab_rows), = q.slab_plan()
        torch.cuda.synchronize()
        g = {p: t.clone() for p, t in g.items()}
    finally:
        wgrad.PAIRED, wgrad.PAIR_MIN_WGS, wgrad.FORCE_SLABS = saved
        for p in params:
            del p._gt_flat_grad
    return g, S, slab_rows, list(names), prior


def _check(tag, conv, x, dy, R, **kw):
    g8, S, slab_rows, names8, prior = _flush(conv, x, dy, R, True, **kw)
    g4, S4, _, names4, _ = _flush(conv, x, dy, R, False, **kw)
    assert "gt_conv_wgrad_paired" in names8 and "gt_conv_wgrad_paired" not in names4 and S == S4, (names8, names4, S, S4)
    rows64.check_conv_param_grads(f"{tag} paired S={S}", conv, g8, x, dy, S, prior=prior)
    for p in g8:
        assert torch.equal(g8[p], g4[p]), f"{tag}: paired and 4-wave gradients differ ({tuple(p.shape)}, max |diff| {(g8[p] - g4[p]).abs().max().item():.3e})"
    return S, slab_rows


def test_pair_grid_covers_every_tile_once():
    from glow_tts_amd import wgrad
    for nco in range(1, 8):
        for nci in range(1, 14):
            tiles = []
            for co, ci, kind in wgrad.pair_grid(nco, nci):
                tiles.append((co, ci))
                if kind == 0 and ci + 1 < nci:
                    tiles.append((co, ci + 1))
                if kind == 1:
                    assert co + 1 < nco
                    tiles.append((co + 1, ci))
            assert sorted(tiles) == [(co, ci) for co in range(nco) for ci in range(nci)], (nco, nci)
            assert len(wgrad.pair_grid(nco, nci)) == (nco * nci + 1) // 2
    assert [k for _, _, k in wgrad.pair_grid(3, 3)] == [0, 0, 0, 1, 0]        # the decoder's 384 x 192: 5 workgroups per job


@pytest.mark.gpu
@pytest.mark.parametrize("R", [40, 64, 129])
@pytest.mark.parametrize("Cin,Cout,k,wn", CASES)
def test_paired_short_rows(built, Cin, Cout, k, wn, R):
    conv = _conv(Cin, Cout, k, wn, seed=Cin + 3 * Cout + k)
    x, dy = _rows(R, Cin, Cout, seed=R + Cin)
    S, _ = _check(f"wgrad k={k} {Cin}->{Cout} R={R}", conv, x, dy, R)
    assert S == 1


@pytest.mark.gpu
@pytest.mark.parametrize("trim", [0, 27])
@pytest.mark.parametrize("Cin,Cout,k,wn", CASES)
def test_paired_ragged_slabs_pieces_and_accumulate(built, Cin, Cout, k, wn, trim):
    from glow_tts_amd import ops
    ctx = ops.RowsCtx(torch.tensor(LENS, dtype=torch.int32, device=dev()), T, lengths_host=LENS)
    R = ctx.R - trim
    conv = _conv(Cin, Cout, k, wn, seed=Cin + 3 * Cout + k)
    x, dy = _rows(R, Cin, Cout, seed=Cin + Cout, mask=ctx.rowmask[:R].unsqueeze(1))
    tag = f"wgrad k={k} {Cin}->{Cout} {'wn' if wn else 'plain'}"
    # dY in three column pieces, 2 forced slabs
    S, slab_rows = _check(f"{tag} pieces", conv, x, dy, R, slabs=2, pieces=True)
    assert S == 2 and slab_rows < R <= 2 * slab_rows and (trim == 0 or (2 * slab_rows - R) % 64), (S, slab_rows, R)
    # accumulate = 1 into gradients that already hold values, 3 forced slabs
    S, slab_rows = _check(f"{tag} accumulate", conv, x, dy, R, slabs=3, prior_seed=k)
    assert S == 3 and 2 * slab_rows < R <= 3 * slab_rows and (trim == 0 or (3 * slab_rows - R) % 64), (S, slab_rows, R)
