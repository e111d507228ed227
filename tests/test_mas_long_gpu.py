"""GPU parity tests of the long-lattice MAS kernel (gt_mas_long_f32, csrc/mas_long.hip): lattices gt_mas_f32 refuses — more than
512 tokens, or direction bits past its LDS — against the oracle (oracle/mas_oracle.c, which follows the reference's core.pyx), and
against gt_mas_f32 itself and the reference's golden paths where both kernels run.  Bit-exact; the one tolerance is the fp32
segment sum of gt_prior_expand_bwd."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "golden"))
from oracle import mas as omas  # noqa: E402

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden", "mas_golden.npz")
KINDS = ["gauss", "ties", "big"]


def dev():
    return torch.device("cuda:0")


def values(rng, kind, shape):
    if kind == "gauss":
        v = rng.normal(-100, 5, size=shape)
    elif kind == "ties":
        v = rng.integers(-2, 2, size=shape)
    else:
        v = rng.normal(-3e8, 2e8, size=shape)             # sums cross max_neg_val = -1e9
    return v.astype(np.float32)


def mixed_lengths(T_x, T_y, B=4):
    """full size | t_x = 1 | t_x == t_y | a short utterance inside the long lattice"""
    if B == 1:
        return np.array([T_x], np.int32), np.array([T_y], np.int32)
    sq = min(T_x, T_y) - 3
    return np.array([T_x, 1, sq, 5], np.int32), np.array([T_y, T_y // 3, sq, T_y // 2], np.int32)


def oracle_paths(v, t_x, t_y):
    p = np.zeros(v.shape, dtype=np.int32)
    omas.oracle_maximum_path_c(p, np.ascontiguousarray(v).copy(), t_x.astype(np.int32), t_y.astype(np.int32))
    return p


def refused_by_lds_kernel(T_x, T_y):
    """gt_mas_f32's host-side rule (csrc/mas.hip): past it, the long kernel is what runs under allow_long=True"""
    from glow_tts_amd import _lib
    return T_x > 512 or _lib.lib().gt_mas_lds_bytes(T_x, T_y) > 160 * 1024


def long_paths(v, t_x, t_y, **kw):
    from glow_tts_amd import monotonic_align as ma
    assert refused_by_lds_kernel(v.shape[1], v.shape[2])
    kw.setdefault("validate", True)
    r = ma.maximum_path_lengths(torch.from_numpy(np.ascontiguousarray(v)).to(dev()), torch.from_numpy(t_x.astype(np.int32)).to(dev()),
                                torch.from_numpy(t_y.astype(np.int32)).to(dev()), allow_long=True, **kw)
    torch.cuda.synchronize()
    return r


def check_against_oracle(v, t_x, t_y, tag):
    want = oracle_paths(v, t_x, t_y)
    r = long_paths(v, t_x, t_y, out_dtype=torch.int32, want_durations=True, want_frame2token=True, keep_workspace=True)
    got = r.path.cpu().numpy()
    bad = [i for i in range(len(want)) if not np.array_equal(got[i], want[i])]
    assert not bad, (tag, "utterances", bad)
    assert np.array_equal(r.durations.cpu().numpy(), want.sum(2).astype(np.float32)), tag
    f2t = r.frame2token.cpu().numpy()
    st = r.workspace.cpu().numpy()
    for i in range(len(want)):
        assert np.array_equal(f2t[i, : t_y[i]], want[i].argmax(0)[: t_y[i]]), (tag, i)
        assert (f2t[i, t_y[i]:] == -1).all(), (tag, i)
        assert np.array_equal(np.diff(st[i]), want[i].sum(1)), (tag, i)      # [B, T_x+1] row start columns
    return r


# 513 x 600: first row of the ninth row block; 513 x 513: all-diagonal; 576 x 577 / 577 x 640: row-block edge, odd T_y (the
# register-staged fill); 1025 x 1100: third band of 512 rows; 640 x 2600: T_y far past one band's diagonal
PAST_512 = [(513, 600), (513, 513), (576, 577), (577, 640), (1025, 1100), (640, 2600)]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("T_x,T_y", PAST_512)
def test_past_512_tokens(built, T_x, T_y, kind):
    rng = np.random.default_rng(1000 * T_x + T_y + KINDS.index(kind))
    t_x, t_y = mixed_lengths(T_x, T_y)
    if T_x == T_y:
        assert t_x[0] == t_y[0] == T_x
    check_against_oracle(values(rng, kind, (4, T_x, T_y)), t_x, t_y, (T_x, T_y, kind))


@pytest.mark.parametrize("kind", KINDS)
def test_the_stated_minimum_limit(built, kind):
    rng = np.random.default_rng(2048 + KINDS.index(kind))
    t_x, t_y = mixed_lengths(2048, 2080, B=1)
    check_against_oracle(values(rng, kind, (1, 2048, 2080)), t_x, t_y, (2048, 2080, kind))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("T_x,T_y", [(384, 1304), (150, 4800)])
def test_lds_bound_below_512_tokens(built, T_x, T_y, kind):
    from glow_tts_amd import _lib
    assert T_x <= 512 and _lib.lib().gt_mas_lds_bytes(T_x, T_y) > 160 * 1024
    rng = np.random.default_rng(1000 * T_x + T_y + KINDS.index(kind))
    t_x, t_y = mixed_lengths(T_x, T_y)
    check_against_oracle(values(rng, kind, (4, T_x, T_y)), t_x, t_y, (T_x, T_y, kind))


# ---- the long entry called directly where gt_mas_f32 runs too -------------------------------------------------------------------
def raw_mas(entry, v, t_x, t_y):
    """`entry` ("gt_mas_f32" / "gt_mas_long_f32") through the raw C-ABI: int32 path, durations, frame2token, [B, T_x+1] starts"""
    from glow_tts_amd import _lib
    L = _lib.lib()
    B, T_x, T_y = v.shape
    vd = torch.from_numpy(np.ascontiguousarray(v)).to(dev())
    tx = torch.from_numpy(t_x.astype(np.int32)).to(dev()); ty = torch.from_numpy(t_y.astype(np.int32)).to(dev())
    path = torch.full((B, T_x, T_y), 7, dtype=torch.int32, device=dev())
    dur = torch.full((B, T_x), -7.0, dtype=torch.float32, device=dev())
    f2t = torch.full((B, T_y), 7, dtype=torch.int32, device=dev())
    nbytes = (L.gt_mas_workspace_bytes if entry == "gt_mas_f32" else L.gt_mas_long_workspace_bytes)(B, T_x, T_y)
    ws = torch.zeros(nbytes // 4, dtype=torch.int32, device=dev())
    rc = getattr(L, entry)(_lib.ptr(vd), None, _lib.ptr(tx), _lib.ptr(ty), _lib.ptr(path), _lib.GT_DT_I32, _lib.ptr(dur), _lib.ptr(f2t),
                           B, T_x, T_y, vd.stride(0), vd.stride(1), _lib.ptr(ws), nbytes, None, _lib.current_stream(dev()))
    assert rc == 0, (entry, rc)
    torch.cuda.synchronize()
    return path.cpu().numpy(), dur.cpu().numpy(), f2t.cpu().numpy(), ws[: B * (T_x + 1)].view(B, T_x + 1).cpu().numpy()


def test_same_answers_where_both_kernels_run(built):
    g = np.load(GOLD)
    assert len(g["values"]) == 48
    want = np.unpackbits(g["paths_packed"], axis=-1)[..., : g["values"].shape[-1]].astype(np.int32)
    cases = [(g["values"].astype(np.float32), g["t_x"].astype(np.int32), g["t_y"].astype(np.int32), want)]
    rng = np.random.default_rng(375872)
    t_x, t_y = mixed_lengths(375, 872)
    cases.append((values(rng, "gauss", (4, 375, 872)), t_x, t_y, None))
    for v, t_x, t_y, gold in cases:
        assert not refused_by_lds_kernel(v.shape[1], v.shape[2])
        lds = raw_mas("gt_mas_f32", v, t_x, t_y)
        lng = raw_mas("gt_mas_long_f32", v, t_x, t_y)
        gold = oracle_paths(v, t_x, t_y) if gold is None else gold
        bad = [i for i in range(len(gold)) if not np.array_equal(lng[0][i], gold[i])]
        assert not bad, bad
        for a, b, what in zip(lds, lng, ("path", "durations", "frame2token", "starts")):
            assert np.array_equal(a, b), what


# ---- contract -------------------------------------------------------------------------------------------------------------------
def test_mask_with_holes_is_multiplied_in(built):
    from glow_tts_amd import monotonic_align as ma
    rng = np.random.default_rng(8)
    b, T_x, T_y = 2, 513, 600
    assert refused_by_lds_kernel(T_x, T_y)
    mask = np.ones((b, T_x, T_y), dtype=np.float32)
    mask[1, 400:, :] = 0; mask[1, :, 500:] = 0               # lengths from the mask: 400 x 500
    mask[:, 3:9, 10:30] = 0; mask[:, 200:330, 250:410] = 0   # holes inside the rectangle
    value = rng.normal(-5, 3, size=(b, T_x, T_y)).astype(np.float32)
    want = omas.oracle_maximum_path(value, mask)
    v = torch.from_numpy(value).to(dev()); v0 = v.clone()
    got = ma.maximum_path(v, torch.from_numpy(mask).to(dev()), validate=True)
    assert got.dtype == v.dtype and got.shape == v.shape
    assert torch.equal(v, v0), "input mutated"
    assert np.array_equal(got.cpu().numpy().astype(np.int32), want)


def test_path_dtypes_empty_utterance_and_input_untouched(built):
    rng = np.random.default_rng(9)
    T_x, T_y = 513, 600
    v = values(rng, "gauss", (3, T_x, T_y))
    t_x = np.array([513, 0, 77], np.int32); t_y = np.array([600, 0, 300], np.int32)      # a zero-length utterance: all-zero path
    want = oracle_paths(v[[0, 2]], t_x[[0, 2]], t_y[[0, 2]])
    for dt in (torch.float32, torch.int32, torch.float16, torch.bfloat16, torch.uint8):
        r = long_paths(v, t_x, t_y, out_dtype=dt)
        assert r.path.dtype == dt
        got = r.path.float().cpu().numpy().astype(np.int32)
        assert np.array_equal(got[[0, 2]], want), dt
        assert got[1].sum() == 0, dt
    from glow_tts_amd import monotonic_align as ma
    vd = torch.from_numpy(v).to(dev()); v0 = vd.clone()
    ma.maximum_path_lengths(vd, torch.from_numpy(t_x).to(dev()), torch.from_numpy(t_y).to(dev()), allow_long=True)
    torch.cuda.synchronize()
    assert torch.equal(vd, v0), "input mutated"


def test_invalid_lengths_and_the_default_are_reported(built):
    from glow_tts_amd import monotonic_align as ma
    v = torch.randn(2, 513, 600, device=dev())
    assert refused_by_lds_kernel(513, 600)
    i32 = lambda *a: torch.tensor(a, dtype=torch.int32, device=dev())  # noqa: E731
    with pytest.raises(ValueError, match="t_x > t_y"):
        ma.maximum_path_lengths(v, i32(513, 300), i32(600, 200), validate=True, allow_long=True)
    with pytest.raises(ValueError, match="exceeds"):
        ma.maximum_path_lengths(v, i32(514, 8), i32(600, 16), validate=True, allow_long=True)
    with pytest.raises(RuntimeError, match="limits"):          # the default is gt_mas_f32 alone, as before
        ma.maximum_path_lengths(v, i32(513, 8), i32(600, 16))
    with pytest.raises(RuntimeError, match="limits"):
        ma.maximum_path_lengths(v, i32(513, 8), i32(600, 16), allow_long=False)
    with pytest.raises(RuntimeError, match="gt_mas_long_f32.*limits"):       # past the long entry's own limits
        ma.maximum_path_lengths(torch.zeros(1, 4097, 4100, device=dev()), i32(1), i32(1), allow_long=True)


def test_captured_on_a_side_stream(built):
    """the call is capturable (Trainer captures the step): no allocation outside the graph's pool, no host synchronisation"""
    from glow_tts_amd import monotonic_align as ma
    T_x, T_y = 513, 600
    assert refused_by_lds_kernel(T_x, T_y)
    rng = np.random.default_rng(10)
    t_x, t_y = mixed_lengths(T_x, T_y)
    lat = [values(rng, "gauss", (4, T_x, T_y)) for _ in range(2)]
    want = [oracle_paths(v, t_x, t_y) for v in lat]
    v = torch.zeros(4, T_x, T_y, device=dev())
    tx = torch.from_numpy(t_x).to(dev()); ty = torch.from_numpy(t_y).to(dev())
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ma.maximum_path_lengths(v, tx, ty, out_dtype=torch.int32, allow_long=True)          # first use outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        r = ma.maximum_path_lengths(v, tx, ty, out_dtype=torch.int32, want_durations=True, allow_long=True)
    for i in (0, 1):
        v.copy_(torch.from_numpy(lat[i]))
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(r.path.cpu().numpy(), want[i]), i
        assert np.array_equal(r.durations.cpu().numpy(), want[i].sum(2).astype(np.float32)), i


# ---- gt_prior_expand_bwd past 512 tokens ------------------------------------------------------------------------------------------
def _expand_bwd(dz, f2t, Tx):
    from glow_tts_amd import _lib
    B, C, Ty = dz.shape
    dx = torch.full((B, C, Tx), 7.0, dtype=torch.float32, device=dev())
    _lib.call.gt_prior_expand_bwd(dz, f2t, dx, B, C, Tx, Ty, _lib.current_stream(dev()))
    torch.cuda.synchronize()
    return dx.cpu().numpy()


@pytest.mark.parametrize("T_x,T_y", [(513, 700), (1025, 1100)])
def test_prior_expand_bwd_past_512_tokens(built, T_x, T_y):
    rng = np.random.default_rng(T_x)
    B, C = 2, 6
    t_x = np.array([T_x, T_x // 2], np.int32); t_y = np.array([T_y, T_y - 101], np.int32)
    r = long_paths(values(rng, "gauss", (B, T_x, T_y)), t_x, t_y, want_frame2token=True)
    f2t = r.frame2token.cpu().numpy()
    assert (f2t[0] >= 0).all() and f2t[0].max() == T_x - 1 and (f2t[1, t_y[1]:] == -1).all()
    dz = rng.normal(size=(B, C, T_y)).astype(np.float32)
    got = _expand_bwd(torch.from_numpy(dz).to(dev()), r.frame2token, T_x)
    want = np.zeros((B, C, T_x), np.float64)
    for b in range(B):
        ok = f2t[b] >= 0
        for c in range(C):
            np.add.at(want[b, c], f2t[b][ok], dz[b, c][ok].astype(np.float64))
    err = np.abs(got - want).max() / np.abs(want).max()
    print(f"gt_prior_expand_bwd {T_x}x{T_y}: max-abs error {err:.3e} of max-abs")
    assert err <= 1e-5


def test_prior_expand_bwd_long_form_equals_the_512_token_kernel(built):
    """(150, 800): the same frame -> token map with the token axis padded past 512 goes to the long form; its first 150 columns
    are the existing kernel's, bit for bit (the same segmented scan in the same order), the padding is zero"""
    from glow_tts_amd import monotonic_align as ma
    rng = np.random.default_rng(150800)
    B, C, T_x, T_y = 2, 6, 150, 800
    r = ma.maximum_path_lengths(torch.from_numpy(values(rng, "gauss", (B, T_x, T_y))).to(dev()),
                                torch.tensor([150, 61], dtype=torch.int32, device=dev()),
                                torch.tensor([800, 433], dtype=torch.int32, device=dev()), want_frame2token=True)
    dz = torch.from_numpy(rng.normal(size=(B, C, T_y)).astype(np.float32)).to(dev())
    short = _expand_bwd(dz, r.frame2token, T_x)
    padded = _expand_bwd(dz, r.frame2token, 600)
    assert np.array_equal(short.view(np.int32), padded[:, :, :T_x].view(np.int32))
    assert (padded[:, :, T_x:] == 0).all()


# ---- in the model ---------------------------------------------------------------------------------------------------------------
def test_training_step_on_a_long_utterance(built):
    """FlowGenerator.forward + backward at T_x = 384, T_y = 1304 (one 15-second utterance with blank tokens): the lattice
    gt_mas_f32 refuses for its LDS, every other stage of the step already ran at this shape"""
    from glow_tts_amd import models
    from oracle import glowtts_ref as R
    from test_encoder_gpu import HP, _make_generator, cpu_state, lens_mask
    B, Tx, Ty = 2, 384, 1304
    assert refused_by_lds_kernel(Tx, Ty)
    gen = _make_generator(2)
    P = cpu_state(gen)
    g = torch.Generator().manual_seed(384)
    xl, yl = torch.tensor([384, 200]), torch.tensor([1304, 700])
    ids = torch.randint(1, 148, (B, Tx), generator=g) * (torch.arange(Tx)[None, :] < xl[:, None])
    y = torch.randn(B, 80, Ty, generator=g) * lens_mask(yl.tolist(), Ty)
    gen = gen.to(dev())
    (z, z_m, z_logs, logdet, z_mask), (x_m, x_logs, x_mask), (attn, l_length, _, _), _, _ = \
        gen(ids.to(dev()), xl.to(dev()), y.to(dev()), yl.to(dev()))
    l_mle = models.mle_loss(z, z_m, z_logs, logdet, z_mask)
    (l_mle + l_length.sum()).backward()
    amask = (x_mask.unsqueeze(-1) * z_mask.unsqueeze(2)).squeeze(1)
    p = omas.oracle_maximum_path(gen.last_logp.cpu().numpy(), amask.cpu().numpy())
    a = attn.squeeze(1).cpu().numpy().astype(np.int32)
    assert np.array_equal(a, p)
    assert np.array_equal(a.sum((1, 2)), yl.numpy())          # durations sum to y_lengths
    out = R.train_forward(P, ids, xl, y, yl, lambda logp, mask: attn.squeeze(1).cpu().float(), HP)
    print(f"l_mle {l_mle.item():.6f} oracle {out['l_mle'].item():.6f}")
    assert abs(l_mle.item() - out["l_mle"].item()) < 2e-2 * max(1.0, abs(out["l_mle"].item()))
    for name, prm in gen.named_parameters():
        if prm.grad is not None:
            assert torch.isfinite(prm.grad).all(), name
    assert any(prm.grad is not None and prm.grad.abs().max().item() > 0 for _, prm in gen.named_parameters())
