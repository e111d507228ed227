"""oracle/loss64.py (the float64 operators tests/test_loss_kernels_fp64_gpu.py and tests/test_row_layout_gpu.py hold the loss, lattice
and layout kernels to) pinned to oracle/glowtts_ref.py run in float64 — logp_lattice, mle_loss, the l_length lines of train_forward,
the prior expansion over generate_path maps, commons.squeeze / unsqueeze — and its backward operators pinned to autograd.  No GPU.

"Equal" for two float64 evaluations is 1e-12 of the tensor's largest magnitude.  The float32 twin of every operator (the same
formula in torch.float32 on the same data) must pass the rule at every shape the GPU test runs, and every planted defect of that
test must miss the rule by rows64.CONTROL_MISS against the twin: a bound that fp32 arithmetic on the CPU breaks, or that cannot see
the defect, would prove nothing on the device."""
import math

import numpy as np
import pytest
import torch

from oracle import glowtts_ref as R
from oracle import loss64 as L64
from oracle import loss_cases as LC
from oracle.rows64 import AGG_F32, CONTROL_MISS, bf16_round, check, gamma

EQ = 1e-12
F64, F32 = torch.float64, torch.float32


def close(a, b, tol=EQ):
    a, b = torch.as_tensor(a, dtype=F64), torch.as_tensor(b, dtype=F64)
    return a.shape == b.shape and float((a - b).abs().max()) <= tol * max(1e-300, float(b.abs().max()))


def holds(name, twin, ref, bound, bads=()):
    """the twin passes the rule against ref; against every planted-defect reference it misses by CONTROL_MISS"""
    r = check(name, twin, ref, bound)
    msg = str(r)
    assert r.ok, msg
    for dname, bad in bads:
        c = check(f"{name} [{dname}]", twin, bad, bound)
        msg += f"; {dname} misses by {c.miss:.3g}x"
        assert c.miss >= CONTROL_MISS, str(c)
    print(msg)
    return r


# ----------------------------------------------------------------------------- pins to oracle/glowtts_ref.py and autograd
def test_logp_is_the_reference_lattice():
    x_m, x_logs, z = (t.double() for t in LC.logp_case((2, 18, 45, 161), True))
    ref, S, S_e = L64.logp(x_m, x_logs, z)
    assert close(ref, R.logp_lattice(x_m, x_logs, z))
    assert close(L64.logp(x_m, None, z)[0], R.logp_lattice(x_m, torch.zeros_like(x_m), z))
    assert (S >= ref.abs() * (1 - 1e-12)).all() and (S_e <= S).all()


def mle_inputs():
    g = torch.Generator().manual_seed(3)
    B, C, T, lens = 3, 4, 9, [9, 1, 5]
    mask = R.sequence_mask(torch.tensor(lens), T).unsqueeze(1).double()
    z, m = torch.randn(B, C, T, generator=g, dtype=F64), torch.randn(B, C, T, generator=g, dtype=F64)
    logs = torch.randn(B, C, T, generator=g, dtype=F64) * 0.4
    return z, m, logs, torch.randn(B, generator=g, dtype=F64), mask, C


def test_mle_is_the_reference_loss_and_its_backward_is_autograd():
    z, m, logs, logdet, mask, C = mle_inputs()
    for lg in (logs, None):
        zz, mm, ld = z.clone().requires_grad_(), m.clone().requires_grad_(), logdet.clone().requires_grad_()
        ll = torch.zeros_like(z) if lg is None else lg.clone()
        ll.requires_grad_()
        want = R.mle_loss(zz, mm, ll, ld, mask)
        loss, denom, bound = L64.mle(z, m, lg, logdet, mask, C)
        assert close(loss, want.detach().reshape(1)) and close(denom, (torch.ones_like(z) * mask).sum().reshape(1))
        assert float(bound) > 0
        (want * 1.7).backward()
        bw = L64.mle_bwd(z, m, lg, torch.tensor([1.7], dtype=F64), denom, 3)      # the kernel divides by the loss's denominator
        assert close(bw["dz"][0], zz.grad.reshape(-1)) and close(bw["dm"][0], mm.grad.reshape(-1))
        assert close(bw["dlogs"][0], ll.grad.reshape(-1)) and close(bw["dlogdet"][0], ld.grad)
        plain = L64.mle_bwd(z, m, lg, torch.tensor([1.7], dtype=F64), None, 3)           # gdenom NULL: g = gscale
        assert close(plain["dz"][0], zz.grad.reshape(-1) * float(denom))
    assert close(L64.mle(z[:0], m[:0], None, logdet, mask, C)[0], (-logdet.sum() / (C * mask.sum()) + 0.5 * math.log(2 * math.pi)).reshape(1))


def test_duration_loss_is_the_l_length_lines_and_its_backward_is_autograd():
    g = torch.Generator().manual_seed(5)
    B, Tx, lens = 3, 7, torch.tensor([7, 1, 4])
    x_mask = R.sequence_mask(lens, Tx).unsqueeze(1).double()
    w = torch.randint(0, 5, (B, 1, Tx), generator=g).double() * x_mask
    logw = (torch.randn(B, 1, Tx, generator=g, dtype=F64) * x_mask).requires_grad_()
    logw_ = torch.log(w + 1e-8) * x_mask                                             # oracle/glowtts_ref.py train_forward
    want = torch.sum((logw - logw_) ** 2, [1, 2]) / torch.sum(x_mask)
    assert close(L64.duration_loss(logw[:, 0], w[:, 0], lens), want.detach())
    gr = torch.randn(B, generator=g, dtype=F64)
    (want * gr).sum().backward()
    assert close(L64.duration_loss_bwd(logw[:, 0], w[:, 0], lens, gr), logw.grad[:, 0])
    junk = torch.where(x_mask[:, 0] > 0, w[:, 0], torch.full_like(w[:, 0], -3.0))     # w on padded tokens is ignored
    assert torch.equal(L64.duration_loss(logw[:, 0], junk, lens), L64.duration_loss(logw[:, 0], w[:, 0], lens))


def test_prior_expand_is_the_path_matmul_and_its_backward_is_autograd():
    g = torch.Generator().manual_seed(7)
    B, C, Tx, Ty = 2, 3, 6, 19
    dur = torch.tensor([[3., 1., 0., 5., 2., 4.], [2., 2., 0., 0., 0., 0.]], dtype=F64)
    xl, yl = torch.tensor([6, 2]), dur.sum(1).long()
    mask = (R.sequence_mask(xl, Tx).unsqueeze(-1) & R.sequence_mask(yl, Ty).unsqueeze(1)).double()
    attn = R.generate_path(dur, mask)                                                # [B, Tx, Ty]
    f2t = torch.where(attn.sum(1) > 0, attn.argmax(1), torch.full((B, Ty), -1))
    x_m = torch.randn(B, C, Tx, generator=g, dtype=F64).requires_grad_()
    z_m = torch.matmul(attn.transpose(1, 2), x_m.transpose(1, 2)).transpose(1, 2)    # models.py:1118
    assert torch.equal(L64.prior_expand(x_m, f2t), z_m.detach())
    dz = torch.randn(B, C, Ty, generator=g, dtype=F64)
    (z_m * dz).sum().backward()
    ref, S, run = L64.prior_expand_bwd(dz, f2t, Tx)
    assert close(ref, x_m.grad) and torch.equal(run, dur.long()) and (S >= ref.abs() * (1 - 1e-12)).all()


def test_embedding_backward_is_autograd_and_forward_is_a_scaled_gather():
    lay, ids, emb, V = LC.emb_case(True, 188, True)
    e = emb.double().requires_grad_()
    dx = torch.randn(lay.R, 192, generator=torch.Generator().manual_seed(1), dtype=F64)
    sc = float(np.float32(LC.EMB_SCALE))
    rows = torch.zeros(lay.R, 188, dtype=F64)
    for b in range(lay.B):
        rows = rows.index_add(0, torch.from_numpy(lay.frame_rows(b)), e[ids[b, :lay.lens[b]]] * sc)
    f32_rows, bf_rows = L64.embedding_fwd(ids, emb, lay, LC.EMB_SCALE, 192)
    assert close(f32_rows[:, :188], rows.detach(), 2.0 ** -23) and (f32_rows[:, 188:] == 0).all()
    assert (f32_rows[~lay.valid] == 0).all() and torch.equal(bf_rows[:, :188], torch.from_numpy(bf16_round(f32_rows[:, :188].numpy())))
    (rows * dx[:, :188]).sum().backward()
    prior = torch.ones(V, 188, dtype=F64)
    ref, S, cnt = L64.embedding_bwd(ids, dx, lay, LC.EMB_SCALE, V, prior)
    assert close(ref, e.grad + prior) and int(cnt.sum()) == sum(lay.lens)


def test_layout_restatements_are_the_reference_squeeze_and_unsqueeze():
    for C, Ty, ragged in [(3, 9, True), (3, 8, False), (1, 2, True), (2, 1, False)]:
        lay, len_sq, y, rows = LC.sqz_case(C, Ty, ragged)
        y = y.double()
        y_len = torch.tensor([2 * min(v, Ty // 2) for v in len_sq])
        mask = R.sequence_mask(y_len, Ty).unsqueeze(1).double()
        got = L64.squeeze_rows(y.numpy(), len_sq, lay)
        assert got.shape == (lay.R, 2 * C) and (got[~lay.valid] == 0).all()         # halos, padding, rounding rows
        if Ty >= 2:
            want, m2 = R.squeeze(y * mask, mask)                                     # [B, 2C, Ty // 2]
            back = L64.bct_from_rows(got, lay)
            assert np.array_equal(back, want.numpy())
            un, _ = R.unsqueeze(want, m2)
            mine = L64.unsqueeze_rows(got, len_sq, lay, Ty)
            assert np.array_equal(mine[:, :, :un.shape[2]], un.numpy()) and (mine[:, :, un.shape[2]:] == 0).all()   # odd trailing frame
        assert np.array_equal(L64.squeeze_rows(L64.unsqueeze_rows(rows.double().numpy(), len_sq, lay, Ty), len_sq, lay),
                              rows.double().numpy() * lay.valid[:, None])


def test_rows_from_bct_and_back():
    lay = L64.Layout(LC.BCT_LENS, LC.BCT_T, True)
    assert lay.R == 136 and L64.Layout(LC.BCT_LENS, LC.BCT_T, False).R == 325
    x = np.random.default_rng(0).standard_normal((5, 3, LC.BCT_T))
    on = np.arange(LC.BCT_T)[None, :] < np.asarray(LC.BCT_LENS)[:, None]
    for ragged in (True, False):
        lay = L64.Layout(LC.BCT_LENS, LC.BCT_T, ragged)
        rows = L64.rows_from_bct(x * on[:, None, :], lay)
        assert (rows[~lay.valid] == 0).all()                                         # zero past the lengths in, zero halos out
        assert np.array_equal(L64.bct_from_rows(rows, lay), x * on[:, None, :])
        full = L64.rows_from_bct(x, lay)                                             # frames past a length are copied as they are
        assert np.array_equal(full[lay.valid], rows[lay.valid]) and (full[lay.rowframe < 0] == 0).all()
    assert np.array_equal(L64.cast([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8], False), [1.0, 1 + 2.0 ** -6])   # ties to even
    assert np.array_equal(L64.rows_f32_to_bf16(np.array([[3.0, 1 + 2.0 ** -9]]), np.array([0.5]), 2), [[1.5, 0.5]])
    assert np.array_equal(L64.rows_add_bf16(np.array([[1.0, 2.0]]), np.array([[2.0 ** -24, 1.0]]), 2), [[1.0, 3.0]])


def test_length_mask_and_rows_add_cond_and_utt_sum():
    assert torch.equal(L64.length_mask([3, 0, 5], 4), R.sequence_mask(torch.tensor([3, 0, 5]), 4).double())
    for ragged in (True, False):
        lay, x, cond, prior = LC.rows_case(ragged, 8)
        f, bf = L64.rows_add_cond(x, cond, lay, lay.rowmask, 8)
        want = (x.double() + cond.double()[lay.rowbatch]) * torch.from_numpy(lay.rowmask.astype(np.float64))[:, None]
        assert close(f, want, 2.0 ** -23) and (f[~lay.valid] == 0).all()
        xn = x.clone()
        xn[~torch.from_numpy(lay.valid)] = float("nan")                              # masked rows are not read
        assert torch.equal(L64.rows_add_cond(xn, cond, lay, lay.rowmask, 8)[0], f)
        ref, S = L64.rows_utt_sum(xn, lay, lay.rowmask, 8, prior)
        want = torch.stack([x.double()[lay.frame_rows(b)].sum(0) for b in range(lay.B)]) + prior.double()
        assert close(ref, want) and torch.isfinite(S).all()
        ref0, _ = L64.rows_utt_sum(x, lay, None, 8)                                  # rowmask NULL: every row the utterance owns
        assert close(ref0.sum(0), x.double().sum(0)) and int(lay.count.sum()) == lay.R


# ----------------------------------------------------------------------------- the float32 twin under the rule, planted defects seen
@pytest.mark.parametrize("with_logs", [False, True])
@pytest.mark.parametrize("shape", LC.LOGP_SHAPES)
def test_logp_twin_passes_and_defects_are_seen(shape, with_logs):
    x_m, x_logs, z = LC.logp_case(shape, with_logs)
    ref, S, S_e = L64.logp(x_m, x_logs, z)
    twin = L64.logp(x_m, x_logs, z, dtype=F32)[0]
    bads = [(d, L64.logp(x_m, x_logs, z, defect=d)[0]) for d in LC.logp_defects(shape, with_logs)]
    r = holds(f"logp twin {shape} logs={with_logs}", twin, ref, L64.logp_bound(shape[1], S, S_e, with_logs), bads)
    assert r.agg < AGG_F32 / 10


@pytest.mark.parametrize("with_logs", [False, True])
@pytest.mark.parametrize("n", LC.mle_ns())
def test_mle_twin_passes_and_probe_indices_cover_both_trips(n, with_logs):
    for B in LC.MLE_B:
        z, m, logs, logdet, mask, C = LC.mle_case(n, B)
        lg = logs if with_logs else None
        loss, denom, bound = L64.mle(z, m, lg, logdet, mask, C)
        tl, td, _ = L64.mle(z, m, lg, logdet, mask, C, dtype=F32)
        assert float(td) == float(denom) and mask.numel() % 4 and float(mask[-1]) == 1
        short = L64.mle(z, m, lg, logdet, mask[:-1], C)[0]                                # a wrong sum(mask): the last float left out
        holds(f"mle twin n={n} B={B} logs={with_logs}", tl, loss, bound, [("mask_short", short)])
    idx = LC.mle_probe_indices(n)
    assert idx[0] == 0 and idx[-1] == n - 1 and (n < LC.mle_trip() or {LC.mle_trip() - 1, LC.mle_trip()} <= set(idx))


@pytest.mark.parametrize("n", LC.mle_bwd_ns())
def test_mle_bwd_twin_passes_and_defects_are_seen(n):
    z, m, logs, gs, gd = LC.mle_bwd_case(n)
    for lg in (logs, None):
        for den in (gd, None):
            ref = L64.mle_bwd(z, m, lg, gs, den, 300)
            twin = L64.mle_bwd(z, m, lg, gs, den, 300, dtype=F32)
            bad = {"dlogs": ("dlogs_no_one", L64.mle_bwd(z, m, lg, gs, den, 300, defect="dlogs_no_one")["dlogs"][0]),
                   "dm": ("dm_sign", L64.mle_bwd(z, m, lg, gs, den, 300, defect="dm_sign")["dm"][0])}
            for k in ("dz", "dm", "dlogs", "dlogdet"):
                holds(f"mle_bwd twin n={n} {k}", twin[k][0], ref[k][0], ref[k][1], [bad[k]] if k in bad else [])


@pytest.mark.parametrize("B,Tx", LC.DUR_SHAPES)
def test_duration_loss_defects_are_seen_at_the_twin_limit(B, Tx):
    logw, w, lens, gr = LC.dur_case(B, Tx)
    assert int(lens.max()) == Tx and (B == 1 or int(lens.min()) == 1)
    for key, op, extra in (("fwd", L64.duration_loss, ()), ("bwd", L64.duration_loss_bwd, (gr,))):
        ref, twin = op(logw, w, lens, *extra), op(logw, w, lens, *extra, dtype=F32)
        assert torch.isfinite(ref).all()
        lim = max(LC.DUR_M[key] * LC.rel_l2(twin, ref), 2.0 ** -23)
        for d in LC.dur_defects(B, Tx):
            miss = LC.rel_l2(twin, op(logw, w, lens, *extra, defect=d)) / lim
            print(f"duration_loss {key} B={B} Tx={Tx}: {d} misses by {miss:.3g}x")
            assert miss >= CONTROL_MISS


@pytest.mark.parametrize("Tx,Ty", LC.PRIOR_SHAPES)
def test_prior_expand_bwd_twin_passes_and_maps_hold_their_edges(Tx, Ty):
    x_m, f2t, dz = LC.prior_case(Tx, Ty)
    ref, S, run = L64.prior_expand_bwd(dz, f2t, Tx)
    twin = L64.prior_expand_bwd(dz, f2t, Tx, dtype=F32)[0]
    bads = [(d, L64.prior_expand_bwd(dz, f2t, Tx, defect=d)[0]) for d in LC.prior_defects(Tx, Ty)]
    holds(f"prior_expand_bwd twin {Tx}x{Ty}", twin, ref, gamma(run.double())[:, None, :] * S, bads)
    if Ty > 64:
        t = f2t[0].tolist()
        assert t[63] != t[64]                                                        # a run ends exactly on lane 63
        assert any(len({j // 64 for j, v in enumerate(row) if v == i}) >= 3 for row in f2t.tolist() for i in set(row) if i >= 0)
        assert any(b - a >= 2 for row in f2t.tolist() for a, b in zip(row, row[1:]) if a >= 0 and b >= 0)   # a token with no frame
        assert t[-1] == -1 and not torch.equal(f2t[0], f2t[1])


@pytest.mark.parametrize("Ce,ld", LC.EMB_DIMS)
@pytest.mark.parametrize("ragged", [False, True])
def test_embedding_bwd_twin_passes_and_defects_are_seen(ragged, Ce, ld):
    lay, ids, emb, V = LC.emb_case(ragged, Ce, True)
    dx = torch.randn(lay.R, ld, generator=LC.gen(Ce, 23))
    prior = torch.randn(V, Ce, generator=LC.gen(Ce, 29))
    ref, S, cnt = L64.embedding_bwd(ids, dx, lay, LC.EMB_SCALE, V, prior)
    twin = L64.embedding_bwd(ids, dx, lay, LC.EMB_SCALE, V, prior, dtype=F32)[0]
    bads = [(d, L64.embedding_bwd(ids, dx, lay, LC.EMB_SCALE, V, prior, defect=d)[0]) for d in ("no_scale", "drop_last")]
    holds(f"embedding_bwd twin ragged={ragged} C={Ce}", twin, ref, gamma(cnt.double())[:, None] * S, bads)


@pytest.mark.parametrize("C,ldo", LC.ROWS_DIMS)
@pytest.mark.parametrize("ragged", [False, True])
def test_rows_utt_sum_twin_passes(ragged, C, ldo):
    lay, x, cond, prior = LC.rows_case(ragged, C)
    for mask, pr in ((lay.rowmask, prior), (None, None)):
        ref, S = L64.rows_utt_sum(x, lay, mask, C, pr)
        twin = L64.rows_utt_sum(x, lay, mask, C, pr, dtype=F32)[0]
        bad = ref + x.double()[int(lay.frame_rows(2)[0]), :C] * (torch.arange(lay.B) == 1)[:, None]      # a frame credited to its neighbour
        holds(f"rows_utt_sum twin ragged={ragged} C={C}", twin, ref, gamma(torch.from_numpy(lay.count).double())[:, None] * S, [("neighbour", bad)])


# ----------------------------------------------------------------------------- GT_MLE_PARTS: header, mirror, the buffer _MleLossFn allocates
def test_mle_partial_buffer_is_sized_from_the_header(monkeypatch):
    from glow_tts_amd import _lib, text_models
    parts = L64.header_constant("GT_MLE_PARTS")
    assert _lib.MLE_PARTS == parts
    seen = {}

    class FakeCall:
        def gt_mle_sums(self, z, m, logs, acc, n, stream):
            seen["acc"] = acc.numel()

        def gt_mle_finish(self, acc, ld, mk, n_mask, B, C, out, stream):
            out.zero_()

    monkeypatch.setattr(text_models, "call", FakeCall())
    monkeypatch.setattr(_lib, "current_stream", lambda dev: None)
    z, m, logs, logdet, mask, C = mle_inputs()
    text_models._MleLossFn.apply(z.float(), m.float(), None, logdet.float(), mask.float())
    assert seen["acc"] == 2 * parts
