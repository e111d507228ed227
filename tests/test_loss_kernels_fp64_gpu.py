"""The fp32 kernels between the decoder and the loss (csrc/align_loss.hip: gt_logp_f32, gt_mle_sums / _finish / _bwd,
gt_duration_loss_fwd / _bwd, gt_prior_expand / _bwd, gt_length_mask; csrc/encoder_ops.hip: gt_embedding_fwd / _bwd, gt_rows_add_cond,
gt_rows_utt_sum)
against float64 on hand-made operands, under the rule of oracle/rows64.py with the operators of oracle/loss64.py.  The shapes,
operands and planted defects are oracle/loss_cases.py's, the ones tests/test_loss64.py validates on the float32 twin.

Every entry is called through _lib.call between guards (oracle/guards.py): outputs inside canaries and pre-filled with canaries,
inputs between NaN guards, accumulate-into outputs pre-filled with non-zero values.  Padded positions of index inputs (ids,
frame2token, the guards of lengths) hold valid in-range values that differ from the real ones: a wrong kernel gives a wrong number.

Each check prints one Report line with the miss factor of every planted defect, each required to be >= rows64.CONTROL_MISS.
__logf (the duration loss) is outside the rule and held to the float32 twin: rel-L2 err_kernel <= max(M err_twin, 2^-23), both
against float64, M = loss_cases.DUR_M (twice the worst ratio measured on an MI355X, rounded up)."""
import itertools

import numpy as np
import pytest
import torch

from oracle import loss64 as L64
from oracle import loss_cases as LC
from oracle.guards import CAN, Guards
from oracle.rows64 import CONTROL_MISS, check, gamma

pytestmark = pytest.mark.gpu
F32, BF16 = torch.float32, torch.bfloat16
GT_E_INVAL = -1


def dev():
    return torch.device("cuda:0")


def api():
    from glow_tts_amd import _lib
    return _lib.call, _lib.current_stream(dev()), _lib


def rule(name, got, ref, bound, bads=(), kind="f32"):
    """the rule against the float64 reference must hold; against every planted-defect reference it must miss by CONTROL_MISS"""
    r = check(name, got, ref, bound, kind)
    msg = str(r)
    misses = []
    for dname, bad in bads:
        c = check(f"{name} [{dname}]", got, bad, bound, kind)
        misses.append((dname, c))
        msg += f"; {dname} misses by {c.miss:.3g}x"
    print(msg)
    assert r.ok, msg
    for dname, c in misses:
        assert c.miss >= CONTROL_MISS, f"planted defect not seen: {c}"
    return r


def exact(name, got, want):
    got, want = got.detach().float().cpu().double().numpy(), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, name
    bad = int((got != want).sum())
    print(f"{name}: {got.size} elements, {bad} differ")
    assert bad == 0, name


# ----------------------------------------------------------------------------- gt_logp_f32
@pytest.mark.parametrize("with_logs", [False, True])
@pytest.mark.parametrize("shape", LC.LOGP_SHAPES)
def test_logp_lattice_against_float64(built, shape, with_logs):
    call, st, _ = api()
    B, C, Tx, Ty = shape
    x_m, x_logs, z = LC.logp_case(shape, with_logs)
    G = Guards(dev())
    out = G.out("logp", (B, Tx, Ty))
    call.gt_logp_f32(G.inp(x_m), G.inp(x_logs), G.inp(z), out, B, C, Tx, Ty, st)
    G.verify()
    ref, S, S_e = L64.logp(x_m, x_logs, z)
    bads = [(d, L64.logp(x_m, x_logs, z, defect=d)[0]) for d in LC.logp_defects(shape, with_logs)]
    rule(f"gt_logp_f32 {shape} x_logs={'set' if with_logs else 'NULL'}", out, ref, L64.logp_bound(C, S, S_e, with_logs), bads)


def test_logp_refuses_an_odd_channel_count(built):
    call, st, _lib = api()
    t = torch.zeros(64, device=dev())
    with pytest.raises(_lib.GtError) as e:
        call.gt_logp_f32(t, None, t, t, 1, 5, 1, 1, st)
    assert e.value.code == GT_E_INVAL


# ----------------------------------------------------------------------------- gt_mle_sums + gt_mle_finish
def mle_launch(G, z, m, logs, n, logdet, mask, C, acc_prior=None):
    """gt_mle_sums into guarded partials (all written), then gt_mle_finish -> (out2 [2], acc2)"""
    call, st, _ = api()
    parts = L64.header_constant("GT_MLE_PARTS")
    acc = G.out("acc2", (2 * parts,), prior=acc_prior)
    call.gt_mle_sums(z, m, logs, acc, n, st)
    out = G.out("out2", (2,))
    call.gt_mle_finish(acc, logdet, mask, mask.numel(), logdet.numel(), C, out, st)
    G.verify()
    return out, acc


@pytest.mark.parametrize("with_logs", [False, True])
@pytest.mark.parametrize("n", LC.mle_ns())
def test_mle_sums_and_finish_against_float64(built, n, with_logs):
    for B in LC.MLE_B:
        z, m, logs, logdet, mask, C = LC.mle_case(n, B)
        lg = logs if with_logs else None
        loss, denom, bound = L64.mle(z, m, lg, logdet, mask, C)
        short = L64.mle(z, m, lg, logdet, mask[:-1], C)[0]
        G = Guards(dev())
        dz, dm, dl = G.inp(z), G.inp(m), G.inp(lg)
        for shift in (0, 1):                                   # the mask 16-byte aligned, and one float off: gt_mle_finish's two loops
            out, _ = mle_launch(G, dz, dm, dl, n, G.inp(logdet), G.inp(mask, shift=shift), C)
            assert (out.data_ptr() % 16 == 0) and mask.numel() % 4 != 0
            tag = f"n={n} logs={'set' if with_logs else 'NULL'} B={B} mask {'aligned' if shift == 0 else '+4 bytes'}"
            rule(f"gt_mle_finish loss {tag}", out[:1], loss, bound, [("mask_short", short)])
            exact(f"gt_mle_finish denom {tag}", out[1:], denom)


@pytest.mark.parametrize("with_logs", [False, True])
@pytest.mark.parametrize("n", LC.mle_ns())
def test_mle_sums_one_hot_probes(built, n, with_logs):
    """one non-zero z - m (and, with logs, one non-zero logs) element at every index where gt_mle_sums changes its path: out[0] must
    hold that element's contribution to 2^-22 relative (e^0 = 1: no __expf error in either probe)"""
    G = Guards(dev())
    z, m = G.inp(torch.zeros(n)), G.inp(torch.zeros(n))
    logs = G.inp(torch.zeros(n)) if with_logs else None
    logdet, mask, C = G.inp(torch.zeros(2)), G.inp(torch.tensor([1., 0., 1., 1., 1.])), 2        # denom 8
    for i in LC.mle_probe_indices(n):
        for probe, val, want in (("z-m", 3.0, 0.5 * 9.0 / 8), ("logs", 0.75, 0.75 / 8))[:2 if with_logs else 1]:
            t = z if probe == "z-m" else logs
            t[i] = val
            out, _ = mle_launch(G, z, m, logs, n, logdet, mask, C)
            t[i] = 0.0
            G.outs.clear()
            got, want = float(out[0]), want + L64.HALF_LOG_2PI
            rel = abs(got - want) / want
            print(f"gt_mle_sums probe n={n} {probe}[{i}]: out[0] {got:.9g} want {want:.9g} rel {rel:.3g}")
            assert rel <= 2.0 ** -22


def test_mle_sums_of_nothing_leaves_zero_partials(built):
    """n == 0 (fixed here: the entry used to return without writing, and gt_mle_finish summed whatever the buffer held)"""
    parts = L64.header_constant("GT_MLE_PARTS")
    _, _, _, logdet, mask, _ = LC.mle_case(7, 2)
    for ptr in (None, torch.zeros(4, device=dev())):
        G = Guards(dev())
        out, acc = mle_launch(G, ptr, ptr, None, 0, G.inp(logdet), G.inp(mask), 3, acc_prior=torch.full((2 * parts,), float("nan")))
        assert bool((acc == 0).all()), "a partial pair was not written"
        loss, denom, bound = L64.mle(torch.zeros(0), torch.zeros(0), None, logdet, mask, 3)
        assert abs(float(loss) - (-float(logdet.double().sum()) / float(denom) + L64.HALF_LOG_2PI)) < 1e-12
        rule("gt_mle_finish loss n=0", out[:1], loss, bound)


# ----------------------------------------------------------------------------- gt_mle_bwd
@pytest.mark.parametrize("n", LC.mle_bwd_ns())
def test_mle_bwd_against_float64(built, n):
    call, st, _ = api()
    z, m, logs, gs, gd = LC.mle_bwd_case(n)
    G = Guards(dev())
    dz_, dm_, dl_, dgs, dgd = G.inp(z), G.inp(m), G.inp(logs), G.inp(gs), G.inp(gd)
    refs = {}
    for lg, den in itertools.product((True, False), (True, False)):
        a = (z, m, logs if lg else None, gs, gd if den else None, max(LC.MLE_BWD_B))
        refs[lg, den] = (L64.mle_bwd(*a), L64.mle_bwd(*a, defect="dlogs_no_one")["dlogs"][0], L64.mle_bwd(*a, defect="dm_sign")["dm"][0])
    launch = 0
    for lg in (True, False):
        for want in itertools.product((True, False), repeat=3):                      # every NULL combination of dz / dm / dlogs
            den, B = bool(launch & 1), LC.MLE_BWD_B[(launch >> 1) & 1]
            with_ld = launch % 5 != 4
            launch += 1
            G.outs.clear()
            outs = {k: G.out(k, (n,)) for k, w in zip(("dz", "dm", "dlogs"), want) if w}
            if with_ld:
                outs["dlogdet"] = G.out("dlogdet", (B,))
            call.gt_mle_bwd(dz_, dm_, dl_ if lg else None, dgs, outs.get("dz"), outs.get("dm"), outs.get("dlogs"), n, dgd if den else None,
                            outs.get("dlogdet"), B, st)
            G.verify()
            ref, bad_dlogs, bad_dm = refs[lg, den]
            for k, got in outs.items():
                bads = {"dlogs": [("dlogs_no_one", bad_dlogs)], "dm": [("dm_sign", bad_dm)]}.get(k, [])
                r, b = ref[k]
                if k == "dlogdet":
                    r, b = r[:B], b[:B]
                rule(f"gt_mle_bwd n={n} logs={'set' if lg else 'NULL'} gdenom={'set' if den else 'NULL'} B={B} {k}", got, r, b, bads)


# ----------------------------------------------------------------------------- gt_duration_loss_fwd / _bwd
def hold_twin(key, name, got, ref, twin, bads):
    ek, et = LC.rel_l2(got, ref), LC.rel_l2(twin, ref)
    lim = max(LC.DUR_M[key] * et, 2.0 ** -23)
    msg = f"RATIO {key} {name}: err_kernel {ek:.3e} err_twin {et:.3e} ratio {ek / max(et, 1e-300):.3f} limit {lim:.3e}"
    misses = [(d, LC.rel_l2(got, bad) / lim) for d, bad in bads]
    print(msg + "".join(f"; {d} misses by {x:.3g}x" for d, x in misses))
    assert ek <= lim, msg
    for d, x in misses:
        assert x >= CONTROL_MISS, f"planted defect {d} not seen: {msg}"


@pytest.mark.parametrize("B,Tx", LC.DUR_SHAPES)
def test_duration_loss_against_float64_and_its_float32_twin(built, B, Tx):
    call, st, _ = api()
    logw, w, lens, gr = LC.dur_case(B, Tx)
    G = Guards(dev())
    d_logw, d_w, d_lens, d_g = G.inp(logw), G.inp(w), G.inp(lens, fill=1), G.inp(gr)
    l = G.out("l_length", (B,))
    call.gt_duration_loss_fwd(d_logw, d_w, d_lens, B, Tx, l, st)
    dl = G.out("dlogw", (B, Tx))
    call.gt_duration_loss_bwd(d_logw, d_w, d_lens, d_g, B, Tx, dl, st)
    G.verify()
    for key, op, extra, got in (("fwd", L64.duration_loss, (), l), ("bwd", L64.duration_loss_bwd, (gr,), dl)):
        ref, twin = op(logw, w, lens, *extra), op(logw, w, lens, *extra, dtype=F32)
        bads = [(d, op(logw, w, lens, *extra, defect=d)) for d in LC.dur_defects(B, Tx)]
        hold_twin(key, f"B={B} Tx={Tx}", got.cpu(), ref, twin, bads)
    on = torch.arange(Tx)[None, :] < lens[:, None]
    assert bool((dl.cpu()[~on] == 0).all()), "dlogw on a padded token (logw is zero there)"


# ----------------------------------------------------------------------------- gt_prior_expand / _bwd
@pytest.mark.parametrize("Tx,Ty", LC.PRIOR_SHAPES)
def test_prior_expand_and_its_backward(built, Tx, Ty):
    call, st, _ = api()
    B, C = LC.PRIOR_B, LC.PRIOR_C
    x_m, f2t, dz = LC.prior_case(Tx, Ty)
    G = Guards(dev())
    d_f2t = G.inp(f2t, fill=0)
    z_m = G.out("z_m", (B, C, Ty))
    call.gt_prior_expand(G.inp(x_m), d_f2t, z_m, B, C, Tx, Ty, st)
    dx = G.out("dx_m", (B, C, Tx))
    call.gt_prior_expand_bwd(G.inp(dz), d_f2t, dx, B, C, Tx, Ty, st)
    G.verify()
    exact(f"gt_prior_expand {Tx}x{Ty}", z_m, L64.prior_expand(x_m, f2t).numpy())
    ref, S, run = L64.prior_expand_bwd(dz, f2t, Tx)
    bads = [(d, L64.prior_expand_bwd(dz, f2t, Tx, defect=d)[0]) for d in LC.prior_defects(Tx, Ty)]
    rule(f"gt_prior_expand_bwd {Tx}x{Ty}", dx, ref, gamma(run.double())[:, None, :] * S, bads)
    assert bool((dx.cpu()[(run == 0)[:, None, :].expand(-1, C, -1)] == 0).all())      # tokens without a frame


# ----------------------------------------------------------------------------- gt_embedding_fwd / _bwd
def row0_of(G, lay):
    return None if lay.row0 is None else G.inp(torch.from_numpy(lay.row0), fill=int(lay.R))


@pytest.mark.parametrize("Ce,ld", LC.EMB_DIMS)
@pytest.mark.parametrize("ragged", [False, True])
def test_embedding_forward_is_exact(built, ragged, Ce, ld):
    call, st, _ = api()
    lay, ids, emb, V = LC.emb_case(ragged, Ce, False)
    want32, want16 = L64.embedding_fwd(ids, emb, lay, LC.EMB_SCALE, ld)
    keep = (torch.arange(ld) >= Ce)[None, :]
    for f32, bf in ((True, True), (True, False), (False, True)):                      # each output is optional
        G = Guards(dev())
        o32 = G.out("out_f32", (lay.R, ld), keep=keep) if f32 else None
        o16 = G.out("out_bf16", (lay.R, ld), dtype=BF16, keep=keep) if bf else None
        call.gt_embedding_fwd(G.inp(ids, fill=0), G.inp(emb), G.inp(torch.tensor(lay.lens, dtype=torch.int32), fill=0), o32, o16,
                              lay.B, lay.T, lay.Tp, row0_of(G, lay), lay.R, Ce, ld, LC.EMB_SCALE, st)
        G.verify()
        tag = f"gt_embedding_fwd ragged={ragged} C={Ce} ld={ld}"
        if f32:
            exact(tag + " fp32", o32[:, :Ce], want32[:, :Ce].numpy())
        if bf:
            exact(tag + " bf16", o16[:, :Ce], want16[:, :Ce].numpy())


@pytest.mark.parametrize("Ce,ld", LC.EMB_DIMS)
@pytest.mark.parametrize("ragged", [False, True])
def test_embedding_backward_against_float64(built, ragged, Ce, ld):
    call, st, _ = api()
    lay, ids, emb, V = LC.emb_case(ragged, Ce, True)
    dx = torch.randn(lay.R, ld, generator=LC.gen(Ce, 23))
    prior = torch.randn(V, Ce, generator=LC.gen(Ce, 29))
    dxn = dx.clone()
    dxn[~torch.from_numpy(lay.valid)] = float("nan")                                 # halo and padded rows are not read
    dxn[:, Ce:] = float("nan")
    G = Guards(dev())
    demb = G.out("demb", (V, Ce), prior=prior)
    call.gt_embedding_bwd(G.inp(ids, fill=0), G.inp(dxn), G.inp(torch.tensor(lay.lens, dtype=torch.int32), fill=0), demb,
                          lay.B, lay.T, lay.Tp, row0_of(G, lay), lay.R, Ce, ld, LC.EMB_SCALE, st)
    G.verify()
    ref, S, cnt = L64.embedding_bwd(ids, dx, lay, LC.EMB_SCALE, V, prior)
    bads = [(d, L64.embedding_bwd(ids, dx, lay, LC.EMB_SCALE, V, prior, defect=d)[0]) for d in ("no_scale", "drop_last")]
    rule(f"gt_embedding_bwd ragged={ragged} C={Ce} ld={ld}", demb, ref, gamma(cnt.double())[:, None] * S, bads)


# ----------------------------------------------------------------------------- gt_rows_add_cond, gt_rows_utt_sum, gt_length_mask
@pytest.mark.parametrize("C,ldo", LC.ROWS_DIMS)
@pytest.mark.parametrize("ragged", [False, True])
def test_rows_add_cond_is_exact(built, ragged, C, ldo):
    call, st, _ = api()
    lay, x, cond, _ = LC.rows_case(ragged, C)
    off = ~torch.from_numpy(lay.valid)
    keep = (torch.arange(ldo) >= C)[None, :]
    for src_f32 in (True, False):
        xs = x if src_f32 else x.to(BF16)
        want32, want16 = L64.rows_add_cond(xs.float(), cond, lay, lay.rowmask, C)
        xn = xs.clone()
        xn[off] = float("nan")                                                       # halos hold NaN and must be ignored
        for f32, bf in ((True, True), (True, False), (False, True)):
            G = Guards(dev())
            o32 = G.out("out", (lay.R, ldo), keep=keep) if f32 else None
            o16 = G.out("outb", (lay.R, ldo), dtype=BF16, keep=keep) if bf else None
            dx = G.inp(xn)
            call.gt_rows_add_cond(dx if src_f32 else None, C, None if src_f32 else dx, C, G.inp(cond), G.inp(torch.from_numpy(lay.rowmask)),
                                  o32, ldo, o16, ldo, lay.B, lay.R, C, lay.Tp, row0_of(G, lay), st)
            G.verify()
            tag = f"gt_rows_add_cond ragged={ragged} C={C} ldo={ldo} src={'fp32' if src_f32 else 'bf16'}"
            if f32:
                exact(tag + " fp32", o32[:, :C], want32.numpy())
            if bf:
                exact(tag + " bf16", o16[:, :C], want16.numpy())


@pytest.mark.parametrize("C,ldo", LC.ROWS_DIMS)
@pytest.mark.parametrize("ragged", [False, True])
def test_rows_utt_sum_against_float64(built, ragged, C, ldo):
    call, st, _ = api()
    lay, x, _, prior = LC.rows_case(ragged, C)
    valid = torch.from_numpy(lay.valid)
    keep = (torch.arange(ldo) >= C)[None, :]
    K = gamma(torch.from_numpy(lay.count).double())[:, None]
    for is_f32, masked, acc in itertools.product((True, False), (True, False), (0, 1)):
        xs = x if is_f32 else x.to(BF16)
        y = xs.clone()
        y[~valid] = float("nan") if masked else 0.0                                  # rowmask given: halos hold NaN; NULL: halos are zero
        mask = lay.rowmask if masked else None
        ref, S = L64.rows_utt_sum(xs.float() * valid[:, None], lay, mask, C, prior if acc else None)
        bad = ref + xs.double()[int(lay.frame_rows(2)[0]), :C] * (torch.arange(lay.B) == 1)[:, None]   # a frame credited to its neighbour
        G = Guards(dev())
        start = torch.full((lay.B, ldo), CAN)
        start[:, :C] = prior
        out = G.out("out", (lay.B, ldo), prior=start if acc else None, keep=keep)
        call.gt_rows_utt_sum(G.inp(y), C, int(is_f32), G.inp(None if mask is None else torch.from_numpy(mask)), out, ldo, acc,
                             lay.B, lay.R, C, lay.Tp, row0_of(G, lay), st)
        G.verify()
        rule(f"gt_rows_utt_sum ragged={ragged} C={C} ldo={ldo} y={'fp32' if is_f32 else 'bf16'} rowmask={'set' if masked else 'NULL'} "
             f"accumulate={acc}", out[:, :C], ref, K * S, [("neighbour", bad)])


@pytest.mark.parametrize("B,T", LC.LENGTH_MASK_SHAPES)
def test_length_mask_is_exact(built, B, T):
    call, st, _ = api()
    assert (B * T) % 256 != 0
    lens = torch.tensor([T, 0, 1, T + 5, T // 2][:B])
    for dt in (torch.int32, torch.int64):
        G = Guards(dev())
        mask = G.out("mask", (B, T))
        call.gt_length_mask(G.inp(lens.to(dt), fill=T), int(dt == torch.int64), mask, B, T, st)
        G.verify()
        exact(f"gt_length_mask {B}x{T} {dt}", mask, L64.length_mask(lens, T).numpy())
