"""The alignment -> loss chain in three launches (csrc/align_loss.hip: gt_align_loss_fwd / _finish / _bwd) against the chain of
entries it replaces — gt_prior_expand, gt_mle_sums, gt_mle_finish, gt_duration_loss_fwd, torch.sum and the add; gt_mle_bwd,
gt_prior_expand_bwd, gt_duration_loss_bwd — BIT for bit on the same operands, against float64 (oracle/loss64.py) under the bounds
tests/test_loss_kernels_fp64_gpu.py holds the unfused kernels to, its refusals, and one eager Trainer step with the switch on
against one with it off.

Operands: B = 3 ragged utterances per shape — utterance 0 full length, with (where the shape has room) one token that owns more than
64 frames, so that its run crosses the backward's 64-frame chunk boundary, and one token that owns none; utterance 1 a ONE-token
text whose mel ends 3 frames (not a multiple of 4) before the padded T_y; utterance 2 TWO frames long.  frame2token is built on the
host from monotone durations and is -1 on every padded frame; z is non-zero on padded frames too (both chains must treat them
alike).  The reference chain is computed once per (C, shape, x_logs) and shared.

out4[2] (the sum of l_length) is compared with torch.sum of the same device vector for every B in SUM_BS (all below 128, where
ATen's order is the one the kernel restates), and with a host restatement of the kernel's own documented order for B = 200."""
import functools

import numpy as np
import pytest
import torch

from oracle import loss64 as L64
from oracle import loss_cases as LC
from oracle.guards import CAN, Guards
from oracle.rows64 import check, gamma

pytestmark = pytest.mark.gpu
F32 = torch.float32
GT_E_INVAL, GT_E_UNSUPPORTED, GT_E_ALIGN = -1, -2, -3
B = 3
CS = [6, 80]
SHAPES = [(1, 4), (7, 32), (70, 96), (150, 160)]
SUM_BS = [1, 2, 3, 5, 8, 13, 16, 31, 32, 33, 64, 100]


def dev():
    return torch.device("cuda:0")


def api():
    from glow_tts_amd import _lib
    return _lib.call, _lib.current_stream(dev()), _lib


def bits_equal(name, got, want):
    a, b = got.detach().contiguous().cpu().view(torch.int32), want.detach().contiguous().cpu().view(torch.int32)
    assert a.shape == b.shape, name
    bad = int((a != b).sum())
    print(f"{name}: {a.numel()} elements, {bad} differ in bits")
    assert bad == 0, name


def rule(name, got, ref, bound):
    r = check(name, got, ref, bound, "f32")
    print(str(r))
    assert r.ok, str(r)


def durations(rng, n_tok, n_frames, big, empty):
    """n_tok monotone durations (zeros allowed) that sum to n_frames; big: token 1 (or 0) owns > 64 frames; empty: the last but one
    token owns none"""
    d = np.zeros(n_tok, dtype=np.int64)
    rest = n_frames
    if big and n_frames >= 70 and n_tok >= 2:
        d[1] = 67
        rest -= 67
    cuts = np.sort(rng.integers(0, rest + 1, size=n_tok - 1))
    d += np.diff(np.concatenate([[0], cuts, [rest]]))
    if empty and n_tok >= 3:
        d[0] += d[n_tok - 2]
        d[n_tok - 2] = 0
    assert d.sum() == n_frames and (d >= 0).all()
    return d


@functools.lru_cache(maxsize=None)
def case(C, Tx, Ty):
    """host operands of one shape"""
    rng = np.random.default_rng(1000 * C + 10 * Tx + Ty)
    g = torch.Generator().manual_seed(7 * C + Tx + Ty)
    x_len = [Tx, 1, min(Tx, 2)]
    y_len = [Ty, max(1, Ty - 3), min(Ty, 2)]
    dur = np.zeros((B, Tx), dtype=np.int64)
    f2t = -np.ones((B, Ty), dtype=np.int32)
    for b in range(B):
        dur[b, :x_len[b]] = durations(rng, x_len[b], y_len[b], big=b == 0, empty=b == 0)
        f2t[b, :y_len[b]] = np.repeat(np.arange(Tx), dur[b])
    if Ty >= 96:
        assert dur[0].max() > 64
    if Tx >= 3:
        assert (dur[0, :x_len[0]] == 0).any()
    assert (Ty - y_len[1]) % 4 != 0 or Ty == 4
    on = torch.arange(Tx)[None, :] < torch.tensor(x_len)[:, None]
    return dict(
        z=torch.randn(B, C, Ty, generator=g) * 1.5, x_m=torch.randn(B, C, Tx, generator=g),
        x_logs=(torch.randn(B, C, Tx, generator=g) * 0.7).clamp_(-2, 2), f2t=torch.from_numpy(f2t),
        logw=torch.randn(B, Tx, generator=g) * on, w=torch.from_numpy(dur).float(), x_len=torch.tensor(x_len, dtype=torch.int32),
        logdet=torch.randn(B, generator=g) * 50, mask=(torch.arange(Ty)[None, :] < torch.tensor(y_len)[:, None]).float()[:, None, :])


@functools.lru_cache(maxsize=None)
def device_case(C, Tx, Ty):
    return {k: v.to(dev()) for k, v in case(C, Tx, Ty).items()}


@functools.lru_cache(maxsize=None)
def unfused(C, Tx, Ty, with_logs, gscale):
    """the chain of existing entries on the device operands -> dict of device tensors (computed once, never written again)"""
    call, st, _ = api()
    d = device_case(C, Tx, Ty)
    new = lambda *s: torch.empty(*s, dtype=F32, device=dev())       # noqa: E731
    n = B * C * Ty
    z_m, z_logs = new(B, C, Ty), (new(B, C, Ty) if with_logs else None)
    call.gt_prior_expand(d["x_m"], d["f2t"], z_m, B, C, Tx, Ty, st)
    if with_logs:
        call.gt_prior_expand(d["x_logs"], d["f2t"], z_logs, B, C, Tx, Ty, st)
    acc = new(2 * L64.header_constant("GT_MLE_PARTS"))
    call.gt_mle_sums(d["z"], z_m, z_logs, acc, n, st)
    out2 = new(2)
    call.gt_mle_finish(acc, d["logdet"], d["mask"], d["mask"].numel(), B, C, out2, st)
    l_length = new(B)
    call.gt_duration_loss_fwd(d["logw"], d["w"], d["x_len"], B, Tx, l_length, st)
    s = torch.sum(l_length)
    total = out2[0] + s
    gs = torch.tensor([gscale], dtype=F32, device=dev())
    dz, dm, dlogs, dlogdet = new(B, C, Ty), new(B, C, Ty), (new(B, C, Ty) if with_logs else None), new(B)
    call.gt_mle_bwd(d["z"], z_m, z_logs, gs, dz, dm, dlogs, n, out2[1:].data_ptr(), dlogdet, B, st)
    dx_m, dx_logs = new(B, C, Tx), (new(B, C, Tx) if with_logs else None)
    call.gt_prior_expand_bwd(dm, d["f2t"], dx_m, B, C, Tx, Ty, st)
    if with_logs:
        call.gt_prior_expand_bwd(dlogs, d["f2t"], dx_logs, B, C, Tx, Ty, st)
    dlogw = new(B, Tx)
    call.gt_duration_loss_bwd(d["logw"], d["w"], d["x_len"], gs.expand(B).contiguous(), B, Tx, dlogw, st)
    torch.cuda.synchronize()
    return dict(z_m=z_m, z_logs=z_logs, acc=acc, out2=out2, l_length=l_length, sum=s, total=total, gs=gs, dz=dz, dx_m=dx_m, dx_logs=dx_logs,
                dlogdet=dlogdet, dlogw=dlogw)


def fused_forward(G, d, C, Tx, Ty, with_logs, with_dur):
    call, st, _ = api()
    z_m = G.out("z_m", (B, C, Ty))
    z_logs = G.out("z_logs", (B, C, Ty)) if with_logs else None
    acc = G.out("acc2", (2 * L64.header_constant("GT_MLE_PARTS"),))
    l_length = G.out("l_length", (B,)) if with_dur else None
    call.gt_align_loss_fwd(G.inp(d["z"]), G.inp(d["x_m"]), G.inp(d["x_logs"]) if with_logs else None, G.inp(d["f2t"], fill=0),
                           G.inp(d["logw"]) if with_dur else None, G.inp(d["w"]) if with_dur else None,
                           G.inp(d["x_len"], fill=1) if with_dur else None, z_m, z_logs, acc, l_length, B, C, Tx, Ty, st)
    out4 = G.out("out4", (4,))
    call.gt_align_loss_finish(acc, G.inp(d["logdet"]), G.inp(d["mask"]), d["mask"].numel(), l_length, B, C, out4, st)
    G.verify()
    return z_m, z_logs, acc, l_length, out4


# ----------------------------------------------------------------------------- A + B: bit-equality and float64
@pytest.mark.parametrize("with_dur", [True, False])
@pytest.mark.parametrize("with_logs", [False, True])
@pytest.mark.parametrize("Tx,Ty", SHAPES)
@pytest.mark.parametrize("C", CS)
def test_forward_and_finish_equal_the_unfused_chain_in_bits(built, C, Tx, Ty, with_logs, with_dur):
    h, ref = case(C, Tx, Ty), unfused(C, Tx, Ty, with_logs, 1.0)
    z_m, z_logs, acc, l_length, out4 = fused_forward(Guards(dev()), h, C, Tx, Ty, with_logs, with_dur)
    tag = f"C={C} {Tx}x{Ty} x_logs={'set' if with_logs else 'NULL'} duration={'on' if with_dur else 'off'}"
    bits_equal(f"z_m {tag}", z_m, ref["z_m"])
    if with_logs:
        bits_equal(f"z_logs {tag}", z_logs, ref["z_logs"])
    bits_equal(f"partial pairs {tag}", acc, ref["acc"])
    bits_equal(f"out4[0:2] (mle loss, denominator) {tag}", out4[:2], ref["out2"])
    if with_dur:
        bits_equal(f"l_length {tag}", l_length, ref["l_length"])
        bits_equal(f"out4[2] against torch.sum(l_length) {tag}", out4[2:3], ref["sum"].reshape(1))
        bits_equal(f"out4[3] against mle + torch.sum(l_length) {tag}", out4[3:4], ref["total"].reshape(1))
    else:
        assert float(out4[2]) == 0.0
        bits_equal(f"out4[3] = out4[0] {tag}", out4[3:4], ref["out2"][:1])
    # float64, with the bounds of the unfused kernels
    lg = h["x_logs"] if with_logs else None
    zm64 = L64.prior_expand(h["x_m"], h["f2t"])
    assert bool((z_m.cpu().double() == zm64).all())
    zl64 = L64.prior_expand(lg, h["f2t"]) if with_logs else None
    loss, denom, bound = L64.mle(h["z"], zm64, zl64, h["logdet"], h["mask"], C)
    rule(f"out4[0] against float64 {tag}", out4[:1], loss, bound)
    assert float(out4[1]) == float(denom)
    if with_dur:
        r64, twin = L64.duration_loss(h["logw"], h["w"], h["x_len"]), L64.duration_loss(h["logw"], h["w"], h["x_len"], dtype=F32)
        ek, et = LC.rel_l2(l_length.cpu(), r64), LC.rel_l2(twin, r64)
        print(f"l_length {tag}: err_kernel {ek:.3e} err_twin {et:.3e}")
        assert ek <= max(LC.DUR_M["fwd"] * et, 2.0 ** -23)
        s64 = r64.sum()
        assert abs(float(out4[2]) - float(s64)) <= (max(LC.DUR_M["fwd"] * et, 2.0 ** -23) * B ** 0.5 + gamma(B)) * float(r64.abs().sum()) + 1e-300


@pytest.mark.parametrize("n", SUM_BS + [200])
def test_finish_sums_l_length_in_the_order_of_torch_sum(built, n):
    call, st, _ = api()
    g = torch.Generator().manual_seed(n)
    G = Guards(dev())
    acc = G.inp(torch.zeros(2 * L64.header_constant("GT_MLE_PARTS")))
    logdet, mask = G.inp(torch.randn(n, generator=g)), G.inp(torch.ones(n, 1, 8))
    for trial in range(4):
        host = torch.rand(n, generator=g) * 3 + 0.01
        ll = G.inp(host)
        out4 = G.out("out4", (4,))
        call.gt_align_loss_finish(acc, logdet, mask, mask.numel(), ll, n, 2, out4, st)
        G.verify()
        G.outs.clear()
        if n < 128:
            want = torch.sum(ll).reshape(1)
        else:                      # past ATen's short-vector form: the order the header documents, restated on the host in fp32
            v = [np.float32(0)] * 64
            for i, x in enumerate(host.numpy()):
                v[i % 64] = np.float32(v[i % 64] + x)
            off = 1
            while off < 64:
                v = [np.float32(v[t] + v[t + off]) if t + off < 64 else v[t] for t in range(64)]
                off <<= 1
            want = torch.tensor([v[0]])
        bits_equal(f"out4[2] B={n} trial {trial}", out4[2:3], want)
        bits_equal(f"out4[3] B={n} trial {trial}", out4[3:4], (out4[0] + out4[2]).reshape(1))


# ----------------------------------------------------------------------------- C: bit-equality and float64
@pytest.mark.parametrize("gscale", [1.0, 0.37])
@pytest.mark.parametrize("with_dur", [True, False])
@pytest.mark.parametrize("with_logs", [False, True])
@pytest.mark.parametrize("Tx,Ty", SHAPES)
@pytest.mark.parametrize("C", CS)
def test_backward_equals_the_unfused_chain_in_bits(built, C, Tx, Ty, with_logs, with_dur, gscale):
    call, st, _ = api()
    h, ref = case(C, Tx, Ty), unfused(C, Tx, Ty, with_logs, gscale)
    G = Guards(dev())
    outs = dict(dz=G.out("dz", (B, C, Ty)), dx_m=G.out("dx_m", (B, C, Tx)), dlogdet=G.out("dlogdet", (B,)))
    if with_logs:
        outs["dx_logs"] = G.out("dx_logs", (B, C, Tx))
    if with_dur:
        outs["dlogw"] = G.out("dlogw", (B, Tx))
    gs, gd = G.inp(torch.tensor([gscale])), G.inp(ref["out2"][1:].cpu())
    call.gt_align_loss_bwd(G.inp(h["z"]), G.inp(ref["z_m"].cpu()), G.inp(ref["z_logs"].cpu()) if with_logs else None, G.inp(h["f2t"], fill=0),
                           G.inp(h["logw"]) if with_dur else None, G.inp(h["w"]) if with_dur else None,
                           G.inp(h["x_len"], fill=1) if with_dur else None, gs, gd, outs["dz"], outs["dx_m"], outs.get("dx_logs"),
                           outs["dlogdet"], outs.get("dlogw"), B, C, Tx, Ty, st)
    G.verify()
    tag = f"C={C} {Tx}x{Ty} x_logs={'set' if with_logs else 'NULL'} duration={'on' if with_dur else 'off'} gscale={gscale}"
    for k, got in outs.items():
        bits_equal(f"{k} {tag}", got, ref[k])
    # float64: gt_mle_bwd's elementwise bounds, carried through gt_prior_expand_bwd's segment sums (gamma(run) on the |.| twin)
    zl = ref["z_logs"].cpu() if with_logs else None
    m64 = L64.mle_bwd(h["z"], ref["z_m"].cpu(), zl, torch.tensor([gscale]), ref["out2"][1:].cpu(), B)
    shp = (B, C, Ty)
    rule(f"dz against float64 {tag}", outs["dz"], m64["dz"][0].reshape(shp), m64["dz"][1].reshape(shp))
    rule(f"dlogdet against float64 {tag}", outs["dlogdet"], *m64["dlogdet"])
    for k, src in (("dx_m", "dm"), ("dx_logs", "dlogs")):
        if k in outs:
            r, bnd = m64[src][0].reshape(shp), m64[src][1].reshape(shp)
            seg, S, run = L64.prior_expand_bwd(r, h["f2t"], Tx)
            e_in = L64.prior_expand_bwd(bnd, h["f2t"], Tx)[0]                # the operands' own errors, summed over the run
            rule(f"{k} against float64 {tag}", outs[k], seg, gamma(run.double())[:, None, :] * (S + e_in) + e_in)
            assert bool((outs[k].cpu()[(run == 0)[:, None, :].expand(-1, C, -1)] == 0).all())      # tokens without a frame
    if with_dur:
        g = torch.full((B,), gscale)
        r64, twin = L64.duration_loss_bwd(h["logw"], h["w"], h["x_len"], g), L64.duration_loss_bwd(h["logw"], h["w"], h["x_len"], g, dtype=F32)
        ek, et = LC.rel_l2(outs["dlogw"].cpu(), r64), LC.rel_l2(twin, r64)
        print(f"dlogw {tag}: err_kernel {ek:.3e} err_twin {et:.3e}")
        assert ek <= max(LC.DUR_M["bwd"] * et, 2.0 ** -23)


# ----------------------------------------------------------------------------- refusals
def test_refusals_return_their_status_and_write_nothing(built):
    _, st, _lib = api()
    L = _lib.lib()
    C, Tx, Ty = 6, 7, 32
    parts = L64.header_constant("GT_MLE_PARTS")
    p = lambda t: None if t is None else _lib.ptr(t)      # noqa: E731

    def fwd(Tx=Tx, Ty=Ty, shift=None, null=None, dur=True):
        Txa = min(Tx, 600)
        t = dict(z=torch.randn(B * C * Ty + 4), x_m=torch.randn(B, C, Txa), x_logs=torch.randn(B, C, Txa),
                 f2t=torch.zeros(B * Ty + 4, dtype=torch.int32), logw=torch.zeros(B, Txa), w=torch.ones(B, Txa),
                 x_len=torch.ones(B, dtype=torch.int32))
        t = {k: v.to(dev()) for k, v in t.items()}
        o = dict(z_m=torch.full((B * C * Ty + 4,), CAN), z_logs=torch.full((B * C * Ty + 4,), CAN), acc=torch.full((2 * parts + 4,), CAN),
                 l_length=torch.full((B,), CAN))
        o = {k: v.to(dev()) for k, v in o.items()}
        a = {**t, **o}
        if shift:
            a[shift] = a[shift][1:]                                         # 4 bytes off the 16-byte boundary
        if not dur:
            a["logw"] = a["w"] = a["x_len"] = a["l_length"] = None
        for k in (null or ()):
            a[k] = None
        rc = L.gt_align_loss_fwd(p(a["z"]), p(a["x_m"]), p(a["x_logs"]), p(a["f2t"]), p(a["logw"]), p(a["w"]), p(a["x_len"]), p(a["z_m"]),
                                 p(a["z_logs"]), p(a["acc"]), p(a["l_length"]), B, C, Tx, Ty, st)
        torch.cuda.synchronize()
        for k, v in o.items():
            assert bool((v == CAN).all()), f"{k} was written by a refused call"
        return rc

    assert fwd(Ty=30) == GT_E_ALIGN
    for k in ("z", "z_m", "z_logs", "f2t"):
        assert fwd(shift=k) == GT_E_ALIGN, k
    assert fwd(Tx=513) == GT_E_UNSUPPORTED
    for k in ("z", "x_m", "f2t", "z_m", "acc"):
        assert fwd(null=[k]) == GT_E_INVAL, k
    assert fwd(null=["z_logs"]) == GT_E_INVAL                  # x_logs without z_logs
    for k in ("w", "logw", "x_len", "l_length"):
        assert fwd(null=[k]) == GT_E_INVAL, k                  # the duration part: logw and w together, with lengths and an output

    def bwd(Tx=Tx, null=None):
        Txa = min(Tx, 600)
        t = dict(z=torch.randn(B, C, Ty), z_m=torch.randn(B, C, Ty), z_logs=torch.randn(B, C, Ty), f2t=torch.zeros(B, Ty, dtype=torch.int32),
                 logw=torch.zeros(B, Txa), w=torch.ones(B, Txa), x_len=torch.ones(B, dtype=torch.int32), gs=torch.ones(1), gd=torch.ones(1))
        t = {k: v.to(dev()) for k, v in t.items()}
        o = dict(dz=torch.full((B, C, Ty), CAN), dx_m=torch.full((B, C, Txa), CAN), dx_logs=torch.full((B, C, Txa), CAN),
                 dlogdet=torch.full((B,), CAN), dlogw=torch.full((B, Txa), CAN))
        o = {k: v.to(dev()) for k, v in o.items()}
        a = {**t, **o}
        for k in (null or ()):
            a[k] = None
        rc = L.gt_align_loss_bwd(p(a["z"]), p(a["z_m"]), p(a["z_logs"]), p(a["f2t"]), p(a["logw"]), p(a["w"]), p(a["x_len"]), p(a["gs"]),
                                 p(a["gd"]), p(a["dz"]), p(a["dx_m"]), p(a["dx_logs"]), p(a["dlogdet"]), p(a["dlogw"]), B, C, Tx, Ty, st)
        torch.cuda.synchronize()
        for k, v in o.items():
            assert bool((v == CAN).all()), f"{k} was written by a refused call"
        return rc

    assert bwd(Tx=513) == GT_E_UNSUPPORTED
    for k in ("z", "z_m", "f2t", "gs", "gd", "dz", "dx_m", "dlogdet", "dx_logs", "w", "dlogw"):
        assert bwd(null=[k]) == GT_E_INVAL, k
    out4 = torch.full((4,), CAN, device=dev())
    one = torch.ones(4, device=dev())
    for a in ((None, one, one), (one, None, one), (one, one, None)):
        assert L.gt_align_loss_finish(p(a[0]), p(a[1]), p(a[2]), 4, None, 2, 2, p(out4), st) == GT_E_INVAL
    assert L.gt_align_loss_finish(p(one), p(one), p(one), 4, None, 2, 2, None, st) == GT_E_INVAL
    torch.cuda.synchronize()
    assert bool((out4 == CAN).all())


# ----------------------------------------------------------------------------- the model: one eager Trainer step, switch on / off
def test_trainer_step_with_the_fused_chain_equals_the_step_without(built):
    """Same seed, same batch, one eager step each, fused_align_loss off, off again and on.  loss and l_mle are bit-equal, and so is
    the gradient of every parameter that is NOT accumulated with float atomics (train.GradBuckets' accumulated parameters:
    LayerNorm / ActNorm / InvConvNear / Embedding and the relative-position tables) — text encoder, duration predictor and decoder
    alike.  The atomically accumulated ones differ between two switch-OFF steps already (measured on an MI355X: encoder.emb.weight
    in 228 of 28 416 elements, the attention's emb_rel_k / emb_rel_v in 374 / 376 of 864, LayerNorm gammas in 13 - 69 of 256, every
    difference one or two ulp of the element), and grad_norm, which sums them, by 5 ulp: no step can be bit-equal to a reference that
    is not bit-equal to itself.  Those are held to the rule for float atomics: per parameter r(a, b) = max |a - b| / max |b|; the noise
    is the largest r(off, off) over these parameters, but at least 2^-23 (one reordered float atomic moves a sum by an ulp: a pair of
    steps that happens to agree measures no noise, not a noise of zero); every r(on, off) must stay within 4 x the noise.
    grad_norm is the root of a sum of squares that gt_adamw_flat accumulates with one same-address float atomic per workgroup, at
    most 1 024 per launch and two launches per step, in whatever order they arrive: K = 2 048 roundings of at most half an ulp of the
    sum that add up like a random walk, sqrt(K) 2^-25 relative on the sum, half that on its root (9 ulp here; four repetitions on an
    MI355X spread over 7 ulp, and two of the four switch-off pairs agreed exactly).  |grad_norm(on) - grad_norm(off)| must stay
    within 4 x max(|grad_norm(off) - grad_norm(off')|, sqrt(K) 2^-26 grad_norm) — 3e-6 relative."""
    from glow_tts_amd import _lib, train
    cfg = dict(train.BASE_MODEL, n_blocks_dec=2, n_layers_enc=1, p_dropout=0.0, p_dropout_dec=0.0)
    batch = train.synth_batch(4, 40, 120, 0, dev())

    def step(fused):
        torch.manual_seed(0)
        m = train.build_model(cfg, device=dev())
        with torch.no_grad():
            for n, p in m.named_parameters():
                if n.endswith("end.weight") or n.endswith("pre.proj.weight"):
                    p.normal_(0, 0.02)
        m.encoder.pre.p_dropout = 0.0
        tr = train.Trainer(m, graph=False, fused_align_loss=fused)
        with _lib.record_calls() as names:
            loss, l_mle = tr.step(*batch)
        torch.cuda.synchronize()
        atomic = {id(p) for p in tr.buckets.params[:tr.buckets.n_accum]}
        grads = {n: p.grad.detach().clone() for n, p in m.named_parameters() if p.grad is not None}
        return loss.clone(), l_mle.clone(), tr.grad_norm.clone(), grads, names, {n for n, p in m.named_parameters() if id(p) in atomic}

    off1, off2, on = step(False), step(False), step(True)
    assert "gt_align_loss_fwd" in on[4] and "gt_align_loss_bwd" in on[4] and "gt_mle_sums" not in on[4] and "gt_prior_expand" not in on[4]
    assert "gt_mas_f32" in on[4] and "gt_align_loss_fwd" not in off1[4] and "gt_mle_sums" in off1[4]
    bits_equal("loss", on[0].reshape(1), off1[0].reshape(1))
    bits_equal("l_mle", on[1].reshape(1), off1[1].reshape(1))
    atomic = off1[5]
    assert set(on[3]) == set(off1[3]) and any(not n.startswith("decoder.") for n in atomic)
    plain = [n for n in off1[3] if n not in atomic]
    assert sum(not n.startswith("decoder.") for n in plain) >= 20 and any(n.startswith("decoder.") for n in plain)
    for n in plain:
        bits_equal(f"grad {n}", on[3][n], off1[3][n])

    def r(a, b):
        return (a - b).abs().max().item() / max(b.abs().max().item(), 1e-30)
    noisy = [n for n in off1[3] if n in atomic]
    noise = max(max(r(off1[3][n], off2[3][n]) for n in noisy), 2.0 ** -23)
    for n in noisy:
        got = r(on[3][n], off1[3][n])
        print(f"grad {n} (float atomics): off / off {r(off1[3][n], off2[3][n]):.3e}, on / off {got:.3e}, limit {4 * noise:.3e}")
        assert got <= 4 * noise, n
    gn = [t[2].item() for t in (off1, off2, on)]
    floor = 2048 ** 0.5 * 2.0 ** -26 * gn[0]
    print(f"grad_norm: off {gn[0]!r}, off again {gn[1]!r}, on {gn[2]!r} (one ulp {float(np.spacing(np.float32(gn[0]))):.3e}, floor {floor:.3e})")
    assert abs(gn[2] - gn[0]) <= 4 * max(abs(gn[1] - gn[0]), floor)
