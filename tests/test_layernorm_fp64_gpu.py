"""gt_layernorm_fwd, gt_layernorm_bwd (atomics), gt_layernorm_bwd_partials + gt_param_partials_reduce through the C-ABI against
float64 on their own operands, under the rule of oracle/rows64.py with the restatement and the derived bounds of oracle/ln64.py.

C in {192, 256, 100} (at C = 100 the lanes' second to fourth slots are partly or wholly off); R = 70 takes the 4-wave 16-row form of the
atomics backward and is no multiple of 16, R = 2085 >= 2048 the 16-wave 32-row form and is no multiple of 32; rowmask has zero rows
at both ends and in the middle.  The operand forms are the product's (ln64.make_case): a only; bf16 y only, as a window with
ldy > C; a + y with p_in = 0.1 and a seed word on the device; relu = 1 with p_out = 0.5; relu = 2 with exact +0 / -0 entries in y;
out_f32, out_bf16 or both; dout_f32, dout_bf16 or both.  Both backward forms are checked against the same float64 reference; the
reduce launch carries three jobs (n_rows = gt_layernorm_bwd_partial_rows(R) — 131 or 5 —, 1 with Cb = 0, and 5)."""
import ctypes

import pytest
import torch

from oracle import dropmask, ln64, rows64

pytestmark = pytest.mark.gpu

EPS, CANARY, PAD = 1e-4, 768.0, 8
SEED_IN, SEED_OUT, WORD = 1234, 4321, 0x0BADC0DE
OUTS = {"a": (True, False), "y": (False, True), "a+y": (True, True), "relu1": (True, True), "relu2": (False, True)}


def dev():
    return torch.device("cuda:0")


def _window(t, fill=CANARY):
    """[R, C] -> a window (ld = C + 3 PAD) of a canary-filled buffer; returns (buffer, window)"""
    buf = torch.full((t.shape[0], t.shape[1] + 3 * PAD), fill, dtype=t.dtype, device=dev())
    buf[:, PAD:PAD + t.shape[1]] = t.to(dev())
    return buf, buf[:, PAD:PAD + t.shape[1]]


def _outside_intact(buf, C):
    return bool((buf[:, :PAD].float() == CANARY).all()) and bool((buf[:, PAD + C:].float() == CANARY).all())


@pytest.mark.parametrize("form", ["a", "y", "a+y", "relu1", "relu2"])
@pytest.mark.parametrize("R_,C", [(70, 192), (70, 256), (70, 100), (2085, 192), (2085, 256), (2085, 100)])
def test_layernorm_vs_float64(built, R_, C, form):
    from glow_tts_amd import _lib
    L = _lib.lib()
    c = ln64.make_case(R_, C, form, seed=1)
    word = form == "a+y"
    c.seed_in, c.seed_out = (dropmask.word_seed(WORD, s) if word else s for s in (SEED_IN, SEED_OUT))   # the kernel XORs the word in
    tag = f"LN {form} R={R_} C={C}"
    P, st = _lib.ptr, _lib.current_stream(dev())
    on = lambda t: None if t is None else t.to(dev())                 # noqa: E731
    a, gam, beta, rm = on(c.a), on(c.gamma), on(c.beta), on(c.rowmask)
    ybuf, y = (None, None) if c.y is None else _window(c.y)
    do32 = on(c.dout_f32)
    dobuf, do16 = (None, None) if c.dout_bf16 is None else _window(c.dout_bf16)
    want32, want16 = OUTS[form]
    o32 = torch.full((R_, C), float("nan"), device=dev()) if want32 else None
    o16buf, o16 = _window(torch.zeros(R_, C, dtype=torch.bfloat16)) if want16 else (None, None)
    mean, rstd = torch.full((R_,), float("nan"), device=dev()), torch.full((R_,), float("nan"), device=dev())
    wd = torch.tensor([WORD], dtype=torch.int32, device=dev()) if word else None
    ld = lambda t: 0 if t is None else t.stride(0)                    # noqa: E731
    _lib.check(L.gt_layernorm_fwd(P(a), P(y), ld(y), P(gam), P(beta), P(rm), P(o32), P(o16), ld(o16), P(mean), P(rstd), R_, C, EPS,
                                  c.p_in, SEED_IN, c.p_out, SEED_OUT, c.relu & 1, P(wd), st), "gt_layernorm_fwd")

    def backward(partials):
        da = torch.full((R_, C), float("nan"), device=dev()) if a is not None else None
        dybuf, dy = _window(torch.zeros(R_, C, dtype=torch.bfloat16)) if y is not None else (None, None)
        dg, db = on(c.prior_gamma).clone(), on(c.prior_beta).clone()
        head = (P(a), P(y), ld(y), P(gam), P(beta), P(rm), P(mean), P(rstd), R_, C, EPS, c.p_in, SEED_IN, c.p_out, SEED_OUT, c.relu, P(wd),
                P(do32), P(do16), ld(do16), P(da), P(dy), ld(dy))
        extra = None
        if not partials:
            _lib.check(L.gt_layernorm_bwd(*head, P(dg), P(db), st), "gt_layernorm_bwd")
        else:
            n = L.gt_layernorm_bwd_partial_rows(R_)
            assert n == -(-R_ // 16)
            part = torch.full((n, 2 * C), float("nan"), device=dev())
            _lib.check(L.gt_layernorm_bwd_partials(*head, P(part), st), "gt_layernorm_bwd_partials")
            # two more jobs of the same launch: one row with Cb = 0, five rows with odd widths
            g = torch.Generator().manual_seed(R_ + C)
            p1, p5 = torch.randn(1, C, generator=g).to(dev()), torch.randn(5, 7 + 3, generator=g).to(dev())
            d1, d5a, d5b = (torch.randn(k, generator=g).to(dev()) for k in (C, 7, 3))
            extra = [(p1.cpu(), d1.cpu().clone(), d1), (p5[:, :7].cpu(), d5a.cpu().clone(), d5a), (p5[:, 7:].cpu(), d5b.cpu().clone(), d5b)]
            args = _lib.PartialsArgs()
            for i, (pp, da_, db_, ca, cb) in enumerate([(part, dg, db, C, C), (p1, d1, None, C, 0), (p5, d5a, d5b, 7, 3)]):
                j = args.job[i]
                j.partials, j.dst_a, j.dst_b, j.n_rows, j.Ca, j.Cb = pp.data_ptr(), da_.data_ptr(), None if db_ is None else db_.data_ptr(), pp.shape[0], ca, cb
            args.n_jobs = 3
            _lib.check(L.gt_param_partials_reduce(ctypes.byref(args), st), "gt_param_partials_reduce")
        torch.cuda.synchronize()
        if dybuf is not None:
            assert _outside_intact(dybuf, C)
        return {"da": None if da is None else da.cpu(), "dy": None if dy is None else dy.cpu(), "dgamma": dg.cpu(), "dbeta": db.cpu()}, extra

    fwd = {"mean": mean.cpu(), "rstd": rstd.cpu(), "out_f32": None if o32 is None else o32.cpu(), "out_bf16": None if o16 is None else o16.cpu()}
    if o16buf is not None:
        assert _outside_intact(o16buf, C)
    for form_b in ("atomics", "partials"):
        got, extra = backward(form_b == "partials")
        c.K_param = ln64.param_terms(R_, form_b, n_rows=-(-R_ // 16))
        rep, share = ln64.check_case(f"{tag} {form_b}", c, {**fwd, **got})
        assert {"mean", "rstd", "dgamma", "dbeta"} <= set(rep) and share <= 1e-4
    for i, (part, prior, dst) in enumerate(extra):                     # the extra jobs: prior + column sums
        part, prior = rows64.t64(part), rows64.t64(prior)
        n = part.shape[0]
        ref, bound = prior + part.sum(0), rows64.gamma(n + 4 + 1) * (prior.abs() + part.abs().sum(0))
        rows64.check_with_control(f"{tag} reduce job {i} ({n} rows) <row 0 left out>", dst.cpu(), ref, bound, ref - part[0])
