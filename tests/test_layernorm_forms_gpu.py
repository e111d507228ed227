"""Every instantiation the LayerNorm entries dispatch to (csrc/encoder_ops.hip: which of a / y and, backward, of dout_f32 / dout_bf16
exist is a template parameter), at row counts around the workgroup geometries: R = 1, 15, 17 (one row short of / past the 16 rows of
a backward workgroup, so the clamped loads of rows past the end are live), 70 (five workgroups, the last one partial); C = 192 and 100
(lanes whose second to fourth channel slots are partly or wholly off read a clamped channel).  Below 2048 rows both backward entries
run the 4-wave x 4-row kernels; R = 2085 (C = 192; no multiple of the 32 rows of a workgroup) takes gt_layernorm_bwd to its 16-wave x
2-row kernels, all nine of them, against the 4 x 4 kernels of gt_layernorm_bwd_partials.

  * forward and both backward forms against float64 on their own operands (the rule of oracle/rows64.py with the bounds of
    oracle/ln64.py; at R = 70 ln64.check_case with its planted defects as well);
  * da / dy of gt_layernorm_bwd and of gt_layernorm_bwd_partials are bit-equal;
  * the column sums of the partial rows agree with what the atomics form added to a zero dgamma / dbeta within the sum of the two
    forms' bounds against their common float64 reference (ln64.backward with each form's number of additions);
  * every output lives in one arena of canary bytes and only the requested ones are passed: afterwards the arena differs from its
    initial state in the requested [R, C] windows ONLY (not in the window's pitch padding, not in the outputs left out).

rowmask is absent at R = 1 and 17 (the kernels then read gamma in its place and discard it), ln64.make_case's at 15 and 70; the seed
word is on the device where dropout is on (the a + y forms)."""
import ctypes

import pytest
import torch

from oracle import dropmask, ln64, rows64

pytestmark = pytest.mark.gpu

EPS, PAD, FILL = 1e-4, 8, 0xA5
SEED_IN, SEED_OUT, WORD = 1234, 4321, 0x0BADC0DE
# what is requested, by the form of dout: forward (out_f32, out_bf16), backward (da, dy) where the operand exists
WANT = {"f32": ((True, False), (True, False)), "bf16": ((False, True), (False, True)), "both": ((True, True), (True, True))}


def dev():
    return torch.device("cuda:0")


class Arena:
    """Outputs carved out of one buffer of FILL bytes, at least 256 bytes apart."""

    def __init__(self, nbytes):
        self.buf = torch.full((nbytes,), FILL, dtype=torch.uint8, device=dev())
        self.off = 256

    def take(self, rows, cols, dtype, pad):
        ld = cols + 2 * pad
        n = rows * ld * torch.empty((), dtype=dtype).element_size()
        flat = self.buf[self.off:self.off + n].view(dtype).view(rows, ld)
        assert self.off + n + 256 <= self.buf.numel()
        self.off += (n + 511) // 256 * 256
        v = flat[:, pad:pad + cols]
        return v

    def only_requested_written(self, requested):
        got = self.buf.clone()
        kept = [v.clone() for v in requested]
        self.buf.fill_(FILL)                                           # the initial bytes, with the requested windows as they are now
        for v, k in zip(requested, kept):
            v.copy_(k)
        return torch.equal(self.buf, got)


def _case(R_, C, fwd, dout):
    c = ln64.make_case(R_, C, "a+y", seed=3)
    if fwd == "a":
        c.y, c.p_in = None, 0.0
    if fwd == "y":
        c.a, c.p_in = None, 0.0
    if dout == "f32":
        c.dout_bf16 = None
    if dout == "bf16":
        c.dout_f32, c.p_out = None, 0.5
    if R_ in (1, 17):
        c.rowmask = None
    c.prior_gamma, c.prior_beta = torch.zeros(C), torch.zeros(C)
    return c


def _rule(tag, c, got):
    """The rule of oracle/rows64.py on every output present, with ln64's float64 restatement and bounds; returns ln64.backward's result.
    No planted defect here: ln64.check_case's defects (one channel left out of the mean, ...) move a bf16 dy of one to seventeen rows
    by less than the 3x its controls ask for, so the cases at R = 70 run check_case as well and the smaller ones only the rule."""
    R_, C = (c.a if c.a is not None else c.y).shape
    ki, si = ln64._keep(c.p_in, c.seed_in, R_, C)
    ko, so = ln64._keep(c.p_out, c.seed_out, R_, C)
    kw = dict(keep_in=ki, scale_in=si, keep_out=ko, scale_out=so, relu=0)
    f = ln64.forward(c.a, c.y, c.gamma, c.beta, c.rowmask, c.eps, **kw)
    g = ln64.backward(c.a, c.y, c.gamma, c.beta, c.rowmask, got["mean"], got["rstd"], c.dout_f32, c.dout_bf16, c.K_param, c.prior_gamma,
                      c.prior_beta, **kw)
    for name, (ref, bound), kind in (("mean", f["mean"], "f32"), ("rstd", f["rstd"], "f32"), ("out_f32", f["out"], "f32"),
                                     ("out_bf16", f["out"], "bf16"), ("da", g["da"], "f32"), ("dy", g["dy"], "bf16"),
                                     ("dgamma", g["dgamma"], "f32"), ("dbeta", g["dbeta"], "f32")):
        if got.get(name) is not None:
            r = rows64.check(f"{tag} {name}", got[name], ref, bound, kind)
            print(r)
            assert r.ok, str(r)
    return g


@pytest.mark.parametrize("dout", ["f32", "bf16", "both"])
@pytest.mark.parametrize("fwd", ["a", "y", "a+y"])
@pytest.mark.parametrize("R_,C", [(r, c) for c in (192, 100) for r in (1, 15, 17, 70)] + [(2085, 192)])
def test_layernorm_forms(built, R_, C, fwd, dout):
    from glow_tts_amd import _lib
    L = _lib.lib()
    c = _case(R_, C, fwd, dout)
    word = c.p_in > 0
    c.seed_in, c.seed_out = (dropmask.word_seed(WORD, s) if word else s for s in (SEED_IN, SEED_OUT))
    tag = f"LN forms {fwd} / dout {dout} R={R_} C={C}"
    P, st = _lib.ptr, _lib.current_stream(dev())
    on = lambda t: None if t is None else t.to(dev())                 # noqa: E731
    ld = lambda t: 0 if t is None else t.stride(0)                    # noqa: E731
    a, gam, beta, rm, do32 = on(c.a), on(c.gamma), on(c.beta), on(c.rowmask), on(c.dout_f32)

    def window(t):                                                    # inputs as windows too (ldy, lddo > C)
        if t is None:
            return None
        buf = torch.zeros(t.shape[0], t.shape[1] + 3 * PAD, dtype=t.dtype, device=dev())
        buf[:, PAD:PAD + t.shape[1]] = t.to(dev())
        return buf[:, PAD:PAD + t.shape[1]]
    y, do16 = window(c.y), window(c.dout_bf16)
    wd = torch.tensor([WORD], dtype=torch.int32, device=dev()) if word else None
    (want32, want16), (want_da, want_dy) = WANT[dout]
    want_da, want_dy = (want_da or y is None) and a is not None, (want_dy or a is None) and y is not None
    n_part = L.gt_layernorm_bwd_partial_rows(R_)
    assert n_part == -(-R_ // 16)

    ar = Arena(1 << 20 if R_ <= 70 else 16 << 20)
    f32, bf = torch.float32, torch.bfloat16
    o32, o16 = ar.take(R_, C, f32, 0), ar.take(R_, C, bf, PAD)         # fp32 rows are dense (pitch C) in the C-ABI, bf16 rows pitched
    mean, rstd = ar.take(1, R_, f32, 0)[0], ar.take(1, R_, f32, 0)[0]
    da = {k: ar.take(R_, C, f32, 0) for k in ("atomics", "partials")}
    dy = {k: ar.take(R_, C, bf, PAD) for k in ("atomics", "partials")}
    part = ar.take(n_part, 2 * C, f32, 0)
    req = [mean, rstd, part] + [o32] * want32 + [o16] * want16 + [da[k] for k in da if want_da] + [dy[k] for k in dy if want_dy]
    sel = lambda want, t: t if want else None                         # noqa: E731

    _lib.check(L.gt_layernorm_fwd(P(a), P(y), ld(y), P(gam), P(beta), P(rm), P(sel(want32, o32)), P(sel(want16, o16)), ld(o16), P(mean), P(rstd),
                                  R_, C, EPS, c.p_in, SEED_IN, c.p_out, SEED_OUT, 0, P(wd), st), "gt_layernorm_fwd")
    dg, db = {k: torch.zeros(C, device=dev()) for k in da}, {k: torch.zeros(C, device=dev()) for k in da}
    for k in da:
        head = (P(a), P(y), ld(y), P(gam), P(beta), P(rm), P(mean), P(rstd), R_, C, EPS, c.p_in, SEED_IN, c.p_out, SEED_OUT, 0, P(wd),
                P(do32), P(do16), ld(do16), P(sel(want_da, da[k])), P(sel(want_dy, dy[k])), ld(dy[k]))
        if k == "atomics":
            _lib.check(L.gt_layernorm_bwd(*head, P(dg[k]), P(db[k]), st), "gt_layernorm_bwd")
        else:
            _lib.check(L.gt_layernorm_bwd_partials(*head, P(part), st), "gt_layernorm_bwd_partials")
            args = _lib.PartialsArgs()
            j = args.job[0]
            j.partials, j.dst_a, j.dst_b, j.n_rows, j.Ca, j.Cb = part.data_ptr(), dg[k].data_ptr(), db[k].data_ptr(), n_part, C, C
            args.n_jobs = 1
            _lib.check(L.gt_param_partials_reduce(ctypes.byref(args), st), "gt_param_partials_reduce")
    torch.cuda.synchronize()

    cpu = lambda want, t: t.cpu().contiguous() if want else None      # noqa: E731
    fw = {"mean": mean.cpu(), "rstd": rstd.cpu(), "out_f32": cpu(want32, o32), "out_bf16": cpu(want16, o16)}
    bounds = {}
    for k in da:
        c.K_param = ln64.param_terms(R_, k, n_rows=n_part)
        got = {**fw, "da": cpu(want_da, da[k]), "dy": cpu(want_dy, dy[k]), "dgamma": dg[k].cpu(), "dbeta": db[k].cpu()}
        g = _rule(f"{tag} {k}", c, got)
        bounds[k] = (g["dgamma"], g["dbeta"])
        if R_ == 70:                                                   # with the planted defects as well (see _rule)
            rep, share = ln64.check_case(f"{tag} {k}", c, got)
            assert {"mean", "rstd", "dgamma", "dbeta"} <= set(rep) and share == 0.0

    # the two forms' element gradients are the same bits
    if want_da:
        assert torch.equal(da["atomics"].view(torch.int32), da["partials"].view(torch.int32)), f"{tag}: da differs between the forms"
    if want_dy:
        assert torch.equal(dy["atomics"].contiguous().view(torch.int16), dy["partials"].contiguous().view(torch.int16)), f"{tag}: dy differs"
    # the partial rows' column sums (exact, in float64) against the atomics form's result
    cols = rows64.t64(part.cpu()).sum(0)
    for i, (name, got) in enumerate((("dgamma", dg["atomics"]), ("dbeta", db["atomics"]))):
        bound = bounds["atomics"][i][1] + bounds["partials"][i][1]
        r = rows64.check(f"{tag} {name}: atomics form vs column sums of the partial rows", got.cpu(), cols[i * C:(i + 1) * C], bound)
        print(r)
        assert r.worst <= 1.0, str(r)
    assert ar.only_requested_written(req), f"{tag}: bytes outside the requested outputs were written"
