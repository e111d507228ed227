"""GPU parity of the dropout-on (train-mode) path: every kernel form that applies or replays a dropout mask, against the
float oracle (oracle/glowtts_ref.py) handed the EXACT masks the kernels draw, restated on the host by oracle/dropmask.py
(the oracle's sites are pinned to the reference's own modules in train mode by tests/test_train_golden.py).

Each comparison runs the product module in .train() at a fixed `_step` and a known device seed word, and compares at the
tolerances of its eval-mode twin (test_decoder_gpu.py, test_encoder_gpu.py, test_predictors_gpu.py).  Each also carries a
negative control: the oracle with a WRONG mask (the previous step's seed word, or the layer seed shifted by one) must
miss the kernel by at least 3x that tolerance — the test sees a mask error and would not pass with dropout silently off.
The exact-recovery tests read the dropped set off the kernels' own saved tensors and compare it bit for bit."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "golden"))
from fill import fill_module  # noqa: E402
from oracle import dropmask as D  # noqa: E402
from oracle import glowtts_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

WORD = 0x2545F491                   # the device seed word the tests start from (int32-representable)
NEG = 3.0                           # a wrong-mask oracle must miss by this many tolerances


def dev():
    return torch.device("cuda:0")


def relerr(a, b):
    return (a - b).abs().max().item() / max(1e-6, b.abs().max().item())


def grad_ok(a, b, tol, atol=2e-3, name=""):
    """test_encoder_gpu.grad_ok: relative L2 plus a loose max-abs bound; the softmax key bias has a zero gradient."""
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


def set_word(w):
    from glow_tts_amd import ops
    ops.seed_word(dev()).fill_(int(np.int64(w & 0xFFFFFFFF).astype(np.uint32).view(np.int32)))


def prev_word(w=WORD):
    return (w - D.SEED_INC) & 0xFFFFFFFF


def negative(got, wrong_outs, tol, what):
    """the kernel's output against oracle outputs built with wrong masks: each misses by >= NEG * tol"""
    for name, want in wrong_outs.items():
        e = relerr(got, want)
        print(f"  negative control [{what} / {name}]: {e:.3g} (>= {NEG * tol:.3g})")
        assert e >= NEG * tol, (what, name, e)


class Worst:
    """worst relative error per tensor class, printed at the end of a test"""

    def __init__(self, what):
        self.what, self.w = what, {}

    def add(self, cls, name, e):
        if e >= self.w.get(cls, ("", -1.0))[1]:
            self.w[cls] = (name, e)
        return e

    def show(self):
        print(f"{self.what}: " + ", ".join(f"{c} {n} {e:.3g}" for c, (n, e) in self.w.items()))


# ----------------------------------------------------------------------------- WaveNet: every kernel form
def _nbm(R, fwd):
    """32-row (1) or 64-row (2) blocks per tile that the whole-WaveNet launch over R rows takes, forward or backward: the library's
    own choice (gt_wn_stack_row_blocks), so a moved threshold cannot silently move a case out of its band"""
    from glow_tts_amd import _lib
    return _lib.lib().gt_wn_stack_row_blocks(int(R), 4, int(fwd))


# form, cond, ragged, lengths, T
WN_CASES = [
    ("stack", "none", False, [70, 33, 1, 64], 70),
    ("stack", "speaker", True, [131, 70, 2, 1, 64, 97], 131),
    ("stack", "per_row", True, [131, 70, 2, 1, 64, 97], 131),
    ("stack_mixed", "speaker", True, [1400, 1300, 1200, 700], 1400),       # 4 160 < R <= 5 096: forward NBM 1, backward NBM 2
    ("stack_nbm2", "per_row", False, [1500, 1500, 900, 1210], 1500),       # R > 5 096: NBM 2 both ways
    ("layer", "speaker", True, [131, 70, 2, 1, 64, 97], 131),
    ("layer", "per_row", False, [70, 33, 1, 64], 70),
    ("two_kernel", "none", True, [131, 70, 2, 1, 64, 97], 131),
    ("two_kernel", "speaker", False, [70, 33, 1, 64], 70),
    ("two_kernel", "per_row", True, [131, 70, 2, 1, 64, 97], 131),
]


@pytest.mark.parametrize("form,cond_kind,ragged,lens,T", WN_CASES)
def test_wn_train_vs_oracle(built, form, cond_kind, ragged, lens, T):
    """modules.WN / WNP on rows (flow_impl.wn_fwd / wn_bwd) with p = 0.2, against R.wn_fwd with the restated gate masks
    (drop_keep_gate, seed + layer): output, d h0, d cond and every parameter gradient (test_decoder_gpu tolerances 3e-2 /
    3e-2 / 6e-2 / 6e-2).  The conditioning enters the oracle through an identity cond_layer, so speaker (one vector per
    utterance, COND 1) and per-row (WNP's per-frame conditioning, COND 2) are both checked AFTER the mask."""
    from glow_tts_amd import flow_impl, modules, ops, wgrad
    H, n, p, seed = 192, 4, 0.2, 4321
    wn = fill_module(modules.WN(160, H, 5, 1, n, 0, p), "wn.").to(dev())
    if form == "two_kernel":
        wn.set_fused(False)
    if form == "layer":
        wn.set_stack(False, False)
    modules.prepare_all(wn)
    lt = torch.tensor(lens, dtype=torch.int32, device=dev())
    rc = ops.RowsCtx(lt, T, lengths_host=lens, round_to=8) if ragged else ops.RowsCtx(lt, T)
    if form == "stack_mixed":
        assert 4160 < rc.R <= 5096 and _nbm(rc.R, True) == 1 and _nbm(rc.R, False) == 2, rc.R
    elif form == "stack_nbm2":
        assert rc.R > 5096 and _nbm(rc.R, True) == 2 and _nbm(rc.R, False) == 2, rc.R
    elif form == "stack":
        assert rc.R <= 4160
    B = len(lens)
    m = lens_mask(lens, T)
    g = torch.Generator().manual_seed(len(lens) * 7 + T)
    h0b = (torch.randn(B, H, T, generator=g) * m)
    r = torch.randn(B, H, T, generator=g) * m
    cond, gref = None, None
    if cond_kind == "speaker":
        cond = (torch.randn(B, 2 * H * n, generator=g) * 0.3)
        gref = cond[:, :, None].clone()
    elif cond_kind == "per_row":
        cb = torch.randn(B, 2 * H * n, T, generator=g) * 0.3 * m
        gref = cb.clone()
    set_word(WORD)
    h0 = rc.to_rows(h0b.to(dev()), torch.bfloat16)
    if cond_kind == "per_row":
        cond = rc.to_rows(cb.to(dev()), torch.float32)
    elif cond is not None:
        cond = cond.to(dev())
    fwd_tag = {"stack": "wn_stack_fwd", "stack_mixed": "wn_stack_fwd", "stack_nbm2": "wn_stack_fwd", "layer": "wn_layer_fwd",
               "two_kernel": "in_layer_gate_conv"}[form]
    ops.KERNEL_TIMER.enable(fwd_tag)
    out, saved = flow_impl.wn_fwd(rc, wn, h0, cond, True, seed, cond_per_row=cond_kind == "per_row")
    nf = ops.KERNEL_TIMER.collect()["count"]
    assert nf == (1 if form.startswith("stack") else n), (form, fwd_tag, nf)
    ops.KERNEL_TIMER.enable("wn_stack_bwd")
    with wgrad.WgradQueue(dev(), site=wn):
        dh0, grads, dcond = flow_impl.wn_bwd(rc, wn, saved, rc.to_rows(r.to(dev()), torch.bfloat16), want_dcond=cond is not None,
                                             cond_per_row=cond_kind == "per_row")
    nb = ops.KERNEL_TIMER.collect()["count"]
    assert nb == (1 if form.startswith("stack") else 0), (form, nb)
    torch.cuda.synchronize()
    print(f"WN {form} cond={cond_kind} ragged={ragged} R={rc.R}: forward NBM {_nbm(rc.R, True)}, backward NBM {_nbm(rc.R, False)}"
          f" ({fwd_tag} x{nf}, wn_stack_bwd x{nb})")

    rows = D.rows_of(rc)
    P = cpu_state(wn, "wn.")
    P["wn.cond_layer.weight"] = torch.eye(2 * H * n)[:, :, None]
    P["wn.cond_layer.bias"] = torch.zeros(2 * H * n)
    x = rc.from_rows(h0.float()).cpu() * m
    xx = x.clone().requires_grad_(True)
    gg = gref.clone().requires_grad_(True) if gref is not None else None
    drop = D.wn_masks(seed, WORD, rows, n, H, p, "wn.")
    o = R.wn_fwd(P, "wn.", xx, m, gg, drop=drop)
    (o * r).sum().backward()
    w = Worst(f"WN {form} {cond_kind}")
    got = rc.from_rows(out.float()).cpu() * m
    assert w.add("output", "out", relerr(got, o.detach())) < 3e-2
    assert w.add("input grad", "dh0", relerr(rc.from_rows(dh0.float()).cpu() * m, xx.grad * m)) < 3e-2
    if cond_kind == "speaker":
        assert w.add("cond grad", "dcond", relerr(dcond.cpu(), gg.grad[:, :, 0])) < 6e-2
    elif cond_kind == "per_row":
        assert w.add("cond grad", "dcond", relerr(rc.from_rows(dcond).cpu() * m, gg.grad * m)) < 6e-2
    byid = {id(t): v for t, v in grads.items()}
    for name, prm in wn.named_parameters():
        ref = P["wn." + name].grad
        assert id(prm) in byid, name
        assert w.add("param grad", name, relerr(byid[id(prm)].float().cpu(), ref)) < 6e-2, name
    w.show()
    dgot = rc.from_rows(dh0.float()).cpu() * m
    for what, sd, wd in (("previous step's word", seed, prev_word()), ("layer seed + 1", seed + 1, WORD)):
        x2 = x.clone().requires_grad_(True)
        o2 = R.wn_fwd(P, "wn.", x2, m, gref, drop=D.wn_masks(sd, wd, rows, n, H, p, "wn."))
        (dx2,) = torch.autograd.grad((o2 * r).sum(), [x2])
        eo, ed = relerr(got, o2.detach()), relerr(dgot, dx2 * m)
        print(f"  negative control [WN {form} / {what}]: out {eo:.3g}, d h0 {ed:.3g} (>= {NEG * 3e-2:.3g})")
        assert max(eo, ed) >= NEG * 3e-2, (what, eo, ed)


@pytest.mark.parametrize("form", ["stack", "layer", "two_kernel"])
@pytest.mark.parametrize("ragged", [False, True])
def test_wn_gate_mask_recovered_exactly(built, form, ragged):
    """Tiny in-layer weights and a positive bias make x_in = bias (+ ~0): a dropped tanh half saves T = tanh(0) = 0, a dropped
    sigmoid half S = sigmoid(0) = 0.5; a kept one T = tanh(1.25 b), S = sigmoid(1.25 b) (scale 1/(1-p), p = 0.2).  The dropped sets read off the saved
    T / S of every layer equal drop_keep_gate(word ^ (seed + layer), row, channel) bit for bit, on every valid frame."""
    from glow_tts_amd import flow_impl, modules, ops
    H, n, p, seed = 192, 4, 0.2, 999
    wn = fill_module(modules.WN(160, H, 5, 1, n, 0, p), "wn.").to(dev())
    with torch.no_grad():
        for il in wn.in_layers:
            il.weight_g.fill_(1e-6)
            il.bias.fill_(1.0)
    if form == "two_kernel":
        wn.set_fused(False)
    if form == "layer":
        wn.set_stack(False, False)
    modules.prepare_all(wn)
    lens, T = [131, 70, 2, 1, 64, 97], 131
    lt = torch.tensor(lens, dtype=torch.int32, device=dev())
    rc = ops.RowsCtx(lt, T, lengths_host=lens, round_to=8) if ragged else ops.RowsCtx(lt, T)
    h0 = (torch.randn(rc.R, H, generator=torch.Generator().manual_seed(3)).to(dev()) * rc.rowmask[:, None]).to(torch.bfloat16)
    set_word(WORD)
    _, (xs, ts, ss, _, _, _) = flow_impl.wn_fwd(rc, wn, h0, None, True, seed)
    torch.cuda.synchronize()
    rows = D.rows_of(rc)
    valid = [rows[b, :l] for b, l in enumerate(lens)]
    vr = np.concatenate(valid)
    t16 = D.thresh16(p)
    for i in range(n):
        t = ts[i].float().cpu().numpy()[vr]
        s = ss[i].float().cpu().numpy()[vr]
        assert (np.abs(t) < 1e-3).sum() + (np.abs(t) > 0.5).sum() == t.size, "T is neither tanh(0) nor tanh(1.25)"
        kt, ks = D.drop_keep_gate(D.word_seed(WORD, seed + i), vr[:, None], np.arange(H)[None, :], t16)
        assert np.array_equal(np.abs(t) > 0.5, kt), (i, (np.abs(t) > 0.5).mean(), kt.mean())
        assert np.array_equal(s > 0.6, ks), (i, (s > 0.6).mean(), ks.mean())
        assert 0.1 < 1 - kt.mean() < 0.3 and 0.1 < 1 - ks.mean() < 0.3


# ----------------------------------------------------------------------------- FlowSpecDecoder module
@pytest.mark.parametrize("ragged,prosody", [(False, False), (True, True)])
def test_decoder_train_vs_oracle(built, ragged, prosody):
    """FlowSpecDecoder (2 blocks, p = 0.5) in .train() at _step 4 -> seed (5 * 7919), block b / chain WaveNet k / layer i at
    seed + 16 b + 4 k + i: z, log-det, d y and every parameter gradient at test_decoder_gpu._run_decoder_case's tolerances
    (z 3e-2, log-det 2e-3 * valid frames + 1e-2, d y 3e-2, parameters 6e-2); with prosody the chain wn -> wn_energy ->
    wn_pitch under a speaker vector (the fused between-WaveNets kernels).  The untouched half of every coupling dilutes a mask
    error in z, so the negative control takes the larger of its z and d y misses."""
    from glow_tts_amd import models, ops
    n_blocks, lens = 2, [50, 27, 12]
    B, T = len(lens), 50
    gin = 256 if prosody else 0
    pd = 0.5
    dec = fill_module(models.FlowSpecDecoder(80, 192, 5, 1, n_blocks, 4, p_dropout=pd, gin_channels=gin, with_prosody_wn=prosody),
                      "decoder.").train()
    P = cpu_state(dec, "decoder.")
    g = torch.Generator().manual_seed(41)
    m = lens_mask(lens, T)
    y = torch.randn(B, 80, T, generator=g) * m
    spk = torch.randn(B, gin, 1, generator=g) if prosody else None
    pit = torch.randn(B, 1, T, generator=g) * m if prosody else None
    ene = torch.randn(B, 1, T, generator=g).abs() * m if prosody else None
    T2 = T // 2
    lsq = [l // 2 for l in lens]
    rows = D.row_map(lsq, T2, ragged=ragged, round_to=ops.RowsConfig(ragged=True).row_round)
    chain = ("wn", "wn_energy", "wn_pitch") if prosody else ("wn",)
    step = 4
    drop = D.decoder_masks(step + 1, WORD, rows, n_blocks, p=pd, chain=chain)
    yy = y.clone().requires_grad_(True)
    gg = spk.clone().requires_grad_(True) if prosody else None
    z, ld = R.decoder_fwd(P, "decoder.", yy, m, gg, n_blocks=n_blocks, pitch=pit, energy=ene, drop=drop)
    rz = torch.randn(z.shape, generator=g) * m[:, :, :z.shape[2]]; rl = torch.randn(B, generator=g) * 0.1
    ((z * rz).sum() + (ld * rl).sum()).backward()

    dec = dec.to(dev())
    dec.rows_cfg = ops.RowsConfig(ragged=ragged)
    if ragged:
        dec.rows_cfg.host_lengths["y"] = list(lens)
    try:
        set_word(WORD)
        dec._step = step
        yd = y.to(dev()).requires_grad_(True)
        gd = spk.to(dev()).requires_grad_(True) if prosody else None
        zd, ldd = dec(yd, m.to(dev()), g=gd, pitch=None if pit is None else pit.to(dev()), energy=None if ene is None else ene.to(dev()))
        ((zd * rz.to(dev())).sum() + (ldd * rl.to(dev())).sum()).backward()
        torch.cuda.synchronize()
    finally:
        dec.rows_cfg = ops.RowsConfig()
    assert dec._step == step + 1
    w = Worst(f"decoder ragged={ragged} prosody={prosody}")
    zc = zd.detach().cpu()
    assert w.add("output", "z", relerr(zc, z.detach())) < 3e-2
    nvalid = torch.tensor(lens, dtype=torch.float32) // 2 * 160
    assert ((ldd.detach().cpu() - ld.detach()).abs() < 2e-3 * nvalid + 1e-2).all(), (ldd.cpu(), ld)
    w.add("log-det", "logdet", relerr(ldd.detach().cpu(), ld.detach()))
    assert w.add("input grad", "dy", relerr(yd.grad.cpu(), yy.grad)) < 3e-2
    if prosody:
        assert w.add("cond grad", "dg", relerr(gd.grad.cpu(), gg.grad)) < 6e-2
    for name, prm in dec.named_parameters():
        ref = P["decoder." + name].grad
        if name.endswith("cond_layer1.weight_v"):          # a mathematically zero gradient (test_decoder_gpu.py: one input channel)
            continue
        assert prm.grad is not None, name
        assert w.add("param grad", name, relerr(prm.grad.cpu(), ref)) < 6e-2, (name, relerr(prm.grad.cpu(), ref))
    w.show()
    for what, st, wd in (("previous step's word", step + 1, prev_word()), ("previous _step", step, WORD)):
        y2 = y.clone().requires_grad_(True)
        z2, ld2 = R.decoder_fwd(P, "decoder.", y2, m, spk, n_blocks=n_blocks, pitch=pit, energy=ene,
                                drop=D.decoder_masks(st, wd, rows, n_blocks, p=pd, chain=chain))
        (dy2,) = torch.autograd.grad((z2 * rz).sum() + (ld2 * rl).sum(), [y2])
        ez, ed = relerr(zc, z2.detach()), relerr(yd.grad.cpu(), dy2)
        print(f"  negative control [decoder / {what}]: z {ez:.3g}, d y {ed:.3g} (>= {NEG * 3e-2:.3g})")
        assert max(ez, ed) >= NEG * 3e-2, (what, ez, ed)


# ----------------------------------------------------------------------------- attention
def _attn_path(T):
    """which kernels gt_attn_fwd / gt_attn_bwd run for this T (D = 96, window 4): the dispatchers' own predicate"""
    from glow_tts_amd import _lib
    return "mfma" if _lib.lib().gt_attn_mfma_shape(int(T), 96, 4) else "generic"


@pytest.mark.parametrize("T,path", [(37, "mfma"), (150, "mfma"), (256, "mfma"), (257, "mfma"), (375, "mfma"), (400, "generic")])
def test_mha_train_vs_oracle(built, T, path):
    """MultiHeadAttention (p = 0.1; the stand-alone module hashes with seed 0 ^ word): the MFMA kernels for T <= 384 (5, 8 and
    12 key tiles: T = 37 / 150, 256, 257 / 375) and the generic kernels above (T = 400); output 3e-2, P 2e-2 (abs), d x
    4e-2, parameters grad_ok 6e-2 (test_encoder_gpu.test_mha_fwd_bwd).  The oracle's DROPPED P feeds both the value matmul
    and the relative-value term."""
    from glow_tts_amd import attentions
    assert _attn_path(T) == path, (T, _attn_path(T))
    p = 0.1
    att = fill_module(attentions.MultiHeadAttention(192, 192, 2, window_size=4, p_dropout=p), "mha.").train()
    P = cpu_state(att, "mha.")
    lens = [T, max(1, T - 2 * (T // 3))]
    B = len(lens)
    xm = lens_mask(lens, T)
    g = torch.Generator().manual_seed(T + 1)
    x = torch.randn(B, 192, T, generator=g) * xm
    xx = x.clone().requires_grad_(True)
    am = xm.unsqueeze(2) * xm.unsqueeze(-1)
    dmask = D.attn_mask(0, WORD, B, 2, T, p)
    o, pr = R.mha_fwd(P, "mha.", xx, xx, am, drop={"mha.drop:0": dmask})
    r = torch.randn(o.shape, generator=g) * xm
    (o * r).sum().backward()
    att = att.to(dev())
    set_word(WORD)
    xd = x.to(dev()).requires_grad_(True)
    od = att(xd, xd, am.to(dev()))
    (od * r.to(dev())).sum().backward()
    torch.cuda.synchronize()
    w = Worst(f"MHA T={T} ({path} kernels)")
    valid = xm.bool().expand_as(o)
    oc = od.detach().cpu()
    assert w.add("output", "out", relerr(oc[valid], o.detach()[valid])) < 3e-2
    pv = (xm.unsqueeze(-1) * xm.unsqueeze(2)).bool().expand_as(pr)
    perr = (att.attn.cpu() * dmask - pr.detach())[pv].abs().max().item()
    assert w.add("P (abs)", "p", perr) < 2e-2
    assert w.add("input grad", "dx", relerr(xd.grad.cpu(), xx.grad)) < 4e-2
    for name, prm in att.named_parameters():
        ref = P["mha." + name].grad
        w.add("param grad", name, relerr(prm.grad.cpu(), ref))
        assert grad_ok(prm.grad.cpu(), ref, 6e-2, name=name), name
    w.show()
    with torch.no_grad():
        wrong = {"previous step's word": R.mha_fwd(P, "mha.", x, x, am, drop={"mha.drop:0": D.attn_mask(0, prev_word(), B, 2, T, p)})[0],
                 "seed + 1": R.mha_fwd(P, "mha.", x, x, am, drop={"mha.drop:0": D.attn_mask(1, WORD, B, 2, T, p)})[0]}
    negative(oc * xm, {k: v * xm for k, v in wrong.items()}, 3e-2, f"MHA T={T}")


@pytest.mark.parametrize("T,path", [(37, "mfma"), (300, "mfma"), (400, "generic")])
@pytest.mark.parametrize("ragged", [False, True])
def test_attention_mask_recovered_exactly(built, T, path, ragged):
    """V one-hot over the key block [0, 96) (conv_v = identity, x[c, t] = [c mod 96 == t]), Ev = 0: the attention output of
    head h, channel j < 96 is the DROPPED probability P'[b, h, i, j] — zero exactly where the kernel dropped.  The dropped set
    equals drop_keep(word ^ seed, (b*H + h)*T + i, j) bit for bit (MFMA kernels at T = 37 and in their 12-tile form at T = 300,
    generic kernels at T = 400), on the uniform and the ragged rows layout."""
    from glow_tts_amd import attentions, encoder_impl, modules, ops
    assert _attn_path(T) == path, (T, _attn_path(T))
    p, seed, H, Dh = 0.5, 77, 2, 96
    att = fill_module(attentions.MultiHeadAttention(192, 192, 2, window_size=4, p_dropout=p), "mha.").to(dev())
    with torch.no_grad():
        att.conv_v.weight.copy_(torch.eye(192, device=dev())[:, :, None])
        att.conv_v.bias.zero_()
        att.emb_rel_v.zero_()
        att.conv_q.weight.mul_(0.3); att.conv_k.weight.mul_(0.3)
    modules.prepare_all(att)
    att._refresh_padded()
    lens = [T, T - T // 3]
    B = len(lens)
    x = torch.zeros(B, 192, T)
    for c in range(192):
        if c % Dh < T:
            x[:, c, c % Dh] = 1.0
    x = x * lens_mask(lens, T)
    lt = torch.tensor(lens, dtype=torch.int32, device=dev())
    rc = ops.RowsCtx(lt, T, lengths_host=lens, round_to=8) if ragged else ops.RowsCtx(lt, T)
    set_word(WORD)
    xb = rc.to_rows(x.to(dev()), torch.bfloat16)
    _, saved = encoder_impl.mha_fwd(rc, att, xb, p, seed)
    torch.cuda.synchronize()
    o, Pu = rc.from_rows(saved[4].float()).cpu(), saved[5].cpu()      # o: [B, C, T] attention output; Pu: un-dropped P
    for b in range(B):
        L = lens[b]
        nk = min(Dh, L)                                                                  # valid keys of the one-hot block
        for h in range(H):
            got = o[b, h * Dh:h * Dh + nk, :L].t()                                      # [i, j]
            assert (Pu[b, h, :L, :nk] > 0).all()
            drop_got = (got == 0).numpy()
            i = np.arange(L)[:, None]
            keep = D.drop_keep(D.word_seed(WORD, seed), (b * H + h) * T + i, np.arange(nk)[None, :], D.thresh32(p))
            assert np.array_equal(drop_got, ~keep), (b, h, drop_got.mean(), 1 - keep.mean())
            want = Pu[b, h, :L, :nk] * torch.from_numpy(keep.astype(np.float32)) * float(D.scale(p))
            assert (got - want).abs().max().item() < 1e-2


# ----------------------------------------------------------------------------- encoder stack, text encoder (prenet), DDS
def test_encoder_train_vs_oracle(built):
    """attentions.Encoder (2 layers, p = 0.1; the stand-alone module seeds layer i with 8 i): the attention-P,
    attention-output, FFN-ReLU and FFN-output sites of both layers; output 3e-2, d x 5e-2, parameters grad_ok 8e-2
    (test_encoder_gpu.test_encoder_stack_fwd_bwd)."""
    from glow_tts_amd import attentions
    p = 0.1
    enc = fill_module(attentions.Encoder(192, 768, 2, 2, 3, p, window_size=4), "enc.").train()
    P = cpu_state(enc, "enc.")
    T, lens = 41, [41, 17, 30]
    B = len(lens)
    xm = lens_mask(lens, T)
    g = torch.Generator().manual_seed(2)
    x = torch.randn(B, 192, T, generator=g) * xm
    rows = D.row_map(lens, T)
    masks = lambda w, off: {k: v for i in range(2) for k, v in D.encoder_layer_masks(8 * i + off, w, rows, i, B, T, p=p, pre="enc.").items()}
    xx = x.clone().requires_grad_(True)
    o = R.encoder_fwd(P, "enc.", xx, xm, n_layers=2, drop=masks(WORD, 0))
    r = torch.randn(o.shape, generator=g)
    (o * r).sum().backward()
    enc = enc.to(dev())
    set_word(WORD)
    xd = x.to(dev()).requires_grad_(True)
    od = enc(xd, xm.to(dev()))
    (od * r.to(dev())).sum().backward()
    torch.cuda.synchronize()
    w = Worst("encoder")
    oc = od.detach().cpu()
    assert w.add("output", "out", relerr(oc, o.detach())) < 3e-2
    assert w.add("input grad", "dx", relerr(xd.grad.cpu(), xx.grad)) < 5e-2
    for name, prm in enc.named_parameters():
        ref = P["enc." + name].grad
        w.add("param grad", name, relerr(prm.grad.cpu(), ref))
        assert grad_ok(prm.grad.cpu(), ref, 8e-2, name=name), name
    w.show()
    with torch.no_grad():
        wrong = {"previous step's word": R.encoder_fwd(P, "enc.", x, xm, n_layers=2, drop=masks(prev_word(), 0)),
                 "layer seed + 1": R.encoder_fwd(P, "enc.", x, xm, n_layers=2, drop=masks(WORD, 1))}
    negative(oc, wrong, 3e-2, "encoder")


def test_text_encoder_prenet_train_vs_oracle(built):
    """models.TextEncoder with the prenet (ConvReluNorm, p = 0.5, drop AFTER the ReLU) and 2 encoder layers (p = 0.1), _step 6 ->
    seed 7 * 104729; prenet layer i at seed + i, encoder layer i at seed + 16 + 8 i: x and x_m at 3e-2
    (test_encoder_gpu.test_text_encoder_fwd)."""
    from glow_tts_amd import models
    gen = fill_module(models.FlowGenerator(148, 192, 768, 256, 80, use_sdp=False, kernel_size=3, n_heads=2, n_layers_enc=2, p_dropout=0.1,
                                           n_blocks_dec=1, kernel_size_dec=5, dilation_rate=1, n_block_layers=4, p_dropout_dec=0.05,
                                           n_sqz=2, window_size=4, mean_only=True, prenet=True), "")
    P = cpu_state(gen)
    g = torch.Generator().manual_seed(6)
    T = 23
    ids = torch.randint(1, 148, (2, T), generator=g); xl = torch.tensor([23, 9])
    rows = D.row_map([23, 9], T)
    step = 6
    masks = lambda w, st: D.text_encoder_masks(st, w, rows, 2, T, n_layers=2, p=0.1, p_pre=0.5)
    with torch.no_grad():
        x, x_m, _, m = R.text_encoder_fwd(P, "encoder.", ids, xl, n_layers=2, drop=masks(WORD, step + 1))
    gen = gen.to(dev()).train()
    gen.prepare()
    set_word(WORD)
    gen.encoder._step = step
    xd, xmd, _, md = gen.encoder(ids.to(dev()), xl.to(dev()), prepared=True)
    torch.cuda.synchronize()
    w = Worst("text encoder")
    xc = xd.detach().cpu()
    assert w.add("output", "x", relerr(xc, x)) < 3e-2 and w.add("output", "x_m", relerr(xmd.detach().cpu(), x_m)) < 3e-2
    w.show()
    with torch.no_grad():
        wrong = {"previous step's word": R.text_encoder_fwd(P, "encoder.", ids, xl, n_layers=2, drop=masks(prev_word(), step + 1))[0],
                 "previous _step": R.text_encoder_fwd(P, "encoder.", ids, xl, n_layers=2, drop=masks(WORD, step))[0]}
    negative(xc, wrong, 3e-2, "text encoder")


def test_dds_train_vs_oracle(built):
    """DilatedDepthSeparableConv (p = 0.5, modules.py:733; the stand-alone module seeds layer i with i): output 2e-2, d x and
    d g 3e-2 on valid frames, parameter gradients 8e-2 (test_predictors_gpu.test_dds_conv_module_fwd_bwd)."""
    from glow_tts_amd import predictors
    p = 0.5
    dds = fill_module(predictors.DilatedDepthSeparableConv(192, 3, 3, p), "dds.").train()
    P = cpu_state(dds, "dds.")
    lens, T = [23, 11], 23
    B = len(lens)
    m = lens_mask(lens, T)
    gen = torch.Generator().manual_seed(9)
    x = torch.randn(B, 192, T, generator=gen) * m
    gc = torch.randn(B, 192, T, generator=gen) * 0.5
    rows = D.row_map(lens, T)
    xx, gg = x.clone().requires_grad_(True), gc.clone().requires_grad_(True)
    o = R.dds_conv(P, "dds.", xx, m, g=gg, drop=D.dds_masks(0, WORD, rows, p=p, pre="dds."))
    r = torch.randn(o.shape, generator=torch.Generator().manual_seed(3)) * m
    (o * r).sum().backward()
    dds = dds.to(dev())
    set_word(WORD)
    xd, gd = x.to(dev()).requires_grad_(True), gc.to(dev()).requires_grad_(True)
    od = dds(xd, m.to(dev()), g=gd)
    (od * r.to(dev())).sum().backward()
    torch.cuda.synchronize()
    w = Worst("DDS")
    oc = od.detach().cpu()
    assert w.add("output", "out", relerr(oc, o.detach())) < 2e-2
    vm = m.bool().expand_as(x)
    assert w.add("input grad", "dx", relerr(xd.grad.cpu()[vm], xx.grad[vm])) < 3e-2
    assert w.add("cond grad", "dg", relerr(gd.grad.cpu()[vm], gg.grad[vm])) < 3e-2
    for name, prm in dds.named_parameters():
        ref = P["dds." + name].grad
        if ref.abs().max().item() < 1e-7:
            continue
        assert w.add("param grad", name, relerr(prm.grad.cpu(), ref)) < 8e-2, name
    w.show()
    with torch.no_grad():
        wrong = {"previous step's word": R.dds_conv(P, "dds.", x, m, g=gc, drop=D.dds_masks(0, prev_word(), rows, p=p, pre="dds.")),
                 "layer seed + 1": R.dds_conv(P, "dds.", x, m, g=gc, drop=D.dds_masks(1, WORD, rows, p=p, pre="dds."))}
    negative(oc, wrong, 2e-2, "DDS")


@pytest.mark.parametrize("ragged", [False, True])
def test_duration_predictor_train_vs_oracle(built, ragged):
    """DurationPredictor (p = 0.1) through the runner FlowGenerator uses (text_models._DurationRunner) at the seed of _step 3
    (text_models.py:582): self.drop after norm_1 at seed + 0 and after norm_2 at seed + 1 (encoder_impl.py:221-223), columns the
    256 filter channels.  logw at 3e-2.  The module has no eval-mode twin of its own, and its bias / LayerNorm gradients carry
    0.1-0.15 of bf16 noise (conv -> ReLU -> LayerNorm, twice) in eval mode too; so the same inputs run once more with dropout
    off, and every parameter gradient in train mode must be within max(0.1, 1.25 x) that eval-mode error (0.1: the DP's
    tolerance in test_encoder_gpu.test_train_forward_backward_vs_oracle) — dropout adds no error of its own."""
    from glow_tts_amd import modules, ops, text_models
    p, F = 0.1, 256
    names = ("conv_1.weight", "conv_1.bias", "norm_1.gamma", "norm_1.beta", "conv_2.weight", "conv_2.bias", "norm_2.gamma",
             "norm_2.beta", "proj.weight", "proj.bias")
    lens, T = [150, 97, 121, 64], 150
    B = len(lens)
    xm = lens_mask(lens, T)
    g = torch.Generator().manual_seed(17)
    x = torch.randn(B, 192, T, generator=g) * xm
    r = torch.randn(B, 1, T, generator=g) * xm
    seed = D.duration_seed(3)
    lt = torch.tensor(lens, dtype=torch.int32, device=dev())

    def run(train):
        dp = fill_module(text_models.DurationPredictor(192, F, 3, p), "dp.")
        P = cpu_state(dp, "dp.")
        dp = dp.to(dev())
        modules.prepare_all(dp)
        rc = ops.RowsCtx(lt, T, lengths_host=lens, round_to=8) if ragged else ops.RowsCtx(lt, T)
        rows = D.rows_of(rc)
        drop = D.duration_masks(seed, WORD, rows, F=F, p=p, pre="dp.") if train else None
        ref = R.duration_predictor_fwd(P, "dp.", x, xm, drop=drop)
        (ref * r).sum().backward()
        set_word(WORD)
        runner = text_models._DurationRunner(dp, rc, rc.to_rows(x.to(dev()), torch.bfloat16), train, seed)
        (logw,) = text_models._RowsFn.apply(runner, 1, *runner.params)
        (logw * r.to(dev())).sum().backward()
        torch.cuda.synchronize()
        prm = dict(dp.named_parameters())
        assert all(prm[n].grad is not None for n in names)
        return P, rows, ref.detach(), logw.detach().cpu() * xm, {n: (prm[n].grad.cpu(), P["dp." + n].grad) for n in names}

    P, rows, ref, lc, gtrain = run(True)
    _, _, _, _, geval = run(False)
    l2 = lambda a, b: (a - b).norm().item() / max(1e-12, b.norm().item())
    w = Worst(f"duration predictor ragged={ragged}")
    assert w.add("output", "logw", relerr(lc, ref)) < 3e-2
    bad = []
    for n in names:
        e_tr, e_ev = l2(*gtrain[n]), l2(*geval[n])
        w.add("param grad (rel L2)", n, e_tr)
        w.add("eval-mode param grad (rel L2)", n, e_ev)
        if not grad_ok(*gtrain[n], max(0.1, 1.25 * e_ev), name=n):
            bad.append((n, round(e_tr, 4), round(e_ev, 4)))
    w.show()
    assert not bad, bad
    with torch.no_grad():
        wrong = {"previous step's word": R.duration_predictor_fwd(P, "dp.", x, xm, drop=D.duration_masks(seed, prev_word(), rows, F=F, p=p,
                                                                                                         pre="dp.")),
                 "seed + 1": R.duration_predictor_fwd(P, "dp.", x, xm, drop=D.duration_masks(seed + 1, WORD, rows, F=F, p=p, pre="dp."))}
    negative(lc, wrong, 3e-2, f"duration predictor ragged={ragged}")
