"""gt_dds_layer_fwd / gt_dds_layer_bwd (csrc/dds_layer.hip: one DDSConv layer per launch and direction) through the C-ABI, against a
float64 restatement of the layer (modules.py:718-735) and against the per-op kernels of csrc/predictor_ops.hip on the same inputs.

The rule.  Both paths run the same arithmetic class (fp32 row work, a bf16x3 product with fp32 accumulation) and may differ in
summation order only, so the fused path's relative L2 error against float64 is held to the per-op path's error ON THE SAME DATA:

    err_fused <= max(2 * err_unfused, floor)        floor = rows64.AGG_F32 (fp32 outputs), 2^-8 (the bf16 hi part of d h2)

for every output (a1 as hi + lo, h2, out, d h2 hi, d h1, the four LayerNorm gradients, and dx / dw / db after gt_dds_dw_bwd), over
WHOLE buffers: masked rows are compared too (zeros; the 1x1 bias for h2).  The same comparison must miss by >= rows64.CONTROL_MISS
against references with one planted defect each (a zeroed 1x1 weight entry, a d = 9 tap that reads across an utterance border, plain
bf16 weights, a dropout mask from seed + 1): a comparison that cannot see these proves nothing.

Geometries (TILE = gt_dds_layer_tile_rows() = 64): R < TILE, R = 2 TILE and R = 2 TILE + 1; an utterance border exactly on a tile
edge (uniform_2tile: row 64; ragged_long: row 192) and one row off it (ragged_2tile_p1: row 63); utterances of 1, 2, 8, 9 and 10
frames (the d = 9 taps fall outside, onto the halo, and just inside); one utterance longer than 2 TILE; masked halo rows in the
middle and trailing masked rounding rows; every dilation 1, 3, 9; p = 0 and p = 0.5; seed_dev NULL and set."""
import functools
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import rows64

pytestmark = pytest.mark.gpu

C = 192
EPS = 1e-5
GUARD = 3                         # canary rows before and after every output buffer
SEED = 4242
SEED_WORD = 0x9E3779B9
FLOORS = {"dh2_hi": 2.0 ** -8}    # every other output is fp32: rows64.AGG_F32
OUTPUTS = ("a1", "h2", "out", "dh2_hi", "dh1", "dgamma2", "dbeta2", "dgamma1", "dbeta1", "dx", "dw", "db")


def dev():
    return torch.device("cuda:0")


def _tile():
    from glow_tts_amd import _lib
    return _lib.call.gt_dds_layer_tile_rows()


def _uniform(Tp, lens):
    """uniform rows layout: utterance b owns rows [b Tp, (b + 1) Tp), its frames behind a 2-row halo"""
    R = Tp * len(lens)
    utt = np.repeat(np.arange(len(lens)), Tp).astype(np.int32)
    mask = np.zeros(R, dtype=np.float32)
    for b, n in enumerate(lens):
        assert n + 4 <= Tp
        mask[b * Tp + 2: b * Tp + 2 + n] = 1
    return utt, mask


def _ragged(frames, R):
    """ragged rows layout: utterance b owns its frames + 2 halo rows on each side; the last one also owns the rows that round R up"""
    utt, mask = np.zeros(R, dtype=np.int32), np.zeros(R, dtype=np.float32)
    r0 = 0
    for b, n in enumerate(frames):
        utt[r0:] = b
        mask[r0 + 2: r0 + 2 + n] = 1
        r0 += n + 4
    assert r0 <= R
    return utt, mask


def geometries():
    T = _tile()
    assert T == 64, "the geometries below place their borders for 64-row tiles: lay them out again for another tile height"
    g = {
        "uniform_small": _uniform(14, [10, 1, 9]),                                  # R = 42 < TILE
        "uniform_2tile": _uniform(T // 4, [12, 2, 8, 9, 10, 1, 12, 11]),            # R = 2 TILE, a border on the tile edge (row 64)
        "ragged_2tile_p1": _ragged([T - 5, 10, 9, 8, 2, 1, 9], 2 * T + 1),          # R = 2 TILE + 1, a border at row 63, 3 trailing masked rows
        "ragged_long": _ragged([2 * T + 12, T - 20, 10], 3 * T + 18),               # 140 frames > 2 TILE, a border at row 192 = 3 TILE
    }
    assert g["uniform_small"][0].size < T and g["uniform_2tile"][0].size == 2 * T and g["ragged_2tile_p1"][0].size == 2 * T + 1
    return g


GEOMS = ("uniform_small", "uniform_2tile", "ragged_2tile_p1", "ragged_long")
CASES = [(gname, d, p, (i + j + k) % 2 == 1) for i, gname in enumerate(GEOMS) for j, d in enumerate((1, 3, 9)) for k, p in enumerate((0.0, 0.5))]


# ------------------------------------------------------------------------------------------------ inputs
class Inputs:
    def __init__(self, gname, seed=0):
        utt, mask = geometries()[gname]
        self.R = R = utt.size
        g = torch.Generator().manual_seed(1000 + seed + 17 * GEOMS.index(gname))
        rn = lambda *s: torch.randn(*s, generator=g)                                # noqa: E731
        self.utt, self.mask = torch.from_numpy(utt), torch.from_numpy(mask)
        self.x = rn(R, C) * self.mask[:, None]
        self.dy = rn(R, C)                                                           # masked rows too: the kernels must ignore them
        self.w_sep = rn(C, 1, 3) * 0.5
        self.b_sep = rn(C) * 0.1
        self.gamma1, self.beta1 = 1 + 0.1 * rn(C), 0.1 * rn(C)
        self.W = rn(C, C, 1) / C ** 0.5
        self.b1 = rn(C) * 0.1
        self.gamma2, self.beta2 = 1 + 0.1 * rn(C), 0.1 * rn(C)
        self.names = ("x", "dy", "w_sep", "b_sep", "gamma1", "beta1", "W", "b1", "gamma2", "beta2", "utt", "mask")
        self.d = types.SimpleNamespace(**{n: getattr(self, n).to(dev()).contiguous() for n in self.names})
        from glow_tts_amd import ops
        self.pc = ops.PackedConv(C, C, 1, split3=True, device=dev()).pack(self.d.W)
        self.seed_word = torch.from_numpy(np.array([SEED_WORD], dtype=np.uint32).view(np.int32)).to(dev())


class Guarded:
    """an output buffer of R rows between GUARD canary rows on each side"""

    def __init__(self, R, width, dtype):
        self.full = torch.empty(R + 2 * GUARD, width, dtype=dtype, device=dev())
        self.full.view(torch.int16 if dtype == torch.bfloat16 else torch.int32).fill_(0x5A5A if dtype == torch.bfloat16 else 0x5A5A5A5A)
        self.t = self.full[GUARD:GUARD + R]
        self.before = self.full.clone()

    def canaries_intact(self):
        a, b = self.full.view(torch.int16 if self.full.dtype == torch.bfloat16 else torch.int32), \
            self.before.view(torch.int16 if self.full.dtype == torch.bfloat16 else torch.int32)
        return torch.equal(a[:GUARD], b[:GUARD]) and torch.equal(a[-GUARD:], b[-GUARD:])


def _st():
    from glow_tts_amd import _lib
    return _lib.current_stream(dev())


# ------------------------------------------------------------------------------------------------ the two kernel paths
def fused_fwd(I, d, p, seed, sw, want3=False):
    from glow_tts_amd._lib import call
    D, R = I.d, I.R
    o = dict(a1=Guarded(R, 3 * C, torch.bfloat16), h2=Guarded(R, C, torch.float32), out=Guarded(R, C, torch.float32))
    if want3:
        o["out3"] = Guarded(R, 3 * C, torch.bfloat16)
    call.gt_dds_layer_fwd(D.x, C, D.w_sep, D.b_sep, D.gamma1, D.beta1, I.pc.fwd, I.pc.Kp_f, D.b1, D.gamma2, D.beta2, D.utt, D.mask,
                          o["a1"].t, 3 * C, o["h2"].t, o["out"].t, o["out3"].t if want3 else None, 3 * C, R, C, d, EPS, p, seed, sw, _st())
    return o


def unfused_fwd(I, d, p, seed, sw):
    from glow_tts_amd import ops
    from glow_tts_amd._lib import call
    D, R = I.d, I.R
    o = dict(a1=Guarded(R, 3 * C, torch.bfloat16), h2=Guarded(R, C, torch.float32), out=Guarded(R, C, torch.float32))
    call.gt_dds_sep_fwd(D.x, C, D.w_sep, D.b_sep, D.gamma1, D.beta1, D.utt, D.mask, o["a1"].t, 3 * C, R, C, d, EPS, _st())
    ctx = types.SimpleNamespace(Tp=R, B=1, row0=None, rowmask=D.mask)
    ops.conv_rows(o["a1"].t, I.pc, ctx, bias=D.b1, out=o["h2"].t)
    call.gt_dds_out_fwd(o["h2"].t, D.x, C, D.gamma2, D.beta2, D.mask, o["out"].t, None, R, C, EPS, p, seed, sw, _st())
    return o


def _dw_bwd(I, d, dh1, o, partials=None):
    from glow_tts_amd._lib import call
    D, R = I.d, I.R
    o["dx"] = Guarded(R, C, torch.float32)
    o["dw"], o["db"] = torch.zeros(C, 3, device=dev()), torch.zeros(C, device=dev())
    call.gt_dds_dw_bwd(D.x, C, dh1, D.dy, D.w_sep, D.utt, D.mask, o["dx"].t, o["dw"], o["db"], None, R, C, d, _st())


def fused_bwd(I, d, p, seed, sw, h2, partials=False):
    from glow_tts_amd import _lib
    from glow_tts_amd._lib import call
    D, R = I.d, I.R
    o = dict(dh2_hi=Guarded(R, C, torch.bfloat16), dh1=Guarded(R, C, torch.float32))
    for k in ("dgamma2", "dbeta2", "dgamma1", "dbeta1"):
        o[k] = torch.zeros(C, device=dev())
    part = Guarded(call.gt_dds_layer_partial_rows(R), 2 * C, torch.float32) if partials else None
    call.gt_dds_layer_bwd(D.x, C, D.w_sep, D.b_sep, D.gamma1, D.beta1, I.pc.dgrad, I.pc.Kp_d, D.gamma2, D.beta2, D.utt, D.mask, h2, D.dy,
                          o["dh2_hi"].t, C, o["dh1"].t, *([None] * 4 if partials else [o[k] for k in ("dgamma2", "dbeta2", "dgamma1", "dbeta1")]),
                          part.t if partials else None, R, C, d, EPS, p, seed, sw, _st())
    if partials:
        n = part.t.shape[0] // 2
        args = _lib.PartialsArgs()
        for i, (rows, a, b) in enumerate(((part.t[:n], "dgamma2", "dbeta2"), (part.t[n:], "dgamma1", "dbeta1"))):
            j = args.job[i]
            j.partials, j.dst_a, j.dst_b, j.n_rows, j.Ca, j.Cb = rows.data_ptr(), o[a].data_ptr(), o[b].data_ptr(), n, C, C
        args.n_jobs = 2
        call.gt_param_partials_reduce(args, _st())
        o["partials"] = part
    _dw_bwd(I, d, o["dh1"].t, o)
    return o


def unfused_bwd(I, d, p, seed, sw, h2):
    from glow_tts_amd import ops
    from glow_tts_amd._lib import call
    D, R = I.d, I.R
    o = dict(dh2=Guarded(R, 3 * C, torch.bfloat16), dh1=Guarded(R, C, torch.float32))
    for k in ("dgamma2", "dbeta2", "dgamma1", "dbeta1"):
        o[k] = torch.zeros(C, device=dev())
    call.gt_dds_out_bwd(h2, D.dy, D.gamma2, D.beta2, D.mask, o["dh2"].t, o["dgamma2"], o["dbeta2"], None, R, C, EPS, p, seed, sw, _st())
    ctx = types.SimpleNamespace(Tp=R, B=1, row0=None, rowmask=D.mask)
    da1 = ops.conv_rows(o["dh2"].t, I.pc, ctx, dgrad=True, out_f32=True)
    call.gt_dds_sep_bwd(D.x, C, D.w_sep, D.b_sep, D.gamma1, D.beta1, D.utt, D.mask, da1, o["dh1"].t, o["dgamma1"], o["dbeta1"], None, R, C, d, EPS,
                        _st())
    o["dh2_hi"] = types.SimpleNamespace(t=o["dh2"].t[:, :C], canaries_intact=o["dh2"].canaries_intact)
    _dw_bwd(I, d, o["dh1"].t, o)
    return o


def values(fwd, bwd):
    """the compared outputs of one path as float64 CPU tensors"""
    v = {}
    a1 = fwd["a1"].t
    v["a1"] = a1[:, :C].double().cpu() + a1[:, 2 * C:].double().cpu()
    for k in ("h2", "out"):
        v[k] = fwd[k].t.double().cpu()
    for k in ("dh2_hi", "dh1", "dx"):
        v[k] = bwd[k].t.double().cpu()
    for k in ("dgamma2", "dbeta2", "dgamma1", "dbeta1", "dw", "db"):
        v[k] = bwd[k].double().cpu()
    return v


def keep_mask(out_p, out_0, I):
    """the dropout keep mask read off a forward, as tests/test_predictors_gpu.py::test_dds_dropout_replays_in_backward does"""
    xm = I.d.x * I.d.mask[:, None]
    y_eval = out_0 - xm
    return (((out_p - xm).abs() > 0) | (y_eval.abs() < 1e-12)).cpu()


# ------------------------------------------------------------------------------------------------ float64 restatement of one layer
def reference(I, d, keep, scale, W=None, cross_border=False):
    """one layer forward in float64 and its backward by autograd; keep: bool [R, C] or None.  Planted defects: W (another 1x1 weight),
    cross_border (the +-d taps ignore the utterance index)."""
    R = I.R
    P = {n: getattr(I, n).double().clone().requires_grad_(True) for n in ("x", "w_sep", "b_sep", "gamma1", "beta1", "b1", "gamma2", "beta2")}
    Wm = (I.W if W is None else W).double()[:, :, 0]
    mask, utt = I.mask.double(), I.utt.long()
    x = P["x"]
    h1 = P["b_sep"] + P["w_sep"][:, 0, 1] * x
    for k, off in ((0, -d), (2, d)):
        idx = torch.arange(R) + off
        idc = idx.clamp(0, R - 1)
        ok = (idx >= 0) & (idx < R) & (mask[idc] != 0)
        if not cross_border:
            ok = ok & (utt[idc] == utt)
        h1 = h1 + P["w_sep"][:, 0, k] * x[idc] * ok[:, None].double()
    h1.retain_grad()
    a1 = F.gelu(F.layer_norm(h1, (C,), P["gamma1"], P["beta1"], EPS)) * mask[:, None]
    h2 = a1 @ Wm.T + P["b1"]
    h2.retain_grad()
    y = F.gelu(F.layer_norm(h2, (C,), P["gamma2"], P["beta2"], EPS))
    if keep is not None:
        y = y * keep.double() * scale
    out = (x + y) * mask[:, None]
    (out * I.dy.double()).sum().backward()
    return {"a1": a1.detach(), "h2": h2.detach(), "out": out.detach(), "dh2_hi": h2.grad, "dh1": h1.grad,
            "dgamma2": P["gamma2"].grad, "dbeta2": P["beta2"].grad, "dgamma1": P["gamma1"].grad, "dbeta1": P["beta1"].grad,
            "dx": x.grad, "dw": P["w_sep"].grad[:, 0, :], "db": P["b_sep"].grad}


def rel_l2(got, ref):
    return float((got - ref).norm() / ref.norm().clamp_min(1e-300))


def limits(vu, ref):
    """per output: max(2 * err_unfused, floor)"""
    return {k: max(2.0 * rel_l2(vu[k], ref[k]), FLOORS.get(k, rows64.AGG_F32)) for k in OUTPUTS}


# ------------------------------------------------------------------------------------------------ one case, run once
@functools.lru_cache(maxsize=None)
def run_case(gname, d, p, with_seed_dev):
    I = Inputs(gname)
    sw = I.seed_word if with_seed_dev else None
    ff, uf = fused_fwd(I, d, p, SEED, sw, want3=True), unfused_fwd(I, d, p, SEED, sw)
    fb, ub = fused_bwd(I, d, p, SEED, sw, ff["h2"].t), unfused_bwd(I, d, p, SEED, sw, uf["h2"].t)
    keep_f = keep_u = None
    if p > 0:
        f0, u0 = fused_fwd(I, d, 0.0, SEED, sw), unfused_fwd(I, d, 0.0, SEED, sw)
        keep_f, keep_u = keep_mask(ff["out"].t, f0["out"].t, I), keep_mask(uf["out"].t, u0["out"].t, I)
    torch.cuda.synchronize()
    return types.SimpleNamespace(I=I, ff=ff, uf=uf, fb=fb, ub=ub, keep_f=keep_f, keep_u=keep_u, scale=1.0 / (1.0 - p), sw=sw,
                                 vf=values(ff, fb), vu=values(uf, ub))


@pytest.mark.parametrize("gname,d,p,with_seed_dev", CASES)
def test_fused_layer_against_float64(built, gname, d, p, with_seed_dev):
    r = run_case(gname, d, p, with_seed_dev)
    I = r.I
    # exact checks first: the dropout mask is the per-op path's bit for bit, a1's two hi copies agree, the bf16x3 copy of `out` is
    # gt_rows_split3's, masked rows are what the per-op path leaves, and no canary row was touched
    if p > 0:
        assert torch.equal(r.keep_f, r.keep_u)
        frac = r.keep_f[I.mask.bool()].float().mean().item()
        assert 0.4 < frac < 0.6, frac
    a1 = r.ff["a1"].t
    assert torch.equal(a1[:, :C], a1[:, C:2 * C])
    o3, o = r.ff["out3"].t, r.ff["out"].t
    hi = o.to(torch.bfloat16)
    assert torch.equal(o3[:, :C], hi) and torch.equal(o3[:, C:2 * C], hi) and torch.equal(o3[:, 2 * C:], (o - hi.float()).to(torch.bfloat16))
    off = ~I.mask.bool().to(dev())
    assert a1[off].float().abs().max().item() == 0 and o[off].abs().max().item() == 0
    assert torch.equal(r.ff["h2"].t[off], I.d.b1.expand(int(off.sum()), C))
    assert r.fb["dh2_hi"].t[off].float().abs().max().item() == 0 and r.fb["dh1"].t[off].abs().max().item() == 0
    assert r.fb["dx"].t[off].abs().max().item() == 0
    for path in (r.ff, r.fb, r.uf, r.ub):
        for k, buf in path.items():
            if hasattr(buf, "canaries_intact"):
                assert buf.canaries_intact(), k
    # the rule
    ref = reference(I, d, r.keep_f, r.scale)
    lim = limits(r.vu, ref)
    bad = []
    for k in OUTPUTS:
        ef, eu = rel_l2(r.vf[k], ref[k]), rel_l2(r.vu[k], ref[k])
        print(f"{gname} d={d} p={p} seed_dev={int(with_seed_dev)} {k}: err_fused {ef:.3e} err_unfused {eu:.3e} ratio {ef / max(eu, 1e-300):.3f} "
              f"limit {lim[k]:.3e}")
        if not ef <= lim[k]:
            bad.append((k, ef, eu, lim[k]))
    assert not bad, bad


DEFECT_CASE = ("ragged_2tile_p1", 9, 0.5, True)


@pytest.mark.parametrize("defect", ["zeroed_weight_entry", "tap_across_border", "plain_bf16_weights", "mask_of_seed_plus_1"])
def test_planted_defects_are_seen(built, defect):
    """the comparison of test_fused_layer_against_float64, against a reference with one planted defect: some output must miss its
    limit (the one the TRUE reference gives: max(2 err_unfused, floor)) by >= CONTROL_MISS"""
    gname, d, p, wsd = DEFECT_CASE
    r = run_case(gname, d, p, wsd)
    I = r.I
    lim = limits(r.vu, reference(I, d, r.keep_f, r.scale))
    kw = dict(keep=r.keep_f, scale=r.scale)
    if defect == "zeroed_weight_entry":
        W = I.W.clone()
        W.view(-1)[int(W.abs().argmax())] = 0
        kw["W"] = W
    elif defect == "tap_across_border":
        kw["cross_border"] = True
    elif defect == "plain_bf16_weights":
        kw["W"] = I.W.to(torch.bfloat16).float()
    else:
        f1, f0 = fused_fwd(I, d, p, SEED + 1, r.sw), fused_fwd(I, d, 0.0, SEED + 1, r.sw)
        kw["keep"] = keep_mask(f1["out"].t, f0["out"].t, I)
        assert not torch.equal(kw["keep"], r.keep_f)
    bad = reference(I, d, **kw)
    miss = {k: rel_l2(r.vf[k], bad[k]) / lim[k] for k in OUTPUTS}
    print(defect, {k: round(v, 2) for k, v in miss.items()})
    assert max(miss.values()) >= rows64.CONTROL_MISS, miss
    # the defect is seen in both directions: by a forward output and by a backward output
    assert max(miss[k] for k in ("a1", "h2", "out")) >= rows64.CONTROL_MISS, miss
    assert max(miss[k] for k in OUTPUTS[3:]) >= rows64.CONTROL_MISS, miss


@pytest.mark.parametrize("gname", GEOMS)
def test_atomics_and_partials_forms_agree(built, gname):
    """one atomic per address and workgroup, or one plain-stored partial row per workgroup summed by gt_param_partials_reduce: the same
    parameter gradients to 1e-5 relative (as test_dds_dropout_replays_in_backward asserts for gt_dds_out_bwd), the same d h2 / d h1"""
    r = run_case(gname, 3, 0.5, True)
    pb = fused_bwd(r.I, 3, 0.5, SEED, r.sw, r.ff["h2"].t, partials=True)
    torch.cuda.synchronize()
    assert pb["partials"].canaries_intact() and pb["dh2_hi"].canaries_intact() and pb["dh1"].canaries_intact()
    for k in ("dgamma2", "dbeta2", "dgamma1", "dbeta1"):
        a, b = pb[k].double(), r.fb[k].double()
        assert float((a - b).abs().max() / b.abs().max()) < 1e-5, k
    assert torch.equal(pb["dh2_hi"].t, r.fb["dh2_hi"].t) and torch.equal(pb["dh1"].t, r.fb["dh1"].t)


@pytest.mark.parametrize("gname,d,p,with_seed_dev", [("ragged_long", 9, 0.5, False), ("uniform_2tile", 3, 0.5, True), ("ragged_2tile_p1", 1, 0.0, False)])
def test_a_forward_of_one_path_feeds_the_backward_of_the_other(built, gname, d, p, with_seed_dev):
    r = run_case(gname, d, p, with_seed_dev)
    I = r.I
    ref = reference(I, d, r.keep_f, r.scale)
    lim = limits(r.vu, ref)
    fu = values(r.ff, unfused_bwd(I, d, p, SEED, r.sw, r.ff["h2"].t))          # fused forward, per-op backward
    uf = values(r.uf, fused_bwd(I, d, p, SEED, r.sw, r.uf["h2"].t))            # per-op forward, fused backward
    torch.cuda.synchronize()
    for name, v in (("fused fwd + per-op bwd", fu), ("per-op fwd + fused bwd", uf)):
        bad = [(k, rel_l2(v[k], ref[k]), lim[k]) for k in OUTPUTS if not rel_l2(v[k], ref[k]) <= lim[k]]
        assert not bad, (name, bad)
