"""The ConvFlow, spline and likelihood row kernels of csrc/predictor_ops.hip (gt_convflow_pre_fwd/bwd, gt_convflow_spline_fwd/bwd/inv,
gt_ea_fwd/bwd, gt_sdp_mid_fwd/bwd, gt_nll_gauss_fwd/bwd) through the C-ABI, each against its float64 restatement (oracle/spline64.py)
on the kernel's own fp32 operands.

The rule.  The spline's conditioning depends on its parameters (bins as narrow as 0.01 give slopes near 1e3), so no fixed tolerance
fits: for every output

    err_kernel <= max(M * err_twin, floor)          floor = rows64.AGG_F32

with err_* the relative L2 error against float64 over the WHOLE buffer (masked rows included) and err_twin the error of the same
operator run in torch float32 on the same operands.  The kernels are another fp32 arithmetic than torch's (__expf, rsqrtf, a hardware
reciprocal in sigmoidf_, another summation order), so M is measured: the next power of two at or above twice the worst measured
err_kernel / err_twin, never above 16 (DESIGN.md 4.6.2 holds the measured ratios).  Chosen: M = 16 for the spline backward's dh, dWp,
dbp, dz_in (measured 6.6, 6.6, 6.7, 4.1), the class (c) rows (y 4.1, log|det| 5.1) and gt_sdp_mid_fwd's z and acc (4.8, 5.3); 8 for the
spline forward's acc (2.9), the inverse's residual and round trip (2.5, 2.7) and dlog_scale (2.5); 4 or 2 for everything else (<= 1.8);
the dictionary M below holds every value.  The errors of the elementwise kernels and of gt_convflow_pre_* are 1e-8 .. 6e-7 throughout,
under the floor by a factor of 30 or more.

The same comparisons must miss by >= rows64.CONTROL_MISS against references with one planted defect each: a log|det| without its
2 log(delta) term, a knot gradient that forgets the bins j > k + 1, an end derivative not pinned to 1, `flip` ignored, a destination
overwritten instead of added to, a border row credited to the neighbouring utterance.

Buffers: every output sits between canary rows; every destination the kernels accumulate into (acc, dWp, dbp, dw_pre, db_pre, dz and dg
of pre_bwd, dlog_scale, dtranslation) starts from non-zero values; the partial-row buffer of gt_convflow_spline_bwd starts as NaN.

Spline inputs: h ~ N(0, 1) [R, 192]; Wp rows 0..19 of std s, rows 20..28 of std s / sqrt(192) * {1, 8} (s = 0.05, 1, 2 is the std of
the raw widths / heights after the 1 / sqrt(C) scale; the factor 8 puts raw derivative parameters beyond +-20, the softplus switch);
bp non-zero.  x: (a) uniform in [-6, 6]; (b) -5, 5, 0 and the fp32 neighbours just outside +-5; the midpoint of every bin and both
tails; (c) the float64 interior knots rounded to fp32 and their two fp32 neighbours (forward values and the inverse only).  For the
backward a row within 1e-5 of an interior knot is moved to its bin's midpoint when the inputs are built (at most 0.5 % of the rows).

Geometries, spline kernels (32 rows per workgroup): R = 31, 32, 33, 70 and 128; an utterance border inside a tile, one exactly at row
32, a one-frame utterance, row 0 of a tile masked, a fully masked tile, trailing masked rows.  Elementwise kernels (256 threads, one
utterance index per 64-lane wave on the fast path): R = 63, 64, 65, 257, 300; borders at rows 40, 64 and 256; lane 0 of a wave masked
with the others valid; a wave without a valid row; three utterances inside one wave."""
import functools
import math
import types

import numpy as np
import pytest
import torch

from oracle import rows64
from oracle import spline64 as S
from test_dds_layer_gpu import Guarded, _st, dev, rel_l2

pytestmark = pytest.mark.gpu

C = 192
F32 = torch.float32
# M per output: the next power of two at or above twice the worst err_kernel / err_twin measured on an MI355X
M = {"spl.z_out": 4.0, "spl.acc": 8.0, "spl.dh": 16.0, "spl.dWp": 16.0, "spl.dbp": 16.0, "spl.dz_in": 16.0,
     "knot.y": 16.0, "knot.lad": 16.0, "inv.residual": 8.0, "inv.roundtrip": 8.0,
     "pre.x0": 2.0, "pre.dw": 2.0, "pre.db": 4.0, "pre.dz": 4.0, "pre.dg": 2.0,
     "ea.y": 2.0, "ea.y_noacc": 2.0, "ea.acc": 2.0, "ea.x_rev": 4.0, "ea.acc_rev": 2.0, "ea.roundtrip": 4.0, "ea.dx": 2.0, "ea.dls": 8.0, "ea.dtr": 4.0,
     "sdp.z": 16.0, "sdp.acc": 16.0, "sdp.dzq": 4.0, "nll.acc": 4.0, "nll.dz": 2.0}


def m_of(key):
    return M[key]


def _key(fam, k):
    return f"{fam}.{k}" if fam else k


def g(x):
    """a CPU tensor on the device"""
    return None if x is None else x.to(dev()).contiguous()


def guarded(prior):
    """a canary-guarded device buffer holding `prior` ([n] or [n, w] fp32)"""
    p = prior.reshape(prior.shape[0], -1)
    b = Guarded(p.shape[0], p.shape[1], F32)
    b.t.copy_(p)
    return b


def out(b, shape=None):
    v = b.t.detach().cpu()
    return v.reshape(shape) if shape is not None else v


# ------------------------------------------------------------------------------------------------ geometries
def _layout(R, utts):
    """utts: (first row, rows owned, first valid row, valid rows) per utterance, in row order; the last one owns the rest"""
    utt, mask = np.zeros(R, dtype=np.int32), np.zeros(R, dtype=np.float32)
    for b, (r0, n, v0, nv) in enumerate(utts):
        utt[r0:] = b
        mask[v0:v0 + nv] = 1
        assert r0 <= v0 and v0 + nv <= r0 + n <= R
    return torch.from_numpy(utt), torch.from_numpy(mask)


def _ragged(R, frames):
    """every utterance owns its frames and a 2-row halo on each side"""
    utts, r0 = [], 0
    for n in frames:
        utts.append((r0, n + 4, r0 + 2, n))
        r0 += n + 4
    assert r0 <= R
    return _layout(R, utts)


SPLINE_GEOMS = {
    "r31": lambda: _ragged(31, [10, 1, 8]),                  # one tile, not full; borders inside it (rows 14, 19); a one-frame utterance
    "r32": lambda: _ragged(32, [12, 12]),                    # exactly one tile
    "r33": lambda: _ragged(33, [24, 1]),                     # a second tile of one row, masked
    "r70": lambda: _ragged(70, [28, 20, 9]),                 # a border exactly at row 32: row 0 of tile 1 masked, the others valid; 1 trailing row
    "r128": lambda: _layout(128, [(0, 64, 2, 20), (64, 64, 66, 40)]),    # tile 1 (rows 32..63) fully masked; trailing masked rows
}
ELEM_GEOMS = {
    "e63": lambda: _layout(63, [(0, 40, 2, 36), (40, 23, 42, 19)]),                        # a border at row 40
    "e64": lambda: _layout(64, [(0, 20, 2, 16), (20, 21, 22, 17), (41, 23, 43, 19)]),      # three utterances inside one wave
    "e65": lambda: _layout(65, [(0, 64, 2, 60), (64, 1, 64, 1)]),                          # a border at row 64; lane 0 masked, the others valid
    "e257": lambda: _layout(257, [(0, 128, 2, 60), (128, 128, 130, 121), (256, 1, 256, 1)]),   # wave 1 has no valid row; a border at row 256
    "e300": lambda: _layout(300, [(0, 40, 2, 36), (40, 24, 42, 20), (64, 192, 66, 188), (256, 44, 258, 38)]),   # borders at 40, 64, 256
}


def test_geometries_hold_what_they_claim(built):
    u, m = SPLINE_GEOMS["r70"]()
    assert u[31] == 0 and u[32] == 1 and m[32] == 0 and m[34:52].all() and m[69] == 0
    u, m = SPLINE_GEOMS["r128"]()
    assert m[32:64].sum() == 0 and m[:32].sum() > 0 and m[106:].sum() == 0
    u, m = SPLINE_GEOMS["r33"]()
    assert m[32] == 0 and u[27] == 0 and u[28] == 1 and m[30] == 1 and m[31] == 0
    assert SPLINE_GEOMS["r31"]()[1][16] == 1 and SPLINE_GEOMS["r31"]()[1][15:18].tolist() == [0, 1, 0]
    u, m = ELEM_GEOMS["e65"]()
    assert m[0] == 0 and m[2:62].all() and u[63] == 0 and u[64] == 1 and m[64] == 1
    u, m = ELEM_GEOMS["e257"]()
    assert m[64:128].sum() == 0 and u[255] == 1 and u[256] == 2 and m[256] == 1
    u, m = ELEM_GEOMS["e64"]()
    assert len(set(u.tolist())) == 3
    u, m = ELEM_GEOMS["e300"]()
    assert [int(u[r]) for r in (39, 40, 63, 64, 255, 256)] == [0, 1, 1, 2, 2, 3] and m[296:].sum() == 0
    assert ELEM_GEOMS["e63"]()[0][39:41].tolist() == [0, 1]


# ------------------------------------------------------------------------------------------------ the rule
def errors(got, ref, twin):
    """per output: (err_kernel, err_twin), relative L2 against float64 over whole buffers"""
    return {k: (rel_l2(got[k].double(), ref[k]), rel_l2(twin[k].double(), ref[k])) for k in ref}


def limits(fam, ref, twin, floors=None):
    return {k: max(m_of(_key(fam, k)) * rel_l2(twin[k].double(), ref[k]), (floors or {}).get(k, rows64.AGG_F32)) for k in ref}


def hold(fam, case, got, ref, twin, floors=None):
    """print the figures of every output, then assert the rule"""
    lim, bad = limits(fam, ref, twin, floors), []
    for k, (ek, et) in errors(got, ref, twin).items():
        print(f"RATIO {_key(fam, k)} {case}: err_kernel {ek:.3e} err_twin {et:.3e} ratio {ek / max(et, 1e-300):.3f} limit {lim[k]:.3e}")
        if not ek <= lim[k]:
            bad.append((k, ek, et, lim[k]))
    assert not bad, (fam, case, bad)


def miss(fam, got, bad_ref, ref, twin, floors=None):
    """by how much each output misses its (true) limit against a reference with a planted defect"""
    lim = limits(fam, ref, twin, floors)
    return {k: rel_l2(got[k].double(), bad_ref[k]) / lim[k] for k in ref}


def seen(name, misses, among=None):
    worst = max(v for k, v in misses.items() if among is None or k in among)
    print("CONTROL", name, {k: float(f"{v:.3g}") for k, v in misses.items()})
    assert worst >= rows64.CONTROL_MISS, (name, misses)


def canaries(bufs):
    for k, b in bufs.items():
        if hasattr(b, "canaries_intact"):
            assert b.canaries_intact(), k


# ------------------------------------------------------------------------------------------------ spline inputs
NEAR_KNOT = 1e-5


def _f32_next(v, up):
    return float(np.nextafter(np.float32(v), np.float32(np.inf if up else -np.inf)))


def build_values(knots, valid, classes, gen):
    """searched values [R] fp32 for rows with knots [R, 11] (float64): the slots below on randomly chosen valid rows, class (a) elsewhere"""
    R = knots.shape[0]
    x = (torch.rand(R, generator=gen) * 12 - 6).float()
    slots = [("mid", j) for j in range(S.NB)] + [("val", v) for v in (-5.5, 5.5, -5.0, 5.0, 0.0, _f32_next(-5.0, False), _f32_next(5.0, True))]
    if "c" in classes:
        slots += [("knot", j, d) for j in range(1, S.NB) for d in (0, -1, 1)]
    rows = valid[torch.randperm(valid.numel(), generator=gen)].tolist()
    assert len(rows) >= 17, "a geometry needs 17 valid rows for the ten bins, the two tails and class (b)"
    for slot, r in zip(slots, rows):
        if slot[0] == "mid":
            x[r] = float((knots[r, slot[1]] + knots[r, slot[1] + 1]) / 2)
        elif slot[0] == "val":
            x[r] = slot[1]
        else:
            v = float(np.float32(float(knots[r, slot[1]])))
            x[r] = v if slot[2] == 0 else _f32_next(v, slot[2] > 0)
    return x


class SplineInputs:
    """operands of the three spline kernels for one geometry and one parameter scale s"""

    def __init__(self, gname, s, classes="ab", per_row_utt=False, seed=0):
        self.utt, self.mask = SPLINE_GEOMS[gname]()
        R = self.R = self.mask.numel()
        if per_row_utt:                                   # every row an utterance of its own: acc is then the per-row log|det|
            self.utt = torch.arange(R, dtype=torch.int32)
        self.B = int(self.utt.max()) + 1
        gen = torch.Generator().manual_seed(7000 + seed + 31 * list(SPLINE_GEOMS).index(gname) + int(1000 * s))
        rn = lambda *sh: torch.randn(*sh, generator=gen)                                        # noqa: E731
        self.h = rn(R, C)
        std = torch.full((S.NPAR,), float(s))
        std[20:] = s / math.sqrt(C) * torch.tensor([1.0, 8.0] * 5)[:9]
        self.Wp, self.bp = rn(S.NPAR, C) * std[:, None], rn(S.NPAR) * 0.5
        self.valid = torch.nonzero(self.mask).reshape(-1)
        self.par64, self.parS = S.proj_params(self.h, self.Wp, self.bp, self.mask)
        uw, uh, _ = S.split_params(self.par64, C)
        kw, kh = S.knots(uw), S.knots(uh)
        x = build_values(kw, self.valid, classes, gen)
        self.replaced = 0
        if "c" not in classes:                            # the backward's condition: no row within NEAR_KNOT of an interior knot
            dist = (x.double()[:, None] - kw[:, 1:-1]).abs().min(-1).values
            near = (dist < NEAR_KNOT) & (x.abs() <= S.TAIL) & (self.mask != 0)
            k = S._bin(x.double(), kw)[:, None]
            mid = ((kw.gather(1, k) + kw.gather(1, k + 1)) / 2)[:, 0].float()
            x = torch.where(near, mid, x)
            self.replaced = int(near.sum())
        self.z_in = torch.stack([rn(R), x], 1)
        self.y_inv = torch.stack([rn(R), build_values(kh, self.valid, "abc", gen)], 1)
        self.dz_out, self.gacc, self.acc0 = rn(R, 2), rn(self.B), rn(self.B)
        self.dWp0, self.dbp0 = rn(S.NPAR, C), rn(S.NPAR)
        self.d = types.SimpleNamespace(**{n: g(getattr(self, n)) for n in ("utt", "mask", "h", "Wp", "bp", "z_in", "y_inv", "dz_out", "gacc")})


def spline_fwd_kernel(I, sign, flip, z_in=None):
    from glow_tts_amd._lib import call
    o = dict(z_out=Guarded(I.R, 2, F32), par=Guarded(I.R, 32, F32), acc=guarded(I.acc0))
    call.gt_convflow_spline_fwd(I.d.h, I.d.Wp, I.d.bp, I.d.z_in if z_in is None else z_in, I.d.mask, I.d.utt, o["z_out"].t, o["par"].t, o["acc"].t,
                                float(sign), int(flip), I.R, C, _st())
    return o


def spline_bwd_kernel(I, par, sign, flip, partials=False):
    from glow_tts_amd import _lib
    from glow_tts_amd._lib import call
    o = dict(dh=Guarded(I.R, C, F32), dWp=guarded(I.dWp0), dbp=guarded(I.dbp0), dz_in=Guarded(I.R, 2, F32))
    if partials:
        n, w = call.gt_convflow_spline_partial_rows(I.R), call.gt_convflow_spline_partial_width()
        assert n == (I.R + 31) // 32 and w == S.NPAR * C + S.NPAR
        o["partials"] = Guarded(n, w, F32)
        o["partials"].t.fill_(float("nan"))
    call.gt_convflow_spline_bwd(I.d.h, I.d.Wp, par, I.d.z_in, I.d.dz_out, I.d.gacc, I.d.mask, I.d.utt, o["dh"].t, None if partials else o["dWp"].t,
                                None if partials else o["dbp"].t, o["partials"].t if partials else None, o["dz_in"].t, float(sign), int(flip), I.R, C, _st())
    if partials:
        o["partials_after"] = o["partials"].t.clone()
        args = _lib.PartialsArgs()
        j = args.job[0]
        j.partials, j.dst_a, j.dst_b, j.n_rows, j.Ca, j.Cb = o["partials"].t.data_ptr(), o["dWp"].t.data_ptr(), o["dbp"].t.data_ptr(), n, S.NPAR * C, S.NPAR
        args.n_jobs = 1
        call.gt_param_partials_reduce(args, _st())
    return o


def spline_inv_kernel(I, z_in):
    from glow_tts_amd._lib import call
    o = dict(z_out=Guarded(I.R, 2, F32))
    call.gt_convflow_spline_inv(I.d.h, I.d.Wp, I.d.bp, z_in, I.d.mask, o["z_out"].t, I.R, C, _st())
    return o


def fwd_ref(I, sign, flip, dtype, utt=None, acc0=None, defect=None, z_in=None):
    par, _ = S.proj_params(I.h, I.Wp, I.bp, I.mask, dtype=dtype)
    z_out, acc, info = S.convflow_spline_fwd(par, I.z_in if z_in is None else z_in, I.mask, I.utt if utt is None else utt,
                                             I.acc0 if acc0 is None else acc0, sign, flip, C, dtype=dtype, defect=defect)
    return {"z_out": z_out, "acc": acc}, info


def bwd_ref(I, par, sign, flip, dtype, utt=None, zero_prior=False, defect=None):
    dh, dWp, dbp, dz_in, gp = S.convflow_spline_bwd(I.h, I.Wp, par, I.z_in, I.dz_out, I.gacc, I.mask, I.utt if utt is None else utt,
                                                    torch.zeros_like(I.dWp0) if zero_prior else I.dWp0,
                                                    torch.zeros_like(I.dbp0) if zero_prior else I.dbp0, sign, flip, C, dtype=dtype, defect=defect)
    return {"dh": dh, "dWp": dWp, "dbp": dbp, "dz_in": dz_in}, gp


SPLINE_S = (0.05, 1.0, 2.0)
SIGN_FLIP = ((-1.0, 1), (1.0, 0), (-1.0, 0), (1.0, 1))         # production passes (-1, 1) only
SPLINE_CASES = [(gname, s, *SIGN_FLIP[(i + j) % 4]) for i, gname in enumerate(SPLINE_GEOMS) for j, s in enumerate(SPLINE_S)]


@functools.lru_cache(maxsize=None)
def run_spline(gname, s, sign, flip):
    I = SplineInputs(gname, s)
    f = spline_fwd_kernel(I, sign, flip)
    b = spline_bwd_kernel(I, f["par"].t, sign, flip)
    bp = spline_bwd_kernel(I, f["par"].t, sign, flip, partials=True)
    inv = spline_inv_kernel(I, I.d.y_inv)
    y_k = f["z_out"].t.flip(1).contiguous() if flip else f["z_out"].t.contiguous()          # [z0, y] again
    rt = spline_inv_kernel(I, y_k)
    torch.cuda.synchronize()
    canaries({**f, **{"b." + k: v for k, v in b.items()}, **{"p." + k: v for k, v in bp.items()}, "inv": inv["z_out"], "rt": rt["z_out"]})
    par = out(f["par"])
    r = types.SimpleNamespace(I=I, sign=sign, flip=flip, par=par, y_k=y_k.cpu())
    r.fwd = {"z_out": out(f["z_out"]), "acc": out(f["acc"], (-1,))}
    r.bwd = {"dh": out(b["dh"]), "dWp": out(b["dWp"]), "dbp": out(b["dbp"], (-1,)), "dz_in": out(b["dz_in"])}
    r.bwd_p = {"dh": out(bp["dh"]), "dWp": out(bp["dWp"]), "dbp": out(bp["dbp"], (-1,)), "dz_in": out(bp["dz_in"])}
    r.partials = bp["partials_after"].cpu()
    r.inv, r.rt = out(inv["z_out"]), out(rt["z_out"])
    r.fwd_ref, r.info = fwd_ref(I, sign, flip, torch.float64)
    r.fwd_twin, _ = fwd_ref(I, sign, flip, F32)
    r.bwd_ref, r.gp = bwd_ref(I, par, sign, flip, torch.float64)
    r.bwd_twin, _ = bwd_ref(I, par, sign, flip, F32)
    return r


def _covers_all_bins(info, valid):
    bins = set(info.bin[valid].tolist())
    assert set(range(-1, S.NB + 1)) <= bins, sorted(bins)


@pytest.mark.parametrize("gname,s,sign,flip", SPLINE_CASES)
def test_spline_forward_against_float64(built, gname, s, sign, flip):
    r = run_spline(gname, s, sign, flip)
    I, case = r.I, f"{gname} s={s} sign={sign:+.0f} flip={flip}"
    _covers_all_bins(r.info, I.valid)
    on, off = I.mask != 0, I.mask == 0
    # params: the exact-fp32 29-row product, elementwise; columns 29..31 and masked rows are zero
    assert float(r.par[:, S.NPAR:].abs().max()) == 0 and float(r.par[off].abs().max()) == 0
    rep = rows64.check(f"params {case}", r.par, I.par64, rows64.gamma(C) * I.parS)
    print(rep)
    assert rep.worst <= 1.0, str(rep)
    if s == 2.0:
        assert (I.par64[on][:, 20:S.NPAR].abs() > 20).any(), "no raw derivative parameter reaches the softplus switch"
    # exact properties: the pass-through channel, the tails, masked rows
    y_col, p_col = (0, 1) if flip else (1, 0)
    z = r.fwd["z_out"]
    assert float(z[off].abs().max()) == 0
    assert torch.equal(z[on][:, p_col], I.z_in[on][:, 0])
    tail = on & ~r.info.inside
    assert int(tail.sum()) >= 4 and torch.equal(z[tail][:, y_col], I.z_in[tail][:, 1])
    hold("spl", case, r.fwd, r.fwd_ref, r.fwd_twin)


@pytest.mark.parametrize("gname,s,sign,flip", SPLINE_CASES)
def test_spline_backward_against_float64(built, gname, s, sign, flip):
    r = run_spline(gname, s, sign, flip)
    I, case = r.I, f"{gname} s={s} sign={sign:+.0f} flip={flip}"
    assert I.replaced <= 0.005 * I.valid.numel(), (I.replaced, I.valid.numel())
    _, info = fwd_ref(I, sign, flip, torch.float64)
    _covers_all_bins(info, I.valid)
    assert float(info.knot_dist[(I.mask != 0) & info.inside].min()) >= NEAR_KNOT
    on, off = I.mask != 0, I.mask == 0
    tail = on & ~info.inside
    gy_col, p_col = (0, 1) if flip else (1, 0)
    for b in (r.bwd, r.bwd_p):
        assert float(b["dz_in"][off].abs().max()) == 0 and float(b["dh"][off].abs().max()) == 0
        assert torch.equal(b["dz_in"][tail][:, 1], I.dz_out[tail][:, gy_col])             # a tail's slope is exactly 1 ...
        assert float(b["dh"][tail].abs().max()) == 0 and float(r.gp[tail].abs().max()) == 0   # ... and its parameters get no gradient
        assert torch.equal(b["dz_in"][on][:, 0], I.dz_out[on][:, p_col])
    hold("spl", case, r.bwd, r.bwd_ref, r.bwd_twin)
    # the partial-row form: every partial written (the buffer started as NaN), the same results after the reduce
    assert torch.isfinite(r.partials).all()
    hold("spl", case + " partial rows", r.bwd_p, r.bwd_ref, r.bwd_twin)


@pytest.mark.parametrize("gname,s,sign,flip", SPLINE_CASES)
def test_spline_inverse_by_its_residual(built, gname, s, sign, flip):
    """the inverse is ill-conditioned where dy/dx is small (torch's float32 inverse itself is off by 0.5 at s = 2), so it is judged by its
    residual |RQS64(x_kernel) - y| against the float32 twin's on the same y, maximum over the valid rows inside [-5, 5]:
    res_kernel <= max(M res_twin, 2^-22 max|y|); the forward error is printed only"""
    r = run_spline(gname, s, sign, flip)
    I, case = r.I, f"{gname} s={s}"
    on, off = I.mask != 0, I.mask == 0
    par32, _ = S.proj_params(I.h, I.Wp, I.bp, I.mask, dtype=F32)
    bad = []
    for name, y_in, got in (("inv.residual", I.y_inv, r.inv), ("inv.roundtrip", r.y_k, r.rt)):
        ref, info = S.convflow_spline_inv(I.par64, y_in, I.mask)
        twin, _ = S.convflow_spline_inv(par32, y_in, I.mask, dtype=F32)
        if name == "inv.residual":
            bins = set(info.bin[I.valid].tolist())
            assert set(range(-1, S.NB + 1)) <= bins, sorted(bins)
        sel = on & info.inside
        tail = on & ~info.inside
        assert float(got[off].abs().max()) == 0
        assert torch.equal(got[on][:, 0], y_in[on][:, 0]) and torch.equal(got[tail][:, 1], y_in[tail][:, 1])
        rk = float(S.inv_residual(I.par64, got[:, 1], y_in[:, 1])[sel].max())
        rt = float(S.inv_residual(I.par64, twin[:, 1], y_in[:, 1])[sel].max())
        lim = max(m_of(name) * rt, 2.0 ** -22 * float(y_in[:, 1].abs().max()))
        print(f"RATIO {name} {case}: err_kernel {rk:.3e} err_twin {rt:.3e} ratio {rk / max(rt, 1e-300):.3f} limit {lim:.3e}; forward error: "
              f"kernel {float((got[:, 1].double() - ref[:, 1])[sel].abs().max()):.3e} twin {float((twin[:, 1].double() - ref[:, 1])[sel].abs().max()):.3e}")
        if not rk <= lim:
            bad.append((name, rk, rt, lim))
    assert float((r.rt[:, 1] - I.z_in[:, 1])[on & ~r.info.inside].abs().max()) == 0           # a tail's round trip is exact
    assert not bad, (case, bad)


KNOT_CASES = [("r70", 0.05), ("r70", 1.0), ("r128", 2.0)]


@pytest.mark.parametrize("gname,s", KNOT_CASES)
def test_spline_forward_at_the_knots(built, gname, s):
    """class (c): x on the float64 interior knots rounded to fp32 and on their two fp32 neighbours.  Every row is an utterance of its own,
    so acc holds the per-row log|det|.  The spline is C1 at a knot, so either neighbouring bin is acceptable: elementwise
    |got - ref| <= M max(twin's error, 2^-22 max(1, slope)) for y and for log|det|, with `ref` the float64 value of the searched bin's
    piece or of the piece across the knot, whichever is nearer (the kernel's fp32 knots differ from the float64 ones by an fp32 step or
    two, so an x that close to a knot may be searched into either bin; log|det| is only C0 there: its slope y'' / y' jumps, by up to
    1e5 at s = 2, and the two pieces differ by that jump times the distance to the knot).  The twin's error is taken the same way."""
    I = SplineInputs(gname, s, classes="abc", per_row_utt=True, seed=1)
    I.acc0 = torch.zeros(I.B)
    f = spline_fwd_kernel(I, 1.0, 0)
    torch.cuda.synchronize()
    canaries(f)
    ref, info = fwd_ref(I, 1.0, 0, torch.float64)
    twin, _ = fwd_ref(I, 1.0, 0, F32)
    alt = S.convflow_spline_fwd(I.par64, I.z_in, I.mask, I.utt, I.acc0, 1.0, 0, C, other_bin=True)
    on = I.mask != 0
    at_knot = on & info.inside & (info.knot_dist <= 2.0 ** -20)
    assert int(at_knot.sum()) >= min(27, I.valid.numel() - 17), int(at_knot.sum())
    slope = info.slope.clamp_min(1.0)
    bad = []
    for key, got, rf, ra, tw in (("knot.y", out(f["z_out"])[:, 1], ref["z_out"][:, 1], alt[0][:, 1], twin["z_out"][:, 1]),
                                 ("knot.lad", out(f["acc"], (-1,)), ref["acc"], alt[1], twin["acc"])):
        def err_of(v):
            e = (v.double() - rf).abs()
            return torch.where(at_knot, torch.minimum(e, (v.double() - ra).abs()), e)
        err, unit = err_of(got), torch.maximum(err_of(tw), 2.0 ** -22 * slope)
        w = int((err / unit)[at_knot].argmax())
        print(f"KNOT {key} {gname} s={s}: worst ratio at a knot {float((err / unit)[at_knot].max()):.3f} (err {float(err[at_knot][w]):.3e}, "
              f"slope {float(info.slope[at_knot][w]):.3e}; against the searched bin alone {float(((got.double() - rf).abs() / unit)[at_knot].max()):.3f}), "
              f"off the knots {float((err / unit)[on & ~at_knot].max()):.3f}, M {m_of(key):g}")
        if not bool((err <= m_of(key) * unit)[at_knot].all()):              # the rows off the knots answer to the aggregate rule
            bad.append((key, float((err / unit)[at_knot].max())))
    assert not bad, bad


SPLINE_DEFECT_CASE = ("r70", 1.0, -1.0, 1)


@pytest.mark.parametrize("defect", ["no_2_over_delta", "far_bins_forgotten", "end_der_free", "flip_ignored", "acc_overwritten", "border_row_to_neighbour"])
def test_spline_planted_defects_are_seen(built, defect):
    gname, s, sign, flip = SPLINE_DEFECT_CASE
    r = run_spline(gname, s, sign, flip)
    I = r.I
    kw_f, kw_b = {}, {}
    if defect in ("no_2_over_delta", "end_der_free", "far_bins_forgotten"):
        kw_f = kw_b = {"defect": defect}
    elif defect == "acc_overwritten":
        kw_f, kw_b = {"acc0": torch.zeros_like(I.acc0)}, {"zero_prior": True}
    elif defect == "border_row_to_neighbour":
        bad_utt = S.credit_neighbour(I.utt, I.mask)
        assert int((bad_utt != I.utt.long()).sum()) == I.B - 1
        kw_f = kw_b = {"utt": bad_utt}
    f2 = flip ^ 1 if defect == "flip_ignored" else flip
    mb = miss("spl", r.bwd, bwd_ref(I, r.par, sign, f2, torch.float64, **kw_b)[0], r.bwd_ref, r.bwd_twin)
    seen(defect + " (backward)", mb)
    if defect != "far_bins_forgotten":                    # a defect of the gradient alone
        mf = miss("spl", r.fwd, fwd_ref(I, sign, f2, torch.float64, **kw_f)[0], r.fwd_ref, r.fwd_twin)
        seen(defect + " (forward)", mf)
    mp = miss("spl", r.bwd_p, bwd_ref(I, r.par, sign, f2, torch.float64, **kw_b)[0], r.bwd_ref, r.bwd_twin)
    seen(defect + " (backward, partial rows)", mp)


# ------------------------------------------------------------------------------------------------ gt_convflow_pre_fwd / bwd
PRE_CASES = [("r31", 2, "g1g2", True, True), ("r33", 1, "none", False, False), ("r70", 2, "g1", True, False), ("r128", 1, "g1", True, True),
             ("r32", 2, "none", False, True)]


@functools.lru_cache(maxsize=None)
def run_pre(gname, ldz, cond, with_dz, with_dg):
    from glow_tts_amd._lib import call
    utt, mask = SPLINE_GEOMS[gname]()
    R = mask.numel()
    gen = torch.Generator().manual_seed(8000 + 7 * list(SPLINE_GEOMS).index(gname) + ldz)
    rn = lambda *sh: torch.randn(*sh, generator=gen)                                            # noqa: E731
    I = types.SimpleNamespace(R=R, mask=mask, z=rn(R, ldz) * 2, w=rn(C, 1, 1), b=rn(C), g1=rn(R, C) if cond != "none" else None,
                              g2=rn(R, C) if cond == "g1g2" else None, dx0=rn(R, C), dw0=rn(C), db0=rn(C), dz0=rn(R, ldz) if with_dz else None,
                              dg0=rn(R, C) if with_dg else None)
    x0 = Guarded(R, C, F32)
    d = types.SimpleNamespace(**{k: g(v) for k, v in vars(I).items() if isinstance(v, torch.Tensor)})
    call.gt_convflow_pre_fwd(d.z, ldz, d.w, d.b, g(I.g1), g(I.g2), d.mask, x0.t, R, C, _st())
    o = dict(dw=guarded(I.dw0), db=guarded(I.db0))
    if with_dz:
        o["dz"] = guarded(I.dz0)
    if with_dg:
        o["dg"] = guarded(I.dg0)
    call.gt_convflow_pre_bwd(d.dx0, d.z, ldz, d.w, d.mask, o["dw"].t, o["db"].t, o["dz"].t if with_dz else None, ldz, o["dg"].t if with_dg else None,
                             R, C, _st())
    torch.cuda.synchronize()
    canaries({"x0": x0, **o})
    got = {"x0": out(x0), "dw": out(o["dw"], (-1,)), "db": out(o["db"], (-1,))}
    dz_full = out(o["dz"]) if with_dz else None
    if with_dz:
        got["dz"] = dz_full[:, 0]
    if with_dg:
        got["dg"] = out(o["dg"])

    def ref(dtype, zero_prior=False):
        zp = (lambda t: None if t is None else torch.zeros_like(t)) if zero_prior else (lambda t: t)
        dw, db, dz, dg = S.convflow_pre_bwd(I.dx0, I.z[:, 0], I.w, I.mask, zp(I.dw0), zp(I.db0), None if I.dz0 is None else zp(I.dz0[:, 0]), zp(I.dg0), dtype=dtype)
        v = {"x0": S.convflow_pre_fwd(I.z[:, 0], I.w, I.b, I.g1, I.g2, I.mask, dtype=dtype), "dw": dw, "db": db}
        if with_dz:
            v["dz"] = dz
        if with_dg:
            v["dg"] = dg
        return v
    return types.SimpleNamespace(I=I, got=got, dz_full=dz_full, ref=ref)


@pytest.mark.parametrize("gname,ldz,cond,with_dz,with_dg", PRE_CASES)
def test_convflow_pre_against_float64(built, gname, ldz, cond, with_dz, with_dg):
    r = run_pre(gname, ldz, cond, with_dz, with_dg)
    I, case = r.I, f"{gname} ldz={ldz} cond={cond} dz={int(with_dz)} dg={int(with_dg)}"
    off = I.mask == 0
    assert float(r.got["x0"][off].abs().max()) == 0
    if with_dz:
        assert torch.equal(r.got["dz"][off], I.dz0[off][:, 0])                      # masked rows keep what they held
        if ldz == 2:
            assert torch.equal(r.dz_full[:, 1], I.dz0[:, 1])                        # the other column is not this kernel's
    if with_dg:
        assert torch.equal(r.got["dg"][off], I.dg0[off])
    ref, twin = r.ref(torch.float64), r.ref(F32)
    hold("pre", case, r.got, ref, twin)
    seen("pre: destinations overwritten " + case, miss("pre", r.got, r.ref(torch.float64, zero_prior=True), ref, twin))


# ------------------------------------------------------------------------------------------------ the elementwise kernels on [R, 2]
SDP_W = (0.0, 1.0, 2.0, 7.0)
SDP_ZU = (0.0, 3.0, -3.0, 25.0, -25.0)


@functools.lru_cache(maxsize=None)
def run_elem(gname):
    from glow_tts_amd._lib import call
    utt, mask = ELEM_GEOMS[gname]()
    R, B = mask.numel(), int(utt.max()) + 1
    gen = torch.Generator().manual_seed(9000 + list(ELEM_GEOMS).index(gname))
    rn = lambda *sh: torch.randn(*sh, generator=gen)                                            # noqa: E731
    I = types.SimpleNamespace(R=R, B=B, utt=utt, mask=mask, x=rn(R, 2) * 2, ls=torch.tensor([[0.3], [-0.5]]) + 0.1 * rn(2, 1), tr=rn(2, 1), dy=rn(R, 2),
                              gacc=rn(B), acc0=rn(B), dls0=rn(2, 1), dtr0=rn(2, 1), eq=rn(R, 2))
    # the duration predictor's middle: every (w, z_u) of SDP_W x SDP_ZU on the valid rows, in turn
    i = torch.cumsum(mask, 0).long() - 1
    I.w = torch.tensor(SDP_W)[(i + 1) % 4] * mask + rn(R).abs() * (1 - mask)
    I.zq = torch.stack([torch.tensor(SDP_ZU)[(i // 4) % 5], rn(R)], 1)
    d = types.SimpleNamespace(**{k: g(v) for k, v in vars(I).items() if isinstance(v, torch.Tensor)})
    st = _st()
    k = {}
    # ElementwiseAffine: forward with and without acc, reverse on the forward's output, backward
    k["ea.y"], k["ea.acc"] = Guarded(R, 2, F32), guarded(I.acc0)
    call.gt_ea_fwd(d.x, d.ls, d.tr, d.mask, d.utt, k["ea.y"].t, k["ea.acc"].t, -1.0, 0, R, st)
    k["ea.y_noacc"] = Guarded(R, 2, F32)
    call.gt_ea_fwd(d.x, d.ls, d.tr, d.mask, d.utt, k["ea.y_noacc"].t, None, 1.0, 0, R, st)
    k["ea.x_rev"], k["ea.acc_rev"] = Guarded(R, 2, F32), guarded(I.acc0)
    call.gt_ea_fwd(d.x, d.ls, d.tr, d.mask, d.utt, k["ea.x_rev"].t, k["ea.acc_rev"].t, 1.0, 1, R, st)
    k["ea.roundtrip"] = Guarded(R, 2, F32)
    call.gt_ea_fwd(k["ea.y"].t, d.ls, d.tr, d.mask, d.utt, k["ea.roundtrip"].t, None, 1.0, 1, R, st)
    k["ea.dx"], k["ea.dls"], k["ea.dtr"] = Guarded(R, 2, F32), guarded(I.dls0), guarded(I.dtr0)
    call.gt_ea_bwd(d.x, d.ls, d.dy, d.gacc, d.mask, d.utt, k["ea.dx"].t, k["ea.dls"].t, k["ea.dtr"].t, -1.0, R, st)
    k["sdp.z"], k["sdp.acc"], k["sdp.dzq"] = Guarded(R, 2, F32), guarded(I.acc0), Guarded(R, 2, F32)
    call.gt_sdp_mid_fwd(d.zq, d.w, d.eq, d.mask, d.utt, k["sdp.z"].t, k["sdp.acc"].t, R, st)
    call.gt_sdp_mid_bwd(d.zq, d.w, d.dy, d.gacc, d.mask, d.utt, k["sdp.dzq"].t, R, st)
    k["nll.acc"], k["nll.dz"] = guarded(I.acc0), Guarded(R, 2, F32)
    call.gt_nll_gauss_fwd(d.x, d.mask, d.utt, k["nll.acc"].t, R, st)
    call.gt_nll_gauss_bwd(d.x, d.gacc, d.mask, d.utt, k["nll.dz"].t, R, st)
    torch.cuda.synchronize()
    canaries(k)
    flat = ("acc", "dls", "dtr")
    got = {n: out(b, (-1,)) if n.split(".")[1].startswith(flat) else out(b) for n, b in k.items()}
    return types.SimpleNamespace(I=I, got=got)


def elem_ref(I, dtype, utt=None, zero_prior=False, y_fwd=None):
    """every output of run_elem by oracle/spline64.py; y_fwd: the kernel's own forward output, the operand of the round trip"""
    utt = I.utt if utt is None else utt
    zp = (lambda t: torch.zeros_like(t)) if zero_prior else (lambda t: t)
    v = {}
    v["ea.y"], v["ea.acc"] = S.ea_fwd(I.x, I.ls, I.tr, I.mask, utt, zp(I.acc0), -1.0, 0, dtype=dtype)
    v["ea.y_noacc"] = v["ea.y"]
    v["ea.x_rev"], v["ea.acc_rev"] = S.ea_fwd(I.x, I.ls, I.tr, I.mask, utt, zp(I.acc0), 1.0, 1, dtype=dtype)
    v["ea.roundtrip"] = S.ea_fwd(y_fwd, I.ls, I.tr, I.mask, utt, None, 1.0, 1, dtype=dtype)[0]
    v["ea.dx"], v["ea.dls"], v["ea.dtr"] = S.ea_bwd(I.x, I.ls, I.dy, I.gacc, I.mask, utt, zp(I.dls0), zp(I.dtr0), -1.0, dtype=dtype)
    v["sdp.z"], v["sdp.acc"] = S.sdp_mid_fwd(I.zq, I.w, I.eq, I.mask, utt, zp(I.acc0), dtype=dtype)
    v["sdp.dzq"] = S.sdp_mid_bwd(I.zq, I.w, I.dy, I.gacc, I.mask, utt, dtype=dtype)
    v["nll.acc"] = S.nll_gauss_fwd(I.x, I.mask, utt, zp(I.acc0), dtype=dtype)
    v["nll.dz"] = S.nll_gauss_bwd(I.x, I.gacc, I.mask, utt, dtype=dtype)
    return v


@pytest.mark.parametrize("gname", list(ELEM_GEOMS))
def test_elementwise_kernels_against_float64(built, gname):
    r = run_elem(gname)
    I, got = r.I, r.got
    on, off = I.mask != 0, I.mask == 0
    for n in ("ea.y", "ea.y_noacc", "ea.x_rev", "ea.roundtrip", "ea.dx", "sdp.z", "sdp.dzq", "nll.dz"):
        assert float(got[n][off].abs().max()) == 0, n
    assert torch.equal(got["ea.y"], got["ea.y_noacc"])
    assert torch.equal(got["sdp.z"][:, 1], I.zq[:, 1] * I.mask) and torch.equal(got["sdp.dzq"][:, 1], I.dy[:, 1] * I.mask)
    ref, twin = elem_ref(I, torch.float64, y_fwd=got["ea.y"]), elem_ref(I, F32, y_fwd=got["ea.y"])
    # reverse(forward(x)) comes back to x (the reference of ea.roundtrip is the exact inverse of the kernel's own y)
    assert rel_l2(got["ea.roundtrip"].double(), (I.x * I.mask[:, None]).double()) <= max(
        m_of("ea.roundtrip") * rel_l2(twin["ea.roundtrip"].double(), (I.x * I.mask[:, None]).double()), rows64.AGG_F32)
    # the duration predictor's middle: both sides of the clamp and the saturated sigmoid are reached; no gradient through the clamp
    z0 = I.w.double() - torch.sigmoid(I.zq[:, 0].double())
    clamped = on & (z0 < 1e-5)
    assert int(clamped.sum()) >= 5 and int((on & (z0 > 1e-5)).sum()) >= 5 and set(I.zq[on][:, 0].tolist()) == set(SDP_ZU)
    assert float((z0[on] - 1e-5).abs().min()) > 1e-6                      # no row where fp32 and float64 could clamp differently
    assert float((got["sdp.z"][clamped][:, 0].double() - math.log(1e-5)).abs().max()) <= 2.0 ** -19      # logf to 2 ulp of 11.5
    ga = I.gacc[I.utt.long()].double()
    through = -ga * (1 - 2 * torch.sigmoid(I.zq[:, 0].double()))          # what is left of d z_u when the clamp passes nothing
    assert float(((got["sdp.dzq"][:, 0].double() - through).abs() - 4 * rows64.FAST_FN * ga.abs())[clamped].max()) <= 0
    hold("", gname, got, ref, twin)
    # planted defects: destinations overwritten; a border row credited to the neighbouring utterance
    acc_like = ("ea.acc", "ea.acc_rev", "ea.dls", "ea.dtr", "sdp.acc", "nll.acc")
    m0 = miss("", got, elem_ref(I, torch.float64, zero_prior=True, y_fwd=got["ea.y"]), ref, twin)
    print("CONTROL overwritten", gname, {k: float(f"{v:.3g}") for k, v in m0.items()})
    assert all(m0[k] >= rows64.CONTROL_MISS for k in acc_like), m0
    m1 = miss("", got, elem_ref(I, torch.float64, utt=S.credit_neighbour(I.utt, I.mask), y_fwd=got["ea.y"]), ref, twin)
    print("CONTROL border row", gname, {k: float(f"{v:.3g}") for k, v in m1.items()})
    assert all(m1[k] >= rows64.CONTROL_MISS for k in ("ea.acc", "ea.acc_rev", "ea.dls", "sdp.acc", "sdp.dzq", "nll.acc", "nll.dz")), m1
