"""The five per-op DDSConv kernels of csrc/predictor_ops.hip (gt_dds_sep_fwd, gt_dds_out_fwd, gt_dds_out_bwd, gt_dds_sep_bwd,
gt_dds_dw_bwd: the default path of the three stochastic predictors) and gt_rows_split3 through the C-ABI, each on its OWN operands
against its float64 restatement (oracle/dds64.py): sep_bwd gets a random d a1, out_* a random h2, dw_bwd a random d h1 and dy, so no
GEMM sits between a kernel and its check.

The rules (DESIGN.md 4.6.3 holds the measured figures).
  Nonlinear kernels (sep_fwd, out_fwd, out_bwd, sep_bwd): for every output, relative L2 against float64 over the WHOLE buffer, masked
  rows included,
      err_kernel <= max(M * err_twin, floor)          floor = rows64.AGG_F32 for every output
  err_twin being the same operator in torch float32 on the CPU on the same operands (a1 and d h2 are bf16 pairs hi + lo on both sides:
  the twin's fp32 values are stored as such a pair too, which carries 2^-17).  M is measured on an MI355X: the next power of two at or
  above twice the worst err_kernel / err_twin, never above 16 (the dictionary M below).
  gt_dds_dw_bwd is linear: rows64.check elementwise, |got - ref| <= gamma(K) S + 2^-24 |ref| with S the absolute-value twin of the
  sum, K = 4 for dx and valid rows + 1 for dw / db (the destinations start from non-zero priors), plus the aggregate.
  Exact: the two hi copies of a1 and of d h2 agree, out_bf16 == bf16(out), masked rows of every row output are 0, every canary row
  and every pad column is intact, gt_rows_split3 equals dds64.split3 bit for bit in its four forms, row outputs are bit-equal between
  the atomics and the partial-row forms.
  Partial rows: each backward also runs with a [gt_dds_bwd_partial_rows(R)][W] buffer that starts as NaN and NULL gradient pointers,
  reduced by gt_param_partials_reduce (dw: one job with Ca = 3 C, Cb = C); the result obeys the same float64 rule and agrees with the
  atomics form to 1e-5 relative.
  Controls: the same comparisons must miss their true limit by >= rows64.CONTROL_MISS against references with one planted defect each.

Geometries (oracle/dds64.py GEOMS; a workgroup is 4 waves x 2 rows = 8 rows): R = 7 (one utterance, all valid, no halo: only the range
guard stops a tap; wave 3 has one row), 8 (one workgroup; 3, 1 and 4 frames back to back: only `utt` decides at d = 1 and 3), 9 (a second
workgroup of one masked row), 33 (2-row halos; 10, 1 and 9 frames; a trailing row), 70 (a border on a workgroup edge with a valid row on
each side, an utterance longer than 3 workgroups, a fully masked last workgroup).  In r8, r33 and r70 x is a column window of an
[R, 256] buffer whose other columns are NaN; in r33 gt_dds_sep_fwd runs with lda = 3 C + 8."""
import functools
import types

import numpy as np
import pytest
import torch

from oracle import dds64 as D
from oracle import rows64
from test_dds64 import split3_inputs
from test_dds_layer_gpu import Guarded, _st, dev, rel_l2
from test_predictor_rows_fp64_gpu import canaries, g, guarded, out, seen

pytestmark = pytest.mark.gpu

C = D.C
EPS = 1e-5
SEED = 4242
SEED_WORD = 0x9E3779B9
F32, BF16 = torch.float32, torch.bfloat16
LDX_WIDE, X_COL0 = 256, 33          # where x is a window: columns 33 .. 224 of a 256-wide buffer
_layout = D.layout

# M per output: the next power of two at or above twice the worst err_kernel / err_twin measured on an MI355X
# worst measured ratios over the 30 cases, both forms: a1 1.001, out 1.059, d h2 1.002, d gamma2 1.180, d beta2 1.085, d h1 1.130,
# d gamma1 1.133, d beta1 1.034; twice each lies in (2, 4]
M = {"sep.a1": 4.0, "out.out": 4.0, "outb.dh2": 4.0, "outb.dgamma": 4.0, "outb.dbeta": 4.0, "sepb.dh1": 4.0, "sepb.dgamma": 4.0,
     "sepb.dbeta": 4.0}
NONLINEAR = tuple(M)
FAMILY = {"sep": ("sep.a1",), "out": ("out.out",), "outb": ("outb.dh2", "outb.dgamma", "outb.dbeta"),
          "sepb": ("sepb.dh1", "sepb.dgamma", "sepb.dbeta"), "dw": ("dw.dx", "dw.dw", "dw.db")}

GEOMS = tuple(D.GEOMS)
CASES = [(gname, d, p, (i + j + k) % 2 == 1) for i, gname in enumerate(GEOMS) for j, d in enumerate((1, 3, 9)) for k, p in enumerate((0.0, 0.5))]
CONTROL_CASE = ("r70", 9, 0.5, True)
assert CONTROL_CASE in CASES


def test_geometries_hold_what_they_claim(built):
    D.geometry_claims()
    assert set(D.WIDE_X) <= set(GEOMS) and D.PADDED_A1 in GEOMS and X_COL0 + C <= LDX_WIDE


def test_partial_rows_are_one_per_workgroup(built):
    from glow_tts_amd._lib import call
    for R in [D.GEOMS[n]()[1].numel() for n in GEOMS] + [1, 16, 17, 17800]:
        assert call.gt_dds_bwd_partial_rows(R) == -(-R // D.WG), R
    for R in (0, -1, -8, -(2 ** 31)):
        assert call.gt_dds_bwd_partial_rows(R) == 0, R


# ------------------------------------------------------------------------------------------------ the kernels
def nan_partials(R, width):
    from glow_tts_amd._lib import call
    n = call.gt_dds_bwd_partial_rows(R)
    p = Guarded(n, width, F32)
    p.t.fill_(float("nan"))
    return p, n


def reduce_partials(part, n, dst_a, dst_b, Ca, Cb):
    from glow_tts_amd import _lib
    args = _lib.PartialsArgs()
    j = args.job[0]
    j.partials, j.dst_a, j.dst_b, j.n_rows, j.Ca, j.Cb = part.t.data_ptr(), dst_a.t.data_ptr(), dst_b.t.data_ptr(), n, Ca, Cb
    args.n_jobs = 1
    _lib.call.gt_param_partials_reduce(args, _st())


def pair(buf):
    """hi + lo of a bf16x3 rows buffer [R, >= 3 C] as float64 on the CPU"""
    t = buf.t.detach().cpu()
    return t[:, :C].double() + t[:, 2 * C:3 * C].double()


@functools.lru_cache(maxsize=None)
def run_case(gname, d, p, with_seed_dev):
    from glow_tts_amd._lib import call
    O = D.operands(gname)
    R, st = O.R, _st()
    word = SEED_WORD if with_seed_dev else 0
    sw = torch.from_numpy(np.array([SEED_WORD], dtype=np.uint32).view(np.int32)).to(dev()) if with_seed_dev else None
    k = types.SimpleNamespace(**{n: g(getattr(O, n)) for n in ("utt", "mask", "dy", "da1", "h2", "dh1", "w", "b", "gamma1", "beta1", "gamma2", "beta2")})
    if gname in D.WIDE_X:
        xbuf = torch.full((R, LDX_WIDE), float("nan"), device=dev())
        xbuf[:, X_COL0:X_COL0 + C] = O.x.to(dev())
        x, ldx = xbuf[:, X_COL0:X_COL0 + C], LDX_WIDE
    else:
        xbuf = x = g(O.x)
        ldx = C
    xbuf_before = xbuf.clone()
    lda = 3 * C + 8 if gname == D.PADDED_A1 else 3 * C
    b = {}
    # forward
    b["a1"] = Guarded(R, lda, BF16)
    call.gt_dds_sep_fwd(x, ldx, k.w, k.b, k.gamma1, k.beta1, k.utt, k.mask, b["a1"].t, lda, R, C, d, EPS, st)
    b["out"], b["out_bf16"], b["out_alone"] = Guarded(R, C, F32), Guarded(R, C, BF16), Guarded(R, C, F32)
    call.gt_dds_out_fwd(k.h2, x, ldx, k.gamma2, k.beta2, k.mask, b["out"].t, b["out_bf16"].t, R, C, EPS, p, SEED, sw, st)
    call.gt_dds_out_fwd(k.h2, x, ldx, k.gamma2, k.beta2, k.mask, b["out_alone"].t, None, R, C, EPS, p, SEED, sw, st)
    # backward, one atomic per address and workgroup; every destination starts from its prior
    b["dh2"], b["dg2"], b["db2"] = Guarded(R, 3 * C, BF16), guarded(O.dg2_0), guarded(O.db2_0)
    call.gt_dds_out_bwd(k.h2, k.dy, k.gamma2, k.beta2, k.mask, b["dh2"].t, b["dg2"].t, b["db2"].t, None, R, C, EPS, p, SEED, sw, st)
    b["dh1"], b["dg1"], b["db1"] = Guarded(R, C, F32), guarded(O.dg1_0), guarded(O.db1_0)
    call.gt_dds_sep_bwd(x, ldx, k.w, k.b, k.gamma1, k.beta1, k.utt, k.mask, k.da1, b["dh1"].t, b["dg1"].t, b["db1"].t, None, R, C, d, EPS, st)
    b["dx"], b["dw"], b["db"] = Guarded(R, C, F32), guarded(O.dw_0), guarded(O.db_0)
    call.gt_dds_dw_bwd(x, ldx, k.dh1, k.dy, k.w, k.utt, k.mask, b["dx"].t, b["dw"].t, b["db"].t, None, R, C, d, st)
    # backward, partial rows: NaN buffers, NULL gradient pointers, then the reduce into destinations holding the same priors
    b["p.dh2"], b["p.dg2"], b["p.db2"] = Guarded(R, 3 * C, BF16), guarded(O.dg2_0), guarded(O.db2_0)
    b["p.outb"], n = nan_partials(R, 2 * C)
    call.gt_dds_out_bwd(k.h2, k.dy, k.gamma2, k.beta2, k.mask, b["p.dh2"].t, None, None, b["p.outb"].t, R, C, EPS, p, SEED, sw, st)
    b["p.dh1"], b["p.dg1"], b["p.db1"] = Guarded(R, C, F32), guarded(O.dg1_0), guarded(O.db1_0)
    b["p.sepb"], _ = nan_partials(R, 2 * C)
    call.gt_dds_sep_bwd(x, ldx, k.w, k.b, k.gamma1, k.beta1, k.utt, k.mask, k.da1, b["p.dh1"].t, None, None, b["p.sepb"].t, R, C, d, EPS, st)
    b["p.dx"], b["p.dw"], b["p.db"] = Guarded(R, C, F32), guarded(O.dw_0), guarded(O.db_0)
    b["p.dwb"], _ = nan_partials(R, 4 * C)
    call.gt_dds_dw_bwd(x, ldx, k.dh1, k.dy, k.w, k.utt, k.mask, b["p.dx"].t, None, None, b["p.dwb"].t, R, C, d, st)
    partials = {n_: b[n_].t.clone() for n_ in ("p.outb", "p.sepb", "p.dwb")}
    reduce_partials(b["p.outb"], n, b["p.dg2"], b["p.db2"], C, C)
    reduce_partials(b["p.sepb"], n, b["p.dg1"], b["p.db1"], C, C)
    reduce_partials(b["p.dwb"], n, b["p.dw"], b["p.db"], 3 * C, C)
    torch.cuda.synchronize()
    r = types.SimpleNamespace(O=O, b=b, d=d, p=p, n_partial_rows=n, lda=lda, partials={n_: v.cpu() for n_, v in partials.items()})
    r.x_untouched = torch.equal(xbuf.view(torch.int32), xbuf_before.view(torch.int32))
    r.got = {"sep.a1": pair(b["a1"]), "out.out": out(b["out"]).double(), "outb.dh2": pair(b["dh2"]), "outb.dgamma": out(b["dg2"], (-1,)).double(),
             "outb.dbeta": out(b["db2"], (-1,)).double(), "sepb.dh1": out(b["dh1"]).double(), "sepb.dgamma": out(b["dg1"], (-1,)).double(),
             "sepb.dbeta": out(b["db1"], (-1,)).double(), "dw.dx": out(b["dx"]).double(), "dw.dw": out(b["dw"], (C, 3)).double(),
             "dw.db": out(b["db"], (-1,)).double()}
    r.got_p = {"outb.dh2": pair(b["p.dh2"]), "outb.dgamma": out(b["p.dg2"], (-1,)).double(), "outb.dbeta": out(b["p.db2"], (-1,)).double(),
               "sepb.dh1": out(b["p.dh1"]).double(), "sepb.dgamma": out(b["p.dg1"], (-1,)).double(), "sepb.dbeta": out(b["p.db1"], (-1,)).double(),
               "dw.dx": out(b["p.dx"]).double(), "dw.dw": out(b["p.dw"], (C, 3)).double(), "dw.db": out(b["p.db"], (-1,)).double()}
    r.keep, r.scale = D.keep_mask(SEED, word, R, p)
    r.ref = D.reference(O, d, r.keep, r.scale, EPS)
    r.twin = D.reference(O, d, r.keep, r.scale, EPS, dtype=F32)
    r.dw_ref = D.dw_bwd(O.x, O.dh1, O.dy, O.w, O.utt, O.mask, d, O.dw_0, O.db_0)
    return r


# ------------------------------------------------------------------------------------------------ the rule of the nonlinear kernels
def limits(ref, twin, keys):
    return {k: max(M[k] * rel_l2(twin[k], ref[k]), rows64.AGG_F32) for k in keys}


def hold(case, got, ref, twin, keys):
    """print the figures of every output, then assert the rule"""
    lim, bad = limits(ref, twin, keys), []
    for k in keys:
        ek, et = rel_l2(got[k], ref[k]), rel_l2(twin[k], ref[k])
        print(f"RATIO {k} {case}: err_kernel {ek:.3e} err_twin {et:.3e} ratio {ek / max(et, 1e-300):.3f} limit {lim[k]:.3e}")
        if not ek <= lim[k]:
            bad.append((k, ek, et, lim[k]))
    assert not bad, (case, bad)


def miss(got, bad_ref, ref, twin, keys):
    """by how much each output misses its (true) limit against a reference with a planted defect"""
    lim = limits(ref, twin, keys)
    return {k: rel_l2(got[k], bad_ref[k]) / lim[k] for k in keys}


def dw_reports(case, got, ref):
    """the elementwise rule of rows64.check on dx, dw and db against a dds64.dw_bwd result"""
    return {"dw.dx": rows64.check(f"dx {case}", got["dw.dx"], ref.dx, rows64.gamma(ref.K_dx) * ref.S_dx),
            "dw.dw": rows64.check(f"dw {case}", got["dw.dw"], ref.dw, rows64.gamma(ref.K_dw) * ref.S_dw),
            "dw.db": rows64.check(f"db {case}", got["dw.db"], ref.db, rows64.gamma(ref.K_db) * ref.S_db)}


def _case(gname, d, p, wsd):
    return f"{gname} d={d} p={p} seed_dev={int(wsd)}"


@pytest.mark.parametrize("gname,d,p,with_seed_dev", CASES)
def test_exact_properties(built, gname, d, p, with_seed_dev):
    r = run_case(gname, d, p, with_seed_dev)
    O, b = r.O, r.b
    canaries(b)
    assert r.x_untouched
    off = ~O.on
    a1, dh2 = b["a1"].t.cpu().view(torch.int16), b["dh2"].t.cpu().view(torch.int16)
    assert torch.equal(a1[:, :C], a1[:, C:2 * C]) and torch.equal(dh2[:, :C], dh2[:, C:2 * C])
    if r.lda > 3 * C:                                       # the pad columns of a1 keep the canary pattern
        assert bool((a1[:, 3 * C:] == 0x5A5A).all())
    # out_bf16 is bf16(out), and asking for it changes nothing in out
    o = b["out"].t.cpu()
    assert torch.equal(b["out_bf16"].t.cpu().view(torch.int16), o.to(BF16).view(torch.int16))
    assert torch.equal(o.view(torch.int32), b["out_alone"].t.cpu().view(torch.int32))
    # masked rows of every row output are exactly zero (the operands hold 1e30 there)
    if int(off.sum()):
        for name in ("a1", "out", "out_bf16", "dh2", "dh1", "dx", "p.dh2", "p.dh1", "p.dx"):
            width = 3 * C if name == "a1" else b[name].t.shape[1]             # a1 may have pad columns: checked above
            assert float(b[name].t.cpu()[off][:, :width].float().abs().max()) == 0, name
    # dropout: what out_fwd dropped is what oracle/dropmask.py says, about half of it at p = 0.5
    if p > 0:
        y = D.ln_gelu_fwd(O.h2, O.gamma2, O.beta2, O.mask, EPS)
        dropped = ((o.double() - O.x.double()) == 0) & (y.abs() > 1e-6) & O.on[:, None]
        assert torch.equal(dropped, (r.keep == 0) & (y.abs() > 1e-6) & O.on[:, None])
        assert 0.4 < float(r.keep[O.on].mean()) < 0.6
    # the partial rows: one per workgroup, every one written (they started as NaN), a fully masked workgroup's row is zero
    assert r.n_partial_rows == -(-O.R // D.WG)
    for name, part in r.partials.items():
        assert part.shape[0] == r.n_partial_rows and bool(torch.isfinite(part).all()), name
        for wg in range(r.n_partial_rows):
            if not bool(O.on[wg * D.WG:(wg + 1) * D.WG].any()):
                assert float(part[wg].abs().max()) == 0, (name, wg)
    # row outputs are bit-equal between the two forms
    for name, kind in (("dh2", torch.int16), ("dh1", torch.int32), ("dx", torch.int32)):
        assert torch.equal(b[name].t.cpu().view(kind), b["p." + name].t.cpu().view(kind)), name


@pytest.mark.parametrize("gname,d,p,with_seed_dev", CASES)
def test_nonlinear_kernels_against_float64(built, gname, d, p, with_seed_dev):
    r = run_case(gname, d, p, with_seed_dev)
    case = _case(gname, d, p, with_seed_dev)
    hold(case, r.got, r.ref, r.twin, NONLINEAR)
    hold(case + " partial rows", r.got_p, r.ref, r.twin, FAMILY["outb"] + FAMILY["sepb"])


@pytest.mark.parametrize("gname,d,p,with_seed_dev", CASES)
def test_dw_bwd_against_float64(built, gname, d, p, with_seed_dev):
    r = run_case(gname, d, p, with_seed_dev)
    case = _case(gname, d, p, with_seed_dev)
    bad = []
    for form, got in (("atomics", r.got), ("partial rows", r.got_p)):
        for k, rep in dw_reports(f"{case} {form}", got, r.dw_ref).items():
            print("CHECK", rep)
            if not rep.ok:
                bad.append(str(rep))
    assert not bad, bad


@pytest.mark.parametrize("gname,d,p,with_seed_dev", CASES)
def test_atomics_and_partials_forms_agree(built, gname, d, p, with_seed_dev):
    """the figure of test_dds_dropout_replays_in_backward and tests/test_dds_layer_gpu.py: 1e-5 relative"""
    r = run_case(gname, d, p, with_seed_dev)
    for k in ("outb.dgamma", "outb.dbeta", "sepb.dgamma", "sepb.dbeta", "dw.dw", "dw.db"):
        a, b = r.got_p[k], r.got[k]
        assert float((a - b).abs().max() / b.abs().max()) < 1e-5, k


# ------------------------------------------------------------------------------------------------ controls
CONTROLS = {"ignore_utt": ("sep", "sepb", "dw"), "taps_swapped": ("sep", "sepb", "dw"), "gelu_tanh": ("sep", "out", "outb", "sepb"),
            "var_cm1": ("sep", "out", "outb", "sepb"), "no_drop_scale": ("outb",), "keep_of_seed_plus_1": ("out", "outb"), "dw_3C": ("dw",),
            "overwrite": ("outb", "sepb", "dw")}


@pytest.mark.parametrize("defect", list(CONTROLS))
def test_planted_defects_are_seen(built, defect):
    """the comparisons above against a reference with one planted defect: every kernel the defect concerns must miss its TRUE limit
    by >= CONTROL_MISS, in the atomics form and in the partial-row form"""
    r = run_case(*CONTROL_CASE)
    O, d = r.O, r.d
    keep, kw = r.keep, {}
    if defect == "keep_of_seed_plus_1":
        keep, _ = D.keep_mask(SEED + 1, SEED_WORD, O.R, r.p)
        assert not torch.equal(keep, r.keep)
    else:
        kw["defect"] = defect
    bad = D.reference(O, d, keep, r.scale, EPS, **kw)
    bad_dw = D.dw_bwd(O.x, O.dh1, O.dy, O.w, O.utt, O.mask, d, O.dw_0, O.db_0, **kw)
    for form, got in (("atomics", r.got), ("partial rows", r.got_p)):
        misses = miss(got, bad, r.ref, r.twin, [k for k in NONLINEAR if k in got])
        misses.update({k: rep.miss for k, rep in dw_reports(defect, got, bad_dw).items()})
        for fam in CONTROLS[defect]:
            keys = [k for k in FAMILY[fam] if k in misses]
            if keys:
                seen(f"{defect} ({fam}, {form})", misses, among=keys)


# ------------------------------------------------------------------------------------------------ gt_rows_split3
SPLIT_SHAPES = [(7, 37, 40, 3 * 37 + 5), (9, 192, 256, 3 * 192 + 8)]        # R, C, ldi > C, ldo > 3 C; R * C is no multiple of 256


@pytest.mark.parametrize("is_f32", [1, 0])
@pytest.mark.parametrize("with_mask", [True, False])
@pytest.mark.parametrize("R,n,ldi,ldo", SPLIT_SHAPES)
def test_rows_split3_bit_for_bit(built, R, n, ldi, ldo, with_mask, is_f32):
    """fp32 or bf16 input, rowmask given or NULL: [hi | hi | lo] equals dds64.split3 bit for bit; the inputs hold +-0, fp32 subnormals,
    exact ties between bf16 neighbours and roundings that carry into the next exponent; the columns past C of the input are NaN, the
    columns past 3 C of the output and the canary rows stay as they were"""
    from glow_tts_amd._lib import call
    assert (R * n) % 256 != 0 and ldi > n and ldo > 3 * n
    v = split3_inputs(R, n, seed=R)
    mask = np.ones(R, dtype=np.float32)
    mask[[1, R - 1]] = 0
    if is_f32:
        src = torch.full((R, ldi), float("nan"))
        src[:, :n] = torch.from_numpy(v)
        ref_in = v
    else:
        hi = rows64.f2bf(v)
        src = torch.full((R, ldi), float("nan")).to(BF16)
        src[:, :n] = torch.from_numpy(hi.view(np.int16)).view(BF16)
        ref_in = hi
    o = Guarded(R, ldo, BF16)
    call.gt_rows_split3(g(src), ldi, is_f32, o.t, ldo, g(torch.from_numpy(mask)) if with_mask else None, R, n, _st())
    torch.cuda.synchronize()
    assert o.canaries_intact()
    got = o.t.cpu().view(torch.int16).numpy().view(np.uint16)
    assert (got[:, 3 * n:] == 0x5A5A).all()
    want = D.split3(ref_in, mask if with_mask else None)
    diff = np.argwhere(got[:, :3 * n] != want)
    assert diff.size == 0, [(int(i), int(j), hex(int(got[i, j])), hex(int(want[i, j]))) for i, j in diff[:8]]
    if not is_f32:
        assert not got[:, 2 * n:3 * n].any()
