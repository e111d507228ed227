"""CPU tests of oracle/dds64.py, the float64 restatement tests/test_dds_ops_fp64_gpu.py holds the per-op DDSConv kernels and
gt_rows_split3 to: its hand-written backwards equal float64 autograd of its forwards to 1e-12, every planted defect moves some output
by at least CONTROL_MISS * AGG_F32 (so the GPU test's controls CAN be seen), split3 survives a round trip and keeps the special values,
the float32 twin is a sane yardstick, and the geometries hold what their comments claim."""
import numpy as np
import pytest
import torch

from oracle import dds64 as D
from oracle import rows64

C = D.C
EPS = 1e-5
F64 = torch.float64
SEED, WORD = 4242, 0x9E3779B9
CONTROL_CASE = ("r70", 9, 0.5)


def rel_l2(got, ref):
    return float((got - ref).norm() / ref.norm().clamp_min(1e-300))


def rel_max(got, ref):
    return float((got - ref).abs().max() / ref.abs().max().clamp_min(1e-300))


def test_geometries_hold_what_they_claim():
    D.geometry_claims()


@pytest.mark.parametrize("d", [1, 3, 9])
def test_hand_written_backwards_equal_autograd(d):
    O = D.operands("r33", seed=d)
    keep, scale = D.keep_mask(SEED, WORD, O.R, 0.5)
    zero, zero3 = torch.zeros(C), torch.zeros(C, 3)
    leaf = lambda t: t.double().clone().requires_grad_(True)                        # noqa: E731
    on = O.on[:, None]
    dy, da1, dh1 = (torch.where(on, t.double(), torch.zeros(1, dtype=F64)) for t in (O.dy, O.da1, O.dh1))
    # gt_dds_out_bwd against autograd of out_fwd
    h2, g2, b2 = leaf(torch.where(on, O.h2, torch.zeros(1))), leaf(O.gamma2), leaf(O.beta2)
    (D.out_fwd(h2, O.x, g2, b2, O.mask, keep, scale, EPS) * dy).sum().backward()
    got = D.out_bwd(O.h2, O.dy, O.gamma2, O.beta2, O.mask, keep, scale, EPS, zero, zero)
    for name, a, b in zip(("dh2", "dgamma2", "dbeta2"), got, (h2.grad, g2.grad, b2.grad)):
        assert rel_max(a, b) <= 1e-12, (name, rel_max(a, b))
    # gt_dds_sep_bwd against autograd of the LayerNorm + GELU of sep_fwd, at h1
    h1, g1, b1 = leaf(D.sep_h1(O.x, O.w, O.b, O.utt, O.mask, d)), leaf(O.gamma1), leaf(O.beta1)
    (D.ln_gelu_fwd(h1, g1, b1, O.mask, EPS) * da1).sum().backward()
    got = D.sep_bwd(O.x, O.w, O.b, O.gamma1, O.beta1, O.utt, O.mask, d, O.da1, EPS, zero, zero)
    for name, a, b in zip(("dh1", "dgamma1", "dbeta1"), got, (h1.grad, g1.grad, b1.grad)):
        assert rel_max(a, b) <= 1e-12, (name, rel_max(a, b))
    assert torch.equal(D.sep_fwd(O.x, O.w, O.b, O.gamma1, O.beta1, O.utt, O.mask, d, EPS), D.ln_gelu_fwd(h1.detach(), O.gamma1, O.beta1, O.mask, EPS))
    # gt_dds_dw_bwd against autograd of the depthwise conv plus the residual
    x, w, b = leaf(O.x), leaf(O.w), leaf(O.b)
    ((D.sep_h1(x, w, b, O.utt, O.mask, d) * dh1).sum() + (x * dy).sum()).backward()
    r = D.dw_bwd(O.x, O.dh1, O.dy, O.w, O.utt, O.mask, d, zero3, zero)
    for name, a, b_ in (("dx", r.dx, x.grad), ("dw", r.dw, w.grad), ("db", r.db, b.grad)):
        assert rel_max(a, b_) <= 1e-12, (name, rel_max(a, b_))
    assert float(x.grad[~O.on].abs().max()) == 0
    # the absolute-value twins bound their sums, and the priors are added
    assert bool((r.dx.abs() <= r.S_dx * (1 + 1e-12)).all() and (r.dw.abs() <= r.S_dw * (1 + 1e-12)).all() and (r.db.abs() <= r.S_db * (1 + 1e-12)).all())
    assert r.K_dx == 4 and r.K_dw == r.K_db == O.n_valid + 1
    rp = D.dw_bwd(O.x, O.dh1, O.dy, O.w, O.utt, O.mask, d, O.dw_0, O.db_0)
    assert rel_max(rp.dw - O.dw_0.double(), r.dw) <= 1e-12 and rel_max(rp.db - O.db_0.double(), r.db) <= 1e-12
    assert torch.equal(rp.S_dw, r.S_dw + O.dw_0.double().abs())


def _all_outputs(O, d, keep, scale, defect=None):
    v = D.reference(O, d, keep, scale, EPS, defect=defect)
    r = D.dw_bwd(O.x, O.dh1, O.dy, O.w, O.utt, O.mask, d, O.dw_0, O.db_0, defect=defect)
    v.update({"dw.dx": r.dx, "dw.dw": r.dw, "dw.db": r.db})
    return v


# which kernels' outputs a defect must move (the families of tests/test_dds_ops_fp64_gpu.py)
AFFECTS = {"ignore_utt": ("sep", "sepb", "dw"), "taps_swapped": ("sep", "sepb", "dw"), "gelu_tanh": ("sep", "out", "outb", "sepb"),
           "var_cm1": ("sep", "out", "outb", "sepb"), "no_drop_scale": ("outb",), "dw_3C": ("dw",), "overwrite": ("outb", "sepb", "dw"),
           "keep_of_seed_plus_1": ("out", "outb")}


@pytest.mark.parametrize("defect", list(AFFECTS))
def test_every_planted_defect_can_be_seen(defect):
    """on the geometry the GPU test runs its controls on: every kernel a defect concerns has an output that moves by a relative L2 of
    at least CONTROL_MISS * AGG_F32, the least a control has to miss the floor of the rule by"""
    gname, d, p = CONTROL_CASE
    O = D.operands(gname)
    keep, scale = D.keep_mask(SEED, WORD, O.R, p)
    ref = _all_outputs(O, d, keep, scale)
    if defect == "keep_of_seed_plus_1":
        keep1, _ = D.keep_mask(SEED + 1, WORD, O.R, p)
        assert not torch.equal(keep1, keep)
        bad = _all_outputs(O, d, keep1, scale)
    else:
        assert defect in D.DEFECTS
        bad = _all_outputs(O, d, keep, scale, defect)
    moved = {k: rel_l2(bad[k], ref[k]) for k in ref}
    print(defect, {k: float(f"{v:.3g}") for k, v in moved.items()})
    for fam in AFFECTS[defect]:
        assert max(v for k, v in moved.items() if k.split(".")[0] == fam) >= rows64.CONTROL_MISS * rows64.AGG_F32, (defect, fam, moved)
    for k, v in moved.items():                                  # ... and no other kernel's reference moves at all
        if k.split(".")[0] not in AFFECTS[defect]:
            assert v == 0, (defect, k, v)


@pytest.mark.parametrize("gname,d", [("r8", 1), ("r8", 3), ("r9", 1), ("r33", 9), ("r70", 1), ("r70", 3), ("r70", 9)])
def test_the_utterance_clause_decides_somewhere(gname, d):
    O = D.operands(gname)
    ref, bad = _all_outputs(O, d, None, 1.0), _all_outputs(O, d, None, 1.0, "ignore_utt")
    for k in ("sep.a1", "sepb.dh1", "dw.dx", "dw.dw"):
        assert rel_l2(bad[k], ref[k]) >= rows64.CONTROL_MISS * rows64.AGG_F32, k
    # r7 is one utterance: there only the range guard stops a tap
    O7 = D.operands("r7")
    assert all(torch.equal(a, b) for a, b in zip(_all_outputs(O7, d, None, 1.0).values(), _all_outputs(O7, d, None, 1.0, "ignore_utt").values()))


def test_the_float32_twin_is_a_sane_yardstick():
    """err_twin of every output is fp32-sized: 16 times it stays under the floor of the rule, so M never lifts a limit above AGG_F32
    because the twin itself is loose (a1 and d h2 as bf16 pairs carry 2^-17)"""
    for gname, d, p in (("r7", 1, 0.0), ("r33", 3, 0.5), ("r70", 9, 0.5)):
        O = D.operands(gname)
        keep, scale = D.keep_mask(SEED, WORD, O.R, p)
        ref, twin = D.reference(O, d, keep, scale, EPS), D.reference(O, d, keep, scale, EPS, dtype=torch.float32)
        for k in ref:
            e = rel_l2(twin[k], ref[k])
            assert 0 < e <= (2.0 ** -17 if k in ("sep.a1", "outb.dh2") else 1e-6), (gname, k, e)


def test_keep_mask_follows_the_hash():
    keep, scale = D.keep_mask(SEED, WORD, 70, 0.5)
    assert scale == 2.0 and keep.shape == (70, C) and 0.45 < float(keep.mean()) < 0.55
    from oracle import dropmask
    h = dropmask.hash_u32(dropmask._mix(SEED ^ WORD, 5, 7))
    assert bool(keep[5, 7]) == bool(h >= 2 ** 31)
    assert D.keep_mask(SEED, WORD, 70, 0.0) == (None, 1.0)


def _special_values():
    """fp32 values a bf16 split can get wrong: +-0, subnormals, exact ties between bf16 neighbours (to even, both ways), roundings that
    carry into the next exponent; nothing near the bf16 overflow"""
    bits = [0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x00008000, 0x00018000, 0x007FFFFF, 0x807FFFFF, 0x00800000,
            0x3F808000, 0x3F818000, 0xBF808000, 0xBF818000,          # ties: down to even (0x3F80), up to even (0x3F82)
            0x3F808001, 0x3F807FFF, 0x3F7F8000, 0x3F7FFFFF, 0xBF7FFFFF, 0x3FFFFFFF, 0x407FC000, 0x7E7F8000, 0x00FF8000]   # carries
    return np.array(bits, dtype=np.uint32).view(np.float32)


def split3_inputs(R, n, seed=0):
    """[R, n] fp32: random values over many exponents with the special values scattered in"""
    rng = np.random.default_rng(100 + seed)
    v = (rng.standard_normal((R, n)) * 10.0 ** rng.integers(-6, 7, (R, n))).astype(np.float32)
    sp = _special_values()
    pos = rng.permutation(R * n)[:sp.size]
    v.reshape(-1)[pos] = sp
    return v


def test_split3_survives_a_round_trip():
    v = split3_inputs(7, 37)
    assert np.isfinite(v).all() and np.abs(v).max() < 1e38
    b = D.split3(v)
    assert b.shape == (7, 111) and b.dtype == np.uint16
    hi, hi2, lo = b[:, :37], b[:, 37:74], b[:, 74:]
    assert np.array_equal(hi, hi2) and np.array_equal(hi, rows64.f2bf(v))
    back = D.pair_value(b).numpy()
    normal = np.abs(v) >= 2.0 ** -110                            # lo of a smaller value falls among the bf16 subnormals
    assert (np.abs(back - v.astype(np.float64))[normal] <= 2.0 ** -16 * np.abs(v)[normal]).all()
    assert (np.abs(back - v.astype(np.float64)) <= 2.0 ** -16 * np.abs(v) + 2.0 ** -134).all()
    # the special values: ties go to even, a carry lands on the next power of two, zeros keep their sign, lo of a bf16 value is +0
    sp = _special_values()
    s = D.split3(sp[None, :])[0]
    n = sp.size
    as_bits = dict(zip(sp.view(np.uint32).tolist(), zip(s[:n].tolist(), s[2 * n:].tolist())))
    assert as_bits[0x3F808000][0] == 0x3F80 and as_bits[0x3F818000][0] == 0x3F82 and as_bits[0xBF808000][0] == 0xBF80 and as_bits[0xBF818000][0] == 0xBF82
    assert as_bits[0x3F7F8000][0] == 0x3F80 and as_bits[0x3FFFFFFF][0] == 0x4000 and as_bits[0x00FF8000][0] == 0x0100
    assert as_bits[0x00000000] == (0x0000, 0x0000) and as_bits[0x80000000] == (0x8000, 0x0000)
    assert as_bits[0x00000001] == (0x0000, 0x0000) and as_bits[0x00008000] == (0x0000, 0x0000) and as_bits[0x00018000] == (0x0002, 0x8000)
    assert as_bits[0x3F808000][1] == 0x3B80                      # 1 + 2^-8 = hi 1 + lo 2^-8, exactly
    # a row mask zeroes rows (keeping the sign of zero), a bf16 input has lo = 0
    mask = np.array([1, 0, 1, 1, 0, 1, 1], dtype=np.float32)
    bm = D.split3(v, mask)
    assert np.array_equal(bm[mask != 0], b[mask != 0]) and not (bm[mask == 0] & 0x7FFF).any()
    hb = torch.from_numpy(hi.view(np.int16)).view(torch.bfloat16)
    bb = D.split3(hb)
    assert np.array_equal(bb[:, :37], hi) and np.array_equal(bb[:, 37:74], hi) and not bb[:, 74:].any()
    assert np.array_equal(D.split3(hi), bb)
    assert torch.equal(D.as_pair(torch.from_numpy(v)), D.pair_value(b))
