"""GPU tests of the three kernels behind full-model synthesis, called directly through the C-ABI (csrc/synth_prosody.hip,
csrc/synth_front.hip): gt_randn_keyed[_call], gt_synth_frame_geometry and gt_synth_contours[_call].

Tolerances: 1e-5 absolute for a generator draw against its float64 restatement — the bound tests/test_synthesis_front_gpu.py has for
gt_randn_rows, the same generator code.  Everything else is exact: the same draw on two rows layouts, the _call form against the
by-value form, the geometry against its host restatement, the contours against the launch sequence they replace."""
import ctypes
import os
import random
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import synth_frame_geometry_host as FG  # noqa: E402
import synth_geometry_host as G  # noqa: E402
import synth_noise_host as H  # noqa: E402
import synth_prosody_host as PH  # noqa: E402

pytestmark = pytest.mark.gpu
HALO = 2
CAN, MARGIN = 768.0, 1024
INVAL = -1


def dev():
    return torch.device("cuda:0")


def guarded(n, dtype, inside):
    """flat buffer with canary margins -> (flat, the n elements in the middle, pre-filled with `inside`)"""
    flat = torch.full((n + 2 * MARGIN,), CAN, dtype=dtype, device=dev())
    flat[MARGIN:MARGIN + n] = inside
    return flat, flat[MARGIN:MARGIN + n]


def margins_untouched(flat, n):
    return bool((flat[:MARGIN] == CAN).all() and (flat[MARGIN + n:] == CAN).all())


def i32(v):
    return torch.tensor(v, dtype=torch.int32, device=dev())


def call_block(seed, ns, nsw, ls, f0, en, ps, es):
    """a gt_synth_call_ext in device memory"""
    from glow_tts_amd import _lib
    c = _lib.SynthCallExt(_lib.SynthCall(seed=seed, noise_scale=ns, noise_scale_w=nsw, length_scale=ls), f0, en, ps, es)
    return torch.frombuffer(bytearray(bytes(c)), dtype=torch.int32).clone().to(dev())


# ---- gt_randn_keyed ------------------------------------------------------------------------------------------------------------
LENS = [1, 7, 12, 30, 9]              # a 1-frame utterance, odd lengths
T_MAX = 30


def layouts():
    """(name, row0 or None, Tp, R): the same lengths uniform, ragged with row_round 8, and ragged at a larger capacity; no R is a
    multiple of 256, the last two need more than one workgroup"""
    from glow_tts_amd.ops import RowsCtx
    B = len(LENS)
    starts, R8 = RowsCtx.row_starts(LENS, T_MAX, 8)
    big = list(starts)
    big[-1] = 600
    assert R8 % 256 and 600 % 256 and (B * (T_MAX + 2 * HALO)) % 256
    return [("uniform", None, T_MAX + 2 * HALO, B * (T_MAX + 2 * HALO)), ("ragged", starts, T_MAX + 2 * HALO + 7, R8),
            ("capacity", big, T_MAX + 2 * HALO + 599, 600)]


@pytest.mark.parametrize("ncol", [1, 2])
def test_randn_keyed_against_the_host_on_three_layouts(built, ncol):
    from glow_tts_amd import _lib
    L = _lib.lib()
    st = _lib.current_stream(dev())
    seed, stream, scale = 0x7fffffff, H.PITCH, 0.25
    lens_d = i32(LENS)
    per_utt = {}
    for name, row0, Tp, R_ in layouts():
        r0 = row0 if row0 is not None else [b * Tp for b in range(len(LENS) + 1)]
        row0_d = None if row0 is None else i32(row0)
        flat, out = guarded(R_ * ncol, torch.float32, float("nan"))
        _lib.check(L.gt_randn_keyed(_lib.ptr(out), _lib.ptr(row0_d), Tp, _lib.ptr(lens_d), len(LENS), R_, ncol, seed, stream, scale, st),
                   "gt_randn_keyed")
        torch.cuda.synchronize()
        assert margins_untouched(flat, R_ * ncol)
        got = out.cpu().view(R_, ncol)
        assert torch.isfinite(got).all()                                           # every row is written
        want = PH.keyed_rows(r0, LENS, R_, ncol, seed, stream, scale)
        err = np.abs(got.numpy().astype(np.float64) - want).max()
        print(f"gt_randn_keyed [{name}, R = {R_}, ncol = {ncol}] vs host float64: {err:.3e}")
        assert err <= 1e-5, err
        inside = np.zeros(R_, dtype=bool)
        for b, n in enumerate(LENS):
            inside[r0[b] + HALO:r0[b] + HALO + n] = True
            per_utt.setdefault(b, []).append(got[r0[b] + HALO:r0[b] + HALO + n].clone())
        assert (got.numpy()[~inside] == 0).all()                                   # halo / padding / rounding rows
        assert (got.numpy()[inside] != 0).all()
    for b, vals in per_utt.items():                                                # the same (b, t) on the three layouts: bit-equal
        assert torch.equal(vals[0], vals[1]) and torch.equal(vals[0], vals[2]), b


def test_randn_keyed_call_equals_by_value(built):
    from glow_tts_amd import _lib
    L = _lib.lib()
    st = _lib.current_stream(dev())
    seed = 4242
    scales = (0.667, 0.8, 0.3, 1.7)                                                # noise_scale, noise_scale_w, f0_noise_scale, energy_noise_scale
    blk = call_block(seed, scales[0], scales[1], 1.0, scales[2], scales[3], 1.0, 1.0)
    name, row0, Tp, R_ = layouts()[1]
    row0_d, lens_d = i32(row0), i32(LENS)
    outs = []
    for which in range(4):
        a = torch.full((R_, 2), float("nan"), device=dev())
        b = torch.full((R_, 2), float("nan"), device=dev())
        _lib.check(L.gt_randn_keyed(_lib.ptr(a), _lib.ptr(row0_d), Tp, _lib.ptr(lens_d), len(LENS), R_, 2, seed, which, scales[which], st),
                   "gt_randn_keyed")
        _lib.check(L.gt_randn_keyed_call(_lib.ptr(b), _lib.ptr(row0_d), Tp, _lib.ptr(lens_d), len(LENS), R_, 2, _lib.ptr(blk), which, which, st),
                   "gt_randn_keyed_call")
        torch.cuda.synchronize()
        assert torch.isfinite(b).all() and torch.equal(a, b), which
        outs.append(b)
    assert not torch.equal(outs[2], outs[3])
    b = torch.zeros(R_, 2, device=dev())
    assert L.gt_randn_keyed_call(_lib.ptr(b), _lib.ptr(row0_d), Tp, _lib.ptr(lens_d), len(LENS), R_, 2, _lib.ptr(blk), 1, 4, st) == INVAL


# ---- gt_synth_frame_geometry ---------------------------------------------------------------------------------------------------
def frame_cases():
    rng = random.Random(7)
    out = []
    for B, Ty_cap in ((1, 41), (3, 64), (1024, 30)):
        lens = [rng.randint(1, Ty_cap) for _ in range(B)]
        lens[0] = Ty_cap                                                           # == Ty_cap
        lens[-1] = 1 if B > 1 else lens[-1]
        if B > 2:
            lens[1] = 7                                                            # odd
        need = sum(v + 2 * HALO for v in lens)
        fits = -(-need // 8) * 8
        fits += 8 if fits % 256 == 0 else 0                                        # a partial last workgroup
        out.append((B, Ty_cap, lens, fits, 0))
        out.append((B, Ty_cap, lens, need - 1, FG.BIT_FRAME_ROWS))                 # one row short
    return out


@pytest.mark.parametrize("case", range(6))
def test_frame_geometry_against_the_host(built, case):
    from glow_tts_amd import _lib
    L = _lib.lib()
    B, Ty_cap, lens, cap, bit = frame_cases()[case]
    assert cap % 256 and cap >= 2 * HALO * B
    want = FG.frame_geometry(lens, Ty_cap, cap)
    assert want["status"] == bit
    f_r0, row0 = guarded(B + 1, torch.int32, -7)
    f_lf, len_f = guarded(B, torch.int32, -7)
    f_rb, rowbatch = guarded(cap, torch.int64, -7)
    f_rf, rowframe = guarded(cap, torch.int32, -7)
    f_rm, rowmask = guarded(cap, torch.float32, float("nan"))
    f_ru, rowutt = guarded(cap, torch.int32, -7)
    f_st, status = guarded(1, torch.int32, 1)                                      # bit 0 set by "gt_synth_geometry": it must survive
    _lib.check(L.gt_synth_frame_geometry(_lib.ptr(i32(lens)), B, Ty_cap, cap, _lib.ptr(row0), _lib.ptr(len_f), _lib.ptr(rowbatch),
                                         _lib.ptr(rowframe), _lib.ptr(rowmask), _lib.ptr(rowutt), _lib.ptr(status),
                                         _lib.current_stream(dev())), "gt_synth_frame_geometry")
    torch.cuda.synchronize()
    for flat, n in ((f_r0, B + 1), (f_lf, B), (f_rb, cap), (f_rf, cap), (f_rm, cap), (f_ru, cap), (f_st, 1)):
        assert margins_untouched(flat, n)
    assert status.item() == (1 | bit)
    assert row0.tolist() == want["row0"] and len_f.tolist() == want["len_f"]
    assert rowbatch.tolist() == want["rowbatch"] and rowutt.tolist() == want["rowbatch"]
    assert rowframe.tolist() == want["rowframe"] and rowmask.tolist() == want["rowmask"]
    r0 = row0.tolist()
    assert all(r0[b] <= r0[b + 1] for b in range(B)) and r0[B] == cap              # monotone, inside the capacity
    assert all(len_f[b].item() + 2 * HALO <= r0[b + 1] - r0[b] for b in range(min(B, 8)))


def test_frame_geometry_refuses_a_capacity_without_the_halos(built):
    from glow_tts_amd import _lib
    L = _lib.lib()
    B = 3
    bufs = [torch.zeros(64, dtype=torch.int64, device=dev()) for _ in range(7)]
    assert L.gt_synth_frame_geometry(_lib.ptr(i32([5, 5, 5])), B, 16, 2 * HALO * B - 1, *[_lib.ptr(b) for b in bufs],
                                     _lib.current_stream(dev())) == INVAL
    torch.cuda.synchronize()
    assert all(int(b.abs().sum()) == 0 for b in bufs)


def test_the_squeezed_geometry_did_not_move(built):
    """gt_synth_geometry shares its kernel with the frame geometry now: one fitting and one overflowing case of
    tests/test_synthesis_graph_cabi's kind against tests/synth_geometry_host.geometry, bit for bit"""
    from glow_tts_amd import _lib
    L = _lib.lib()
    y_len = [64, 1, 33, 70, 18]
    for Ty_cap, R_cap in ((64, 136), (64, 99)):
        B = len(y_len)
        want = G.geometry(y_len, Ty_cap, R_cap)
        row0, len_sq, y_eff = (torch.full((n,), -7, dtype=torch.int32, device=dev()) for n in (B + 1, B, B))
        rowbatch = torch.full((R_cap,), -7, dtype=torch.int64, device=dev())
        rowframe, rowutt = (torch.full((R_cap,), -7, dtype=torch.int32, device=dev()) for _ in range(2))
        rowmask = torch.full((R_cap,), float("nan"), device=dev())
        status = torch.full((1,), -7, dtype=torch.int32, device=dev())
        _lib.check(L.gt_synth_geometry(_lib.ptr(i32(y_len)), B, Ty_cap, R_cap, _lib.ptr(row0), _lib.ptr(len_sq), _lib.ptr(y_eff),
                                       _lib.ptr(rowbatch), _lib.ptr(rowframe), _lib.ptr(rowmask), _lib.ptr(rowutt), _lib.ptr(status),
                                       _lib.current_stream(dev())), "gt_synth_geometry")
        torch.cuda.synchronize()
        assert status.item() == want["status"] and row0.tolist() == want["row0"] and len_sq.tolist() == want["len_sq"]
        assert y_eff.tolist() == want["y_len_eff"] and rowbatch.tolist() == want["rowbatch"] == rowutt.tolist()
        assert rowframe.tolist() == want["rowframe"] and rowmask.tolist() == want["rowmask"]
    assert want["status"] == (G.BIT_FRAMES | G.BIT_ROWS)


# ---- gt_synth_contours ---------------------------------------------------------------------------------------------------------
def contour_setup(lens, ragged):
    """frame-rate and squeezed rows contexts of `lens`, the predictors' outputs as masked frame rows, and the four-launch sequence
    the kernel replaces: from_rows -> * scale -> flow_impl.contour_rows"""
    from glow_tts_amd import ops
    Ty = max(lens)
    lsq = [v // 2 for v in lens]
    rcf = ops.RowsCtx(i32(lens), Ty, lengths_host=lens if ragged else None, round_to=8)
    rcy = ops.RowsCtx(i32(lsq), Ty // 2, lengths_host=lsq if ragged else None, round_to=8)
    g = torch.Generator().manual_seed(len(lens) + Ty)
    prow = (torch.randn(rcf.R, generator=g).to(dev()) * 3 + 5) * rcf.rowmask
    erow = (torch.randn(rcf.R, generator=g).to(dev()).abs() + 0.5) * rcf.rowmask
    return rcf, rcy, prow.contiguous(), erow.contiguous(), Ty


def contour_reference(rcf, rcy, rows, scale, B, Ty):
    from glow_tts_amd import flow_impl
    c = rcf.from_rows(rows[:, None].contiguous()).squeeze(1) * scale
    return c, flow_impl.contour_rows(rcy, c, B, 2 * rcy.T)


@pytest.mark.parametrize("ragged", [True, False])
@pytest.mark.parametrize("lens", [[1, 7, 12, 30, 9], [29, 1, 300, 2]])           # an odd longest utterance; more than one workgroup
def test_contours_equal_the_launch_sequence(built, lens, ragged):
    from glow_tts_amd import _lib
    L = _lib.lib()
    st = _lib.current_stream(dev())
    B = len(lens)
    rcf, rcy, prow, erow, Ty = contour_setup(lens, ragged)
    assert 0 in [v // 2 for v in lens]                                             # a 1-frame utterance: len_sq = 0
    ps, es = 1.37, 0.81
    blk = call_block(1, 1.0, 1.0, 1.0, 1.0, 1.0, ps, es)
    want_p, want_psig = contour_reference(rcf, rcy, prow, ps, B, Ty)
    want_e, want_esig = contour_reference(rcf, rcy, erow, es, B, Ty)
    for b, n in enumerate(lens):                                                   # the reference itself is zero past every length
        assert n >= Ty or want_p[b, n:].abs().max().item() == 0
    for use_p, use_e in ((True, False), (False, True), (True, True)):
        for from_call in (False, True):
            f_ps, psig = guarded(rcy.R * 2, torch.float32, float("nan"))
            f_es, esig = guarded(rcy.R * 2, torch.float32, float("nan"))
            f_p, pitch = guarded(B * Ty, torch.float32, float("nan"))
            f_e, energy = guarded(B * Ty, torch.float32, float("nan"))
            head = (_lib.ptr(prow) if use_p else None, _lib.ptr(erow) if use_e else None, _lib.ptr(rcf.row0), rcf.Tp, _lib.ptr(rcf.lengths),
                    rcf.R, _lib.ptr(rcy.row0), rcy.Tp, _lib.ptr(rcy.lengths), rcy.R, _lib.ptr(psig) if use_p else None,
                    _lib.ptr(esig) if use_e else None, _lib.ptr(pitch) if use_p else None, _lib.ptr(energy) if use_e else None, B, Ty)
            if from_call:
                _lib.check(L.gt_synth_contours_call(*head, _lib.ptr(blk), st), "gt_synth_contours_call")
            else:
                _lib.check(L.gt_synth_contours(*head, ps, es, st), "gt_synth_contours")
            torch.cuda.synchronize()
            for flat, n in ((f_ps, rcy.R * 2), (f_es, rcy.R * 2), (f_p, B * Ty), (f_e, B * Ty)):
                assert margins_untouched(flat, n)
            key = (use_p, use_e, from_call)
            if use_p:                                                              # fully written (no NaN left), bit-equal
                assert torch.equal(psig.view(rcy.R, 2), want_psig), key
                assert torch.equal(pitch.view(B, Ty), want_p), key
            else:                                                                  # an output that was not asked for is not touched
                assert torch.isnan(psig).all() and torch.isnan(pitch).all(), key
            if use_e:
                assert torch.equal(esig.view(rcy.R, 2), want_esig), key
                assert torch.equal(energy.view(B, Ty), want_e), key
            else:
                assert torch.isnan(esig).all() and torch.isnan(energy).all(), key
    assert want_psig.abs().max().item() > 0 and not torch.equal(want_psig, want_esig)


def test_contour_rows_reach_the_decoder(built):
    """FlowSpecDecoder.reverse_rows(pitch_rows=, energy_rows=): the contour rows gt_synth_contours wrote, used in place of the
    contours, give the mel of reverse_rows(pitch=, energy=) bit for bit"""
    sys.path.insert(0, os.path.join(os.path.dirname(__file__), "golden"))
    from fill import fill_module
    from glow_tts_amd import _lib, models
    L = _lib.lib()
    lens = [30, 7, 1, 12]
    B = len(lens)
    rcf, rcy, prow, erow, Ty = contour_setup(lens, True)
    dec = fill_module(models.FlowSpecDecoder(80, 192, 5, 1, 2, 4, p_dropout=0.05, gin_channels=256, with_prosody_wn=True), "decoder.").eval().to(dev())
    dec.store_inverse(True)
    g = torch.Generator().manual_seed(3)
    rows = (torch.randn(rcy.R, 160, generator=g).to(dev()) * rcy.rowmask[:, None]).contiguous()
    spk = torch.randn(B, 256, 1, generator=g).to(dev())
    pitch, psig = contour_reference(rcf, rcy, prow, 1.0, B, Ty)
    energy, esig = contour_reference(rcf, rcy, erow, 1.0, B, Ty)
    want = dec.reverse_rows(rcy, rows, g=spk, pitch=pitch, energy=energy).clone()
    p2, e2 = torch.empty_like(psig), torch.empty_like(esig)
    _lib.check(L.gt_synth_contours(_lib.ptr(prow), _lib.ptr(erow), _lib.ptr(rcf.row0), rcf.Tp, _lib.ptr(rcf.lengths), rcf.R, _lib.ptr(rcy.row0),
                                   rcy.Tp, _lib.ptr(rcy.lengths), rcy.R, _lib.ptr(p2), _lib.ptr(e2), None, None, B, Ty, 1.0, 1.0,
                                   _lib.current_stream(dev())), "gt_synth_contours")
    got = dec.reverse_rows(rcy, rows, g=spk, pitch_rows=p2, energy_rows=e2).clone()
    torch.cuda.synchronize()
    assert torch.equal(got, want) and torch.isfinite(got).all()
    assert not torch.equal(got, dec.reverse_rows(rcy, rows, g=spk, pitch_rows=p2))            # the energy rows matter
    with pytest.raises(ValueError):
        dec.reverse_rows(rcy, rows, g=spk, pitch=pitch, pitch_rows=p2)
