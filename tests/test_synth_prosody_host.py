"""CPU tests behind full-model synthesis: the host restatement of gt_synth_frame_geometry against
RowsCtx.row_starts and against its own invariants under overflow, the keyed-noise restatement against the generator, and the new
C-ABI entries — declared, exported, mirrored with the C struct's size, and validating their arguments before any launch."""
import ctypes
import os
import random
import re
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import synth_frame_geometry_host as FG  # noqa: E402
import synth_geometry_host as G  # noqa: E402
import synth_noise_host as H  # noqa: E402
import synth_prosody_host as PH  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVAL, UNSUPPORTED, ALIGN = -1, -2, -3
P = 4096                                                                          # a non-NULL, aligned "pointer" that is never read
HALO = 2


def header_text():
    txt = open(os.path.join(ROOT, "include", "glowtts_hip.h")).read()
    return re.sub(r"/\*.*?\*/", "", txt, flags=re.S)


def test_frame_geometry_restatement_equals_row_starts(built):
    """where the rows fit: RowsCtx.row_starts(y_len_eff, T = Ty_cap) with starts[B] = Rf_cap, then gt_rows_ctx_fill's tables"""
    from glow_tts_amd.ops import RowsCtx
    rng = random.Random(4)
    for B, Ty_cap in ((1, 9), (3, 64), (37, 801), (1024, 30)):
        lens = [rng.randint(1, Ty_cap) for _ in range(B)]
        lens[0], lens[-1] = Ty_cap, 1
        for rnd in (8, 128):
            starts, R = RowsCtx.row_starts(lens, Ty_cap, rnd)
            got = FG.frame_geometry(lens, Ty_cap, R)
            assert got["status"] == 0 and got["row0"] == starts and got["len_f"] == lens
            for b in range(B):
                rows = range(starts[b], starts[b + 1])
                assert all(got["rowbatch"][m] == b for m in rows)
                assert [got["rowframe"][m] for m in rows] == [m - starts[b] - HALO for m in rows]
                assert [got["rowmask"][m] for m in rows] == [1.0 if 0 <= m - starts[b] - HALO < lens[b] else 0.0 for m in rows]
    # lengths above the frame capacity are clipped (gt_synth_geometry's y_len_eff never is: the kernel clips all the same)
    assert FG.frame_geometry([70, 3], 64, 256)["len_f"] == [64, 3]


def test_frame_geometry_restatement_under_overflow():
    rng = random.Random(5)
    for B, Ty_cap in ((1, 40), (3, 64), (50, 33)):
        lens = [rng.randint(1, Ty_cap) for _ in range(B)]
        need = sum(v + 2 * HALO for v in lens)
        for cap in (need - 1, need - 7, (need + 2 * HALO * B) // 2, 2 * HALO * B):
            got = FG.frame_geometry(lens, Ty_cap, cap)
            r0, lf = got["row0"], got["len_f"]
            assert got["status"] == FG.BIT_FRAME_ROWS
            assert r0[0] == 0 and r0[B] == cap and all(r0[b] <= r0[b + 1] for b in range(B))
            assert all(0 <= lf[b] <= lens[b] and lf[b] + 2 * HALO <= r0[b + 1] - r0[b] for b in range(B))
            assert len(got["rowbatch"]) == len(got["rowframe"]) == len(got["rowmask"]) == cap
            assert sum(got["rowmask"]) == sum(lf) < sum(lens)
            # the closed form the kernel uses: row0[b] = min(unclipped offset, cap - 2 HALO (B - b))
            off = 0
            for b in range(B):
                assert r0[b] == min(off, cap - 2 * HALO * (B - b))
                off += lens[b] + 2 * HALO


def test_frame_geometry_is_the_squeezed_rule_on_whole_frames():
    """the same overflow rule as gt_synth_geometry: on even lengths 2 v the squeezed geometry of 2 v equals the frame geometry of v"""
    lens = [5, 1, 9, 3]
    for cap in (40, 31, 20, 16):
        a, b = FG.frame_geometry(lens, 12, cap), G.geometry([2 * v for v in lens], 24, cap)
        assert a["row0"] == b["row0"] and a["len_f"] == b["len_sq"] and a["rowframe"] == b["rowframe"] and a["rowmask"] == b["rowmask"]
        assert (a["status"] != 0) == bool(b["status"] & G.BIT_ROWS)


def test_keyed_noise_restatement():
    """a draw depends on (seed, stream, utterance, frame, column pair) only — not on where the rows layout puts the frame"""
    lens = [1, 7, 12]
    a = PH.keyed_rows([0, 5, 16, 40], lens, 40, 2, 11, H.PITCH, 0.5)
    b = PH.keyed_rows([0, 9, 24, 64], lens, 64, 2, 11, H.PITCH, 0.5)
    for (ra, rb), n in zip(((0, 0), (5, 9), (16, 24)), lens):
        assert np.array_equal(a[ra + HALO:ra + HALO + n], b[rb + HALO:rb + HALO + n])
    e0, e1 = H.randn_pair(11, H.PITCH, 2, 3, 0)
    assert a[16 + HALO + 3, 0] == 0.5 * e0 and a[16 + HALO + 3, 1] == 0.5 * e1
    assert (a[:HALO] == 0).all() and (a[HALO + 1:5 + HALO] == 0).all() and (a[16 + HALO + 12:] == 0).all()
    bct = PH.keyed_bct(lens, 12, 11, H.PITCH, 0.5)
    assert np.array_equal(bct[1, :, :7].T, a[5 + HALO:5 + HALO + 7]) and (bct[1, :, 7:] == 0).all()
    assert not np.array_equal(PH.keyed_rows([0, 5, 16, 40], lens, 40, 2, 11, H.ENERGY, 0.5), a)


def test_header_declares_the_entries():
    txt = header_text()
    assert re.search(r"typedef\s+struct\s+gt_synth_call_ext\s*\{\s*gt_synth_call\s+base\s*;\s*float\s+f0_noise_scale\s*;\s*float\s+"
                     r"energy_noise_scale\s*;\s*float\s+pitch_scale\s*;\s*float\s+energy_scale\s*;\s*\}\s*gt_synth_call_ext\s*;", txt)
    for name in ("gt_randn_keyed", "gt_randn_keyed_call", "gt_synth_frame_geometry", "gt_synth_contours", "gt_synth_contours_call",
                 "gt_synth_call_ext_size"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", txt), name
    # the call block of the plain synthesiser keeps its layout
    assert re.search(r"typedef\s+struct\s+gt_synth_call\s*\{\s*uint32_t\s+seed\s*;\s*float\s+noise_scale\s*;\s*float\s+noise_scale_w\s*;"
                     r"\s*float\s+length_scale\s*;\s*\}\s*gt_synth_call\s*;", txt)


def test_library_exports_the_entries_and_struct_sizes(built):
    from glow_tts_amd import _lib
    L = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("gt_randn_keyed", "gt_randn_keyed_call", "gt_synth_frame_geometry", "gt_synth_contours", "gt_synth_contours_call",
                 "gt_synth_call_ext_size"):
        assert hasattr(L, name) and name in _lib.PROTOTYPES, name
    L = _lib.lib()
    assert ctypes.sizeof(_lib.SynthCallExt) == L.gt_synth_call_ext_size() == 32
    assert ctypes.sizeof(_lib.SynthCall) == L.gt_synth_call_size() == 16                # unchanged
    assert _lib.SynthCallExt.base.offset == 0 and _lib.SynthCallExt.f0_noise_scale.offset == 16
    assert [f[0] for f in _lib.SynthCallExt._fields_] == ["base", "f0_noise_scale", "energy_noise_scale", "pitch_scale", "energy_scale"]


def test_randn_keyed_argument_validation_needs_no_device(built):
    from glow_tts_amd import _lib
    L = _lib.lib()
    k, kc = L.gt_randn_keyed, L.gt_randn_keyed_call
    assert k(P, P, 40, P, 3, 0, 2, 1, 1, 1.0, None) == 0                          # R == 0
    assert k(P, P, 40, P, 3, -1, 2, 1, 1, 1.0, None) == INVAL
    assert k(P, P, 40, P, 3, 64, 0, 1, 1, 1.0, None) == INVAL
    assert k(None, P, 40, P, 3, 64, 2, 1, 1, 1.0, None) == INVAL
    assert k(P, P, 40, None, 3, 64, 2, 1, 1, 1.0, None) == INVAL                  # lengths
    assert k(P, P, 40, P, 0, 64, 2, 1, 1, 1.0, None) == INVAL                     # rows without an utterance
    assert k(P, None, 40, P, 3, 64, 2, 1, 1, 1.0, None) == INVAL                  # uniform rows: R == B * Tp
    assert k(P + 2, P, 40, P, 3, 64, 2, 1, 1, 1.0, None) == ALIGN
    assert k(P, P + 1, 40, P, 3, 64, 2, 1, 1, 1.0, None) == ALIGN
    assert k(P, P, 40, P, 3, 1 << 30, 5, 1, 1, 1.0, None) == UNSUPPORTED
    # the _call form: as gt_randn_rows_call
    assert kc(P, P, 40, P, 3, 0, 2, None, 1, 1, None) == 0
    assert kc(P, P, 40, P, 3, 8, 2, None, 1, 1, None) == INVAL
    assert kc(None, P, 40, P, 3, 8, 2, P, 1, 1, None) == INVAL
    assert kc(P, P, 40, P, 3, 8, 2, P, 1, 4, None) == INVAL                       # which_scale: 0 .. 3
    assert kc(P, P, 40, P, 3, 8, 2, P, 1, -1, None) == INVAL
    assert kc(P, P, 40, P, 3, 8, 2, P + 1, 1, 0, None) == ALIGN
    assert kc(P + 2, P, 40, P, 3, 8, 2, P, 1, 3, None) == ALIGN


def test_frame_geometry_argument_validation_needs_no_device(built):
    from glow_tts_amd import _lib
    geo = _lib.lib().gt_synth_frame_geometry
    ok = [P] * 7                                                                  # row0_f len_f rowbatch rowframe rowmask rowutt status
    assert geo(P, 0, 64, 128, *ok, None) == 0                                     # B == 0
    assert geo(P, 3, 64, 0, *ok, None) == 0                                       # Rf_cap == 0
    assert geo(P, -1, 64, 128, *ok, None) == INVAL
    assert geo(P, 1025, 64, 8192, *ok, None) == UNSUPPORTED
    assert geo(P, 3, (1 << 20) + 1, 128, *ok, None) == UNSUPPORTED
    assert geo(None, 3, 64, 128, *ok, None) == INVAL
    for i in (0, 1, 2, 3, 4, 6):                                                  # every required output; rowutt (5) is optional
        a = list(ok)
        a[i] = None
        assert geo(P, 3, 64, 128, *a, None) == INVAL, i
    assert geo(P, 3, 64, 11, *ok, None) == INVAL                                  # no room for 3 x 2 halos
    a = list(ok)
    a[0] = P + 2
    assert geo(P, 3, 64, 128, *a, None) == ALIGN
    a = list(ok)
    a[2] = P + 4                                                                  # rowbatch is int64
    assert geo(P, 3, 64, 128, *a, None) == ALIGN


def test_contours_argument_validation_needs_no_device(built):
    from glow_tts_amd import _lib
    L = _lib.lib()

    def call(pr=P, er=P, row0_f=P, Tp_f=40, len_f=P, Rf=64, row0=P, Tp=30, len_sq=P, R_=48, psig=P, esig=P, pitch=P, energy=P, B=3, Ty=20,
             blk=False):
        head = (pr, er, row0_f, Tp_f, len_f, Rf, row0, Tp, len_sq, R_, psig, esig, pitch, energy, B, Ty)
        return L.gt_synth_contours_call(*head, blk, None) if blk is not False else L.gt_synth_contours(*head, 1.0, 1.0, None)

    assert call(B=0) == 0
    assert call(B=-1) == INVAL and call(R_=-1) == INVAL
    assert call(len_f=None) == INVAL and call(len_sq=None) == INVAL
    assert call(row0_f=None) == INVAL and call(row0=None) == INVAL                # uniform rows: the row counts are B * Tp
    assert call(Rf=0) == INVAL                                                    # inputs without rows
    assert call(pr=P + 2) == ALIGN and call(pitch=P + 1) == ALIGN
    assert call(psig=P + 4) == ALIGN and call(esig=P + 4) == ALIGN                # a row's two parities are one 8-byte store
    assert call(blk=None) == INVAL and call(blk=P + 2) == ALIGN
