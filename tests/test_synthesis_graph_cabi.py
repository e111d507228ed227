"""CPU tests of the C-ABI behind the captured synthesis graph: gt_synth_geometry, gt_synth_prior_call,
gt_randn_rows_call and gt_synth_call are declared, exported, mirrored by the binding with the C struct's size, and validate their
arguments before any launch (no device needed)."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVAL, UNSUPPORTED, ALIGN = -1, -2, -3
P = 4096                                                                          # a non-NULL, aligned "pointer" that is never read


def header_text():
    txt = open(os.path.join(ROOT, "include", "glowtts_hip.h")).read()
    return re.sub(r"/\*.*?\*/", "", txt, flags=re.S)


def test_header_declares_the_entries():
    txt = header_text()
    assert re.search(r"typedef\s+struct\s+gt_synth_call\s*\{\s*uint32_t\s+seed\s*;\s*float\s+noise_scale\s*;\s*float\s+noise_scale_w\s*;"
                     r"\s*float\s+length_scale\s*;\s*\}\s*gt_synth_call\s*;", txt)
    assert re.search(r"\bint\s+gt_synth_geometry\s*\(\s*const\s+int32_t\s*\*\s*y_len\s*,", txt)
    assert re.search(r"\bint\s+gt_synth_prior_call\s*\(\s*const\s+gt_synth_prior_args\s*\*\s*args\s*,\s*const\s+gt_synth_call\s*\*\s*call\s*,"
                     r"\s*void\s*\*\s*stream\s*\)\s*;", txt)
    assert re.search(r"\bint\s+gt_randn_rows_call\s*\(.*?const\s+gt_synth_call\s*\*\s*call\s*,\s*uint32_t\s+stream_id\s*,\s*int\s+which_scale\s*,"
                     r"\s*void\s*\*\s*stream\s*\)\s*;", txt, flags=re.S)
    # the by-value entries and their struct keep their signatures
    assert re.search(r"\bint\s+gt_synth_prior\s*\(\s*const\s+gt_synth_prior_args\s*\*\s*args\s*,\s*void\s*\*\s*stream\s*\)\s*;", txt)
    assert re.search(r"\bint\s+gt_randn_rows\s*\(\s*float\s*\*\s*out\s*,\s*int\s+R\s*,\s*int\s+ncol\s*,\s*uint32_t\s+seed\s*,\s*uint32_t\s+stream_id\s*,"
                     r"\s*float\s+scale\s*,\s*void\s*\*\s*stream\s*\)\s*;", txt)


def test_library_exports_the_entries(built):
    from glow_tts_amd import _lib
    L = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("gt_synth_geometry", "gt_synth_prior_call", "gt_randn_rows_call", "gt_synth_call_size"):
        assert hasattr(L, name) and name in _lib.PROTOTYPES, name


def test_struct_mirrors_have_the_c_structs_sizes(built):
    from glow_tts_amd import _lib
    L = _lib.lib()
    assert ctypes.sizeof(_lib.SynthCall) == L.gt_synth_call_size() == 16
    assert [f[0] for f in _lib.SynthCall._fields_] == ["seed", "noise_scale", "noise_scale_w", "length_scale"]
    assert ctypes.sizeof(_lib.SynthPriorArgs) == L.gt_synth_prior_args_size()          # unchanged by the new entries


def test_geometry_argument_validation_needs_no_device(built):
    from glow_tts_amd import _lib
    geo = _lib.lib().gt_synth_geometry
    ok = [P] * 8                                                                  # row0 len_sq y_len_eff rowbatch rowframe rowmask rowutt status
    assert geo(P, 0, 64, 128, *ok, None) == 0                                     # B == 0
    assert geo(P, 3, 64, 0, *ok, None) == 0                                       # R_cap == 0
    assert geo(None, 0, 64, 128, *([None] * 8), None) == 0
    assert geo(P, -1, 64, 128, *ok, None) == INVAL
    assert geo(P, 3, 63, 128, *ok, None) == INVAL                                 # Ty_cap is even
    assert geo(P, 1025, 64, 8192, *ok, None) == UNSUPPORTED                       # B > GT_STEP_MAX_B
    assert geo(P, 3, (1 << 20) + 2, 128, *ok, None) == UNSUPPORTED
    assert geo(None, 3, 64, 128, *ok, None) == INVAL
    for i in (0, 1, 2, 3, 4, 5, 7):                                               # every required output; rowutt (6) is optional
        a = list(ok)
        a[i] = None
        assert geo(P, 3, 64, 128, *a, None) == INVAL, i
    assert geo(P, 3, 64, 11, *ok, None) == INVAL                                  # no room for 3 x 2 halos
    a = list(ok)
    a[0] = P + 2
    assert geo(P, 3, 64, 128, *a, None) == ALIGN
    a = list(ok)
    a[3] = P + 4                                                                  # rowbatch is int64
    assert geo(P, 3, 64, 128, *a, None) == ALIGN


def test_call_entries_argument_validation_needs_no_device(built):
    from glow_tts_amd import _lib
    L = _lib.lib()
    assert L.gt_synth_prior_call(None, P, None) == INVAL
    a = _lib.SynthPriorArgs()
    assert L.gt_synth_prior_call(ctypes.byref(a), None, None) == 0                # R == 0: nothing to do, as the by-value entry
    a.R, a.B, a.C, a.Tx, a.Ty, a.Tp = 128, 3, 80, 19, 64, 36 + 127
    a.x_m = a.cum = a.x_len = a.y_len = a.rows = a.row0 = P
    assert L.gt_synth_prior_call(ctypes.byref(a), None, None) == INVAL            # no call block
    assert L.gt_synth_prior_call(ctypes.byref(a), P + 2, None) == ALIGN
    a.Tx = 513
    assert L.gt_synth_prior_call(ctypes.byref(a), P, None) == UNSUPPORTED
    assert L.gt_randn_rows_call(P, 0, 2, None, 1, 1, None) == 0
    assert L.gt_randn_rows_call(P, 8, 2, None, 1, 1, None) == INVAL
    assert L.gt_randn_rows_call(None, 8, 2, P, 1, 1, None) == INVAL
    assert L.gt_randn_rows_call(P, 8, 2, P, 1, 2, None) == INVAL                  # which_scale: 0 or 1
    assert L.gt_randn_rows_call(P, 8, 2, P + 1, 1, 0, None) == ALIGN
    assert L.gt_randn_rows_call(P + 2, 8, 2, P, 1, 0, None) == ALIGN


def test_call_scalars_are_the_call_block_field_for_field():
    """synthesis.CallScalars.words: the bytes of gt_synth_call_ext built field by field; the plain block is its first 16 bytes"""
    from glow_tts_amd import _lib
    from glow_tts_amd.synthesis import CallScalars
    names = [f[0] for f in _lib.SynthCall._fields_] + [f[0] for f in _lib.SynthCallExt._fields_[1:]]
    assert list(CallScalars._fields) == names                                     # the field order of gt_synth_call_ext
    vals = dict(seed=0xFFFFFFFE, noise_scale=0.667, noise_scale_w=0.8, length_scale=1.3, f0_noise_scale=0.3, energy_noise_scale=0.9,
                pitch_scale=1.25, energy_scale=0.75)
    c = CallScalars(**vals)
    want = _lib.SynthCallExt(_lib.SynthCall(*[vals[k] for k in names[:4]]), *[vals[k] for k in names[4:]])
    ext, plain = c.words(True), c.words(False)
    assert ext.dtype == plain.dtype and str(ext.dtype) == "torch.int32"
    assert ctypes.sizeof(_lib.SynthCallExt) == 32 and ext.numel() * 4 == 32 and plain.numel() * 4 == 16
    assert ext.numpy().tobytes() == bytes(want)
    for i, k in enumerate(names):                                                 # ... and word by word, under the struct's own names
        field = want.base if i < 4 else want
        raw = (ctypes.c_uint32 if k == "seed" else ctypes.c_float)(getattr(field, k))
        assert ext.numpy().tobytes()[4 * i:4 * i + 4] == bytes(raw), k
    assert ext.numpy().tobytes()[:16] == plain.numpy().tobytes() == bytes(want.base)
    assert CallScalars(seed=-1).words(False)[0].item() == -1                      # the seed is taken modulo 2^32
    assert CallScalars(seed=3)[1:] == (1.,) * 7                                   # infer's defaults
