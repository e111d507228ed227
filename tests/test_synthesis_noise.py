"""CPU tests of the synthesis front end: the statistics of its counter-hash Gaussian generator as restated on the
host (tests/synth_noise_host.py — the device is held to that restatement in tests/test_synthesis_front_gpu.py), and the C-ABI of
csrc/synth_front.hip: gt_synth_lengths / gt_synth_prior / gt_randn_rows are declared, exported, mirrored by the binding with the C
struct's size and field order, and validate their arguments before any launch (no device needed).

Every bound is 5 sigma of the statistic's own sampling error under the null hypothesis of independent standard normals, at
n = 2 * 6400 * 160 = 2 048 000 samples per seed: mean 1/sqrt(n), variance sqrt(2/n), kurtosis sqrt(24/n), a correlation over n/2
pairs 1/sqrt(n/2).  |e| <= sqrt(-2 ln 2^-24) = 5.768 by construction (u >= 2^-24)."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import synth_noise_host as H  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEEDS = [0, 1, 2, 12345, 0x7fffffff]
S, C = 6400, 160


def _draw(seed, stream=0, b=0, defect=False):
    """[2, S, C] float64: e0 and e1 of every (s, c); defect: u2 takes h1 again (the planted fault the checks must catch)"""
    h1, h2 = H.hashes(seed, stream, b, np.arange(S)[:, None], np.arange(C)[None, :])
    return np.stack(H.pair_from_hashes(h1, h1 if defect else h2))


def _corr(a, b):
    a, b = a.ravel() - a.mean(), b.ravel() - b.mean()
    return float((a * b).mean() / np.sqrt((a * a).mean() * (b * b).mean()))


def _statistics(e, others):
    """{name: (value, bound)} of one seed's draw e [2, S, C]; others: the draws of seed + 1, b + 1 and stream + 1"""
    n = e.size
    x = e.ravel()
    mu, var = x.mean(), x.var()
    kurt = ((x - mu) ** 4).mean() / var ** 2
    cb = 5.0 / np.sqrt(n / 2)
    out = {"mean": (abs(mu), 5.0 / np.sqrt(n)), "var": (abs(var - 1.0), 5.0 * np.sqrt(2.0 / n)),
           "kurtosis": (abs(kurt - 3.0), 5.0 * np.sqrt(24.0 / n)), "max": (np.abs(x).max(), 5.77),
           "e0~e1": (abs(_corr(e[0], e[1])), cb), "c~c+1": (abs(_corr(e[:, :, :-1], e[:, :, 1:])), cb),
           "s~s+1": (abs(_corr(e[:, :-1], e[:, 1:])), cb)}
    for name, o in others.items():
        out[name] = (abs(_corr(e, o)), cb)
    return out


@pytest.mark.parametrize("seed", SEEDS)
def test_generator_statistics(seed):
    e = _draw(seed)
    assert e.size == 2048000
    st = _statistics(e, {"seed~seed+1": _draw(seed + 1), "b~b+1": _draw(seed, b=1), "stream~stream+1": _draw(seed, stream=1)})
    print(f"seed {seed:#x}: " + ", ".join(f"{k} {v:.3e} (<= {b:.3e})" for k, (v, b) in st.items()))
    for k, (v, b) in st.items():
        assert v <= b, (seed, k, v, b)


def test_a_planted_defect_is_caught():
    """u2 drawn from h1 again instead of h2 = hash_u32(h1 + K3): the angle then depends on the radius, and the checks must say so."""
    e = _draw(12345, defect=True)
    st = _statistics(e, {})
    failed = [k for k, (v, b) in st.items() if v > b]
    print("planted defect fails:", failed)
    assert failed


def test_uniforms_are_exact_in_fp32_and_inside_the_open_interval():
    h = np.array([0, 1, 0x1FF, 0x200, 0x7FFFFFFF, 0xFFFFFFFF], dtype=np.uint32)
    u = H.uniform(h)
    assert (u > 0).all() and (u < 1).all()
    assert np.array_equal(u.astype(np.float32).astype(np.float64), u)
    assert u.min() == 2.0 ** -24 and np.sqrt(-2 * np.log(u.min())) <= 5.77


def test_rows_helper_matches_the_pair_definition():
    r = H.randn_rows(5, 3, 9, H.PITCH, scale=0.5)
    e0, e1 = H.randn_pair(9, H.PITCH, 0, 4, 1)
    assert r.shape == (5, 3) and r[4, 2] == 0.5 * e0
    e0, e1 = H.randn_pair(9, H.PITCH, 0, 2, 0)
    assert r[2, 0] == 0.5 * e0 and r[2, 1] == 0.5 * e1
    p = H.prior_noise(9, 2, 4, 7)
    e0, e1 = H.randn_pair(9, H.PRIOR, 2, 3, 1)
    assert p.shape == (4, 7) and p[1, 6] == e0
    e0, e1 = H.randn_pair(9, H.PRIOR, 2, 2, 3)
    assert p[3, 5] == e1


# ---- the C-ABI (modelled on tests/test_synthesis_cabi.py) ----------------------------------------------------------------------
def header_text():
    txt = open(os.path.join(ROOT, "include", "glowtts_hip.h")).read()
    return re.sub(r"/\*.*?\*/", "", txt, flags=re.S)


def test_header_declares_the_front_end_entries():
    txt = header_text()
    assert re.search(r"\bint\s+gt_synth_lengths\s*\(\s*const\s+float\s*\*\s*dur\s*,", txt)
    assert re.search(r"\bint\s+gt_synth_prior\s*\(\s*const\s+gt_synth_prior_args\s*\*\s*args\s*,\s*void\s*\*\s*stream\s*\)\s*;", txt)
    assert re.search(r"\bint\s+gt_randn_rows\s*\(\s*float\s*\*\s*out\s*,", txt)
    assert re.search(r"typedef\s+struct\s+gt_synth_prior_args\s*\{.*?\}\s*gt_synth_prior_args\s*;", txt, flags=re.S)


def test_library_exports_the_front_end_entries(built):
    from glow_tts_amd import _lib
    L = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("gt_synth_lengths", "gt_synth_prior", "gt_synth_prior_args_size", "gt_randn_rows"):
        assert hasattr(L, name), name
        assert name in _lib.PROTOTYPES, name


def test_struct_mirror_has_the_c_structs_size_and_fields(built):
    from glow_tts_amd import _lib
    L = _lib.lib()
    assert ctypes.sizeof(_lib.SynthPriorArgs) == L.gt_synth_prior_args_size()
    body = re.search(r"typedef\s+struct\s+gt_synth_prior_args\s*\{(.*?)\}\s*gt_synth_prior_args\s*;", header_text(), flags=re.S).group(1)
    names = []
    for decl in body.split(";"):
        for part in decl.split(","):
            m = re.search(r"([A-Za-z_][A-Za-z0-9_]*)\s*(?:\[\d+\])?\s*$", part.strip())
            if m:
                names.append(m.group(1))
    assert names == [f[0] for f in _lib.SynthPriorArgs._fields_]


def test_argument_validation_needs_no_device(built):
    from glow_tts_amd import _lib
    L = _lib.lib()
    INVAL, UNSUPPORTED, ALIGN = -1, -2, -3
    assert L.gt_synth_prior(None, None) == INVAL
    a = _lib.SynthPriorArgs()
    assert L.gt_synth_prior(ctypes.byref(a), None) == 0                          # R == 0: nothing to do
    a.R, a.B = 64, 0
    assert L.gt_synth_prior(ctypes.byref(a), None) == 0                          # B == 0 as well
    a.B = -1
    assert L.gt_synth_prior(ctypes.byref(a), None) == INVAL
    a.R, a.B, a.C, a.Tx, a.Ty, a.Tp = 2 * 36, 2, 80, 19, 64, 36
    assert L.gt_synth_prior(ctypes.byref(a), None) == INVAL                      # required pointers are NULL
    a.x_m = a.cum = a.x_len = a.y_len = a.rows = 4096
    a.Tx = 513
    assert L.gt_synth_prior(ctypes.byref(a), None) == UNSUPPORTED
    a.Tx, a.C = 19, 81
    assert L.gt_synth_prior(ctypes.byref(a), None) == UNSUPPORTED
    a.C, a.R = 80, 2 * 36 + 1
    assert L.gt_synth_prior(ctypes.byref(a), None) == INVAL                      # uniform rows: R == B * Tp
    a.R = 2 * 36
    a.x_m = 4096 + 4
    assert L.gt_synth_prior(ctypes.byref(a), None) == ALIGN
    a.x_m, a.rows = 4096, 4096 + 8
    assert L.gt_synth_prior(ctypes.byref(a), None) == ALIGN
    a.rows, a.z_logs = 4096, 4096 + 4
    assert L.gt_synth_prior(ctypes.byref(a), None) == ALIGN
    # gt_synth_lengths
    assert L.gt_synth_lengths(None, None, None, None, None, 0, 19, None) == 0    # B == 0
    assert L.gt_synth_lengths(None, None, None, None, None, 2, 19, None) == INVAL
    assert L.gt_synth_lengths(None, None, None, None, None, -1, 19, None) == INVAL
    assert L.gt_synth_lengths(4096, 4096, 4096, 4096, None, 2, 513, None) == UNSUPPORTED
    assert L.gt_synth_lengths(4096, 4096, 4096, 4096, None, 2, 0, None) == INVAL
    # gt_randn_rows
    assert L.gt_randn_rows(None, 0, 2, 1, 1, 1.0, None) == 0                     # R == 0
    assert L.gt_randn_rows(None, 8, 2, 1, 1, 1.0, None) == INVAL
    assert L.gt_randn_rows(4096, -1, 2, 1, 1, 1.0, None) == INVAL
    assert L.gt_randn_rows(4096, 8, 0, 1, 1, 1.0, None) == INVAL
    assert L.gt_randn_rows(4096 + 2, 8, 2, 1, 1, 1.0, None) == ALIGN
