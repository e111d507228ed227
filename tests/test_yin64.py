"""CPU tests of the pitch front end's references (no GPU, no library): tests/yin64.py against the recorded outputs of the reference's
yin.compute_yin (tests/golden/yin_golden.npz, written by tests/golden/make_yin_golden.py), the NumPy fp32 emulation of the kernel's
summation order against the derived bound eps_c, and the power of the comparison the GPU tests make.

A frame is set aside as ambiguous when a comparison the float64 walk consulted is within eps_c = (2 w_len + tau_max + 8) 2^-24 = 1.5e-4
relative (tests/yin64.py derives it): the bound comes from the number format, not from any output of the kernel."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import yin64 as Y  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "yin_golden.npz")
SETS = (("f0", Y.GET_F0), ("def", Y.YIN_DEFAULTS))


@functools.lru_cache(maxsize=None)
def golden():
    g = np.load(GOLDEN)
    return {k: g[k] for k in g.files}


def names():
    return [str(s) for s in golden()["signals"]]


@functools.lru_cache(maxsize=None)
def restated(name, suffix):
    p = dict(SETS)[suffix]
    x = golden()[f"{name}_wav"].astype(np.float64) / 32768.0
    return Y.yin64(x, p["sr"], p["w_len"], p["hop"], p["f0_min"], p["f0_max"], p["thresh"])


def test_fixture_is_what_the_issue_describes():
    g = golden()
    assert 1 <= len(names()) <= 6 and os.path.getsize(GOLDEN) < 200 * 1024
    for name in names():
        x = g[f"{name}_wav"]
        assert x.dtype == np.int16 and x.ndim == 1 and len(x) <= 12000
        for suffix, p in SETS:
            n = Y.n_frames(len(x), p["w_len"], p["hop"])
            assert n >= 40
            for k in ("pitches", "harmonic_rates", "argmins"):
                assert g[f"{name}_{k}_{suffix}"].shape == (n,)
    assert (g["noise_pitches_f0"] == 0).all() and (g["vibrato_pitches_f0"] > 0).all()
    sil = g["silence_wav"]
    assert (sil[:3000] == 0).all() and (sil[8000:] == 0).all() and np.abs(sil[3000:8000]).max() > 10000


@pytest.mark.parametrize("suffix", ["f0", "def"])
def test_restatement_equals_the_reference(suffix):
    g, p = golden(), dict(SETS)[suffix]
    tau_min, _ = Y.taus(p["sr"], p["f0_min"], p["f0_max"])
    for name in names():
        r = restated(name, suffix)
        pit, harm, am = (g[f"{name}_{k}_{suffix}"] for k in ("pitches", "harmonic_rates", "argmins"))
        ok = ~(np.isnan(pit) | np.isnan(harm) | np.isnan(am))                            # NaN entries of the reference are masked
        assert ok.sum() >= 0.5 * len(ok), name
        ref_tau = np.where(pit > 0, np.round(p["sr"] / np.where(pit > 0, pit, 1.0)), 0).astype(np.int64)
        assert (ref_tau[ok] == r["tau"][ok]).all(), name
        assert (pit[ok] == Y.contour(r["tau"], p["sr"])[ok]).all(), name
        assert (np.abs(harm[ok] - r["harm"][ok]) <= 1e-9).all(), name
        assert (am[ok] == Y.argmin_contour(r["argmin"], tau_min, p["sr"])[ok]).all(), name


def test_silence_rule_is_the_only_departure():
    p = Y.GET_F0
    x = golden()["silence_wav"].astype(np.float64) / 32768.0
    a = restated("silence", "f0")
    b = Y.yin64(x, p["sr"], p["w_len"], p["hop"], p["f0_min"], p["f0_max"], p["thresh"], silence=False)
    silent = np.isnan(b["c"]).any(1)
    assert silent.sum() >= 5 and (~silent).sum() >= 5
    assert (a["c"][~silent] == b["c"][~silent]).all()
    fully = np.isnan(b["c"][:, 1:]).all(1)
    assert fully.sum() >= 3 and (a["tau"][fully] == 0).all() and (a["harm"][fully] == 1.0).all() and (a["argmin"][fully] == 0).all()
    assert not a["amb_argmin"][fully].any()


def test_float64_sets_aside_at_most_two_percent():
    total = 0
    for name in names():
        r = restated(name, "f0")
        amb = r["amb_tau"] | r["amb_argmin"]
        total += len(amb)
        print(name, "ambiguous frames:", int(amb.sum()), "of", len(amb))
        assert amb.mean() <= 0.02, name
    assert total >= 185


def test_fp32_hop_order_within_eps_c_and_same_decisions():
    p = Y.GET_F0
    tau_min, tau_max = Y.taus(p["sr"], p["f0_min"], p["f0_max"])
    eps = Y.eps_c(p["w_len"], tau_max)
    assert abs(eps - 1.488e-4) < 1e-7
    worst = 0.0
    for name in names():
        x = (golden()[f"{name}_wav"].astype(np.float32) / np.float32(32768.0)).astype(np.float32)
        r = restated(name, "f0")
        c32 = Y.hop32(x, tau_max).astype(np.float64)
        assert c32.shape == r["c"].shape
        rel = np.abs(c32 - r["c"]) / np.abs(r["c"])
        worst = max(worst, float(rel.max()))
        assert (rel <= eps).all(), name
        d = Y.decide(c32, tau_min, tau_max, float(np.float32(p["thresh"])))
        keep_t, keep_a = ~r["amb_tau"], ~r["amb_argmin"]
        assert (d["tau"][keep_t] == r["tau"][keep_t]).all(), name
        assert (d["argmin"][keep_a] == r["argmin"][keep_a]).all(), name
        assert (np.abs(d["harm"][keep_t] - r["harm"][keep_t]) <= eps * np.abs(r["harm"][keep_t])).all(), name
    print(f"fp32 hop order, worst |c32 - c64| / c64 = {worst:.3e} (eps_c = {eps:.3e})")


@pytest.mark.parametrize("defect", [dict(window="fixed"), dict(descent=False), dict(centred=True)], ids=["fixed_window", "no_descent", "centred"])
def test_planted_defect_changes_pitches(defect):
    """the comparison of the GPU tests (tau exact on non-ambiguous frames, at most 2 % set aside) sees each planted defect"""
    p = Y.GET_F0
    shares = {}
    for name in names():
        x = golden()[f"{name}_wav"].astype(np.float64) / 32768.0
        r = restated(name, "f0")
        bad = Y.yin64(x, p["sr"], p["w_len"], p["hop"], p["f0_min"], p["f0_max"], p["thresh"], **defect)
        keep = ~r["amb_tau"]
        shares[name] = float((bad["tau"][keep] != r["tau"][keep]).mean())
    print(defect, shares)
    assert max(shares.values()) > 0.02, shares
