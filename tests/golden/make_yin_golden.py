"""Generate tests/golden/yin_golden.npz by IMPORTING the reference's yin.py where it lies (nothing of it is copied):

    python tests/golden/make_yin_golden.py

Five int16 test signals of at most 12 000 samples and, per signal, what yin.compute_yin returns for x / 32768 (float64) with the
notebooks' get_f0 parameters (1024 / 256 / 50-600 Hz, key suffix `_f0`) and once more with compute_yin's own defaults (512 / 256 /
100-500 Hz, suffix `_def`, a geometry the kernel rejects and tests/yin64.py must still match): pitches, harmonic_rates, argmins.

  noise     uniform noise: unvoiced
  vibrato   a 220 Hz tone with 5 Hz vibrato and two harmonics
  glide     an 80 -> 400 Hz glide
  gated     a 130 Hz tone switched on and off
  silence   a tone between stretches of exact zeros (the reference's 0 / 0 = NaN; the kernel's silence rule)
Every voiced signal carries a 1e-3 noise floor: exactly periodic int16 data makes d exactly 0 at the period, where the reference's
own FFT rounding noise decides its walk."""
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("GLOWTTS_REFERENCE", "/root/reference")
sys.path.insert(0, os.path.dirname(HERE))
import yin64 as Y  # noqa: E402

SIGNALS = ("noise", "vibrato", "glide", "gated", "silence")
L, SR = 1024 + 256 * 40, 22050.0                                                          # 40 frames of 1024 / 256
# the noise floors' seeds.  A period that falls midway between two lags makes c[t] and c[t + 1] agree to 1e-4 at the minimum, a frame no
# fp32 evaluation can be held to; a glide passes through such periods.  The glide's and the gated tone's seeds are ones at which the
# FLOAT64 restatement alone (tests/yin64.py, eps_c) calls no frame ambiguous; tests/test_yin64.py holds every signal to at most 2 %.
SEEDS = dict(noise=11, vibrato=12, glide=16, gated=22, silence=15)


def signal(name):
    n = np.arange(L, dtype=np.float64)
    rng = np.random.default_rng(SEEDS[name])
    floor = 1e-3 * rng.standard_normal(L)
    if name == "noise":
        x = rng.uniform(-0.9, 0.9, L)
    elif name == "vibrato":
        ph = 2.0 * np.pi * (220.0 * n / SR + (6.0 / 5.0) * np.sin(2.0 * np.pi * 5.0 * n / SR) / (2.0 * np.pi))
        x = 0.5 * np.sin(ph) + 0.25 * np.sin(2.0 * ph + 0.3) + 0.12 * np.sin(3.0 * ph + 1.1) + floor
    elif name == "glide":
        f = 80.0 + (400.0 - 80.0) * n / L
        x = 0.7 * np.sin(2.0 * np.pi * np.cumsum(f) / SR) + floor
    elif name == "gated":
        gate = ((n // 2200) % 2 == 0).astype(np.float64)
        x = gate * (0.6 * np.sin(2.0 * np.pi * 130.0 * n / SR) + 0.2 * np.sin(2.0 * np.pi * 260.0 * n / SR)) + floor
    elif name == "silence":
        x = 0.6 * np.sin(2.0 * np.pi * 169.6 * n / SR) + floor                                 # a period of 130.01 lags
        x[:3000] = 0.0
        x[8000:] = 0.0
    else:
        raise KeyError(name)
    return np.round(np.clip(x, -1.0, 1.0) * 32767.0).astype(np.int16)


def main():
    sys.path.insert(0, REF)
    import yin as ref_yin
    out = {"signals": np.array(SIGNALS)}
    for name in SIGNALS:
        xi = signal(name)
        out[f"{name}_wav"] = xi
        x = xi.astype(np.float64) / 32768.0
        for suffix, p in (("f0", Y.GET_F0), ("def", Y.YIN_DEFAULTS)):
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")                                           # the silent frames' 0 / 0
                pitches, harm, argmins, _ = ref_yin.compute_yin(x, p["sr"], p["w_len"], p["hop"], p["f0_min"], p["f0_max"], p["thresh"])
            out[f"{name}_pitches_{suffix}"] = np.asarray(pitches, dtype=np.float64)
            out[f"{name}_harmonic_rates_{suffix}"] = np.asarray(harm, dtype=np.float64)
            out[f"{name}_argmins_{suffix}"] = np.asarray(argmins, dtype=np.float64)
    path = os.path.join(HERE, "yin_golden.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
