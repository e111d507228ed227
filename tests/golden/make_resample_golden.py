"""Writes tests/golden/resample_poly_scipy.npz: scipy.signal.resample_poly's own float64 outputs (scipy 1.15, default window
('kaiser', 5.0), zero padding) for the five rate pairs of tests/resample64.py at L in {1, 5, down + 1, 700} on float64 uniform noise,
and scipy's prototype filter firwin(20 max(up, down) + 1, 1 / max(up, down), window=('kaiser', 5.0)) * up per pair.
Data only; run it by hand where scipy is installed:

    python tests/golden/make_resample_golden.py"""
import os
import sys

import numpy as np
from scipy import signal

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import resample64 as R  # noqa: E402

out = {}
for orig, new in R.PAIRS:
    up, down = R.ratio(orig, new)
    m = max(up, down)
    out[f"{orig}_{new}_h"] = signal.firwin(20 * m + 1, 1.0 / m, window=("kaiser", 5.0)) * up
for orig, new in R.PAIRS:
    up, down = R.ratio(orig, new)
    for tag in R.GOLDEN_LENGTHS:
        L = R.golden_length(tag, down)
        x = np.random.default_rng([orig, L]).uniform(-1.0, 1.0, L)
        out[f"{orig}_{new}_{tag}_x"] = x
        out[f"{orig}_{new}_{tag}_y"] = signal.resample_poly(x, up, down)
np.savez_compressed(os.path.join(HERE, "resample_poly_scipy.npz"), **out)
print("wrote", len(out), "arrays")
