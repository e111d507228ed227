"""TEST INFRASTRUCTURE ONLY — host (numpy, float64) restatement of gt_randn_keyed (csrc/synth_prosody.hip): the
stochastic predictors' noise keyed by (utterance, token or frame), on top of tests/synth_noise_host.py's generator."""
import numpy as np

import synth_noise_host as H

HALO = 2


def keyed_pair(seed, stream, b, length, ncol, scale=1.0):
    """the draws of utterance b: [length, ncol] float64 — out[t, col] = scale * (e0 | e1 by the parity of col) of (b, s = t, c = col // 2)"""
    col = np.arange(ncol)
    e0, e1 = H.randn_pair(seed, stream, b, np.arange(length)[:, None], (col // 2)[None, :])
    return np.where((col % 2 == 0)[None, :], e0, e1) * scale


def keyed_rows(row0, lengths, R, ncol, seed, stream, scale=1.0):
    """gt_randn_keyed on the rows layout row0 [B + 1] (utterance b's frame t is row row0[b] + HALO + t): [R, ncol] float64, zero on
    every halo / padding / rounding row"""
    out = np.zeros((R, ncol))
    for b, n in enumerate(lengths):
        out[row0[b] + HALO:row0[b] + HALO + n] = keyed_pair(seed, stream, b, n, ncol, scale)
    return out


def keyed_bct(lengths, T, seed, stream, scale=1.0):
    """the same draws as the [B, 2, T] noise tensor a predictor's reverse pass takes (zero past every length)"""
    out = np.zeros((len(lengths), 2, T))
    for b, n in enumerate(lengths):
        out[b, :, :n] = keyed_pair(seed, stream, b, n, 2, scale).T
    return out
