"""float64 NumPy restatement of the spectral-subtraction denoiser (helper of tests/test_denoise_*.py, not a test): NVIDIA's WaveGlow
`Denoiser` (denoiser.py, mode="zeros") on tests/gl64.py's transform / inverse, in the reference's polar form and in the form the
kernel writes, the geometry rule of the analysis behind a vocoder, and the error bounds of the fp32 kernels — derived, not fitted.

The bound.  shrink(X, c) = X max(1 - c / |X|, 0) on a complex X and a real c >= 0 is the proximal map of c |.|: non-expansive in X,
|shrink(X, c) - shrink(X', c)| <= |X - X'|, and |shrink(X, c) - shrink(X, c')| <= |c - c'| (tests/test_denoise_host.py checks both on
random pairs).  gt_denoise_spec computes the fp32 epilogue of the fp32 DFT X^ with c^ = fl(strength * bias[k]) (strength and bias the
fp32 words the kernel reads, restated exactly in float64 here), so per component of Y[k][f]

  |Y^ - Y64| <= sqrt(2) d_f            |X^ - X64| <= sqrt(2) d_f, d_f = (N + 4) u S_f per component (tests/mel64.py)
              + u c                     the one rounding of the product c^
              + C_EPI u (|X^| + c)      the epilogue's own roundings, counted below; |X^| <= |X64| + sqrt(2) d_f

  C_EPI = 10:  re^2 + im^2 by fmaf is 2 roundings = 1 u on |X| after the root, sqrtf 1 ulp = 2 u: m^ = m (1 + 3 u) enters the
               difference (3 u m) and the divisor (3 u m); the subtraction m - c rounds once (u (m + c), counted as 1 u m + 1 u c);
               the division 1 ulp = 2 u; the product with re or im 1 u; each on a value of at most |X^|.
  Bin 512 is real (y = sign(x) max(|x| - c, 0)): one subtraction — inside the same bound.
There is no phase-indeterminacy cap (the map is continuous at X = 0 for c >= 0), and no element is excluded.

The waveform: gt_istft on Y^ is within gl64.istft_bound of gl64.inverse on the same Y^; inverse is linear, so the spectrum error
passes through it as gl64.abs_sum(bound, bound).  istft_bound is taken on |Y64| + bound >= |Y^|."""
import numpy as np

import gl64 as G
import mel64

N, HOP, NBIN, U = G.N, G.HOP, G.NBIN, G.U
C_EPI = 10


def analysis_frames(n, lost, F_max=None):
    """the geometry rule: a vocoder's row holds 256 max(n - lost, 0) samples for n mel frames (n clamped to the capacity F_max); the
    analysis has samples / 256 + 1 frames, 0 where there is no sample"""
    n = n if F_max is None else min(n, F_max)
    samples = HOP * max(n - lost, 0)
    return samples // HOP + 1 if samples else 0


def shrink(re, im, c):
    """Y = X max(|X| - c, 0) / |X| — the form the kernel writes; X = 0 gives (max(-c, 0), 0).  c broadcasts against [513, F]."""
    re, im = np.asarray(re, dtype=np.float64), np.asarray(im, dtype=np.float64)
    c = np.broadcast_to(np.asarray(c, dtype=np.float64), re.shape)
    m = np.hypot(re, im)
    safe = np.where(m > 0, m, 1.0)
    s = np.maximum(m - c, 0.0) / safe
    return np.where(m > 0, re * s, np.maximum(-c, 0.0)), np.where(m > 0, im * s, 0.0)


def polar(re, im, c):
    """the reference's route: mag, phase = |X|, atan2(Im X, Re X); mag_d = clamp(mag - c, min=0); (mag_d cos(phase), mag_d sin(phase))"""
    re, im = np.asarray(re, dtype=np.float64), np.asarray(im, dtype=np.float64)
    mag, phase = np.hypot(re, im), np.arctan2(im, re)
    mag_d = np.maximum(mag - np.broadcast_to(np.asarray(c, dtype=np.float64), re.shape), 0.0)
    return mag_d * np.cos(phase), mag_d * np.sin(phase)


def c_of(bias, strength):
    """c_k [513, 1] float64 from the fp32 words the kernel reads (the product is exact in float64)"""
    return (np.float64(np.float32(strength)) * np.asarray(bias, dtype=np.float32).astype(np.float64))[:, None]


def denoise64(x, bias, strength, route=shrink):
    """x [L] (L a multiple of 256, > 512) -> dict(re, im: the denoised spectrum [513, F], wav [L], X: (re, im) of the analysis,
    S [F] = sum |w x_f|)"""
    xre, xim = G.transform(x)
    yre, yim = route(xre, xim, c_of(bias, strength))
    yim = yim.copy()
    yim[0], yim[NBIN - 1] = 0.0, 0.0                                                        # their inverse basis rows are zero
    S = np.abs(mel64.frames64(x) * mel64.window64()[None, :]).sum(1)
    return dict(re=yre, im=yim, wav=G.inverse(yre, yim), X=(xre, xim), S=S)


def spec_bound(ref, bias, strength):
    """per component of Y [513, F] (see the module's docstring)"""
    c = c_of(bias, strength)
    dX = np.sqrt(2.0) * (N + 4) * U * ref["S"][None, :]
    return dX + U * c + C_EPI * U * (np.hypot(*ref["X"]) + dX + c)


def wav_bound(ref, bias, strength):
    """per sample: the spectrum bound through the inverse, plus gt_istft's own error on a spectrum of at most |Y64| + bound"""
    sb = spec_bound(ref, bias, strength)
    sb_im = sb.copy()
    sb_im[0], sb_im[NBIN - 1] = 0.0, 0.0
    return G.abs_sum(sb, sb_im) + G.istft_bound(np.abs(ref["re"]) + sb, np.abs(ref["im"]) + sb_im)


# ---- known wrong variants (the GPU test's docstring states by how much each misses, measured here in float64)
def wrong_next_bin(x, bias, strength):
    """the bias of bin k + 1 subtracted from bin k"""
    b = np.asarray(bias, dtype=np.float32)
    return denoise64(x, np.concatenate([b[1:], b[-1:]]), strength)


def wrong_no_clamp(x, bias, strength):
    """the clamp left out: |X| - c goes negative and the phasor flips"""
    def route(re, im, c):
        m = np.hypot(re, im)
        safe = np.where(m > 0, m, 1.0)
        return re * (m - c) / safe, im * (m - c) / safe
    return denoise64(x, bias, strength, route=route)


def clamped_share(x, bias, strength):
    """the share of (bin, frame) elements the subtraction clamps to zero"""
    xre, xim = G.transform(x)
    return float((np.hypot(xre, xim) <= c_of(bias, strength)).mean())
