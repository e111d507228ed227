"""float64 NumPy restatement of the mel-inversion kernel's semantics (csrc/gl_mel.hip: gt_gl_from_mel; helper of
tests/test_gl_mel_*.py, not a test): the phase generator in integer arithmetic (tests/synth_noise_host.py's hash on stream 4), the
magnitudes mag64 = max(pinv32 exp(mel32), 0) on the kernel's own fp32 operands, the spectrum mag64 (cos pi t, sin pi t) with t exact,
and the error bounds of the fp32 kernel.  The bounds are COUNTED, in units of u = 2^-24 times S[j, f] = sum_k |pinv[j, k]| exp(mel[k, f]):

  magnitudes   c_m = n_mel + 1 + 4
      n_mel  roundings of the k-ascending chain (one per fmaf)
          1  the product's rounding (an MFMA form rounds it; the fmaf chain does not — counted either way)
          4  expf: 1 ulp in the HIP math API's table, counted as 2 ulp = 4 u as tests/gl64.py counts sincosf
      the clamp max(., 0) is 1-Lipschitz: |max(a, 0) - max(b, 0)| <= |a - b|, so no element is left out.
  spectrum     c_s = c_m + 1 + 4
          1  the product mag * cos / mag * sin
          4  sincospif: 1 ulp in the table, counted as 2 ulp = 4 u (|cos|, |sin| <= 1 and mag64 <= S)
For n_mel = 80: c_m = 85, c_s = 90; for n_mel = 37: 42 and 47."""
import numpy as np

import mel64
import synth_noise_host as SN

U = mel64.U
NBIN = mel64.NBIN
PHASE_STREAM = 4                                     # 0..3: the prior, duration, pitch and energy draws
C_EXP, C_SINCOS = 4, 4


def c_mag(n_mel):
    return n_mel + 1 + C_EXP


def c_spec(n_mel):
    return c_mag(n_mel) + 1 + C_SINCOS


def phase_hash(seed, b, f, j, stream=PHASE_STREAM):
    """uint32, broadcast over f and j: hash_u32(key(seed, stream, b) + f K1 + j K2) mod 2^32"""
    k = SN._u64(SN.key(seed, stream, b))
    return SN.hash_u32((k + SN._u64(f) * np.uint64(SN.K1) + SN._u64(j) * np.uint64(SN.K2)) & SN._M32)


def phase_u(h):
    """u = ((h >> 9) + 0.5) 2^-23 in (0, 1)"""
    return SN.uniform(h)


def phase_t(seed, b, F, nbin=NBIN, stream=PHASE_STREAM):
    """t [nbin, F] float64 = 2 u - 1 = (2 (h >> 9) + 1 - 2^23) 2^-23: an odd integer below 2^23 in magnitude over 2^23, exact in
    fp32; the phase is pi t"""
    h = phase_hash(seed, b, np.arange(F)[None, :], np.arange(nbin)[:, None], stream)
    m = (h >> np.uint32(9)).astype(np.int64)
    return (2 * m + 1 - 2 ** 23).astype(np.float64) * 2.0 ** -23


def mag64(pinv32, mel32):
    """[513, F] float64 on the kernel's own fp32 operands"""
    return np.maximum(pinv32.astype(np.float64) @ np.exp(mel32.astype(np.float64)), 0.0)


def abs_sum(pinv32, mel32):
    return np.abs(pinv32.astype(np.float64)) @ np.exp(mel32.astype(np.float64))


def mag_bound(pinv32, mel32):
    return c_mag(pinv32.shape[1]) * U * abs_sum(pinv32, mel32)


def spec_bound(pinv32, mel32):
    return c_spec(pinv32.shape[1]) * U * abs_sum(pinv32, mel32)


def spectrum64(m64, t):
    """(re, im) [513, F]: mag64 (cos pi t, sin pi t); Im of bin 512 is not kept by the layout (reads back as 0), Im of bin 0 is"""
    re, im = m64 * np.cos(np.pi * t), m64 * np.sin(np.pi * t)
    im[NBIN - 1] = 0.0
    return re, im


def chain32(pinv32, e32, clamp=True):
    """fp32 emulation of the kernel's sum: ONE chain over k ascending, each step the fp32 rounding of the exact p * e + acc (the
    product of two fp32 is exact in float64; the float64 sum's own rounding is 2^29 times finer than the fp32 one that follows)"""
    acc = np.zeros((pinv32.shape[0], e32.shape[1]), dtype=np.float32)
    p64, e64 = pinv32.astype(np.float64), e32.astype(np.float64)
    for k in range(pinv32.shape[1]):
        acc = (p64[:, k:k + 1] * e64[k:k + 1, :] + acc.astype(np.float64)).astype(np.float32)
    return np.maximum(acc, np.float32(0.0)) if clamp else acc


# ---- the GPU tests' ragged batch ------------------------------------------------------------------------------------------------------
def ragged_frames(tile_frames):
    """frame counts at the layout's edges: 4, 5, the 32-frame group, the Griffin-Lim tile T and T + 1"""
    return [4, 5, 31, 32, 33, tile_frames, tile_frames + 1]


def ragged_signals(frames):
    return [mel64.signal(mel64.SIGNALS[i % len(mel64.SIGNALS)], mel64.HOP * (F - 1)) for i, F in enumerate(frames)]
