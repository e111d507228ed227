"""float64 NumPy restatement of the waveform back end's semantics (helper of tests/test_griffin_lim_*.py, not a test): the inverse
basis pinv(4 fourier_basis).T times the periodic Hann window in closed form, the transform of a reflect-padded utterance, the
inverse (per-frame synthesis, overlap-add, division by the float32 squared-window envelope accumulated as the reference accumulates
it, times 4, 512 samples trimmed at both ends), the Griffin-Lim loop, and the error bounds of the fp32 kernels.  Signals, window and
frames come from tests/mel64.py."""
import numpy as np

import mel64

N, HOP, NBIN = mel64.N, mel64.HOP, mel64.NBIN
U = mel64.U
SCALE = N / HOP

# gt_istft against inverse() on the same fp32 (mag, phase), in units of u * sum |ib| |Y| (overlap-added, over the envelope, times 4):
#   513  products of a fold chain (512 MFMA steps + bin 512), one rounding each
#     1  the basis entry rounded to fp32
#     5  Y = mag * cos(phase): the product's rounding and 2 ulp = 4 u of sincosf
#     1  x = a +- b
#     3  the overlap-add of 4 frames
#    10  the envelope: w rounded, squared (3 u per term), 3 additions in the kernel; 4 roundings in the reference's float32 envelope
#     1  the division (the factor 4 is exact)
C_ISTFT = 513 + 1 + 5 + 1 + 3 + 10 + 1
# the same output against the ORIGINAL signal adds what rounding (mag, phase) to fp32 does to Y, (1 + pi) u |Y|, and the reference's
# float32 envelope, 4 u |x| <= 4 u S: 9 u S
C_RECON = 9
# gt_gl_project: a unit phasor moves by at most 2 |dX| / |X|, |dX| <= sqrt(2) d_f
C_PHASOR = 2.0 * np.sqrt(2.0)
# re^2 + im^2 (fmaf: 2 roundings, 1 u on |X| after the root), sqrtf 1, M / |X| 1, the product 1, and as many again for the other
# component's share of |X|: 8 u M
C_ROUND = 8


def inverse_basis64():
    """[2 * 513, 1024] float64: row k is c_k (cos, -sin)(2 pi k n / N) w[n] / (N * 4), c_k = 1 for bins 0 and 512, else 2; columns n
    and N - n are exact mirrors, the sine rows of bins 0 and 512 exact zeros"""
    k = np.arange(NBIN, dtype=np.int64)[:, None]
    m = (k * np.arange(N // 2 + 1, dtype=np.int64)[None, :]) % N
    ang = 2.0 * np.pi * m.astype(np.float64) / N
    c_k = np.where((k == 0) | (k == N // 2), 1.0, 2.0) / (N * SCALE)
    w = mel64.window64()[None, :N // 2 + 1]
    cos_h = np.cos(ang) * c_k * w
    sin_h = np.where((2 * m) % N == 0, 0.0, -np.sin(ang)) * c_k * w
    full = np.empty((2 * NBIN, N))
    full[:NBIN, :N // 2 + 1], full[NBIN:, :N // 2 + 1] = cos_h, sin_h
    full[:NBIN, N // 2 + 1:], full[NBIN:, N // 2 + 1:] = cos_h[:, N // 2 - 1:0:-1], -sin_h[:, N // 2 - 1:0:-1]
    return full


def pinv_basis64():
    """the reference's construction: float64 pinv(4 * [real; imag] rows of fft(eye(N))).T times the window"""
    fourier = np.fft.fft(np.eye(N))
    basis = np.vstack([np.real(fourier[:NBIN]), np.imag(fourier[:NBIN])])
    return np.linalg.pinv(SCALE * basis).T * mel64.window64()[None, :]


_FWD = None


def transform(x):
    """x [L] -> (re, im) [513, F] float64, F = 1 + L // 256: the windowed DFT of the reflect-padded utterance's frames"""
    global _FWD
    if _FWD is None:
        _FWD = mel64.basis64()
    spec = mel64.frames64(x) @ _FWD.T
    return spec[:, :NBIN].T.copy(), spec[:, NBIN:].T.copy()


def envelope32(F):
    """the reference's window_sumsquare: a float32 buffer to which each frame's float64 w^2 is added in ascending frame order"""
    env = np.zeros(N + HOP * (F - 1), dtype=np.float32)
    w2 = mel64.window64() ** 2
    for f in range(F):
        env[f * HOP:f * HOP + N] += w2
    return env


def _overlap_add(frames):
    F = frames.shape[0]
    out = np.zeros(N + HOP * (F - 1))
    for f in range(F):
        out[f * HOP:f * HOP + N] += frames[f]
    return out


def inverse(re, im, basis=None, envelope=True, imag_sign=1.0):
    """(re, im) [513, F] -> [256 (F - 1)] float64"""
    basis = inverse_basis64() if basis is None else basis
    F = re.shape[1]
    frames = np.asarray(re, dtype=np.float64).T @ basis[:NBIN] + imag_sign * np.asarray(im, dtype=np.float64).T @ basis[NBIN:]
    out = _overlap_add(frames)
    if envelope:
        env = envelope32(F)
        nz = env > np.finfo(np.float32).tiny
        out[nz] /= env[nz].astype(np.float64)
    out *= SCALE
    return out[N // 2:-(N // 2)]


def flat_weight_basis():
    """classic mistake: bins 1..511 weighted like bins 0 and 512 (the one-sided spectrum's factor 2 forgotten)"""
    b = inverse_basis64()
    b[1:NBIN - 1] *= 0.5
    b[NBIN + 1:2 * NBIN - 1] *= 0.5
    return b


def abs_sum(re, im, basis=None):
    """S [256 (F - 1)]: sum |ib| |Y| over the bins and the frames that cover a sample, over the envelope, times 4"""
    basis = np.abs(inverse_basis64() if basis is None else basis)
    F = re.shape[1]
    out = _overlap_add(np.abs(re).T @ basis[:NBIN] + np.abs(im).T @ basis[NBIN:])
    env = envelope32(F).astype(np.float64)
    out = np.where(env > np.finfo(np.float32).tiny, out / np.maximum(env, 1e-300), out) * SCALE
    return out[N // 2:-(N // 2)]


def istft_bound(re, im):
    return C_ISTFT * U * abs_sum(re, im)


def recon_bound(re, im):
    return (C_ISTFT + C_RECON) * U * abs_sum(re, im)


def project64(x, M):
    """-> (Yre, Yim, |X|, S_f): Y = M X / |X| ((M, 0) where X = 0) of the utterance x, and the per-frame sum |w x_f|"""
    re, im = transform(x)
    mag = np.hypot(re, im)
    safe = np.where(mag > 0, mag, 1.0)
    yre = np.where(mag > 0, M * re / safe, M)
    yim = np.where(mag > 0, M * im / safe, 0.0)
    S = np.abs(mel64.frames64(x) * mel64.window64()[None, :]).sum(1)
    return yre, yim, mag, S


def project_bound(M, mag, S):
    """per component of Y: M min(2, c' d_f / |X64|) + c'' u M, d_f = (N + 4) u S_f (tests/mel64.py).  A bin with a tiny |X| has an
    undetermined phase: the first term is then 2 M, and the element stays in the comparison."""
    d = (N + 4) * U * S[None, :]
    with np.errstate(divide="ignore"):
        turn = np.minimum(2.0, C_PHASOR * d / mag)
    return M * turn + C_ROUND * U * M


def convergence(x, M):
    re, im = transform(x)
    return np.linalg.norm(np.hypot(re, im) - M) / np.linalg.norm(M)


def griffin_lim64(M, angles, n_iters):
    """the reference's loop in float64 -> (x_0, x_n)"""
    M = np.asarray(M, dtype=np.float64)
    basis = inverse_basis64()
    x0 = x = inverse(M * np.cos(angles), M * np.sin(angles), basis)
    for _ in range(n_iters):
        re, im = transform(x)
        ang = np.arctan2(im, re)
        x = inverse(M * np.cos(ang), M * np.sin(ang), basis)
    return x0, x


FRAMES_SMALL = (4, 5)


def ragged_frames(tile_frames, tile_hops):
    """frame counts of the GPU tests' ragged batch: 4, 5, then T, T + 1, T + 2 frames for the frame tile and T, T + 1, T + 2 hops
    (one frame more each) for the hop tile, duplicates dropped"""
    out = list(FRAMES_SMALL)
    for f in [tile_frames + i for i in range(3)] + [tile_hops + 1 + i for i in range(3)]:
        if f not in out:
            out.append(f)
    return out


def ragged_signals(frames):
    """mel64's five signals in turn, utterance i with 256 (frames[i] - 1) samples"""
    return [mel64.signal(mel64.SIGNALS[i % len(mel64.SIGNALS)], HOP * (F - 1)) for i, F in enumerate(frames)]
