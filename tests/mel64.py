"""float64 NumPy restatement of the mel front end's semantics (helper of tests/test_mel_front_*.py, not a test): per utterance
np.pad(mode="reflect") by 512, frames of 1024 at hop 256, the float64 periodic-Hann-windowed DFT basis, hypot, the 2-norm over the 513
bins, the mel projection and log(max(., clip)).  Also the five test signals and the per-frame error bound of the fp32 kernel."""
import numpy as np

N, HOP, NBIN, CLIP = 1024, 256, 513, 1e-5
U = 2.0 ** -24


def window64():
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(N, dtype=np.float64) / N)          # periodic Hann


def basis64(window=None):
    """[2 * 513, 1024] float64: exact cos / -sin (not an FFT of the identity: no rounding beyond the evaluation), windowed"""
    k = np.arange(NBIN, dtype=np.float64)[:, None]
    n = np.arange(N, dtype=np.float64)[None, :]
    ang = 2.0 * np.pi * ((k * n) % N) / N
    return np.vstack([np.cos(ang), -np.sin(ang)]) * (window64() if window is None else window)[None, :]


def frames64(x):
    """x [L] (L > 512) -> [F, 1024] float64 frames of the reflect-padded utterance, F = 1 + L // 256"""
    x = np.asarray(x, dtype=np.float64)
    xp = np.pad(x, (N // 2, N // 2), mode="reflect")
    F = 1 + len(x) // HOP
    return np.stack([xp[f * HOP:f * HOP + N] for f in range(F)])


def mel64(x, mel_basis, basis=None, clip=CLIP):
    """-> dict(mag [513, F], energy [F], lin [n_mel, F] = mel_basis mag, mel [n_mel, F] = log(max(lin, clip)), S [F] = sum |w x_f|)"""
    fr = frames64(x)
    basis = basis64() if basis is None else basis
    spec = fr @ basis.T                                                                   # [F, 1026]
    mag = np.hypot(spec[:, :NBIN], spec[:, NBIN:]).T
    lin = np.asarray(mel_basis, dtype=np.float64) @ mag
    return dict(mag=mag, energy=np.sqrt((mag * mag).sum(0)), lin=lin, mel=np.log(np.maximum(lin, clip)),
                S=np.abs(fr * window64()[None, :]).sum(1))


def bounds(ref, mel_basis, clip=CLIP):
    """The fp32 kernel's per-frame bounds against `ref` = mel64(...).  A k-ordered fp32 chain of N products has N roundings, the operands
    are rounded once each and the centre fold adds one more: every DFT component is within d_f = (N + 4) u S_f of float64.  Then
      |mag - mag64| <= sqrt(2) d_f + 4 u mag64,     |energy - energy64| <= sqrt(513) sqrt(2) d_f + 520 u energy64,
      |mel - log m| <= log1p(dmel / m) + 4 * 2^-23 * max(1, |log m|),  dmel = mel_basis (sqrt(2) d_f) + 520 u lin64,  m = max(lin64, clip)."""
    d = (N + 4) * U * ref["S"]
    mb = np.asarray(mel_basis, dtype=np.float64)
    m = np.maximum(ref["lin"], clip)
    dmel = mb.sum(1)[:, None] * (np.sqrt(2.0) * d)[None, :] + 520 * U * ref["lin"]
    return dict(mag=np.sqrt(2.0) * d[None, :] + 4 * U * ref["mag"],
                energy=np.sqrt(513.0) * np.sqrt(2.0) * d + 520 * U * ref["energy"],
                mel=np.log1p(dmel / m) + 4 * 2.0 ** -23 * np.maximum(1.0, np.abs(np.log(m))))


SIGNALS = ("noise", "sine_bin40", "loud_quiet", "dc_nyquist", "chirp")
LENGTHS = (513, 1061, 256 * 64 - 1, 256 * 64, 256 * 65 + 255)                              # 3, 5, 64, 65, 66 frames (the tile is 64)


def signal(name, L, sr=22050.0):
    """the five signals of the mel front end's tests, float32 in [-1, 1], at most 34 000 samples"""
    assert L <= 34000
    n = np.arange(L, dtype=np.float64)
    rng = np.random.default_rng(SIGNALS.index(name) + 1)
    if name == "noise":
        x = rng.uniform(-1.0, 1.0, L)
    elif name == "sine_bin40":
        x = 0.9 * np.sin(2.0 * np.pi * 40.0 * n / N)
    elif name == "loud_quiet":                                                              # loud and quiet bins in one frame
        x = 0.99 * np.sin(2.0 * np.pi * 40.37 * n / N) + 1e-4 * rng.standard_normal(L)
    elif name == "dc_nyquist":                                                              # bins 0 and 512 carry the energy
        x = 0.5 + 0.5 * (-1.0) ** n
    elif name == "chirp":                                                                   # linear, 0 -> 11 kHz over the signal
        x = 0.9 * np.sin(2.0 * np.pi * (0.5 * 11000.0 / max(L, 1) * n * n) / sr)
    else:
        raise KeyError(name)
    return np.clip(x, -1.0, 1.0).astype(np.float32)


def ragged_batch():
    """the B = 5 ragged batch: signal i at length LENGTHS[i] -> (list of float32 arrays, lengths)"""
    return [signal(s, L) for s, L in zip(SIGNALS, LENGTHS)], list(LENGTHS)
