"""What the resampler's tests share (a plain helper module like tests/yin64.py): the float64 direct form of
scipy.signal.resample_poly(x, up, down) with its default window, the case list, and the bound of a fp32 evaluation.

  direct form   (up, down) reduced; half = 10 max(up, down); h = the prototype of 2 half + 1 taps; T = ceil(len(h) / up);
                bank[p, j] = h[p + j up], 0 past the end of h.  An utterance of L samples has n_out = ceil(L up / down) outputs;
                output n: q = n down + half, p = q mod up, k0 = q div up, y[n] = sum_{j < T} bank[p, j] x[k0 - j], x = 0 outside [0, L).
  bound         with u = 2^-24:  |y - y64| <= (T + 2) u sum_j |bank[p, j] x[k0 - j]| + T 2^-126,  y64 the float64 sum on the SAME fp32
                operands (the bank and the samples are rounded before the comparison, not inside it).  T products and T - 1
                additions in any order, fused or not: each term passes through at most T roundings (its product and the additions
                behind it), (1 + u)^T - 1 <= (T + 2) u for T u << 1; a product or partial sum below the normal range loses at most
                2^-149 absolutely, T of them stay far below T 2^-126.  No element is excluded.
  cases         five signals (signal()): uniform noise, a sine at 0.45 of the lower rate, DC at full scale, impulses at samples 0 and
                L - 1, and an int16 full-scale square wave; five rate pairs (PAIRS); a sixth (32 000 Hz) in ALL_PAIRS for the C-ABI."""
import numpy as np

U = 2.0 ** -24
PAIRS = ((48000, 22050), (16000, 22050), (44100, 22050), (24000, 22050), (22050, 16000))
ALL_PAIRS = PAIRS + ((32000, 22050),)
TAPS = {(48000, 22050): 44, (16000, 22050): 21, (44100, 22050): 41, (24000, 22050): 22, (22050, 16000): 28, (32000, 22050): 30}
SIGNALS = ("noise", "sine", "dc", "impulses", "square_i16")
GOLDEN_LENGTHS = ("1", "5", "down+1", "700")


def ratio(orig, new):
    """(up, down) reduced"""
    g = int(np.gcd(int(orig), int(new)))
    return int(new) // g, int(orig) // g


def golden_length(tag, down):
    return down + 1 if tag == "down+1" else int(tag)


def n_out(L, up, down):
    return -(-int(L) * up // down)


def length_for(m, up, down):
    """the shortest input whose n_out is at least m (exactly m wherever up <= down: n_out then takes every value)"""
    L = (m - 1) * down // up + 1
    while n_out(L, up, down) < m:
        L += 1
    while L > 1 and n_out(L - 1, up, down) >= m:
        L -= 1
    return L


def filter64(up, down):
    """the prototype, restated here on its own (audio.resample_filter64 is compared with it and with scipy)"""
    m = max(up, down)
    half = 10 * m
    n = np.arange(-half, half + 1, dtype=np.float64)
    a = n / half
    win = np.i0(5.0 * np.sqrt(np.maximum(0.0, 1.0 - a * a))) / np.i0(5.0)
    x = np.pi * n / m
    h = np.where(n == 0, 1.0, np.sin(x) / np.where(n == 0, 1.0, x)) / m * win
    return h / h.sum() * up


def bank64(h, up):
    T = -(-len(h) // up)
    full = np.zeros(up * T)
    full[:len(h)] = h
    return np.ascontiguousarray(full.reshape(T, up).T)


def terms(x, bank, up, down, count=None, index_shift=0, edges="zero"):
    """[n_out, T] float64 products bank[p, j] x[k0 - j] of every output (count: another number of outputs).  The planted defects of
    tests/test_resample_host.py: index_shift moves q by that many upsampled samples, edges="clamp" repeats the end samples."""
    x = np.asarray(x, dtype=np.float64)
    bank = np.asarray(bank, dtype=np.float64)
    L, T = len(x), bank.shape[1]
    count = n_out(L, up, down) if count is None else count
    if count == 0 or L == 0:
        return np.zeros((count, T))
    q = np.arange(count, dtype=np.int64) * down + 10 * max(up, down) + index_shift
    p, k0 = q % up, q // up
    k = k0[:, None] - np.arange(T, dtype=np.int64)[None, :]
    inside = (k >= 0) & (k < L)
    xv = x[np.clip(k, 0, L - 1)]
    if edges == "zero":
        xv = np.where(inside, xv, 0.0)
    return bank[p] * xv


def direct(x, bank, up, down, **kw):
    """-> (y64 [n_out], the sum of the products' magnitudes [n_out])"""
    t = terms(x, bank, up, down, **kw)
    return t.sum(axis=1), np.abs(t).sum(axis=1)


def bound(mag, T):
    return (T + 2) * U * mag + T * 2.0 ** -126


def twin32(x32, bank32, up, down):
    """a float32 evaluation in tap order (j ascending, product rounded, then the addition rounded): one of the orders the bound covers"""
    t = terms(x32, bank32, up, down)
    acc = np.zeros(t.shape[0], dtype=np.float32)
    for j in range(t.shape[1]):
        acc = (acc + t[:, j].astype(np.float32)).astype(np.float32)
    return acc


def signal(name, L, orig, new, seed=0):
    """one of SIGNALS at L samples: fp32 in [-1, 1], or int16 for the square wave"""
    i = np.arange(L, dtype=np.float64)
    if name == "noise":
        return np.random.default_rng([seed, L, orig]).uniform(-1.0, 1.0, L).astype(np.float32)
    if name == "sine":
        return np.sin(2.0 * np.pi * 0.45 * min(orig, new) / orig * i).astype(np.float32)
    if name == "dc":
        return np.ones(L, dtype=np.float32)
    if name == "impulses":
        x = np.zeros(L, dtype=np.float32)
        x[:1] = x[L - 1:] = 1.0
        return x
    if name == "square_i16":
        return np.where((np.arange(L) // 7) % 2 == 0, 32767, -32768).astype(np.int16)
    raise KeyError(name)


def as_f32(x):
    """the fp32 image of a waveform: int16 scaled by 2^-15 (exact)"""
    return x.astype(np.float32) / np.float32(32768.0) if x.dtype == np.int16 else x
