"""float64 NumPy restatement of the pitch front end's semantics (helper of tests/test_yin*.py, not a test): the reference's
yin.compute_yin with the difference function as the DIRECT sum d[t] = sum_{j < w_len - t} (x[j] - x[j + t])^2 (the reference gets the
same numbers through an FFT), the cumulative-mean normalisation, getPitch's walk and the argmin; frames hop i .. hop i + w_len - 1 for
i in range(0, len - w_len, hop), neither centred nor reflected.

  silence=True   the kernel's one departure: a lag whose running sum of d is 0 gets c = 1 (the reference: 0 / 0 = NaN)
  walk           also reports whether a frame is AMBIGUOUS at eps: some comparison the float64 walk consulted (c[t] against thresh,
                 c[t + 1] against c[t], the two smallest c of the argmin) is within eps relative, so that an fp32 evaluation of c,
                 itself within eps_c of float64, may decide it the other way.  Two smallest c that are EQUAL are not ambiguous:
                 c[0] = 1 and c[1] = d[1] / d[1] = 1 in every frame, and the silence rule's ones, are exact in fp32 as well, and
                 the first index wins in both (a frame whose minimum is that 1 has argmin 0).
  eps_c          = (2 w_len + tau_max + 8) 2^-24: d is a sum of non-negative fp32 terms, each (x - y)^2 within 3 u and the chain of
                 at most w_len additions within w_len u more, so d is within (w_len + 4) u; the prefix sum of non-negatives adds
                 at most tau_max u to the (w_len + 4) u of its terms; one multiply and one divide.
  hop32          NumPy fp32 emulation of the kernel's summation order: per hop h and lag t the chain
                 F_t[h] = sum_{n in hop h} (x[n] - x[n + t])^2 in n order, T_t[h] the same chain stopped after 256 - t mod 256 terms,
                 d_f[t] = ((F[f] + F[f+1]) + F[f+2]) + T[f+3] (t < 256), (F[f] + F[f+1]) + T[f+2] (t >= 256); prefix sum = 8 lags in
                 sequence, then a Hillis-Steele scan over the 64 groups.  (The kernel's fmaf rounds x^2 + acc once; here the exact
                 float64 sum is rounded to fp32, the same value but for a double rounding of about one case in 2^29.)
  defects        three planted ones for tests/test_yin64.py: window="fixed" (w_len - tau_max terms at every lag), descent=False
                 (the first lag below the threshold is returned), centred=True (frames start 512 samples early, reflect-padded)."""
import numpy as np

U = 2.0 ** -24
GET_F0 = dict(sr=22050, w_len=1024, hop=256, f0_min=50, f0_max=600, thresh=0.1)          # the notebooks' get_f0
YIN_DEFAULTS = dict(sr=22050, w_len=512, hop=256, f0_min=100, f0_max=500, thresh=0.1)    # compute_yin's own defaults


def taus(sr, f0_min, f0_max):
    return int(sr / f0_max), int(sr / f0_min)


def eps_c(w_len, tau_max):
    return (2 * w_len + tau_max + 8) * U


def n_frames(L, w_len, hop):
    return len(range(0, L - w_len, hop))


def frames64(x, w_len, hop, centred=False):
    x = np.asarray(x, dtype=np.float64)
    n = n_frames(len(x), w_len, hop)
    if centred:
        x = np.pad(x, (w_len // 2, w_len // 2), mode="reflect")
    return np.stack([x[i * hop:i * hop + w_len] for i in range(n)]) if n else np.zeros((0, w_len))


def difference64(fr, tau_max, window="shrinking"):
    """fr [F, w_len] -> d [F, tau_max]"""
    F, w_len = fr.shape
    tau_max = min(tau_max, w_len)
    d = np.zeros((F, tau_max))
    for t in range(1, tau_max):
        n = w_len - t if window == "shrinking" else w_len - tau_max
        diff = fr[:, :n] - fr[:, t:t + n]
        d[:, t] = (diff * diff).sum(1)
    return d


def cmnd(d, silence=True):
    """c[0] = 1, c[t] = d[t] t / sum_{1..t} d; silence: a zero running sum gives 1 instead of NaN"""
    F, tau_max = d.shape
    cum = np.cumsum(d[:, 1:], axis=1)
    num = d[:, 1:] * np.arange(1, tau_max)[None, :]
    with np.errstate(invalid="ignore", divide="ignore"):
        c = num / cum
    if silence:
        c = np.where(cum > 0, c, 1.0)
    return np.concatenate([np.ones((F, 1)), c], axis=1)


def close(a, b, eps):
    return abs(a - b) <= eps * max(abs(a), abs(b))


def walk(c, tau_min, tau_max, thresh, eps=0.0, descent=True):
    """one frame's c -> (p, ambiguous): getPitch, and whether any comparison it made is within eps relative"""
    amb = False
    t = tau_min
    while t < tau_max:
        amb = amb or close(c[t], thresh, eps)
        if c[t] < thresh:
            while descent and t + 1 < tau_max:
                amb = amb or close(c[t + 1], c[t], eps)
                if not c[t + 1] < c[t]:
                    break
                t += 1
            return t, amb
        t += 1
    return 0, amb


def decide(c, tau_min, tau_max, thresh, eps=0.0, descent=True):
    """c [F, tau_max] -> dict(tau [F] int, harm [F], argmin [F] int (np.argmin), amb_tau [F] bool, amb_argmin [F] bool)"""
    F = c.shape[0]
    tau, harm, am = np.zeros(F, dtype=np.int64), np.zeros(F), np.zeros(F, dtype=np.int64)
    amb_t, amb_a = np.zeros(F, dtype=bool), np.zeros(F, dtype=bool)
    for i in range(F):
        p, amb_t[i] = walk(c[i], tau_min, tau_max, thresh, eps, descent)
        tau[i] = p
        am[i] = int(np.argmin(c[i]))
        harm[i] = c[i, p] if p else c[i].min()
        two = np.sort(c[i])[:2]
        amb_a[i] = two[0] != two[1] and close(two[0], two[1], eps)       # an exact tie (c[0] = c[1] = 1, silence) is one in fp32 too
    return dict(tau=tau, harm=harm, argmin=am, amb_tau=amb_t, amb_argmin=amb_a)


def yin64(x, sr, w_len, hop, f0_min, f0_max, thresh, silence=True, eps=None, window="shrinking", descent=True, centred=False):
    """x [L] -> decide()'s dict plus c [F, tau_max], for the float64 direct-sum restatement (or one of the planted defects)"""
    tau_min, tau_max = taus(sr, f0_min, f0_max)
    eps = eps_c(w_len, tau_max) if eps is None else eps
    c = cmnd(difference64(frames64(x, w_len, hop, centred), tau_max, window), silence)
    out = decide(c, tau_min, tau_max, thresh, eps, descent)
    out["c"] = c
    return out


def contour(tau, sr):
    """f0 = sr / tau, 0 where tau = 0 (float64)"""
    tau = np.asarray(tau, dtype=np.float64)
    return np.where(tau > 0, sr / np.maximum(tau, 1), 0.0)


def argmin_contour(am, tau_min, sr):
    am = np.asarray(am, dtype=np.float64)
    return np.where(am > tau_min, sr / np.maximum(am, 1), 0.0)


def _add32(a, b):
    return (a.astype(np.float64) + b.astype(np.float64)).astype(np.float32)


def hop32(x, tau_max, hop=256, w_len=1024):
    """x [L] float32 -> c [F, tau_max] float32 in the kernel's summation order (w_len = 4 hops, lags < 2 hops)"""
    assert w_len == 4 * hop and tau_max <= 2 * hop
    x = np.asarray(x, dtype=np.float32)
    F = n_frames(len(x), w_len, hop)
    if F == 0:
        return np.zeros((0, tau_max), dtype=np.float32)
    nlag = 2 * hop
    xp = np.concatenate([x, np.zeros((F + 3) * hop + nlag, dtype=np.float32)])          # zeros behind the utterance, as staged
    H = F + 3
    lag = np.arange(nlag)
    stop = hop - lag % hop                                                              # T: after this many terms
    acc = np.zeros((H, nlag), dtype=np.float32)
    T = np.zeros((H, nlag), dtype=np.float32)
    base = np.arange(H)[:, None] * hop
    for n in range(hop):
        d = (xp[base + n] - xp[base + n + lag[None, :]]).astype(np.float32)             # fp32 subtraction
        acc = (acc.astype(np.float64) + d.astype(np.float64) ** 2).astype(np.float32)   # fmaf: one rounding
        T = np.where(stop[None, :] == n + 1, acc, T)
    f = np.arange(F)
    lo = _add32(_add32(_add32(acc[f], acc[f + 1]), acc[f + 2]), T[f + 3])
    hi = _add32(_add32(acc[f], acc[f + 1]), T[f + 2])
    d = np.where(lag[None, :] < hop, lo, hi)
    d[:, 0] = 0.0
    # the prefix sum: 8 lags in sequence, then Hillis-Steele over the 64 groups, then group offset + local prefix
    g = d.reshape(F, nlag // 8, 8)
    loc = np.zeros_like(g)
    loc[:, :, 0] = g[:, :, 0]
    for k in range(1, 8):
        loc[:, :, k] = _add32(loc[:, :, k - 1], g[:, :, k])
    run = loc[:, :, 7].copy()
    off = 1
    while off < run.shape[1]:
        sh = np.concatenate([np.zeros((F, off), dtype=np.float32), run[:, :-off]], axis=1)
        new = _add32(run, sh)
        new[:, :off] = run[:, :off]
        run = new
        off *= 2
    excl = np.concatenate([np.zeros((F, 1), dtype=np.float32), run[:, :-1]], axis=1)
    cum = _add32(np.broadcast_to(excl[:, :, None], loc.shape), loc).reshape(F, nlag)
    num = (d.astype(np.float64) * lag[None, :]).astype(np.float32)
    with np.errstate(invalid="ignore", divide="ignore"):
        c = (num.astype(np.float64) / cum.astype(np.float64)).astype(np.float32)
    c = np.where(cum > 0, c, np.float32(1.0))
    c[:, 0] = 1.0
    return c[:, :tau_max]
