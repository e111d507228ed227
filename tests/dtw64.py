"""What the tests of the synthesis metrics share (csrc/dtw.hip, glow_tts_amd.metrics): the float64 restatement of the
definitions in plain loops, the path checker, and the error bounds, derived here from the fp32 format on the kernels' own fp32
operands.  A plain helper module like tests/resample64.py.

Definitions.  Cepstrum of a log-mel frame m[0..N): c[k] = sqrt(2 / N) sum_n m[n] cos(pi k (n + 1/2) / N), k = 1..K (the orthonormal
DCT-II without c0).  Frame distance d(i, j) = alpha sqrt(sum_k (a_i[k] - b_j[k])^2).  DTW: D(0, 0) = d(0, 0), D(i, j) = d(i, j) +
min(D(i-1, j-1), D(i-1, j), D(i, j-1)), a missing predecessor +inf, the first of that order on equal values; cost = D(Fa-1, Fb-1);
the path runs from (0, 0) to (Fa-1, Fb-1).

Bounds (u = 2^-24, gamma(n) = n u / (1 - n u)).
  cepstrum   N products and N - 1 adds in fp32, one rounding each: |c - c64| <= gamma(N + 1) sum_n |w[k, n] m[n]|.
  distance   a - b: one rounding; its square: one more on a value that carries two (the factor twice): each term of the sum is off by
             at most 3 u relative; the K - 1 adds of non-negative terms add at most (K - 1) u: the sum is within (K + 2) u.  The square
             root halves that and rounds once, the product with alpha rounds once: eps_d = ((K + 2) / 2 + 2) u = (K / 2 + 3) u, to first
             order, for sums that stay normal numbers (features of order 1 do).  The kernel always sums 16 terms (the padding is
             exact zeros, which cost nothing), so K = 16 covers every case: eps_d = 11 u.
  DTW        a computed D along a path of at most Fa + Fb - 1 cells is a sum of computed d's with one rounding per add:
             delta = eps_d + (Fa + Fb) u bounds the relative error of the computed cost of ANY path (all terms non-negative).
             Rounding is monotone, so the computed optimum is at most the computed cost of the float64-optimal path:
             cost <= (1 + delta) D64, and the kernel's own path p has C64(p) <= cost / (1 - delta) <= (1 + 2 delta) D64 to first
             order.  Hence C64(p) - D64 <= 2 delta D64 and |cost - D64| <= 2 delta D64.
  F0 sums    (x - y)^2: three roundings; the cents term is formed in fp64 and rounded once; then at most P - 1 adds:
             |s - s64| <= gamma(P + 3) s64."""
import math

import numpy as np

U = 2.0 ** -24
ALPHA_DB = 10.0 * math.sqrt(2.0) / math.log(10.0)


def gamma(n):
    return n * U / (1.0 - n * U)


def dct_matrix(N, K):
    """float64 [K, N]: rows 1..K of the orthonormal DCT-II"""
    n = np.arange(N, dtype=np.float64)
    k = np.arange(1, K + 1, dtype=np.float64)
    return math.sqrt(2.0 / N) * np.cos(math.pi * k[:, None] * (n[None, :] + 0.5) / N)


def cepstrum64(mel, w):
    """mel [N, F], w [K, N] (the kernel's fp32 operands) -> (c64 [F, K], bound [F, K])"""
    m, w = mel.astype(np.float64), w.astype(np.float64)
    c = np.einsum("kn,nf->fk", w, m)
    mag = np.einsum("kn,nf->fk", np.abs(w), np.abs(m))
    return c, gamma(w.shape[1] + 1) * mag


def dist64(a, b, alpha=1.0):
    """a [Fa, K], b [Fb, K] fp32 operands -> d [Fa, Fb] float64; alpha as the fp32 the kernel is handed"""
    a, b = a.astype(np.float64), b.astype(np.float64)
    return float(np.float32(alpha)) * np.sqrt(((a[:, None, :] - b[None, :, :]) ** 2).sum(-1))


def dtw64(d):
    """the recurrence in plain loops -> (cost, path [(i, j)] forward from (0, 0)); diagonal, then (i-1, j), then (i, j-1) on ties"""
    Fa, Fb = d.shape
    if Fa == 0 or Fb == 0:
        return 0.0, []
    inf = float("inf")
    D = [[inf] * Fb for _ in range(Fa)]
    step = [[0] * Fb for _ in range(Fa)]
    dl = d.tolist()
    for i in range(Fa):
        Di, Dp, di, si = D[i], (D[i - 1] if i else None), dl[i], step[i]
        for j in range(Fb):
            if i == 0 and j == 0:
                Di[0] = di[0]
                continue
            m, s = (Dp[j - 1], 0) if (i and j) else (inf, 0)
            if i and Dp[j] < m:
                m, s = Dp[j], 1
            if j and Di[j - 1] < m:
                m, s = Di[j - 1], 2
            Di[j] = di[j] + m
            si[j] = s
    i, j, path = Fa - 1, Fb - 1, []
    while True:
        path.append((i, j))
        if i == 0 and j == 0:
            break
        s = step[i][j]
        if s != 2:
            i -= 1
        if s != 1:
            j -= 1
    return D[Fa - 1][Fb - 1], path[::-1]


def path_cost64(d, path):
    return float(sum(d[i, j] for i, j in path))


def check_path(rows, n, Fa, Fb):
    """rows int [ld, 2] as the kernel writes them, n = path_len: from (0, 0) to (Fa-1, Fb-1) by steps (1,1) / (1,0) / (0,1), -1 behind"""
    rows = np.asarray(rows)
    assert (rows[n:] == -1).all()
    if Fa == 0 or Fb == 0:
        assert n == 0
        return
    assert max(Fa, Fb) <= n <= Fa + Fb - 1, (n, Fa, Fb)
    p = rows[:n]
    assert tuple(p[0]) == (0, 0) and tuple(p[-1]) == (Fa - 1, Fb - 1)
    st = np.diff(p, axis=0)
    assert (((st == 0) | (st == 1)).all(axis=1) & (st.sum(axis=1) >= 1)).all()


def dtw_delta(Fa, Fb, K=16):
    return (K / 2.0 + 3.0) * U + (Fa + Fb) * U


def dist32_along(a, b, path, alpha=1.0):
    """the kernel's own arithmetic in float32 along a path: sixteen differences, products and a sum over k ascending, the correctly
    rounded square root, times alpha; then the sum of d in path order -> float32"""
    f = np.float32
    a, b, alpha = a.astype(f), b.astype(f), f(alpha)
    total = None
    for i, j in path:
        e = a[i] - b[j]
        sq = e * e
        acc = sq[0]
        for k in range(1, len(sq)):
            acc = f(acc + sq[k])
        d = f(alpha * np.sqrt(acc))
        total = d if total is None else f(d + total)
    return total


def f0_stats64(fa, fb, path):
    """contours in Hz (0 = unvoiced, fp32 operands) along the path -> (n_vv, n_vu, n_gross, sse_hz, sse_cents) in float64"""
    n_vv = n_vu = n_gross = 0
    s_hz = s_ct = 0.0
    for i, j in path:
        x, y = float(fa[i]), float(fb[j])
        if x > 0 and y > 0:
            n_vv += 1
            s_hz += (x - y) ** 2
            s_ct += (1200.0 * math.log2(x / y)) ** 2
            n_gross += abs(x - y) > 0.2 * y
        elif (x > 0) != (y > 0):
            n_vu += 1
    return n_vv, n_vu, n_gross, s_hz, s_ct


def warped_pair(Fa, Fb, K, seed):
    """a random sequence b [Fb, K] and a randomly time-warped, lightly perturbed copy a [Fa, K] of it (fp32): the optimal path runs
    well off the diagonal"""
    rng = np.random.RandomState(seed)
    b = rng.randn(Fb, K).cumsum(0) * 0.3 + rng.randn(Fb, K) * 0.2 if Fb else np.zeros((0, K))
    if Fa == 0 or Fb == 0:
        return rng.randn(Fa, K).astype(np.float32), b.astype(np.float32)
    knots = np.sort(rng.rand(Fa)) ** rng.uniform(0.5, 2.0)
    idx = np.clip(np.round(knots / max(knots[-1], 1e-9) * (Fb - 1)).astype(int), 0, Fb - 1)
    a = b[idx] + rng.randn(Fa, K) * 0.05
    return a.astype(np.float32), b.astype(np.float32)
