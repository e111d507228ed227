"""float64 NumPy restatement of ITU-R BS.1770-4 integrated loudness and of the normalisation rule (helper of tests/test_loudness_*.py,
not a test), written from the definition alone: the K-weighting cascade run SERIALLY over the whole utterance, 100 ms segment sums,
400 ms blocks, both gates, the gain; then the chunked decomposition csrc/loudness.hip uses (zero-state pass, transition scan, second
pass) restated on top of it, four known wrong variants, the ragged test cases, and the error bounds of the kernels — derived, not fitted.

The bound.  The cascade is linear with the state (s1, s2 of the shelf, s1, s2 of the high-pass; transposed direct
form II).  A rounding error committed anywhere — in a filter step of either pass, in the state scan — is an error INJECTED into one
state slot at one sample index, and travels to the output z through the cascade's own impulse response from that slot.  With
G_i = sum_n |h_i[n]| the l1 gain from slot i to z (computed here by running the filter on unit states) and eps_i a bound on what one
sample index injects into slot i over all passes,

    |z^ - z64| <= dz = sum_i G_i eps_i,    eps_i = U64 (filter_i(pass 3) + filter_i(pass 1) + scan_i)

  filter_i   a state update is two fused multiply-adds: 2 roundings, each at most U64 times the sum of the addends' magnitudes A_i
             (A_0 = |b1 x| + |a1 y| + |s2| and so on); the output y = b0 x + s1 rounds once and is a slot-0 injection (U64 |y|), z
             likewise for slot 2.  The magnitudes are taken from the float64 run itself: of the serial filter for pass 3, of the
             zero-state chunk runs for pass 1.
  scan_i     s_k = M s_{k-1} + e_k is four fused multiply-adds a row: 4 U64 (sum_j |M_ij| S_j + E_i) with S_j = max |state_j| and
             E_i <= S_i + sum_j |M_ij| S_j; it runs twice with M (a run from zero, then from its true start), twice with M^16 (the
             same one level up) and once with M^256.
             M itself is the exact power of the one-sample matrix rounded once (audio.kweighting_transition64): U64 sum_j |M_ij| S_j
             more, counted as a fifth rounding.
             Counting them at every sample index where they occur once in Lc (16 Lc, 256 Lc) only makes the bound larger.
Then a sum of n squares in order, E = sum z^2:  |E^ - E64| <= sum (2 |z| dz + dz^2) + (n + 2) U64 E, a block z_j likewise over its four
segments, l = 10 log10 carries a relative error rho of its argument to 10 / ln 10 * rho LU, and the gated means are means of positive
terms (relative error at most the worst term's) as long as the gated SETS agree — which the cases guarantee: every block of every case
lies at least GATE_MARGIN = 1e-3 LU from both gates (asserted by `cases`).  The stats row is fp32: L and g round once more (2^-24).

    |L^ - L64| <= 10 / ln 10 * (rho + 8 U64) + 2^-24 |L64|               rho = max over the blocks of A of the block's relative bound
    |y^ - g64 x| <= |g64 x| (2 * 2^-24 + 2^-48 + ln 10 / 20 * dL_double)  g's rounding to fp32, the product's, g's own error"""
import functools

import numpy as np

U64, U32 = 2.0 ** -53, 2.0 ** -24
GATE_MARGIN = 1e-3
ABS_GATE, REL_GATE, OFFSET = -70.0, -10.0, -0.691

# the constants of the recommendation's two filters, as the issue states them
SHELF_DB, SHELF_Q, SHELF_HZ, SHELF_VB = 3.99984385397, 0.7071752369554193, 1681.9744509555319, 0.499666774155
HP_Q, HP_HZ = 0.5003270373253953, 38.13547087613982
TABLE_48K = ((1.53512485958697, -2.69169618940638, 1.19839281085285), (-1.69065929318241, 0.73248077421585),
             (-1.99004745483398, 0.99007225036621))


def kweighting(fs):
    """((b, a) of the shelf, (b, a) of the high-pass), float64, a[0] = 1"""
    K = np.tan(np.pi * SHELF_HZ / fs)
    Vh = 10.0 ** (SHELF_DB / 20.0)
    Vb = Vh ** SHELF_VB
    a0 = 1.0 + K / SHELF_Q + K * K
    b = np.array([(Vh + Vb * K / SHELF_Q + K * K) / a0, 2.0 * (K * K - Vh) / a0, (Vh - Vb * K / SHELF_Q + K * K) / a0])
    a = np.array([1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / SHELF_Q + K * K) / a0])
    K = np.tan(np.pi * HP_HZ / fs)
    a0 = 1.0 + K / HP_Q + K * K
    return (b, a), (np.array([1.0, -2.0, 1.0]), np.array([1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / HP_Q + K * K) / a0]))


def step(coef, x, s, mags=None):
    """one sample through the cascade; x and the four states are floats or arrays (one entry per chunk).  -> (z, new states).
    mags (a list of 6 running maxima: the addend sums of the four state updates, |y|, |z|) is updated where given."""
    (b, a), (c, d) = coef
    s1, s2, t1, t2 = s
    y = b[0] * x + s1
    z = c[0] * y + t1
    if mags is not None:
        for i, v in enumerate((np.abs(b[1] * x) + np.abs(a[1] * y) + np.abs(s2), np.abs(b[2] * x) + np.abs(a[2] * y),
                               np.abs(c[1] * y) + np.abs(d[1] * z) + np.abs(t2), np.abs(c[2] * y) + np.abs(d[2] * z), np.abs(y), np.abs(z))):
            mags[i] = max(mags[i], float(np.max(v)))
    return z, (b[1] * x - a[1] * y + s2, b[2] * x - a[2] * y, c[1] * y - d[1] * z + t2, c[2] * y - d[2] * z)


def kfilter(x, fs, state=(0.0, 0.0, 0.0, 0.0), want_state=False, want_shelf=False):
    """z = highpass(shelf(x)), serially over the whole signal in Python floats (float64); want_shelf: (z, y = shelf(x))"""
    (b, a), (c, d) = kweighting(fs)
    b0, b1, b2, a1, a2 = (float(v) for v in (*b, a[1], a[2]))
    c0, c1, c2, d1, d2 = (float(v) for v in (*c, d[1], d[2]))
    s1, s2, t1, t2 = (float(v) for v in state)
    out, mid = np.empty(len(x)), np.empty(len(x))
    for n, xn in enumerate(np.asarray(x, dtype=np.float64).tolist()):
        y = b0 * xn + s1
        mid[n] = y
        s1 = b1 * xn - a1 * y + s2
        s2 = b2 * xn - a2 * y
        z = c0 * y + t1
        t1 = c1 * y - d1 * z + t2
        t2 = c2 * y - d2 * z
        out[n] = z
    if want_shelf:
        return out, mid
    return (out, (s1, s2, t1, t2)) if want_state else out


def transition(fs, n):
    """M [4, 4]: n samples of zero input take the state s to M s — by running the filter itself on the four unit states"""
    coef = kweighting(fs)
    M = np.zeros((4, 4))
    for j in range(4):
        s = tuple(1.0 if i == j else 0.0 for i in range(4))
        for _ in range(n):
            _, s = step(coef, 0.0, s)
        M[:, j] = s
    return M


def lk(z):
    with np.errstate(divide="ignore"):
        return OFFSET + 10.0 * np.log10(z)


def blocks(z, fs, overlap=0.75):
    """(segment sums E [S], block mean squares z_j [J]) of the filtered signal z; below 400 ms: one block over all of it"""
    Ns, N = fs // 10, len(z)
    Nb = 4 * Ns
    if N == 0:
        return np.zeros(0), np.zeros(0)
    if N < Nb:
        return np.zeros(0), np.array([np.sum(z * z) / N])
    E = np.array([np.sum(z[s * Ns:(s + 1) * Ns] ** 2) for s in range(N // Ns)])
    hop = int(round(4 * (1.0 - overlap)))                  # segments between two blocks: 1 at 75 %, 2 at 50 %
    J = (N // Ns - 4) // hop + 1
    return E, np.array([E[j * hop:j * hop + 4].sum() / Nb for j in range(J)])


def gate(zj, relative=True, offset=OFFSET):
    """(L, Gamma, A, R) of the block mean squares: A, R boolean masks"""
    with np.errstate(divide="ignore"):
        l = offset + 10.0 * np.log10(zj)
    A = l > ABS_GATE
    if not A.any():
        return -np.inf, -np.inf, A, A.copy()
    with np.errstate(divide="ignore"):
        gamma = offset + 10.0 * np.log10(zj[A].mean()) + REL_GATE
    R = A & (l > gamma) if relative else A
    return float(offset + 10.0 * np.log10(zj[R].mean())), float(gamma), A, R


def gain(L, peak, target, peak_dbfs):
    """(g, whether the peak rule engaged)"""
    if L == -np.inf:
        return 1.0, False
    g, ceil = 10.0 ** ((target - L) / 20.0), 10.0 ** (peak_dbfs / 20.0)
    if peak > 0 and g * peak > ceil:
        return ceil / peak, True
    return g, False


def loudness64(x, fs, target=-23.0, peak_dbfs=-1.0, z=None, overlap=0.75, relative=True, offset=OFFSET):
    """x [N] -> dict(L, gamma, peak, g, engaged, J, nA, nR, E, zj, A, R, z)"""
    x = np.asarray(x, dtype=np.float64)
    z = kfilter(x, fs) if z is None else z
    E, zj = blocks(z, fs, overlap)
    L, gamma, A, R = gate(zj, relative, offset)
    peak = float(np.abs(x).max()) if len(x) else 0.0
    g, engaged = gain(L, peak, target, peak_dbfs)
    return dict(L=L, gamma=gamma, peak=peak, g=g, engaged=engaged, J=len(zj), nA=int(A.sum()), nR=int(R.sum()), E=E, zj=zj, A=A, R=R, z=z)


# ---- the chunked decomposition, restated: zero-state pass, M scan, second pass (vectorised over the chunks)
def chunked(x, fs, Lc, drop_state=False, mags=None):
    """z of x by chunks of Lc samples: every chunk from zero state -> its end state e_k; s_k = M s_{k-1} + e_k; every chunk again from
    s_{k-1}.  drop_state: the wrong variant that starts every chunk from zero.  mags: step's running maxima, for the zero-state pass."""
    x = np.asarray(x, dtype=np.float64)
    N = len(x)
    if N == 0:
        return np.zeros(0)
    coef, K = kweighting(fs), -(-N // Lc)
    xp = np.zeros(K * Lc)
    xp[:N] = x
    xp = xp.reshape(K, Lc)
    s = tuple(np.zeros(K) for _ in range(4))
    for i in range(Lc):                                    # (the padded tail of the last chunk runs too: its end state is never used)
        _, s = step(coef, xp[:, i], s, mags)
    e = np.stack(s, 1)                                     # [K, 4]
    start = np.zeros((K, 4))
    if not drop_state:
        M = transition(fs, Lc)
        for k in range(1, K):
            start[k] = M @ start[k - 1] + e[k - 1]
    s = tuple(start[:, i].copy() for i in range(4))
    z = np.empty((K, Lc))
    for i in range(Lc):
        z[:, i], s = step(coef, xp[:, i], s)
    return z.reshape(-1)[:N]


# ---- the bounds
@functools.lru_cache(maxsize=None)
def slot_gains(fs):
    """G [4]: sum_n |z[n]| of the zero-input response to a unit in state slot i (the l1 gain from an injection there to the output)"""
    G = np.zeros(4)
    for i in range(4):
        z = kfilter(np.zeros(fs // 2), fs, state=tuple(1.0 if j == i else 0.0 for j in range(4)))
        assert np.abs(z[-fs // 20:]).max() < 1e-12 * np.abs(z).max()      # decayed: the tail adds nothing
        G[i] = np.abs(z).sum()
    return G


def z_bound(x, fs, Lc):
    """dz: the bound on |z^ - z64| at every sample (see the module's docstring)"""
    x = np.asarray(x, dtype=np.float64)
    if len(x) == 0:
        return 0.0
    (b, a), (c, d) = kweighting(fs)
    z, y = kfilter(x, fs, want_shelf=True)
    # the serial run's states after every sample, from x, y and z: s2 = b2 x - a2 y, s1 = b1 x - a1 y + s2[n - 1], and so on
    s2, t2 = b[2] * x - a[2] * y, c[2] * y - d[2] * z
    s2p, t2p = np.concatenate([[0.0], s2[:-1]]), np.concatenate([[0.0], t2[:-1]])
    s1, t1 = b[1] * x - a[1] * y + s2p, c[1] * y - d[1] * z + t2p
    serial = [np.max(np.abs(b[1] * x) + np.abs(a[1] * y) + np.abs(s2p)), np.max(np.abs(b[2] * x) + np.abs(a[2] * y)),
              np.max(np.abs(c[1] * y) + np.abs(d[1] * z) + np.abs(t2p)), np.max(np.abs(c[2] * y) + np.abs(d[2] * z)),
              np.max(np.abs(y)), np.max(np.abs(z))]
    smax = np.array([np.abs(v).max() for v in (s1, s2, t1, t2)])
    zero = [0.0] * 6
    chunked(x, fs, Lc, mags=zero)
    eps = np.zeros(4)
    for m in (serial, zero):
        eps += np.array([2 * m[0] + m[4], 2 * m[1], 2 * m[2] + m[5], 2 * m[3]])
    M1 = transition(fs, Lc)
    for M, times in ((M1, 2), (np.linalg.matrix_power(M1, 16), 2), (np.linalg.matrix_power(M1, 256), 1)):
        eps += times * 5 * (2 * np.abs(M) @ smax + smax)
    return float(U64 * (slot_gains(fs) @ eps))


def sum_bound(z, dz, n_terms):
    """bound on a sum of squares of the values z taken in order, each within dz"""
    z = np.abs(z)
    return float(np.sum(2 * z * dz + dz * dz) + (n_terms + 2) * U64 * np.sum(z * z))


def bounds(x, fs, ref, Lc):
    """dict(dz, dE [S] on the segment sums, rho: the worst relative bound over the blocks, dL_double, dL on the fp32 L)"""
    Ns, N = fs // 10, len(x)
    dz = z_bound(x, fs, Lc)
    z = ref["z"]
    dE = np.array([sum_bound(z[s * Ns:(s + 1) * Ns], dz, Ns) for s in range(len(ref["E"]))])
    if N == 0 or not ref["A"].any():
        return dict(dz=dz, dE=dE, rho=0.0, dL_double=0.0, dL=0.0)
    if N < 4 * Ns:
        rho = sum_bound(z, dz, N) / np.sum(z * z)
    else:
        rho = max((dE[j:j + 4].sum() + 4 * U64 * ref["E"][j:j + 4].sum()) / ref["E"][j:j + 4].sum() for j in np.flatnonzero(ref["A"]))
    dLd = 10.0 / np.log(10.0) * (rho + 8 * U64)
    return dict(dz=dz, dE=dE, rho=float(rho), dL_double=float(dLd), dL=float(dLd + U32 * abs(ref["L"])))


def sample_bound(x, ref, dL_double):
    """per sample of y = fp32(g) x against g64 x"""
    return np.abs(ref["g"] * np.asarray(x, dtype=np.float64)) * (2 * U32 + U32 * U32 + np.log(10.0) / 20.0 * dL_double + 4 * U64)


# ---- known wrong variants (float64; the GPU test's docstring states by how much each misses the bound on L)
def wrong_dropped_state(x, fs, Lc, **kw):
    return loudness64(x, fs, z=chunked(x, fs, Lc, drop_state=True), **kw)


def wrong_no_relative_gate(x, fs, Lc, **kw):
    return loudness64(x, fs, relative=False, **kw)


def wrong_no_offset(x, fs, Lc, **kw):
    return loudness64(x, fs, offset=0.0, **kw)


def wrong_half_overlap(x, fs, Lc, **kw):
    return loudness64(x, fs, overlap=0.5, **kw)


WRONG = (wrong_dropped_state, wrong_no_relative_gate, wrong_no_offset, wrong_half_overlap)


# ---- the cases: seeded noise bursts at staggered levels, one level per 100 ms segment
LEVELS = {"L": 0.3, "M": 0.3 * 10.0 ** (-30.0 / 20.0), "T": 0.3 * 10.0 ** (-75.0 / 20.0)}
PATTERN = "LLLLMMMMTTTTTLLLL"                              # blocks of every mixture: both gates bite from 13 segments on


def burst(N, fs, seed):
    """fp32 [N]: uniform noise, segment s at the level PATTERN[s mod 17]"""
    rng = np.random.default_rng(seed)
    Ns = fs // 10
    amp = np.array([LEVELS[PATTERN[(n // Ns) % len(PATTERN)]] for n in range(0, max(N, 1), Ns)]).repeat(Ns)[:N]
    return (rng.uniform(-1.0, 1.0, N) * amp).astype(np.float32)


def gate_margin(ref):
    """the least distance in LU of a block's level from the gate that decides it (inf where there is no block)"""
    l = lk(ref["zj"])
    d = [np.abs(l - ABS_GATE)]
    if ref["A"].any():
        d.append(np.abs(l[ref["A"]] - ref["gamma"]))
    d = np.concatenate(d) if len(l) else np.zeros(0)
    return float(d.min()) if len(d) else np.inf


def cases(fs, lengths, seed=0, targets=(-23.0,), peak_dbfs=-1.0):
    """[(x fp32, {target: loudness64's dict})] for the lengths; asserts the condition on the cases: every block at least GATE_MARGIN
    from both gates, and the peak rule decided by a relative margin of 1e-6"""
    out = []
    for i, N in enumerate(lengths):
        x = burst(N, fs, seed + i)
        base = loudness64(x, fs, targets[0], peak_dbfs)
        assert gate_margin(base) >= GATE_MARGIN, (fs, N, gate_margin(base))
        refs = {}
        for t in targets:
            g, engaged = gain(base["L"], base["peak"], t, peak_dbfs)
            if base["L"] > -np.inf and base["peak"] > 0:
                free = 10.0 ** ((t - base["L"]) / 20.0) * base["peak"] / 10.0 ** (peak_dbfs / 20.0)
                assert abs(free - 1.0) > 1e-6, (fs, N, t)
            refs[t] = dict(base, g=g, engaged=engaged)
        out.append((x, refs))
    return out
