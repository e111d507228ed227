"""TEST INFRASTRUCTURE ONLY — float64 restatement of the ActNorm data-dependent initialisation (csrc/flow_ops.hip: gt_actnorm_ddi, its
stats and finish kernels; the reference's ActNorm.initialize, modules.py:607-619) with bounds derived from the kernel's roundings, a
float32 twin, the planted defects the tests must see, and the operands of tests/test_ddi64.py / tests/test_actnorm_ddi_fp64_gpu.py.

The operation, over the n = sum len valid rows of x [R, C] (every other row of the rows layout is zero):

    M = sum x / n     Q = sum x^2 / n     V = Q - M^2     L = 0.5 ln max(V, 1e-6)     logs = -L     bias = -M e^{-L}

What the kernel rounds, U = 2^-24 one fp32 rounding, u = 2^-53 one fp64 rounding, A = sum |x|:

  sums    fp64, R terms per channel in whatever order the workgroups' atomics land (x^2 is exact in fp64: 48 significant bits), then
          one fp64 division: g = (R + 2) u (1 + U) relative to A / n and to Q — negligible, included.
  m, msq  one fp32 rounding of each quotient:            e_m = U |M| + g A / n          e_q = U Q + g Q
  v       fl(msq - m m), contracted into an fma or not.  m^2 is off M^2 by 2 |M| e_m + e_m^2; an uncontracted product adds
          U m^2 and the subtraction U |msq - p|; the fma's single rounding is the smaller of the two.  With
              e_1 = e_q + 2 |M| e_m + e_m^2 + U (|M| + e_m)^2         e_v = e_1 + U (|V| + e_1)
          |v - V| <= e_v = U (Q + 3 M^2 + |V|) + second-order terms.  The cancellation is real: for a channel of mean 40 and
          deviation 0.2 e_v / V is 1e-2, and the bound says so.
  clamp   max(v, 1e-6f): the fp32 constant is off 1e-6 by c = |fl32(1e-6) - 1e-6| <= U 1e-6.  The comparison is only meaningful where
          the clamp DECISION is not within rounding (`condition`): a channel either has V exactly 0 — a constant channel whose
          value, square and sums are exact in fp32, so m, msq and v carry no error at all: e_m = e_q = e_v = 0, and e_vc = c — or
          V >= 1e-2 with V - e_v > 1e-6 (asserted), where e_vc = e_v.
  l       0.5f logf(vc), the halving exact:              e_L = 0.5 (d + F (|ln Vc| + d)),  d = e_vc / (Vc - e_vc)
          (the logarithm's derivative at the nearer end of [Vc - e_vc, Vc + e_vc]).
  logs    -l, exact:                                     bound_logs = e_L
  bias    fl(-m expf(-l)): e^{-l} is off e^{-L} by the factor e^{+-e_L}, expf by F, the product by U:
              k = e^{e_L} (1 + F) (1 + U)                bound_bias = e^{-L} (|M| (k - 1) + e_m k)

F is the allowance for the PRECISE logf and expf of the device library, relative to their results.  A ROCm installation
carries that library as bitcode only, with no document that states an ulp bound for either function, so F is the
project's FAST_FN = 2^-21 (oracle/rows64.py): four times the fp32 spacing 2^-23, wider than any bound documented for a precise fp32
logarithm or exponential.  Nothing here is measured on the kernel.

`ddi` returns the float64 values and the two bounds; `dtype=numpy.float32` gives the float32 twin: the kernel's contract up to the
quotients (fp64 sums — sums in fp32 would carry gamma_n U sum x^2, which the kernel does not incur and the bound does not allow), then
the reference's own expressions in its order (m_sq - m ** 2, clamp, 0.5 log, -m exp(-logs)) in float32.  `defect=` plants one of
DEFECTS; `defects_for` lists the ones a case can show."""
import numpy as np

from .loss64 import HALO, Layout
from .rows64 import CONTROL_MISS, FAST_FN

U = 2.0 ** -24
U64 = 2.0 ** -53
CLAMP = 1e-6
CLAMP_F32 = float(np.float32(CLAMP))
V_MIN = 1e-2                                     # the condition on the inputs: V exactly 0 or V >= V_MIN
DEFECTS = ("denom_R", "denom_BTp", "no_clamp", "exp_plus", "skip_last", "wrap256")


def _np(x, dtype=np.float64):
    if hasattr(x, "detach"):
        x = x.detach().cpu().numpy()
    return np.asarray(x, dtype=dtype)


def stats(x_rows, valid, n):
    """(M, Q, V, A / n, exact) in float64 over the valid rows; exact[c]: a constant channel whose value and square are exact in fp32."""
    x = _np(x_rows)[np.asarray(_np(valid, bool))]
    n = float(n)
    M, Q, A = x.sum(0) / n, (x * x).sum(0) / n, np.abs(x).sum(0) / n
    V = Q - M * M
    const = (x == x[:1]).all(0) & (x.shape[0] == n)
    exact = const & (M == x[0]) & (Q == x[0] * x[0]) & (Q.astype(np.float32) == Q)
    return M, Q, V, A, exact


def condition(x_rows, valid, n):
    """The condition on the inputs: every channel has V exactly 0 (an exact constant channel) or V >= V_MIN.  -> (V, exact)"""
    M, Q, V, A, exact = stats(x_rows, valid, n)
    ok = np.where(exact, V == 0.0, V >= V_MIN)
    assert ok.all(), f"channels {np.nonzero(~ok)[0].tolist()} have a clamp decision within rounding: V = {V[~ok].tolist()}"
    return V, exact


def ddi(x_rows, valid, n, defect=None, dtype=np.float64, geom=None, g=None):
    """-> (logs [C], bias [C], bound_logs [C], bound_bias [C]), float64 arrays (the twin's values are float32 values).
    x_rows [R, C] the fp32 rows the kernel reads, valid [R] its rows with rowmask != 0, n = sum len.
    geom = (B, Tp) is needed by defect "denom_BTp" only.  g: the relative error of the two sums and their division, where it is not
    the kernel's (tests/test_ddi64.py holds the reference's own fp32 sums to (n + 3) U)."""
    assert defect is None or defect in DEFECTS, defect
    x_rows = _np(x_rows)
    R, C = x_rows.shape
    den = float(n)
    if defect == "denom_R":
        den = float(R)
    if defect == "denom_BTp":
        den = float(geom[0] * geom[1])
    M, Q, V, A, exact = stats(x_rows, valid, n)
    scale = float(n) / den
    Md, Qd = M * scale, Q * scale
    if defect == "wrap256":
        src = np.where(np.arange(C) >= 256, np.arange(C) - 256, np.arange(C))
        Md, Qd = Md[src], Qd[src]
    with np.errstate(divide="ignore", over="ignore", invalid="ignore"):
        if dtype == np.float32:
            m, msq = Md.astype(np.float32), Qd.astype(np.float32)
            v = msq - m ** 2
            vc = v if defect == "no_clamp" else np.maximum(v, np.float32(CLAMP))
            l = np.float32(0.5) * np.log(vc)
            logs, bias = -l, -m * np.exp(l if defect == "exp_plus" else -l)
            assert logs.dtype == bias.dtype == np.float32
        else:
            Vd = Qd - Md * Md
            Vc = Vd if defect == "no_clamp" else np.maximum(Vd, CLAMP)
            L = 0.5 * np.log(Vc)
            logs, bias = -L, -Md * np.exp(L if defect == "exp_plus" else -L)
    logs, bias = logs.astype(np.float64), bias.astype(np.float64)
    if defect == "skip_last":
        logs[C - 1] = bias[C - 1] = 0.0                      # the parameters' values before the initialisation
    # the bounds: of the operation itself, whatever defect the values carry
    g = (R + 2) * U64 * (1 + U) if g is None else g
    e_m = np.where(exact, 0.0, U * np.abs(M) + g * A)
    e_q = np.where(exact, 0.0, U * Q + g * Q)
    e_1 = e_q + 2 * np.abs(M) * e_m + e_m ** 2 + U * (np.abs(M) + e_m) ** 2
    e_v = np.where(exact, 0.0, e_1 + U * (np.abs(V) + e_1))
    clamped = V < CLAMP
    assert (exact | (V - e_v > CLAMP_F32)).all(), "a clamp decision is within rounding (see `condition`)"
    assert (V[exact] == 0.0).all()
    Vc = np.maximum(V, CLAMP)
    e_vc = np.where(clamped, abs(CLAMP_F32 - CLAMP), e_v)
    d = e_vc / (Vc - e_vc)
    Lc = 0.5 * np.log(Vc)
    e_L = 0.5 * (d + FAST_FN * (np.abs(2 * Lc) + d))
    k = np.exp(e_L) * (1 + FAST_FN) * (1 + U)
    bound_bias = np.exp(-Lc) * (np.abs(M) * (k - 1) + e_m * k)
    return logs, bias, e_L, bound_bias


def ratio(got, ref, bound):
    """worst |got - ref| / bound over every element (0 where got == ref; inf where the difference is not finite)"""
    got, ref, bound = _np(got).reshape(-1), _np(ref).reshape(-1), _np(bound).reshape(-1)
    assert got.shape == ref.shape == bound.shape, (got.shape, ref.shape, bound.shape)
    with np.errstate(invalid="ignore", divide="ignore"):
        err = np.abs(got - ref)
        r = np.where(got == ref, 0.0, err / bound)
    r = np.where(np.isfinite(r), r, np.inf)
    return float(r.max())


def compare(name, got_logs, got_bias, x_rows, valid, n, geom=None, defects=(), log=print):
    """The assertion of both tests: |got - ref| <= bound on every element of logs and bias, and against every planted defect's
    reference the same comparison misses (by CONTROL_MISS on logs or on bias).  Prints and returns the worst error / bound."""
    logs, bias, bl, bb = ddi(x_rows, valid, n)
    r_logs, r_bias = ratio(got_logs, logs, bl), ratio(got_bias, bias, bb)
    msg = f"{name}: worst err/bound logs {r_logs:.3g} bias {r_bias:.3g}"
    misses = {}
    for dname in defects:
        dl, db, _, _ = ddi(x_rows, valid, n, defect=dname, geom=geom)
        misses[dname] = max(ratio(got_logs, dl, bl), ratio(got_bias, db, bb))
        msg += f"; {dname} misses by {misses[dname]:.3g}x"
    log(msg)
    assert r_logs <= 1.0 and r_bias <= 1.0, msg
    for dname, miss in misses.items():
        assert miss >= CONTROL_MISS, f"planted defect not seen: {dname} ({msg})"
    return max(r_logs, r_bias)


# ----------------------------------------------------------------------------- the cases of both tests
LENS33 = [12, 1] + [(5 * i) % 12 + 1 for i in range(30)] + [12]          # a one-frame utterance; the first and the last full length
# name -> (lens, T, ragged, round_to, C): C = 2 / 160 / 260 (260: channels on the second trip of the finish kernel's c += 256 loop);
# R <= 64 (one workgroup of the stats kernel), 65, and past 5 * 64; B = 1 and 33; uniform rows with padded frames, ragged rows with
# rounding rows behind the last utterance
CASES = {
    "uniform B=1 R=64 C=2": ([60], 60, False, 1, 2),
    "uniform B=1 R=65 C=160": ([61], 61, False, 1, 160),
    "uniform B=1 R=40 C=260": ([30], 36, False, 1, 260),
    "ragged B=1 R=61 C=160": ([57], 64, True, 1, 160),
    "ragged B=1 R=65 C=260": ([61], 61, True, 1, 260),
    "ragged B=1 R=64 C=2": ([50], 50, True, 64, 2),
    "uniform B=33 R=528 C=260": (LENS33, 12, False, 1, 260),
    "uniform B=33 R=528 C=160": (LENS33, 12, False, 1, 160),
    "ragged B=33 R=384 C=160": (LENS33, 12, True, 64, 160),
    "ragged B=33 R=384 C=260": (LENS33, 12, True, 64, 260),
    "ragged B=33 R=346 C=2": (LENS33, 12, True, 1, 2),
}


def special_channels(C):
    """channel -> (mean, std) or a constant: mel-like (-5, 1.5), the cancelling one (40, 0.2), the constant 0.5 that reaches the clamp;
    every other channel is N(0.3, 1.7^2).  C = 260 has the cancelling and the constant channel on the second trip too."""
    if C == 2:
        return {0: (40.0, 0.2), 1: 0.5}
    return {1: (-5.0, 1.5), 2: (40.0, 0.2), C - 3: (40.0, 0.2), C - 1: 0.5}


def case(name):
    """-> (x_rows float32 [R, C] with zeros in every invalid row, Layout, n)"""
    lens, T, ragged, rnd, C = CASES[name]
    lay = Layout(lens, T, ragged, rnd)
    assert name.split(" R=")[1].split(" ")[0] == str(lay.R) and HALO == 2, (name, lay.R)
    rng = np.random.default_rng(list(CASES).index(name) + 11)
    x = rng.normal(0.3, 1.7, size=(lay.R, C))
    for c, spec in special_channels(C).items():
        x[:, c] = spec if isinstance(spec, float) else rng.normal(spec[0], spec[1], size=lay.R)
    x = (x * lay.valid[:, None]).astype(np.float32)
    return x, lay, int(lay.valid.sum())


def defects_for(name):
    """the planted defects case `name` can show (every case has invalid rows and a clamped channel; "wrap256" needs C > 256)"""
    C = CASES[name][4]
    return [d for d in DEFECTS if d != "wrap256" or C > 256]
