"""TEST INFRASTRUCTURE ONLY — float64 restatement of gt_adamw_flat (csrc/optim.hip), written from the comment above its kernel:

    hyper = {lr, beta1, beta2, eps, weight_decay, t}            (t already incremented for this update)
    m' = b1 m + (1 - b1) g;   v' = b2 v + (1 - b2) g^2;   bc_i = 1 - b_i^t
    p' = p (1 - lr wd) - U,   U = lr / bc1 * m' / den,   den = sqrt(v') / sqrt(bc2) + eps
    gnorm_sq += sum g^2                                          (one atomic per workgroup)

`step` takes the kernel's OWN fp32 operands (p, g, m, v and the six hyper values as the fp32 numbers the device holds) as float64
and returns {"p" | "m" | "v": (ref, bound)} for rows64.check / check_with_control, which add the output's own rounding 2^-24 |ref|.

The bounds follow from the build: -O3 without fast-math, so +, *, / and sqrtf are correctly rounded (one rounding u = 2^-24
relative, or tiny = 2^-149 absolute where a result is subnormal) and powf is the only library function.  1 - b is exact for
b in [1/2, 1] (Sterbenz), so ob1, ob2 carry no error.

  e_m = 3u (|b1 m| + |(1 - b1) g|) + tiny        a product and the sum on each term; an FMA contraction only removes a rounding
  e_v = 4u v' + tiny                             two products and the sum on the g^2 term; every term is non-negative
  e_p = 3u |p decay| + c u |U| + (lr / bc1) e_m / den + |U| e_v / (2 sqrt(v') sqrt(bc2) den) + tiny
        3u |p decay|    decay = fl(1 - fl(lr wd)) and the product
        c u |U|         c = 16 + E (r1 + r2 / 2): at most 16 roundings on the way from m', v' to U (sqrtf, / bc2s, + eps, the
                        roundings inside bc1, bc2s, step_size, the product, the quotient; second-order terms), and powf's error of
                        E ulps carried through the cancellation in 1 - b^t: r_i = b_i^t / (1 - b_i^t), halved under the root
        the e_m term    U is linear in m'
        the e_v term    d sqrt(v') = e_v / (2 sqrt(v')), then / sqrt(bc2) and through 1 / den; where v' = 0 it is
                        sqrt(tiny) / den |U|
  For t >= 1000 with the project's betas b^t underflows or is below 1e-8: r_i = 0 and nothing in the bound is measured.

POWF_ULPS (E) is the one number here that is not derived; DESIGN.md 4.19 says where it comes from.

`gnorm_sq`: ref = prior + sum g^2, bound = gamma(K) sum g^2 + u |prior|, K the longest chain of fp32 additions behind the result:
4 per grid-stride trip of a thread, 6 for the wave butterfly, 3 for the four waves, one atomic per workgroup.

Planted defects (`defect=`): the wrong rules the tests must see (rows64.CONTROL_MISS) — `required` says where each one is visible at
all.  `case` is the operand recipe and HYPERS / TS the grid shared by tests/test_adamw64.py (a numpy float32 emulation of the kernel's
statement order, CPU) and tests/test_adamw_fp64_gpu.py (the kernel)."""
import math

import numpy as np

from .rows64 import RHO, gamma

U32 = RHO["f32"]               # one fp32 rounding, relative
TINY = 2.0 ** -149             # the smallest fp32 subnormal: one rounding of a subnormal result, absolute
POWF_ULPS = 1                  # E: powf's error in ulps

# csrc/optim.hip's launch geometry: float4 per thread, 256 threads per workgroup, at most 1024 workgroups, grid-stride beyond
WG, VEC, MAX_BLOCKS = 256, 4, 1024
CAP = MAX_BLOCKS * WG * VEC    # floats one trip of the grid covers

DEFECTS = ("eps_inside", "eps_under_root", "step_minus_one", "no_bias_correction", "coupled_decay", "no_decay")
BIAS_DEFECTS = ("eps_inside", "step_minus_one", "no_bias_correction")

# (lr, beta1, beta2, eps, weight_decay): the project's AdamW at the top and at the bottom of the OneCycle range, and torch's defaults
# turned up (b2 = .999 keeps the bias correction alive at t = 1000, lr wd = 2e-4 makes the decay visible on every element)
HYPERS = ((2e-4, .9, .98, 1e-9, .01), (8e-6, .95, .98, 1e-9, .01), (2e-3, .85, .999, 1e-8, .1))
TS = (1, 2, 10, 100, 1000, 100000)


def hyper32(lr, b1, b2, eps, wd, t):
    """the six values as the device holds them (fp32)"""
    return np.asarray([lr, b1, b2, eps, wd, t], dtype=np.float32)


def _a(x):
    if hasattr(x, "detach"):
        x = x.detach().cpu().numpy()
    return np.asarray(x, dtype=np.float64)


def launch_blocks(n):
    """workgroups gt_adamw_flat launches for n floats"""
    return min(MAX_BLOCKS, (n // VEC + WG - 1) // WG)


def _pow(b, t):
    return float(np.power(np.float64(b), np.float64(t)))           # underflows to 0 for large t, like powf


def step(p, g, m, v, hyper, E=POWF_ULPS, defect=None):
    """One update of n floats in float64 -> {"p": (p', e_p), "m": (m', e_m), "v": (v', e_v)} (numpy float64; bounds without the
    output's own rounding).  defect (the bounds stay those of the true rule's formulas on the defective values):
      eps_inside          den = (sqrt(v') + eps) / sqrt(bc2)
      eps_under_root      den = sqrt(v' / bc2 + eps)
      step_minus_one      bias corrections with t - 1 (t = 1: b^0 = 1 would divide by zero; no correction then)
      no_bias_correction  bc1 = bc2 = 1
      coupled_decay       g + wd p in place of g, no decoupled factor
      no_decay            p' = p - U"""
    assert defect is None or defect in DEFECTS, defect
    p, g, m, v = _a(p), _a(g), _a(m), _a(v)
    lr, b1, b2, eps, wd, t = (float(h) for h in _a(hyper).reshape(6))
    tt = t - 1 if defect == "step_minus_one" else t
    if defect == "no_bias_correction" or tt == 0:
        pw1 = pw2 = 0.0
    else:
        pw1, pw2 = _pow(b1, tt), _pow(b2, tt)
    bc1, bc2 = 1.0 - pw1, 1.0 - pw2
    decay = 1.0 if defect in ("no_decay", "coupled_decay") else 1.0 - lr * wd
    ge = g + wd * p if defect == "coupled_decay" else g
    m1 = b1 * m + (1.0 - b1) * ge
    v1 = b2 * v + (1.0 - b2) * ge * ge
    root = np.sqrt(v1)
    if defect == "eps_inside":
        den = (root + eps) / math.sqrt(bc2)
    elif defect == "eps_under_root":
        den = np.sqrt(v1 / bc2 + eps)
    else:
        den = root / math.sqrt(bc2) + eps
    upd = lr / bc1 * m1 / den
    p1 = p * decay - upd

    e_m = 3 * U32 * (np.abs(b1 * m) + np.abs((1.0 - b1) * ge)) + TINY
    e_v = 4 * U32 * v1 + TINY
    c = 16.0 + E * (pw1 / bc1 + 0.5 * pw2 / bc2)
    au = np.abs(upd)
    with np.errstate(divide="ignore", invalid="ignore"):
        through_root = np.where(v1 > 0, au * e_v / (2.0 * root * math.sqrt(bc2) * den), math.sqrt(TINY) / den * au)
    e_p = 3 * U32 * np.abs(p * decay) + c * U32 * au + (lr / bc1) * e_m / den + through_root + TINY
    return {"p": (p1, e_p), "m": (m1, e_m), "v": (v1, e_v)}


def powf_ulps_needed(got_p, p, g, m, v, hyper):
    """The smallest E with which `got_p` passes step()'s bound on p' (the bound is linear in E); <= 0: the derived part alone holds
    it.  Measuring only: no test asserts with it."""
    ref, b0 = step(p, g, m, v, hyper, E=0.0)["p"]
    b1 = step(p, g, m, v, hyper, E=1.0)["p"][1]
    need = np.abs(_a(got_p) - ref) - b0 - U32 * np.abs(ref)
    slope = b1 - b0
    with np.errstate(divide="ignore", invalid="ignore"):
        e = np.where(need > 0, need / slope, 0.0)
    return float(np.max(e)) if e.size else 0.0


def required(defect, hyper):
    """Whether a check of p' must see `defect` at these hyper-parameters.
      coupled_decay, eps_under_root   everywhere: wd p against g, and eps against v' / bc2, differ on the recipe's elements at any t
      the bias-correction defects     differ from the true rule only through b^t: required where b2^t >= 2^-10 (the project's
                                      b2 = .98 to t = 100, b2 = .999 at t = 1000); beyond, b^t sinks under fp32's rounding of
                                      1 - b^t and the rules are the same
      no_decay                        changes p' by lr wd |p| against a bound of about 4u |p| (3u |p decay| and p''s own rounding):
                                      required where lr wd >= 2^-20 = 16u, which leaves the factor CONTROL_MISS; at lr wd = 8e-8
                                      the change is under one ulp of p"""
    lr, b1, b2, eps, wd, t = (float(h) for h in _a(hyper).reshape(6))
    if defect in BIAS_DEFECTS:
        return _pow(b2, t) >= 2.0 ** -10
    if defect == "no_decay":
        return lr * wd >= 2.0 ** -20
    return True


def gnorm_depth(n, blocks=None):
    blocks = launch_blocks(n) if blocks is None else blocks
    trips = -(-(n // VEC) // (blocks * WG)) if blocks else 0
    return 4 * trips + 6 + 3 + blocks


def gnorm_sq(g, prior=0.0, drop=()):
    """One launch over g (n floats): (ref, bound) as 1-element arrays.  prior: what gnorm_sq held.  drop: indices left out of the sum
    (the planted defect)."""
    g = _a(g).reshape(-1)
    sq = g * g
    s = float(sq.sum())
    drop = np.asarray(sorted(drop), dtype=np.int64)
    ref = float(prior) + s - float(sq[drop].sum())
    return np.asarray([ref]), np.asarray([gamma(gnorm_depth(g.size)) * s + U32 * abs(float(prior))])


def gnorm_sq_launches(g, ranges, prior=0.0, drop=()):
    """Several launches into one gnorm_sq, each over floats [s, e) of g: every launch's result is the next one's prior (its own
    rounding u |ref| joins the bound).  -> (ref, bound)"""
    g = _a(g).reshape(-1)
    ref, bound = np.asarray([float(prior)]), np.asarray([0.0])
    for k, (s, e) in enumerate(ranges):
        d = [i - s for i in drop if s <= i < e]
        r, b = gnorm_sq(g[s:e], float(ref[0]), d)
        bound = bound + b + (U32 * np.abs(ref) if k else 0.0)
        ref = r
    return ref, bound


# ----------------------------------------------------------------------------- numpy float32 emulation of the kernel's statement order
def emulate32(p, g, m, v, hyper, prior=0.0):
    """The kernel's statements in numpy float32, in its order, without FMA contraction -> (p', m', v', gnorm_sq) float32.  The sum
    follows the kernel's tree: per-thread chain over the grid-stride trips, xor butterfly over 64 lanes, four waves, one add per
    workgroup onto `prior` in workgroup order."""
    f = np.float32
    p, g, m, v = (np.asarray(x, dtype=f).reshape(-1) for x in (p, g, m, v))
    lr, b1, b2, eps, wd, t = (f(h) for h in np.asarray(hyper, dtype=f).reshape(6))
    one = f(1)
    bc1 = one - np.power(b1, t)
    bc2s = np.sqrt(one - np.power(b2, t))
    step_size, decay, ob1, ob2 = lr / bc1, one - lr * wd, one - b1, one - b2
    m1 = b1 * m + ob1 * g
    v1 = b2 * v + ob2 * g * g
    p1 = p * decay - step_size * m1 / (np.sqrt(v1) / bc2s + eps)
    assert p1.dtype == m1.dtype == v1.dtype == f
    n = g.size
    blocks = launch_blocks(n)
    acc = f(prior)
    if blocks:
        threads = blocks * WG
        trips = -(-(n // VEC) // threads)
        sq = np.zeros(trips * threads * VEC, dtype=f)
        sq[:n] = g * g
        sq = sq.reshape(trips, threads, VEC)
        ss = np.zeros(threads, dtype=f)
        for i in range(trips):
            for k in range(VEC):
                ss = ss + sq[i, :, k]
        ss = ss.reshape(blocks * 4, 64)
        lane = np.arange(64)
        for off in (32, 16, 8, 4, 2, 1):
            ss = ss + ss[:, lane ^ off]
        red = ss[:, 0].reshape(blocks, 4)
        per_wg = ((red[:, 0] + red[:, 1]) + red[:, 2]) + red[:, 3]
        for b in range(blocks):
            acc = f(acc + per_wg[b])
    return p1, m1, v1, f(acc)


# ----------------------------------------------------------------------------- operands
def case(n, seed=0):
    """p, g, m, v (float32 [n]) by index mod 8, so that every special value lands in every position of a float4 and of a lane pair:
      |g| log-uniform in [1e-12, 1e3] with a random sign; g = 0 on residue 3
      p ~ N(0, 1); p = 0 on residue 5 (the update is the whole result); p 1e-4 on residue 6 (|p| ~ lr)
      m ~ s N(0, 1) / 2, v ~ s^2 U(1/4, 4) at the gradient's scale s, each exactly 0 on a random third of the elements — among
      them v = 0, g = 0, m != 0, where the update is m' / eps; element 3 is always that case."""
    rng = np.random.default_rng(1000003 * seed + n)
    res = np.arange(n) % 8
    s = 10.0 ** rng.uniform(-12.0, 3.0, n)
    g = s * rng.choice([-1.0, 1.0], n)
    g[res == 3] = 0.0
    p = rng.standard_normal(n)
    p[res == 5] = 0.0
    p[res == 6] *= 1e-4
    m = 0.5 * s * rng.standard_normal(n)
    v = s * s * rng.uniform(0.25, 4.0, n)
    m[rng.integers(0, 3, n) == 0] = 0.0
    v[rng.integers(0, 3, n) == 0] = 0.0
    if n > 3:
        m[3], v[3] = 0.5 * s[3], 0.0                   # the m' / eps case is in every case, the single float4 included
    return tuple(np.ascontiguousarray(x, dtype=np.float32) for x in (p, g, m, v))
