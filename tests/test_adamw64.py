"""oracle/adamw64.py (the float64 restatement tests/test_adamw_fp64_gpu.py holds gt_adamw_flat to) pinned to torch.optim.AdamW run in
float64, and its bounds and planted defects tried on a numpy float32 emulation of the kernel's statement order.  No GPU.

"Equal" for two float64 evaluations is 1e-12 of the tensor's largest magnitude.  The emulation must pass the rule on the GPU test's
operand recipe at every (hyper set, t) of its grid, and every planted defect must miss by rows64.CONTROL_MISS wherever
adamw64.required says the GPU test requires it: a bound that fp32 arithmetic on the CPU breaks, or that cannot see the defect, would
prove nothing on the device."""
import numpy as np
import pytest
import torch

from oracle import adamw64 as A
from oracle.rows64 import check, check_with_control

EQ = 1e-12
N = 65536
GRID_TS = (1, 2, 3, 10, 100, 1000, 100000)


def close(a, b, tol=EQ):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and float(np.abs(a - b).max()) <= tol * max(1e-300, float(np.abs(b).max()))


# ----------------------------------------------------------------------------- the restatement is torch.optim.AdamW
@pytest.mark.parametrize("lr,betas,eps,wd", [(2e-4, (.9, .98), 1e-9, .01), (2e-3, (.85, .999), 1e-8, .1)])
@pytest.mark.parametrize("scheduled", [False, True])
def test_restatement_is_torch_adamw_in_float64(lr, betas, eps, wd, scheduled):
    gen = torch.Generator().manual_seed(5)
    n = 257
    q = torch.nn.Parameter(torch.randn(n, generator=gen, dtype=torch.float64))
    opt = torch.optim.AdamW([q], lr=lr, betas=betas, eps=eps, weight_decay=wd, foreach=False)
    p, m, v = q.detach().numpy().copy(), np.zeros(n), np.zeros(n)
    for t in range(1, 6):
        lr_t, b1_t = (lr * (1 + 0.3 * t), betas[0] - 0.01 * t) if scheduled else (lr, betas[0])
        opt.param_groups[0]["lr"], opt.param_groups[0]["betas"] = lr_t, (b1_t, betas[1])
        g = torch.randn(n, generator=gen, dtype=torch.float64) * 10.0 ** float(t - 3)
        q.grad = g.clone()
        opt.step()
        out = A.step(p, g.numpy(), m, v, [lr_t, b1_t, betas[1], eps, wd, t])
        p, m, v = out["p"][0], out["m"][0], out["v"][0]
        st = opt.state[q]
        assert close(p, q.detach().numpy()) and close(m, st["exp_avg"].numpy()) and close(v, st["exp_avg_sq"].numpy()), t


def test_every_defect_is_a_different_rule_and_the_true_rule_is_not():
    p, g, m, v = A.case(1024)
    h = A.hyper32(*A.HYPERS[2], 10)
    ref = A.step(p, g, m, v, h)
    again = A.step(p, g, m, v, h, defect=None)
    assert all(np.array_equal(ref[k][0], again[k][0]) for k in "pmv")
    for d in A.DEFECTS:
        assert not np.array_equal(A.step(p, g, m, v, h, defect=d)["p"][0], ref["p"][0]), d
    with pytest.raises(AssertionError):
        A.step(p, g, m, v, h, defect="no_such_defect")


def test_recipe_holds_the_cases_it_promises():
    p, g, m, v = A.case(N)
    res = np.arange(N) % 8
    assert (g[res == 3] == 0).all() and (p[res == 5] == 0).all() and np.abs(p[res == 6]).max() < 1e-3
    a = np.abs(g[res != 3])
    assert a.min() >= 1e-12 * (1 - 1e-6) and a.max() <= 1e3 and a.min() < 1e-11 and a.max() > 1e2
    for r in range(8):                                           # v = 0, g = 0, m != 0 and every zero pattern, in every lane position
        k = res == r
        assert ((m[k] == 0) & (v[k] != 0)).any() and ((m[k] != 0) & (v[k] == 0)).any() and ((m[k] == 0) & (v[k] == 0)).any()
    assert ((g == 0) & (v == 0) & (m != 0)).sum() > N // 64


# ----------------------------------------------------------------------------- the float32 emulation under the rule
@pytest.mark.parametrize("t", GRID_TS)
@pytest.mark.parametrize("hset", range(len(A.HYPERS)))
def test_float32_emulation_holds_the_bounds_and_sees_the_defects(hset, t):
    p, g, m, v = A.case(N)
    h = A.hyper32(*A.HYPERS[hset], t)
    got = dict(zip("pmv", A.emulate32(p, g, m, v, h)[:3]))
    ref = A.step(p, g, m, v, h)
    bads = {d: A.step(p, g, m, v, h, defect=d) for d in A.DEFECTS}
    name = f"emulation {A.HYPERS[hset]} t={t}"
    need = {d: bads[d]["p"][0] for d in A.DEFECTS if A.required(d, h)}
    r = check_with_control(f"{name} p'", got["p"], *ref["p"], need)
    for d in A.DEFECTS:                                          # the others only logged
        if d not in need:
            print(f"  not required: {d} misses by {check(d, got['p'], bads[d]['p'][0], ref['p'][1]).miss:.3g}x")
    for k in "mv":
        check_with_control(f"{name} {k}'", got[k], *ref[k], {"coupled_decay": bads["coupled_decay"][k][0]})
    if t <= 100:
        print(f"  powf ulps needed: {A.powf_ulps_needed(got['p'], p, g, m, v, h):.3g}")
    assert set(need) >= {"coupled_decay", "eps_under_root"}
    assert (set(A.BIAS_DEFECTS) <= set(need)) == (t <= 100 or (t == 1000 and A.HYPERS[hset][2] == .999))
    assert ("no_decay" in need) == (hset != 1)


# ----------------------------------------------------------------------------- the gradient norm
@pytest.mark.parametrize("n", [4, 1028, A.CAP + 4, 2 * A.CAP + A.CAP // 2 + 12])
def test_gradient_norm_emulation_holds_its_bound_and_sees_a_dropped_float4(n):
    rng = np.random.default_rng(n)
    g = rng.standard_normal(n).astype(np.float32)
    big = np.float32(np.sqrt(0.05 * n / 4))
    g[-4:] = big                                                 # the last float4 carries ~5 % of the sum
    prior = 0.37 * n
    z = np.zeros_like(g)
    got = A.emulate32(z, g, z, z, A.hyper32(*A.HYPERS[0], 1), prior=prior)[3]
    ref, bound = A.gnorm_sq(g, prior)
    bad = A.gnorm_sq(g, prior, drop=range(n - 4, n))[0]
    assert bad[0] < ref[0]
    check_with_control(f"gnorm_sq emulation n={n} (depth {A.gnorm_depth(n)})", np.asarray([got]), ref, bound, bad)
    halves = A.gnorm_sq_launches(g, [(0, n // 8 * 4), (n // 8 * 4, n)], prior)
    assert close(halves[0], ref) and halves[1][0] > 0


def test_launch_geometry_restated():
    assert A.CAP == 1024 * 256 * 4
    assert [A.launch_blocks(n) for n in (0, 4, 1024, 1028, A.CAP - 4, A.CAP, A.CAP + 4, 3 * A.CAP)] == [0, 1, 1, 2, 1024, 1024, 1024, 1024]
    assert A.gnorm_depth(A.CAP) == 4 + 9 + 1024 and A.gnorm_depth(A.CAP + 4) == 8 + 9 + 1024 and A.gnorm_depth(4) == 4 + 9 + 1
