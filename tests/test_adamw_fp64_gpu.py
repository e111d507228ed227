"""gt_adamw_flat (csrc/optim.hip) — the one kernel that writes the model — against float64 on its own fp32 operands, under the rule
of oracle/rows64.py with the restatement, bounds and planted defects of oracle/adamw64.py (tests/test_adamw64.py tries them on a
float32 emulation first).

Every launch goes through _lib.call on guarded buffers (oracle/guards.py): p, g, m, v, hyper and gnorm_sq each sit between canary
margins, g and hyper are compared bit for bit with their copies afterwards.  The operands are adamw64.case: gradients over fifteen
decades, zero gradients, p = 0 and |p| ~ lr (the update is the whole result), zero moments (v = 0, g = 0, m != 0: the update is
m / eps), by index mod 8 so that each lands in every position of a float4.

The sizes come from optim.hip's launch geometry — one float4 per thread, 256 threads per workgroup, at most 1024 workgroups,
grid-stride beyond; CAP = 1024 * 256 * 4 floats is one trip of the grid:
    4                       one float4
    1020, 1024, 1028        one workgroup less a float4, exactly, and the first thread of a second one
    CAP - 4, CAP            the last sizes without a second trip
    CAP + 4                 the first thread that strides
    2 CAP + CAP / 2 + 12    an uneven third trip
The three hyper sets of adamw64.HYPERS at t in {1, 2, 10, 100, 1000, 1e5} run on 1028 and CAP + 4, one set at t = 10 on the rest.
Each check prints one Report line with the miss factor of every required planted defect (>= rows64.CONTROL_MISS)."""
import functools

import numpy as np
import pytest
import torch

from oracle import adamw64 as A
from oracle.guards import Guards
from oracle.rows64 import check, check_with_control

pytestmark = pytest.mark.gpu
CAP = A.CAP
THIRD_TRIP = 2 * CAP + CAP // 2 + 12
SIZES = (4, 1020, 1024, 1028, CAP - 4, CAP, CAP + 4, THIRD_TRIP)
FULL_GRID = (1028, CAP + 4)
CASES = [(n, h, t) for n in FULL_GRID for h in range(len(A.HYPERS)) for t in A.TS] + [(n, 0, 10) for n in SIZES if n not in FULL_GRID]
GT_E_INVAL, GT_E_ALIGN = -1, -3


def dev():
    return torch.device("cuda:0")


def api():
    from glow_tts_amd import _lib
    return _lib.call, _lib.current_stream(dev()), _lib


@functools.lru_cache(maxsize=None)
def operands(n):
    """adamw64.case(n), computed once and never written"""
    return A.case(n)


def same_bits(a, b):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    b = b.detach().cpu().numpy() if isinstance(b, torch.Tensor) else np.asarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def place(G, p, g, m, v, hyper, prior=None):
    """the four operands, hyper and (with a prior) gnorm_sq on the device, each between canaries -> dict of views"""
    d = {k: G.out(k, x.shape, prior=torch.from_numpy(x)) for k, x in zip("pgmv", (p, g, m, v))}
    d["hyper"] = G.out("hyper", (6,), prior=torch.from_numpy(np.asarray(hyper, dtype=np.float32)))
    d["gnorm"] = None if prior is None else G.out("gnorm_sq", (1,), prior=torch.tensor([prior], dtype=torch.float32))
    return d


def launch(d, n, lo=0):
    call, st, _ = api()
    call.gt_adamw_flat(d["p"][lo:], d["g"][lo:], d["m"][lo:], d["v"][lo:], n, d["hyper"], d["gnorm"], st)


def pmv_rule(name, got, p, g, m, v, h, extra_p=None):
    """p', m', v' under the rule, p' against every planted defect adamw64.required names at these hyper-parameters (the others
    computed only where they are cheap to show), m' and v' against the coupled decay (the one defect that reaches them)"""
    ref = A.step(p, g, m, v, h)
    need = {d: A.step(p, g, m, v, h, defect=d) for d in A.DEFECTS if A.required(d, h) or d == "coupled_decay"}
    bads = {d: need[d]["p"][0] for d in need if A.required(d, h)}
    bads.update(extra_p or {})
    out = {"p": check_with_control(f"{name} p'", got["p"], *ref["p"], bads)}
    for k in "mv":
        out[k] = check_with_control(f"{name} {k}'", got[k], *ref[k], {"coupled_decay": need["coupled_decay"][k][0]})
    return out


# ----------------------------------------------------------------------------- the update, every size and hyper set
@pytest.mark.parametrize("n,hset,t", CASES)
def test_update_against_float64(built, n, hset, t):
    p, g, m, v = operands(n)
    h = A.hyper32(*A.HYPERS[hset], t)
    prior = 0.25 + n
    G = Guards(dev())
    d = place(G, p, g, m, v, h, prior)
    launch(d, n)
    G.verify()
    assert same_bits(d["g"], g), "the gradient was written"
    assert same_bits(d["hyper"], h), "hyper was written"
    got = {k: d[k].cpu().numpy() for k in "pmv"}
    name = f"gt_adamw_flat n={n} {A.HYPERS[hset]} t={t}"
    r = pmv_rule(name, got, p, g, m, v, h)
    gr = check(f"{name} gnorm_sq", d["gnorm"].cpu().numpy(), *A.gnorm_sq(g, prior))
    print(gr)
    assert gr.ok, str(gr)
    if t <= 100:                                                 # what DESIGN.md 4.19 records about powf
        e1 = check("E=1", got["p"], *A.step(p, g, m, v, h, E=1.0)["p"])
        print(f"POWF {name}: worst err/bound {r['p'].worst:.3f} (E={A.POWF_ULPS}), {e1.worst:.3f} (E=1); "
              f"powf ulps needed {A.powf_ulps_needed(got['p'], p, g, m, v, h):.3g}")


# ----------------------------------------------------------------------------- the gradient norm
def sentinels(n):
    """{name: indices of one float4}: where a reduction loses elements (each is given >= 2 % of the sum)"""
    blocks = A.launch_blocks(n)
    s = {"last float4": n - 4, "last lane of workgroup 0": min(n, A.WG * A.VEC) - 4, "lane 0 of the last workgroup": (blocks - 1) * A.WG * A.VEC}
    if n > CAP:
        s["first float4 of the second trip"] = CAP
    return {k: tuple(range(i, i + 4)) for k, i in s.items()}


@pytest.mark.parametrize("n", [1028, CAP + 4, THIRD_TRIP])
def test_gradient_norm_counts_every_element_once(built, n):
    p, _, m, v = operands(n)
    g = np.random.default_rng(n).standard_normal(n).astype(np.float32)
    sent = sentinels(n)
    for idx in sent.values():
        g[list(idx)] = np.float32(np.sqrt(0.05 * n / 4))
    total = float((g.astype(np.float64) ** 2).sum())
    assert all(float((g[list(i)].astype(np.float64) ** 2).sum()) >= 0.02 * total for i in sent.values())
    h = A.hyper32(*A.HYPERS[0], 10)
    prior = 0.37 * n
    G = Guards(dev())
    d = place(G, p, g, m, v, h, prior)
    launch(d, n)
    G.verify()
    ref, bound = A.gnorm_sq(g, prior)
    bads = {f"without the {k}": A.gnorm_sq(g, prior, drop=i)[0] for k, i in sent.items()}
    bads["prior overwritten"] = A.gnorm_sq(g, 0.0)[0]
    check_with_control(f"gnorm_sq n={n} one launch on a prior", d["gnorm"].cpu().numpy(), ref, bound, bads)
    whole = {k: d[k].cpu().numpy() for k in "pmv"}

    half = n // 8 * 4                                            # two launches over two halves add up to the whole
    G2 = Guards(dev())
    d2 = place(G2, p, g, m, v, h, prior)
    call, st, _ = api()
    for s, e in ((0, half), (half, n)):
        call.gt_adamw_flat(d2["p"][s:], d2["g"][s:], d2["m"][s:], d2["v"][s:], e - s, d2["hyper"], d2["gnorm"], st)
    G2.verify()
    ref2, bound2 = A.gnorm_sq_launches(g, [(0, half), (half, n)], prior)
    assert abs(ref2[0] - ref[0]) <= 1e-12 * ref[0]
    bads2 = {f"without the {k}": A.gnorm_sq_launches(g, [(0, half), (half, n)], prior, drop=i)[0] for k, i in sent.items()}
    bads2["first half lost"] = A.gnorm_sq(g[half:], prior)[0]
    check_with_control(f"gnorm_sq n={n} two launches", d2["gnorm"].cpu().numpy(), ref2, bound2, bads2)
    assert all(same_bits(d2[k], whole[k]) for k in "pmv"), "two half launches and one whole launch update differently"

    G3 = Guards(dev())                                           # gnorm_sq = NULL: the same update, bit for bit
    d3 = place(G3, p, g, m, v, h, None)
    launch(d3, n)
    G3.verify()
    assert all(same_bits(d3[k], whole[k]) for k in "pmv"), "the update depends on gnorm_sq being given"


# ----------------------------------------------------------------------------- sub-ranges (what FlatAdamW._launch does for every run)
@pytest.mark.parametrize("s,n", [(68, 1028), (4, CAP + 4)])
def test_launch_on_a_sub_range_leaves_the_rest_alone(built, s, n):
    assert s % 4 == 0 and s % 64 != 0
    N = s + n + 100
    p, g, m, v = operands(N)
    g = g.copy()                                                 # the floats next to the range would each add 5 % to the norm
    g[s - 1] = g[s + n] = np.float32(np.sqrt(0.05 * float((g[s:s + n].astype(np.float64) ** 2).sum())))
    h = A.hyper32(*A.HYPERS[2], 10)
    prior = 3.0
    G = Guards(dev())
    d = place(G, p, g, m, v, h, prior)
    assert all(d[k][s:].data_ptr() % 16 == 0 and d[k][s:].data_ptr() % 256 != 0 for k in "pgmv")
    launch(d, n, lo=s)
    G.verify()
    assert same_bits(d["g"], g) and same_bits(d["hyper"], h)
    for k, x in zip("pmv", (p, m, v)):
        assert same_bits(d[k][:s], x[:s]) and same_bits(d[k][s + n:], x[s + n:]), f"{k}: written outside [{s}, {s + n})"
    got = {k: d[k][s:s + n].cpu().numpy() for k in "pmv"}
    name = f"gt_adamw_flat on [{s}, {s + n}) of {N}"
    pmv_rule(name, got, p[s:s + n], g[s:s + n], m[s:s + n], v[s:s + n], h)
    ref, bound = A.gnorm_sq(g[s:s + n], prior)
    bads = {"the float before the range counted": ref + float(g[s - 1]) ** 2, "the float after the range counted": ref + float(g[s + n]) ** 2}
    check_with_control(f"{name} gnorm_sq", d["gnorm"].cpu().numpy(), ref, bound, bads)


# ----------------------------------------------------------------------------- status codes
def test_status_codes_and_nothing_written_when_refused(built):
    call, st, _lib = api()
    n = 1024
    p, g, m, v = operands(n + 4)
    h = A.hyper32(*A.HYPERS[0], 10)
    G = Guards(dev())
    d = place(G, p, g, m, v, h, 5.0)
    start = {k: d[k].clone() for k in ("p", "g", "m", "v", "hyper", "gnorm")}

    def untouched(what):
        G.verify()
        assert all(same_bits(d[k], start[k]) for k in start), f"{what}: something was written"

    def refused(code, what, *args):
        with pytest.raises(_lib.GtError) as e:
            call.gt_adamw_flat(*args, st)
        assert e.value.code == code, (what, e.value.code)
        untouched(what)

    a = [d["p"], d["g"], d["m"], d["v"]]
    call.gt_adamw_flat(*a, 0, d["hyper"], d["gnorm"], st)                      # n = 0 -> GT_OK
    untouched("n = 0")
    refused(GT_E_ALIGN, "n = 6", *a, 6, d["hyper"], d["gnorm"])
    for i, k in enumerate("pgmv"):
        off = list(a)
        off[i] = a[i][1:]
        assert off[i].data_ptr() % 16 == 4
        refused(GT_E_ALIGN, f"{k} + 4 bytes", *off, n, d["hyper"], d["gnorm"])
        null = list(a)
        null[i] = None
        refused(GT_E_INVAL, f"{k} NULL", *null, n, d["hyper"], d["gnorm"])
    refused(GT_E_INVAL, "hyper NULL", *a, n, None, d["gnorm"])


# ----------------------------------------------------------------------------- a captured graph reads hyper from the device
def test_captured_graph_follows_hyper_on_the_device(built):
    """One linear graph: hyper[5:6].add_(1), then the launch.  Three replays with a new lr and beta1 written between them: each must
    be the restatement at THAT replay's lr, beta1 and t, on the operands the replay before left (the kernel's own)."""
    call, _, _lib = api()
    n, t0 = 1028, 7
    p, g, m, v = operands(n)
    lr, b1, b2, eps, wd = A.HYPERS[0]
    G = Guards(dev())
    d = place(G, p, g, m, v, A.hyper32(lr, b1, b2, eps, wd, t0), 0.0)
    scratch = {k: d[k].clone() for k in ("p", "g", "m", "v", "hyper", "gnorm")}
    side, graph = torch.cuda.Stream(), torch.cuda.CUDAGraph()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        scratch["hyper"][5:6].add_(1.0)                                          # one eager run of both nodes, on copies
        call.gt_adamw_flat(scratch["p"], scratch["g"], scratch["m"], scratch["v"], n, scratch["hyper"], scratch["gnorm"], _lib.current_stream(dev()))
        with torch.cuda.graph(graph, stream=side):
            d["hyper"][5:6].add_(1.0)
            call.gt_adamw_flat(d["p"], d["g"], d["m"], d["v"], n, d["hyper"], d["gnorm"], _lib.current_stream(dev()))
    torch.cuda.synchronize()
    G.verify()
    assert all(same_bits(d[k], x) for k, x in zip("pmv", (p, m, v))), "capturing ran the kernel"
    state = {"p": p, "m": m, "v": v}
    schedule = [(lr, b1), (lr * 1.5, b1 - 0.02), (lr * 0.4, b1 + 0.03)]
    gn_ref, gn_bound = np.zeros(1), np.zeros(1)
    for k, (lr_k, b1_k) in enumerate(schedule):
        d["hyper"][:2].copy_(torch.tensor([lr_k, b1_k], dtype=torch.float32))
        graph.replay()
        torch.cuda.synchronize()
        G.verify()
        h = A.hyper32(lr_k, b1_k, b2, eps, wd, t0 + 1 + k)
        assert same_bits(d["hyper"], h) and same_bits(d["g"], g)
        got = {q: d[q].cpu().numpy() for q in "pmv"}
        stale = {}
        if k:                                                                  # the first replay's lr / beta1 / t kept: what a graph with baked-in scalars does
            stale["first replay's lr kept"] = A.step(state["p"], g, state["m"], state["v"], A.hyper32(lr, b1_k, b2, eps, wd, t0 + 1 + k))["p"][0]
            stale["first replay's t kept"] = A.step(state["p"], g, state["m"], state["v"], A.hyper32(lr_k, b1_k, b2, eps, wd, t0 + 1))["p"][0]
        pmv_rule(f"graph replay {k} lr={lr_k:.3g} b1={b1_k:.3g} t={t0 + 1 + k}", got, state["p"], g, state["m"], state["v"], h, extra_p=stale)
        if k:
            bad_m = A.step(state["p"], g, state["m"], state["v"], A.hyper32(lr_k, b1, b2, eps, wd, t0 + 1 + k))["m"]
            check_with_control(f"graph replay {k} m' against beta1 of the first replay", got["m"], *A.step(state["p"], g, state["m"], state["v"], h)["m"], bad_m[0])
        gn_bound = gn_bound + A.gnorm_sq(g)[1] + A.U32 * gn_ref
        gn_ref = gn_ref + A.gnorm_sq(g)[0]
        r = check(f"graph replay {k} gnorm_sq", d["gnorm"].cpu().numpy(), gn_ref, gn_bound)
        assert r.ok, str(r)
        state = got


# ----------------------------------------------------------------------------- FlatAdamW's layout over the kernel
def test_flat_adamw_layout_early_tail_and_skipped_parameter(built):
    """GradBuckets over sizes that are no multiples of its 64-float alignment, one parameter without a gradient in the middle,
    step_early on the tail and step() on the rest: every float of the flat buffers against the restatement — active floats updated
    once, the skipped parameter and its padding bit-identical, padding exactly +0 — and a norm that counts every active element once
    (sentinels on both sides of the early / late seam and of the skipped parameter; its stale gradient slice holds large values)."""
    from glow_tts_amd import ops, train
    shapes, skip, early_from = [(7, 5), (3,), (11, 2, 3), (5,), (63, 33), (130,)], 2, 4
    sizes = [int(np.prod(s)) for s in shapes]
    assert all(k % 64 for k in sizes)
    total = sum(-(-k // 64) * 64 for k in sizes)
    rp, rg, rm, rv = operands(total)
    params = [torch.nn.Parameter(torch.zeros(s, device=dev())) for s in shapes]
    gb = train.GradBuckets(params, world=1)
    assert gb.total == total and all(a is b for a, b in zip(gb.params, params))
    off = gb.offsets
    inside = np.zeros(total, dtype=bool)
    for o, k in zip(off, sizes):
        inside[o:o + k] = True
    with torch.no_grad():
        for q, o, k in zip(params, off, sizes):
            q.copy_(torch.from_numpy(rp[o:o + k]).view_as(q))
    lr, b1, b2, eps, wd = A.HYPERS[2]
    opt = train.FlatAdamW(gb, lr, (b1, b2), eps, wd)
    opt.m.copy_(torch.from_numpy(np.where(inside, rm, 0).astype(np.float32)))
    opt.v.copy_(torch.from_numpy(np.where(inside, rv, 0).astype(np.float32)))
    opt.hyper[5] = 9.0
    g = np.where(inside, np.random.default_rng(7).standard_normal(total), 0).astype(np.float32)
    seam = off[early_from]
    sent = {"last before the skipped parameter": off[skip - 1] + sizes[skip - 1] - 1, "first after the skipped parameter": off[skip + 1],
            "last before the seam": off[early_from - 1] + sizes[early_from - 1] - 1, "first after the seam": seam}
    for i in sent.values():
        g[i] = 12.0
    g[off[skip]:off[skip] + sizes[skip]] = 40.0                                  # stale: this parameter has no gradient in this step
    gb.flat.copy_(torch.from_numpy(g))
    for i, (q, o, k) in enumerate(zip(params, off, sizes)):
        q.grad = None if i == skip else torch.from_numpy(g[o:o + k]).view_as(q).to(dev())
    before = {"p": opt.flat_p.cpu().numpy().copy(), "m": opt.m.cpu().numpy().copy(), "v": opt.v.cpu().numpy().copy()}
    assert same_bits(before["p"], np.where(inside, rp, 0).astype(np.float32))

    ops.arena_begin(dev())
    gb.gather()
    assert gb.active == [i != skip for i in range(len(shapes))] and same_bits(gb.flat, g)
    opt.step_early(seam, total)
    gn = opt.step().clone()
    torch.cuda.synchronize()
    ops.arena_end(dev())

    runs = [(0, off[skip]), (off[skip + 1], total)]
    assert gb.active_runs() == runs
    act = np.zeros(total, dtype=bool)
    for s, e in runs:
        act[s:e] = True
    h = A.hyper32(lr, b1, b2, eps, wd, 10)
    assert same_bits(opt.hyper, h) and same_bits(gb.flat, g)
    got = {"p": opt.flat_p.cpu().numpy(), "m": opt.m.cpu().numpy(), "v": opt.v.cpu().numpy()}
    for k in "pmv":
        assert same_bits(got[k][~act], before[k][~act]), f"{k}: the skipped parameter or its padding was written"
        assert not got[k][~inside].view(np.uint32).any(), f"{k}: padding is not +0"
    a = {k: x[act] for k, x in before.items()}
    once = A.step(a["p"], g[act], a["m"], a["v"], h)
    tail = np.arange(total)[act] >= seam
    twice = A.step(once["p"][0], g[act], once["m"][0], once["v"][0], h)["p"][0]
    pmv_rule("FlatAdamW step_early + step, active floats", {k: x[act] for k, x in got.items()}, a["p"], g[act], a["m"], a["v"], h,
             extra_p={"the early tail updated again by step()": np.where(tail, twice, once["p"][0])})
    for q, o, k in zip(params, off, sizes):                                       # the parameters ARE the flat buffer
        assert same_bits(q.detach().reshape(-1), got["p"][o:o + k])

    launches = [(seam, total), (0, off[skip]), (off[skip + 1], seam)]
    ref, bound = A.gnorm_sq_launches(g, launches)
    assert abs(ref[0] - float((g[act].astype(np.float64) ** 2).sum())) <= 1e-12 * ref[0]
    bads = {f"without the {k}": A.gnorm_sq_launches(g, launches, drop=[i])[0] for k, i in sent.items()}
    bads.update({f"the {k} twice": ref + 144.0 for k in ("last before the seam", "first after the seam")})
    bads["the skipped parameter's stale gradient counted"] = ref + 1600.0 * sizes[skip]
    check_with_control("FlatAdamW gnorm_sq", gn.cpu().numpy().reshape(1), ref, bound, bads)
