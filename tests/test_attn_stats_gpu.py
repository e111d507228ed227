"""gt_attn_fwd_stats / gt_attn_bwd_stats (the P-free pair of csrc/attn_long.hip) through the C-ABI, beside gt_attn_fwd / gt_attn_bwd on
the SAME operands, in the guarded harness of tests/test_attn_long_fp64_gpu.py (its constants, cases and layout: guard rows, NaN-filled
P / stats / workspaces, canaries on every row no store may touch, q / k / v and dq / dk / dv as windows of one buffer).

What is demanded
  forward   `out` buffers equal bit for bit, canaries included; stats finite for every i < T; rden == max_j P[i, :] bit for bit
            against the saved-P forward's P (at the arg-max exp(0) = 1: an identity); |mx - max_j s64| <= gamma(K["scores"]) max_j S.
  dq        torch.equal to gt_attn_bwd's (same P bits, same Dsum, same bf16 dS operand, same MFMA chain).
  dk dv dEk dEv   the key side recomputes the scores in the other operand orientation, so no bit equality.  X64 = the tensor end to end
            in float64 from the kernels' bf16 operands, bf16 Ek / Ev and the true keep mask, no intermediate rounding.  With
            err(X) = |X - X64|_2 / |X64|_2 over the owned rows:   err(new) <= 1.5 err(saved-P)  and  max|new - X64| <= 2 max|saved-P - X64|.
            Both paths round the same quantities at the same places (bf16 P', bf16 dS, bf16 outputs) and differ in fp32 summation
            order only: the expected ratio is 1.0; 1.5 and 2 leave room for another rounding realisation.  The reference is the
            saved-P path measured in the same test.
  controls  planted defects that cannot fault: the stats backward with drop_seed + 1 (p = 0.1), and with rden * (1 + 2^-6) in a copy
            of stats (p = 0): the dk / dv check above must fail for both.
  padded    dirty dout on padded frames (case 512): dq there is 0, and the checks hold against the reference from clean dout.
  the limit T = 4096, B = 1, len 4089: forward, dq, dk, dv on head 1 (dEk / dEv sum over both heads: only finite there).

Measured on an MI355X (the worst over 506, 512, 513, 1025 and, for dk / dv, 4096; err ratio, max-error ratio):
  dk 1.0000, 1.0000    dv 1.0000, 1.0000    dEk 1.0001, 1.0001    dEv 1.0000, 1.0000    (err itself: dk, dv 2.0e-3 .. 2.4e-3 on both paths)
  mx within 0.005 of its bound.  Controls: drop_seed + 1 misses by 126x (dk err ratio 189, dv 242), rden (1 + 2^-6) by 14.2x (the
  weakest: dk max-error ratio 28.3 against 2; its err ratios are 6.9 and 7.9 against 1.5).
"""
import functools
import types

import pytest
import torch

from oracle import attn64, dropmask, rows64
from test_attn_long_fp64_gpu import CANARY, CASES, D, GUARD, H, SEED, WIN, WORD, dev

pytestmark = pytest.mark.gpu

ERR_RATIO, MAX_RATIO = 1.5, 2.0


class Pair:
    """Both pairs run once on one set of operands; the device tensors the controls need stay alive."""


@functools.lru_cache(maxsize=None)
def run_pair(T, lens, ragged, p, word, dirty):
    from glow_tts_amd import _lib, ops
    L = _lib.lib()
    lens = list(lens)
    B, C = len(lens), H * D
    assert L.gt_attn_long_shape(T, D, WIN) == 1
    lens_t = torch.tensor(lens, dtype=torch.int32, device=dev())
    rc = ops.RowsCtx(lens_t, T, lengths_host=lens, round_to=128) if ragged else ops.RowsCtx(lens_t, T)
    R_ = rc.R
    g = torch.Generator().manual_seed(7 * T + D + int(ragged))
    m = rc.rowmask[:, None].cpu()
    qkv = ((torch.randn(R_, 3 * C, generator=g) * 0.5) * m).to(torch.bfloat16)
    do = torch.randn(R_, C, generator=g) * m
    Ek, Ev = torch.randn(2 * WIN + 1, D, generator=g) * 0.1, torch.randn(2 * WIN + 1, D, generator=g) * 0.1
    prior_dEk, prior_dEv = torch.randn(2 * WIN + 1, D, generator=g), torch.randn(2 * WIN + 1, D, generator=g)
    if ragged:
        row0 = rc.row0.cpu().tolist()
        rbase, n_own = [row0[b] + ops.HALO for b in range(B)], [row0[b + 1] - row0[b] for b in range(B)]
    else:
        rbase, n_own = [b * rc.Tp + ops.HALO for b in range(B)], [rc.Tp] * B
    own = [min(T, n_own[b] - ops.HALO) for b in range(B)]
    do_clean = do.to(torch.bfloat16)
    if dirty:                                                         # padded FRAMES only: halo rows stay zero (the rows contract)
        for b in range(B):
            do[rbase[b] + lens[b]:rbase[b] + T] = torch.randn(T - lens[b], C, generator=g)
    do = do.to(torch.bfloat16)

    def guarded(t, fill):
        buf = torch.full((R_ + 2 * GUARD, t.shape[1]), fill, dtype=t.dtype, device=dev())
        buf[GUARD:GUARD + R_] = t.to(dev())
        return buf, buf[GUARD:GUARD + R_]

    nan = float("nan")
    x = Pair()
    x.L, x.rc, x.B, x.T, x.C, x.p, x.lens = L, rc, B, T, C, p, lens
    x.qb, x.qv = guarded(qkv, nan)
    x.dob, x.dov = guarded(do, nan)
    x.Ekd, x.Evd = Ek.to(dev()), Ev.to(dev())
    x.wd = torch.tensor([WORD], dtype=torch.int32, device=dev()) if word else None
    x.prior_dEk, x.prior_dEv = prior_dEk, prior_dEv
    x.written = torch.zeros(R_ + 2 * GUARD, dtype=torch.bool)
    for b in range(B):
        x.written[GUARD + rbase[b]:GUARD + rbase[b] + own[b]] = True
    st, r0 = _lib.current_stream(dev()), _lib.ptr(rc.row0)
    q, k, v = x.qv[:, :C], x.qv[:, C:2 * C], x.qv[:, 2 * C:]
    fixed = (_lib.ptr(q), _lib.ptr(k), _lib.ptr(v), 3 * C, _lib.ptr(x.Ekd), _lib.ptr(x.Evd), _lib.ptr(rc.lengths))
    tail = lambda seed: (B, T, rc.Tp, r0, H, D, WIN, p, seed, _lib.ptr(x.wd), st)     # noqa: E731

    def out_buffers():
        ob, ov = guarded(torch.full((R_, C), CANARY, dtype=torch.bfloat16), CANARY)
        return ob, ov

    def grad_buffers():
        gb, gv = guarded(torch.full((R_, 3 * C), CANARY, dtype=torch.bfloat16), CANARY)
        return gb, gv, prior_dEk.to(dev()), prior_dEv.to(dev())

    # ---- the saved-P pair
    P = torch.full((B, H, T, T), nan, dtype=torch.float32, device=dev())
    ob0, ov0 = out_buffers()
    gb0, gv0, dEk0, dEv0 = grad_buffers()
    wsb0 = L.gt_attn_bwd_workspace_bytes(B, T, H)
    ws0 = torch.full((wsb0,), 0xFF, dtype=torch.uint8, device=dev())
    _lib.check(L.gt_attn_fwd(*fixed, _lib.ptr(ov0), C, _lib.ptr(P), *tail(SEED)), "gt_attn_fwd")
    _lib.check(L.gt_attn_bwd(*fixed, _lib.ptr(x.dov), C, _lib.ptr(P), _lib.ptr(ws0), wsb0, _lib.ptr(gv0[:, :C]), _lib.ptr(gv0[:, C:2 * C]),
                             _lib.ptr(gv0[:, 2 * C:]), 3 * C, _lib.ptr(dEk0), _lib.ptr(dEv0), *tail(SEED)), "gt_attn_bwd")
    torch.cuda.synchronize()
    del ws0
    # ---- the stats pair
    assert L.gt_attn_stats_bytes(B, T, H) == 8 * B * H * T
    x.stats = torch.full((B, H, T, 2), nan, dtype=torch.float32, device=dev())
    ob1, ov1 = out_buffers()
    _lib.check(L.gt_attn_fwd_stats(*fixed, _lib.ptr(ov1), C, _lib.ptr(x.stats), *tail(SEED)), "gt_attn_fwd_stats")
    x.wsb = L.gt_attn_bwd_stats_workspace_bytes(B, T, H)

    def stats_bwd(seed=SEED, stats=None):
        """One gt_attn_bwd_stats call into fresh canary buffers and a NaN-filled workspace -> (buffer, dEk, dEv) on the CPU"""
        gb, gv, dEk, dEv = grad_buffers()
        ws = torch.full((x.wsb // 4,), nan, dtype=torch.float32, device=dev())
        s_ = x.stats if stats is None else stats
        _lib.check(L.gt_attn_bwd_stats(*fixed, _lib.ptr(x.dov), C, _lib.ptr(s_), _lib.ptr(ws), x.wsb, _lib.ptr(gv[:, :C]),
                                       _lib.ptr(gv[:, C:2 * C]), _lib.ptr(gv[:, 2 * C:]), 3 * C, _lib.ptr(dEk), _lib.ptr(dEv), *tail(seed)),
                   "gt_attn_bwd_stats")
        torch.cuda.synchronize()
        x.ws_last = ws.cpu()
        return gb.cpu(), dEk.cpu(), dEv.cpu()

    x.stats_bwd = stats_bwd
    gb1, dEk1, dEv1 = stats_bwd()

    c = types.SimpleNamespace(B=B, H=H, T=T, D=D, win=WIN, lens=lens, p=p, own=own, Ek=Ek, Ev=Ev,
                              seed=dropmask.word_seed(WORD, SEED) if word else SEED)
    heads = lambda X, b: [attn64.utt_rows(X, rbase[b], n_own[b], T)[:, h * D:(h + 1) * D] for h in range(H)]   # noqa: E731
    c.q, c.k, c.v = ([heads(qkv[:, i * C:(i + 1) * C], b) for b in range(B)] for i in range(3))
    c.dO = [heads(do_clean, b) for b in range(B)]                     # the reference sees CLEAN dout
    x.c = c

    def stored(X):
        """[R, C] output rows -> [B, H, T, D] float64, rows >= own[b] zero (not looked at)"""
        out = torch.zeros(B, H, T, D, dtype=torch.float64)
        for b in range(B):
            rows = rows64.t64(X[GUARD + rbase[b]:GUARD + rbase[b] + own[b]])
            for h in range(H):
                out[b, h, :own[b]] = rows[:, h * D:(h + 1) * D]
        return out

    def grads_of(gb, dEk, dEv):
        return {"buf": gb, "dq": stored(gb[:, :C]), "dk": stored(gb[:, C:2 * C]), "dv": stored(gb[:, 2 * C:]), "dEk": dEk.double(), "dEv": dEv.double()}

    x.grads_of = grads_of
    x.P, x.ob0, x.ob1 = P.cpu(), ob0.cpu(), ob1.cpu()
    x.saved = grads_of(gb0.cpu(), dEk0.cpu(), dEv0.cpu())
    x.new = grads_of(gb1, dEk1, dEv1)
    x.stats_cpu = x.stats.cpu()
    return x


@functools.lru_cache(maxsize=None)
def ref64(key, heads=None):
    """dk, dv [B, H, T, D] and dEk, dEv [9, D] end to end in float64 from the kernels' bf16 operands, bf16 Ek / Ev and the true keep
    mask, no intermediate rounding.  heads: only these heads (dEk / dEv are then None: they sum over all of them)."""
    x = run_pair(*key)
    c = x.c
    T = c.T
    K = attn64.terms(True, T, D, WIN, c.B, H)
    Ek, Ev = attn64.operands(c.Ek, True), attn64.operands(c.Ev, True)
    sc = dropmask.scale(c.p) if c.p else 1.0
    dk, dv = torch.zeros(c.B, H, T, D, dtype=torch.float64), torch.zeros(c.B, H, T, D, dtype=torch.float64)
    pk, pv = [], []
    for b in range(c.B):
        n = int(c.lens[b])
        for h in (range(H) if heads is None else heads):
            q, k, v, dO = c.q[b][h], c.k[b][h], c.v[b][h], c.dO[b][h]
            keep = attn64.keep_mask(c.seed, b, h, H, T, c.p)
            s, _ = attn64.scores(q, k, Ek, n, T, WIN)
            P = torch.softmax(s, 1)
            del s
            dS, _ = attn64.ds(P, dO, v, Ev, keep, sc, n, K["dpd"], WIN)
            Pdb = attn64.pd_bwd(attn64.drop(P, keep, sc, "f64"), n)
            del P
            dk[b, h], dv[b, h] = attn64.dk(dS, q)[0], attn64.dv(Pdb, dO)[0]
            pk.append(attn64.band_grad(dS, q, WIN))
            pv.append(attn64.band_grad(Pdb, dO, WIN))
            del dS, Pdb
    if heads is not None:
        return {"dk": dk, "dv": dv, "dEk": None, "dEv": None}
    return {"dk": dk, "dv": dv, "dEk": attn64.accumulate(pk, x.prior_dEk, 1)[0], "dEv": attn64.accumulate(pv, x.prior_dEv, 1)[0]}


def owned(x, X, heads=None):
    """the owned rows of a [B, H, T, D] tensor as one vector"""
    hs = range(H) if heads is None else heads
    return torch.cat([X[b, h, :x.c.own[b]].reshape(-1) for b in range(x.B) for h in hs])


def ratios(x, name, new, saved, ref, heads=None):
    """(err(new) / err(saved), max|new - X64| / max|saved - X64|) of one tensor"""
    sel = (lambda X: owned(x, X, heads)) if name in ("dk", "dv") else (lambda X: X.reshape(-1))
    n_, s_, r_ = sel(new), sel(saved), sel(ref)
    e_new, e_old = float((n_ - r_).norm() / r_.norm()), float((s_ - r_).norm() / r_.norm())
    m_new, m_old = float((n_ - r_).abs().max()), float((s_ - r_).abs().max())
    assert e_old > 0 and m_old > 0, "the saved-P path cannot be exact in bf16"
    return e_new / e_old, m_new / m_old, e_new, e_old


def check4(x, names, new, ref, tag, heads=None, log=print):
    """{name: factor by which the tensor exceeds its limits (<= 1: the check holds)}"""
    out = {}
    for nm in names:
        re_, rm_, e_new, e_old = ratios(x, nm, new[nm], x.saved[nm], ref[nm], heads)
        out[nm] = max(re_ / ERR_RATIO, rm_ / MAX_RATIO)
        log(f"{tag} {nm}: err new {e_new:.3e} saved-P {e_old:.3e} ratio {re_:.4f} (<= {ERR_RATIO}); max-error ratio {rm_:.4f} (<= {MAX_RATIO})")
    return out


def check_forward(x, heads=None):
    c = x.c
    assert torch.equal(x.ob0, x.ob1), "out differs from gt_attn_fwd's (or a canary moved)"
    assert bool(torch.isfinite(x.stats_cpu).all()), "a stats entry of a query row i < T was not written"
    assert torch.equal(x.stats_cpu[..., 1], x.P.max(dim=-1).values), "rden != max_j P[i, j]"
    K = attn64.terms(True, c.T, D, WIN, c.B, H)
    Ek = attn64.operands(c.Ek, True)
    worst = 0.0
    for b in range(c.B):
        for h in (range(H) if heads is None else heads):
            s, S = attn64.scores(c.q[b][h], c.k[b][h], Ek, int(c.lens[b]), c.T, WIN)
            bound = rows64.gamma(K["scores"]) * S.max(1).values
            err = (x.stats_cpu[b, h, :, 0].double() - s.max(1).values).abs()
            worst = max(worst, float((err / bound.clamp(min=1e-300)).max()) if bool((bound > 0).any()) else 0.0)
            assert bool((err <= bound).all()), f"mx of utterance {b} head {h}: {float((err - bound).max()):.3e} past the bound"
    print(f"attn-stats T={c.T}: mx within {worst:.3f} of its bound")


def check_canaries(x, gb):
    assert bool((gb[~x.written].float() == CANARY).all()), "a store outside the rows the utterances own"
    assert bool(torch.isfinite(gb[x.written].float()).all())


@pytest.mark.parametrize("T,lens,ragged,p,word,dirty", CASES)
def test_stats_pair_beside_the_saved_p_pair(built, T, lens, ragged, p, word, dirty):
    key = (T, tuple(lens), ragged, p, word, dirty)
    x = run_pair(*key)
    tag = f"attn-stats T={T} {'ragged' if ragged else 'uniform'} p={p}"
    check_forward(x)                                                                  # 1
    check_canaries(x, x.new["buf"])                                                   # 2
    assert bool(torch.isfinite(x.ws_last).all()), "a workspace record of a query row i < T was not written"
    assert torch.equal(x.new["buf"][:, :x.C], x.saved["buf"][:, :x.C]), "dq differs from gt_attn_bwd's"   # 3
    f = check4(x, ("dk", "dv", "dEk", "dEv"), x.new, ref64(key), tag)                 # 4 (6: the reference saw clean dout)
    assert all(v <= 1.0 for v in f.values()), f
    if dirty:                                                                          # 6
        for b in range(x.B):
            assert bool((x.new["dq"][b, :, lens[b]:x.c.own[b]] == 0).all())


@pytest.mark.parametrize("case,defect", [(0, "seed"), (1, "rden")])
def test_planted_defects_miss(built, case, defect):
    T, lens, ragged, p, word, dirty = CASES[case]
    key = (T, tuple(lens), ragged, p, word, dirty)
    x = run_pair(*key)
    if defect == "seed":
        assert p > 0
        gb, dEk, dEv = x.stats_bwd(seed=SEED + 1)
    else:
        assert p == 0
        bad = x.stats.clone()
        bad[..., 1] *= 1.0 + 2.0 ** -6
        gb, dEk, dEv = x.stats_bwd(stats=bad)
    check_canaries(x, gb)                                                              # a defect, not a fault
    f = check4(x, ("dk", "dv"), x.grads_of(gb, dEk, dEv), ref64(key), f"attn-stats T={T} CONTROL {defect}")
    print(f"attn-stats T={T} CONTROL {defect}: misses by {min(f.values()):.2f}x")
    assert all(v > 1.0 for v in f.values()), f


def test_stats_pair_at_the_token_limit(built):
    T, n, h = 4096, 4089, 1
    key = (T, (n,), True, 0.0, False, False)
    x = run_pair(*key)
    assert bool(torch.isfinite(x.P).all())
    check_forward(x, heads=(h,))
    check_canaries(x, x.new["buf"])                                                   # both heads' outputs finite
    check_canaries(x, x.ob1)
    assert torch.equal(x.new["buf"][:, :x.C], x.saved["buf"][:, :x.C]), "dq differs from gt_attn_bwd's"
    f = check4(x, ("dk", "dv"), x.new, ref64(key, heads=(h,)), f"attn-stats T={T} head {h}", heads=(h,))
    assert all(v <= 1.0 for v in f.values()), f
    assert bool((x.new["dq"][0, :, n:x.c.own[0]] == 0).all())
    assert bool(torch.isfinite(x.new["dEk"]).all()) and bool(torch.isfinite(x.new["dEv"]).all())
    run_pair.cache_clear()                                                             # 134 MB of P and the operands
    ref64.cache_clear()
