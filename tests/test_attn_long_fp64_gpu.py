"""gt_attn_fwd / gt_attn_bwd past 505 tokens (the key-tiled MFMA kernels of csrc/attn_long.hip) through the C-ABI against float64 on
their own operands: the harness of tests/test_attn_fp64_gpu.py (guard rows, NaN-filled P and workspace, canaries on every row no
store may touch, q / k / v and dq / dk / dv as windows of one buffer) and attn64.check_case(mfma=True): the long family rounds as
the MFMA family does (bf16 Ek / Ev, bf16 P', bf16 dS^T / P'^T in the same workspace format).

rescales = ceil(T / 32) + 1: the forward's pass 1 rescales its running denominator once per 32-key tile and once more when the two
lane halves merge (the scheme of gt_attn_fwd_mfma_long_kernel, kept).

Shapes: the smallest that reach each edge, H = 2, D = 96, lens [T - 7, 1, T]:
  506   ragged, p = 0.1   first long shape, T & 3 != 0 (scalar P path), partial last tile, 4 query workgroups; seed word on the device
  512   uniform, p = 0    exact tiles, 16-byte P path; non-zero dout on padded frames
  513   ragged, p = 0.1   one key past a tile; a fifth workgroup that holds one query (three waves that only stage)
  1025  ragged, p = 0.1   B = 2, lens [1018, 1]: twice the first case's key loop plus one key — nothing is sized by T (the LDS of
                          the three kernels is a compile-time constant: DESIGN.md 4.5 quotes the build's resource lines)
  4096  ragged, p = 0     the limit, B = 1, len 4089: head 1 only, the same teacher-forced checks from attn64's pieces under
                          rows64.check, without the planted defects (those are proven at the shapes above)
Tolerances: the derived bounds of oracle/attn64.py and the aggregate limits of oracle/rows64.py; nothing is chosen here."""
import types

import pytest
import torch

from oracle import attn64, dropmask, rows64

pytestmark = pytest.mark.gpu

H, D, WIN, GUARD, CANARY = 2, 96, 4, 8, 768.0
SEED, WORD = 0x51ED270B, 0x1234ABCD

# (T, lens, ragged, p, seed word on the device, non-zero dout on padded rows)
CASES = [(506, [499, 1, 506], True, 0.1, True, False),
         (512, [505, 1, 512], False, 0.0, False, True),
         (513, [506, 1, 513], True, 0.1, False, False),
         (1025, [1018, 1], True, 0.1, False, False)]


def dev():
    return torch.device("cuda:0")


def run_case(T, lens, ragged, p, word, dirty):
    """One gt_attn_fwd + gt_attn_bwd call in the guarded harness; returns check_case's (c, got) on the CPU (dS / Pd as bf16 views)."""
    from glow_tts_amd import _lib, ops
    L = _lib.lib()
    B, C = len(lens), H * D
    assert L.gt_attn_long_shape(T, D, WIN) == 1 and L.gt_attn_mfma_shape(T, D, WIN) == 0
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
    if dirty:                                                         # padded FRAMES only: halo rows stay zero (the rows contract)
        for b in range(B):
            do[rbase[b] + lens[b]:rbase[b] + T] = torch.randn(T - lens[b], C, generator=g)
    do = do.to(torch.bfloat16)

    def guarded(t, fill):
        buf = torch.full((R_ + 2 * GUARD, t.shape[1]), fill, dtype=t.dtype, device=dev())
        buf[GUARD:GUARD + R_] = t.to(dev())
        return buf, buf[GUARD:GUARD + R_]

    nan = float("nan")
    qb, qv = guarded(qkv, nan)
    dob, dov = guarded(do, nan)
    ob, ov = guarded(torch.full((R_, C), CANARY, dtype=torch.bfloat16), CANARY)
    gb, gv = guarded(torch.full((R_, 3 * C), CANARY, dtype=torch.bfloat16), CANARY)
    P = torch.full((B, H, T, T), nan, dtype=torch.float32, device=dev())
    Ekd, Evd = Ek.to(dev()), Ev.to(dev())
    dEk, dEv = prior_dEk.to(dev()), prior_dEv.to(dev())
    wsb = L.gt_attn_bwd_workspace_bytes(B, T, H)
    ws = torch.full((wsb,), 0xFF, dtype=torch.uint8, device=dev())    # bf16 NaN patterns: an unwritten entry is seen
    wd = torch.tensor([WORD], dtype=torch.int32, device=dev()) if word else None
    st, r0 = _lib.current_stream(dev()), _lib.ptr(rc.row0)
    q, k, v = qv[:, :C], qv[:, C:2 * C], qv[:, 2 * C:]
    _lib.check(L.gt_attn_fwd(_lib.ptr(q), _lib.ptr(k), _lib.ptr(v), 3 * C, _lib.ptr(Ekd), _lib.ptr(Evd), _lib.ptr(rc.lengths), _lib.ptr(ov), C,
                             _lib.ptr(P), B, T, rc.Tp, r0, H, D, WIN, p, SEED, _lib.ptr(wd), st), "gt_attn_fwd")
    _lib.check(L.gt_attn_bwd(_lib.ptr(q), _lib.ptr(k), _lib.ptr(v), 3 * C, _lib.ptr(Ekd), _lib.ptr(Evd), _lib.ptr(rc.lengths), _lib.ptr(dov), C,
                             _lib.ptr(P), _lib.ptr(ws), wsb, _lib.ptr(gv[:, :C]), _lib.ptr(gv[:, C:2 * C]), _lib.ptr(gv[:, 2 * C:]), 3 * C,
                             _lib.ptr(dEk), _lib.ptr(dEv), B, T, rc.Tp, r0, H, D, WIN, p, SEED, _lib.ptr(wd), st), "gt_attn_bwd")
    torch.cuda.synchronize()
    ob, gb, P, ws = ob.cpu(), gb.cpu(), P.cpu(), ws.cpu()

    # canaries: guard rows, halos and every row past an utterance's stored rows are untouched
    written = torch.zeros(R_ + 2 * GUARD, dtype=torch.bool)
    for b in range(B):
        written[GUARD + rbase[b]:GUARD + rbase[b] + own[b]] = True
    for buf in (ob, gb):
        assert bool((buf[~written].float() == CANARY).all()), "a store outside the rows the utterances own"
        assert bool(torch.isfinite(buf[written].float()).all())

    c = types.SimpleNamespace(B=B, H=H, T=T, D=D, win=WIN, lens=lens, p=p, own=own, Ek=Ek, Ev=Ev, prior_dEk=prior_dEk, prior_dEv=prior_dEv,
                              seed=dropmask.word_seed(WORD, SEED) if word else SEED)           # the kernel XORs the device word in
    heads = lambda X, b: [attn64.utt_rows(X, rbase[b], n_own[b], T)[:, h * D:(h + 1) * D] for h in range(H)]   # noqa: E731
    c.q, c.k, c.v = ([heads(qkv[:, i * C:(i + 1) * C], b) for b in range(B)] for i in range(3))
    c.dO = [heads(do, b) for b in range(B)]

    def stored(X):
        """[R, C] output rows -> [B, H, T, D] float64, rows >= own[b] zero (not looked at)"""
        out = torch.zeros(B, H, T, D, dtype=torch.float64)
        for b in range(B):
            rows = rows64.t64(X[GUARD + rbase[b]:GUARD + rbase[b] + own[b]])
            for h in range(H):
                out[b, h, :own[b]] = rows[:, h * D:(h + 1) * D]
        return out

    got = {"P": P, "out": stored(ob), "dq": stored(gb[:, :C]), "dk": stored(gb[:, C:2 * C]), "dv": stored(gb[:, 2 * C:]),
           "dEk": dEk.cpu(), "dEv": dEv.cpu()}
    TI = -(-T // 32) * 32                                             # bf16 dS^T [B,H,T(j),TI(i)], then P'^T in the same shape
    n = B * H * T * TI
    w16 = ws[:4 * n].view(torch.bfloat16).view(2, B, H, T, TI)
    assert bool((w16[..., T:] == 0).all()), "columns i >= T of the padded query axis must be zero"
    got["dS"], got["Pd"] = w16[0, ..., :T].transpose(-1, -2), w16[1, ..., :T].transpose(-1, -2)
    return c, got


@pytest.mark.parametrize("T,lens,ragged,p,word,dirty", CASES)
def test_long_attention_vs_float64(built, T, lens, ragged, p, word, dirty):
    tag = f"attn T={T} D={D} {'ragged' if ragged else 'uniform'} p={p}"
    print(f"{tag}: gt_attn_long_fwd_kernel / gt_attn_long_bwd_q_kernel + gt_attn_long_bwd_kv_kernel"
          + (", seed word on the device" if word else "") + (", non-zero dout on padded rows" if dirty else ""))
    c, got = run_case(T, lens, ragged, p, word, dirty)
    got["dS"], got["Pd"] = got["dS"].double(), got["Pd"].double()
    rep = attn64.check_case(tag, c, got, True, -(-T // 32) + 1)
    assert set(rep) == {"P", "out", "dS", "Pd", "dq", "dk", "dv", "dEk", "dEv"}
    if dirty:                                                         # padded queries contribute nothing, whatever dout holds
        for b in range(c.B):
            assert bool((got["dq"][b, :, lens[b]:c.own[b]] == 0).all())


def check_head(c, got, b, h):
    """The teacher-forced checks of check_case for ONE (utterance, head), from attn64's pieces under rows64.check, without the planted
    defects and without dEk / dEv (sums over every head).  Returns the reports."""
    T, n, own = c.T, int(c.lens[b]), int(c.own[b])
    K = attn64.terms(True, T, D, WIN, c.B, H)
    Ek, Ev = attn64.operands(c.Ek, True), attn64.operands(c.Ev, True)
    q, k, v, dO = c.q[b][h], c.k[b][h], c.v[b][h], c.dO[b][h]
    keep = attn64.keep_mask(c.seed, b, h, H, T, c.p)
    sc = dropmask.scale(c.p) if c.p else 1.0
    reps = []

    def chk(name, g, ref, bound, kind, rows=None):
        sel = (lambda x: x) if rows is None else (lambda x: x[:rows])
        r = rows64.check(f"attn T={T} utterance {b} head {h} {name}", sel(rows64.t64(g)), sel(ref), sel(bound), kind)
        print(r)
        reps.append(r)

    # 1. P from the kernel's q, k, Ek
    s, S = attn64.scores(q, k, Ek, n, T, WIN)
    Pr, Pb = attn64.softmax_rows(s, rows64.gamma(K["scores"]) * S, -(-T // 32) + 1)
    Pk = got["P"][b, h]
    chk("P", Pk, Pr, Pb, "f32")
    del s, S, Pr, Pb
    # 2. out from the kernel's own P
    Pd = attn64.drop(Pk, keep, sc, "bf16")
    O, SO = attn64.out(Pd, v, Ev, WIN)
    chk("out", got["out"][b, h], O, rows64.gamma(K["out"]) * SO, "bf16", own)
    # 3. the workspace from the kernel's P, v, Ev, dO
    dSr, dSb = attn64.ds(Pk, dO, v, Ev, keep, sc, n, K["dpd"], WIN)
    dSw, Pdw = rows64.t64(got["dS"][b, h]), rows64.t64(got["Pd"][b, h])
    chk("dS", dSw, dSr, dSb, "bf16")
    del dSr, dSb
    Pdb = attn64.pd_bwd(Pd, n)
    chk("Pd", Pdw, Pdb, torch.zeros_like(Pdb), "bf16")
    del Pd, Pdb
    # 4. dq, dk, dv from the workspace's own values
    r_, s_ = attn64.dq(dSw, k, Ek, WIN)
    chk("dq", got["dq"][b, h], r_, rows64.gamma(K["dq"]) * s_, "bf16", own)
    r_, s_ = attn64.dk(dSw, q)
    chk("dk", got["dk"][b, h], r_, rows64.gamma(K["dk"]) * s_, "bf16", own)
    r_, s_ = attn64.dv(Pdw, dO)
    chk("dv", got["dv"][b, h], r_, rows64.gamma(K["dv"]) * s_, "bf16", own)
    return reps


def test_long_attention_at_the_token_limit(built):
    T, n, b, h = 4096, 4089, 0, 1
    c, got = run_case(T, [n], True, 0.0, False, False)
    assert bool(torch.isfinite(got["P"]).all())                       # both heads written, every entry
    reps = check_head(c, got, b, h)
    assert len(reps) == 7 and all(r.ok for r in reps), [str(r) for r in reps if not r.ok]
    assert bool((got["dq"][b, :, n:c.own[b]] == 0).all())
    assert bool(torch.isfinite(got["dEk"]).all()) and bool(torch.isfinite(got["dEv"]).all())
