"""gt_attn_bwd for T <= 160 (gt_attn_bwd_fused_kernel of csrc/attn_mfma.hip: the whole backward of one (utterance, head) in one
workgroup) through the C-ABI against float64 on its own operands: the guarded harness of tests/test_attn_fp64_gpu.py (q / k / v and
dq / dk / dv as windows of one [R, 3 C] buffer, NaN guards, canaries on every row no store may touch, the workspace prefilled with
0xFF) and attn64.check_case(mfma=True).  B = 3, H = 2, D = 96, lens [T - 7, 1, T] ([min(33, T), 1, T] for T <= 40).

tests/test_attn_fp64_gpu.py reaches T = 3, 33, 129 and 160; the edges of the one-workgroup kernel added here:
  31   partial single tile, scalar P loads (T odd)
  32   exactly one tile, TI = T, 16-byte P loads
  65   the third tile holds one query; seed word on the device
  128  four full tiles, the fifth wave without a tile
  159  five tiles, T & 3 != 0
All five ragged with p = 0.1; 32 and 128 also uniform with p = 0, and 128 with non-zero dout on padded rows.
Tolerances: the derived bounds of oracle/attn64.py and the aggregate limits of oracle/rows64.py; nothing is chosen here."""
import types

import pytest
import torch

from oracle import attn64, dropmask, rows64

pytestmark = pytest.mark.gpu

H, D, WIN, B, GUARD, CANARY = 2, 96, 4, 3, 8, 768.0
SEED, WORD = 0x51ED270B, 0x1234ABCD

# (T, ragged, p, seed word on the device, non-zero dout on padded rows)
CASES = [(T, True, 0.1, T == 65, False) for T in (31, 32, 65, 128, 159)]
CASES += [(32, False, 0.0, False, False), (128, False, 0.0, False, True)]


def dev():
    return torch.device("cuda:0")


def run_case(T, lens, ragged, p, word, dirty):
    """One gt_attn_fwd + gt_attn_bwd call in the guarded harness; returns check_case's (c, got) on the CPU and the raw bf16 workspace
    [2, B, H, T, TI]."""
    from glow_tts_amd import _lib, ops
    L = _lib.lib()
    C = H * D
    assert L.gt_attn_mfma_shape(T, D, WIN) == 1 and T <= 160
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
    return c, got, w16


@pytest.mark.parametrize("T,ragged,p,word,dirty", CASES)
def test_fused_attention_backward_vs_float64(built, T, ragged, p, word, dirty):
    lens = [min(33, T) if T <= 40 else T - 7, 1, T]
    tag = f"attn T={T} D={D} {'ragged' if ragged else 'uniform'} p={p}"
    print(f"{tag}: launch_fwd<5> / gt_attn_bwd_fused_kernel" + (", seed word on the device" if word else "")
          + (", non-zero dout on padded rows" if dirty else ""))
    c, got, w16 = run_case(T, lens, ragged, p, word, dirty)
    w64 = w16.double()
    assert bool(torch.isfinite(w64).all()), "a workspace row j < T keeps its 0xFF prefill"        # every row j < T, all TI columns
    assert bool((w64[..., T:] == 0).all()), "columns i >= T of the padded query axis must be zero"
    got["dS"], got["Pd"] = w64[0, ..., :T].transpose(-1, -2), w64[1, ..., :T].transpose(-1, -2)
    rep = attn64.check_case(tag, c, got, True, 0)
    assert set(rep) == {"P", "out", "dS", "Pd", "dq", "dk", "dv", "dEk", "dEv"}
    if dirty:                                                         # padded queries contribute nothing, whatever dout holds
        for b in range(B):
            assert bool((got["dq"][b, :, lens[b]:c.own[b]] == 0).all())
