"""gt_attn_fwd / gt_attn_bwd through the C-ABI against float64 on their own operands, under the rule of oracle/rows64.py with the
restatement and the derived bounds of oracle/attn64.py.  One forward and one backward call per case; the checks are teacher-forced
(P from the kernel's q, k, Ek; out from the kernel's P; the workspace from the kernel's P, v, Ev, dO; dq, dk, dv, dEk, dEv from the
workspace's own values), every one with its planted defects.

T per code path and per edge (csrc/attn_mfma.hip's dispatchers; the smallest values that reach each one):
  launch_fwd<5>, launch_bwd<5,4> all tiles      3;  33 (second key tile, scalar P stores);  129 (second 128-query workgroup);  160 (T & 3 == 0:
                                                float4 P stores and loads)
  launch_fwd<8>, launch_bwd<8,2> one tile       161;  256
  launch_fwd_long<12>, launch_bwd<12,4> V in L2 257;  375 (scalar);  384 (vector)
  generic (csrc/encoder_ops.hip)                385;  T = 40 with D = 64 (generic by head size)
Lengths [T - 7, 1, T] ([min(33, T), 1, T] for T <= 40): a tile-crossing utterance, a length-1 one, the last one full length.  q, k, v
are windows of one [R, 3 C] buffer, dq, dk, dv of one gradient buffer, the outputs lie between guard rows, and every row no store may
touch (guards, halos, rows past an utterance's own) holds a canary.

One more case hands an MFMA shape (T = 33, D = 96) to the generic kernels by layout: the q, k, v buffer's row pitch is 3 C + 2 elements
(ld & 7 != 0, rows still 4-byte aligned), which the MFMA kernels do not take.  Both directions then run the generic kernels: the
workspace holds the fp32 dS and the case is checked under the generic rule."""
import types

import pytest
import torch

from oracle import attn64, dropmask, rows64

pytestmark = pytest.mark.gpu

H, WIN, B, GUARD, CANARY = 2, 4, 3, 8, 768.0
SEED, WORD = 0x51ED270B, 0x1234ABCD

# (T, D, ragged, p, seed word on the device, non-zero dout on padded rows)
CASES = [(T, 96, True, 0.1, T == 129, False) for T in (3, 33, 129, 160, 161, 256, 257, 375, 384, 385)]
CASES += [(40, 64, True, 0.1, False, False)]
CASES += [(T, 96, False, 0.0, False, T in (33, 385)) for T in (33, 160, 256, 384, 385)]


def dev():
    return torch.device("cuda:0")


GENERIC = "generic gt_attn_fwd_kernel / gt_attn_bwd_q_kernel + gt_attn_bwd_kv_kernel"


def _variant(T, D):
    if D != 96 or T > 384:
        return 0, GENERIC
    if T <= 160:
        return 1, "launch_fwd<5> / launch_bwd<5,4> (all tiles)"
    if T <= 256:
        return 1, "launch_fwd<8> / launch_bwd<8,2> (one tile)"
    return 1, "launch_fwd_long<12> / launch_bwd<12,4> (one tile, V from L2)"


@pytest.mark.parametrize("T,D,ragged,p,word,dirty", CASES)
def test_attention_vs_float64(built, T, D, ragged, p, word, dirty):
    _run_case(T, D, ragged, p, word, dirty)


def test_attention_unaligned_pitch_vs_float64(built):
    """An MFMA shape whose row pitch the MFMA kernels refuse: the generic kernels run it, forward and backward."""
    _run_case(33, 96, True, 0.1, False, False, pad=2)


def _run_case(T, D, ragged, p, word, dirty, pad=0):
    """pad: extra elements in the row pitch of the q, k, v buffer; pad & 7 != 0 takes an MFMA shape to the generic kernels"""
    from glow_tts_amd import _lib, ops
    L = _lib.lib()
    C = H * D
    lens = [min(33, T) if T <= 40 else T - 7, 1, T]
    mfma, variant = _variant(T, D)
    assert L.gt_attn_mfma_shape(T, D, WIN) == mfma
    tag = f"attn T={T} D={D} {'ragged' if ragged else 'uniform'} p={p}"
    if pad:
        assert mfma == 1 and (3 * C + pad) & 7 and not (3 * C + pad) & 1      # an MFMA shape, a pitch it refuses, rows 4-byte aligned
        mfma, variant, tag = 0, GENERIC + f" by layout (row pitch 3 C + {pad})", tag + f" pitch 3C+{pad}"
    print(f"{tag}: {variant}" + (", seed word on the device" if word else "") + (", non-zero dout on padded rows" if dirty else ""))
    lens_t = torch.tensor(lens, dtype=torch.int32, device=dev())
    rc = ops.RowsCtx(lens_t, T, lengths_host=lens, round_to=128) if ragged else ops.RowsCtx(lens_t, T)
    R_ = rc.R
    g = torch.Generator().manual_seed(7 * T + D + int(ragged))
    m = rc.rowmask[:, None].cpu()
    qkv = ((torch.randn(R_, 3 * C, generator=g) * 0.5) * m).to(torch.bfloat16)
    do = torch.randn(R_, C, generator=g) * m
    Ek, Ev = torch.randn(2 * WIN + 1, D, generator=g) * 0.1, torch.randn(2 * WIN + 1, D, generator=g) * 0.1
    prior_dEk, prior_dEv = torch.randn(2 * WIN + 1, D, generator=g), torch.randn(2 * WIN + 1, D, generator=g)
    # geometry of every utterance: first frame row, rows it owns, rows 0 .. own - 1 behind rbase are stored
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

    def guarded(t, fill, pad=0):
        buf = torch.full((R_ + 2 * GUARD, t.shape[1] + pad), fill, dtype=t.dtype, device=dev())
        buf[GUARD:GUARD + R_, :t.shape[1]] = t.to(dev())
        return buf, buf[GUARD:GUARD + R_, :t.shape[1]]

    nan = float("nan")
    qb, qv = guarded(qkv, nan, pad)
    dob, dov = guarded(do, nan)
    ob, ov = guarded(torch.full((R_, C), CANARY, dtype=torch.bfloat16), CANARY)
    gb, gv = guarded(torch.full((R_, 3 * C), CANARY, dtype=torch.bfloat16), CANARY)
    P = torch.full((B, H, T, T), nan, dtype=torch.float32, device=dev())
    Ekd, Evd = Ek.to(dev()), Ev.to(dev())
    dEk, dEv = prior_dEk.to(dev()), prior_dEv.to(dev())
    wsb = L.gt_attn_bwd_workspace_bytes(B, T, H)
    ws = torch.full((wsb,), 0xFF, dtype=torch.uint8, device=dev())    # bf16 / fp32 NaN patterns: an unwritten entry is seen
    wd = torch.tensor([WORD], dtype=torch.int32, device=dev()) if word else None
    st, r0 = _lib.current_stream(dev()), _lib.ptr(rc.row0)
    q, k, v = qv[:, :C], qv[:, C:2 * C], qv[:, 2 * C:]
    _lib.check(L.gt_attn_fwd(_lib.ptr(q), _lib.ptr(k), _lib.ptr(v), 3 * C + pad, _lib.ptr(Ekd), _lib.ptr(Evd), _lib.ptr(rc.lengths), _lib.ptr(ov), C,
                             _lib.ptr(P), B, T, rc.Tp, r0, H, D, WIN, p, SEED, _lib.ptr(wd), st), "gt_attn_fwd")
    _lib.check(L.gt_attn_bwd(_lib.ptr(q), _lib.ptr(k), _lib.ptr(v), 3 * C + pad, _lib.ptr(Ekd), _lib.ptr(Evd), _lib.ptr(rc.lengths), _lib.ptr(dov), C,
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
           "dEk": dEk.cpu(), "dEv": dEv.cpu(), "Pd": None}
    if mfma:                                                          # bf16 dS^T [B,H,T(j),TI(i)], then P'^T in the same shape
        TI = -(-T // 32) * 32
        n = B * H * T * TI
        w16 = ws[:4 * n].view(torch.bfloat16).view(2, B, H, T, TI).double()
        assert bool((w16[..., T:] == 0).all()), "columns i >= T of the padded query axis must be zero"
        got["dS"], got["Pd"] = w16[0, ..., :T].transpose(-1, -2), w16[1, ..., :T].transpose(-1, -2)
    else:                                                             # fp32 dS [B,H,T,T]
        got["dS"] = ws[:4 * B * H * T * T].view(torch.float32).view(B, H, T, T).double()
    rescales = -(-T // 32) + 1 if (mfma and T > 256) else 0           # the long forward's online denominator
    rep = attn64.check_case(tag, c, got, bool(mfma), rescales)
    assert set(rep) == {"P", "out", "dS", "dq", "dk", "dv", "dEk", "dEv"} | ({"Pd"} if mfma else set())
    if dirty:                                                         # padded queries contribute nothing, whatever dout holds
        for b in range(B):
            assert bool((got["dq"][b, :, lens[b]:own[b]] == 0).all())
