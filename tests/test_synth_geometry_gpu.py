"""GPU tests of the kernels behind the captured synthesis graph (csrc/synth_front.hip): gt_synth_geometry against its
host restatement (tests/synth_geometry_host.py) and against gt_rows_ctx_fill run on the host-computed offsets, and the entries
that read the call's scalars from device memory (gt_synth_prior_call / gt_randn_rows_call) against their by-value twins.

Everything here is integer geometry or the same arithmetic on the same operands: every comparison is exact.  All outputs live
inside canary margins that must stay untouched, and are pre-filled with NaN / garbage that must be overwritten."""
import ctypes
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "golden"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import synth_geometry_host as G  # noqa: E402

pytestmark = pytest.mark.gpu
HALO = 2
CAN, MARGIN = 768.0, 1024


def dev():
    return torch.device("cuda:0")


def guarded(n, dtype, inside):
    flat = torch.full((n + 2 * MARGIN,), CAN, dtype=dtype, device=dev())
    flat[MARGIN:MARGIN + n] = inside
    return flat, flat[MARGIN:MARGIN + n]


def margins_untouched(flat, n):
    return bool((flat[:MARGIN] == CAN).all() and (flat[MARGIN + n:] == CAN).all())


def lengths_case(B, R_cap, kind):
    """(y_len [B], Ty_cap) for a named row total.  Utterance 0 has Ty_cap frames (Ty_cap + 1 in the frame-overflow case), utterance 1
    has 1 frame (squeezed length 0), the others are odd and filled in order until the rows come out as `kind` asks: 37 rows below the
    capacity, exactly the capacity, one row more, or (`middle`) everything at full length, up to three times the capacity."""
    if B == 1:
        fit = R_cap - 2 * HALO
        l, Ty_cap = {"fits": (fit - 37, 4 * R_cap), "exact": (fit, 4 * R_cap), "one_more": (fit + 1, 4 * R_cap),
                     "middle": (fit + 9, 4 * R_cap), "frames": (fit - 36, 2 * (fit - 37))}[kind]
        return [2 * l + 1], Ty_cap
    half = min(R_cap // 2, max(2, 3 * R_cap // B))         # squeezed frames of a full-length utterance
    Ty_cap = 2 * half
    if kind == "middle":                                   # the cut falls early; the last utterance asks for 3 rows and gets none
        return [Ty_cap] + [Ty_cap - 1] * (B - 2) + [7], Ty_cap
    ls = [half, 0] + [0] * (B - 2)
    target = {"fits": R_cap - 37, "exact": R_cap, "one_more": R_cap + 1, "middle": 1 << 30, "frames": R_cap - 37}[kind]
    spare = target - (2 * HALO * B + half)
    assert spare >= 0
    for i in (reversed(range(2, B)) if kind == "one_more" else range(2, B)):       # one_more: the last utterance has a frame to lose
        ls[i] = min(half, spare)
        spare -= ls[i]
    y = [2 * v + (v < half) for v in ls]                   # odd where that stays inside Ty_cap
    y[0] = Ty_cap + 1 if kind == "frames" else Ty_cap
    return y, Ty_cap


def run_geometry(y_len, Ty_cap, R_cap):
    from glow_tts_amd import _lib
    L = _lib.lib()
    st = _lib.current_stream(dev())
    B = len(y_len)
    yl = torch.tensor(y_len, dtype=torch.int32, device=dev())
    bufs = dict(row0=guarded(B + 1, torch.int32, -7), len_sq=guarded(B, torch.int32, -7), y_len_eff=guarded(B, torch.int32, -7),
                rowbatch=guarded(R_cap, torch.int64, -7), rowframe=guarded(R_cap, torch.int32, -7),
                rowmask=guarded(R_cap, torch.float32, float("nan")), rowutt=guarded(R_cap, torch.int32, -7),
                status=guarded(1, torch.int32, -7))
    order = ("row0", "len_sq", "y_len_eff", "rowbatch", "rowframe", "rowmask", "rowutt", "status")
    _lib.check(L.gt_synth_geometry(_lib.ptr(yl), B, Ty_cap, R_cap, *[_lib.ptr(bufs[k][1]) for k in order], st), "gt_synth_geometry")
    torch.cuda.synchronize()
    for k in order:
        assert margins_untouched(bufs[k][0], bufs[k][1].numel()), k
    return {k: bufs[k][1] for k in order}


def ctx_fill(row0, lens, R):
    """gt_rows_ctx_fill on host-computed offsets: the tables a ragged RowsCtx would hold"""
    from glow_tts_amd import _lib
    B = len(lens)
    r0 = torch.tensor(row0, dtype=torch.int32, device=dev())
    ln = torch.tensor(lens, dtype=torch.int32, device=dev())
    rb = torch.empty(R, dtype=torch.int64, device=dev())
    rf = torch.empty(R, dtype=torch.int32, device=dev())
    rm = torch.empty(R, dtype=torch.float32, device=dev())
    ru = torch.empty(R, dtype=torch.int32, device=dev())
    _lib.check(_lib.lib().gt_rows_ctx_fill(_lib.ptr(r0), _lib.ptr(ln), _lib.ptr(rb), _lib.ptr(rf), _lib.ptr(rm), _lib.ptr(ru), B, R,
                                           _lib.current_stream(dev())), "gt_rows_ctx_fill")
    torch.cuda.synchronize()
    return rb, rf, rm, ru


KINDS = {"fits": 0, "exact": 0, "one_more": 2, "middle": 2, "frames": 1}
# B = 65 / 1024 need 4 B rows for their halos alone: below that the entry refuses (checked), and the limit B = 1024 is laid out in
# a capacity that holds it
SHAPES = [(1, 128), (1, 640), (3, 128), (3, 640), (65, 128), (65, 640), (1024, 128), (1024, 640), (1024, 8192)]


@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("B,R_cap", SHAPES)
def test_geometry_against_the_host_and_ctx_fill(built, B, R_cap, kind):
    if 2 * HALO * B > R_cap:                               # the halos alone do not fit: refused by the entry, nothing is launched
        from glow_tts_amd import _lib
        z = torch.zeros(8, dtype=torch.int64, device=dev())
        p = _lib.ptr(z)
        assert _lib.lib().gt_synth_geometry(p, B, 40, R_cap, p, p, p, p, p, p, p, p, _lib.current_stream(dev())) == -1
        return
    y_len, Ty_cap = lengths_case(B, R_cap, kind)
    want = G.geometry(y_len, Ty_cap, R_cap)
    wish = [min(v, Ty_cap) // 2 for v in y_len]
    need = sum(w + 2 * HALO for w in wish)
    assert want["status"] == KINDS[kind], (want["status"], y_len[:8], need)
    if kind == "exact":
        assert need == R_cap
    if kind == "one_more":                                 # the cut falls in the last utterance
        assert need == R_cap + 1 and want["len_sq"][:-1] == wish[:-1] and want["len_sq"][-1] == wish[-1] - 1
    if kind == "middle" and B > 1:                         # ... or in the middle: the utterances behind it get length 0
        cut = next(b for b in range(B) if want["len_sq"][b] < wish[b])
        assert cut < B - 1 and all(v == 0 for v in want["len_sq"][cut + 1:]) and all(w > 0 for w in wish[cut + 1:])
    if B >= 3 and kind != "middle":
        assert 1 in y_len and any(v & 1 and v > 1 for v in y_len) and (Ty_cap in y_len or Ty_cap + 1 in y_len)
    got = run_geometry(y_len, Ty_cap, R_cap)
    assert got["status"].item() == want["status"]
    for k in ("row0", "len_sq", "y_len_eff", "rowbatch", "rowframe", "rowutt"):
        assert got[k].cpu().tolist() == (want[k] if k != "rowutt" else want["rowbatch"]), k
    assert got["rowmask"].cpu().tolist() == want["rowmask"]
    rb, rf, rm, ru = ctx_fill(want["row0"], want["len_sq"], R_cap)
    assert torch.equal(got["rowbatch"], rb) and torch.equal(got["rowframe"], rf) and torch.equal(got["rowutt"], ru)
    assert torch.equal(got["rowmask"], rm)
    if want["status"] == 0:                                # ... and the offsets are RowsCtx.row_starts' with starts[B] = R_cap
        from glow_tts_amd import ops
        starts, _ = ops.RowsCtx.row_starts([v // 2 for v in y_len], Ty_cap // 2, 1)
        starts[-1] = R_cap
        assert got["row0"].cpu().tolist() == starts


# ---- the call's scalars from device memory ---------------------------------------------------------------------------------------
def call_block(seed, noise_scale=1.0, noise_scale_w=1.0, length_scale=1.0):
    from glow_tts_amd import _lib
    c = _lib.SynthCall(seed=seed, noise_scale=noise_scale, noise_scale_w=noise_scale_w, length_scale=length_scale)
    host = torch.frombuffer(bytearray(bytes(c)), dtype=torch.int32).clone()
    return host.to(dev())


def test_randn_rows_call_is_the_by_value_entry(built):
    from glow_tts_amd import _lib
    L = _lib.lib()
    st = _lib.current_stream(dev())
    for R_, ncol, seed, stream, ns, nsw, which in ((300, 2, 12345, 1, 0.667, 0.25, 1), (7, 5, 0x7fffffff, 3, 0.5, 2.0, 0)):
        scale = (ns, nsw)[which]
        f_a, a = guarded(R_ * ncol, torch.float32, float("nan"))
        f_b, b = guarded(R_ * ncol, torch.float32, float("nan"))
        f_c, c = guarded(R_ * ncol, torch.float32, float("nan"))
        _lib.check(L.gt_randn_rows(_lib.ptr(a), R_, ncol, seed, stream, scale, st), "gt_randn_rows")
        _lib.check(L.gt_randn_rows_call(_lib.ptr(b), R_, ncol, _lib.ptr(call_block(seed, ns, nsw)), stream, which, st), "gt_randn_rows_call")
        _lib.check(L.gt_randn_rows_call(_lib.ptr(c), R_, ncol, _lib.ptr(call_block(seed + 1, ns, nsw)), stream, which, st), "gt_randn_rows_call")
        torch.cuda.synchronize()
        assert margins_untouched(f_a, R_ * ncol) and margins_untouched(f_b, R_ * ncol) and margins_untouched(f_c, R_ * ncol)
        assert torch.isfinite(a).all() and torch.equal(a, b)              # bit-identical
        assert not torch.equal(a, c)                                      # planted control: another seed in the block must show


@pytest.mark.parametrize("mean_only", [False, True])
def test_synth_prior_call_is_the_by_value_entry(built, mean_only):
    from glow_tts_amd import _lib, ops
    L = _lib.lib()
    st = _lib.current_stream(dev())
    g = torch.Generator().manual_seed(11)
    B, C, Tx, seed, ns = 3, 80, 19, 4321, 0.667
    xl = torch.tensor([19, 11, 7], dtype=torch.int32, device=dev())
    dur = (torch.randint(0, 9, (B, Tx), generator=g).float() * (torch.arange(Tx)[None, :] < xl.cpu()[:, None])).to(dev())
    x_m = torch.randn(B, C, Tx, generator=g).to(dev())
    x_logs = None if mean_only else (torch.randn(B, C, Tx, generator=g) * 0.3).to(dev())
    cum = torch.empty(B, Tx, dtype=torch.int32, device=dev())
    y_len = torch.empty(B, dtype=torch.int32, device=dev())
    _lib.check(L.gt_synth_lengths(_lib.ptr(dur), _lib.ptr(xl), _lib.ptr(cum), _lib.ptr(y_len), None, B, Tx, st), "gt_synth_lengths")
    lens = y_len.cpu().tolist()
    Ty = max(lens)
    assert Ty > 64                                                         # more than one tile per utterance
    lsq = [v // 2 for v in lens]
    rc = ops.RowsCtx(torch.tensor(lsq, dtype=torch.int32, device=dev()), Ty // 2, lengths_host=lsq, round_to=128)

    def run(entry, blk, aseed, ans):
        out = dict(rows=guarded(rc.R * 2 * C, torch.float32, float("nan")), z_m=guarded(B * C * Ty, torch.float32, float("nan")),
                   z_logs=guarded(B * C * Ty, torch.float32, float("nan")), frame2token=guarded(B * Ty, torch.int32, -7),
                   attn=guarded(B * Tx * Ty, torch.float32, float("nan")))
        args = _lib.fill_args(_lib.SynthPriorArgs, x_m=x_m, x_logs=x_logs, cum=cum, x_len=xl, y_len=y_len, row0=rc.row0, Tp=rc.Tp, R=rc.R,
                              B=B, C=C, Tx=Tx, Ty=Ty, seed=aseed, noise_scale=ans, **{k: v[1] for k, v in out.items()})
        if blk is None:
            _lib.check(L.gt_synth_prior(ctypes.byref(args), st), "gt_synth_prior")
        else:
            _lib.check(L.gt_synth_prior_call(ctypes.byref(args), _lib.ptr(blk), st), "gt_synth_prior_call")
        torch.cuda.synchronize()
        for k, (flat, v) in out.items():
            assert margins_untouched(flat, v.numel()), k
        return {k: v[1] for k, v in out.items()}

    by_value = run("value", None, seed, ns)
    by_call = run("call", call_block(seed, ns), 999, 0.0)                  # the by-value fields of the struct are ignored
    other = run("call", call_block(seed + 1, ns), seed, ns)
    assert not torch.isnan(by_value["rows"]).any()
    for k in by_value:
        assert torch.equal(by_value[k], by_call[k]), k
    assert not torch.equal(by_value["rows"], other["rows"])                # planted control
    for k in ("z_m", "z_logs", "frame2token", "attn"):                     # ... which leaves what does not depend on the seed alone
        assert torch.equal(by_value[k], other[k]), k
