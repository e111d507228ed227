"""gt_conv_gemm_bf16 (csrc/conv_gemm.hip, csrc/conv_common.h) against float64 on its own operands: every kernel instantiation, every
epilogue switch, under the rule of oracle/rows64.py with the restatement of oracle/conv64.py.  The cases, operands and planted defects
are oracle/conv_cases.py's, the ones tests/test_conv64.py validates on the float32 twin.

The C-ABI is called directly between guards (oracle/guards.py) on hand-made bf16 operands and weight images packed by the product's
packer (ops.PackedConv -> gt_pack_conv_weights); the reference uses the weights DECODED from the image the kernel reads.  X has a row
stride wider than Cin with NaN past Cin, Y / T / S a row stride wider than their columns with canaries kept in the gap, cond, the
addend and the saved T / S / y NaN past their columns; every output element must be written.  One case runs in place (addend = out,
a column slice of a wider fp32 buffer, as the decoder's start-conv data gradient does).

Each check prints one Report line per output with the miss factor of every planted defect, each required to be >= CONTROL_MISS."""
import numpy as np
import pytest
import torch

from oracle import conv64 as C64
from oracle import conv_cases as CC
from oracle import rows64 as R64
from oracle.guards import CAN, Guards

pytestmark = pytest.mark.gpu
F32, BF16 = torch.float32, torch.bfloat16
NAN_BITS = 0x7FC0


def dev():
    return torch.device("cuda:0")


def api():
    from glow_tts_amd import _lib
    return _lib.call, _lib.current_stream(dev())


def bf16_rows(vals, ld, bits=False):
    """[R, n] values (or raw bf16 bits) -> bf16 tensor [R, ld] with NaN in the columns past n"""
    R, n = vals.shape
    full = np.full((R, ld), NAN_BITS, dtype=np.uint16)
    full[:, :n] = vals if bits else R64.f2bf(vals)
    return torch.from_numpy(full.view(np.int16)).view(BF16)


def f32_rows(vals, ld):
    R, n = vals.shape
    full = np.full((R, ld), np.nan, dtype=np.float32)
    full[:, :n] = vals
    return torch.from_numpy(full)


def packed(c, raw):
    """the product's packer on the case's weights -> (image, Np, Kp, W [taps][N][Cin] decoded from that image)"""
    from glow_tts_amd import ops
    co, ci = raw["conv"]
    taps = c["taps"]
    pc = ops.PackedConv(co, ci, taps, gate=c["gate"] == 1, device=dev(), split3=c["x3"]).pack(torch.from_numpy(raw["v"]).to(dev()))
    torch.cuda.synchronize()
    assert pc.flags == CC.flags_of(c)
    if c["dgrad"]:
        img, Np, Kp = pc.dgrad, pc.Np_d, pc.Kp_d
        assert (Np, Kp) == (CC.np_of(ci), CC.kp_of(c["Cin"]))
        if c["x3"]:                                              # [ci][w_hi | w_lo | w_hi over co]: the GEMM's own convention
            W = R64.decode_fwd(img.cpu(), ci, c["Cin"], 1, Np, Kp, 0)
        else:
            W = R64.conv_rows_dgrad_weights(R64.decode_dgrad(img.cpu(), co, ci, taps, Np, Kp, 0))
    else:
        img, Np, Kp = pc.fwd, pc.Np_f, pc.Kp_f
        assert (Np, Kp) == (CC.np_of(co, c["gate"] == 1), CC.kp_of(c["Cin"]))
        W = R64.decode_fwd(img.cpu(), co, c["Cin"], taps, Np, Kp, 0 if c["x3"] else pc.flags)
    assert tuple(W.shape) == (taps, c["N"], c["Cin"])
    return img, Np, Kp, W


def launch(c, raw, img, Np, Kp, tile=None, out=None):
    """one guarded call of the entry -> {output: tensor [R, columns]} on the device"""
    call, st = api()
    R, N, Cin, gate = c["R"], c["N"], c["Cin"], c["gate"]
    out_f32 = (out or c["out"]) == "f32" and not gate
    G = Guards(dev())
    X = G.inp(bf16_rows(raw["X"], Cin + 8))
    bias = G.inp(torch.from_numpy(raw["bias"])) if c["bias"] else None
    cond, ldc, row0, B, Tp = None, 0, None, 0, raw["Tp"]
    if c["cond"]:
        ldc = raw["cond"].shape[1]
        cn = raw["cond"].copy()
        cn[:, N:] = np.nan
        cond = G.inp(torch.from_numpy(cn))
        if c["cond"] != "row":
            B = raw["B"]
            if c["cond"] == "ragged":
                row0 = G.inp(torch.tensor(raw["row0"], dtype=torch.int32), fill=0)
    rowmask = G.inp(torch.from_numpy(raw["rowmask"])) if c["mask"] else None
    n_out = N // 2 if gate == 1 else (2 * N if gate == 2 else N)
    dt = F32 if out_f32 else BF16
    # a gap of 4 (fp32) / 8 (bf16) columns; N = 4 and 12 in bf16: ldy % 8 == 4 turns the 16-byte store off
    ldy = n_out + (4 if out_f32 else 8)
    addend, ldadd = None, 0
    if c["addend"] == "inplace":
        ldy = 2 * n_out
        prior = torch.full((R, ldy), CAN, dtype=F32)
        prior[:, :n_out] = torch.from_numpy(raw["addend"])
        Y = G.out("y", (R, ldy), dt, prior=prior, keep=torch.arange(ldy) >= n_out)
        addend, ldadd = Y, ldy
    else:
        Y = G.out("y", (R, ldy), dt, keep=torch.arange(ldy) >= n_out)
        if c["addend"]:
            ldadd = n_out + (4 if out_f32 else 8)
            addend = G.inp(f32_rows(raw["addend"], ldadd) if out_f32 else bf16_rows(raw["addend"], ldadd))
    gate_t = gate_s = None
    ldts = 0
    if gate == 1:
        ldts = n_out + 8
        gate_t = G.out("t", (R, ldts), BF16, keep=torch.arange(ldts) >= n_out)
        gate_s = G.out("s", (R, ldts), BF16, keep=torch.arange(ldts) >= n_out)
    elif gate == 2:
        ldts = N + 8
        gate_t, gate_s = G.inp(bf16_rows(raw["T"], ldts)), G.inp(bf16_rows(raw["S"], ldts))
    elif gate == 3:
        ldts = N + 8
        gate_t = G.inp(bf16_rows(raw["ysaved"], ldts, bits=True))
    word = None
    if c["word"] is not None:
        w = c["word"] - (1 << 32) if c["word"] >= (1 << 31) else c["word"]
        word = G.inp(torch.tensor([w], dtype=torch.int32), fill=0)
    call.gt_conv_gemm_bf16(X, X.stride(0), img, bias, cond, ldc, rowmask, Y, ldy, int(out_f32), addend, ldadd, gate_t, gate_s, ldts,
                           R, N, Cin, c["taps"], Tp, Np, Kp, int(c["relu"]), gate, float(c["p"]), raw["seed"], word, row0, B,
                           c["tile"] if tile is None else tile, st)
    G.verify()
    got = {"y": Y[:, :n_out]}
    if gate == 1:
        got["t"], got["s"] = gate_t[:, :n_out], gate_s[:, :n_out]
    return got


_REFS = {}


def references(c, raw, W):
    """float64 references of a key, computed once and shared by the tiles that run the same operands"""
    if c["key"] not in _REFS:
        op = CC.op_of(c, raw, W)
        _REFS[c["key"]] = (W, op) + C64.references(op, c["defects"], c["bm"])
    W0, op, refs, amb, bads = _REFS[c["key"]]
    assert torch.equal(W0, W), "the packed image differs between two packs of the same weights"
    return op, refs, amb, bads


@pytest.mark.parametrize("name", [c["name"] for c in CC.CASES])
def test_conv_gemm_against_float64(built, name):
    c = CC.BY_NAME[name]
    raw = CC.operands(c)
    img, Np, Kp, W = packed(c, raw)
    got = launch(c, raw, img, Np, Kp)
    op, refs, amb, bads = references(c, raw, W)
    reports, misses = C64.rule(name, op, got, refs, amb, bads)
    print("CONV64|%s|%s|%s|%s|%.3g|%.3g|%.3g" % (name, CC.TILE_NAME[c["tile"]], "gate" if c["gate"] == 1 else "plain", C64.kinds(op)["y"],
                                                max(r.worst for r in reports.values()), max(r.agg for r in reports.values()),
                                                min(misses.values())))
    if c["edge"] == "clamp":
        # pinned, not assumed: with non-zero end rows the zero-padded sum is NOT what the kernel computes
        zero = C64.run(dict(op, edge="zero"))[0]["y"]
        miss = R64.check(name + " [edge=zero]", got["y"], zero[0], zero[1], "f32").miss
        print(f"{name}: the zero-padded reference misses by {miss:.3g}x")
        assert miss >= R64.CONTROL_MISS
        k2 = c["taps"] // 2                                       # and only the first and last k/2 output rows can tell them apart
        inner = R64.check(name + " [inner rows]", got["y"][k2:-k2], zero[0][k2:-k2], zero[1][k2:-k2], "f32")
        assert inner.ok, str(inner)


@pytest.mark.parametrize("label,shape,tiles", CC.EQUAL_TILES, ids=[e[0] for e in CC.EQUAL_TILES])
def test_every_tile_gives_bit_identical_fp32_outputs(built, label, shape, tiles):
    """Both kernels accumulate every output in the same (K slice, tap, k16) order, so every tile variant gives the same fp32 bits for
    the same operands: a tile-specific indexing defect shows at full strength."""
    c = CC.case(f"equal tiles {label}", shape["R"], shape["N"], shape["Cin"], shape["taps"], tiles[0], cond="ragged", mask=True)
    raw = CC.operands(c)
    img, Np, Kp, _ = packed(c, raw)
    outs = {t: launch(c, raw, img, Np, Kp, tile=t)["y"].clone() for t in tiles}
    first = outs[tiles[0]]
    assert bool((first != 0).any())
    for t in tiles[1:]:
        diff = int((outs[t].view(torch.int32) != first.view(torch.int32)).sum())
        print(f"equal tiles {label}: {CC.TILE_NAME[t]} vs {CC.TILE_NAME[tiles[0]]}: {diff} of {first.numel()} fp32 outputs differ in bits")
        assert diff == 0, CC.TILE_NAME[t]


def test_empty_call_writes_nothing(built):
    call, st = api()
    G = Guards(dev())
    prior = torch.full((4, 8), 3.0)
    Y = G.out("y", (4, 8), F32, prior=prior)
    x = torch.zeros(8, 8, dtype=BF16, device=dev())
    w = torch.zeros(64 * 64, dtype=torch.int16, device=dev())
    call.gt_conv_gemm_bf16(x, 8, w, None, None, 0, None, Y, 8, 1, None, 0, None, None, 0, 0, 8, 8, 1, 1, 64, 64, 0, 0, 0.0, 0, None, None, 0, 0, st)
    G.verify()
    assert bool((Y == 3.0).all())


@pytest.mark.parametrize("ragged", [False, True])
def test_rows_ctx_keeps_the_end_rows_masked(built, ragged):
    """the conv's precondition (zero first and last k/2 <= HALO rows) comes from the rows layout: rows [0, HALO) and [R - HALO, R)
    are halo rows whatever the lengths, full-length first and last utterances included"""
    from glow_tts_amd import ops
    for lens, T in (([7, 3, 7], 7), ([1], 1), ([5, 1, 2], 6), ([128, 60], 128)):
        lt = torch.tensor(lens, dtype=torch.int32, device=dev())
        rc = ops.RowsCtx(lt, T, lengths_host=lens, round_to=8) if ragged else ops.RowsCtx(lt, T)
        torch.cuda.synchronize()
        rm = rc.rowmask.cpu()
        assert rm.numel() == rc.R
        assert float(rm[:ops.HALO].abs().sum()) == 0 and float(rm[rc.R - ops.HALO:].abs().sum()) == 0, (lens, ragged)
        assert int(rm.sum()) == sum(lens)
        # to_rows copies frames past an utterance's length as they are (the ragged layout's rounding rows hold them): masked input,
        # as every caller provides it
        x = (torch.ones(len(lens), 8, T, device=dev()) * rc.mask_bt()[:, None, :]).to(BF16)
        rows = rc.to_rows(x).float().cpu()
        assert float(rows[:ops.HALO].abs().sum()) == 0 and float(rows[rc.R - ops.HALO:].abs().sum()) == 0, (lens, ragged)
