"""TEST INFRASTRUCTURE ONLY — the cases of the conv GEMM's float64 tests, shared by tests/test_conv64.py (CPU: the restatement, its
float32 twin and the planted defects at exactly these shapes) and tests/test_conv_gemm_fp64_gpu.py (the kernel).

A case is a dict: the GEMM's shape (R rows, N output channels, Cin reduction channels per tap — for a data gradient N is the conv's
input and Cin its output channel count, for bf16x3 Cin = 3 x the conv's), the tile forced through the C-ABI, the epilogue switches
and the planted defects its check must see.  operands(case) builds the hand-made operands from a seed derived from the case's name;
op_of(case, raw, W) assembles the dict oracle/conv64.py takes, W being the weights decoded from the image the kernel reads."""
import zlib

import numpy as np
import torch

from oracle import dropmask as DM
from oracle import rows64 as R64

HALO = 2
AUTO, T64x64, T64x128, T128x64, T128x128, T256x64, TAPS = range(7)
TILE_BM = {AUTO: 128, T64x64: 64, T64x128: 64, T128x64: 128, T128x128: 128, T256x64: 256, TAPS: 64}
TILE_NAME = {AUTO: "auto", T64x64: "64x64", T64x128: "64x128", T128x64: "128x64", T128x128: "128x128", T256x64: "256x64", TAPS: "taps"}
SHORT_TILE_MAX_WGS = 256          # conv_gemm.hip: GT_TILE_AUTO takes the 64-row tiles up to this many 128-row workgroups


def round_up(x, m):
    return -(-x // m) * m


def np_of(N, gate1=False):
    """packed rows of an image with N output channels (ops.PackedConv: Np_f / Np_d)"""
    return N if gate1 else (round_up(N, 128) if round_up(N, 64) % 128 == 0 else round_up(N, 64))


def kp_of(K):
    return round_up(K, 64)


def auto_threshold_rows(Np):
    """the largest R at which GT_TILE_AUTO still takes a 64-row tile: ceil(R / 128) * (Np / bn) <= SHORT_TILE_MAX_WGS.  (The second
    threshold of the code, ceil(R / 64) * (Np / 64) <= 4 * SHORT_TILE_MAX_WGS for the all-taps kernel, never binds: ceil(R / 64) <=
    2 ceil(R / 128) and Np / 64 <= 2 Np / bn, so it holds whenever the first does.)"""
    bn = 128 if Np % 128 == 0 else 64
    return (SHORT_TILE_MAX_WGS // (Np // bn)) * 128


def case(name, R, N, Cin, taps, tile, **kw):
    c = dict(name=name, R=R, N=N, Cin=Cin, taps=taps, tile=tile, dgrad=False, x3=False, gate=0, out="f32", bias=True, cond=None,
             relu=False, p=0.0, addend=None, mask=False, word=None, halo=True, edge="zero", defects=("weight_col",), bm=TILE_BM[tile])
    c.update(kw)
    c.setdefault("key", name)                                                  # cases with one key share operands and references
    if c["gate"]:
        c["out"] = "bf16"
    return c


def _tile_sweep():
    """every tile at R in {bm - 1, bm, bm + 1, 8 bm + 1, 5}: the ninth row tile wraps the 8-XCD order; 5 = one one-frame utterance"""
    out = []
    shapes = [(-1, 80, 3), (0, 192, 5), (1, 8, 1), (None, 80, 5), (5, 192, 3)]
    for tile in (T64x64, T64x128, T128x64, T128x128, TAPS):
        bm = TILE_BM[tile]
        N = 768 if tile in (T64x128, T128x128) else 192                       # 6 x 128 / 3 x 64 column tiles
        for d, Cin, taps in shapes:
            R = 5 if d == 5 else (8 * bm + 1 if d is None else bm + d)
            # R = 5 is one utterance of one frame: its edge taps read halo rows only, so the zeroed column is the centre tap's.
            # The row defects sit on the second tile edge, 2 bm (an utterance ends on the first): the 8 bm + 1 shape, k = 5
            defects = ("weight_mid",) if R == 5 else ("weight_col", "cond_utt") + (("row_above", "row_below") if R > 2 * bm + 2 else ())
            out.append(case(f"sweep {TILE_NAME[tile]} R={R}", R, N, Cin, taps, tile, cond="ragged", mask=True, defects=defects))
    for tile in (T64x128, T128x128, T256x64):                                  # the gate kernels
        bm = TILE_BM[tile]
        for d, Cin, taps in shapes:
            R = 5 if d == 5 else (8 * bm + 1 if d is None else bm + d)
            N = 384 if d is None else 128
            # R = 5 is one utterance of one frame: its edge taps read halo rows only, so the zeroed column is the centre tap's.
            # The row defects sit on the second tile edge, 2 bm (an utterance ends on the first): the 8 bm + 1 shape, k = 5
            defects = ("weight_mid",) if R == 5 else ("weight_col", "cond_utt") + (("row_above", "row_below") if R > 2 * bm + 2 else ())
            out.append(case(f"sweep gate {TILE_NAME[tile]} R={R}", R, N, Cin, taps, tile, gate=1, cond="ragged", defects=defects))
    return out


def _channel_sweep():
    """the widths the product uses: N = 8 proj_pad, 576 qkv, 768 / 192 the FFN, Cin = 80 ends inside a K slice; N = 4 and 12 take the
    half-chunk path, N = 4 with a row stride that turns the 16-byte bf16 store off"""
    out = []
    for N, Cin, taps in [(4, 8, 1), (8, 192, 1), (12, 80, 3), (80, 192, 1), (160, 768, 1), (192, 768, 3), (576, 192, 1), (768, 192, 3),
                         (192, 80, 5)]:
        for o in ("f32", "bf16"):
            for tile in (AUTO, T128x64):
                key = f"channels N={N} Cin={Cin} k={taps} {o}"
                out.append(case(f"{key} {TILE_NAME[tile]}", 129, N, Cin, taps, tile, out=o, mask=True, key=key, bm=64,
                                defects=("weight_col", "last_half")))
    return out


def _epilogues():
    out = []
    R, N, Cin, k = 193, 192, 192, 3
    for tile in (T64x64, TAPS, T128x64):
        t = TILE_NAME[tile]
        e = lambda name, **kw: out.append(case(f"epi {name} {t}", kw.pop("R", R), kw.pop("N", N), kw.pop("Cin", Cin), kw.pop("taps", k),
                                               tile, key=f"epi {name}", bm=64, **kw))
        e("bias", defects=("weight_col", "row_above", "row_below"))
        e("cond ragged", cond="ragged", defects=("cond_utt",))
        e("cond uniform", R=195, cond="uniform", defects=("cond_utt",))
        e("cond per row", cond="row", defects=("cond_utt",))
        e("relu", relu=True, out="bf16")
        e("ffn relu drop mask", relu=True, p=0.1, mask=True, out="bf16", N=768, defects=("keep_bit", "weight_col"))
        e("ffn seed word", relu=True, p=0.1, mask=True, out="bf16", word=0x9E3779B9, defects=("keep_bit",))
        e("addend bf16", addend="same", out="bf16", defects=("no_addend",))
        e("addend f32", addend="same", defects=("no_addend",))
        e("addend in place", addend="inplace", N=80, Cin=192, taps=1, bias=False, defects=("no_addend",))
        e("mask", mask=True, out="bf16")
        e("addend mask bf16", addend="same", mask=True, out="bf16", taps=1, defects=("no_addend",))      # the WaveNet's residual conv
        e("addend mask f32", addend="same", mask=True, defects=("no_addend",))                           # the prenet's projection
        e("relu drop addend", relu=True, p=0.1, addend="same", out="bf16", defects=("keep_bit", "no_addend"))
        e("gate2", gate=2, bias=False, addend="same", defects=("no_addend", "weight_col"))
        e("gate2 drop", gate=2, bias=False, addend="same", p=0.05, defects=("keep_bit",))
        e("gate3 p=0", gate=3, bias=False, N=768, Cin=192)
        e("gate3 p=0.1", gate=3, bias=False, p=0.1, N=768, Cin=192)
        # the combinations the product calls
        e("dgrad mask", dgrad=True, bias=False, mask=True, out="bf16", taps=5)
        e("dgrad addend", dgrad=True, bias=False, addend="same", out="bf16", taps=5, defects=("no_addend",))
        e("dgrad gate2", dgrad=True, bias=False, gate=2, addend="same", p=0.05, taps=1, defects=("keep_bit", "no_addend"))
        e("dgrad gate3", dgrad=True, bias=False, gate=3, p=0.1, N=768, Cin=192)
        e("x3 fwd", x3=True, Cin=3 * 192, taps=1)
        e("x3 dgrad", x3=True, dgrad=True, bias=False, Cin=3 * 192, taps=1)
    for tile in (T64x128, T128x128, T256x64):
        t = TILE_NAME[tile]
        for cond in (None, "ragged"):
            for p in (0.0, 0.05):
                d = ("weight_col",) + (("cond_utt",) if cond else ()) + (("keep_bit",) if p else ())
                out.append(case(f"epi gate1 cond={cond} p={p} {t}", 2 * TILE_BM[tile] + 1, 384, 192, 5, tile, gate=1, cond=cond, p=p,
                                word=0x51ED27 if p else None, defects=d))
    return out


def _auto():
    """GT_TILE_AUTO on both sides of its threshold, for Np = 192 (64-column tiles) and 768 (128-column tiles)"""
    out = []
    for N in (192, 768):
        r = auto_threshold_rows(np_of(N))
        for R in (r, r + 1):
            out.append(case(f"auto N={N} R={R}", R, N, 8, 3, AUTO, mask=True, defects=("weight_col", "row_above", "row_below")))
    return out


def _end_rows():
    """non-zero first and last rows: the kernels clamp the row index (edge = "clamp"), pinned on every kernel"""
    return [case(f"end rows k={k} {TILE_NAME[tile]}", 131, 192, 80, k, tile, halo=False, edge="clamp", bias=False)
            for tile in (T64x64, T128x64, TAPS) for k in (3, 5)]


CASES = _tile_sweep() + _channel_sweep() + _epilogues() + _auto() + _end_rows()
assert len({c["name"] for c in CASES}) == len(CASES)
BY_NAME = {c["name"]: c for c in CASES}

# the same operands through every tile the shape allows: the kernels accumulate in one (K slice, tap, k16) order
EQUAL_TILES = [("N=768", dict(R=321, N=768, Cin=192, taps=3), (T64x64, T64x128, T128x64, T128x128, TAPS, AUTO)),
               ("N=192 k=5", dict(R=321, N=192, Cin=80, taps=5), (T64x64, T128x64, TAPS, AUTO)),
               ("N=192 k=1", dict(R=321, N=192, Cin=768, taps=1), (T64x64, T128x64, TAPS, AUTO))]


# ----------------------------------------------------------------------------- geometry
def layout(R, bm):
    """ragged utterances filling [0, R): row0 [B + 1] — one utterance of length 1 (5 rows) first, one that ends exactly on the first
    tile edge where the rows allow it, every utterance at least one frame"""
    step = (3 * bm) // 8 + 3
    cuts = [0, R]
    for c in [5, bm] + list(range(5 + step, R, step)):
        if 0 < c < R and all(abs(c - q) >= 5 for q in cuts):
            cuts.append(c)
    return sorted(cuts)


def rowmask_of(row0, R):
    m = np.zeros(R, dtype=np.float32)
    for a, b in zip(row0[:-1], row0[1:]):
        m[a + HALO:b - HALO] = 1
    return m


def _bf(x):
    return R64.bf2f(R64.f2bf(x)).astype(np.float32)


def operands(c):
    """hand-made operands of a case (numpy / plain values), the same on the CPU and on the device"""
    g = np.random.default_rng(zlib.crc32(c["key"].encode()))
    R, N, Cin, taps = c["R"], c["N"], c["Cin"], c["taps"]
    raw = {}
    if c["cond"] == "uniform":
        Tp = 13
        assert R % Tp == 0
        row0 = list(range(0, R + 1, Tp))
    else:
        Tp = R
        row0 = layout(R, c["bm"])
    B = len(row0) - 1
    raw.update(row0=row0, B=B, Tp=Tp, rowmask=rowmask_of(row0, R))
    X = _bf(g.standard_normal((R, Cin)).astype(np.float32))
    if c["halo"]:
        X *= raw["rowmask"][:, None]
    raw["X"] = X
    # the conv whose image the kernel reads: v [Cout, Cin, taps]; a data gradient swaps the roles, bf16x3 splits the reduction axis
    km = 3 if c["x3"] else 1
    co, ci = (Cin // km, N) if c["dgrad"] else (N, Cin // km)
    v = (g.standard_normal((co, ci, taps)) / np.sqrt(Cin * taps / km)).astype(np.float32)
    raw["v"] = v if c["x3"] else _bf(v)              # bf16x3 keeps the fp32 weight: its hi / lo halves are the packer's
    raw["conv"] = (co, ci)
    if c["bias"]:
        raw["bias"] = (0.1 * g.standard_normal(N)).astype(np.float32)
    if c["cond"]:
        rows = R if c["cond"] == "row" else B
        raw["cond"] = (0.5 * g.standard_normal((rows, N + 4))).astype(np.float32)       # ldc = N + 4
        raw["utt"] = np.arange(R) if c["cond"] == "row" else np.repeat(np.arange(B), np.diff(row0))
    n_out = N // 2 if c["gate"] == 1 else N
    if c["addend"]:
        a = g.standard_normal((R, n_out)).astype(np.float32)
        raw["addend"] = a if (c["out"] == "f32" and not c["gate"]) else _bf(a)
    if c["gate"] == 2:
        raw["T"] = _bf(np.tanh(g.standard_normal((R, N))).astype(np.float32))
        raw["S"] = _bf((1 / (1 + np.exp(-g.standard_normal((R, N))))).astype(np.float32))
    if c["gate"] == 3:
        y = R64.f2bf(np.maximum(g.standard_normal((R, N)), 0).astype(np.float32))        # ~half +0
        y[g.random((R, N)) < 0.1] = 0x8000                                               # and -0: the kernel masks with 0x7fff
        raw["ysaved"] = y
    raw["seed"] = 0x1234 + (zlib.crc32(c["key"].encode()) & 0xFFFF)
    return raw


def op_of(c, raw, W):
    """the dict oracle/conv64.run takes; W [taps][N][Cin]: the weights the kernel reads, in the GEMM's convention"""
    R, N = c["R"], c["N"]
    op = dict(X=raw["X"].astype(np.float64), W=W, gate=c["gate"], out=c["out"], edge=c["edge"], relu=c["relu"],
              bias=raw.get("bias"), cond=raw.get("cond"), utt=raw.get("utt"), addend=raw.get("addend"),
              rowmask=raw["rowmask"] if c["mask"] else None, T=raw.get("T"), S=raw.get("S"), ysaved=raw.get("ysaved"))
    p = c["p"]
    if p:
        op["scale"] = float(DM.scale(p))
        seed = DM.word_seed(c["word"] or 0, raw["seed"])
        m = np.arange(R)[:, None]
        if c["gate"] == 1:
            op["keep"] = DM.drop_keep_gate(seed, m, np.arange(N // 2)[None, :], DM.thresh16(p))
        elif c["gate"] == 2:
            op["keep"] = DM.drop_keep_gate(seed, m, np.arange(N)[None, :], DM.thresh16(p))
        elif c["gate"] == 0:
            op["keep"] = DM.drop_keep(seed, m, np.arange(N)[None, :], DM.thresh32(p))
    return op


def flags_of(c):
    return 8 if c["x3"] else (1 if c["gate"] == 1 else 0)


def host_weights(c, raw):
    """the weights as gt_pack_conv_weights packs them, through the numpy packer and rows64's decoders -> W [taps][N][Cin] (the CPU
    test's stand-in for the device image; the device test decodes the product's own image)"""
    co, ci = raw["conv"]
    taps, fl = c["taps"], flags_of(c)
    v = torch.from_numpy(raw["v"])
    if c["x3"]:
        hi = R64.bf16_round(raw["v"])
        lo = R64.bf16_round((raw["v"] - hi.astype(np.float32)).astype(np.float32))
        Wf = np.concatenate([hi, lo, hi], 1).transpose(2, 0, 1)                       # [1][co][3 ci]: [w_hi | w_lo | w_hi]
        if not c["dgrad"]:
            return torch.from_numpy(np.ascontiguousarray(Wf))
        Wd = np.concatenate([hi, lo, hi], 0).transpose(2, 1, 0)                       # [1][ci][3 co]
        return torch.from_numpy(np.ascontiguousarray(Wd))
    Wn = R64.packed_weights(v)                                                        # [taps][co][ci]
    if c["dgrad"]:
        Np, Kp = np_of(ci), kp_of(co)
        img = R64.pack_image_np(Wn.numpy(), Np, Kp, fl, dgrad=True)
        return R64.conv_rows_dgrad_weights(R64.decode_dgrad(img, co, ci, taps, Np, Kp, fl))
    Np, Kp = np_of(co, c["gate"] == 1), kp_of(ci)
    img = R64.pack_image_np(Wn.numpy(), Np, Kp, fl)
    return R64.decode_fwd(img, co, ci, taps, Np, Kp, fl)
