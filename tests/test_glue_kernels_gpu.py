"""The small kernels every training step runs, each called through its C-ABI entry on hand-made operands between guards
(oracle/guards.py) and compared BIT FOR BIT with a plain numpy restatement:

  gt_rows_gather_tokens          (csrc/predictor_ops.hip)  frame rows <- token rows of the hard alignment, 16 bytes per thread
  gt_mas_lengths_from_mask_f32   (csrc/mas.hip)            t_x, t_y from the mask's first column / row, any strides
  gt_step_zero                   (csrc/encoder_ops.hip)    the fills at the head of a step + the dropout seed's bump
  gt_step_inputs                 (csrc/encoder_ops.hip)    padded copies + ragged row contexts of a replayed step, one grid split by blk0

Inputs sit between NaN guards (integer inputs: in-range values that differ from the real ones); rows and columns a kernel must not
read hold NaN bits; outputs are pre-filled with canaries, or with a value no result can take, so a skipped element, a read outside
the operand and a write past the end are all reported."""
import numpy as np
import pytest
import torch

from oracle.guards import CAN, Guards
from oracle.loss64 import HALO, Layout

pytestmark = pytest.mark.gpu
INVAL, ALIGN = -1, -3
NEVER = -12345                                               # no row table, row offset or length holds it
I16, I32, I64 = torch.int16, torch.int32, torch.int64


def dev():
    return torch.device("cuda:0")


def api():
    from glow_tts_amd import _lib
    return _lib.call, _lib.current_stream(dev()), _lib


def same_bits(name, got, want):
    got, want = got.detach().cpu().numpy(), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (name, got.shape, want.shape, got.dtype, want.dtype)
    bad = np.nonzero(got.reshape(-1) != want.reshape(-1))[0]
    print(f"{name}: {got.size} elements, {bad.size} differ")
    assert bad.size == 0, f"{name}: {bad.size} elements differ, first at {bad[0]}: got {got.reshape(-1)[bad[0]]}, want {want.reshape(-1)[bad[0]]}"


# ----------------------------------------------------------------------------- gt_rows_gather_tokens
TEXT_LENS, FRAME_LENS = [1, 5, 37], [150, 3, 120]
BF16_NAN = np.int16(0x7FC1)


def gather_case(C, ldx, ragged):
    """text rows [R_x, ldx] (bf16 bits; NaN bits in the pitch columns and in every row that holds no token), frame2token with
    repeated and skipped tokens and -1 past each utterance's frames, the two layouts, and the expected frame rows"""
    rng = np.random.default_rng(C + ldx + ragged)
    lx, lf = Layout(TEXT_LENS, max(TEXT_LENS), ragged, 8), Layout(FRAME_LENS, max(FRAME_LENS), ragged, 10)
    assert lf.R * C // 8 > 256 and (lf.R * C // 8) % 256 != 0
    x = np.full((lx.R, ldx), BF16_NAN, dtype=np.int16)
    vals = torch.from_numpy(rng.normal(0, 2, size=(int(lx.valid.sum()), C)).astype(np.float32)).to(torch.bfloat16).view(I16).numpy()
    vals[0, :2] = [np.int16(-0x8000), 0]                     # -0 and +0 travel as they are
    x[np.nonzero(lx.valid)[0][:, None], np.arange(C)[None, :]] = vals
    Ty = max(FRAME_LENS)
    f2t = np.full((lf.B, Ty), -1, dtype=np.int32)
    for b, (tx, ty) in enumerate(zip(TEXT_LENS, FRAME_LENS)):
        f2t[b, :ty] = np.sort(rng.integers(0, tx, size=ty))  # monotone: tokens repeat (ty > tx) and are skipped (ty < tx)
    assert len(set(f2t[1, :3])) < 5 and len(set(f2t[2, :120])) <= 37 and (np.diff(f2t[2, :120]) == 0).any()
    want = np.zeros((lf.R, C), dtype=np.int16)
    for m in np.nonzero(lf.valid)[0]:
        b = lf.rowbatch[m]
        want[m] = x[lx.base[b] + HALO + f2t[b, lf.rowframe[m]], :C]
    assert not (want == BF16_NAN).any()
    return lx, lf, x, f2t, want


@pytest.mark.parametrize("ragged", [False, True])
@pytest.mark.parametrize("pitch", [0, 8])
@pytest.mark.parametrize("C", [8, 192])
def test_gather_tokens_bit_for_bit(built, C, pitch, ragged):
    call, st, _ = api()
    ldx = C + pitch
    lx, lf, x, f2t, want = gather_case(C, ldx, ragged)
    G = Guards(dev())
    out = G.out("out", (lf.R, C), dtype=torch.bfloat16)
    xr = G.inp(torch.from_numpy(x).view(torch.bfloat16))
    row0_x = G.inp(torch.from_numpy(lx.row0), fill=0) if ragged else None
    row0_f = G.inp(torch.from_numpy(lf.row0), fill=0) if ragged else None
    assert xr.data_ptr() % 16 == 0 and out.data_ptr() % 16 == 0
    call.gt_rows_gather_tokens(xr, ldx, G.inp(torch.from_numpy(f2t), fill=0), f2t.shape[1], row0_x, lx.Tp,
                               G.inp(torch.from_numpy(lf.rowbatch.astype(np.int32)), fill=0), row0_f, lf.Tp,
                               G.inp(torch.from_numpy(lf.rowmask)), out, lf.R, C, st)
    G.verify()
    same_bits(f"gt_rows_gather_tokens C={C} ldx={ldx} {'ragged' if ragged else 'uniform'}", out.view(I16), want)


def test_gather_tokens_refusals_leave_the_output_alone(built):
    call, st, _lib = api()
    C = 8
    lx, lf, x, f2t, want = gather_case(C, C + 8, True)
    G = Guards(dev())
    out = G.out("out", (lf.R + 1, C), dtype=torch.bfloat16)
    xr = G.inp(torch.from_numpy(x).view(torch.bfloat16))
    rest = (G.inp(torch.from_numpy(lf.rowbatch.astype(np.int32)), fill=0), G.inp(torch.from_numpy(lf.row0), fill=0), lf.Tp, G.inp(torch.from_numpy(lf.rowmask)))
    head = (G.inp(torch.from_numpy(f2t), fill=0), f2t.shape[1], G.inp(torch.from_numpy(lx.row0), fill=0), lx.Tp)
    flat_x, flat_o = xr.reshape(-1), out.reshape(-1)
    for xa, ld, oa, c, code in ((flat_x[4:], C + 8, out, C, ALIGN), (xr, C + 8, flat_o[4:], C, ALIGN), (flat_x[1:], C + 8, out, C, ALIGN),
                                (xr, C - 8, out, C, INVAL), (xr, 8, out, 16, INVAL), (xr, C + 4, out, C, INVAL), (xr, C + 8, out, 4, INVAL)):
        with pytest.raises(_lib.GtError) as e:
            call.gt_rows_gather_tokens(xa, ld, *head, *rest, oa, lf.R, c, st)
        assert e.value.code == code, (ld, c, code)
    torch.cuda.synchronize()
    assert bool((out.float() == CAN).all())


# ----------------------------------------------------------------------------- gt_mas_lengths_from_mask_f32
MAS_SHAPES = [(1, 1), (1, 2049), (513, 1), (255, 4), (256, 1000), (257, 2049), (513, 4), (513, 2049), (256, 1)]


def mas_mask(T_x, T_y, seed):
    """[5, T_x, T_y] of 0 / 1: rectangles of every length (one empty, one full), with holes away from row 0 and column 0"""
    rng = np.random.default_rng(seed)
    tx = [T_x, 0, max(1, T_x // 2), 1, max(1, T_x - 1)]
    ty = [T_y, 0, max(1, T_y - 1), 1, max(1, T_y // 3)]
    m = np.zeros((5, T_x, T_y), dtype=np.float32)
    for b in range(5):
        m[b, :tx[b], :ty[b]] = 1
    holes = rng.random(m.shape) < 0.3
    holes[:, 0, :] = holes[:, :, 0] = False
    m[holes] = 0
    return m, m[:, :, 0].astype(np.float64).sum(1).astype(np.int32), m[:, 0, :].astype(np.float64).sum(1).astype(np.int32)


@pytest.mark.parametrize("shape", MAS_SHAPES)
def test_mas_lengths_from_a_window_of_a_larger_buffer(built, shape):
    call, st, _ = api()
    T_x, T_y = shape
    m, want_x, want_y = mas_mask(T_x, T_y, T_x + T_y)
    assert CAN not in want_x and CAN not in want_y and want_x[1] == want_y[1] == 0 and want_x[0] == T_x and want_y[0] == T_y
    big = torch.full((5, T_x + 3, T_y + 5), 1e6)
    big[:, 1:1 + T_x, 2:2 + T_y] = torch.from_numpy(m)
    G = Guards(dev())
    win = G.inp(big)[:, 1:1 + T_x, 2:2 + T_y]
    assert win.stride(0) > T_x * win.stride(1) and win.stride(1) > T_y and win.stride(2) == 1
    t_x, t_y = G.out("t_x", (5,), dtype=I32), G.out("t_y", (5,), dtype=I32)
    call.gt_mas_lengths_from_mask_f32(win, t_x, t_y, 5, T_x, T_y, win.stride(0), win.stride(1), st)
    G.verify()
    same_bits(f"t_x {shape}", t_x, want_x)
    same_bits(f"t_y {shape}", t_y, want_y)


def test_mas_lengths_through_the_host_entry(built):
    """monotonic_align.lengths_from_mask on a bool mask, an fp16 mask and a mask whose last dimension is not contiguous"""
    from glow_tts_amd import monotonic_align as ma
    m, want_x, want_y = mas_mask(257, 1000, 3)
    md = torch.from_numpy(m).to(dev())
    tr = torch.from_numpy(np.ascontiguousarray(m.transpose(0, 2, 1))).to(dev()).transpose(1, 2)
    assert tr.stride(2) != 1 and tr.shape == md.shape
    for name, mask in (("bool", md != 0), ("fp16", md.half()), ("transposed", tr), ("fp32", md)):
        t_x, t_y = ma.lengths_from_mask(mask)
        same_bits(f"lengths_from_mask {name} t_x", t_x, want_x)
        same_bits(f"lengths_from_mask {name} t_y", t_y, want_y)


# ----------------------------------------------------------------------------- gt_step_zero
PATTERN = 0x55555555
SEED_INC = 0x632BE5AB


def zero_setup(sizes):
    """one int32 buffer of PATTERN words; region j of sizes[j] bytes starts 16-byte aligned with guard words behind it
    -> (buffer, byte offsets, expected words after the call)"""
    offs, at = [], 64
    for s in sizes:
        offs.append(at)
        at += s + 32                                         # 32 bytes of guard words behind every region (an empty one included)
    buf = torch.full((at // 4 + 16,), PATTERN, dtype=I32, device=dev())
    assert buf.data_ptr() % 16 == 0
    want = np.full(buf.numel(), PATTERN, dtype=np.int32)
    for o, s in zip(offs, sizes):
        want[o // 4:(o + s) // 4] = 0
    return buf, offs, want


def zero_args(_lib, buf, offs, sizes, seed=None, inc=0, n=None):
    a = _lib.StepZeroArgs()
    for j, (o, s) in enumerate(zip(offs, sizes)):
        a.ptr[j], a.bytes[j] = buf.data_ptr() + o, s
    a.seed_word, a.seed_inc, a.n = (None if seed is None else seed.data_ptr()), inc, (len(sizes) if n is None else n)
    return a


def seed_tensor(value):
    s = torch.full((8,), PATTERN, dtype=I32, device=dev())
    s[4:5] = torch.from_numpy(np.array([value], dtype=np.uint32).view(np.int32)).to(dev())
    return s, s[4:5]


def seed_value(s):
    w = s.cpu().numpy().view(np.uint32)
    assert (np.delete(w, 4) == PATTERN).all(), "a word next to the seed was written"
    return int(w[4])


@pytest.mark.parametrize("sizes", [(16, 0, 4096 + 16, 48), (4096 + 16, 48, 16, 0), (0, 0, 16, 4096 + 16), (48, 4096 + 16, 0, 16)])
@pytest.mark.parametrize("with_seed", [False, True])
def test_step_zero_region_boundaries_inside_a_workgroup(built, sizes, with_seed):
    _, st, _lib = api()
    assert len(sizes) == _lib.ZERO_MAX and sum(sizes) // 16 > 256
    buf, offs, want = zero_setup(sizes)
    s, word = seed_tensor(0xFFFFFFF0) if with_seed else (None, None)
    assert _lib.lib().gt_step_zero(zero_args(_lib, buf, offs, sizes, seed=word, inc=SEED_INC), st) == 0
    torch.cuda.synchronize()
    same_bits(f"gt_step_zero {sizes}", buf, want)
    if with_seed:                                            # the increment wraps past 2^32
        assert seed_value(s) == (0xFFFFFFF0 + SEED_INC) - 2 ** 32


def test_step_zero_empty_regions_advance_the_seed_exactly_once(built):
    _, st, _lib = api()
    for sizes in ((), (0,), (0, 0, 0, 0)):
        buf, offs, want = zero_setup(sizes)
        s, word = seed_tensor(7)
        assert _lib.lib().gt_step_zero(zero_args(_lib, buf, offs, sizes, seed=word, inc=SEED_INC), st) == 0
        torch.cuda.synchronize()
        assert seed_value(s) == 7 + SEED_INC, sizes
        same_bits(f"gt_step_zero {sizes}", buf, want)
        # ... and with neither regions nor a seed the call is a no-op
        assert _lib.lib().gt_step_zero(zero_args(_lib, buf, offs, sizes), st) == 0
        torch.cuda.synchronize()
        same_bits(f"gt_step_zero {sizes}, no seed", buf, want)


def test_step_zero_refusals_write_nothing(built):
    _, st, _lib = api()
    sizes = (16, 0, 4096 + 16, 48)
    buf, offs, _ = zero_setup(sizes)
    s, word = seed_tensor(7)
    untouched = np.full(buf.numel(), PATTERN, dtype=np.int32)
    L = _lib.lib()
    for j in range(4):                                       # a misaligned pointer, a byte count that is no multiple of 16: any region
        o = list(offs); o[j] += 4
        assert L.gt_step_zero(zero_args(_lib, buf, o, sizes, seed=word, inc=SEED_INC), st) == ALIGN, j
        z = list(sizes); z[j] += 8
        assert L.gt_step_zero(zero_args(_lib, buf, offs, z, seed=word, inc=SEED_INC), st) == ALIGN, j
    assert L.gt_step_zero(zero_args(_lib, buf, offs, sizes, seed=word, inc=SEED_INC, n=_lib.ZERO_MAX + 1), st) == INVAL
    assert L.gt_step_zero(zero_args(_lib, buf, offs, sizes, seed=word, inc=SEED_INC, n=-1), st) == INVAL
    torch.cuda.synchronize()
    same_bits("gt_step_zero refused", buf, untouched)
    assert seed_value(s) == 7


# ----------------------------------------------------------------------------- gt_step_inputs
# (rows, src_words, dst_words, bytes per element): rows * dst_words = 1 / 1024 / 1025 (one word, the last word of a workgroup's 1024,
# the first of the next), src_words == dst_words, src_words == 0 (every row zeroed), 2-byte elements packed two per word, rows that
# span workgroups
COPIES = [(1, 1, 1, 4), (1, 1000, 1024, 4), (1, 1025, 1025, 4), (25, 40, 41, 4), (32, 0, 32, 4), (7, 3, 5, 4), (3, 123, 160, 4), (5, 3, 4, 2),
          (2, 700, 2000, 4), (1025, 1, 1, 4)]
# (lens, T, round_to): B = 1 with R over two workgroups; B = GT_STEP_MAX_B utterances of one frame (R = 5120); a mixed batch
CTXS = [([300], 300, 64), ([1] * 1024, 1, 64), ([33, 17, 40, 5, 29, 40, 12], 40, 64)]


def make_copy(G, spec, seed):
    rows, sw, dw, esz = spec
    dt, npdt, per = (I32, np.int32, 1) if esz == 4 else (I16, np.int16, 2)
    rng = np.random.default_rng(seed)
    src = rng.integers(1000, 30000, size=(rows, max(sw * per, 1))).astype(npdt)      # never 0, never the canary
    want = np.zeros((rows, dw * per), dtype=npdt)
    want[:, :sw * per] = src[:, :sw * per]
    s = G.inp(torch.from_numpy(src if sw else src[:, :1]), fill=NEVER)
    d = G.out(f"copy {spec}", (rows, dw * per), dtype=dt)
    return s, d, want


def make_ctx(G, spec, call=None, st=None):
    """guarded outputs of one context + the host restatement; with `call`: filled by gt_rows_ctx_fill instead (the twin)"""
    lens, T, rnd = spec
    lay = Layout(lens, T, True, rnd)
    B, R = lay.B, lay.R
    geo = np.concatenate([lay.row0, np.asarray(lens, dtype=np.int32)]).astype(np.int32)
    never = lambda n, dt: torch.full((n,), NEVER, dtype=dt)
    o = dict(geo_dst=G.out("geo_dst", (2 * B + 1,), dtype=I32, prior=never(2 * B + 1, I32)),
             rowbatch=G.out("rowbatch", (R,), dtype=I64, prior=never(R, I64)), rowframe=G.out("rowframe", (R,), dtype=I32, prior=never(R, I32)),
             rowmask=G.out("rowmask", (R,)), rowutt=G.out("rowutt", (R,), dtype=I32, prior=never(R, I32)))
    src = G.inp(torch.from_numpy(geo), fill=3)
    want = dict(geo_dst=geo, rowbatch=lay.rowbatch.astype(np.int64), rowframe=lay.rowframe.astype(np.int32), rowmask=lay.rowmask,
                rowutt=lay.rowbatch.astype(np.int32))
    if call is not None:
        call.gt_rows_ctx_fill(src[:B + 1], src[B + 1:], o["rowbatch"], o["rowframe"], o["rowmask"], o["rowutt"], B, R, st)
        o["geo_dst"].copy_(src)
    return src, o, want, B, R


def run_step_inputs(copies, ctxs):
    call, st, _lib = api()
    G = Guards(dev())
    a = _lib.StepInputsArgs()
    cs = [make_copy(G, spec, i) for i, spec in enumerate(copies)]
    for j, (spec, (s, d, _)) in enumerate(zip(copies, cs)):
        c = a.copy[j]
        c.src, c.dst, c.rows, c.src_words, c.dst_words, c.blk0 = s.data_ptr(), d.data_ptr(), spec[0], spec[1], spec[2], -7    # blk0: the call's
    xs = [make_ctx(G, spec) for spec in ctxs]
    for j, (src, o, _, B, R) in enumerate(xs):
        c = a.ctx[j]
        c.geo_src, c.B, c.R, c.blk0 = src.data_ptr(), B, R, -7
        for k, v in o.items():
            setattr(c, k, v.data_ptr())
    a.n_copy, a.n_ctx = len(copies), len(ctxs)
    call.gt_step_inputs(a, st)
    G.verify()
    assert all(a.copy[j].blk0 == -7 for j in range(len(copies))) and all(a.ctx[j].blk0 == -7 for j in range(len(ctxs)))    # the caller's structure is not written
    for spec, (_, d, want) in zip(copies, cs):
        same_bits(f"copy {spec}", d, want)
    G2 = Guards(dev())
    for spec, (_, o, want, B, R) in zip(ctxs, xs):
        _, twin, _, _, _ = make_ctx(G2, spec, call, st)
        for k in want:
            same_bits(f"ctx B={B} R={R} {k}", o[k], want[k])
            same_bits(f"ctx B={B} R={R} {k} vs gt_rows_ctx_fill", twin[k], want[k])
    G2.verify()


def test_step_inputs_maxima_in_one_call(built):
    """GT_STEP_MAX_COPIES copies and GT_STEP_MAX_CTX contexts in one grid: every block finds its job through blk0"""
    _, _, _lib = api()
    assert len(COPIES) == _lib.STEP_MAX_COPIES and len(CTXS) == _lib.STEP_MAX_CTX and len(CTXS[1][0]) == _lib.STEP_MAX_B
    assert sorted(r * d for r, _, d, _ in COPIES)[:1] == [1] and {1024, 1025} <= {r * d for r, _, d, _ in COPIES}
    run_step_inputs(COPIES, CTXS)


@pytest.mark.parametrize("which", ["copies only", "contexts only", "one of each", "contexts reversed"])
def test_step_inputs_partitions(built, which):
    copies, ctxs = {"copies only": (COPIES, []), "contexts only": ([], CTXS), "one of each": (COPIES[2:3], CTXS[:1]),
                    "contexts reversed": (COPIES[1:4][::-1], CTXS[::-1])}[which]
    run_step_inputs(copies, ctxs)


def test_step_inputs_refusals_write_nothing(built):
    _, st, _lib = api()
    G = Guards(dev())
    s, d, _ = make_copy(G, (4, 3, 5, 4), 0)
    src, o, _, B, R = make_ctx(G, CTXS[2])

    def args(n_copy=1, n_ctx=1, **kw):
        a = _lib.StepInputsArgs()
        for j in range(min(n_copy, _lib.STEP_MAX_COPIES)):
            c = a.copy[j]
            c.src, c.dst, c.rows, c.src_words, c.dst_words = s.data_ptr() + kw.get("src_off", 0), d.data_ptr() + kw.get("dst_off", 0), 4, kw.get("sw", 3), kw.get("dw", 5)
        for j in range(min(n_ctx, _lib.STEP_MAX_CTX)):
            c = a.ctx[j]
            c.geo_src, c.B, c.R = src.data_ptr(), kw.get("B", B), kw.get("R", R)
            for k, v in o.items():
                setattr(c, k, v.data_ptr())
        a.n_copy, a.n_ctx = n_copy, n_ctx
        return a
    L = _lib.lib()
    for kw, code in ((dict(B=_lib.STEP_MAX_B + 1), INVAL), (dict(B=0), INVAL), (dict(R=0), INVAL), (dict(sw=6), INVAL), (dict(sw=-1), INVAL),
                     (dict(dw=0, sw=0), INVAL), (dict(src_off=2), ALIGN), (dict(dst_off=2), ALIGN), (dict(src_off=1), ALIGN),
                     (dict(n_copy=_lib.STEP_MAX_COPIES + 1), INVAL), (dict(n_ctx=_lib.STEP_MAX_CTX + 1), INVAL), (dict(n_copy=-1), INVAL)):
        assert L.gt_step_inputs(args(**kw), st) == code, kw
    torch.cuda.synchronize()
    assert bool((d == int(CAN)).all()) and bool((o["rowmask"] == CAN).all()) and all(bool((o[k] == NEVER).all()) for k in o if k != "rowmask")
