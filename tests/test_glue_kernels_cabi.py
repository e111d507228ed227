"""CPU tests of the refusals of the small per-step entries — gt_rows_gather_tokens (csrc/predictor_ops.hip), gt_actnorm_ddi
(csrc/flow_ops.hip), gt_mas_lengths_from_mask_f32 (csrc/mas.hip), gt_step_zero and gt_step_inputs (csrc/encoder_ops.hip) — as
include/glowtts_hip.h states them.  Everything here is host code: every call returns before a launch, so the FAKE pointers (as in
tests/test_dds_layer_cabi.py) are never dereferenced."""
import pytest

FAKE = 0x1000           # non-null, 16-byte aligned, never dereferenced
INVAL, UNSUPPORTED, ALIGN = -1, -2, -3
C = 192

GATHER = ["x_rows", "ldx", "frame2token", "Ty", "row0_x", "Tp_x", "utt_f", "row0_f", "Tp_f", "rowmask_f", "out", "R_f", "C", "stream"]
GATHER_GOOD = dict(ldx=C + 8, Ty=150, Tp_x=41, Tp_f=154, R_f=462, C=C, stream=None)
GATHER_REQUIRED = ["x_rows", "frame2token", "utt_f", "rowmask_f", "out"]


@pytest.fixture()
def L(built):
    from glow_tts_amd import _lib
    return _lib.lib()


def gather(L, **kw):
    return L.gt_rows_gather_tokens(*[kw[n] if n in kw else GATHER_GOOD.get(n, FAKE) for n in GATHER])


def test_gather_tokens_is_mirrored(L):
    from glow_tts_amd import _lib
    assert len(_lib.PROTOTYPES["gt_rows_gather_tokens"][1]) == len(GATHER)


def test_gather_tokens_nulls_and_shapes_are_invalid(L):
    for name in GATHER_REQUIRED:
        assert gather(L, **{name: None}) == INVAL, name
        assert gather(L, **{name: None}, **({} if name == "out" else {"out": FAKE + 8})) == INVAL, name      # ... before the alignment
    for bad in (dict(R_f=0), dict(R_f=-3), dict(C=0), dict(C=-8), dict(C=C + 4, ldx=C + 8), dict(C=7), dict(ldx=C + 4), dict(ldx=C + 1)):
        assert gather(L, **bad) == INVAL, bad
        assert gather(L, **bad, x_rows=FAKE + 2) == INVAL, bad


def test_gather_tokens_refuses_a_pitch_below_the_channel_count(L):
    for ldx in (C - 8, 8, 0, -8):
        assert gather(L, ldx=ldx) == INVAL, ldx
        assert gather(L, ldx=ldx, out=FAKE + 8) == INVAL, ldx


def test_gather_tokens_refuses_pointers_off_16_bytes(L):
    for off in (2, 4, 8, 14):
        assert gather(L, x_rows=FAKE + off) == ALIGN, off
        assert gather(L, out=FAKE + off) == ALIGN, off
        assert gather(L, x_rows=FAKE + off, out=FAKE + off, ldx=C) == ALIGN, off
    # the index and mask tables are read element by element: any alignment of theirs passes these checks (and the NULL layouts, the
    # uniform form, too) — shown with a misaligned row pointer, the LAST check
    assert gather(L, frame2token=FAKE + 4, utt_f=FAKE + 4, rowmask_f=FAKE + 4, row0_x=None, row0_f=None, x_rows=FAKE + 8) == ALIGN


def test_actnorm_ddi_refusals(L):
    names = ["x", "len", "B", "R", "C", "workspace", "logs", "bias", "stream"]
    good = dict(B=3, R=100, C=160, stream=None)
    call = lambda **kw: L.gt_actnorm_ddi(*[kw[n] if n in kw else good.get(n, FAKE) for n in names])
    for name in ("x", "len", "workspace", "logs", "bias"):
        assert call(**{name: None}) == INVAL, name
    for name in ("B", "R", "C"):
        for v in (0, -1, -(2 ** 31)):
            assert call(**{name: v}) == INVAL, (name, v)


def test_mas_lengths_refusals(L):
    names = ["mask", "t_x", "t_y", "B", "T_x", "T_y", "stride_b", "stride_x", "stream"]
    good = dict(B=5, T_x=10, T_y=20, stride_b=200, stride_x=20, stream=None)
    call = lambda **kw: L.gt_mas_lengths_from_mask_f32(*[kw[n] if n in kw else good.get(n, FAKE) for n in names])
    for bad in (dict(B=-1), dict(T_x=0), dict(T_y=0), dict(T_x=-4), dict(mask=None), dict(t_x=None), dict(t_y=None)):
        assert call(**bad) == INVAL, bad
    assert call(B=0) == 0 and call(B=0, mask=None, t_x=None, t_y=None) == 0          # an empty batch: nothing to do


def zero_args(_lib, ptrs, sizes, n=None, seed=FAKE):
    a = _lib.StepZeroArgs()
    for j, (p, s) in enumerate(zip(ptrs, sizes)):
        a.ptr[j], a.bytes[j] = p, s
    a.seed_word, a.seed_inc, a.n = seed, 1, len(sizes) if n is None else n
    return a


def test_step_zero_refusals(L):
    from glow_tts_amd import _lib
    assert _lib.ZERO_MAX == 4
    assert L.gt_step_zero(None, None) == INVAL
    assert L.gt_step_zero(zero_args(_lib, [FAKE] * 4, [16] * 4, n=5), None) == INVAL
    assert L.gt_step_zero(zero_args(_lib, [], [], n=-1), None) == INVAL
    for j in range(4):
        for off in (4, 8, 1):
            assert L.gt_step_zero(zero_args(_lib, [FAKE + (off if i == j else 0) for i in range(4)], [16, 0, 4112, 48]), None) == ALIGN, (j, off)
        for extra in (8, 4, 1, 15):
            assert L.gt_step_zero(zero_args(_lib, [FAKE] * 4, [16 + (extra if i == j else 0) for i in range(4)]), None) == ALIGN, (j, extra)
        assert L.gt_step_zero(zero_args(_lib, [None if i == j else FAKE for i in range(4)], [16] * 4), None) == ALIGN, j
    assert L.gt_step_zero(zero_args(_lib, [FAKE], [2 ** 35 + 16]), None) == UNSUPPORTED           # more 16-byte words than one grid indexes
    assert L.gt_step_zero(zero_args(_lib, [], [], seed=None), None) == 0                            # nothing to do: no launch


def inputs_args(_lib, n_copy=1, n_ctx=1, **kw):
    a = _lib.StepInputsArgs()
    for j in range(max(0, min(n_copy, _lib.STEP_MAX_COPIES))):
        c = a.copy[j]
        c.src, c.dst, c.rows, c.src_words, c.dst_words = kw.get("src", FAKE), kw.get("dst", FAKE), kw.get("rows", 4), kw.get("sw", 3), kw.get("dw", 5)
    for j in range(max(0, min(n_ctx, _lib.STEP_MAX_CTX))):
        c = a.ctx[j]
        for k in ("geo_src", "geo_dst", "rowbatch", "rowframe", "rowmask", "rowutt"):
            setattr(c, k, kw.get(k, FAKE))
        c.B, c.R = kw.get("B", 7), kw.get("R", 256)
    a.n_copy, a.n_ctx = n_copy, n_ctx
    return a


def test_step_inputs_refusals(L):
    from glow_tts_amd import _lib
    assert (_lib.STEP_MAX_COPIES, _lib.STEP_MAX_CTX, _lib.STEP_MAX_B) == (10, 3, 1024)
    assert L.gt_step_inputs(None, None) == INVAL
    for bad in (dict(n_copy=11), dict(n_copy=-1), dict(n_ctx=4), dict(n_ctx=-1), dict(B=1025), dict(B=0), dict(R=0), dict(R=-1),
                dict(sw=6), dict(sw=-1), dict(dw=0, sw=0), dict(rows=0), dict(src=None), dict(dst=None),
                dict(geo_src=None), dict(geo_dst=None), dict(rowbatch=None), dict(rowframe=None), dict(rowmask=None)):
        assert L.gt_step_inputs(inputs_args(_lib, **bad), None) == INVAL, bad
    for bad in (dict(src=FAKE + 2), dict(dst=FAKE + 2), dict(src=FAKE + 1), dict(dst=FAKE + 3)):
        assert L.gt_step_inputs(inputs_args(_lib, **bad), None) == ALIGN, bad
    assert L.gt_step_inputs(inputs_args(_lib, n_copy=0, n_ctx=0), None) == 0                         # nothing to do: no launch
