"""CPU tests of gt_conv_gemm_bf16's argument checks (csrc/conv_gemm.hip): host code that runs without a GPU.  Every call below is
refused — or, at R == 0, returns — before a launch, so the pointers are never dereferenced."""
import pytest

FAKE = 0x10000          # a non-null, 16-byte aligned address
OK, INVAL, UNSUPPORTED, ALIGN = 0, -1, -2, -3
AUTO, T64x64, T64x128, T128x64, T128x128, T256x64, TAPS = range(7)


@pytest.fixture()
def conv(built):
    from glow_tts_amd import _lib
    L = _lib.lib()

    def call(X=FAKE, ldx=192, Wp=FAKE, bias=None, cond=None, ldc=0, rowmask=None, Y=FAKE, ldy=192, out_f32=0, addend=None, ldadd=0,
             gate_t=None, gate_s=None, ldts=0, R=100, N=192, Cin=192, taps=3, Tp=100, Np=192, Kp=192, relu=0, gate=0, drop_p=0.0,
             seed=0, seed_dev=None, row0=None, B=0, tile=AUTO):
        return L.gt_conv_gemm_bf16(X, ldx, Wp, bias, cond, ldc, rowmask, Y, ldy, out_f32, addend, ldadd, gate_t, gate_s, ldts,
                                   R, N, Cin, taps, Tp, Np, Kp, relu, gate, drop_p, seed, seed_dev, row0, B, tile, None)
    return call


def test_shape_and_pointer_refusals(conv):
    assert conv(R=-1) == INVAL and conv(N=0) == INVAL and conv(Cin=0) == INVAL
    assert conv(X=None) == INVAL and conv(Wp=None) == INVAL and conv(Y=None) == INVAL
    assert conv(tile=-1) == INVAL and conv(tile=7) == INVAL
    assert conv(Np=160) == INVAL                                  # Np % 64
    assert conv(N=192, Np=128, Kp=192) == INVAL                   # Np < N
    assert conv(cond=FAKE, ldc=192, Tp=0) == INVAL                # cond needs the rows per utterance
    assert conv(cond=FAKE, ldc=192, row0=FAKE, B=0) == INVAL      # a ragged layout needs its utterance count


def test_an_empty_call_returns_ok_before_anything_is_looked_at(conv):
    assert conv(R=0) == OK
    assert conv(R=0, X=None, Wp=None, Y=None, taps=4, tile=99) == OK


def test_unsupported_taps_and_dropout(conv):
    for taps in (0, 2, 4, 6, 7):
        assert conv(taps=taps) == UNSUPPORTED, taps
    assert conv(drop_p=1.0) == UNSUPPORTED and conv(drop_p=1.5) == UNSUPPORTED


def test_alignment_the_entry_already_checked(conv):
    assert conv(N=190) == ALIGN and conv(Cin=188) == ALIGN and conv(ldx=196) == ALIGN and conv(ldy=194) == ALIGN
    assert conv(Kp=200) == ALIGN and conv(Cin=256, Kp=192) == ALIGN
    assert conv(X=FAKE + 8) == ALIGN and conv(Wp=FAKE + 8) == ALIGN and conv(Y=FAKE + 8) == ALIGN
    assert conv(addend=FAKE, ldadd=194) == ALIGN


def test_alignment_of_the_epilogue_operands(conv):
    """bias, cond and a fp32 addend are read as float4, a bf16 addend as 8-byte halves, cond rows at a stride of ldc floats"""
    for off in (4, 8, 12):
        assert conv(bias=FAKE + off) == ALIGN, off
        assert conv(cond=FAKE + off, ldc=192) == ALIGN, off
        assert conv(addend=FAKE + off, ldadd=192, out_f32=1) == ALIGN, off
    for ldc in (193, 194, 195):
        assert conv(cond=FAKE, ldc=ldc) == ALIGN, ldc
    for off in (2, 4, 6):
        assert conv(addend=FAKE + off, ldadd=192) == ALIGN, off
    assert conv(addend=FAKE + 8, ldadd=192, out_f32=1) == ALIGN   # 8 bytes do for bf16 only
    for off in (1, 2, 3):
        assert conv(rowmask=FAKE + off) == ALIGN, off
    # the aligned forms pass these checks: they are refused by a LATER one (an unknown tile), not by GT_E_ALIGN
    assert conv(bias=FAKE, cond=FAKE, ldc=196, addend=FAKE + 8, ldadd=192, rowmask=FAKE + 4, tile=7) == INVAL
    assert conv(addend=FAKE + 16, ldadd=192, out_f32=1, tile=7) == INVAL


def test_tiles_the_shape_does_not_allow(conv):
    assert conv(tile=T64x128) == INVAL and conv(tile=T128x128) == INVAL          # Np = 192 is no multiple of 128
    assert conv(tile=T256x64) == INVAL                                            # gate only
    g = dict(gate=1, gate_t=FAKE, gate_s=FAKE, ldts=192, N=384, Np=384)
    assert conv(tile=TAPS, **g) == INVAL and conv(tile=T64x64, **g) == INVAL and conv(tile=T128x64, **g) == INVAL


def test_gate_forward_preconditions(conv):
    g = dict(gate=1, gate_t=FAKE, gate_s=FAKE, ldts=192, N=384, Np=384, tile=T64x64)     # valid but for the tile: INVAL at the very end
    assert conv(**g) == INVAL
    assert conv(**{**g, "gate_t": None}) == INVAL and conv(**{**g, "gate_s": None}) == INVAL
    assert conv(**{**g, "N": 192, "Np": 192}) == INVAL                            # N % 128
    assert conv(**{**g, "Np": 512}) == INVAL                                      # Np != N
    assert conv(**{**g, "out_f32": 1}) == INVAL
    # the gate epilogue applies no relu, addend or rowmask: refused, never silently ignored
    assert conv(**{**g, "tile": AUTO, "addend": FAKE, "ldadd": 192}) == INVAL
    assert conv(**{**g, "tile": AUTO, "rowmask": FAKE}) == INVAL and conv(**{**g, "tile": AUTO, "relu": 1}) == INVAL
    assert conv(**{**g, "ldts": 196}) == ALIGN and conv(**{**g, "ldy": 196}) == ALIGN
    assert conv(**{**g, "gate_t": FAKE + 8}) == ALIGN and conv(**{**g, "gate_s": FAKE + 8}) == ALIGN


@pytest.mark.parametrize("gate", [2, 3])
def test_fused_backward_preconditions(conv, gate):
    g = dict(gate=gate, gate_t=FAKE, gate_s=FAKE, ldts=192, ldy=384, tile=T64x128)       # valid but for the tile
    assert conv(**g) == INVAL
    assert conv(**{**g, "gate_t": None, "tile": AUTO}) == INVAL
    if gate == 2:
        assert conv(**{**g, "gate_s": None, "tile": AUTO}) == INVAL
        assert conv(**{**g, "gate_s": FAKE + 8}) == ALIGN
    for bad in (dict(out_f32=1), dict(relu=1), dict(N=196, Np=256, Kp=192), dict(ldts=196), dict(ldy=388)):
        assert conv(**{**g, "tile": AUTO, **bad}) == INVAL, bad
    assert conv(**{**g, "gate_t": FAKE + 8}) == ALIGN
