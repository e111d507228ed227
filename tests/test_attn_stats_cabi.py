"""CPU tests of the P-free attention pair (gt_attn_fwd_stats / gt_attn_bwd_stats, csrc/attn_long.hip): the two size functions, the
refusal table of include/glowtts_hip.h entry by entry and in its order (NULL pointers, then the token limit and the shape, then the
workspace size, then alignment), and the host-side switches.  Everything here is host code: every call returns before a launch,
so the FAKE pointers (as in tests/test_attn_long_cabi.py) are never dereferenced."""
import types

import pytest

FAKE = 0x1000           # non-null, 16-byte aligned, never dereferenced
INVAL, UNSUPPORTED, ALIGN = -1, -2, -3


def _fwd(L, T, D=96, win=4, B=1, H=2, stats=FAKE, q=FAKE, ld=None, ldo=None, out=FAKE):
    ld = 3 * H * D if ld is None else ld
    ldo = H * D if ldo is None else ldo
    return L.gt_attn_fwd_stats(q, FAKE, FAKE, ld, FAKE, FAKE, FAKE, out, ldo, stats, B, T, T + 2, None, H, D, win, 0.0, 0, None, None)


def _bwd(L, T, D=96, win=4, B=1, H=2, stats=FAKE, ws=FAKE, ws_bytes=None, q=FAKE, ld=None, lddo=None, lddq=None, dEv=FAKE):
    ws_bytes = L.gt_attn_bwd_stats_workspace_bytes(B, T, H) if ws_bytes is None else ws_bytes
    ld = 3 * H * D if ld is None else ld
    lddo = H * D if lddo is None else lddo
    lddq = 3 * H * D if lddq is None else lddq
    return L.gt_attn_bwd_stats(q, FAKE, FAKE, ld, FAKE, FAKE, FAKE, FAKE, lddo, stats, ws, ws_bytes, FAKE, FAKE, FAKE, lddq,
                               FAKE, dEv, B, T, T + 2, None, H, D, win, 0.0, 0, None, None)


def test_size_functions(built):
    from glow_tts_amd import _lib
    L = _lib.lib()
    assert L.gt_attn_stats_bytes(1, 506, 2) == 8 * 1 * 2 * 506 == 8096
    assert L.gt_attn_stats_bytes(32, 4096, 2) == 8 * 32 * 2 * 4096 == 2097152
    # one record of 20 floats per query row: Dsum, 9 + 9 band entries, one pad
    assert L.gt_attn_bwd_stats_workspace_bytes(1, 506, 2) == 80 * 1 * 2 * 506 == 80960
    assert L.gt_attn_bwd_stats_workspace_bytes(32, 4096, 2) == 80 * 32 * 2 * 4096 == 20971520
    for f in (L.gt_attn_stats_bytes, L.gt_attn_bwd_stats_workspace_bytes):
        for bad in ((0, 506, 2), (1, 0, 2), (1, 506, 0), (-1, 506, 2), (1, -506, 2), (1, 506, -2)):
            assert f(*bad) == 0, bad
    # O(B H T): 4096 tokens at B = 32 take 23 MB where P and the saved-P workspace take 4.3 GB each
    assert L.gt_attn_stats_bytes(32, 4096, 2) + L.gt_attn_bwd_stats_workspace_bytes(32, 4096, 2) < 2 ** 25
    assert L.gt_attn_bwd_workspace_bytes(32, 4096, 2) > 2 ** 32


@pytest.mark.parametrize("T", [506, 512, 513, 1025, 4096])
def test_accepted_shapes_reach_the_alignment_check(built, T):
    """The other direction of every refusal below: with nothing wrong but one stride, the call gets as far as the LAST check."""
    from glow_tts_amd import _lib
    L = _lib.lib()
    assert _fwd(L, T, ld=3 * 2 * 96 + 4) == ALIGN and _bwd(L, T, ld=3 * 2 * 96 + 4) == ALIGN


def test_null_pointers_come_first(built):
    from glow_tts_amd import _lib
    L = _lib.lib()
    assert _fwd(L, 506, stats=None) == INVAL and _bwd(L, 506, stats=None) == INVAL
    assert _fwd(L, 506, q=None) == INVAL and _fwd(L, 506, out=None) == INVAL
    assert _bwd(L, 506, ws=None) == INVAL and _bwd(L, 506, q=None) == INVAL and _bwd(L, 506, dEv=None) == INVAL
    # ... before the shape, the workspace size and alignment
    assert _fwd(L, 4097, stats=None) == INVAL and _bwd(L, 4097, stats=None) == INVAL
    assert _fwd(L, 505, D=64, stats=None, ld=7) == INVAL and _bwd(L, 505, stats=None, ws_bytes=0, ld=7) == INVAL


def test_token_limit_and_shape_predicate(built):
    from glow_tts_amd import _lib
    L = _lib.lib()
    for T in (505, 4097, 1, 384, 100000):                            # no generic fallback: the family is the feature
        assert L.gt_attn_long_shape(T, 96, 4) == 0
        assert _fwd(L, T) == UNSUPPORTED and _bwd(L, T) == UNSUPPORTED, T
    assert _fwd(L, 600, D=64) == UNSUPPORTED and _bwd(L, 600, D=64) == UNSUPPORTED
    assert _fwd(L, 600, win=3) == UNSUPPORTED and _bwd(L, 600, win=3) == UNSUPPORTED
    # ... before the workspace size and alignment
    assert _bwd(L, 4097, ws_bytes=0) == UNSUPPORTED and _bwd(L, 505, ws_bytes=0, ld=7) == UNSUPPORTED
    assert _fwd(L, 505, ld=7) == UNSUPPORTED and _fwd(L, 600, D=64, stats=FAKE + 4) == UNSUPPORTED


def test_workspace_size(built):
    from glow_tts_amd import _lib
    L = _lib.lib()
    for B, T in ((1, 506), (3, 1025), (32, 4096)):
        need = L.gt_attn_bwd_stats_workspace_bytes(B, T, 2)
        assert _bwd(L, T, B=B, ws_bytes=need - 1) == INVAL
        assert _bwd(L, T, B=B, ws_bytes=need - 1, ld=7) == INVAL     # ... before alignment
        assert _bwd(L, T, B=B, ws_bytes=need, ld=7) == ALIGN         # exactly enough: the next check is reached
        assert _bwd(L, T, B=B, ws_bytes=0) == INVAL


def test_alignment(built):
    from glow_tts_amd import _lib
    L = _lib.lib()
    C = 2 * 96
    assert _fwd(L, 506, ld=3 * C + 4) == ALIGN and _fwd(L, 506, ldo=C + 2) == ALIGN
    assert _fwd(L, 506, q=FAKE + 8) == ALIGN and _fwd(L, 506, stats=FAKE + 4) == ALIGN
    assert _bwd(L, 506, ld=3 * C + 4) == ALIGN and _bwd(L, 506, lddo=C + 4) == ALIGN and _bwd(L, 506, lddq=3 * C + 2) == ALIGN
    assert _bwd(L, 506, q=FAKE + 8) == ALIGN and _bwd(L, 506, ws=FAKE + 8) == ALIGN and _bwd(L, 506, stats=FAKE + 4) == ALIGN


def test_saved_p_backward_still_needs_its_p(built):
    from glow_tts_amd import _lib
    L = _lib.lib()
    for T in (100, 506, 4096):
        ws = L.gt_attn_bwd_workspace_bytes(1, T, 2)
        assert L.gt_attn_bwd(FAKE, FAKE, FAKE, 576, FAKE, FAKE, FAKE, FAKE, 192, None, FAKE, ws, FAKE, FAKE, FAKE, 576,
                             FAKE, FAKE, 1, T, T + 2, None, 2, 96, 4, 0.0, 0, None, None) == INVAL


def test_defaults_keep_p(built):
    from glow_tts_amd import attentions, ops
    assert ops.RowsConfig().attn_keep_p is True and ops.DEFAULT_ROWS.attn_keep_p is True
    assert attentions.MultiHeadAttention(192, 192, 2, window_size=4).keep_p is True


def test_mha_fwd_names_the_limit_before_it_touches_anything_with_stats(built):
    from glow_tts_amd import encoder_impl
    rc = types.SimpleNamespace(T=4097)                            # nothing else is read: no tensor, no module, no device
    with pytest.raises(ValueError, match="4096"):
        encoder_impl.mha_fwd(rc, None, None, 0.1, 0, keep_p="stats")


def test_trainer_takes_the_switch():
    import inspect
    from glow_tts_amd import train
    assert inspect.signature(train.Trainer.__init__).parameters["attn_keep_p"].default is None
