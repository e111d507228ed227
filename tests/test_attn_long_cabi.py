"""CPU tests of the long-text attention dispatch (csrc/attn_long.hip behind gt_attn_fwd / gt_attn_bwd): the shape predicate, the
token limit of both entries and of encoder_impl.mha_fwd are host code and run without a GPU; no kernel is launched."""
import os
import re
import types

import pytest

FAKE = 0x1000           # a non-null, 16-byte aligned address that is never dereferenced: every call below returns before a launch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_long_shape_predicate(built):
    from glow_tts_amd import _lib
    L = _lib.lib()
    assert L.gt_attn_long_shape(506, 96, 4) == 1 and L.gt_attn_long_shape(4096, 96, 4) == 1
    assert L.gt_attn_long_shape(505, 96, 4) == 0 and L.gt_attn_long_shape(4097, 96, 4) == 0
    assert L.gt_attn_long_shape(600, 64, 4) == 0 and L.gt_attn_long_shape(600, 96, 3) == 0


def test_mfma_shape_predicate_is_unchanged(built):
    from glow_tts_amd import _lib
    L = _lib.lib()
    assert L.gt_attn_mfma_shape(384, 96, 4) == 1 and L.gt_attn_mfma_shape(385, 96, 4) == 0
    assert L.gt_attn_mfma_shape(506, 96, 4) == 0                  # the two families are told apart by their own predicates


def _fwd(L, T, D=96, win=4, B=1, H=2):
    return L.gt_attn_fwd(FAKE, FAKE, FAKE, 3 * H * D, FAKE, FAKE, FAKE, FAKE, H * D, FAKE, B, T, T + 2, None, H, D, win, 0.0, 0, None, None)


def _bwd(L, T, D=96, win=4, B=1, H=2, ws_bytes=None):
    ws_bytes = L.gt_attn_bwd_workspace_bytes(B, T, H) if ws_bytes is None else ws_bytes
    return L.gt_attn_bwd(FAKE, FAKE, FAKE, 3 * H * D, FAKE, FAKE, FAKE, FAKE, H * D, FAKE, FAKE, ws_bytes, FAKE, FAKE, FAKE, 3 * H * D,
                         FAKE, FAKE, B, T, T + 2, None, H, D, win, 0.0, 0, None, None)


def test_past_the_token_limit_both_entries_refuse_before_any_launch(built):
    from glow_tts_amd import _lib
    L = _lib.lib()
    assert _fwd(L, 4097) == -2 and _bwd(L, 4097) == -2
    assert _bwd(L, 4097, ws_bytes=0) == -2                        # unsupported whatever workspace is offered
    assert _fwd(L, 4097, D=64) == -2 and _bwd(L, 4097, D=64) == -2
    assert _fwd(L, 100000) == -2 and _bwd(L, 100000) == -2


def test_the_limit_is_the_headers_macro_and_the_mas_token_limit(built):
    from glow_tts_amd import encoder_impl
    with open(os.path.join(ROOT, "include", "glowtts_hip.h")) as f:
        hdr = f.read()
    lim = int(re.search(r"#define\s+GT_ATTN_LONG_MAX_T\s+(\d+)", hdr).group(1))
    assert lim == 4096 == int(re.search(r"#define\s+GT_MAS_LONG_MAX_TX\s+(\d+)", hdr).group(1))
    assert encoder_impl.ATTN_MAX_T == lim


def test_mha_fwd_names_the_limit_before_it_touches_anything(built):
    from glow_tts_amd import encoder_impl
    rc = types.SimpleNamespace(T=4097)                            # nothing else is read: no tensor, no module, no device
    with pytest.raises(ValueError, match="4096"):
        encoder_impl.mha_fwd(rc, None, None, 0.1, 0)
