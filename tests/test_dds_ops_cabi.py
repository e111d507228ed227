"""CPU tests of the host side of the five per-op DDSConv entries and gt_rows_split3 (csrc/predictor_ops.hip): the refusals of
include/glowtts_hip.h entry by entry, as the code has them.  GT_E_INVAL comes first (a required pointer NULL, R <= 0, dilation <= 0,
a row pitch below 3 C, a dropout probability outside [0, 1), a backward without `partials` and without a gradient pointer), then
GT_E_UNSUPPORTED for C != 192.  EVERY call here is refused: a refused call returns before its launch, so the FAKE pointers (as in
tests/test_dds_layer_cabi.py) are never dereferenced; that a call passes the GT_E_INVAL checks is shown by C = 256 coming back
GT_E_UNSUPPORTED."""
import pytest

FAKE = 0x1000           # non-null, 16-byte aligned, never dereferenced
INVAL, UNSUPPORTED = -1, -2
C = 192

# positional arguments by name; GOOD passes every check, so a test changes exactly what it is about
ARGS = {
    "gt_rows_split3": ["in", "ldi", "is_f32", "out", "ldo", "rowmask", "R", "C", "stream"],
    "gt_dds_sep_fwd": ["x", "ldx", "w", "b", "gamma", "beta", "utt", "rowmask", "a1", "lda", "R", "C", "dilation", "eps", "stream"],
    "gt_dds_out_fwd": ["h2", "x", "ldx", "gamma", "beta", "rowmask", "out", "out_bf16", "R", "C", "eps", "drop_p", "seed", "seed_dev", "stream"],
    "gt_dds_out_bwd": ["h2", "dy", "gamma", "beta", "rowmask", "dh2", "dgamma", "dbeta", "partials", "R", "C", "eps", "drop_p", "seed", "seed_dev",
                       "stream"],
    "gt_dds_sep_bwd": ["x", "ldx", "w", "b", "gamma", "beta", "utt", "rowmask", "da1", "dh1", "dgamma", "dbeta", "partials", "R", "C", "dilation",
                       "eps", "stream"],
    "gt_dds_dw_bwd": ["x", "ldx", "dh1", "dy", "w", "utt", "rowmask", "dx", "dw", "db", "partials", "R", "C", "dilation", "stream"],
}
GOOD = dict(ldi=C, is_f32=1, ldo=3 * C, ldx=C, lda=3 * C, R=100, C=C, dilation=3, eps=1e-5, drop_p=0.5, seed=7, seed_dev=None, stream=None,
            partials=None, out_bf16=None)
REQUIRED = {
    "gt_rows_split3": ["in", "out"],
    "gt_dds_sep_fwd": ["x", "w", "b", "gamma", "beta", "utt", "rowmask", "a1"],
    "gt_dds_out_fwd": ["h2", "x", "gamma", "beta", "rowmask", "out"],
    "gt_dds_out_bwd": ["h2", "dy", "gamma", "beta", "rowmask", "dh2"],
    "gt_dds_sep_bwd": ["x", "w", "b", "gamma", "beta", "utt", "rowmask", "da1", "dh1"],
    "gt_dds_dw_bwd": ["x", "dh1", "dy", "w", "utt", "rowmask", "dx"],
}
GRADS = {"gt_dds_out_bwd": ["dgamma", "dbeta"], "gt_dds_sep_bwd": ["dgamma", "dbeta"], "gt_dds_dw_bwd": ["dw", "db"]}
DDS = [e for e in ARGS if e != "gt_rows_split3"]
DILATED = ["gt_dds_sep_fwd", "gt_dds_sep_bwd", "gt_dds_dw_bwd"]
DROPPING = ["gt_dds_out_fwd", "gt_dds_out_bwd"]


@pytest.fixture()
def L(built):
    from glow_tts_amd import _lib
    return _lib.lib()


def _call(L, entry, **kw):
    assert set(kw) <= set(ARGS[entry]), (entry, kw)
    return getattr(L, entry)(*[kw[n] if n in kw else GOOD.get(n, FAKE) for n in ARGS[entry]])


def test_entries_are_mirrored_with_these_arguments(L):
    from glow_tts_amd import _lib
    for entry, names in ARGS.items():
        assert entry in _lib.PROTOTYPES and hasattr(L, entry), entry
        assert len(_lib.PROTOTYPES[entry][1]) == len(names), entry
    assert "gt_dds_bwd_partial_rows" in _lib.PROTOTYPES


def test_partial_rows_is_one_row_per_eight(L):
    for R, want in ((1, 1), (7, 1), (8, 1), (9, 2), (33, 5), (70, 9), (17800, 2225)):
        assert L.gt_dds_bwd_partial_rows(R) == want == -(-R // 8), R
    for R in (0, -1, -8, -(2 ** 31)):
        assert L.gt_dds_bwd_partial_rows(R) == 0, R


@pytest.mark.parametrize("entry", list(ARGS))
def test_a_required_null_pointer_is_invalid(L, entry):
    wide = {k: 3 * 256 for k in ("ldo", "lda") if k in ARGS[entry]}
    for name in REQUIRED[entry]:
        assert _call(L, entry, **{name: None}) == INVAL, name
        assert _call(L, entry, **{name: None}, C=256, **wide) == INVAL, name               # ... before the channel count is looked at


@pytest.mark.parametrize("entry", list(ARGS))
def test_no_rows_is_invalid(L, entry):
    for R in (0, -1, -(2 ** 31)):
        assert _call(L, entry, R=R) == INVAL, R


@pytest.mark.parametrize("entry", DILATED)
def test_a_dilation_below_one_is_invalid(L, entry):
    for d in (0, -1, -3):
        assert _call(L, entry, dilation=d) == INVAL, d
        assert _call(L, entry, dilation=d, C=64) == INVAL, d


def test_a_row_pitch_below_3c_is_invalid(L):
    assert _call(L, "gt_dds_sep_fwd", lda=3 * C - 1) == INVAL and _call(L, "gt_dds_sep_fwd", lda=0) == INVAL
    assert _call(L, "gt_rows_split3", ldo=3 * C - 1) == INVAL and _call(L, "gt_rows_split3", ldo=C) == INVAL
    assert _call(L, "gt_rows_split3", C=37, ldo=110) == INVAL                       # any C: 3 * 37 = 111
    assert _call(L, "gt_rows_split3", C=0) == INVAL and _call(L, "gt_rows_split3", C=-192) == INVAL


@pytest.mark.parametrize("entry", DROPPING)
def test_a_dropout_probability_outside_0_1_is_invalid(L, entry):
    for p in (-0.1, -1e-9, 1.0, 1.5, float("inf"), float("-inf")):
        assert _call(L, entry, drop_p=p) == INVAL, p
        assert _call(L, entry, drop_p=p, C=256) == INVAL, p


@pytest.mark.parametrize("entry", DDS)
def test_another_channel_count_is_unsupported_after_the_invalid_checks(L, entry):
    kw = dict(lda=3 * 256) if entry == "gt_dds_sep_fwd" else {}
    for bad in (191, 193, 256, 64):
        assert _call(L, entry, C=bad, **kw) == UNSUPPORTED, bad
    # the optional pointers may be NULL or set; every other dilation and every probability in [0, 1) passes the invalid checks
    opt = {"gt_dds_out_fwd": dict(out_bf16=FAKE, seed_dev=FAKE), "gt_dds_out_bwd": dict(seed_dev=FAKE)}.get(entry, {})
    assert _call(L, entry, C=256, **kw, **opt) == UNSUPPORTED
    if entry in DILATED:
        for d in (1, 2, 9, 27, 1000):
            assert _call(L, entry, C=256, dilation=d, **kw) == UNSUPPORTED, d
    if entry in DROPPING:
        for p in (0.0, 0.05, 0.999):
            assert _call(L, entry, C=256, drop_p=p) == UNSUPPORTED, p
    if entry == "gt_dds_sep_fwd":
        assert _call(L, entry, C=256, lda=3 * 256 + 8) == UNSUPPORTED
    # an x pitch is not checked by these entries
    if "ldx" in ARGS[entry]:
        assert _call(L, entry, C=256, ldx=1, **kw) == UNSUPPORTED


@pytest.mark.parametrize("entry", list(GRADS))
def test_a_backward_needs_its_gradient_pointers_or_a_partials_buffer(L, entry):
    a, b = GRADS[entry]
    for missing in ({a: None}, {b: None}, {a: None, b: None}):
        assert _call(L, entry, **missing) == INVAL, missing
        assert _call(L, entry, **missing, C=256) == INVAL, missing
        # with a partials buffer the gradient pointers may be NULL: the call gets as far as the channel count
        assert _call(L, entry, **missing, partials=FAKE, C=256) == UNSUPPORTED, missing
    assert _call(L, entry, partials=FAKE, C=256) == UNSUPPORTED
    for name in REQUIRED[entry]:                                 # ... and a partials buffer excuses nothing else
        assert _call(L, entry, **{name: None}, partials=FAKE, **{a: None, b: None}) == INVAL, name
