"""CPU tests of the fused DDSConv layer kernels (gt_dds_layer_fwd / gt_dds_layer_bwd, csrc/dds_layer.hip): the entries and their two
size functions, the refusal table of include/glowtts_hip.h entry by entry and in its order (NULL pointers, then the shape, then the
dropout probability, then strides / alignment), and the host-side switch.  Everything here is host code: every call returns before a
launch, so the FAKE pointers (as in tests/test_attn_stats_cabi.py) are never dereferenced."""
import pytest

FAKE = 0x1000           # non-null, 16-byte aligned, never dereferenced
INVAL, UNSUPPORTED, ALIGN = -1, -2, -3
C = 192

# positional arguments of the two entries, by name, with values that pass every check (so a test changes exactly one)
FWD = ["x", "ldx", "w_sep", "b_sep", "gamma1", "beta1", "w1x1", "Kp", "b1x1", "gamma2", "beta2", "utt", "rowmask", "a1", "lda", "h2", "out",
       "out3", "ldo3", "R", "C", "dilation", "eps", "drop_p", "seed", "seed_dev", "stream"]
BWD = ["x", "ldx", "w_sep", "b_sep", "gamma1", "beta1", "w1x1", "Kp", "gamma2", "beta2", "utt", "rowmask", "h2", "dy", "dh2", "lddh", "dh1",
       "dgamma2", "dbeta2", "dgamma1", "dbeta1", "partials", "R", "C", "dilation", "eps", "drop_p", "seed", "seed_dev", "stream"]
GOOD = dict(ldx=C, Kp=576, lda=3 * C, ldo3=3 * C, lddh=C, R=100, C=C, dilation=3, eps=1e-5, drop_p=0.5, seed=7, seed_dev=None, stream=None,
            out3=None, partials=None)
FWD_REQUIRED = ["x", "w_sep", "b_sep", "gamma1", "beta1", "w1x1", "b1x1", "gamma2", "beta2", "utt", "rowmask", "a1", "h2", "out"]
BWD_REQUIRED = ["x", "w_sep", "b_sep", "gamma1", "beta1", "w1x1", "gamma2", "beta2", "utt", "rowmask", "h2", "dy", "dh2", "dh1"]
BWD_GRADS = ["dgamma2", "dbeta2", "dgamma1", "dbeta1"]


def _call(L, which, **kw):
    names = FWD if which == "fwd" else BWD
    vals = [kw[n] if n in kw else GOOD.get(n, FAKE) for n in names]
    return getattr(L, "gt_dds_layer_" + which)(*vals)


@pytest.fixture()
def L(built):
    from glow_tts_amd import _lib
    return _lib.lib()


def test_entries_exist_and_are_mirrored(L):
    from glow_tts_amd import _lib
    for name in ("gt_dds_layer_fwd", "gt_dds_layer_bwd", "gt_dds_layer_partial_rows", "gt_dds_layer_tile_rows"):
        assert name in _lib.PROTOTYPES and hasattr(L, name), name
    assert len(_lib.PROTOTYPES["gt_dds_layer_fwd"][1]) == len(FWD) and len(_lib.PROTOTYPES["gt_dds_layer_bwd"][1]) == len(BWD)


def test_size_functions(L):
    T = L.gt_dds_layer_tile_rows()
    assert T == 64
    # two partial rows of 2 C floats per workgroup: [d gamma2 | d beta2] rows first, then the [d gamma1 | d beta1] rows
    for R, want in ((1, 2), (T - 1, 2), (T, 2), (T + 1, 4), (2 * T, 4), (2 * T + 1, 6), (17800, 2 * 279)):
        assert L.gt_dds_layer_partial_rows(R) == want == 2 * -(-R // T), R
    for R in (0, -1, -64, -(2 ** 31)):
        assert L.gt_dds_layer_partial_rows(R) == 0, R


def test_accepted_calls_reach_the_last_check(L):
    """The other direction of every refusal below: with nothing wrong but one stride, the call gets as far as the LAST check."""
    for d in (1, 3, 9, 27, 81):
        assert _call(L, "fwd", dilation=d, ldx=C - 1) == ALIGN and _call(L, "bwd", dilation=d, ldx=C - 1) == ALIGN
    assert _call(L, "fwd", drop_p=0.0, lda=3 * C - 1) == ALIGN and _call(L, "bwd", drop_p=0.0, lddh=C - 1) == ALIGN
    # the optional pointers: seed_dev, out_split3, and the four gradient pointers when there is a partials buffer
    assert _call(L, "fwd", out3=FAKE, seed_dev=FAKE, Kp=575) == ALIGN
    assert _call(L, "bwd", partials=FAKE, seed_dev=FAKE, Kp=575, **{g: None for g in BWD_GRADS}) == ALIGN


def test_null_pointers_come_first(L):
    for name in FWD_REQUIRED:
        assert _call(L, "fwd", **{name: None}) == INVAL, name
        # ... before the shape, the dropout probability and the strides
        assert _call(L, "fwd", **{name: None}, C=256, dilation=2, R=0, drop_p=1.0, ldx=1) == INVAL, name
    for name in BWD_REQUIRED:
        assert _call(L, "bwd", **{name: None}) == INVAL, name
        assert _call(L, "bwd", **{name: None}, C=256, dilation=2, R=0, drop_p=1.0, ldx=1) == INVAL, name
    for name in BWD_GRADS:                                   # required without a partials buffer, optional with one
        assert _call(L, "bwd", **{name: None}) == INVAL, name
        assert _call(L, "bwd", **{name: None}, C=256) == INVAL, name
        assert _call(L, "bwd", **{name: None}, partials=FAKE, C=256) == UNSUPPORTED, name


@pytest.mark.parametrize("which", ["fwd", "bwd"])
def test_shape_comes_second(L, which):
    for bad in (dict(C=191), dict(C=256), dict(C=0), dict(dilation=0), dict(dilation=-3), dict(dilation=2), dict(dilation=6), dict(dilation=10),
                dict(R=0), dict(R=-5)):
        assert _call(L, which, **bad) == UNSUPPORTED, bad
        # ... before the dropout probability and the strides / alignment
        assert _call(L, which, **bad, drop_p=1.0) == UNSUPPORTED, bad
        assert _call(L, which, **bad, ldx=1, Kp=100, w1x1=FAKE + 2) == UNSUPPORTED, bad


@pytest.mark.parametrize("which", ["fwd", "bwd"])
def test_dropout_probability_comes_third(L, which):
    for p in (-0.1, 1.0, 1.5, float("nan")):
        assert _call(L, which, drop_p=p) == INVAL, p
        assert _call(L, which, drop_p=p, ldx=1, Kp=100, w1x1=FAKE + 2) == INVAL, p            # ... before strides / alignment


def test_strides_and_alignment_come_last(L):
    for which in ("fwd", "bwd"):
        assert _call(L, which, ldx=C - 1) == ALIGN
        assert _call(L, which, Kp=3 * C - 8) == ALIGN and _call(L, which, Kp=3 * C + 4) == ALIGN
        assert _call(L, which, w1x1=FAKE + 8) == ALIGN and _call(L, which, w1x1=FAKE + 2) == ALIGN
    assert _call(L, "fwd", lda=3 * C - 1) == ALIGN
    assert _call(L, "fwd", out3=FAKE, ldo3=3 * C - 1) == ALIGN
    assert _call(L, "bwd", lddh=C - 1) == ALIGN


def test_switch_defaults_to_off_and_follows_the_setters(built):
    import torch
    from glow_tts_amd import _lib, models, predictors
    assert predictors.DDS_FUSED is False                        # GT_DDS_FUSED is unset in the test environment
    dds = predictors.DilatedDepthSeparableConv(192, 3, 3, 0.5)
    assert dds.fused is False
    assert dds.set_fused() is True and dds.fused is True
    assert dds.set_fused(False) is False and dds.fused is False
    sdp = predictors.StochasticDurationPredictor(192, 192, 3, 0.5, 4, gin_channels=16)
    all_dds = [m for m in sdp.modules() if isinstance(m, predictors.DilatedDepthSeparableConv)]
    assert len(all_dds) == 2 + 2 * 4 and not any(m.fused for m in all_dds)
    assert hasattr(models.FlowGenerator, "set_fused_predictors")
    # the method needs nothing of FlowGenerator but .modules(): it is tried on the predictor without building a whole model
    assert models.FlowGenerator.set_fused_predictors(sdp) == len(all_dds) and all(m.fused for m in all_dds)
    assert models.FlowGenerator.set_fused_predictors(sdp, False) == len(all_dds) and not any(m.fused for m in all_dds)
    # no quiet fall-back: a CPU tensor still raises, with the switch on as well as off
    for on in (False, True):
        dds.set_fused(on)
        with pytest.raises((_lib.CpuTensorError, RuntimeError, AttributeError, AssertionError)):
            dds(torch.zeros(1, 192, 8), torch.ones(1, 1, 8))
