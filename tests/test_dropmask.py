"""CPU self-checks of oracle/dropmask.py, the host restatement of the kernels' dropout hash (csrc/common.h:24-41)."""
import numpy as np
import pytest

from oracle import dropmask as D


def _hash_ref(x):
    """csrc/common.h hash_u32 written out on Python ints."""
    x &= 0xFFFFFFFF
    x ^= x >> 16; x = (x * 0x7feb352d) & 0xFFFFFFFF
    x ^= x >> 15; x = (x * 0x846ca68b) & 0xFFFFFFFF
    x ^= x >> 16
    return x


def test_hash_matches_hand_computed_values():
    assert int(D.hash_u32(0)) == 0
    # x = 1: x ^= x >> 16 -> 1; * 0x7feb352d; ^= >> 15 -> 0x7febcafb; * 0x846ca68b mod 2^32; ^= >> 16
    xs = [1, 2, 0x9E3779B1, 0xFFFFFFFF, 123456789]
    got = D.hash_u32(np.array(xs, dtype=np.uint32))
    assert got.dtype == np.uint32
    assert [int(v) for v in got] == [0x688990c0, 0xd1132181, 0x6d523710, 0x6768824a, 0xa8f1db88]
    assert [int(v) for v in got] == [_hash_ref(x) for x in xs]
    # the (seed, row, col) mix wraps mod 2^32
    s, r, c = 0xFFFFFFF0, 70000, 9000
    want = _hash_ref((s + r * 0x9E3779B1 + c * 0x85EBCA6B) & 0xFFFFFFFF)
    assert int(D.hash_u32(D._mix(s, r, c))) == want


def test_thresholds_follow_the_c_abi_fp32():
    # p reaches the launchers as a C float: (uint32)((double)(float)p * 2^32)
    assert D.thresh32(0.5) == 0x80000000
    assert D.thresh32(0.05) == int(float(np.float32(0.05)) * 2 ** 32)
    assert D.thresh16(0.05) == (D.thresh32(0.05) + 0x8000) >> 16 == 3277
    assert D.scale(0.1) == np.float32(1.0) / np.float32(0.9)


def _binomial_ok(keep, p):
    n = keep.size
    q = 1.0 - p
    return abs(keep.mean() - q) <= 5.0 * np.sqrt(p * q / n)


@pytest.mark.parametrize("p", [0.1, 0.5])
def test_keep_rate_within_binomial_bounds(p):
    rows = np.arange(4096)[:, None]
    cols = np.arange(192)[None, :]
    keep = D.drop_keep(D.word_seed(0x1234, 777), rows, cols, D.thresh32(p))
    assert _binomial_ok(keep, p), keep.mean()


def test_gate_keep_rate_16bit_within_binomial_bounds():
    p = 0.05
    rows = np.arange(4096)[:, None]
    kt, ks = D.drop_keep_gate(D.word_seed(0xBEEF, 4), rows, np.arange(192)[None, :], D.thresh16(p))
    assert _binomial_ok(kt, p) and _binomial_ok(ks, p), (kt.mean(), ks.mean())


def _uncorrelated(a, b):
    a, b = a.reshape(-1).astype(np.float64), b.reshape(-1).astype(np.float64)
    r = np.corrcoef(a, b)[0, 1]
    return abs(r) < 5.0 / np.sqrt(a.size), r


def test_pairs_that_must_not_correlate():
    rows = np.arange(2048)[:, None]
    cols = np.arange(192)[None, :]
    w, s = 0x5151, 40000
    # the tanh and sigmoid halves of one gate hash
    kt, ks = D.drop_keep_gate(D.word_seed(w, s), rows, cols, D.thresh16(0.5))
    ok, r = _uncorrelated(kt, ks)
    assert ok, r
    th = D.thresh32(0.5)
    # adjacent layer seeds s, s + 1
    ok, r = _uncorrelated(D.drop_keep(D.word_seed(w, s), rows, cols, th), D.drop_keep(D.word_seed(w, s + 1), rows, cols, th))
    assert ok, r
    # adjacent steps: word, word + 0x632BE5AB
    w2 = (w + D.SEED_INC) & 0xFFFFFFFF
    ok, r = _uncorrelated(D.drop_keep(D.word_seed(w, s), rows, cols, th), D.drop_keep(D.word_seed(w2, s), rows, cols, th))
    assert ok, r


def test_row_maps_follow_the_rows_layout():
    from glow_tts_amd import ops
    lens = [7, 3, 5]
    u = D.row_map(lens, 7)
    assert u.shape == (3, 7) and u[1, 0] == (7 + 2 * ops.HALO) + ops.HALO
    r = D.row_map(lens, 7, ragged=True, round_to=8)
    starts, R = ops.RowsCtx.row_starts(lens, 7, 8)
    assert list(r[:, 0]) == [s + ops.HALO for s in starts[:3]] and R % 8 == 0
    # valid frames own distinct rows in both layouts
    for m in (u, r):
        valid = np.concatenate([m[b, :n] for b, n in enumerate(lens)])
        assert len(set(valid.tolist())) == valid.size


def test_site_masks_are_distinct_within_one_step():
    lens = [11, 6]
    rows = D.row_map(lens, 11)
    word = 0x0BADCAFE
    te = D.text_encoder_masks(5, word, rows, 2, 11, n_layers=2)
    assert len(te) == 3 + 4 * 2
    a = te["encoder.encoder.drop:1"]                              # layer 0, FFN output (seed + 3)
    b = te["encoder.encoder.drop:2"]                              # layer 1, attention output
    assert not np.array_equal(a.numpy(), b.numpy())
    p0 = te["encoder.encoder.attn_layers.0.drop:0"]
    p1 = te["encoder.encoder.attn_layers.1.drop:0"]
    assert p0.shape == (2, 2, 11, 11) and not np.array_equal(p0.numpy(), p1.numpy())
    # every pair of same-shaped sites of this step differs
    keys = sorted(te)
    for i, k in enumerate(keys):
        for k2 in keys[i + 1:]:
            if te[k].shape == te[k2].shape:
                assert not np.array_equal(te[k].numpy(), te[k2].numpy()), (k, k2)
    dec = D.decoder_masks(3, word, D.row_map([6, 3], 6), n_blocks=2)
    assert len(dec) == 8
    vals = list(dec.values())
    assert all(not np.array_equal(vals[i].numpy(), vals[j].numpy()) for i in range(8) for j in range(i + 1, 8))
    # a step later (decoder seed moves, word moves) both change the masks
    assert not np.array_equal(D.decoder_masks(4, word, D.row_map([6, 3], 6), 2)["decoder.flows.2.wn.drop:0"].numpy(),
                              vals[0].numpy())
    w2 = (word + D.SEED_INC) & 0xFFFFFFFF
    assert not np.array_equal(D.decoder_masks(3, w2, D.row_map([6, 3], 6), 2)["decoder.flows.2.wn.drop:0"].numpy(),
                              vals[0].numpy())


def test_mask_values_are_keep_times_scale():
    rows = D.row_map([9], 9)
    m = D.channel_mask(17, 99, rows, 64, 0.1).numpy()
    assert set(np.unique(m).tolist()) <= {0.0, float(D.scale(0.1))}
    g = D.gate_mask(17, 99, rows, 32, 0.05).numpy()
    kt, ks = D.drop_keep_gate(D.word_seed(99, 17), rows[:, None, :], np.arange(32)[None, :, None], D.thresh16(0.05))
    assert np.array_equal(g[:, :32] > 0, kt) and np.array_equal(g[:, 32:] > 0, ks)
