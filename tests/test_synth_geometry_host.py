"""CPU tests of the host restatement of gt_synth_geometry (tests/synth_geometry_host.py): on lengths that fit it IS
ops.RowsCtx.row_starts with starts[B] = R_cap; on lengths that do not, the layout stays inside R_cap with every utterance's halos
kept, and the status bits follow their definitions."""
import os
import random
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import synth_geometry_host as G  # noqa: E402

HALO = 2


def row_starts(lens_sq, T, rnd):
    from glow_tts_amd import ops
    assert ops.HALO == HALO
    return ops.RowsCtx.row_starts(lens_sq, T, rnd)


def test_lengths_that_fit_give_row_starts():
    rng = random.Random(5)
    for _ in range(200):
        B = rng.choice([1, 2, 3, 7, 32, 65])
        Ty_cap = 2 * rng.randint(1, 400)
        y_len = [rng.randint(1, Ty_cap) for _ in range(B)]
        rnd = rng.choice([8, 128, 512])
        starts, R = row_starts([v // 2 for v in y_len], Ty_cap // 2, rnd)
        R_cap = R + rnd * rng.randint(0, 2)                              # exactly the rounded size, or spare capacity behind it
        starts[-1] = R_cap
        g = G.geometry(y_len, Ty_cap, R_cap)
        assert g["status"] == 0
        assert g["row0"] == starts
        assert g["len_sq"] == [v // 2 for v in y_len] and g["y_len_eff"] == y_len
        # the tables: what gt_rows_ctx_fill computes from these offsets
        for m in (0, 1, HALO, R_cap // 2, R_cap - 1):
            b = max(i for i in range(B) if starts[i] <= m)
            t = m - starts[b] - HALO
            assert (g["rowbatch"][m], g["rowframe"][m]) == (b, t)
            assert g["rowmask"][m] == (1.0 if 0 <= t < y_len[b] // 2 else 0.0)


def test_lengths_that_do_not_fit_stay_inside_the_capacity():
    rng = random.Random(6)
    seen = set()
    for _ in range(300):
        B = rng.choice([1, 2, 3, 7, 32])
        Ty_cap = 2 * rng.randint(1, 200)
        y_len = [rng.randint(1, Ty_cap + (rng.random() < 0.3) * 50) for _ in range(B)]
        need = sum(min(v, Ty_cap) // 2 + 2 * HALO for v in y_len)
        R_cap = max(2 * HALO * B, need - rng.choice([0, 0, 1, 2, 17, need // 2, need]))
        g = G.geometry(y_len, Ty_cap, R_cap)
        row0, len_sq = g["row0"], g["len_sq"]
        assert g["status"] & G.BIT_FRAMES == (G.BIT_FRAMES if any(v > Ty_cap for v in y_len) else 0)
        assert g["status"] & G.BIT_ROWS == (G.BIT_ROWS if need > R_cap else 0)
        seen.add(g["status"])
        assert row0[0] == 0 and row0[B] == R_cap
        assert all(row0[b] <= row0[b + 1] for b in range(B)) and all(v <= R_cap for v in row0)
        assert all(0 <= len_sq[b] <= min(y_len[b], Ty_cap) // 2 for b in range(B))
        assert all(len_sq[b] + 2 * HALO <= row0[b + 1] - row0[b] for b in range(B))
        assert all(g["y_len_eff"][b] // 2 == len_sq[b] and g["y_len_eff"][b] <= min(y_len[b], Ty_cap) for b in range(B))
        assert len(g["rowmask"]) == R_cap and sum(g["rowmask"]) == sum(len_sq)
        if not g["status"] & G.BIT_ROWS:
            assert len_sq == [min(v, Ty_cap) // 2 for v in y_len]
        else:                                                            # utterances in order: behind the first cut nothing is longer than its wish
            cut = next(b for b in range(B) if len_sq[b] < min(y_len[b], Ty_cap) // 2)
            assert len_sq[:cut] == [min(v, Ty_cap) // 2 for v in y_len[:cut]]
            assert all(v == 0 for v in len_sq[cut + 1:])
    assert seen == {0, 1, 2, 3}


def test_the_named_cases():
    # exactly R_cap rows / one row more (the cut falls in the last utterance) / a cut in the middle, later utterances get 0
    y_len = [40, 1, 33, 40]                                                # squeezed 20, 0, 16, 20 -> 56 + 16 = 72 rows
    assert G.geometry(y_len, 40, 72)["status"] == 0
    g = G.geometry(y_len, 40, 71)
    assert g["status"] == G.BIT_ROWS and g["len_sq"] == [20, 0, 16, 19] and g["y_len_eff"] == [40, 1, 33, 38]
    g = G.geometry(y_len, 40, 40)
    assert g["status"] == G.BIT_ROWS and g["len_sq"] == [20, 0, 4, 0] and g["row0"] == [0, 24, 28, 36, 40]
    g = G.geometry([41, 40], 40, 128)
    assert g["status"] == G.BIT_FRAMES and g["len_sq"] == [20, 20] and g["y_len_eff"] == [40, 40] and g["row0"] == [0, 24, 128]
