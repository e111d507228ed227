"""CPU tests of the contract the three neural vocoders meet (glow_tts_amd.audio._MelVocoder): what compile_synthesis
and workspace / workspace_bytes derive from it — mel_channels, wav_len, buffer_spec(B, F_max) as (name, dtype, elements), and the one
capacity refusal — on the tiny modules of the vocoders' own tests.  The closed forms are the ones tests/test_{hifigan,bigvgan,vocos}_host.py
state for the full-size shapes: (14 | 16 | 18) E + 4 B U F with E = B F W, and Vocos's."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bigvgan64 as G  # noqa: E402
import hifigan64 as H  # noqa: E402
import vocos64 as V  # noqa: E402

F32, BF16 = torch.float32, torch.bfloat16
W = 128                                            # max(C_0, max_i U_i C_i) of every tiny generator: 64 / 4 x 32 / 8 x 16 and 96 / 2 x 48 / 4 x 32
# name -> (constructor, arguments, mel_channels, samples per frame, frames lost, bytes per element of E over the streams, names and dtypes)
CASES = {
    "hifigan1": ("HiFiGAN", dict(H.TINY, resblock="1", n_mel_channels=16), 16, 8, 0, 14, [("u", F32), ("r", F32), ("s", F32), ("t", BF16)]),
    "hifigan2": ("HiFiGAN", dict(H.TINY, resblock="2", n_mel_channels=16), 16, 8, 0, 16, [("u", F32), ("r", F32), ("s", F32), ("t", F32)]),
    "bigvgan24": ("BigVGAN", dict(G.TINY24, resblock="1", n_mel_channels=16), 16, 4, 0, 18,
                  [("u", F32), ("r", F32), ("s", F32), ("t", F32), ("a", BF16)]),
    "bigvgan2": ("BigVGAN", dict(G.TINY, resblock="2", n_mel_channels=16), 16, 8, 0, 18,
                 [("u", F32), ("r", F32), ("s", F32), ("t", F32), ("a", BF16)]),
    "vocos": ("Vocos", dict(V.TINY), 80, 256, 1, None, [("x", F32), ("a", BF16), ("o", F32), ("spec", F32)]),
    "vocos100": ("Vocos", dict(V.TINY, input_channels=100), 112, 256, 1, None, [("x", F32), ("a", BF16), ("o", F32), ("spec", F32)]),
}


def make(case):
    from glow_tts_amd import audio
    kind, kw = CASES[case][:2]
    return getattr(audio, kind)(**kw)


@pytest.mark.parametrize("case", list(CASES))
def test_contract(built, case):
    from glow_tts_amd import _lib, audio
    _, _, n_mel, hop, lost, per_e, streams = CASES[case]
    voc = make(case)
    assert isinstance(voc, audio._MelVocoder) and voc.mel_channels == n_mel and voc.hop_length == hop and voc.min_frames == lost + 1
    assert [voc.wav_len(f) for f in (0, 1, 2)] == [0, hop * (1 - lost), hop * (2 - lost)] and voc.wav_len(70) == hop * (70 - lost)
    for B, F in ((3, 70), (1, 1)):
        if F < voc.min_frames:
            with pytest.raises(ValueError):
                voc.buffer_spec(B, F)
            with pytest.raises(ValueError):
                voc.workspace_bytes(B, F)
            continue
        spec = voc.buffer_spec(B, F)
        assert all(len(entry) == 3 and isinstance(entry[2], int) for entry in spec)
        assert [(name, dt) for name, dt, _ in spec] == streams
        if per_e is None:                                                           # Vocos: C = 128
            sizes = [B * F * 128, B * F * 128, B * F * 1026, _lib.lib().gt_gl_spec_bytes(B, F) // 4]
            closed = B * F * (6 * 128 + 4 * 1026) + _lib.lib().gt_gl_spec_bytes(B, F) + 4 * B * 256 * (F - 1)
        else:
            assert voc._width() == W
            sizes = [B * F * W] * len(streams)
            closed = per_e * B * F * W + 4 * B * hop * F
        assert [n for _, _, n in spec] == sizes
        derived = sum(n * torch.empty(0, dtype=dt).element_size() for _, dt, n in spec) + 4 * B * voc.wav_len(F)
        assert voc.workspace_bytes(B, F) == derived == closed


@pytest.mark.parametrize("case", list(CASES))
def test_capacity_past_2_31_is_refused(built, case):
    """the vocoder's own bound — B F_max W for the convolutional generators, B F_max 1026 for Vocos — at its first refused capacity and
    at the last one it takes; zero and negative capacities"""
    voc = make(case)
    per_frame = 1026 if CASES[case][5] is None else W
    F_first = -(-2 ** 31 // per_frame)                                              # the first F with 1 x F x per_frame >= 2^31
    assert (F_first - 1) * per_frame < 2 ** 31 <= F_first * per_frame
    assert len(voc.buffer_spec(1, F_first - 1)) == len(CASES[case][6])
    for B, F in ((1, F_first), (2, F_first // 2 + 1), (4096, 4096), (0, 70), (3, 0), (-1, 70)):
        with pytest.raises(ValueError, match="workspace for"):
            voc.buffer_spec(B, F)
        with pytest.raises(ValueError, match="workspace for"):
            voc.workspace(B, F, "cpu")                                              # refused before anything is allocated
        with pytest.raises(ValueError, match="workspace for"):
            voc.workspace_bytes(B, F)
