"""CPU tests of the HiFi-GAN vocoder's host side (glow_tts_amd.audio.HiFiGAN): the transposed-convolution identity the
kernel path rests on, state-dict loading in both checkpoint forms, the constructor's refusals, the weight image's layout, and the two
independent float64 writings of the definition (tests/hifigan64.py) against each other."""
import os
import sys

import numpy as np
import pytest
import torch
from torch.nn import functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hifigan64 as H  # noqa: E402


@pytest.mark.parametrize("u,k", [(8, 16), (4, 8), (2, 4)])
def test_transposed_conv_is_a_three_tap_conv(u, k):
    """conv_transpose1d(x, w, b, stride u, padding u / 2) == the 3-tap convolution with transposed_as_conv's weights, its [L, u Cout]
    output read as [u L, Cout]: float64, to 1e-13, at lengths 1, 2 and 9"""
    from glow_tts_amd import audio
    g = torch.Generator().manual_seed(u)
    Cin, Cout = 6, 5
    w = torch.randn(Cin, Cout, k, dtype=torch.float64, generator=g)
    b = torch.randn(Cout, dtype=torch.float64, generator=g)
    W3 = audio.transposed_as_conv(w, u)
    assert W3.shape == (u * Cout, Cin, 3)
    for L in (1, 2, 9):
        x = torch.randn(1, Cin, L, dtype=torch.float64, generator=g)
        ref = F.conv_transpose1d(x, w, b, stride=u, padding=(k - u) // 2)[0]                 # [Cout, u L]
        y = F.conv1d(x, W3, b.repeat(u), padding=1)[0]                                       # [u Cout, L]
        got = y.t().reshape(L * u, Cout).t()
        assert ref.shape == got.shape == (Cout, u * L)
        assert float((got - ref).abs().max()) <= 1e-13
    with pytest.raises(ValueError):
        audio.transposed_as_conv(torch.zeros(2, 2, 7), 3)


@pytest.mark.parametrize("resblock", ["1", "2"])
def test_state_dict_loading_in_both_forms(resblock):
    """a weight-normed torch generator's state dict (weight_g / weight_v), wrapped in {"generator": ...} or bare, and the same after
    remove_weight_norm: equal key sets, folded weights equal to fp32 rounding"""
    from glow_tts_amd import audio
    torch.manual_seed(3)
    ref = H.TorchGenerator(H.TINY, resblock, weight_norm=True)
    with torch.no_grad():
        for n, p in ref.named_parameters():
            if n.endswith("weight_g"):
                p.mul_(torch.rand_like(p) + 0.5)                                             # g != ||v||: the fold is not the identity
    normed = {k: v.clone() for k, v in ref.state_dict().items()}
    assert any(k.endswith("weight_g") for k in normed)
    voc = audio.HiFiGAN(resblock=resblock, **H.TINY)
    voc.load_generator_state({"generator": normed})
    folded = {k: v.clone() for k, v in voc.state_dict().items()}
    plain = {k: v.clone() for k, v in ref.remove_weight_norm().state_dict().items()}
    assert set(folded) == set(plain) and not any("weight_g" in k or "weight_v" in k for k in plain)
    for k in plain:
        assert folded[k].dtype == torch.float32 and folded[k].shape == plain[k].shape, k
        if k.endswith(".bias"):
            assert torch.equal(folded[k], plain[k]), k
        else:
            v64, g64 = normed[k + "_v"].double(), normed[k + "_g"].double()
            w64 = g64 * v64 / v64.reshape(v64.shape[0], -1).norm(dim=1).reshape(-1, 1, 1)
            assert torch.equal(folded[k], w64.float()), k                                     # float64 fold, rounded once
            assert float((folded[k] - plain[k]).abs().max()) <= 2.0 ** -22 * float(plain[k].abs().max()), k
    voc2 = audio.HiFiGAN(resblock=resblock, **H.TINY)
    voc2.load_generator_state(plain)
    voc3 = audio.HiFiGAN(resblock=resblock, **H.TINY)
    voc3.load_generator_state(normed)
    for k in plain:
        assert torch.equal(voc2.state_dict()[k], plain[k]) and torch.equal(voc3.state_dict()[k], folded[k]), k
    with pytest.raises(RuntimeError):
        voc.load_generator_state({k: v for k, v in plain.items() if k != "conv_post.bias"})


def test_from_config_and_v1_shape():
    from glow_tts_amd import audio
    cfg = dict(resblock="1", upsample_rates=[8, 8, 2, 2], upsample_kernel_sizes=[16, 16, 4, 4], upsample_initial_channel=512,
               resblock_kernel_sizes=[3, 7, 11], resblock_dilation_sizes=[[1, 3, 5], [1, 3, 5], [1, 3, 5]], num_mels=80, sampling_rate=22050)
    voc = audio.HiFiGAN.from_config(cfg)
    assert sum(p.numel() for p in voc.parameters()) == 13926017
    assert voc.launches == 78 and voc.hop_length == 256 and voc.channels == [512, 256, 128, 64, 32]
    assert voc.workspace_bytes(32, 800) == 14 * 32 * 800 * 8192 + 4 * 32 * 256 * 800
    assert set(voc.state_dict()) == set(H.TorchGenerator(H.V1).state_dict())
    v2 = audio.HiFiGAN(resblock="2", upsample_rates=(8, 8, 4), upsample_kernel_sizes=(16, 16, 8), upsample_initial_channel=256,
                       resblock_kernel_sizes=(3, 5, 7), resblock_dilation_sizes=((1, 2), (2, 6), (3, 12)))
    assert v2.launches == 2 + 3 * (1 + 6) and v2.hop_length == 256


@pytest.mark.parametrize("kw", [
    dict(upsample_rates=(4, 2), upsample_kernel_sizes=(8, 5)),                               # k != 2u
    dict(upsample_rates=(3, 2), upsample_kernel_sizes=(6, 4)),                               # odd u
    dict(upsample_rates=(4, 2), upsample_kernel_sizes=(8, 4), upsample_initial_channel=96),  # 96 -> 48 -> 24: not a multiple of 16
    dict(upsample_rates=(4, 2), upsample_kernel_sizes=(8, 4), upsample_initial_channel=72),
    dict(n_mel_channels=81),
    dict(resblock_kernel_sizes=(3, 6, 11)),                                                  # even
    dict(resblock_kernel_sizes=(3, 7, 13)),                                                  # > 11
    dict(resblock="3"),
    dict(upsample_rates=(4, 2), upsample_kernel_sizes=(8,)),
])
def test_constructor_refusals(kw):
    from glow_tts_amd import audio
    args = dict(H.TINY)
    args.update(kw)
    with pytest.raises(ValueError):
        audio.HiFiGAN(**args)


def test_weight_image_layout(built):
    """voc_pack against the header's index formula (hifigan64.decode_image), zeros in the padding"""
    from glow_tts_amd import _lib, audio
    L = _lib.lib()
    assert L.gt_voc_k_chunk(64) == 64 and L.gt_voc_k_chunk(128) == 64 and L.gt_voc_k_chunk(80) == 32 and L.gt_voc_k_chunk(16) == 32
    assert L.gt_voc_k_chunk(0) == 0 and L.gt_voc_k_chunk(24) == 0
    g = torch.Generator().manual_seed(5)
    for N, Cin, taps in ((1, 32, 7), (40, 80, 3), (64, 64, 11), (160, 128, 1)):
        w = torch.randn(N, Cin, taps, generator=g)
        img = audio.voc_pack(w)
        kc = L.gt_voc_k_chunk(Cin)
        W = H.decode_image(img, N, Cin, taps, kc)
        assert np.array_equal(W, w.to(torch.bfloat16).double().numpy().transpose(2, 0, 1))


@pytest.mark.parametrize("resblock", ["1", "2"])
def test_float64_generator_against_a_batched_torch_generator(resblock):
    """the helper's channels-last generator (explicit taps, scatter-form transposed convolution) against torch's conv1d /
    conv_transpose1d in float64 on ONE utterance: two independent writings of the definition"""
    torch.manual_seed(11)
    ref = H.TorchGenerator(H.TINY, resblock).double()
    rng = np.random.default_rng(2)
    for frames in (1, 2, 23):
        mel = H.random_mel(rng, 80, frames)
        want = ref(torch.from_numpy(mel).double()[None])[0, 0].detach().numpy()
        got = H.generator64(ref.state_dict(), H.TINY, mel, resblock)
        assert got.shape == want.shape == (8 * frames,)
        assert float(np.abs(got - want).max()) <= 1e-12
    assert H.generator64(ref.state_dict(), H.TINY, np.zeros((80, 0), dtype=np.float32), resblock).shape == (0,)
    # the emulation is the same network with rounded operands: close, and not equal
    e = H.rel_l2(H.generator64(ref.state_dict(), H.TINY, mel, resblock, emul=True), want)
    assert 0 < e < 0.05
