"""CPU tests of the BigVGAN vocoder's host side (glow_tts_amd.audio.BigVGAN): the filter, the two float64 writings of
Activation1d (tests/bigvgan64.py) against each other, the halo of the closed form, the float64 generator against the torch one, the
published parameter tree, both checkpoint forms, the constructor's refusals and the host padding of a 24-channel stage."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bigvgan64 as G  # noqa: E402
import hifigan64 as H  # noqa: E402

LENGTHS = (1, 2, 3, 5, 6, 7, 11, 12, 13, 40)


def test_filter_values():
    from glow_tts_amd import audio
    f = G.filter64()
    want = np.array(G.FILTER + G.FILTER[::-1])
    assert f.shape == (12,) and float(np.abs(f - want).max()) <= 1e-15
    assert float(np.abs(f - f[::-1]).max()) <= 1e-16 and abs(f.sum() - 1) <= 1e-15 and abs(np.abs(f).sum() - 1.3328) < 1e-4
    assert float(np.abs(audio.kaiser_sinc_filter64() - f).max()) <= 1e-15         # the module's own builder: numpy's Kaiser window
    act = audio._Activation1d(4, "snake", True)
    for buf in (act.upsample.filter, act.downsample.lowpass.filter):
        assert buf.shape == (1, 1, 12) and torch.equal(buf.reshape(-1), torch.from_numpy(f).float())


@pytest.mark.parametrize("L", LENGTHS)
def test_two_writings_of_the_activation_agree(L):
    rng = np.random.default_rng(L)
    C = 3
    x = rng.uniform(-10, 10, (L, C))
    a, ib = rng.uniform(0.1, 7, C), 1 / (rng.uniform(0.1, 7, C) + 1e-9)
    y_torch = G.act64_torch(x, a, ib)
    y, bound = G.act64(x, a, ib)
    assert y.shape == y_torch.shape == (L, C) and float(np.abs(y - y_torch).max()) <= 1e-12
    assert (bound > 0).all() and float(bound.max()) < 2e-2                      # far below the values' own scale of 10
    # the planted defects are other functions: past the end from a clamped x, and a clamp at an inner edge
    if L >= 2:                                                                      # L = 1: a constant, on which both agree
        assert float(np.abs(G.act64(x, a, ib, defect="v_past_end")[0] - y).max()) > 1e-3
    if L >= 12:
        bad = G.act64(x, a, ib, defect="tile_clamp", edge=L // 2)[0]
        assert np.array_equal(bad[:L // 2], y[:L // 2]) and float(np.abs(bad - y).max()) > 1e-3


def test_halo_is_five_positions():
    rng = np.random.default_rng(7)
    L, t = 40, 20
    x = rng.standard_normal((L, 2))
    a, ib = np.array([1.3, 0.4]), np.array([0.7, 2.0])
    y = G.act64(x, a, ib)[0]
    for d in (-6, 6):
        x2 = x.copy()
        x2[t + d] += 1.0
        assert np.array_equal(G.act64(x2, a, ib)[0][t], y[t]), d
    for d in (-5, 5):
        x2 = x.copy()
        x2[t + d] += 1.0
        assert float(np.abs(G.act64(x2, a, ib)[0][t] - y[t]).min()) > 0, d


@pytest.mark.parametrize("resblock,activation,logscale,tanh", [("1", "snakebeta", True, True), ("2", "snake", True, True),
                                                               ("1", "snake", False, False)])
def test_float64_generator_against_the_torch_generator(resblock, activation, logscale, tanh):
    kw = dict(resblock=resblock, activation=activation, snake_logscale=logscale, use_tanh_at_final=tanh, use_bias_at_final=tanh)
    ref = G.seeded(G.TINY, 11, alpha_range=(-1.0, 1.0) if logscale else (0.2, 2.0), **kw).double()
    rng = np.random.default_rng(2)
    cfg = dict(G.TINY, **kw)
    for frames in (1, 2, 23):
        mel = G.random_mel(rng, 16, frames)
        want = ref(torch.from_numpy(mel).double()[None])[0, 0].detach().numpy()
        got = G.generator64(ref.state_dict(), cfg, mel)
        assert got.shape == want.shape == (8 * frames,)
        assert float(np.abs(got - want).max()) <= 1e-10
    assert G.generator64(ref.state_dict(), cfg, np.zeros((16, 0), dtype=np.float32)).shape == (0,)
    e = G.rel_l2(G.generator64(ref.state_dict(), cfg, mel, emul=True), want)
    assert 0 < e < 0.05


@pytest.mark.parametrize("resblock", ["1", "2"])
@pytest.mark.parametrize("activation", ["snake", "snakebeta"])
def test_parameter_tree_has_the_published_names(resblock, activation):
    from glow_tts_amd import audio
    ref = G.TorchBigVGAN(G.TINY, resblock, n_mel=16, activation=activation)
    voc = audio.BigVGAN(resblock=resblock, n_mel_channels=16, activation=activation, **G.TINY)
    want, got = ref.state_dict(), voc.state_dict()
    assert list(got) == list(want) or set(got) == set(want)
    for k in want:
        assert got[k].shape == want[k].shape and got[k].dtype == torch.float32, k
    assert ("resblocks.0.activations.0.act.beta" in got) == (activation == "snakebeta")
    assert "ups.0.0.weight" in got and "activation_post.downsample.lowpass.filter" in got
    assert isinstance(voc, audio.HiFiGAN)
    n_act = len(G.TINY["upsample_rates"]) * 3 * (6 if resblock == "1" else 3) + 1
    assert voc.snake_launches == n_act and voc.launches == voc.conv_launches + n_act


def test_state_dict_loading_in_both_forms():
    from glow_tts_amd import audio
    ref = G.seeded(G.TINY, 3, weight_norm=True)
    with torch.no_grad():
        for n, p in ref.named_parameters():
            if n.endswith("weight_g"):
                p.mul_(torch.rand_like(p) + 0.5)
    normed = {k: v.clone() for k, v in ref.state_dict().items()}
    assert any(k.endswith("weight_g") for k in normed)
    voc = audio.BigVGAN(n_mel_channels=16, **G.TINY)
    voc.load_generator_state({"generator": normed})
    folded = {k: v.clone() for k, v in voc.state_dict().items()}
    plain = {k: v.clone() for k, v in ref.remove_weight_norm().state_dict().items()}
    assert set(folded) == set(plain)
    for k in plain:
        if k.endswith(".weight"):
            assert float((folded[k] - plain[k]).abs().max()) <= 2.0 ** -22 * float(plain[k].abs().max()), k
        else:
            assert torch.equal(folded[k], plain[k]), k                             # biases, alpha, beta, filters
    voc2 = audio.BigVGAN(n_mel_channels=16, **G.TINY)
    voc2.load_generator_state(plain)
    for k in plain:
        assert torch.equal(voc2.state_dict()[k], plain[k]), k
    with pytest.raises(RuntimeError):
        voc.load_generator_state({k: v for k, v in plain.items() if k != "activation_post.act.alpha"})
    with pytest.raises(RuntimeError):
        audio.BigVGAN(n_mel_channels=16, activation="snake", **G.TINY).load_generator_state(plain)   # an unexpected act.beta


def test_from_config_on_the_published_base_config():
    from glow_tts_amd import audio
    voc = audio.BigVGAN.from_config(dict(G.BASE_CONFIG, sampling_rate=22050))
    ref = G.TorchBigVGAN(G.BASE)
    assert sum(p.numel() for p in voc.parameters()) == sum(p.numel() for p in ref.parameters())
    assert set(voc.state_dict()) == set(ref.state_dict())
    assert voc.conv_launches == 78 and voc.snake_launches == 73 and voc.launches == 151 and voc.hop_length == 256
    assert voc.activation == "snakebeta" and voc.snake_logscale and voc.use_tanh_at_final and voc.use_bias_at_final
    assert voc.workspace_bytes(32, 800) == 18 * 32 * 800 * 8192 + 4 * 32 * 256 * 800
    assert voc.t_dtype == torch.float32
    E = 32 * 800 * 8192
    assert voc.buffer_spec(32, 800) == [("u", torch.float32, E), ("r", torch.float32, E), ("s", torch.float32, E), ("t", torch.float32, E),
                                        ("a", torch.bfloat16, E)]
    big = audio.BigVGAN.from_config(dict(G.BASE_CONFIG, upsample_rates=[4, 4, 2, 2, 2, 2], upsample_kernel_sizes=[8, 8, 4, 4, 4, 4],
                                         upsample_initial_channel=1536, use_tanh_at_final=False, use_bias_at_final=False))
    assert big.channels[-1] == 24 and big.padded_channels[-1] == 32 and big.conv_post.bias is None and not big.use_tanh_at_final
    hv1 = audio.HiFiGAN(**H.V1)                                                     # HiFi-GAN's own description is unchanged
    assert hv1.buffer_spec(32, 800) == [("u", torch.float32, E), ("r", torch.float32, E), ("s", torch.float32, E), ("t", torch.bfloat16, E)]


@pytest.mark.parametrize("kw", [
    dict(upsample_rates=(4, 2), upsample_kernel_sizes=(8, 5)),                               # k != 2u
    dict(upsample_rates=(3, 2), upsample_kernel_sizes=(6, 4)),                               # odd u
    dict(n_mel_channels=100),
    dict(resblock_kernel_sizes=(3, 6, 11)),                                                  # even
    dict(resblock_kernel_sizes=(3, 7, 13)),                                                  # > 11
    dict(resblock="3"),
    dict(activation="relu"),
    dict(upsample_rates=(4, 2), upsample_kernel_sizes=(8,)),
    dict(upsample_initial_channel=66),                                                       # does not halve twice
])
def test_constructor_refusals(kw):
    from glow_tts_amd import audio
    args = dict(G.TINY, n_mel_channels=16)
    args.update(kw)
    with pytest.raises(ValueError):
        audio.BigVGAN(**args)
    with pytest.raises(ValueError):                                                          # HiFi-GAN still wants multiples of 16
        audio.HiFiGAN(**dict(G.TINY24))


def test_padded_images_and_parameter_blocks(built):
    """TINY24 (96 -> 48 -> 24 channels): the last stage runs at 32; the padding is zero (alpha' 1, 1 / beta' 0), the real entries are
    those of the unpadded tensors; the parameters keep their published shapes"""
    from glow_tts_amd import _lib, audio
    ref = G.seeded(G.TINY24, 5)
    voc = audio.BigVGAN(n_mel_channels=16, **G.TINY24)
    voc.load_generator_state(ref.state_dict())
    assert voc.channels == [96, 48, 24] and voc.padded_channels == [96, 48, 32] and voc._width() == max(96, 2 * 48, 4 * 32)
    assert voc.ups[1][0].weight.shape == (48, 24, 4) and voc.activation_post.act.alpha.shape == (24,)
    imgs, blocks = voc.images(), voc.snake_blocks()
    convs, acts = voc._convs(), voc._activations()
    assert len(imgs) == voc.conv_launches == len(convs) and len(blocks) == voc.snake_launches == len(acts)
    L = _lib.lib()
    f32 = torch.from_numpy(G.filter64()).float()
    for act, blk in zip(acts, blocks):
        C = act.act.alpha.numel()
        Cp = (C + 15) // 16 * 16
        assert blk.dtype == torch.float32 and blk.numel() == 2 * Cp + 24
        a, ib = G.snake_params(act.act.alpha.numpy(), act.act.beta.numpy(), "snakebeta", True)
        assert torch.equal(blk[:C], torch.from_numpy(a).float()) and torch.equal(blk[Cp:Cp + C], torch.from_numpy(ib).float())
        assert bool((blk[C:Cp] == 1).all()) and bool((blk[Cp + C:2 * Cp] == 0).all())
        assert torch.equal(blk[2 * Cp:2 * Cp + 12], f32) and torch.equal(blk[2 * Cp + 12:], f32)
    # the last stage's images, decoded: real entries are the weights rounded to bf16, everything else zero
    (img_up, b_up), (img_c, b_c), (img_post, b_post) = imgs[1 + 1 + 18], imgs[1 + 1 + 18 + 1], imgs[-1]
    up, conv, post = convs[1 + 1 + 18], convs[1 + 1 + 18 + 1], convs[-1]
    assert up is voc.ups[1][0] and conv is voc.resblocks[3].convs1[0] and post is voc.conv_post
    bf = lambda w: w.to(torch.bfloat16).double().numpy()  # noqa: E731
    W = H.decode_image(img_up, 2 * 32, 48, 3, L.gt_voc_k_chunk(48)).reshape(3, 2, 32, 48)
    W3 = bf(audio.transposed_as_conv(up.weight, 2)).reshape(2, 24, 48, 3).transpose(3, 0, 1, 2)
    assert np.array_equal(W[:, :, :24], W3) and not W[:, :, 24:].any()
    assert torch.equal(b_up.view(2, 32)[:, :24], up.bias.expand(2, 24)) and not b_up.view(2, 32)[:, 24:].any()
    W = H.decode_image(img_c, 32, 32, 3, L.gt_voc_k_chunk(32))
    assert np.array_equal(W[:, :24, :24], bf(conv.weight).transpose(2, 0, 1)) and not W[:, 24:].any() and not W[:, :, 24:].any()
    assert torch.equal(b_c[:24], conv.bias) and not b_c[24:].any()
    W = H.decode_image(img_post, 1, 32, 7, L.gt_voc_k_chunk(32))
    assert np.array_equal(W[:, :, :24], bf(post.weight).transpose(2, 0, 1)) and not W[:, :, 24:].any() and torch.equal(b_post, post.bias)
    # a changed alpha is followed
    with torch.no_grad():
        voc.activation_post.act.alpha.add_(0.25)
    assert not torch.equal(voc.snake_blocks()[-1][:24], blocks[-1][:24])
