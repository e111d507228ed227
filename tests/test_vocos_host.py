"""CPU tests of the Vocos vocoder's host side (glow_tts_amd.audio.Vocos) and of the float64 restatement its GPU tests
measure against (tests/vocos64.py):

  * vocos64.generator64 agrees with a second, independent float64 writing of the published model — torch modules (Conv1d, LayerNorm,
    Linear, GELU) and torch.istft(center=True, window=hann_window(1024)) — on every utterance of a ragged batch;
  * STFT.inverse's definition (inverse_basis64, the sum of squared windows, x 4, 512 trimmed per side: vocos64.istft64) IS
    torch.istft(center=True): to 1e-12 on random, inconsistent spectra with non-zero Im in bins 0 and 512;
  * the layer-scale folding, the published parameter names, checkpoint loading (dropped keys, a missing key), from_config, the
    constructor's refusals, the image layouts and the zero-padded 100-band embedding."""
import os
import sys

import numpy as np
import pytest
import torch
from torch import nn

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hifigan64 as H  # noqa: E402
import vocos64 as V  # noqa: E402


def make(cfg=None, seed=5, **kw):
    from glow_tts_amd import audio
    torch.manual_seed(seed)
    return V.init_for_tests(audio.Vocos(**dict(cfg or V.TINY, **kw)), seed + 1)


class TorchBlock(nn.Module):
    def __init__(self, dim, inter):
        super().__init__()
        self.dwconv = nn.Conv1d(dim, dim, 7, padding=3, groups=dim)
        self.norm = nn.LayerNorm(dim, eps=1e-6)
        self.pwconv1, self.act, self.pwconv2 = nn.Linear(dim, inter), nn.GELU(), nn.Linear(inter, dim)
        self.gamma = nn.Parameter(torch.ones(dim))

    def forward(self, x):                                                          # [1, C, F]
        y = self.norm(self.dwconv(x).transpose(1, 2))
        y = self.gamma * self.pwconv2(self.act(self.pwconv1(y)))
        return x + y.transpose(1, 2)


class TorchVocos(nn.Module):
    """the published VocosBackbone + ISTFTHead(padding="center") with torch's own modules"""

    def __init__(self, input_channels, dim, intermediate_dim, num_layers):
        super().__init__()
        self.backbone = nn.Module()
        self.backbone.embed = nn.Conv1d(input_channels, dim, 7, padding=3)
        self.backbone.norm = nn.LayerNorm(dim, eps=1e-6)
        self.backbone.convnext = nn.ModuleList(TorchBlock(dim, intermediate_dim) for _ in range(num_layers))
        self.backbone.final_layer_norm = nn.LayerNorm(dim, eps=1e-6)
        self.head = nn.Module()
        self.head.out = nn.Linear(dim, 1026)

    def forward(self, mel):                                                        # [1, n_mel, F]
        bb = self.backbone
        x = bb.norm(bb.embed(mel).transpose(1, 2)).transpose(1, 2)
        for blk in bb.convnext:
            x = blk(x)
        o = self.head.out(bb.final_layer_norm(x.transpose(1, 2))).transpose(1, 2)
        mag, p = o.chunk(2, dim=1)
        mag = torch.clip(torch.exp(mag), max=1e2)
        S = mag * (torch.cos(p) + 1j * torch.sin(p))
        return torch.istft(S, 1024, 256, 1024, torch.hann_window(1024, dtype=mel.dtype), center=True)


def test_generator64_agrees_with_the_torch_formulation(built):
    voc = make()
    sd = voc.state_dict()
    ref = TorchVocos(**V.TINY).double()
    ref.load_state_dict({k: v.double() for k, v in sd.items()}, strict=True)
    rng = np.random.default_rng(2)
    for n in (2, 3, 9, 21):
        mel = V.random_mel(rng, 80, n)
        want = ref(torch.from_numpy(mel).double()[None])[0].detach().numpy()
        got = V.generator64(sd, V.TINY, mel)
        assert got.shape == want.shape == (256 * (n - 1),)
        assert np.abs(want).max() > 1e-3
        assert V.rel_l2(got, want) < 1e-11, (n, V.rel_l2(got, want))
        emul = V.generator64(sd, V.TINY, mel, emul=True)
        assert 0 < V.rel_l2(emul, got) < 0.05                                     # the rounding model moves it, a little
    assert V.generator64(sd, V.TINY, V.random_mel(rng, 80, 1)).shape == (0,)


def test_stft_inverse_definition_is_torch_istft():
    rng = np.random.default_rng(3)
    for F in (2, 3, 4, 5, 12):
        re, im = rng.standard_normal((513, F)), rng.standard_normal((513, F))
        assert im[0].any() and im[512].any()
        want = torch.istft(torch.from_numpy(re + 1j * im), 1024, 256, 1024, torch.hann_window(1024, dtype=torch.float64), center=True)
        got = V.istft64(re, im)
        assert got.shape == tuple(want.shape) == (256 * (F - 1),)
        assert np.abs(got - want.numpy()).max() <= 1e-12


def test_layer_scale_folding(built):
    from glow_tts_amd import audio
    voc = make()
    blk = voc.backbone.convnext[1]
    w2, b2 = audio.fold_layer_scale(blk.gamma, blk.pwconv2.weight, blk.pwconv2.bias)
    g64, W64, b64 = blk.gamma.double(), blk.pwconv2.weight.double(), blk.pwconv2.bias.double()
    assert w2.dtype == b2.dtype == torch.float32
    assert torch.equal(w2, (g64[:, None] * W64).float()) and torch.equal(b2, (g64 * b64).float())
    u = torch.randn(9, V.TINY["intermediate_dim"], dtype=torch.float64)
    folded = u @ (g64[:, None] * W64).T + g64 * b64
    assert torch.allclose(folded, g64 * (u @ W64.T + b64), rtol=0, atol=1e-13)
    Wn, bn = V.fold64(blk.gamma.numpy(), blk.pwconv2.weight.numpy(), blk.pwconv2.bias.numpy(), emul=True)
    assert np.array_equal(Wn, w2.to(torch.bfloat16).double().numpy()) and np.array_equal(bn, b2.double().numpy())


def published_names(num_layers):
    names = ["backbone.embed.weight", "backbone.embed.bias", "backbone.norm.weight", "backbone.norm.bias",
             "backbone.final_layer_norm.weight", "backbone.final_layer_norm.bias", "head.out.weight", "head.out.bias"]
    for i in range(num_layers):
        names += [f"backbone.convnext.{i}.{k}" for k in ("gamma", "dwconv.weight", "dwconv.bias", "norm.weight", "norm.bias",
                                                         "pwconv1.weight", "pwconv1.bias", "pwconv2.weight", "pwconv2.bias")]
    return names


def test_parameter_tree_and_checkpoint_loading(built):
    from glow_tts_amd import audio
    voc = make()
    assert sorted(voc.state_dict()) == sorted(published_names(2))
    assert voc.backbone.embed.weight.shape == (128, 80, 7) and voc.backbone.convnext[0].dwconv.weight.shape == (128, 1, 7)
    assert voc.backbone.convnext[0].pwconv1.weight.shape == (256, 128) and voc.head.out.weight.shape == (1026, 128)
    assert voc.launches == 10 and audio.Vocos().launches == 22
    assert not any(p.requires_grad for p in voc.parameters())
    g = torch.Generator().manual_seed(9)
    sd = {k: torch.randn(v.shape, generator=g, dtype=torch.float64) for k, v in voc.state_dict().items()}
    sd["feature_extractor.mel_spec.spectrogram.window"] = torch.hann_window(1024)
    sd["feature_extractor.mel_spec.mel_scale.fb"] = torch.zeros(513, 80)
    sd["head.istft.window"] = torch.hann_window(1024)
    voc.load_vocos_state(sd)
    for k, v in voc.state_dict().items():
        assert v.dtype == torch.float32 and torch.equal(v, sd[k].float()), k
    del sd["backbone.convnext.1.gamma"]
    with pytest.raises(RuntimeError):
        voc.load_vocos_state(sd)
    sd["backbone.convnext.1.gamma"] = torch.ones(128)
    sd["backbone.convnext.1.norm.scale.weight"] = torch.ones(4, 128)               # an AdaLayerNorm's: unexpected
    with pytest.raises(RuntimeError):
        voc.load_vocos_state(sd)


def test_from_config_and_refusals(built):
    from glow_tts_amd import audio
    cfg = {"feature_extractor": {"class_path": "vocos.feature_extractors.MelSpectrogramFeatures",
                                 "init_args": {"sample_rate": 24000, "n_fft": 1024, "hop_length": 256, "n_mels": 100, "padding": "center"}},
           "backbone": {"class_path": "vocos.models.VocosBackbone",
                        "init_args": {"input_channels": 100, "dim": 512, "intermediate_dim": 1536, "num_layers": 8}},
           "head": {"class_path": "vocos.heads.ISTFTHead", "init_args": {"dim": 512, "n_fft": 1024, "hop_length": 256, "padding": "center"}}}
    voc = audio.Vocos.from_config(cfg)
    assert (voc.input_channels, voc.padded_channels, voc.dim, voc.intermediate_dim, voc.num_layers) == (100, 112, 512, 1536, 8)
    assert voc.hop_length == 256 and voc.n_fft == 1024 and sorted(voc.state_dict()) == sorted(published_names(8))
    bad = {k: dict(v, init_args=dict(v["init_args"])) for k, v in cfg.items()}
    bad["head"]["init_args"]["padding"] = "same"
    with pytest.raises(ValueError):
        audio.Vocos.from_config(bad)
    bad["head"]["init_args"]["padding"] = "center"
    bad["backbone"]["init_args"]["adanorm_num_embeddings"] = 4
    with pytest.raises(ValueError):
        audio.Vocos.from_config(bad)
    for kw in (dict(padding="same"), dict(adanorm_num_embeddings=4), dict(n_fft=2048), dict(hop_length=512), dict(n_fft=800, hop_length=200),
               dict(dim=192), dict(dim=64), dict(dim=1024), dict(intermediate_dim=1536 + 64), dict(intermediate_dim=2048 + 128),
               dict(intermediate_dim=0), dict(num_layers=0)):
        with pytest.raises(ValueError):
            audio.Vocos(**kw)
    audio.Vocos(dim=256, intermediate_dim=2048, num_layers=1)                     # the largest hidden width passes
    with pytest.raises(audio.CpuWaveError):
        make()(torch.zeros(1, 80, 8))
    with pytest.raises(ValueError):                                                # run takes multiples of 16 only
        make(input_channels=100).run(torch.zeros(1, 100, 8), torch.zeros(1, dtype=torch.int32), {})


def test_image_layouts_and_the_padded_embedding(built):
    from glow_tts_amd import _lib
    L = _lib.lib()
    assert L.gt_vocos_hidden_chunk() == V.HIDDEN_CHUNK
    voc = make(input_channels=100)
    im = voc.images()
    assert voc.images() is im and len(im["blocks"]) == 2
    C, Hd = 128, 256
    We = H.decode_image(im["embed"][0], C, 112, 7, L.gt_voc_k_chunk(112))          # asserts the image's padding is zero
    want = voc.backbone.embed.weight.to(torch.bfloat16).double().numpy().transpose(2, 0, 1)
    assert np.array_equal(We[:, :, :100], want) and not We[:, :, 100:].any()
    blk, mod = im["blocks"][1], voc.backbone.convnext[1]
    W1 = H.decode_image(blk["W1"], Hd, C, 1, L.gt_voc_k_chunk(C))[0]
    assert np.array_equal(W1, mod.pwconv1.weight.to(torch.bfloat16).double().numpy())
    W2 = H.decode_image(blk["W2"], C, Hd, 1, L.gt_voc_k_chunk(Hd))[0]
    assert np.array_equal(W2, V.fold64(mod.gamma.numpy(), mod.pwconv2.weight.numpy(), mod.pwconv2.bias.numpy(), True)[0])
    assert torch.equal(blk["wd"], mod.dwconv.weight.view(C, 7)) and torch.equal(blk["bd"], mod.dwconv.bias)
    assert torch.equal(blk["g"], mod.norm.weight) and torch.equal(blk["b1"], mod.pwconv1.bias)
    Wh = H.decode_image(im["head"][0], 1026, C, 1, L.gt_voc_k_chunk(C))[0]
    assert np.array_equal(Wh, voc.head.out.weight.to(torch.bfloat16).double().numpy())
    assert [n for n, _, _ in voc.buffer_spec(3, 70)] == ["x", "a", "o", "spec"]
    assert voc.workspace_bytes(3, 70) == 3 * 70 * (6 * C + 4 * 1026) + L.gt_gl_spec_bytes(3, 70) + 4 * 3 * 256 * 69
    with torch.no_grad():
        mod.gamma.mul_(2.0)
    assert voc.images() is not im
