"""CPU tests of the WaveGlow vocoder's host side (audio.WaveGlow) and of the float64 restatement the GPU tests measure
against (tests/waveglow64.py):

  - generator64 (numpy, channels-last, scatter-form upsampling) against TorchWaveGlow.infer (torch's conv_transpose1d / conv1d /
    unfold, float64) to 1e-10: the group ordering of spect, the early-output order and the slot walk of the latent;
  - generator64's samples pushed through the FORWARD flow give the latent back, to 1e-8: the reverse flow is the inverse;
  - the transposed convolution as a centred 7-tap convolution, and the grouped row order of its image;
  - both checkpoint layouts (cond_layer / cond_layers.i), with and without weight norm, load to equal parameters and equal images;
  - every constructor refusal, wav_len, buffer_spec and workspace_bytes;
  - init_for_tests keeps |log s| O(0.1) per flow and the emulation inside the GPU tests' conditions.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import waveglow64 as W  # noqa: E402


def make(cfg, seed=5):
    from glow_tts_amd import audio
    return W.init_for_tests(audio.WaveGlow(**cfg), seed)


def state(voc):
    return {k: v.detach().cpu() for k, v in voc.state_dict().items()}


@pytest.mark.parametrize("frames", [1, 3])
def test_generator64_agrees_with_the_torch_formulation_and_inverts(built, frames):
    voc = make(W.TINY)
    sd = state(voc)
    tw = W.TorchWaveGlow(W.TINY)
    tw.load_state_dict({k: v.double() for k, v in sd.items()}, strict=True)
    mel = W.random_mel(np.random.default_rng(frames), 80, frames)
    stats = []
    wav = W.generator64(sd, W.TINY, mel, seed=11, b=2, stats=stats)
    assert wav.shape == (256 * frames,) and len(stats) == W.TINY["n_flows"]
    Z = torch.from_numpy(W.latent64(11, 2, 32 * frames)).t()[None]
    mel_t = torch.from_numpy(mel).double()[None]
    with torch.no_grad():
        ref = tw.infer(mel_t, Z)[0].numpy()
        back = tw(mel_t, torch.from_numpy(wav)[None])[0].numpy()
    scale = max(1.0, float(np.abs(ref).max()))
    assert float(np.abs(wav - ref).max()) <= 1e-10 * scale, float(np.abs(wav - ref).max())
    assert float(np.abs(back - Z[0].numpy()).max()) <= 1e-8, float(np.abs(back - Z[0].numpy()).max())
    assert float(np.abs(ref).max()) > 1e-3
    # another row of the batch, another seed: another latent
    assert not np.allclose(W.latent64(11, 2, 8), W.latent64(11, 3, 8)) and not np.allclose(W.latent64(11, 2, 8), W.latent64(12, 2, 8))


def test_upsampler_as_a_seven_tap_convolution(built):
    from glow_tts_amd import audio
    g = torch.Generator().manual_seed(3)
    w = torch.randn(6, 5, 16, generator=g, dtype=torch.float64)
    x = torch.randn(1, 6, 9, generator=g, dtype=torch.float64)
    ref = torch.nn.functional.conv_transpose1d(x, w, stride=4)[:, :, :36]                  # the last k - u = 12 outputs dropped
    W7 = audio.transposed_tail_as_conv(w, 4)
    assert W7.shape == (20, 6, 7) and not W7[:, :, 4:].any()
    y = torch.nn.functional.conv1d(x, W7, padding=3)                                        # [1, 4 * 5, 9], row r * 5 + c
    got = y.view(1, 4, 5, 9).permute(0, 2, 3, 1).reshape(1, 5, 36)
    assert torch.allclose(got, ref, rtol=0, atol=1e-12)
    with pytest.raises(ValueError):
        audio.transposed_tail_as_conv(w, 5)
    perm = audio.gate_interleave(64)
    assert perm.tolist() == list(range(0, 32)) + list(range(64, 96)) + list(range(32, 64)) + list(range(96, 128))


def test_both_checkpoint_layouts_and_weight_norm_load_to_equal_images(built):
    from glow_tts_amd import audio
    torch.manual_seed(9)
    tw = W.TorchWaveGlow(W.TINY, per_layer_cond=True, weight_norm=True)
    sd_norm = {k: v.clone() for k, v in tw.state_dict().items()}
    assert any(k.endswith("cond_layers.1.weight_g") for k in sd_norm) and "WN.0.in_layers.0.weight_v" in sd_norm
    for m in tw.modules():
        if hasattr(m, "weight_g"):
            torch.nn.utils.remove_weight_norm(m)
    sd_folded = {k: v.clone() for k, v in tw.state_dict().items()}
    assert not any(k.endswith("weight_g") for k in sd_folded)
    sd_v5 = {k: v for k, v in sd_folded.items() if ".cond_layers." not in k}
    for j in range(W.TINY["n_flows"]):
        for kind in ("weight", "bias"):
            sd_v5[f"WN.{j}.cond_layer.{kind}"] = torch.cat([sd_folded[f"WN.{j}.cond_layers.{i}.{kind}"] for i in range(W.TINY["n_layers"])], 0)
    vocs = []
    for sd in (sd_norm, sd_folded, sd_v5):
        voc = audio.WaveGlow(**W.TINY)
        voc.load_waveglow_state(sd)
        vocs.append(voc)
    ref = vocs[2].state_dict()
    assert set(ref) == set(state(make(W.TINY)))
    for voc in vocs[:2]:
        for k, v in voc.state_dict().items():
            assert torch.allclose(v, ref[k], rtol=2e-7, atol=1e-9), k
    assert torch.equal(vocs[1].state_dict()["WN.2.cond_layer.weight"], ref["WN.2.cond_layer.weight"])

    def flat(im):
        out = list(im["up"])
        for fl in im["flows"]:
            out += [*fl["start"], *fl["end"], fl["inv"]]
            for ly in fl["layers"]:
                out += [ly["W_in"], ly["W_cond"], ly["b_in"], ly["b_cond"], *ly["res"]]
        return out
    a, b = flat(vocs[1].images()), flat(vocs[2].images())
    assert len(a) == len(b) == 2 + 4 * (5 + 3 * 6)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    with pytest.raises(KeyError):
        audio.WaveGlow(**W.TINY).load_waveglow_state({k: v for k, v in sd_folded.items() if k != "WN.1.cond_layers.2.bias"})
    with pytest.raises(RuntimeError):
        audio.WaveGlow(**W.TINY).load_waveglow_state({k: v for k, v in sd_v5.items() if k != "upsample.bias"})


def test_image_layouts(built):
    """the boundary's matrices in slot order, the gate's images with interleaved rows, the upsampler's 20480 grouped rows"""
    import hifigan64 as H
    from glow_tts_amd import audio
    voc = make(W.TINY)
    im = voc.images()
    assert voc.images() is im and voc.flow_channels == [8, 8, 6, 6] and voc.n_remaining == 6
    sd = state(voc)
    C = 64
    fl = im["flows"][3]                                                                    # c = 6: slots 2 .. 7, halves 2..4 | 5..7
    assert fl["start"][0].shape == (C, 8) and torch.equal(fl["start"][0][:, 2:5], sd["WN.3.start.weight"][:, :, 0])
    assert not fl["start"][0][:, :2].any() and not fl["start"][0][:, 5:].any()
    we = sd["WN.3.end.weight"][:, :, 0]
    assert torch.equal(fl["end"][0][:, 1:4], we[:3].t()) and torch.equal(fl["end"][0][:, 5:8], we[3:].t())
    assert not fl["end"][0][:, 0].any() and not fl["end"][0][:, 4].any()
    assert torch.equal(fl["end"][1][1:4], sd["WN.3.end.bias"][:3]) and torch.equal(fl["end"][1][5:8], sd["WN.3.end.bias"][3:])
    inv = torch.linalg.inv(sd["convinv.3.conv.weight"][:, :, 0].double())
    assert torch.equal(fl["inv"][2:, 2:], inv.float()) and not fl["inv"][:2].any() and not fl["inv"][:, :2].any()
    perm = audio.gate_interleave(C).numpy()
    Win = H.decode_image(fl["layers"][1]["W_in"], 2 * C, C, 3, 64)                          # [3][2C][C]
    want = R64_round(sd["WN.3.in_layers.1.weight"].numpy()).transpose(2, 0, 1)[:, perm]
    assert np.array_equal(Win, want)
    Wc = H.decode_image(fl["layers"][1]["W_cond"], 2 * C, 640, 1, 64)[0]
    assert np.array_equal(Wc, R64_round(sd["WN.3.cond_layer.weight"].numpy()[2 * C:4 * C, :, 0])[perm])
    up = H.decode_image(im["up"][0], 20480, 80, 7, 32)
    w = R64_round(sd["upsample.weight"].numpy())
    for (l, m, i, j) in ((0, 0, 0, 0), (31, 79, 7, 3), (5, 17, 3, 2)):
        assert np.array_equal(up[3 - j, 640 * l + 8 * m + i], w[:, m, 8 * l + i + 256 * j])
    assert not up[4:].any() and torch.equal(im["up"][1].view(32, 80, 8)[7, :, 3], sd["upsample.bias"])
    with torch.no_grad():
        voc.WN[0].end.bias.add_(1.0)
    assert voc.images() is not im


def R64_round(x):
    from oracle import rows64 as R64
    return R64.bf16_round(np.asarray(x, dtype=np.float32))


def test_from_config_and_refusals(built):
    from glow_tts_amd import audio
    cfg = {"waveglow_config": {"n_mel_channels": 80, "n_flows": 12, "n_group": 8, "n_early_every": 4, "n_early_size": 2,
                               "WN_config": {"n_layers": 8, "n_channels": 256, "kernel_size": 3}}}
    for c in (cfg, cfg["waveglow_config"]):
        voc = audio.WaveGlow.from_config(c)
        assert (voc.n_flows, voc.n_layers, voc.n_channels, voc.sigma) == (12, 8, 256, 0.666)
        assert voc.flow_channels == [8] * 4 + [6] * 4 + [4] * 4 and voc.n_remaining == 4
        assert voc.launches == 1 + 192 + 13 == 206
        assert voc.seeded and (voc.hop_length, voc.min_frames, voc.mel_channels) == (256, 1, 80)
    assert not audio.HiFiGAN.seeded and not audio.Vocos.seeded
    assert audio.WaveGlow.from_config(dict(cfg["waveglow_config"], sigma=0.9)).sigma == 0.9
    for kw, word in ((dict(n_group=4), "n_group"), (dict(n_group=16), "n_group"), (dict(kernel_size=5), "kernel_size"),
                     (dict(n_channels=96), "n_channels"), (dict(n_channels=0), "n_channels"), (dict(n_channels=576), "n_channels"),
                     (dict(n_layers=9), "n_layers"), (dict(n_layers=0), "n_layers"), (dict(upsample_kernel_size=800), "upsampler"),
                     (dict(upsample_stride=200), "upsampler"), (dict(n_early_size=4), "n_early_size"),
                     (dict(n_flows=17, n_early_every=4), "channel"), (dict(n_flows=12, n_early_every=2), "channel"),
                     (dict(n_mel_channels=100), "mel"), (dict(sigma=-1.0), "sigma"), (dict(n_flows=0), "positive")):
        with pytest.raises(ValueError, match=word):
            audio.WaveGlow(**dict(W.TINY, **kw))
    assert audio.WaveGlow(n_flows=13, n_early_every=4, n_channels=64, n_layers=1).flow_channels[-1] == 2


def test_lengths_and_workspace(built):
    from glow_tts_amd import audio
    voc = audio.WaveGlow(**W.TINY)
    assert [voc.wav_len(f) for f in (0, 1, 7)] == [0, 256, 1792]
    spec = voc.buffer_spec(3, 7)
    L = 32 * 7
    assert spec == [("state", torch.float32, 3 * L * 128), ("g", torch.bfloat16, 3 * L * 64), ("spect", torch.bfloat16, 3 * L * 640)]
    assert voc.workspace_bytes(3, 7) == 3 * L * (10 * 64 + 1280) + 1024 * 3 * 7
    pub = audio.WaveGlow()
    assert pub.workspace_bytes(32, 800) == 32 * 25600 * (2560 + 1280) + 1024 * 32 * 800 == 3171942400
    for B, F_ in ((0, 5), (1, 0), (64, 1 << 14)):                                          # 64 * 32 * 2^14 * 640 >= 2^31
        with pytest.raises(ValueError):
            voc.buffer_spec(B, F_)
    with pytest.raises(audio.CpuWaveError):
        voc(torch.zeros(1, 80, 4))
    with pytest.raises(ValueError, match="no seed"):
        audio._MelVocoder.run(audio.Vocos(num_layers=1), torch.zeros(1, 80, 4), torch.zeros(1, dtype=torch.int32), {"wav": torch.zeros(1, 768)}, seed=3)


def test_init_for_tests_meets_the_gpu_tests_conditions(built):
    """|log s| stays O(0.1) per flow, and the CPU emulation alone satisfies 0 < E_emul < 0.05 and max |exact| > 1e-3 at the shapes of
    tests/test_waveglow_gpu.py (TINY; PUBLISHED is checked there, next to the device, from the same helper)"""
    sd = state(make(W.TINY, seed=7))
    rng = np.random.default_rng(17)
    exact, emul, stats = [], [], []
    for b, n in enumerate(W.TINY_FRAMES):
        mel = W.random_mel(rng, 80, n)
        exact.append(W.generator64(sd, W.TINY, mel, 3, b, stats=stats))
        emul.append(W.generator64(sd, W.TINY, mel, 3, b, emul=True))
    exact, emul = np.concatenate(exact), np.concatenate(emul)
    e = W.rel_l2(emul, exact)
    print(f"TINY: max |log s| {max(stats):.3f}, E_emul {e:.3e}, max |exact| {np.abs(exact).max():.3f}")
    assert 0.01 < max(stats) < 1.0
    assert 0 < e < 0.05 and float(np.abs(exact).max()) > 1e-3
