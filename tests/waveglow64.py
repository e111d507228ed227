"""TEST INFRASTRUCTURE ONLY — float64 restatements for the WaveGlow vocoder (csrc/waveglow.hip, audio.WaveGlow) and the
configurations of its tests.  A plain helper like tests/hifigan64.py.

  latent64          Z [L, 8] of utterance b: sigma times the counter generator's normals on stream 5 (tests/synth_noise_host.py)
  generator64       WaveGlow.infer on ONE utterance, channels-last numpy with explicit tap loops and a scatter-form transposed
                    convolution (emul=True: the kernels' numerics — the GEMM operands, spect and g rounded to bf16, the rest float64)
  TorchWaveGlow     a straightforward torch writing of the published network in float64 (conv_transpose1d / conv1d / unfold), in BOTH
                    directions (`infer` from a given latent, `forward` back to it), with either conditioning layout and optional weight
                    norm: the second, independent writing of the definition and the source of checkpoint-form state dicts
  init_for_tests    random weights a flow can be tested on: orthogonal 1x1 weights, a non-zero `end` (the original zero-initialises it)
"""
import warnings

import numpy as np
import torch
from torch import nn
from torch.nn import functional as F

import hifigan64 as H
import synth_noise_host as N
from oracle import rows64 as R64

TINY = dict(n_flows=4, n_early_every=2, n_channels=64, n_layers=3)
PUBLISHED = dict(n_flows=12, n_early_every=4, n_channels=256, n_layers=8)
TINY_FRAMES = (0, 1, 2, 3, 5)                    # 32 * 5 = 160 group positions cross a 128-position tile
STREAM = 5                                       # GT_WG_NOISE_STREAM
END_STD = 0.02                                   # init_for_tests: std of `end`'s weights; |log s| stays O(0.1) per flow (test_waveglow_host.py)
SIGMA = 0.666


def flow_channels(cfg):
    return [8 - 2 * len([e for e in range(1, k + 1) if e % cfg["n_early_every"] == 0]) for k in range(cfg["n_flows"])]


def init_for_tests(voc, seed):
    """in place: the module's default initialisation, then orthogonal 1x1 weights with positive determinant (the original's), a normal
    `end` of std END_STD with a small bias, and an upsampler scaled to give spect O(1)"""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for p in voc.parameters():
            bound = 1.0 / np.sqrt(max(p[0].numel(), 1)) if p.dim() > 1 else 0.1
            p.copy_((torch.rand(p.shape, generator=g) * 2 - 1) * bound)
        voc.upsample.weight.mul_(0.25)
        for j in range(voc.n_flows):
            c = voc.flow_channels[j]
            q = torch.linalg.qr(torch.randn(c, c, generator=g, dtype=torch.float64))[0]
            if torch.det(q) < 0:
                q[:, 0] = -q[:, 0]
            q = q + 0.05 * torch.randn(c, c, generator=g, dtype=torch.float64)
            voc.convinv[j].conv.weight.copy_(q.float()[:, :, None])
            voc.WN[j].end.weight.copy_(torch.randn(voc.WN[j].end.weight.shape, generator=g) * END_STD)
            voc.WN[j].end.bias.copy_(torch.randn(voc.WN[j].end.bias.shape, generator=g) * 0.01)
    return voc


def latent64(seed, b, L, sigma=SIGMA):
    """Z [L, 8] float64: Z[l, 2p], Z[l, 2p + 1] = sigma (e0, e1) of randn_pair(key(seed, 5, b), l, p)"""
    e0, e1 = N.randn_pair(seed, STREAM, b, np.arange(L)[:, None], np.arange(4)[None, :])
    Z = np.empty((L, 8))
    Z[:, 0::2], Z[:, 1::2] = e0, e1
    return Z * sigma


def _r(x, emul):
    """a GEMM operand: rounded to bf16 under emulation"""
    x = np.asarray(x, dtype=np.float64)
    return R64.bf16_round(x.astype(np.float32)) if emul else x


def spect64(p, mel, emul):
    """mel [80, F] -> spect [32 F, 640]: the transposed convolution in scatter form, its last 768 outputs dropped, grouped by 8 with
    channel 8 band + sample % 8"""
    Fr = mel.shape[1]
    w, x = _r(p["upsample.weight"], emul), _r(mel.T, emul)                     # [80, 80, 1024], [F, 80]
    y = np.zeros((256 * Fr + 768, 80))
    for m in range(1024):
        y[m:m + 256 * Fr:256] += x @ w[:, :, m]
    y = y[:256 * Fr] + p["upsample.bias"]
    s = y.reshape(32 * Fr, 8, 80).transpose(0, 2, 1).reshape(32 * Fr, 640)
    return _r(s, emul)


def wn64(p, q, cfg, a0, spect, emul):
    """WN_j on one utterance: a0 [L, h], spect [L, 640] -> [L, 2h]"""
    C, n = cfg["n_channels"], cfg["n_layers"]
    x = a0 @ p[q + "start.weight"][:, :, 0].T + p[q + "start.bias"]
    skip = np.zeros_like(x)
    for i in range(n):
        W = np.ascontiguousarray(_r(p[q + f"in_layers.{i}.weight"], emul).transpose(2, 0, 1))
        acts = H.conv64(_r(x, emul), W, 3, 2 ** i)[0] + p[q + f"in_layers.{i}.bias"]
        sl = slice(2 * C * i, 2 * C * (i + 1))
        acts = acts + spect @ _r(p[q + "cond_layer.weight"][sl, :, 0], emul).T + p[q + "cond_layer.bias"][sl]
        g = _r(np.tanh(acts[:, :C]) / (1.0 + np.exp(-acts[:, C:])), emul)
        r = g @ _r(p[q + f"res_skip_layers.{i}.weight"][:, :, 0], emul).T + p[q + f"res_skip_layers.{i}.bias"]
        if i < n - 1:
            x, skip = x + r[:, :C], skip + r[:, C:]
        else:
            skip = skip + r
    return skip @ p[q + "end.weight"][:, :, 0].T + p[q + "end.bias"]


def generator64(sd, cfg, mel, seed, b, emul=False, sigma=SIGMA, stats=None):
    """WaveGlow.infer on ONE utterance: sd the module's state dict (published names, v5 conditioning layout), mel [80, F] -> wav [256 F]
    float64, the latent that of batch row b.  emul: the GEMM operands (weights, the mel, the residual stream as staged), spect and g
    rounded to bf16; everything else float64.  stats (a list): max |log s| per flow is appended."""
    p = {k: v.detach().cpu().double().numpy() for k, v in sd.items()}
    mel = np.asarray(mel, dtype=np.float64)
    Fr = mel.shape[1]
    if Fr == 0:
        return np.zeros(0)
    L, chans = 32 * Fr, flow_channels(cfg)
    Z = latent64(seed, b, L, sigma)
    spect = spect64(p, mel, emul)
    a = Z[:, 8 - chans[-1]:]
    for j in range(cfg["n_flows"] - 1, -1, -1):
        h = a.shape[1] // 2
        o = wn64(p, f"WN.{j}.", cfg, a[:, :h], spect, emul)
        if stats is not None:
            stats.append(float(np.abs(o[:, h:]).max()))
        a = np.concatenate([a[:, :h], (a[:, h:] - o[:, :h]) * np.exp(-o[:, h:])], 1)
        a = a @ np.linalg.inv(p[f"convinv.{j}.conv.weight"][:, :, 0]).T
        if j % cfg["n_early_every"] == 0 and j > 0:
            lo = 8 - a.shape[1]
            a = np.concatenate([Z[:, lo - 2:lo], a], 1)
    return a.reshape(-1)


rel_l2 = H.rel_l2
random_mel = H.random_mel


# ----------------------------------------------------------------------------- a straightforward torch WaveGlow, both directions
def _wn(m, on):
    if not on:
        return m
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return nn.utils.weight_norm(m)


class _TorchWN(nn.Module):
    def __init__(self, n_in, C, n, per_layer_cond, wn):
        super().__init__()
        self.C, self.n, self.per_layer = C, n, per_layer_cond
        self.start = _wn(nn.Conv1d(n_in, C, 1), wn)
        self.in_layers = nn.ModuleList(_wn(nn.Conv1d(C, 2 * C, 3, dilation=2 ** i, padding=2 ** i), wn) for i in range(n))
        if per_layer_cond:
            self.cond_layers = nn.ModuleList(_wn(nn.Conv1d(640, 2 * C, 1), wn) for _ in range(n))
        else:
            self.cond_layer = _wn(nn.Conv1d(640, 2 * C * n, 1), wn)
        self.res_skip_layers = nn.ModuleList(_wn(nn.Conv1d(C, 2 * C if i < n - 1 else C, 1), wn) for i in range(n))
        self.end = nn.Conv1d(C, 2 * n_in, 1)

    def forward(self, audio, spect):
        C = self.C
        audio = self.start(audio)
        output = torch.zeros_like(audio)
        cond = None if self.per_layer else self.cond_layer(spect)
        for i in range(self.n):
            c = self.cond_layers[i](spect) if self.per_layer else cond[:, 2 * C * i:2 * C * (i + 1)]
            acts = self.in_layers[i](audio) + c
            acts = torch.tanh(acts[:, :C]) * torch.sigmoid(acts[:, C:])
            rs = self.res_skip_layers[i](acts)
            if i < self.n - 1:
                audio, output = audio + rs[:, :C], output + rs[:, C:]
            else:
                output = output + rs
        return self.end(output)


class _TorchInv(nn.Module):
    def __init__(self, c):
        super().__init__()
        self.conv = nn.Conv1d(c, c, 1, bias=False)


class TorchWaveGlow(nn.Module):
    """the published network with torch's own convolutions, float64; per_layer_cond: the older `cond_layers.i` layout; weight_norm: the
    checkpoint form (weight_g / weight_v) of every layer the original normalises"""

    def __init__(self, cfg, per_layer_cond=False, weight_norm=False):
        super().__init__()
        self.cfg = cfg
        chans = flow_channels(cfg)
        self.upsample = nn.ConvTranspose1d(80, 80, 1024, stride=256)
        self.WN = nn.ModuleList(_TorchWN(c // 2, cfg["n_channels"], cfg["n_layers"], per_layer_cond, weight_norm) for c in chans)
        self.convinv = nn.ModuleList(_TorchInv(c) for c in chans)
        self.double()

    def spect(self, mel):
        s = self.upsample(mel)
        s = s[:, :, :-(1024 - 256)]
        s = s.unfold(2, 8, 8).permute(0, 2, 1, 3)
        return s.contiguous().view(s.size(0), s.size(1), -1).permute(0, 2, 1)

    def infer(self, mel, Z):
        """mel [1, 80, F], Z [1, 8, L] (the whole latent, channel order as the forward direction emits it) -> wav [1, 8 L]"""
        cfg = self.cfg
        spect = self.spect(mel)
        n_rem = flow_channels(cfg)[-1]
        audio, used = Z[:, 8 - n_rem:], 8 - n_rem
        for k in reversed(range(cfg["n_flows"])):
            h = audio.size(1) // 2
            a0, a1 = audio[:, :h], audio[:, h:]
            out = self.WN[k](a0, spect)
            a1 = (a1 - out[:, :h]) / torch.exp(out[:, h:])
            audio = torch.cat([a0, a1], 1)
            audio = F.conv1d(audio, torch.linalg.inv(self.convinv[k].conv.weight[:, :, 0])[:, :, None])
            if k % cfg["n_early_every"] == 0 and k > 0:
                audio = torch.cat((Z[:, used - 2:used], audio), 1)
                used -= 2
        return audio.permute(0, 2, 1).contiguous().view(audio.size(0), -1)

    def forward(self, mel, wav):
        """the training direction: wav [1, 8 L] -> Z [1, 8, L]"""
        cfg = self.cfg
        spect = self.spect(mel)
        audio = wav.unfold(1, 8, 8).permute(0, 2, 1)
        outs = []
        for k in range(cfg["n_flows"]):
            if k % cfg["n_early_every"] == 0 and k > 0:
                outs.append(audio[:, :2])
                audio = audio[:, 2:]
            audio = self.convinv[k].conv(audio)
            h = audio.size(1) // 2
            a0, a1 = audio[:, :h], audio[:, h:]
            out = self.WN[k](a0, spect)
            audio = torch.cat([a0, torch.exp(out[:, h:]) * a1 + out[:, :h]], 1)
        outs.append(audio)
        return torch.cat(outs, 1)
