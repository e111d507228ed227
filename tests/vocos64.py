"""TEST INFRASTRUCTURE ONLY — float64 restatements for the Vocos vocoder (csrc/vocos.hip, audio.Vocos) and the shapes
of its tests.  A plain helper like tests/hifigan64.py.

  ln64, dwconv64, gelu64   the pieces of a ConvNeXt block on ONE utterance, channels-last [L, C], zero padding at the utterance's own ends
  istft64           STFT.inverse's definition in float64: frames = inverse_basis64()^T Y, overlap-added, divided by the sum of the
                    squared windows that cover a sample, times n_fft / hop = 4, 512 samples trimmed at both ends
  generator64       the published generator on ONE utterance from a state dict under the published names: mel [n_mel, F] ->
                    wav [256 (F - 1)] (nothing below 2 frames).  emul=True is the device's rounding model: bf16 where the kernels round
                    to bf16 — the mel and the embedding weights, every norm's bf16 output, W1, u and gamma W2 (folded in float64,
                    through fp32), the head's operand and weights — and float64 everywhere else
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hifigan64 as H  # noqa: E402
from oracle import rows64 as R64  # noqa: E402

N_FFT, HOP, NBIN = 1024, 256, 513
EPS = 1e-6
HIDDEN_CHUNK = 128                                       # gt_vocos_hidden_chunk(); the GPU tests assert it
TINY = dict(input_channels=80, dim=128, intermediate_dim=2 * HIDDEN_CHUNK, num_layers=2)
PUBLISHED = dict(input_channels=80, dim=512, intermediate_dim=1536, num_layers=8)

rel_l2 = H.rel_l2
random_mel = H.random_mel


def bf16(x):
    """value of bf16(fp32(x)) as float64"""
    return R64.bf16_round(np.asarray(x, dtype=np.float64).astype(np.float32))


def ln64(x, g, b, eps=EPS):
    """LayerNorm over the last axis, (mean, variance of the centred values)"""
    d = x - x.mean(axis=-1, keepdims=True)
    return d / np.sqrt((d * d).mean(axis=-1, keepdims=True) + eps) * g + b


def dwconv64(x, w, b):
    """x [L, C], depthwise weight [C, 1, 7] or [C, 7], bias [C] -> [L, C]; taps outside [0, L) contribute 0"""
    w = np.asarray(w, dtype=np.float64).reshape(x.shape[1], 7)
    L = x.shape[0]
    y = np.tile(np.asarray(b, dtype=np.float64), (L, 1))
    for j in range(7):
        s = j - 3
        lo, hi = max(0, -s), min(L, L - s)
        if lo < hi:
            y[lo:hi] += x[lo + s:hi + s] * w[:, j]
    return y


def gelu64(x):
    return 0.5 * x * (1.0 + torch.erf(torch.from_numpy(np.ascontiguousarray(x)) / np.sqrt(2.0)).numpy())


def gelu_grad_max():
    """max |gelu'(x)| = 1.1290 (at x = sqrt 2): the factor that carries a pre-activation's bound through the GELU"""
    return 1.13


_BASIS = None


def istft64(re, im):
    """(re, im) [513, F] float64 -> [256 (F - 1)]: the definition of the reference's STFT.inverse"""
    global _BASIS
    from glow_tts_amd import audio
    if _BASIS is None:
        _BASIS = audio.inverse_basis64()
    re, im = np.asarray(re, dtype=np.float64), np.asarray(im, dtype=np.float64)
    F = re.shape[1]
    frames = re.T @ _BASIS[:NBIN] + im.T @ _BASIS[NBIN:]
    w2 = audio.hann_periodic(N_FFT).astype(np.float64) ** 2
    out, env = np.zeros(N_FFT + HOP * (F - 1)), np.zeros(N_FFT + HOP * (F - 1))
    for f in range(F):
        out[f * HOP:f * HOP + N_FFT] += frames[f]
        env[f * HOP:f * HOP + N_FFT] += w2
    nz = env > np.finfo(np.float32).tiny
    out[nz] /= env[nz]
    return (out * (N_FFT / HOP))[N_FFT // 2:-(N_FFT // 2)]


def fold64(gamma, w2, b2, emul):
    """(gamma W2, gamma b2) in float64; emul: rounded to fp32 once, the matrix then to bf16 (its image)"""
    g = np.asarray(gamma, dtype=np.float64)
    W, b = g[:, None] * np.asarray(w2, dtype=np.float64), g * np.asarray(b2, dtype=np.float64)
    if emul:
        W, b = bf16(W), b.astype(np.float32).astype(np.float64)
    return W, b


def head64(o):
    """head rows o [F, 1026] -> (re, im) [513, F]"""
    m = np.minimum(np.exp(o[:, :NBIN]), 100.0)
    return (m * np.cos(o[:, NBIN:])).T, (m * np.sin(o[:, NBIN:])).T


def generator64(sd, cfg, mel, emul=False):
    p = {k: v.detach().cpu().double().numpy() for k, v in sd.items()}
    mel = np.asarray(mel, dtype=np.float64)
    if mel.shape[1] < 2:
        return np.zeros(0)
    r = bf16 if emul else (lambda v: v)
    x = H.conv64(r(mel.T), np.ascontiguousarray(r(p["backbone.embed.weight"]).transpose(2, 0, 1)), 7, 1)[0] + p["backbone.embed.bias"]
    x = ln64(x, p["backbone.norm.weight"], p["backbone.norm.bias"])
    for i in range(cfg["num_layers"]):
        q = f"backbone.convnext.{i}."
        a = r(ln64(dwconv64(x, p[q + "dwconv.weight"], p[q + "dwconv.bias"]), p[q + "norm.weight"], p[q + "norm.bias"]))
        u = r(gelu64(a @ r(p[q + "pwconv1.weight"]).T + p[q + "pwconv1.bias"]))
        W2, b2 = fold64(p[q + "gamma"], p[q + "pwconv2.weight"], p[q + "pwconv2.bias"], emul)
        x = x + (u @ W2.T + b2)
    a = r(ln64(x, p["backbone.final_layer_norm.weight"], p["backbone.final_layer_norm.bias"]))
    o = a @ r(p["head.out.weight"]).T + p["head.out.bias"]
    return istft64(*head64(o))


def init_for_tests(voc, seed):
    """torch's default initialisation under `seed` is the module's own; on top: gamma ~ U(0.1, 1) and the head's weight x 4 (phases of
    a few radians, magnitudes over e^+-2)"""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for blk in voc.backbone.convnext:
            blk.gamma.copy_(torch.rand(blk.gamma.shape, generator=g) * 0.9 + 0.1)
        voc.head.out.weight.mul_(4.0)
    return voc
