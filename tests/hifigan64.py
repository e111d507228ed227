"""TEST INFRASTRUCTURE ONLY — float64 restatements for the HiFi-GAN vocoder (csrc/hifigan.hip, audio.HiFiGAN) and the
case lists of its tests.  A plain helper like tests/gl64.py.

  decode_image      gt_voc_conv's bf16 weight image -> float64 [taps][N][Cin], by the index formula of include/glowtts_hip.h
  prologue          the kernel's operand: fp32 leaky ReLU, rounded to bf16 (numpy float32 arithmetic)
  conv64            one utterance's dilated convolution with zero padding at its own ends, and its absolute-value twin
  generator64       the generator on ONE utterance, channels-last with explicit tap loops and a scatter-form transposed convolution
                    (emul=True: the kernel's numerics — operands rounded to bf16 where the kernel rounds them, the rest float64)
  TorchGenerator    a straightforward torch writing of the published generator (conv1d / conv_transpose1d, optional weight norm): the
                    second, independent writing of the definition, and the source of weight-normed state dicts
"""
import warnings

import numpy as np
import torch
from torch import nn
from torch.nn import functional as F

from oracle import rows64 as R64

TINY = dict(upsample_rates=(4, 2), upsample_kernel_sizes=(8, 4), upsample_initial_channel=64, resblock_kernel_sizes=(3, 7, 11),
            resblock_dilation_sizes=((1, 3, 5),) * 3)
V1 = dict(upsample_rates=(8, 8, 2, 2), upsample_kernel_sizes=(16, 16, 4, 4), upsample_initial_channel=512,
          resblock_kernel_sizes=(3, 7, 11), resblock_dilation_sizes=((1, 3, 5),) * 3)
TINY_FRAMES = (13, 1, 2, 40, 0, 7)
SLOPE = 0.1


# ----------------------------------------------------------------------------- the kernel's operands
def image_index(j, n, ci, N, Cin, kc):
    """flat element index of W[j][n][ci] in the image [taps][Np / 32][Kp / 16][64 lanes][8], lane = 32 h + r"""
    j, n, ci = (np.asarray(a, dtype=np.int64) for a in (j, n, ci))
    Np, Kp = (N + 31) // 32 * 32, (Cin + kc - 1) // kc * kc
    return (((j * (Np >> 5) + (n >> 5)) * (Kp >> 4) + (ci >> 4)) * 64 + 32 * ((ci & 15) >> 3) + (n & 31)) * 8 + (ci & 7)


def image_elems(N, Cin, taps, kc):
    return taps * ((N + 31) // 32 * 32) * ((Cin + kc - 1) // kc * kc)


def decode_image(img, N, Cin, taps, kc):
    """bf16 image (torch.bfloat16 or raw bits) -> float64 numpy [taps][N][Cin]"""
    flat = R64.bf2f(img).astype(np.float64)
    assert flat.size == image_elems(N, Cin, taps, kc), (flat.size, N, Cin, taps, kc)
    j, n, ci = np.meshgrid(np.arange(taps), np.arange(N), np.arange(Cin), indexing="ij")
    W = flat[image_index(j, n, ci, N, Cin, kc)]
    used = np.zeros(flat.size, dtype=bool)
    used[image_index(j, n, ci, N, Cin, kc)] = True
    assert not flat[~used].any(), "the image's padding is not zero"
    return W


def prologue(x32, slope):
    """float32 array -> the MFMA operand's value, float64: v < 0 ? v * slope : v in fp32, rounded to bf16"""
    x32 = np.asarray(x32, dtype=np.float32)
    v = np.where(x32 < 0, (x32 * np.float32(slope)).astype(np.float32), x32)
    return R64.bf16_round(v)


def conv64(X, W, taps, dil):
    """X [L, Cin] float64 (the operand values), W [taps][N][Cin] -> (Y, S) [L, N]: Y[t] = sum_j X[t + (j - taps // 2) dil] W[j]^T with
    zeros outside [0, L), S the same over absolute values"""
    L = X.shape[0]
    Y = np.zeros((L, W.shape[1]))
    S = np.zeros_like(Y)
    for j in range(taps):
        s = (j - taps // 2) * dil
        lo, hi = max(0, -s), min(L, L - s)
        if lo < hi:
            Y[lo:hi] += X[lo + s:hi + s] @ W[j].T
            S[lo:hi] += np.abs(X[lo + s:hi + s]) @ np.abs(W[j]).T
    return Y, S


# ----------------------------------------------------------------------------- the generator on one utterance
def _lrelu(x, slope):
    return np.where(x < 0, x * slope, x)


def _operand(x, slope, emul):
    """the conv's input: emul — the kernel's (fp32 multiply, bf16); exact — the float64 leaky ReLU"""
    if emul:
        return prologue(x.astype(np.float32), slope)
    return _lrelu(x, slope)


def _wt(w, emul):
    w = np.asarray(w, dtype=np.float64)
    return R64.bf16_round(w.astype(np.float32)) if emul else w


def _conv(x, w, b, dil, slope, emul):
    """x [L, Cin], conv weight w [N, Cin, k] -> [L, N]"""
    W = np.ascontiguousarray(_wt(w, emul).transpose(2, 0, 1))
    return conv64(_operand(x, slope, emul), W, W.shape[0], dil)[0] + np.asarray(b, dtype=np.float64)


def _up(x, w, b, u, slope, emul):
    """x [L, Cin], transposed-conv weight w [Cin, Cout, k], stride u, padding (k - u) / 2 -> [u L, Cout]: the scatter definition,
    y[u i + m - pad] += x[i] w[:, :, m]"""
    w = _wt(w, emul)
    Cin, Cout, k = w.shape
    pad, L = (k - u) // 2, x.shape[0]
    xo = _operand(x, slope, emul)
    y = np.zeros((u * L + 2 * pad + k, Cout))
    for m in range(k):
        y[m:m + u * L:u] += xo @ w[:, :, m]
    return y[pad:pad + u * L] + np.asarray(b, dtype=np.float64)


def generator64(sd, cfg, mel, resblock="1", emul=False):
    """the generator on ONE utterance: sd the module's state dict (original names), mel [n_mel, F] -> wav [U F] float64.
    emul: operands (weights, and every convolution's input after its leaky ReLU) rounded to bf16, the tensor between a resblock's two
    convolutions stored as bf16, the resblock mean as a multiply by fp32(1 / K); everything else float64."""
    p = {k: v.detach().cpu().double().numpy() for k, v in sd.items()}
    mel = np.asarray(mel, dtype=np.float64)
    if mel.shape[1] == 0:
        return np.zeros(0)
    K = len(cfg["resblock_kernel_sizes"])
    x = _conv(mel.T, p["conv_pre.weight"], p["conv_pre.bias"], 1, 1.0, emul)
    for i, u in enumerate(cfg["upsample_rates"]):
        x = _up(x, p[f"ups.{i}.weight"], p[f"ups.{i}.bias"], u, SLOPE, emul)
        total = None
        for j, ds in enumerate(cfg["resblock_dilation_sizes"]):
            q, xs = f"resblocks.{i * K + j}.", x
            for m, d in enumerate(ds):
                if resblock == "1":
                    t = _conv(xs, p[q + f"convs1.{m}.weight"], p[q + f"convs1.{m}.bias"], d, SLOPE, emul)
                    if emul:
                        t = R64.bf16_round(t.astype(np.float32))
                    xs = _conv(t, p[q + f"convs2.{m}.weight"], p[q + f"convs2.{m}.bias"], 1, SLOPE, emul) + xs
                else:
                    xs = _conv(xs, p[q + f"convs.{m}.weight"], p[q + f"convs.{m}.bias"], d, SLOPE, emul) + xs
            total = xs if total is None else total + xs
        x = total * float(np.float32(1.0 / K)) if emul else total / K
    return np.tanh(_conv(x, p["conv_post.weight"], p["conv_post.bias"], 1, 0.01, emul))[:, 0]


def rel_l2(a, b):
    return float(np.linalg.norm(np.asarray(a) - np.asarray(b)) / max(np.linalg.norm(np.asarray(b)), 1e-300))


# ----------------------------------------------------------------------------- a straightforward torch generator
def _wn(m, on):
    if not on:
        return m
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return nn.utils.weight_norm(m)


class _TorchResBlock(nn.Module):
    def __init__(self, kind, C, k, dilations, wn):
        super().__init__()
        self.kind = kind
        mk = lambda d: _wn(nn.Conv1d(C, C, k, 1, dilation=d, padding=d * (k - 1) // 2), wn)  # noqa: E731
        if kind == "1":
            self.convs1 = nn.ModuleList(mk(d) for d in dilations)
            self.convs2 = nn.ModuleList(mk(1) for _ in dilations)
        else:
            self.convs = nn.ModuleList(mk(d) for d in dilations)

    def forward(self, x):
        if self.kind == "1":
            for c1, c2 in zip(self.convs1, self.convs2):
                x = c2(F.leaky_relu(c1(F.leaky_relu(x, SLOPE)), SLOPE)) + x
        else:
            for c in self.convs:
                x = c(F.leaky_relu(x, SLOPE)) + x
        return x


class TorchGenerator(nn.Module):
    """the published generator with torch's own convolutions; weight_norm=True gives the checkpoint form (weight_g / weight_v)"""

    def __init__(self, cfg, resblock="1", n_mel=80, weight_norm=False):
        super().__init__()
        rates, kernels, C0 = cfg["upsample_rates"], cfg["upsample_kernel_sizes"], cfg["upsample_initial_channel"]
        self.K = len(cfg["resblock_kernel_sizes"])
        self.conv_pre = _wn(nn.Conv1d(n_mel, C0, 7, 1, padding=3), weight_norm)
        self.ups = nn.ModuleList(_wn(nn.ConvTranspose1d(C0 >> i, C0 >> (i + 1), k, u, padding=(k - u) // 2), weight_norm)
                                 for i, (u, k) in enumerate(zip(rates, kernels)))
        self.resblocks = nn.ModuleList(_TorchResBlock(resblock, C0 >> (i + 1), k, d, weight_norm) for i in range(len(rates))
                                       for k, d in zip(cfg["resblock_kernel_sizes"], cfg["resblock_dilation_sizes"]))
        self.conv_post = _wn(nn.Conv1d(C0 >> len(rates), 1, 7, 1, padding=3), weight_norm)

    def forward(self, x):
        x = self.conv_pre(x)
        for i, up in enumerate(self.ups):
            x = up(F.leaky_relu(x, SLOPE))
            xs = None
            for j in range(self.K):
                y = self.resblocks[i * self.K + j](x)
                xs = y if xs is None else xs + y
            x = xs / self.K
        return torch.tanh(self.conv_post(F.leaky_relu(x)))

    def remove_weight_norm(self):
        for m in self.modules():
            if hasattr(m, "weight_g"):
                nn.utils.remove_weight_norm(m)
        return self


def random_mel(rng, n_mel, frames):
    """log-mel-like values: the range of log(clamp(mel, 1e-5)) on speech"""
    return rng.uniform(-11.5, 1.5, (n_mel, frames)).astype(np.float32)
