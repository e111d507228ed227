"""TEST INFRASTRUCTURE ONLY — float64 restatements for the BigVGAN vocoder (csrc/voc_snake.hip, audio.BigVGAN) and the
case lists of its tests.  A plain helper like tests/hifigan64.py, whose convolutions it reuses.

  filter64          the 12-tap Kaiser-windowed sinc of both resamplers, from its formula
  snake_params      (alpha, beta, activation, logscale) -> (alpha', 1 / (beta' + 1e-9)) in float64: gt_voc_snake's per-channel pair
  act64_torch       Activation1d on one utterance by the four torch operations (replicate pad, conv_transpose1d, snake, replicate pad,
                    strided conv1d) in float64
  act64             the closed form with explicit loops, its error bound for the kernel's fp32 arithmetic, and the two planted defects
  generator64       the generator on ONE utterance (emul=True: bf16 where the device rounds)
  TorchBigVGAN      a straightforward torch writing with the published module tree (optional weight norm): the source of state dicts
                    and the second, independent writing of the definition
"""
import os
import sys

import numpy as np
import torch
from torch import nn
from torch.nn import functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hifigan64 as H  # noqa: E402
from oracle import rows64 as R64  # noqa: E402

TINY = dict(upsample_rates=(4, 2), upsample_kernel_sizes=(8, 4), upsample_initial_channel=64, resblock_kernel_sizes=(3, 7, 11),
            resblock_dilation_sizes=((1, 3, 5),) * 3)
TINY24 = dict(TINY, upsample_rates=(2, 2), upsample_kernel_sizes=(4, 4), upsample_initial_channel=96)
TINY32 = dict(TINY24, upsample_initial_channel=128)      # TINY24's padded widths as a configuration of its own: 128 -> 64 -> 32
BASE = dict(upsample_rates=(8, 8, 2, 2), upsample_kernel_sizes=(16, 16, 4, 4), upsample_initial_channel=512,
            resblock_kernel_sizes=(3, 7, 11), resblock_dilation_sizes=((1, 3, 5),) * 3)
# the published base model's config.json (22 kHz, 80 bands), the keys from_config reads
BASE_CONFIG = dict(BASE, resblock="1", num_mels=80, activation="snakebeta", snake_logscale=True, upsample_rates=[8, 8, 2, 2],
                   upsample_kernel_sizes=[16, 16, 4, 4], resblock_kernel_sizes=[3, 7, 11],
                   resblock_dilation_sizes=[[1, 3, 5], [1, 3, 5], [1, 3, 5]])
TINY_FRAMES = (13, 1, 2, 40, 0, 7)
FILTER = (0.00202896644989624, 0.00938946394406788, -0.02554346406529466, -0.05765737547536495, 0.12857260908132875,
          0.4432098000653667)
EPS_SIN = 2.0 ** -23           # the device library's sinf: 2 ulp (the HIP math API's stated maximum) of a value below 1, absolute
ULP = 2.0 ** -24               # one fp32 rounding, relative


def filter64():
    """kaiser_sinc_filter1d(cutoff 0.25, half_width 0.3, kernel_size 12) in float64"""
    A = 2.285 * 5 * np.pi * 1.2 + 7.95
    assert A > 50
    w = torch.kaiser_window(12, periodic=False, beta=0.1102 * (A - 8.7), dtype=torch.float64).numpy()
    time = np.arange(-6, 6) + 0.5
    f = 0.5 * w * np.sinc(0.5 * time)
    return f / f.sum()


def snake_params(alpha, beta, activation, logscale):
    al = np.asarray(alpha, dtype=np.float64)
    be = np.asarray(beta, dtype=np.float64) if activation == "snakebeta" else al
    if logscale:
        al, be = np.exp(al), np.exp(be)
    return al, 1.0 / (be + 1e-9)


def act64_torch(x, a, ib, fu=None, fd=None):
    """x [L, C] float64 (one utterance, channels-last), a = alpha', ib = 1 / (beta' + 1e-9) [C] -> y [L, C]: the four torch operations"""
    fu = filter64() if fu is None else np.asarray(fu, dtype=np.float64)
    fd = filter64() if fd is None else np.asarray(fd, dtype=np.float64)
    L, C = x.shape
    if L == 0:
        return np.zeros((0, C))
    xt = torch.from_numpy(np.ascontiguousarray(x.T))[None]                         # [1, C, L]
    wu = torch.from_numpy(fu).view(1, 1, 12).expand(C, 1, 12).contiguous()
    wd = torch.from_numpy(fd).view(1, 1, 12).expand(C, 1, 12).contiguous()
    xp = F.pad(xt, (5, 5), mode="replicate")
    u = 2 * F.conv_transpose1d(xp, wu, stride=2, groups=C)[..., 15:-15]
    at, ibt = torch.from_numpy(np.asarray(a, dtype=np.float64)).view(1, C, 1), torch.from_numpy(np.asarray(ib, dtype=np.float64)).view(1, C, 1)
    v = u + ibt * torch.sin(at * u) ** 2
    vp = F.pad(v, (5, 6), mode="replicate")
    return F.conv1d(vp, wd, stride=2, groups=C)[0].t().numpy()


def act64(x, a, ib, fu=None, fd=None, defect=None, edge=None):
    """The closed form with explicit loops: x [L, C] -> (y [L, C], bound [L, C]).

      u[2q] = 2 sum_j f[11 - 2j] x[cl(q - 3 + j)],  u[2q + 1] = 2 sum_j f[10 - 2j] x[cl(q - 2 + j)],  v = u + ib sin^2(a u),
      y[t] = sum_k f[k] v[min(max(2t + k - 5, 0), 2L - 1)]

    bound: what the kernel's fp32 arithmetic may differ by, before the output's own bf16 rounding.  With Su the absolute-value twin of u
    (a 6-term fmaf chain: gamma(6) Su), the argument a u rounded once (ULP |a u|), sinf within EPS_SIN, |d sin^2| <= 2 |d sin| + ULP,
    the fmaf into v rounded once:
        e_v = gamma(6) Su (1 + 2 a ib) + ib (2 (ULP |a u| + EPS_SIN) + ULP) + ULP |v|
        bound[t] = sum_k |f[k]| e_v[.] + gamma(12) sum_k |f[k]| |v[.]|
    defect "v_past_end": v evaluated at out-of-range indices from the clamped x instead of replicated.
    defect "tile_clamp": the outputs from position `edge` on computed as if the utterance began there (the window clamped at a tile edge)."""
    fu = filter64() if fu is None else np.asarray(fu, dtype=np.float64)
    fd = filter64() if fd is None else np.asarray(fd, dtype=np.float64)
    x = np.asarray(x, dtype=np.float64)
    L, C = x.shape
    if L == 0:
        return np.zeros((0, C)), np.zeros((0, C))
    if defect == "tile_clamp":
        y, bound = act64(x, a, ib, fu, fd)
        if edge is not None and 0 < edge < L:
            y = y.copy()
            y[edge:] = act64(x[edge:], a, ib, fu, fd)[0]
        return y, bound
    a, ib = np.asarray(a, dtype=np.float64), np.asarray(ib, dtype=np.float64)
    cl = lambda i: min(max(i, 0), L - 1)  # noqa: E731
    lo = -6 if defect == "v_past_end" else 0                                       # v's index range held: [lo, 2L - lo)
    n = 2 * L - 2 * lo
    u, su = np.zeros((n, C)), np.zeros((n, C))
    for i in range(lo, 2 * L - lo):
        q, odd = i // 2, i % 2                                                     # floor division: i = 2q + odd for negative i too
        for j in range(6):
            f = fu[10 - 2 * j] if odd else fu[11 - 2 * j]
            xv = x[cl(q - 2 + j)] if odd else x[cl(q - 3 + j)]
            u[i - lo] += 2 * f * xv
            su[i - lo] += 2 * abs(f) * np.abs(xv)
    v = u + ib * np.sin(a * u) ** 2
    e_v = R64.gamma(6) * su * (1 + 2 * a * ib) + ib * (2 * (ULP * np.abs(a * u) + EPS_SIN) + ULP) + ULP * np.abs(v)
    y, bound = np.zeros((L, C)), np.zeros((L, C))
    for t in range(L):
        for k in range(12):
            i = 2 * t + k - 5
            if defect != "v_past_end":
                i = min(max(i, 0), 2 * L - 1)
            y[t] += fd[k] * v[i - lo]
            bound[t] += abs(fd[k]) * (e_v[i - lo] + R64.gamma(12) * np.abs(v[i - lo]))
    return y, bound


# ----------------------------------------------------------------------------- the generator on one utterance
def _act(x, p, prefix, cfg, emul):
    a, ib = snake_params(p[prefix + "act.alpha"], p.get(prefix + "act.beta"), cfg.get("activation", "snakebeta"),
                         cfg.get("snake_logscale", True))
    if emul:                                                                       # the parameter block is fp32
        a, ib = a.astype(np.float32).astype(np.float64), ib.astype(np.float32).astype(np.float64)
    y = act64_torch(x, a, ib, p[prefix + "upsample.filter"].reshape(-1), p[prefix + "downsample.lowpass.filter"].reshape(-1))
    return R64.bf16_round(y.astype(np.float32)) if emul else y


def generator64(sd, cfg, mel, emul=False):
    """the generator on ONE utterance: sd a state dict under the published names (weight norm removed), cfg the constructor's keywords
    (resblock, activation, snake_logscale, use_tanh_at_final ... with the constructor's defaults), mel [n_mel, F] -> wav [U F] float64.
    emul: bf16 exactly where the device rounds — every activation's output, the packed weights, and gt_voc_conv's own rounding of the
    two fp32 inputs that meet no activation (the mel, and the input of a transposed convolution); the resblock mean as a multiply by
    fp32(1 / K); everything else float64."""
    p = {k: v.detach().cpu().double().numpy() for k, v in sd.items()}
    mel = np.asarray(mel, dtype=np.float64)
    if mel.shape[1] == 0:
        return np.zeros(0)
    kind, K = str(cfg.get("resblock", "1")), len(cfg["resblock_kernel_sizes"])
    # hifigan64's convolutions with slope 1: the operand is the input itself (emul: rounded to bf16, a no-op on an activation's output)
    conv = lambda x, name, d: H._conv(x, p[name + ".weight"], p.get(name + ".bias", 0.0), d, 1.0, emul)  # noqa: E731
    x = conv(mel.T, "conv_pre", 1)
    for i, u in enumerate(cfg["upsample_rates"]):
        x = H._up(x, p[f"ups.{i}.0.weight"], p[f"ups.{i}.0.bias"], u, 1.0, emul)
        total = None
        for j, ds in enumerate(cfg["resblock_dilation_sizes"]):
            q, xs = f"resblocks.{i * K + j}.", x
            for m, d in enumerate(ds):
                if kind == "1":
                    t = conv(_act(xs, p, q + f"activations.{2 * m}.", cfg, emul), q + f"convs1.{m}", d)
                    xs = conv(_act(t, p, q + f"activations.{2 * m + 1}.", cfg, emul), q + f"convs2.{m}", 1) + xs
                else:
                    xs = conv(_act(xs, p, q + f"activations.{m}.", cfg, emul), q + f"convs.{m}", d) + xs
            total = xs if total is None else total + xs
        x = total * float(np.float32(1.0 / K)) if emul else total / K
    y = conv(_act(x, p, "activation_post.", cfg, emul), "conv_post", 1)[:, 0]
    return np.tanh(y) if cfg.get("use_tanh_at_final", True) else np.clip(y, -1.0, 1.0)


rel_l2 = H.rel_l2
random_mel = H.random_mel


# ----------------------------------------------------------------------------- a straightforward torch generator
class _Snake(nn.Module):
    def __init__(self, C, logscale, with_beta):
        super().__init__()
        self.logscale = logscale
        self.alpha = nn.Parameter(torch.zeros(C) if logscale else torch.ones(C))
        if with_beta:
            self.beta = nn.Parameter(torch.zeros(C) if logscale else torch.ones(C))

    def forward(self, x):
        alpha = self.alpha[None, :, None]
        beta = self.beta[None, :, None] if hasattr(self, "beta") else alpha
        if self.logscale:
            alpha, beta = torch.exp(alpha), torch.exp(beta)
        return x + (1.0 / (beta + 1e-9)) * torch.sin(x * alpha) ** 2


class _UpSample1d(nn.Module):
    def __init__(self):
        super().__init__()
        self.register_buffer("filter", torch.from_numpy(filter64()).float().view(1, 1, 12))

    def forward(self, x):
        C = x.shape[1]
        x = F.pad(x, (5, 5), mode="replicate")
        x = 2 * F.conv_transpose1d(x, self.filter.to(x.dtype).expand(C, -1, -1), stride=2, groups=C)
        return x[..., 15:-15]


class _LowPassFilter1d(nn.Module):
    def __init__(self):
        super().__init__()
        self.register_buffer("filter", torch.from_numpy(filter64()).float().view(1, 1, 12))

    def forward(self, x):
        C = x.shape[1]
        return F.conv1d(F.pad(x, (5, 6), mode="replicate"), self.filter.to(x.dtype).expand(C, -1, -1), stride=2, groups=C)


class _DownSample1d(nn.Module):
    def __init__(self):
        super().__init__()
        self.lowpass = _LowPassFilter1d()

    def forward(self, x):
        return self.lowpass(x)


class _Activation1d(nn.Module):
    def __init__(self, C, activation, logscale):
        super().__init__()
        self.act = _Snake(C, logscale, activation == "snakebeta")
        self.upsample, self.downsample = _UpSample1d(), _DownSample1d()

    def forward(self, x):
        return self.downsample(self.act(self.upsample(x)))


class _AMPBlock(nn.Module):
    def __init__(self, kind, C, k, dilations, wn, activation, logscale):
        super().__init__()
        self.kind = kind
        mk = lambda d: H._wn(nn.Conv1d(C, C, k, 1, dilation=d, padding=d * (k - 1) // 2), wn)  # noqa: E731
        if kind == "1":
            self.convs1 = nn.ModuleList(mk(d) for d in dilations)
            self.convs2 = nn.ModuleList(mk(1) for _ in dilations)
        else:
            self.convs = nn.ModuleList(mk(d) for d in dilations)
        n = (2 if kind == "1" else 1) * len(dilations)
        self.activations = nn.ModuleList(_Activation1d(C, activation, logscale) for _ in range(n))

    def forward(self, x):
        if self.kind == "1":
            for m, (c1, c2) in enumerate(zip(self.convs1, self.convs2)):
                x = c2(self.activations[2 * m + 1](c1(self.activations[2 * m](x)))) + x
        else:
            for c, a in zip(self.convs, self.activations):
                x = c(a(x)) + x
        return x


class TorchBigVGAN(nn.Module):
    """the published generator with torch's own operations; weight_norm=True gives the checkpoint form (weight_g / weight_v)"""

    def __init__(self, cfg, resblock="1", n_mel=80, weight_norm=False, activation="snakebeta", snake_logscale=True, use_tanh_at_final=True,
                 use_bias_at_final=True):
        super().__init__()
        rates, kernels, C0 = cfg["upsample_rates"], cfg["upsample_kernel_sizes"], cfg["upsample_initial_channel"]
        self.K, self.use_tanh = len(cfg["resblock_kernel_sizes"]), use_tanh_at_final
        self.conv_pre = H._wn(nn.Conv1d(n_mel, C0, 7, 1, padding=3), weight_norm)
        self.ups = nn.ModuleList(nn.ModuleList([H._wn(nn.ConvTranspose1d(C0 >> i, C0 >> (i + 1), k, u, padding=(k - u) // 2), weight_norm)])
                                 for i, (u, k) in enumerate(zip(rates, kernels)))
        self.resblocks = nn.ModuleList(_AMPBlock(str(resblock), C0 >> (i + 1), k, d, weight_norm, activation, snake_logscale)
                                       for i in range(len(rates))
                                       for k, d in zip(cfg["resblock_kernel_sizes"], cfg["resblock_dilation_sizes"]))
        self.activation_post = _Activation1d(C0 >> len(rates), activation, snake_logscale)
        self.conv_post = H._wn(nn.Conv1d(C0 >> len(rates), 1, 7, 1, padding=3, bias=use_bias_at_final), weight_norm)

    def forward(self, x):
        x = self.conv_pre(x)
        for i, up in enumerate(self.ups):
            x = up[0](x)
            xs = None
            for j in range(self.K):
                y = self.resblocks[i * self.K + j](x)
                xs = y if xs is None else xs + y
            x = xs / self.K
        x = self.conv_post(self.activation_post(x))
        return torch.tanh(x) if self.use_tanh else torch.clamp(x, -1.0, 1.0)

    def remove_weight_norm(self):
        for m in self.modules():
            if hasattr(m, "weight_g"):
                nn.utils.remove_weight_norm(m)
        return self


def seeded(cfg, seed, n_mel=16, alpha_range=(-1.0, 1.0), **kw):
    """a TorchBigVGAN with seeded weights and alpha / beta drawn uniformly from alpha_range (log scale: alpha' in [e^-1, e])"""
    torch.manual_seed(seed)
    g = TorchBigVGAN(cfg, n_mel=n_mel, **kw).eval()
    gen = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for name, p in g.named_parameters():
            if name.endswith(".alpha") or name.endswith(".beta"):
                p.copy_(torch.rand(p.shape, generator=gen) * (alpha_range[1] - alpha_range[0]) + alpha_range[0])
    return g
