"""The two small kernels the conv GEMM's fused epilogues were only ever compared with, against float64 under the rule of
oracle/rows64.py, between guards (oracle/guards.py), with planted defects:

  gt_relu_drop_bwd (csrc/flow_ops.hip)   dc = bf16(d * fp32(1 / (1 - p))) where the saved y is not +-0, else exactly 0: one fp32
                                         rounding, bound u |ref| (+ the bf16 output's own rounding).  Defects: -0 taken as non-zero
                                         (a 0xffff mask for 0x7fff), the scale left out.
  gt_colsum (csrc/conv_wgrad.hip)        out[n] += sum_m Y[m, n], bf16 or fp32 rows, 128-row slabs added with one atomic each:
                                         R + ceil(R / 128) + 1 additions in any order -> gamma_K * (sum |Y| + |prior|).
                                         Defects: the last row left out, the prior overwritten instead of accumulated into."""
import numpy as np
import pytest
import torch

from oracle import dropmask as DM
from oracle import rows64 as R64
from oracle.guards import Guards
from oracle.rows64 import RHO, check_with_control, gamma

pytestmark = pytest.mark.gpu
F32, BF16 = torch.float32, torch.bfloat16
SHAPES = [(R, N) for R in (1, 65, 513) for N in (8, 80, 768)]


def dev():
    return torch.device("cuda:0")


def api():
    from glow_tts_amd import _lib
    return _lib.call, _lib.current_stream(dev())


def bf16_rows(bits, ld):
    R, n = bits.shape
    full = np.full((R, ld), 0x7FC0, dtype=np.uint16)                # NaN past the columns
    full[:, :n] = bits
    return torch.from_numpy(full.view(np.int16)).view(BF16)


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("R,N", SHAPES)
def test_relu_drop_bwd_against_float64(built, R, N, p):
    call, st = api()
    g = np.random.default_rng(R * 1000 + N)
    d = R64.f2bf(g.standard_normal((R, N)).astype(np.float32))
    y = R64.f2bf(np.maximum(g.standard_normal((R, N)), 0).astype(np.float32))
    y[g.random((R, N)) < 0.2] = 0x8000                              # -0: a zero
    y[0, 0], y[0, 1], y[0, 2] = 0x0000, 0x8000, 0x3F80              # every kind in every shape
    G = Guards(dev())
    out = G.out("dc", (R, N + 8), BF16, keep=torch.arange(N + 8) >= N)
    call.gt_relu_drop_bwd(G.inp(bf16_rows(d, N + 16)), N + 16, G.inp(bf16_rows(y, N + 24)), N + 24, out, N + 8, R, N, float(p), st)
    G.verify()
    dv = torch.from_numpy(R64.bf2f(d).astype(np.float64))
    scale = float(DM.scale(p)) if p else 1.0
    ref = torch.where(torch.from_numpy((y & 0x7FFF) != 0), dv * scale, torch.zeros_like(dv))
    bads = {"minus_zero_kept": torch.where(torch.from_numpy(y != 0), dv * scale, torch.zeros_like(dv))}
    if p:
        bads["no_scale"] = ref / scale
    got = out[:, :N]
    check_with_control(f"gt_relu_drop_bwd R={R} N={N} p={p}", got, ref, RHO["f32"] * ref.abs(), bads, kind="bf16")
    assert bool((got.float().cpu()[ref == 0] == 0).all())          # exact zeros where the saved activation is +-0


@pytest.mark.parametrize("is_f32", [False, True])
@pytest.mark.parametrize("R,N", SHAPES)
def test_colsum_accumulates_against_float64(built, R, N, is_f32):
    call, st = api()
    g = np.random.default_rng(R * 1000 + N + 7)
    Y = g.standard_normal((R, N)).astype(np.float32)
    prior = g.standard_normal(N).astype(np.float32)
    G = Guards(dev())
    out = G.out("colsum", (N,), F32, prior=torch.from_numpy(prior))
    ld = N + 8
    if is_f32:
        full = np.full((R, ld), np.nan, dtype=np.float32)
        full[:, :N] = Y
        rows = torch.from_numpy(full)
    else:
        rows = bf16_rows(R64.f2bf(Y), ld)
        Y = R64.bf2f(R64.f2bf(Y))
    call.gt_colsum(G.inp(rows), ld, int(is_f32), out, R, N, st)
    G.verify()
    Yd, pr = torch.from_numpy(Y.astype(np.float64)), torch.from_numpy(prior.astype(np.float64))
    ref = Yd.sum(0) + pr
    bound = gamma(R + -(-R // 128) + 1) * (Yd.abs().sum(0) + pr.abs())
    check_with_control(f"gt_colsum R={R} N={N} {'fp32' if is_f32 else 'bf16'}", out, ref, bound,
                       {"last_row": ref - Yd[-1], "overwritten": ref - pr}, kind="f32")
