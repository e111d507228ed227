"""GPU tests of single gt_voc_snake launches (csrc/voc_snake.hip) in float64 on the kernel's OWN operands: the fp32
input and the fp32 parameter block, by the closed form of tests/bigvgan64.py (act64, which agrees with the four torch operations:
tests/test_bigvgan_host.py).  The rule is the project's (oracle/rows64.py): elementwise |got - ref| <= bound + rho_bf16 |ref|, where
bound carries gamma(6) over u's absolute-value twin through the snake (the argument's own rounding ULP |a u| and the device sinf's
EPS_SIN, times 2 / beta') and gamma(12) over y's twin (bigvgan64.act64 derives it); AGG_BF16 on the aggregate; no element is excluded.
Two planted defects in the reference that the same checks must miss by >= 3x: v evaluated past the utterance's end from the clamped x
instead of replicated, and the window clamped at a tile edge inside the utterance.  With M = gt_voc_snake_tile_positions():

  lengths          0, 1, 2, 5, 6, 7, 11, 12, M - 1, M, M + 1, 2M + 3 in one batch, at C = 16, 48 and 160
  len_mul          4, with one count past L_cap, at padded strides
  parameters       snake (beta' = alpha') and snakebeta; alpha' 0.1 .. 7 (log-uniform), |x| up to 10

NaN lies behind every utterance's end in X; the outputs must be finite and exactly 0 in [len_b, L_cap), the canaries
(oracle.guards.Guards) intact, and every batch row bit-equal to its utterance launched alone at another capacity."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bigvgan64 as G  # noqa: E402
from oracle import rows64 as R64  # noqa: E402

pytestmark = pytest.mark.gpu


def dev():
    return torch.device("cuda:0")


def tile():
    from glow_tts_amd import _lib
    return _lib.lib().gt_voc_snake_tile_positions()


def block(rng, C, kind):
    """(P fp32 [2 C + 24], a, ib, fu, fd as the float64 values of its entries)"""
    a = np.exp(rng.uniform(np.log(0.1), np.log(7.0), C))
    b = a if kind == "snake" else np.exp(rng.uniform(np.log(0.1), np.log(7.0), C))
    f = G.filter64()
    P = np.concatenate([a, 1.0 / (b + 1e-9), f, f]).astype(np.float32)
    P64 = P.astype(np.float64)
    return P, P64[:C], P64[C:2 * C], P64[2 * C:2 * C + 12], P64[2 * C + 12:]


def run(X, P, n_frames, len_mul, B, L_cap, C, x_sb, y_sb, guards=None):
    """one launch; X a device fp32 buffer of B rows of pitch x_sb -> bf16 [B, y_sb] as float64 numpy"""
    from glow_tts_amd import _lib
    if guards is None:
        Y = torch.full((B, y_sb), 768.0, dtype=torch.bfloat16, device=dev())
    else:
        keep = torch.zeros(B, y_sb, dtype=torch.bool)
        keep[:, L_cap * C:] = True
        Y = guards.out("Y", (B, y_sb), dtype=torch.bfloat16, keep=keep)
    a = _lib.fill_args(_lib.VocSnakeArgs, X=X, x_stride_b=x_sb, P=P, Y=Y, y_stride_b=y_sb, len_mul=len_mul,
                       n_frames=torch.tensor(n_frames, dtype=torch.int32, device=dev()), B=B, L_cap=L_cap, C=C)
    _lib.call.gt_voc_snake(a, _lib.current_stream(dev()))
    if guards is not None:
        guards.verify()
    torch.cuda.synchronize()
    return Y


def launch(seed, name, n_frames, C, kind, len_mul=1, L_cap=None, pad=0):
    from oracle.guards import Guards
    rng = np.random.default_rng(seed)
    M = tile()
    B = len(n_frames)
    L_cap = max(n_frames) * len_mul + 2 if L_cap is None else L_cap
    lens = [min(max(v, 0) * len_mul, L_cap) for v in n_frames]
    assert ((L_cap + M - 1) // M) * B * ((C + 31) // 32) <= 256                     # a quick launch
    P, a, ib, fu, fd = block(rng, C, kind)
    xs = [rng.uniform(-10, 10, (n, C)).astype(np.float32) for n in lens]
    x_sb, y_sb = L_cap * C + pad, L_cap * C + 2 * pad
    xh = np.full((B, x_sb), np.nan, dtype=np.float32)                               # NaN behind every utterance's end and in the pitch
    for b, x in enumerate(xs):
        xh[b, :lens[b] * C] = x.reshape(-1)
    g = Guards(dev())
    X, Pd = g.inp(torch.from_numpy(xh).to(dev())), g.inp(torch.from_numpy(P).to(dev()))
    Y = run(X, Pd, n_frames, len_mul, B, L_cap, C, x_sb, y_sb, guards=g)
    got = Y.float().cpu().double().numpy()[:, :L_cap * C].reshape(B, L_cap, C)
    for b in range(B):
        assert np.isfinite(got[b]).all() and not got[b, lens[b]:].any(), (name, b)  # exact zeros in [len_b, L_cap)
    # ---- batch independence and the capacity form: each utterance alone, at another capacity, bit for bit
    for b in range(B):
        cap = lens[b] + 1 + b
        xa = np.full((1, cap * C), np.nan, dtype=np.float32)
        xa[0, :lens[b] * C] = xs[b].reshape(-1)
        alone = run(torch.from_numpy(xa).to(dev()), Pd, [lens[b]], 1, 1, cap, C, cap * C, cap * C)
        assert torch.equal(alone.view(cap, C)[:lens[b]].cpu(), Y[b, :lens[b] * C].view(lens[b], C).cpu()), (name, b)
        assert not alone.view(cap, C)[lens[b]:].float().abs().any()
    # ---- float64 on the kernel's own operands, and the two planted defects
    b_long = int(np.argmax(lens))
    assert lens[b_long] > M                                                         # the tile-edge defect needs a second tile
    refs = {d: [G.act64(x.astype(np.float64), a, ib, fu, fd, defect=d, edge=M if i == b_long else None) for i, x in enumerate(xs)]
            for d in (None, "v_past_end", "tile_clamp")}
    cat = lambda parts, k: torch.from_numpy(np.concatenate([p[k].reshape(-1) for p in parts]))  # noqa: E731
    got_valid = torch.from_numpy(np.concatenate([got[b, :lens[b]].reshape(-1) for b in range(B)]))
    assert got_valid.numel() == sum(lens) * C
    return R64.check_with_control(name, got_valid, cat(refs[None], 0), cat(refs[None], 1),
                                  {"v evaluated past the end from the clamped x": cat(refs["v_past_end"], 0),
                                   "window clamped at a tile edge": cat(refs["tile_clamp"], 0)}, kind="bf16")


@pytest.mark.parametrize("C,kind", [(16, "snakebeta"), (48, "snake"), (160, "snakebeta")])
def test_lengths_at_every_edge(built, C, kind):
    M = tile()
    launch(C, f"lengths, C = {C}, {kind}", [0, 1, 2, 5, 6, 7, 11, 12, M - 1, M, M + 1, 2 * M + 3], C, kind)


def test_len_mul_past_capacity_and_padded_strides(built):
    M = tile()
    L_cap = M + 24
    launch(9, "len_mul 4, padded strides", [0, 1, 3, (M + 24) // 4 + 5, 16], 32, "snakebeta", len_mul=4, L_cap=L_cap, pad=8)
