"""GPU tests of single gt_voc_conv launches (csrc/hifigan.hip) in float64 on the kernel's OWN operands: the decoded
weight image, and the input after the stated prologue (fp32 leaky ReLU in numpy float32, rounded to bf16).  The rule is the project's
(oracle/rows64.py): elementwise |got - ref| <= gamma(K) S + eps_epi + rho_out |ref| with K = taps Cin + 3, S the absolute-value twin
including |bias| + |res| + |acc|, eps_epi = FAST_FN where tanh is on; the aggregate checks AGG_F32 / AGG_BF16; and two planted defects
that the same checks must miss by >= 3x — one weight entry of the LAST tap zeroed, one input position at a tile edge zeroed.  No
element is excluded.  With M = gt_voc_tile_positions():

  1 widest halo    taps 11, dil 5, Cin = N = 32, slope 0.1, fp32 in, bf16 out; lengths 0, 1, 24, 25, 26, M - 1, M, M + 1, 2M + 3
  2 conv_pre       taps 7, Cin 80 from the channel-major mel (stride_c != F, stride_b padded), slope 1, N = 64, fp32 out
  3 upsampling     taps 3, Cin 32, N = 8 * 16, slope 0.1; read back as [8 L, 16] against float64 conv_transpose1d of the unrearranged
                   weights, lengths 1, 2, M + 1
  4 conv_post      taps 7, Cin 32, N = 1, slope 0.01, tanh, fp32 out at a row pitch larger than L (lengths through len_mul = 4)
  5 epilogue       res, acc and scale = 1/3 together with Y aliasing acc; bf16 input, fp32 output (Cin = N = 64)
  6 tap arithmetic dilation 3 with taps 7 (Cin 64, N 160) and dilation 1 with taps 3 (Cin 64, N 16) on one batch, one count past L_cap

In every case NaN lies behind each utterance's end in X, res and acc; the outputs must be finite and exactly 0 in [len_b, L_cap), and
the canaries (oracle.guards.Guards) around every output intact.  Together the cases run all six instantiations of the kernel."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hifigan64 as H  # noqa: E402
from oracle import rows64 as R64  # noqa: E402

pytestmark = pytest.mark.gpu


def dev():
    return torch.device("cuda:0")


def tile():
    from glow_tts_amd import _lib
    return _lib.lib().gt_voc_tile_positions()


def bf16_exact(a):
    return R64.bf2f(R64.f2bf(np.asarray(a, dtype=np.float32)))


def launch(rng, name, lens, taps, dil, Cin, N, slope, n_frames=None, len_mul=1, x_mel=False, x_bf16=False, y_bf16=False, tanh=False,
           with_res=False, with_acc=False, scale=1.0, alias_acc=False, y_pitch=None, W=None, bias=None, ref_fn=None):
    """one launch on a ragged batch and the rule on all of its valid outputs; returns the passing report"""
    from glow_tts_amd import _lib, audio
    from oracle.guards import Guards
    L = _lib.lib()
    B, L_cap, M = len(lens), max(lens) + 2, tile()
    if n_frames is None:
        n_frames = list(lens)
    lens = [min(max(v, 0) * len_mul, L_cap) for v in n_frames]
    g = Guards(dev())
    W = (rng.standard_normal((N, Cin, taps)) / np.sqrt(taps * Cin)).astype(np.float32) if W is None else W
    bias = rng.standard_normal(N).astype(np.float32) if bias is None else bias
    xs = [rng.standard_normal((n, Cin)).astype(np.float32) for n in lens]
    if x_bf16:
        xs = [bf16_exact(x) for x in xs]
    # ---- device operands: NaN behind every utterance's end
    if x_mel:
        sc = L_cap + 5
        sb = Cin * sc + 24
        xh = np.full((B, sb), np.nan, dtype=np.float32)
        for b, x in enumerate(xs):
            xh[b, :Cin * sc].reshape(Cin, sc)[:, :lens[b]] = x.T
        X = g.inp(torch.from_numpy(xh).to(dev()))
        x_sb, x_sc = sb, sc
    else:
        xh = np.full((B, L_cap, Cin), np.nan, dtype=np.float32)
        for b, x in enumerate(xs):
            xh[b, :lens[b]] = x
        X = g.inp(torch.from_numpy(xh).to(dev()).to(torch.bfloat16 if x_bf16 else torch.float32))
        x_sb, x_sc = L_cap * Cin, 0
    img = g.inp(audio.voc_pack(torch.from_numpy(W).to(dev())))
    side = {}
    for key, on in (("res", with_res), ("acc", with_acc)):
        if on:
            h = np.full((B, L_cap, N), np.nan, dtype=np.float32)
            for b in range(B):
                h[b, :lens[b]] = rng.standard_normal((lens[b], N)).astype(np.float32)
            side[key] = h
    res = g.inp(torch.from_numpy(side["res"]).to(dev())) if with_res else None
    if y_pitch is not None:                                                        # N == 1: rows of `y_pitch` elements, L_cap used
        assert N == 1 and y_pitch > L_cap
        keep = torch.zeros(B, y_pitch, dtype=torch.bool)
        keep[:, L_cap:] = True
        Y = g.out("Y", (B, y_pitch), keep=keep)
        y_sb, ldy = y_pitch, 1
    elif alias_acc:
        Y = g.out("Y", (B, L_cap, N), prior=torch.from_numpy(side["acc"]))
        y_sb, ldy = L_cap * N, N
    else:
        Y = g.out("Y", (B, L_cap, N), dtype=torch.bfloat16 if y_bf16 else torch.float32)
        y_sb, ldy = L_cap * N, N
    acc = Y if alias_acc else (g.inp(torch.from_numpy(side["acc"]).to(dev())) if with_acc else None)
    a = _lib.fill_args(_lib.VocConvArgs, X=X, x_stride_b=x_sb, x_stride_c=x_sc, W=img, bias=g.inp(torch.from_numpy(bias).to(dev())),
                       res=res, acc=acc, Y=Y, y_stride_b=y_sb, ldy=ldy, len_mul=len_mul,
                       n_frames=torch.tensor(n_frames, dtype=torch.int32, device=dev()), B=B, L_cap=L_cap, Cin=Cin, N=N, taps=taps,
                       dil=dil, x_bf16=int(x_bf16), x_mel=int(x_mel), y_bf16=int(y_bf16), tanh_out=int(tanh), slope=slope, scale=scale)
    assert ((L_cap + M - 1) // M) * B <= 64                                        # a few dozen workgroup rows: a quick launch
    _lib.call.gt_voc_conv(a, _lib.current_stream(dev()))
    g.verify()                                                                     # canaries intact, nothing unwritten, no NaN
    got = Y.float().cpu().double().numpy()
    got = got[:, :L_cap].reshape(B, L_cap, 1) if y_pitch is not None else got
    # ---- float64 on the kernel's own operands
    W64 = H.decode_image(img, N, Cin, taps, L.gt_voc_k_chunk(Cin))
    assert np.array_equal(W64, bf16_exact(W).astype(np.float64).transpose(2, 0, 1))
    sc64 = float(np.float32(scale))
    K = taps * Cin + 3
    b_long = int(np.argmax(lens))
    edge = M if lens[b_long] > M else lens[b_long] - 1                            # the first position of the second tile
    Wbad = W64.copy()
    Wbad[taps - 1, :, Cin // 3] = 0

    def reference(Wt, zero_pos=None):
        outs, bounds = [], []
        for b in range(B):
            xo = H.prologue(xs[b], slope)
            if zero_pos is not None and b == b_long:
                xo = xo.copy()
                xo[zero_pos] = 0
            y, s = ref_fn(xo, Wt) if ref_fn is not None else H.conv64(xo, Wt, taps, dil)
            y, s = y + bias.astype(np.float64), s + np.abs(bias.astype(np.float64))
            for key in side:
                v = side[key][b, :lens[b]].astype(np.float64)
                y, s = y + v, s + np.abs(v)
            y, bound = y * sc64, R64.gamma(K) * s * abs(sc64)
            if tanh:
                y, bound = np.tanh(y), bound + R64.FAST_FN                        # |tanh'| <= 1
            outs.append(y)
            bounds.append(bound)
        return np.concatenate(outs), np.concatenate(bounds)

    ref, bound = reference(W64)
    bad = {"last tap's weight entry zeroed": reference(Wbad)[0], "tile-edge input position zeroed": reference(W64, edge)[0]}
    got_valid = np.concatenate([got[b, :lens[b]] for b in range(B)])
    assert got_valid.shape == ref.shape and ref.size == sum(lens) * N
    for b in range(B):
        assert np.isfinite(got[b]).all() and not got[b, lens[b]:].any(), (name, b)  # exact zeros in [len_b, L_cap)
    return R64.check_with_control(name, torch.from_numpy(got_valid), torch.from_numpy(ref), torch.from_numpy(bound),
                                  {k: torch.from_numpy(v) for k, v in bad.items()}, kind="bf16" if y_bf16 else "f32")


def test_widest_halo(built):
    M = tile()
    launch(np.random.default_rng(1), "widest halo", [0, 1, 24, 25, 26, M - 1, M, M + 1, 2 * M + 3], 11, 5, 32, 32, 0.1, y_bf16=True)


def test_conv_pre_from_the_channel_major_mel(built):
    M = tile()
    launch(np.random.default_rng(2), "conv_pre", [0, 1, 3, 7, 40, M + 1], 7, 1, 80, 64, 1.0, x_mel=True)


def test_upsampling_form_against_conv_transpose1d(built):
    from glow_tts_amd import audio
    M, u, Cout, Cin = tile(), 8, 16, 32
    rng = np.random.default_rng(3)
    w = bf16_exact(rng.standard_normal((Cin, Cout, 2 * u)) / np.sqrt(2 * Cin))    # ConvTranspose1d's [Cin, Cout, k], exact in bf16
    b = rng.standard_normal(Cout).astype(np.float32)
    W3 = audio.transposed_as_conv(torch.from_numpy(w), u).numpy()

    def transposed(xo, Wt):
        """float64 conv_transpose1d of the UNREARRANGED weights (Wt only says whether the defect's weights are asked for), flattened
        to the kernel's [L, u Cout]"""
        import torch.nn.functional as F
        wt = torch.from_numpy(w).double()
        if not np.array_equal(Wt, torch.from_numpy(W3).double().numpy().transpose(2, 0, 1)):
            return H.conv64(xo, Wt, 3, 1)
        x = torch.from_numpy(xo).t()[None]
        y = F.conv_transpose1d(x, wt, None, stride=u, padding=u // 2)[0]          # [Cout, u L]
        s = F.conv_transpose1d(x.abs(), wt.abs(), None, stride=u, padding=u // 2)[0]
        L = xo.shape[0]
        return y.t().reshape(L, u * Cout).numpy(), s.t().reshape(L, u * Cout).numpy()

    launch(rng, "upsampling form", [1, 2, M + 1], 3, 1, Cin, u * Cout, 0.1, W=W3, bias=np.tile(b, u), ref_fn=transposed)


def test_conv_post(built):
    M = tile()
    launch(np.random.default_rng(4), "conv_post", [0, 4, 32, M + 4], 7, 1, 32, 1, 0.01, n_frames=[0, 1, 8, (M + 4) // 4], len_mul=4,
           tanh=True, y_pitch=M + 4 + 2 + 9)


def test_epilogue_res_acc_scale_aliasing(built):
    M = tile()
    launch(np.random.default_rng(5), "epilogue", [0, 5, M + 1, 77], 3, 1, 64, 64, 0.1, x_bf16=True, with_res=True, with_acc=True,
           scale=1.0 / 3.0, alias_acc=True)


@pytest.mark.parametrize("taps,dil,N", [(7, 3, 160), (3, 1, 16)])
def test_tap_and_dilation_arithmetic(built, taps, dil, N):
    M = tile()
    lens = [M + 30, 9, M - 1, 2]
    launch(np.random.default_rng(6), f"taps {taps} dil {dil}", lens, taps, dil, 64, N, 0.1, n_frames=[M + 30 + 2 + 7, 9, M - 1, 2])
