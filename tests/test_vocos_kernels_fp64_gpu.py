"""GPU tests of single launches of the Vocos kernels (csrc/vocos.hip) in float64 on the kernels' OWN operands, by the
rule of oracle/rows64.py as tests/test_hifigan_fp64_gpu.py applies it: elementwise |got - ref| <= bound + rho_out |ref|, the aggregate
checks AGG_F32 / AGG_BF16, and planted defects that the same checks must miss by >= 3x.  No element is excluded.  In every case NaN lies
behind each utterance's end in every activation input, the outputs must be finite and exactly 0 in [len_b, L_cap), and the canaries
(oracle.guards.Guards) around every output intact.  M = gt_vocos_tile_positions().

  gt_vocos_norm   C = 64 and 512, with and without the depthwise part, fp32 and bf16 out; lengths 0, 1, 3, 4, 7, M - 1, M, M + 1, 2M + 3
                  (the 7-tap halo is 3 positions).  h = bd + sum w x in float64 with e_h = gamma(8) S_h; the LayerNorm's bound is
                  oracle/ln64.py's model line by line (mean, centred values, variance, rsqrtf, two multiplies and the add).  Defects: the
                  last tap's weight of one channel zeroed (depthwise cases); one channel left out of the mean (plain cases).  wd == NULL
                  in place is bit-identical to out of place.
  gt_vocos_mlp    C = 128, H = 2 chunks (lengths 0, 1, M - 1, M, M + 1, 2M + 3, one frame count past L_cap, Y aliasing R) and C = 512,
                  H = 1536 (lengths 5, 9).  With U stored the two stages are checked on the kernel's own operands:
                    stage 1  U against bf16(gelu(float64 pre-activation of the decoded W1 image and A)): 1.13 gamma(C + 2) S (|gelu'| <=
                             1.13) + the fp32 GELU's own roundings 2^-24 (4 |x| + 2 |u|) (erff <= 2 ulp, three multiplies / adds) + one bf16
                             ulp of |u| (a rounding may flip).  Defects: one A position at a tile edge zeroed, one W1 entry zeroed.
                    stage 2  Y against float64 on the stored U and the decoded W2 image: gamma(H + 3) S, S including |b2| + |R|.  Defects:
                             one W2 entry of the LAST hidden chunk zeroed, one U position at a tile edge zeroed.
                  Y is bit-identical with U NULL.
  gt_vocos_polar  against float64 exp / cos / sin through audio.spec_unpack; frames 0, 1, 31, 32, 33 and one past the 64-frame tile;
                  log-magnitudes up to 5 (e^5 > 100: the clip), phases in +-50 rad; all of spec defined, zeros from frame F_b on up to
                  the padded Fp.  Bound 8 u m with u = 2^-24: expf <= 1 ulp (2 u m), cosf / sinf <= 2 ulp of a value <= 1 (4 u m), the
                  product's rounding (u m), one u to spare.  Defect: the clip at 100 left out."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hifigan64 as H  # noqa: E402
import vocos64 as V  # noqa: E402
from oracle import rows64 as R64  # noqa: E402

pytestmark = pytest.mark.gpu
U32 = R64.RHO["f32"]
LENS = lambda M: [0, 1, 3, 4, 7, M - 1, M, M + 1, 2 * M + 3]  # noqa: E731


def dev():
    return torch.device("cuda:0")


def lib():
    from glow_tts_amd import _lib
    return _lib.lib()


def ragged(rng, lens, L_cap, C, bf16=False):
    """[B, L_cap, C] float32 with NaN behind every utterance, and the list of its valid parts"""
    xs = [rng.standard_normal((n, C)).astype(np.float32) for n in lens]
    if bf16:
        xs = [R64.bf2f(R64.f2bf(x)) for x in xs]
    full = np.full((len(lens), L_cap, C), np.nan, dtype=np.float32)
    for b, x in enumerate(xs):
        full[b, :len(x)] = x
    return full, xs


def zeros_behind(got, lens, name):
    for b, n in enumerate(lens):
        assert np.isfinite(got[b]).all() and not got[b, n:].any(), (name, b)


# ------------------------------------------------------------------------------------------------------------------- gt_vocos_norm
def ln_ref(h, e_h, g, be, eps, skip=None):
    """(LayerNorm(h), its bound) by oracle/ln64.py's model; skip: that channel left out of the mean's sum (a planted defect)"""
    C = h.shape[1]
    hm = h.copy()
    if skip is not None:
        hm[:, skip] = 0
    k = dict(axis=1, keepdims=True)
    mean = hm.sum(**k) / C
    e_mean = (e_h.sum(**k) + R64.gamma(C) * np.abs(h).sum(**k)) / C + U32 * np.abs(mean)
    dd = h - mean
    e_dd = e_h + e_mean + U32 * np.abs(dd)
    var = (dd * dd).sum(**k) / C
    e_var = ((2 * np.abs(dd) * e_dd + U32 * dd * dd).sum(**k) + R64.gamma(C) * (dd * dd).sum(**k)) / C + U32 * var
    rstd = 1.0 / np.sqrt(var + eps)
    e_rstd = rstd * ((e_var + U32 * (var + eps)) / (2 * (var + eps)) + R64.FAST_FN)
    n = dd * rstd * g + be
    return n, np.abs(rstd * g) * e_dd + np.abs(dd * g) * e_rstd + 3 * U32 * np.abs(dd * rstd * g) + U32 * np.abs(n)


def norm_call(X, wd, bd, g, be, Y, n_frames, B, L_cap, C, y_bf16, eps):
    from glow_tts_amd import _lib
    a = _lib.fill_args(_lib.VocosNormArgs, X=X, x_stride_b=L_cap * C, wd=wd, bd=bd, g=g, be=be, Y=Y, y_stride_b=L_cap * C,
                       n_frames=n_frames, B=B, L_cap=L_cap, C=C, y_bf16=int(y_bf16), eps=eps)
    _lib.call.gt_vocos_norm(a, _lib.current_stream(dev()))


@pytest.mark.parametrize("C,dw,y_bf16", [(64, True, True), (64, False, False), (512, True, True), (512, False, True), (512, True, False)])
def test_vocos_norm(built, C, dw, y_bf16):
    from oracle.guards import Guards
    M = lib().gt_vocos_tile_positions()
    lens = LENS(M)
    B, L_cap, eps = len(lens), max(lens) + 2, 1e-6
    assert ((L_cap + lib().gt_vocos_norm_tile_positions() - 1) // lib().gt_vocos_norm_tile_positions()) * B <= 64   # a quick launch
    rng = np.random.default_rng(C + 2 * dw + y_bf16)
    full, xs = ragged(rng, lens, L_cap, C)
    wd = (rng.standard_normal((C, 7)) / np.sqrt(7)).astype(np.float32)
    bd, g, be = (rng.standard_normal(C).astype(np.float32) for _ in range(3))
    gd = Guards(dev())
    t = lambda v: gd.inp(torch.from_numpy(v).to(dev()))  # noqa: E731
    X, n_frames = t(full), torch.tensor(lens, dtype=torch.int32, device=dev())
    Y = gd.out("Y", (B, L_cap, C), dtype=torch.bfloat16 if y_bf16 else torch.float32)
    g_d, be_d = t(g), t(be)
    norm_call(X, t(wd) if dw else None, t(bd) if dw else None, g_d, be_d, Y, n_frames, B, L_cap, C, y_bf16, eps)
    gd.verify()
    got = Y.float().cpu().double().numpy()
    zeros_behind(got, lens, "norm")

    def reference(w, skip=None):
        outs, bounds = [], []
        for x in xs:
            x64 = x.astype(np.float64)
            if dw:
                h = V.dwconv64(x64, w.astype(np.float64), bd.astype(np.float64))
                e_h = R64.gamma(8) * V.dwconv64(np.abs(x64), np.abs(w.astype(np.float64)), np.abs(bd.astype(np.float64)))
            else:
                h, e_h = x64, np.zeros_like(x64)
            n, e = ln_ref(h, e_h, g.astype(np.float64), be.astype(np.float64), eps, skip)
            outs.append(n); bounds.append(e)
        return np.concatenate(outs), np.concatenate(bounds)

    ref, bound = reference(wd)
    if dw:
        wbad = wd.copy()
        wbad[C // 3, 6] = 0
        bad = {"last tap's weight of one channel zeroed": reference(wbad)[0]}
    else:
        bad = {"one channel left out of the mean": reference(wd, skip=C // 3)[0]}
    got_valid = np.concatenate([got[b, :n] for b, n in enumerate(lens)])
    R64.check_with_control(f"norm C={C} dw={dw}", torch.from_numpy(got_valid), torch.from_numpy(ref), torch.from_numpy(bound),
                           {k: torch.from_numpy(v) for k, v in bad.items()}, kind="bf16" if y_bf16 else "f32")

    if not dw and not y_bf16:                                                      # in place: bit-identical
        gi = Guards(dev())
        Yi = gi.out("Y in place", (B, L_cap, C), prior=torch.from_numpy(full))
        norm_call(Yi, None, None, g_d, be_d, Yi, n_frames, B, L_cap, C, 0, eps)
        gi.verify()
        assert torch.equal(Yi.view(torch.int32), Y.view(torch.int32))


# ------------------------------------------------------------------------------------------------------------------- gt_vocos_mlp
def mlp_case(name, C, Hd, lens, n_frames, seed):
    from glow_tts_amd import _lib, audio
    from oracle.guards import Guards
    L = lib()
    M = L.gt_vocos_tile_positions()
    B, L_cap = len(lens), max(lens)
    assert [min(max(v, 0), L_cap) for v in n_frames] == list(lens)
    assert ((L_cap + M - 1) // M) * B <= 64
    rng = np.random.default_rng(seed)
    a_full, as_ = ragged(rng, lens, L_cap, C, bf16=True)
    r_full, rs = ragged(rng, lens, L_cap, C)
    W1 = (rng.standard_normal((Hd, C)) * (1.5 / np.sqrt(C))).astype(np.float32)      # pre-activations of a few units: both GELU branches
    W2 = (rng.standard_normal((C, Hd)) / np.sqrt(Hd)).astype(np.float32)
    b1, b2 = rng.standard_normal(Hd).astype(np.float32) * 0.5, rng.standard_normal(C).astype(np.float32)
    gd = Guards(dev())
    t = lambda v: gd.inp(torch.from_numpy(v).to(dev()))  # noqa: E731
    A = gd.inp(torch.from_numpy(a_full).to(dev()).to(torch.bfloat16))
    img1, img2 = gd.inp(audio.voc_pack(torch.from_numpy(W1).to(dev())[:, :, None])), gd.inp(audio.voc_pack(torch.from_numpy(W2).to(dev())[:, :, None]))
    b1_d, b2_d = t(b1), t(b2)
    nf = torch.tensor(n_frames, dtype=torch.int32, device=dev())
    Y = gd.out("Y (aliases R)", (B, L_cap, C), prior=torch.from_numpy(r_full))
    keep = torch.zeros(B, L_cap, Hd, dtype=torch.bool)
    for b, n in enumerate(lens):
        keep[b, n:] = True                                                         # U behind an utterance is not written
    Ub = gd.out("U", (B, L_cap, Hd), dtype=torch.bfloat16, keep=keep)

    def launch(R, Yo, Uo):
        a = _lib.fill_args(_lib.VocosMlpArgs, A=A, a_stride_b=L_cap * C, W1=img1, b1=b1_d, W2=img2, b2=b2_d, R=R, r_stride_b=L_cap * C,
                           Y=Yo, y_stride_b=L_cap * C, U=Uo, u_stride_b=L_cap * Hd, n_frames=nf, B=B, L_cap=L_cap, C=C, H=Hd)
        _lib.call.gt_vocos_mlp(a, _lib.current_stream(dev()))

    launch(Y, Y, Ub)
    gd.verify()
    got_y, got_u = Y.cpu().double().numpy(), Ub.float().cpu().double().numpy()
    zeros_behind(got_y, lens, name)
    # ---- the kernel's own operands
    W1_64 = H.decode_image(img1, Hd, C, 1, L.gt_voc_k_chunk(C))[0]
    W2_64 = H.decode_image(img2, C, Hd, 1, L.gt_voc_k_chunk(Hd))[0]
    assert np.array_equal(W1_64, R64.bf16_round(W1)) and np.array_equal(W2_64, R64.bf16_round(W2))
    b_long = int(np.argmax(lens))
    edge = M if lens[b_long] > M else lens[b_long] - 1                            # the first position of the second tile
    b1_64, b2_64 = b1.astype(np.float64), b2.astype(np.float64)

    def stage1(W, zero_pos=None):
        outs, bounds = [], []
        for b, a in enumerate(as_):
            a64 = a.astype(np.float64)
            if zero_pos is not None and b == b_long:
                a64 = a64.copy()
                a64[zero_pos] = 0
            pre, S = a64 @ W.T + b1_64, np.abs(a64) @ np.abs(W).T + np.abs(b1_64)
            u = V.gelu64(pre)
            outs.append(u)
            bounds.append(V.gelu_grad_max() * R64.gamma(C + 2) * S + U32 * (4 * np.abs(pre) + 2 * np.abs(u)) + R64.bf16_ulp(u))
        return np.concatenate(outs), np.concatenate(bounds)

    ref1, bound1 = stage1(W1_64)
    W1bad = W1_64.copy()
    W1bad[:, C // 3] = 0
    u_valid = np.concatenate([got_u[b, :n] for b, n in enumerate(lens)])
    R64.check_with_control(f"{name} stage 1", torch.from_numpy(u_valid), torch.from_numpy(ref1), torch.from_numpy(bound1),
                           {"tile-edge A position zeroed": torch.from_numpy(stage1(W1_64, edge)[0]),
                            "W1 entry zeroed": torch.from_numpy(stage1(W1bad)[0])}, kind="bf16")

    def stage2(W, zero_pos=None):
        outs, bounds = [], []
        for b, n in enumerate(lens):
            u = got_u[b, :n]
            if zero_pos is not None and b == b_long:
                u = u.copy()
                u[zero_pos] = 0
            r64 = rs[b].astype(np.float64)
            outs.append(u @ W.T + b2_64 + r64)
            bounds.append(R64.gamma(Hd + 3) * (np.abs(u) @ np.abs(W).T + np.abs(b2_64) + np.abs(r64)))
        return np.concatenate(outs), np.concatenate(bounds)

    ref2, bound2 = stage2(W2_64)
    W2bad = W2_64.copy()
    W2bad[:, Hd - L.gt_vocos_hidden_chunk() + 5] = 0                               # an entry of the last hidden chunk
    y_valid = np.concatenate([got_y[b, :n] for b, n in enumerate(lens)])
    R64.check_with_control(f"{name} stage 2", torch.from_numpy(y_valid), torch.from_numpy(ref2), torch.from_numpy(bound2),
                           {"W2 entry of the last chunk zeroed": torch.from_numpy(stage2(W2bad)[0]),
                            "tile-edge U position zeroed": torch.from_numpy(stage2(W2_64, edge)[0])}, kind="f32")
    # ---- without U, out of place: the same bits
    g2 = Guards(dev())
    Y2 = g2.out("Y (U NULL)", (B, L_cap, C))
    launch(g2.inp(torch.from_numpy(r_full).to(dev())), Y2, None)
    g2.verify()
    assert torch.equal(Y2.view(torch.int32), Y.view(torch.int32))


def test_vocos_mlp_two_chunks(built):
    L = lib()
    M, HC = L.gt_vocos_tile_positions(), L.gt_vocos_hidden_chunk()
    assert HC == V.HIDDEN_CHUNK
    lens = [0, 1, M - 1, M, M + 1, 2 * M + 3]
    mlp_case("mlp C=128", 128, 2 * HC, lens, [0, 1, M - 1, M, M + 1, 2 * M + 3 + 9], 11)


def test_vocos_mlp_published_width(built):
    mlp_case("mlp C=512", 512, 1536, [5, 9], [5, 9], 12)


# ------------------------------------------------------------------------------------------------------------------- gt_vocos_polar
def test_vocos_polar(built):
    from glow_tts_amd import _lib, audio
    from oracle.guards import Guards
    L = lib()
    tile = L.gt_gl_tile_frames()
    frames = [0, 1, 31, 32, 33, tile + 1]
    B, F_max = len(frames), tile + 3
    Fp = (F_max + tile - 1) // tile * tile
    assert Fp // 32 * 4 * B <= 128                                                 # small workgroups, a quick launch
    rng = np.random.default_rng(21)
    o = np.full((B, F_max, 1026), np.nan, dtype=np.float32)
    for b, n in enumerate(frames):
        o[b, :n, :513] = rng.uniform(-3.0, 5.0, (n, 513))
        o[b, :n, 513:] = rng.uniform(-50.0, 50.0, (n, 513))
    assert np.nanmax(o[:, :, :513]) > np.log(100.0) and np.nanmax(np.abs(o[:, :, 513:])) > 49.0
    gd = Guards(dev())
    O = gd.inp(torch.from_numpy(o).to(dev()))
    spec = gd.out("spec", (L.gt_gl_spec_bytes(B, F_max) // 4,))                    # every element must be written
    a = _lib.fill_args(_lib.VocosPolarArgs, O=O, o_stride_b=F_max * 1026, n_frames=torch.tensor(frames, dtype=torch.int32, device=dev()),
                       spec=spec, B=B, F_max=F_max, n_fft=1024)
    _lib.call.gt_vocos_polar(a, _lib.current_stream(dev()))
    gd.verify()
    re, im = (v.cpu().double().numpy() for v in audio.spec_unpack(spec, B, Fp))    # [B, 513, Fp]: the padded frames included
    got, ref, bad, bound = [], [], [], []
    for b, n in enumerate(frames):
        Fb = n if n >= 2 else 0                                                    # below 2 frames: no sample, nothing kept
        assert not re[b, :, Fb:].any() and not im[b, :, Fb:].any(), b
        x, p = o[b, :Fb, :513].astype(np.float64).T, o[b, :Fb, 513:].astype(np.float64).T
        m, raw = np.minimum(np.exp(x), 100.0), np.exp(x)
        s = np.sin(p)
        s[512] = 0                                                                 # Im of bin 512 is not kept
        got += [re[b, :, :Fb].ravel(), im[b, :, :Fb].ravel()]
        ref += [(m * np.cos(p)).ravel(), (m * s).ravel()]
        bad += [(raw * np.cos(p)).ravel(), (raw * s).ravel()]
        bound += [8 * U32 * m.ravel()] * 2
    got, ref, bad, bound = (torch.from_numpy(np.concatenate(v)) for v in (got, ref, bad, bound))
    assert float(ref.abs().max()) > 99.0
    R64.check_with_control("polar", got, ref, bound, {"clip at 100 left out": bad}, kind="f32")
