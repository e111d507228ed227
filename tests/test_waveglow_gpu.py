"""GPU tests of the WaveGlow vocoder (glow_tts_amd.audio.WaveGlow on csrc/waveglow.hip and gt_voc_conv).

Kernels alone, against float64 ON THEIR OWN operands with derived bounds:
  gt_wg_gate      the rule of oracle/rows64.py (gamma_K S + the gate's epilogue bound + the bf16 output's rounding), K = 3C + 640 + 2,
                  at C in {64, 256} x dilation in {1, 4, 128}, lengths 0, 1, tile - 1, tile + 1 and one below the dilation (every tap
                  outside), NaN behind every length and in the stale output, every utterance with its own spect.
  gt_wg_boundary  all three forms at c in {4, 6, 8} against float64 with fp32 fmaf-chain bounds gamma(K) sum |terms| carried through
                  the coupling and the 1x1; its noise against the host restatement (tests/synth_noise_host.py, 1e-5 as the front
                  end's noise test asks); samples exactly zero behind len_b.

Whole model: the rule and margin of tests/test_hifigan_gpu.py — tests/waveglow64.py has the exact float64 generator and a CPU EMULATION
of the kernels' numerics; E_emul = ||emul - exact|| / ||exact|| is computed here on the CPU, never from the code under test, and the
device must satisfy ||gpu - exact|| / ||exact|| <= 2 E_emul per utterance and over the batch, with 0 < E_emul < 0.05 and
max |exact| > 1e-3.  A batch row's latent is keyed by its row index b: "alone" means alone in row b.

Measured on an MI355X (ratio = device error / E_emul over the batch; the bound is 2; per utterance the ratio was 0.999 - 1.054):
  TINY, frames (0, 1, 2, 3, 5)     E_emul 1.370e-04, device 1.379e-04, ratio 1.007
  PUBLISHED, B = 2, frames (2, 5)  E_emul 7.567e-04, device 7.934e-04, ratio 1.049
  gt_wg_gate alone: worst error / bound 0.28 - 0.57, bf16 mismatches <= 0.024 %, the planted defect missed by 62 - 189 x
  gt_wg_boundary alone: worst error / bound <= 0.027
"""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hifigan64 as H  # noqa: E402
import waveglow64 as W  # noqa: E402
from oracle import rows64 as R64  # noqa: E402

pytestmark = pytest.mark.gpu
SEED = 3


def dev():
    return torch.device("cuda:0")


def nan_fill(t):
    t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32).fill_(-1)       # NaN patterns: nothing stale may matter
    return t


# ----------------------------------------------------------------------------- gt_wg_gate alone
@pytest.mark.parametrize("C", [64, 256])
@pytest.mark.parametrize("dil", [1, 4, 128])
def test_gate_kernel_against_float64(built, C, dil):
    from glow_tts_amd import _lib, audio
    tile = _lib.call.gt_wg_tile_positions()
    lens = [0, 1, tile - 1, tile + 1, max(dil - 1, 2)]
    B, Lc, Cs = len(lens), tile + 12, 640
    g = torch.Generator().manual_seed(100 * C + dil)
    X = torch.full((B, Lc, 2 * C), float("nan"))
    S = torch.full((B, Lc, Cs), float("nan"))
    for b, n in enumerate(lens):
        X[b, :n, :C] = torch.randn(n, C, generator=g)
        S[b, :n] = torch.randn(n, Cs, generator=g)
    S = S.to(torch.bfloat16)
    w_in = torch.randn(2 * C, C, 3, generator=g) / np.sqrt(3 * C)
    w_c = torch.randn(2 * C, Cs, 1, generator=g) / np.sqrt(Cs)
    b_in, b_c = torch.randn(2 * C, generator=g) * 0.1, torch.randn(2 * C, generator=g) * 0.1
    perm = audio.gate_interleave(C)
    d = dev()
    Xd, Sd, G = X.to(d), S.to(d), nan_fill(torch.empty(B, Lc, C, dtype=torch.bfloat16, device=d))
    imgs = audio.voc_pack(w_in[perm].to(d)), audio.voc_pack(w_c[perm].to(d))
    bi, bc = b_in.to(d), b_c.to(d)
    nf = torch.tensor(lens, dtype=torch.int32, device=d)
    _lib.call.gt_wg_gate(_lib.fill_args(_lib.WgGateArgs, X=Xd, x_stride_b=Lc * 2 * C, ldx=2 * C, Cs=Cs, S=Sd, s_stride_b=Lc * Cs,
                                        W_in=imgs[0], W_cond=imgs[1], b_in=bi, b_cond=bc, G=G, g_stride_b=Lc * C, len_mul=1, n_frames=nf,
                                        B=B, L_cap=Lc, C=C, taps=3, dil=dil), _lib.current_stream(d))
    torch.cuda.synchronize()
    got = G.float().cpu()
    Wi = np.ascontiguousarray(R64.bf16_round(w_in.numpy()).transpose(2, 0, 1))          # the kernel's own operands, decoded
    Wc = R64.bf16_round(w_c.numpy()[:, :, 0])
    bias = b_in.double().numpy() + b_c.double().numpy()
    K = 3 * C + Cs + 2
    for b, n in enumerate(lens):
        assert not got[b, n:].any(), (b, "zeros behind the utterance")
        if not n:
            continue
        xo, so = R64.bf16_round(X[b, :n, :C].numpy()), S[b, :n].double().numpy()
        Y, Sa = H.conv64(xo, Wi, 3, dil)
        Y = Y + so @ Wc.T + bias
        Sa = Sa + np.abs(so) @ np.abs(Wc).T + np.abs(b_in.double().numpy()) + np.abs(b_c.double().numpy())
        out, _ = R64.gate_fwd(torch.from_numpy(Y), torch.from_numpy(Sa), K, C)
        ref, bound = out["acts"]
        bad = ref.clone()
        bad[:, ::7] = torch.tanh(torch.from_numpy(Y[:, :C:7])) * torch.sigmoid(torch.from_numpy((Y - so @ Wc.T)[:, C::7]))   # sigmoid half without its conditioning
        r = R64.check_with_control(f"gate C={C} dil={dil} utt {b} len {n}", got[b, :n], ref, bound, bad, kind="bf16")
        assert r.ok


# ----------------------------------------------------------------------------- gt_wg_boundary alone
def boundary_case(form, c, C, g):
    """(c_in, c_out, weights) of one form at c channels"""
    if form == "first":
        c_in, c_out = 0, c
    elif form == "middle":
        c_in, c_out = c, min(c + 2, 8)
    else:
        c_in, c_out = c, 8
    h, lo, lo2, h2 = c_in // 2, 8 - c_in, 8 - c_out, c_out // 2
    w = {}
    if c_in:
        w_end, b_end = torch.zeros(C, 8), torch.zeros(8)
        w_end[:, 4 - h:4], w_end[:, 8 - h:8] = torch.randn(C, h, generator=g) * 0.02, torch.randn(C, h, generator=g) * 0.02
        b_end[4 - h:4], b_end[8 - h:8] = torch.randn(h, generator=g) * 0.1, torch.randn(h, generator=g) * 0.1
        w_inv = torch.zeros(8, 8)
        w_inv[lo:, lo:] = torch.linalg.qr(torch.randn(c_in, c_in, generator=g))[0] + 0.1 * torch.randn(c_in, c_in, generator=g)
        w.update(w_end=w_end, b_end=b_end, w_inv=w_inv)
    if form != "last":
        w_start = torch.zeros(C, 8)
        w_start[:, lo2:lo2 + h2] = torch.randn(C, h2, generator=g)
        w.update(w_start=w_start, b_start=torch.randn(C, generator=g))
    return c_in, c_out, w


@pytest.mark.parametrize("form", ["first", "middle", "last"])
@pytest.mark.parametrize("c", [4, 6, 8])
def test_boundary_kernel_against_float64(built, form, c):
    from glow_tts_amd import _lib
    C, sigma, seed = 128, 0.666, 77
    lens = [0, 1, 31, 33, 70]
    B, Lc = len(lens), 75
    g = torch.Generator().manual_seed(10 * c + len(form))
    c_in, c_out, w = boundary_case(form, c, C, g)
    state = torch.full((B, Lc, 2 * C), float("nan"))
    A = torch.full((B, Lc, 8), float("nan"))
    for b, n in enumerate(lens):
        state[b, :n, C:] = torch.randn(n, C, generator=g) * 3
        A[b, :n, 8 - c_in:] = torch.randn(n, c_in, generator=g)
    d = dev()
    sd_, Ad = state.to(d), A.to(d)
    wd = {k: v.to(d).contiguous() for k, v in w.items()}
    seed_dev = torch.tensor([seed], dtype=torch.int32, device=d)
    nf = torch.tensor(lens, dtype=torch.int32, device=d)
    _lib.call.gt_wg_boundary(_lib.fill_args(
        _lib.WgBoundaryArgs, state=sd_, st_stride_b=Lc * 2 * C, ld=2 * C, C=C, A=Ad, a_stride_b=8 * Lc, w_end=wd.get("w_end"),
        b_end=wd.get("b_end"), w_inv=wd.get("w_inv"), w_start=wd.get("w_start"), b_start=wd.get("b_start"), n_frames=nf,
        seed_dev=seed_dev, seed=12345, sigma=sigma, len_mul=1, B=B, L_cap=Lc, c_in=c_in, c_out=c_out), _lib.current_stream(d))
    torch.cuda.synchronize()
    got_s, got_a = sd_.double().cpu().numpy(), Ad.double().cpu().numpy()
    u, gam = 2.0 ** -24, R64.gamma
    h, lo, lo2, h2 = c_in // 2, 8 - c_in, 8 - c_out, c_out // 2
    p = {k: v.double().numpy() for k, v in w.items()}
    for b, n in enumerate(lens):
        if form == "last":
            assert not got_a[b, n:].any(), "samples exactly zero behind len_b"
        else:
            assert np.isnan(got_a[b, n:]).all() and np.isnan(got_s[b, n:]).all(), "nothing behind len_b is written"
        if not n:
            continue
        a, ea = np.zeros((n, 8)), np.zeros((n, 8))                                     # the slots and their error bound
        if c_in:
            a[:, lo:] = A[b, :n, lo:].double().numpy()
            sk = state[b, :n, C:].double().numpy()
            e = sk @ p["w_end"] + p["b_end"]
            ee = gam(C + 1) * (np.abs(sk) @ np.abs(p["w_end"]) + np.abs(p["b_end"]))
            for s in range(8 - h, 8):
                sh, ls, esh, els = e[:, s - 4], e[:, s], ee[:, s - 4], ee[:, s]
                val = (a[:, s] - sh) * np.exp(-ls)
                ea[:, s] = np.exp(-ls) * esh + np.abs(val) * (els * 1.01 + 8 * u) + 2 * u * np.abs(a[:, s] - sh) * np.exp(-ls)
                a[:, s] = val
            ea = np.abs(p["w_inv"][None] * 1.0) @ ea[:, :, None]
            ea = ea[:, :, 0] + gam(8) * (np.abs(a) @ np.abs(p["w_inv"]).T)
            a = a @ p["w_inv"].T
        Z = W.latent64(seed, b, n, sigma)
        a[:, lo2:lo], ea[:, lo2:lo] = Z[:, lo2:lo], 1e-5
        assert np.all(got_a[b, :n, :lo2] == 0)
        err = np.abs(got_a[b, :n] - a)
        lim = ea + u * np.abs(a)
        print(f"boundary {form} c={c} utt {b}: worst err/bound {float((err[:, lo2:] / lim[:, lo2:]).max()):.3g}")
        assert np.all(err[:, lo2:] <= lim[:, lo2:]), (form, c, b)
        if c_in < c_out:
            assert float(np.abs(got_a[b, :n, lo2:lo] - Z[:, lo2:lo]).max()) <= 1e-5 and float(np.abs(Z[:, lo2:lo]).max()) > 0.1
        if form != "last":
            ws, a0 = p["w_start"][:, lo2:lo2 + h2], got_a[b, :n, lo2:lo2 + h2]          # the kernel's own slots
            x = a0 @ ws.T + p["b_start"]
            xb = gam(h2 + 1) * (np.abs(a0) @ np.abs(ws).T + np.abs(p["b_start"])) + u * np.abs(x)
            assert np.all(np.abs(got_s[b, :n, :C] - x) <= xb), (form, c, b)
            assert not got_s[b, :n, C:].any(), "the skip accumulator starts from 0"
    if form == "last":
        assert torch.equal(sd_.cpu().view(torch.int32), state.view(torch.int32)), "the last form does not touch the state"


# ----------------------------------------------------------------------------- the whole model
@functools.lru_cache(maxsize=None)
def model(name):
    from glow_tts_amd import audio
    cfg = getattr(W, name)
    return W.init_for_tests(audio.WaveGlow(**cfg), 7).to(dev())


def batch(frames, seed):
    """(mel [B, 80, F_max] with NaN behind every utterance's frames)"""
    rng = np.random.default_rng(seed)
    mel = np.full((len(frames), 80, max(frames)), np.nan, dtype=np.float32)
    for b, n in enumerate(frames):
        mel[b, :, :n] = W.random_mel(rng, 80, n)
    return mel


@functools.lru_cache(maxsize=None)
def references(name, frames, seed):
    """[(exact, emul)] per utterance, computed once on the CPU"""
    voc, cfg = model(name), getattr(W, name)
    sd = {k: v.cpu() for k, v in voc.state_dict().items()}
    mel = batch(frames, seed)
    return [(W.generator64(sd, cfg, mel[b, :, :n], SEED, b), W.generator64(sd, cfg, mel[b, :, :n], SEED, b, emul=True))
            for b, n in enumerate(frames)]


def check_against_float64(name, frames, seed, wav):
    got = wav.double().cpu().numpy()
    assert got.shape == (len(frames), 256 * max(frames)) and np.isfinite(got).all()
    refs = references(name, frames, seed)
    for b, n in enumerate(frames):
        assert not got[b, 256 * n:].any(), (name, b)
        ex, em = refs[b]
        if n:
            eb, db = W.rel_l2(em, ex), W.rel_l2(got[b, :256 * n], ex)
            print(f"{name} utt {b} F={n}: emulation {eb:.3e}, device {db:.3e}, ratio {db / eb:.3f}")
            assert 0 < eb and db <= 2 * eb, (name, b, db, eb)
    exact, emul = (np.concatenate([r[i] for r in refs]) for i in (0, 1))
    dev_ = np.concatenate([got[b, :256 * n] for b, n in enumerate(frames)])
    e_emul, e_dev = W.rel_l2(emul, exact), W.rel_l2(dev_, exact)
    print(f"{name}: E_emul {e_emul:.3e}, device error {e_dev:.3e}, ratio {e_dev / e_emul:.3f} (bound 2)")
    assert 0 < e_emul < 0.05 and float(np.abs(exact).max()) > 1e-3
    assert e_dev <= 2 * e_emul, (e_dev, e_emul)


def vocode(voc, mel, frames, seed=SEED):
    return voc(torch.from_numpy(mel).to(dev()), torch.tensor(frames, dtype=torch.int32, device=dev()), mel_lengths_host=list(frames), seed=seed)


def test_tiny_config_ragged_batch(built):
    voc, frames = model("TINY"), W.TINY_FRAMES
    wav, wav_lengths = vocode(voc, batch(frames, 17), frames)
    assert wav_lengths.tolist() == [256 * n for n in frames]
    check_against_float64("TINY", frames, 17, wav)


def test_published_config_and_its_launches(built):
    from glow_tts_amd import _lib
    voc, frames = model("PUBLISHED"), (2, 5)
    voc.images()                                                                          # packed outside the launches that are counted
    with _lib.record_calls() as names:
        wav, _ = vocode(voc, batch(frames, 29), frames)
    assert names.count("gt_voc_conv") == 1 + 96 and names.count("gt_wg_gate") == 96 and names.count("gt_wg_boundary") == 13
    assert len(names) == voc.launches == 1 + 192 + 13
    check_against_float64("PUBLISHED", frames, 29, wav)


def test_batch_independence_capacity_form_and_seeds(built):
    """a batch row is bit-identical to the utterance alone in its row (every other row empty, its mel NaN: the latent is keyed by the
    row); run() into a NaN-filled workspace of capacity (B + 1, F_max + 11) is bit-identical to forward(); the same
    seed gives the same bits, another seed other samples"""
    voc, frames = model("TINY"), W.TINY_FRAMES
    mel = batch(frames, 17)
    B, F_max = mel.shape[0], mel.shape[2]
    wav, _ = vocode(voc, mel, frames)
    bits = lambda t: t.contiguous().view(torch.int32)  # noqa: E731
    for b, n in enumerate(frames):
        if not n:
            continue
        alone = np.full_like(mel, np.nan)
        alone[b] = mel[b]
        only = tuple(n if i == b else 0 for i in range(B))
        out, _ = vocode(voc, alone, only)
        assert torch.equal(bits(out[b]), bits(wav[b])) and not bool(out[:b].any()) and not bool(out[b + 1:].any()), b
    bufs = voc.workspace(B + 1, F_max + 11, dev())
    for t in bufs.values():
        nan_fill(t)
    big = torch.full((B + 1, 80, F_max + 16), float("nan"), device=dev())
    big[:B, :, :F_max] = torch.from_numpy(mel).to(dev())
    n_frames = torch.tensor(list(frames) + [0], dtype=torch.int32, device=dev())
    seed_dev = torch.tensor([SEED], dtype=torch.int32, device=dev())
    out = voc.run(big, n_frames, bufs, seed_dev=seed_dev)
    assert out.shape == (B + 1, 256 * (F_max + 11)) and out is bufs["wav"]
    assert torch.equal(bits(out[:B, :256 * F_max]), bits(wav))
    assert not bool(out[:B, 256 * F_max:].any()) and not bool(out[B].any())
    again, _ = vocode(voc, mel, frames)
    other, _ = vocode(voc, mel, frames, seed=SEED + 1)
    assert torch.equal(bits(again), bits(wav)) and not torch.equal(other, wav)
    assert float((other - wav).abs().max()) > 1e-2
    with pytest.raises(ValueError):
        voc(torch.zeros(1, 40, 3, device=dev()))
