"""GPU tests of the device front end of synthesis (csrc/synth_front.hip, FlowGenerator.set_synthesis_front):
gt_randn_rows / gt_synth_lengths / gt_synth_prior against the host restatement of the generator (tests/synth_noise_host.py) and
oracle/glowtts_ref.generate_path, then FlowGenerator.infer with the switch on against the switch off and against the float oracle.

Tolerances: 1e-5 absolute for a generator draw against its float64 restatement (an fp32 evaluation on the CPU is within 1.6e-6; the
margin covers the device's logf / sincospif), 1e-5 of the tensor's max-abs for the fp32 rows, exact for every integer
and gathered output, 3e-2 of max-abs for a mel against the float oracle's reverse decoder (tests/test_decoder_gpu.py), and the
front-on mel error at most twice the front-off one (floor 1e-3), the rule of tests/test_synthesis_fused_gpu.py."""
import ctypes
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "golden"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import synth_noise_host as H  # noqa: E402
from fill import fill_module  # noqa: E402
from oracle import glowtts_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HALO = 2
CAN, MARGIN = 768.0, 1024


def dev():
    return torch.device("cuda:0")


def relerr(a, b):
    return (a - b).abs().max().item() / max(1e-6, b.abs().max().item())


def cpu_state(mod, prefix=""):
    return {prefix + k: v.detach().cpu().float() for k, v in mod.state_dict().items()}


def guarded(n, dtype, inside):
    """flat buffer with canary margins -> (flat, the n elements in the middle, pre-filled with `inside`)"""
    flat = torch.full((n + 2 * MARGIN,), CAN, dtype=dtype, device=dev())
    flat[MARGIN:MARGIN + n] = inside
    return flat, flat[MARGIN:MARGIN + n]


def margins_untouched(flat, n):
    return bool((flat[:MARGIN] == CAN).all() and (flat[MARGIN + n:] == CAN).all())


def test_randn_rows_against_the_host(built):
    from glow_tts_amd import _lib
    L = _lib.lib()
    for R_, ncol, seed, stream, scale in ((300, 2, 12345, H.PITCH, 1.0), (7, 5, 0x7fffffff, H.ENERGY, 0.25)):
        flat, out = guarded(R_ * ncol, torch.float32, float("nan"))
        _lib.check(L.gt_randn_rows(_lib.ptr(out), R_, ncol, seed, stream, scale, _lib.current_stream(dev())), "gt_randn_rows")
        torch.cuda.synchronize()
        want = H.randn_rows(R_, ncol, seed, stream, scale)
        err = np.abs(out.cpu().numpy().astype(np.float64).reshape(R_, ncol) - want).max()
        print(f"gt_randn_rows [{R_}, {ncol}] vs host float64: {err:.3e}")
        assert margins_untouched(flat, R_ * ncol)
        assert err <= 1e-5, err


# ---- the two kernels called directly ------------------------------------------------------------------------------------------
def run_front(dur, x_len, x_m, x_logs, noise_scale, seed, ragged):
    """gt_synth_lengths + gt_synth_prior on guarded buffers -> dict of results (device tensors, host lengths, the rows context)"""
    from glow_tts_amd import _lib, ops
    L = _lib.lib()
    st = _lib.current_stream(dev())
    B, Tx = dur.shape
    C = x_m.shape[1]
    dur_d, xl = dur.to(dev()).contiguous(), x_len.to(torch.int32).to(dev())
    f_cum, cum = guarded(B * Tx, torch.int32, -7)
    f_yl, y_len = guarded(B, torch.int32, -7)
    f_lw, logw = guarded(B * Tx, torch.float32, float("nan"))
    _lib.check(L.gt_synth_lengths(_lib.ptr(dur_d), _lib.ptr(xl), _lib.ptr(cum), _lib.ptr(y_len), _lib.ptr(logw), B, Tx, st), "gt_synth_lengths")
    torch.cuda.synchronize()
    assert margins_untouched(f_cum, B * Tx) and margins_untouched(f_yl, B) and margins_untouched(f_lw, B * Tx)
    lens = y_len.cpu().tolist()
    Ty = max(lens)
    lsq = [v // 2 for v in lens]
    rc = ops.RowsCtx(torch.tensor(lsq, dtype=torch.int32, device=dev()), Ty // 2, lengths_host=lsq if ragged else None, round_to=8)
    f_rows, rows = guarded(rc.R * 2 * C, torch.float32, float("nan"))
    f_zm, z_m = guarded(B * C * Ty, torch.float32, float("nan"))
    f_zl, z_logs = guarded(B * C * Ty, torch.float32, float("nan"))
    f_ft, f2t = guarded(B * Ty, torch.int32, -7)
    f_at, attn = guarded(B * Tx * Ty, torch.float32, float("nan"))
    xm_d = x_m.to(dev()).contiguous()
    xs_d = None if x_logs is None else x_logs.to(dev()).contiguous()
    args = _lib.fill_args(_lib.SynthPriorArgs, x_m=xm_d, x_logs=xs_d, cum=cum, x_len=xl, y_len=y_len, row0=rc.row0, Tp=rc.Tp, R=rc.R,
                          rows=rows, z_m=z_m, z_logs=z_logs, frame2token=f2t, attn=attn, B=B, C=C, Tx=Tx, Ty=Ty, seed=seed,
                          noise_scale=noise_scale)
    _lib.check(L.gt_synth_prior(ctypes.byref(args), st), "gt_synth_prior")
    torch.cuda.synchronize()
    for flat, n in ((f_rows, rc.R * 2 * C), (f_zm, B * C * Ty), (f_zl, B * C * Ty), (f_ft, B * Ty), (f_at, B * Tx * Ty)):
        assert margins_untouched(flat, n)
    return dict(cum=cum.view(B, Tx).cpu(), y_len=lens, logw=logw.view(B, Tx).cpu(), rows=rows.view(rc.R, 2 * C).cpu(),
                z_m=z_m.view(B, C, Ty).cpu(), z_logs=z_logs.view(B, C, Ty).cpu(), f2t=f2t.view(B, Ty).cpu(),
                attn=attn.view(B, Tx, Ty).cpu(), rc=rc, Ty=Ty,
                base=rc.row0.cpu().tolist() if ragged else [b * rc.Tp for b in range(B + 1)])


def rows_reference(z, lens, base, R_):
    """z [B, C, Ty] float64 -> the squeezed rows [R, 2C] float64 (zero halo / padding rows) and the mask of rows that hold frames"""
    B, C, _ = z.shape
    want = np.zeros((R_, 2 * C))
    inside = np.zeros(R_, dtype=bool)
    for b in range(B):
        for s in range(lens[b] // 2):
            r = base[b] + HALO + s
            want[r, :C], want[r, C:] = z[b, :, 2 * s], z[b, :, 2 * s + 1]
            inside[r] = True
    return want, inside


def test_prior_rows_are_the_noise_itself(built):
    """x_m = 0, x_logs = 0, noise_scale = 1: the rows are the generator's draws, about 200 squeezed rows of 3 utterances."""
    B, C, Tx, seed = 3, 80, 10, 2
    dur = torch.tensor([[14.0] * 10, [13.0] * 10, [13.0] * 9 + [14.0]])            # 140 / 130 / 131 frames -> 70 + 65 + 65 rows
    out = run_front(dur, torch.tensor([Tx] * B), torch.zeros(B, C, Tx), torch.zeros(B, C, Tx), 1.0, seed, True)
    assert out["y_len"] == [140, 130, 131]
    z = np.stack([H.prior_noise(seed, b, C, out["Ty"]) for b in range(B)])
    want, inside = rows_reference(z, out["y_len"], out["base"], out["rc"].R)
    assert inside.sum() == 200
    got = out["rows"].numpy().astype(np.float64)
    err = np.abs(got - want).max()
    print(f"gt_synth_prior noise rows vs host float64: {err:.3e}")
    assert err <= 1e-5, err
    assert (got[~inside] == 0).all()


def _durations(Tx, rows):
    return torch.tensor(rows, dtype=torch.float32).reshape(len(rows), Tx)


@functools.lru_cache(maxsize=None)
def front_case(name):
    """(dur [B, Tx] with 0 on masked tokens, x_len, x_m, x_logs) of a named case, built once"""
    g = torch.Generator().manual_seed(17)
    if name == "Tx1":                                   # one token; a 2-frame utterance
        dur, xl = _durations(1, [[5], [2], [1]]), [1, 1, 1]
    elif name == "Tx2":                                 # a zero-duration token at the end / at the start
        dur, xl = _durations(2, [[3, 0], [0, 4], [2, 7]]), [2, 2, 2]
    elif name == "Tx19":
        xl = [19, 11, 19, 7, 19, 3]
        dur = torch.randint(0, 7, (6, 19), generator=g).float()
        dur[0, 0] = 0; dur[0, 9:12] = 0; dur[0, 18] = 0           # zero durations at the start, in the middle and at the end
        dur[0, 5] += 1 - dur[0].sum() % 2                         # an odd y_len
        dur[2] = 0                                                # durations that sum to 0: y_len = 1, no squeezed row, prior 0
        dur[5] = 0; dur[5, 1] = 2                                 # a 2-frame utterance
        dur = dur * (torch.arange(19)[None, :] < torch.tensor(xl)[:, None])
    elif name == "Tx512":
        xl = [512, 300]
        dur = torch.randint(0, 3, (2, 512), generator=g).float()
        dur[0, 0] = 0; dur[0, 511] = 0
        dur = dur * (torch.arange(512)[None, :] < torch.tensor(xl)[:, None])
    B, Tx = dur.shape
    x_m = torch.randn(B, 80, Tx, generator=g)
    x_logs = torch.randn(B, 80, Tx, generator=g) * 0.3
    return dur, torch.tensor(xl), x_m, x_logs


@functools.lru_cache(maxsize=None)
def front_reference(name):
    """generate_path and the gathers of models.py:1196-1201 on the host, once per case"""
    dur, xl, x_m, x_logs = front_case(name)
    B, Tx = dur.shape
    y_len = torch.clamp_min(dur.sum(1), 1).long()
    Ty = int(y_len.max())
    x_mask = (torch.arange(Tx)[None, :] < xl[:, None]).float()
    z_mask = (torch.arange(Ty)[None, :] < y_len[:, None]).float()
    attn = R.generate_path(dur, x_mask[:, :, None] * z_mask[:, None, :])
    f2t = torch.where(attn.sum(1) > 0, attn.argmax(1), torch.full((B, Ty), -1))
    idx = f2t.clamp(min=0)[:, None, :].expand(B, 80, Ty)
    own = (f2t >= 0)[:, None, :].float()
    return dict(cum=torch.cumsum(dur, 1).int(), y_len=y_len.tolist(), Ty=Ty, attn=attn, f2t=f2t.int(),
                z_m=torch.gather(x_m, 2, idx) * own, z_logs=torch.gather(x_logs, 2, idx) * own,
                logw=torch.log(1e-8 + dur) * x_mask)


@pytest.mark.parametrize("ragged", [True, False])
@pytest.mark.parametrize("noise_scale", [0.0, 0.667])
@pytest.mark.parametrize("mean_only", [False, True])
@pytest.mark.parametrize("name", ["Tx1", "Tx2", "Tx19", "Tx512"])
def test_lengths_and_prior_against_generate_path(built, name, mean_only, noise_scale, ragged):
    dur, xl, x_m, x_logs = front_case(name)
    ref = front_reference(name)
    seed = 99
    out = run_front(dur, xl, x_m, None if mean_only else x_logs, noise_scale, seed, ragged)
    B, C, Ty = x_m.shape[0], 80, ref["Ty"]
    if name == "Tx19":
        assert ref["y_len"][2] == 1 and ref["y_len"][0] % 2 == 1 and ref["y_len"][5] == 2
        if ragged:
            assert out["rc"].R % 64 != 0
    assert torch.equal(out["cum"], ref["cum"])
    assert out["y_len"] == ref["y_len"]
    assert torch.equal(out["f2t"], ref["f2t"])
    assert torch.equal(out["attn"], ref["attn"])
    assert torch.equal(out["z_m"], ref["z_m"])                                    # bit-equal to the gather
    assert torch.equal(out["z_logs"], torch.zeros_like(ref["z_logs"]) if mean_only else ref["z_logs"])
    assert torch.allclose(out["logw"], ref["logw"], rtol=1e-6, atol=1e-6)          # logf on two platforms: a few fp32 ulp
    z_logs = np.zeros((B, C, Ty)) if mean_only else ref["z_logs"].numpy().astype(np.float64)
    noise = np.stack([H.prior_noise(seed, b, C, Ty) for b in range(B)])
    z = ref["z_m"].numpy().astype(np.float64) + np.exp(z_logs) * noise * float(np.float32(noise_scale))
    want, inside = rows_reference(z, ref["y_len"], out["base"], out["rc"].R)
    got = out["rows"].numpy().astype(np.float64)
    assert not np.isnan(got).any()                                                 # every row was written ...
    assert (got[~inside] == 0).all()                                               # ... halo / padding / rounding rows as zeros
    err = np.abs(got - want).max() / max(1e-6, np.abs(want).max())
    print(f"gt_synth_prior rows [{name}, mean_only={mean_only}, noise_scale={noise_scale}, ragged={ragged}]: {err:.3e} of max-abs")
    assert err <= 1e-5, err
    if noise_scale == 0.0:
        assert np.array_equal(got, want)


# ---- FlowGenerator.infer ---------------------------------------------------------------------------------------------------------
def small_generator():
    """the model of test_infer_with_the_switch_on (tests/test_synthesis_fused_gpu.py)"""
    from glow_tts_amd import models
    gen = fill_module(models.FlowGenerator(148, 192, 768, 256, 80, use_sdp=False, kernel_size=3, n_heads=2, n_layers_enc=2, p_dropout=0.1,
                                           n_blocks_dec=2, kernel_size_dec=5, dilation_rate=1, n_block_layers=4,
                                           p_dropout_dec=0.05, n_sqz=2, window_size=4, mean_only=True, prenet=True), "").eval()
    P = cpu_state(gen)
    g = torch.Generator().manual_seed(3)
    ids = torch.randint(1, 148, (2, 19), generator=g)
    xl = torch.tensor([19, 11])
    ids = ids * (torch.arange(19)[None, :] < xl[:, None])
    return gen.to(dev()), P, ids.to(dev()), xl.to(dev())


def test_switch_behaviour(built):
    gen, P, ids, xl = small_generator()
    assert gen.synthesis_front is False                                            # opt-in
    assert gen.store_inverse() is False and gen.synthesis_front is False
    with pytest.raises(ValueError, match="set_synthesis_front"):
        gen.infer(ids, xl, noise_scale=0.0, seed=1)
    assert gen.store_inverse(fused_reverse=True, device_front=True) == (True, True)
    assert gen.store_inverse(device_front=None) is True and gen.synthesis_front is True      # None leaves both switches
    assert gen.store_inverse(fused_reverse=False) is False and gen.synthesis_front is True
    assert gen.set_synthesis_front(False) is False and gen.synthesis_front is False


@pytest.mark.parametrize("fused", [False, True])
def test_infer_front_on_against_front_off_without_noise(built, fused):
    gen, P, ids, xl = small_generator()
    res = []
    for front in (False, True):
        assert gen.store_inverse(fused_reverse=fused, device_front=front) == (fused, front)
        (y, z_m, z_logs, ld, z_mask), (x_m, x_logs, x_mask), (attn, logw, logw_), (pit, ene) = \
            gen.infer(ids, xl, noise_scale=0.0, **(dict(seed=5) if front else {}))
        torch.cuda.synchronize()
        assert ld is None and pit is None and ene is None
        res.append(dict(y=y.clone(), z_m=z_m.clone(), z_logs=z_logs.clone(), z_mask=z_mask.clone(), attn=attn.clone(),
                        logw=logw.clone(), logw_=logw_.clone()))
    off, on = res
    for k in ("attn", "logw", "logw_", "z_m", "z_logs", "z_mask"):
        assert on[k].shape == off[k].shape and on[k].dtype == off[k].dtype, k
        assert torch.equal(on[k], off[k]), k
    assert on["y"].shape == off["y"].shape and on["y"].dtype == off["y"].dtype
    zk = on["z_mask"].cpu()
    y_want = R.decoder_rev(P, "decoder.", on["z_m"].cpu() * zk, zk, n_blocks=2)
    e_off, e_on = relerr(off["y"].cpu(), y_want), relerr(on["y"].cpu(), y_want)
    print(f"infer mel vs oracle [fused_reverse={fused}]: front off {e_off:.3e}, front on {e_on:.3e}, between them {relerr(on['y'], off['y']):.3e}")
    assert torch.isfinite(on["y"]).all()
    assert e_on < 3e-2, e_on
    assert e_on <= max(2 * e_off, 1e-3), (e_on, e_off)


@pytest.mark.parametrize("fused", [False, True])
def test_infer_with_noise_against_the_oracle(built, fused):
    """noise_scale = 0.667, seed = 1234: the host rebuilds z from the returned z_m / z_logs and the restated noise, the float oracle's
    reverse decoder gives the mel."""
    gen, P, ids, xl = small_generator()
    gen.store_inverse(fused_reverse=fused, device_front=True)
    ns, seed = 0.667, 1234
    (y, z_m, z_logs, ld, z_mask), _, _, _ = gen.infer(ids, xl, noise_scale=ns, seed=seed)
    torch.cuda.synchronize()
    B, C, Ty = z_m.shape
    y_len = z_mask.squeeze(1).sum(1).long().tolist()
    noise = np.stack([H.prior_noise(seed, b, C, Ty) for b in range(B)])
    z64 = (z_m.cpu().numpy().astype(np.float64) + np.exp(z_logs.cpu().numpy().astype(np.float64)) * noise * float(np.float32(ns)))
    z64 = z64 * z_mask.cpu().numpy().astype(np.float64)
    rcy, rows = gen._front_last["rc"], gen._front_last["rows"]
    want_rows, inside = rows_reference(z64, y_len, rcy.row0.cpu().tolist(), rcy.R)
    got_rows = rows.cpu().numpy().astype(np.float64)
    e_rows = np.abs(got_rows - want_rows).max() / np.abs(want_rows).max()
    y_want = R.decoder_rev(P, "decoder.", torch.from_numpy(z64).float(), z_mask.cpu(), n_blocks=2)
    e = relerr(y.cpu(), y_want)
    print(f"seeded infer [fused_reverse={fused}]: latent rows vs host {e_rows:.3e} of max-abs, mel vs oracle {e:.3e}")
    assert (got_rows[~inside] == 0).all() and e_rows <= 1e-5, e_rows
    assert y.shape == y_want.shape and torch.isfinite(y).all()
    assert e < 3e-2, e
    assert min(y_len) < y.shape[2]
    for b in range(B):                                                             # padded frames of the mel
        assert y[b, :, y_len[b]:].numel() == 0 or y[b, :, y_len[b]:].abs().max().item() == 0


def test_a_seed_reproduces_the_call(built):
    gen, P, ids, xl = small_generator()
    gen.store_inverse(fused_reverse=True, device_front=True)

    def call(**kw):
        (y, z_m, z_logs, ld, z_mask), _, _, _ = gen.infer(ids, xl, noise_scale=0.667, **kw)
        torch.cuda.synchronize()
        return y.clone(), gen._front_last["rows"].clone(), z_mask.clone()

    torch.manual_seed(1)
    y1, r1, m1 = call(seed=77)
    torch.manual_seed(2)
    y2, r2, m2 = call(seed=77)
    assert torch.equal(r1, r2) and torch.equal(m1, m2)                             # the sampled latent and the lengths
    assert torch.equal(y1, y2)                                                     # ... and the mel, bit for bit
    y3, r3, m3 = call(seed=78)
    assert torch.equal(m1, m3) and not torch.equal(r1, r3) and not torch.equal(y1, y3)
    torch.manual_seed(3)
    y4, r4, _ = call()
    torch.manual_seed(3)
    y5, r5, _ = call()
    assert torch.equal(r4, r5) and torch.equal(y4, y5)                             # no seed=: torch.manual_seed governs the call
    torch.manual_seed(4)
    y6, r6, _ = call()
    assert not torch.equal(r4, r6)


def test_cfg5_infer_with_the_front_on(built):
    """cfg 5 cut to 2 decoder blocks / 2 encoder layers: the stochastic predictors draw from the generator's streams 1-3.
    noise_scale_w = 0 keeps the durations (so the shapes) those of the front-off call."""
    from glow_tts_amd import models
    from test_synthesis_fused_gpu import CFG5
    cfg = dict(CFG5, n_blocks_dec=2, n_layers_enc=2)
    gen = fill_module(models.FlowGenerator(n_vocab=187, out_channels=80, n_lang=10, **cfg), "").eval().to(dev())
    g = torch.Generator().manual_seed(2)
    B, Tx = 2, 15
    xl = torch.tensor([15, 9])
    ids = torch.randint(1, 187, (B, Tx), generator=g) * (torch.arange(Tx)[None, :] < xl[:, None])
    graw, emo = torch.randn(B, 512, generator=g), torch.randint(0, 5, (B,), generator=g)
    cart = torch.rand(B, 3, generator=g) * torch.tensor([1.5, 3.1, 4.6]) + torch.tensor([0.0, 0.0, -1.55])
    lid = torch.randint(0, 3, (B,), generator=g)
    d = lambda v: v.to(dev())                                         # noqa: E731
    kw = dict(g=d(graw), emo=d(emo), emo_cartesian=d(cart), l=d(lid), noise_scale=0.5, noise_scale_w=0.0)
    gen.store_inverse(fused_reverse=True, device_front=False)
    off = gen.infer(d(ids), d(xl), **kw)
    gen.set_synthesis_front(True)
    on = gen.infer(d(ids), d(xl), seed=7, **kw)
    on2 = gen.infer(d(ids), d(xl), seed=7, **kw)
    other = gen.infer(d(ids), d(xl), seed=8, **kw)
    torch.cuda.synchronize()
    for grp_on, grp_off in zip(on, off):
        for a, b in zip(grp_on, grp_off):
            assert (a is None) == (b is None)
            if a is not None:
                assert a.shape == b.shape and a.dtype == b.dtype
                assert torch.isfinite(a).all()
    (mel, z_m, z_logs, ld, z_mask), _, (attn, logw, logw_), (pit, ene) = on
    assert torch.equal(attn, off[2][0]) and torch.equal(z_mask, off[0][4])           # same durations on both paths
    assert torch.equal(pit, on2[3][0]) and torch.equal(ene, on2[3][1])               # pitch / energy reproduce under the seed
    assert not torch.equal(pit, other[3][0]) and not torch.equal(ene, other[3][1])
    # the frame -> token map the kernel returned (the predictors gathered with it) against the one rebuilt from attn
    a2 = attn.squeeze(1)
    want = torch.where(a2.sum(1) > 0, a2.argmax(1), torch.full_like(a2.argmax(1), -1)).int()
    f2t = gen._front_last["frame2token"]
    assert f2t.shape == want.shape and (want >= 0).any() and (want < 0).any()
    assert torch.equal(f2t, want)


_CHILD = r"""
import os, sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], "tests", "golden"))
import torch
from torch.utils._python_dispatch import TorchDispatchMode
from fill import fill_module
from glow_tts_amd import models, _lib
dev = torch.device("cuda:0")
gen = fill_module(models.FlowGenerator(148, 192, 768, 256, 80, use_sdp=False, kernel_size=3, n_heads=2, n_layers_enc=2, p_dropout=0.1,
                                       n_blocks_dec=2, kernel_size_dec=5, dilation_rate=1, n_block_layers=4, p_dropout_dec=0.05,
                                       n_sqz=2, window_size=4, mean_only=True, prenet=True), "").eval().to(dev)
g = torch.Generator().manual_seed(3)
xl = torch.tensor([19, 11])
ids = (torch.randint(1, 148, (2, 19), generator=g) * (torch.arange(19)[None, :] < xl[:, None])).to(dev)
xl = xl.to(dev)
# aten operators that only make a view, an allocation or a host-side answer: no kernel
FREE = {"view", "_unsafe_view", "reshape", "_reshape_alias", "transpose", "t", "permute", "squeeze", "unsqueeze", "expand", "slice",
        "select", "as_strided", "detach", "alias", "empty", "empty_like", "empty_strided", "new_empty", "new_empty_strided",
        "unbind", "split", "split_with_sizes", "unfold", "narrow", "is_pinned", "_local_scalar_dense", "lift_fresh", "_pin_memory",
        "resize_", "set_", "size", "stride", "numel", "sym_size", "is_same_size", "record_stream"}


class Count(TorchDispatchMode):
    def __init__(self):
        super().__init__()
        self.names = []

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        out = func(*args, **(kwargs or {}))
        name = func.overloadpacket.__name__
        flat = list(args) + list((kwargs or {}).values()) + (list(out) if isinstance(out, (tuple, list)) else [out])
        if name not in FREE and any(isinstance(t, torch.Tensor) and t.is_cuda for t in flat):
            self.names.append("aten::" + name)
        return out


assert type(_lib.lib()).__name__ == "_Traced", "GT_TRACE_CALLS is not in effect"
lines = []
for front in (False, True):
    gen.store_inverse(fused_reverse=True, device_front=front)
    kw = dict(seed=5) if front else {}
    gen.infer(ids, xl, noise_scale=0.667, **kw)          # warm-up: allocator, pinned staging, rows contexts
    torch.cuda.synchronize()
    with _lib.record_calls() as entries, Count() as c:
        out = gen.infer(ids, xl, noise_scale=0.667, **kw)
    torch.cuda.synchronize()
    assert torch.isfinite(out[0][0]).all()
    lines.append("front=%d entries=%d aten=%d" % (front, len(entries), len(c.names)))
    lines += ["  " + n for n in entries + c.names]
open(sys.argv[2], "w").write("\n".join(lines) + "\n")
"""


def test_launch_count_of_a_front_on_infer(built, tmp_path):
    """A fresh child process runs one infer with the front off and one with it on (same model, same inputs, fused reverse on both) and
    counts what each call puts on the device: the C-ABI entries (the binding's recorder) plus the aten operators that touch a device
    tensor and are not a view / allocation.  The front-on call must need fewer."""
    log = tmp_path / "launches.txt"
    env = dict(os.environ, GT_TRACE_CALLS=str(tmp_path / "last_call.txt"))
    try:
        p = subprocess.run([sys.executable, "-c", _CHILD, ROOT, str(log)], env=env, timeout=300, capture_output=True, text=True)
    except subprocess.TimeoutExpired:
        pytest.exit("the child process of the launch-count test ran into its time limit: nothing more is started on this GPU", returncode=1)
    if p.returncode in (124, 134, 137, 139, -6, -9, -11):                # time limit, abort, kill, segmentation fault: the card may be faulted
        last = (tmp_path / "last_call.txt").read_text().strip() if (tmp_path / "last_call.txt").exists() else "?"
        pytest.exit(f"the child process of the launch-count test died with status {p.returncode} (last C-ABI call: {last}): "
                    f"nothing more is started on this GPU\n{p.stderr[-2000:]}", returncode=1)
    if p.returncode != 0:
        pytest.fail(f"child exited with status {p.returncode}:\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}")
    text = log.read_text()
    print(text)
    counts = {}
    for line in text.splitlines():
        if line.startswith("front="):
            f = dict(kv.split("=") for kv in line.split())
            counts[int(f["front"])] = (int(f["entries"]), int(f["aten"]))
    off, on = sum(counts[0]), sum(counts[1])
    print(f"launches of one infer: front off {off} (C-ABI {counts[0][0]} + aten {counts[0][1]}), front on {on} (C-ABI {counts[1][0]} + aten {counts[1][1]})")
    assert "gt_synth_prior" in text and "gt_synth_lengths" in text
    assert on < off, (on, off)
