"""GPU tests of synthesis past 512 tokens: gt_synth_lengths_long / gt_synth_prior_long[_call] (csrc/synth_front.hip),
gt_attn_fwd with P == NULL (csrc/attn_long.hip), and FlowGenerator.infer / compile_synthesis on texts of 513 and 520 tokens.

The harnesses and the bounds are those of the short forms' tests: guarded buffers and generate_path for the two kernels
(tests/test_synthesis_front_gpu.py: integer and gathered outputs exact, logw to 1e-6, the fp32 rows within 1e-5 of max-abs of the float64
restatement and exact without noise), 3e-2 of max-abs for a mel against the float oracle's reverse decoder with the front-on error at
most twice the front-off one (floor 1e-3), bit-identity between a replayed graph and infer(seed=) on the same rows
(tests/test_synthesis_graph_gpu.py, tests/test_synthesis_graph_cfg5_gpu.py), bit-identity between the forward that stores P and the
one that does not.  Shapes: the smallest that reach each edge —
  Tx 513   x_len [513, 300]      the first length past the old limit, the last token in a 513th slot
  Tx 1025  x_len [1025, 1024, 7] past two 512-token chunks (65 threads of the scan), an utterance that ends on a chunk edge
  Tx 4096  x_len [4096], B = 1   the limit: every thread of the scan owns 16 tokens, 16 KiB of cum under the binary searches
  attention T 506 (T & 3 != 0: the scalar P path), 512, 513 (a key tile of one row), 4096."""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "golden"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import synth_noise_host as H  # noqa: E402
from fill import fill_module  # noqa: E402
from oracle import glowtts_ref as R  # noqa: E402
from test_synthesis_front_gpu import cpu_state, guarded, margins_untouched, relerr, rows_reference  # noqa: E402

pytestmark = pytest.mark.gpu
HALO = 2


def dev():
    return torch.device("cuda:0")


# ---- the two kernels called directly ------------------------------------------------------------------------------------------
def run_front(dur, x_len, x_m, x_logs, noise_scale, seed, ragged, long=True, with_attn=True):
    """gt_synth_lengths[_long] + gt_synth_prior[_long] on guarded buffers (run_front of tests/test_synthesis_front_gpu.py with the
    entries chosen by `long` and the attn output optional) -> dict of results on the host"""
    from glow_tts_amd import _lib, ops
    L = _lib.lib()
    st = _lib.current_stream(dev())
    lengths, prior = (L.gt_synth_lengths_long, L.gt_synth_prior_long) if long else (L.gt_synth_lengths, L.gt_synth_prior)
    B, Tx = dur.shape
    C = x_m.shape[1]
    dur_d, xl = dur.to(dev()).contiguous(), x_len.to(torch.int32).to(dev())
    f_cum, cum = guarded(B * Tx, torch.int32, -7)
    f_yl, y_len = guarded(B, torch.int32, -7)
    f_lw, logw = guarded(B * Tx, torch.float32, float("nan"))
    _lib.check(lengths(_lib.ptr(dur_d), _lib.ptr(xl), _lib.ptr(cum), _lib.ptr(y_len), _lib.ptr(logw), B, Tx, st), "lengths")
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
    f_at, attn = guarded(B * Tx * Ty, torch.float32, float("nan")) if with_attn else (None, None)
    xm_d = x_m.to(dev()).contiguous()
    xs_d = None if x_logs is None else x_logs.to(dev()).contiguous()
    args = _lib.fill_args(_lib.SynthPriorArgs, x_m=xm_d, x_logs=xs_d, cum=cum, x_len=xl, y_len=y_len, row0=rc.row0, Tp=rc.Tp, R=rc.R,
                          rows=rows, z_m=z_m, z_logs=z_logs, frame2token=f2t, attn=attn, B=B, C=C, Tx=Tx, Ty=Ty, seed=seed,
                          noise_scale=noise_scale)
    _lib.check(prior(ctypes.byref(args), st), "prior")
    torch.cuda.synchronize()
    for flat, n in ((f_rows, rc.R * 2 * C), (f_zm, B * C * Ty), (f_zl, B * C * Ty), (f_ft, B * Ty)) + (((f_at, B * Tx * Ty),) if with_attn else ()):
        assert margins_untouched(flat, n)
    return dict(cum=cum.view(B, Tx).cpu(), y_len=lens, logw=logw.view(B, Tx).cpu(), rows=rows.view(rc.R, 2 * C).cpu(),
                z_m=z_m.view(B, C, Ty).cpu(), z_logs=z_logs.view(B, C, Ty).cpu(), f2t=f2t.view(B, Ty).cpu(),
                attn=attn.view(B, Tx, Ty).cpu() if with_attn else None, rc=rc, Ty=Ty,
                base=rc.row0.cpu().tolist() if ragged else [b * rc.Tp for b in range(B + 1)])


@functools.lru_cache(maxsize=None)
def front_case(name):
    """(dur [B, Tx] with 0 on masked tokens, x_len, x_m, x_logs) of a named case, built once.  Tx19 / Tx512 are the cases of
    tests/test_synthesis_front_gpu.py, rebuilt."""
    g = torch.Generator().manual_seed(17)
    if name == "Tx19":
        xl = [19, 11, 19, 7, 19, 3]
        dur = torch.randint(0, 7, (6, 19), generator=g).float()
        dur[0, 0] = 0; dur[0, 9:12] = 0; dur[0, 18] = 0
        dur[0, 5] += 1 - dur[0].sum() % 2
        dur[2] = 0
        dur[5] = 0; dur[5, 1] = 2
    else:
        xl = {"Tx512": [512, 300], "Tx513": [513, 300], "Tx1025": [1025, 1024, 7], "Tx4096": [4096]}[name]
        Tx = max(xl)
        dur = torch.randint(0, 3, (len(xl), Tx), generator=g).float()
        dur[0, 0] = 0; dur[0, Tx - 1] = 0                         # zero durations at the first and at the last token of utterance 0
    Tx = dur.shape[1]
    dur = dur * (torch.arange(Tx)[None, :] < torch.tensor(xl)[:, None])
    B = dur.shape[0]
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


def check_front(name, mean_only, noise_scale, ragged, with_attn):
    dur, xl, x_m, x_logs = front_case(name)
    ref = front_reference(name)
    seed = 99
    out = run_front(dur, xl, x_m, None if mean_only else x_logs, noise_scale, seed, ragged, with_attn=with_attn)
    B, C, Ty = x_m.shape[0], 80, ref["Ty"]
    assert torch.equal(out["cum"], ref["cum"])
    assert out["y_len"] == ref["y_len"]
    assert torch.equal(out["f2t"], ref["f2t"])
    if with_attn:
        assert torch.equal(out["attn"], ref["attn"])
    assert torch.equal(out["z_m"], ref["z_m"])                                    # bit-equal to the gather
    assert torch.equal(out["z_logs"], torch.zeros_like(ref["z_logs"]) if mean_only else ref["z_logs"])
    assert torch.allclose(out["logw"], ref["logw"], rtol=1e-6, atol=1e-6)
    z_logs = np.zeros((B, C, Ty)) if mean_only else ref["z_logs"].numpy().astype(np.float64)
    noise = np.stack([H.prior_noise(seed, b, C, Ty) for b in range(B)])
    z = ref["z_m"].numpy().astype(np.float64) + np.exp(z_logs) * noise * float(np.float32(noise_scale))
    want, inside = rows_reference(z, ref["y_len"], out["base"], out["rc"].R)
    got = out["rows"].numpy().astype(np.float64)
    assert not np.isnan(got).any()                                                 # every row was written ...
    assert (got[~inside] == 0).all()                                               # ... halo / padding / rounding rows as zeros
    err = np.abs(got - want).max() / max(1e-6, np.abs(want).max())
    print(f"gt_synth_prior_long rows [{name}, mean_only={mean_only}, noise_scale={noise_scale}, ragged={ragged}]: {err:.3e} of max-abs")
    assert err <= 1e-5, err
    if noise_scale == 0.0:
        assert np.array_equal(got, want)


@pytest.mark.parametrize("ragged", [True, False])
@pytest.mark.parametrize("noise_scale", [0.0, 0.667])
@pytest.mark.parametrize("mean_only", [False, True])
@pytest.mark.parametrize("name", ["Tx513", "Tx1025"])
def test_long_lengths_and_prior_against_generate_path(built, name, mean_only, noise_scale, ragged):
    ref = front_reference(name)
    assert ref["cum"][0, 0] == 0 and ref["cum"][0, -1] == ref["cum"][0, -2]         # the zero durations at both ends of utterance 0
    check_front(name, mean_only, noise_scale, ragged, True)


@pytest.mark.parametrize("noise_scale", [0.0, 0.667])
def test_long_lengths_and_prior_at_the_token_limit(built, noise_scale):
    """Tx = 4096, B = 1, attn = NULL"""
    check_front("Tx4096", False, noise_scale, True, False)


@pytest.mark.parametrize("name", ["Tx19", "Tx512"])
def test_long_entries_equal_the_short_ones(built, name):
    dur, xl, x_m, x_logs = front_case(name)
    short = run_front(dur, xl, x_m, x_logs, 0.667, 99, True, long=False)
    long_ = run_front(dur, xl, x_m, x_logs, 0.667, 99, True, long=True)
    assert short["y_len"] == long_["y_len"] and short["base"] == long_["base"]
    for k in ("cum", "logw", "rows", "z_m", "z_logs", "f2t", "attn"):
        assert torch.equal(short[k], long_[k]), k
    assert long_["rows"].abs().max().item() > 0


def test_long_lengths_clamp(built):
    """every duration 1e9: clamped to 2^18 per token, 4096 tokens sum to 2^30 inside int32; a row of NaN durations counts as zeros"""
    from glow_tts_amd import _lib
    L = _lib.lib()
    st = _lib.current_stream(dev())
    Tx = 4096
    for fill, B in ((1e9, 1), (float("nan"), 1)):
        dur = torch.full((B, Tx), fill, dtype=torch.float32, device=dev())
        xl = torch.full((B,), Tx, dtype=torch.int32, device=dev())
        f_cum, cum = guarded(B * Tx, torch.int32, -7)
        f_yl, y_len = guarded(B, torch.int32, -7)
        _lib.check(L.gt_synth_lengths_long(_lib.ptr(dur), _lib.ptr(xl), _lib.ptr(cum), _lib.ptr(y_len), None, B, Tx, st), "gt_synth_lengths_long")
        torch.cuda.synchronize()
        assert margins_untouched(f_cum, B * Tx) and margins_untouched(f_yl, B)
        c = cum.cpu().long()
        if fill == 1e9:
            assert torch.equal(c, (torch.arange(Tx) + 1) << 18)                    # strictly increasing, non-negative
            assert bool((c[1:] > c[:-1]).all()) and int(c.min()) > 0
            assert y_len.cpu().tolist() == [1 << 30]
        else:
            assert bool((c == 0).all()) and y_len.cpu().tolist() == [1]


# ---- FlowGenerator.infer at 513 tokens ---------------------------------------------------------------------------------------------
def build_generator():
    """the model of tests/test_synthesis_front_gpu.py::small_generator"""
    from glow_tts_amd import models
    gen = fill_module(models.FlowGenerator(148, 192, 768, 256, 80, use_sdp=False, kernel_size=3, n_heads=2, n_layers_enc=2, p_dropout=0.1,
                                           n_blocks_dec=2, kernel_size_dec=5, dilation_rate=1, n_block_layers=4,
                                           p_dropout_dec=0.05, n_sqz=2, window_size=4, mean_only=True, prenet=True), "").eval()
    return gen.to(dev()), cpu_state(gen)


def text(Tx, xl, seed=3):
    g = torch.Generator().manual_seed(seed)
    xl = torch.tensor(xl)
    ids = torch.randint(1, 148, (len(xl), Tx), generator=g) * (torch.arange(Tx)[None, :] < xl[:, None])
    return ids, xl


@pytest.mark.parametrize("fused", [False, True])
def test_infer_front_on_against_front_off_at_513_tokens(built, fused):
    gen, P = build_generator()
    ids, xl = text(513, [513, 260])
    ids, xl = ids.to(dev()), xl.to(dev())
    res = []
    for front in (False, True):
        assert gen.store_inverse(fused_reverse=fused, device_front=front) == (fused, front)
        (y, z_m, z_logs, ld, z_mask), (x_m, x_logs, x_mask), (attn, logw, logw_), (pit, ene) = \
            gen.infer(ids, xl, noise_scale=0.0, length_scale=1.0, **(dict(seed=5) if front else {}))
        torch.cuda.synchronize()
        res.append(dict(y=y.clone(), z_m=z_m.clone(), z_logs=z_logs.clone(), z_mask=z_mask.clone(), attn=attn.clone(),
                        logw=logw.clone(), logw_=logw_.clone()))
    off, on = res
    lens = on["z_mask"].squeeze(1).sum(1).long().tolist()
    print(f"513 tokens: predicted lengths {lens}")
    assert 513 <= max(lens) <= 4096                                                # every real token has at least one frame
    for k in ("attn", "logw", "logw_", "z_m", "z_logs", "z_mask"):
        assert on[k].shape == off[k].shape and on[k].dtype == off[k].dtype, k
        assert torch.equal(on[k], off[k]), k
    assert on["attn"].shape[2] == 513
    assert on["y"].shape == off["y"].shape and on["y"].dtype == off["y"].dtype
    zk = on["z_mask"].cpu()
    y_want = R.decoder_rev(P, "decoder.", on["z_m"].cpu() * zk, zk, n_blocks=2)
    e_off, e_on = relerr(off["y"].cpu(), y_want), relerr(on["y"].cpu(), y_want)
    print(f"infer mel vs oracle at 513 tokens [fused_reverse={fused}]: front off {e_off:.3e}, front on {e_on:.3e}")
    assert torch.isfinite(on["y"]).all()
    assert e_on < 3e-2, e_on
    assert e_on <= max(2 * e_off, 1e-3), (e_on, e_off)


def test_seeded_infer_at_513_tokens(built):
    gen, P = build_generator()
    ids, xl = text(513, [513, 260])
    gen.store_inverse(fused_reverse=True, device_front=True)
    ns, seed = 0.667, 1234
    (y, z_m, z_logs, ld, z_mask), _, _, _ = gen.infer(ids.to(dev()), xl.to(dev()), noise_scale=ns, seed=seed)
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
    print(f"seeded infer at 513 tokens: lengths {y_len}, latent rows vs host {e_rows:.3e} of max-abs, mel vs oracle {e:.3e}")
    assert (got_rows[~inside] == 0).all() and e_rows <= 1e-5, e_rows
    assert y.shape == y_want.shape and torch.isfinite(y).all()
    assert e < 3e-2, e
    assert min(y_len) < y.shape[2]
    for b in range(B):                                                             # padded frames of the mel
        assert y[b, :, y_len[b]:].numel() == 0 or y[b, :, y_len[b]:].abs().max().item() == 0


# ---- the captured graph --------------------------------------------------------------------------------------------------------------
GB, GTX = 2, 520
# (text length, x_lengths, seed, noise_scale, length_scale): a long text, and a short one through the same synthesiser (stretched over
# more than one 64-frame tile of the prior kernel)
GCALLS = ((520, [520, 506], 5, 0.667, 1.0), (19, [19, 11], 9, 0.3, 40.0))


def rows_needed(lens):
    return sum(v // 2 + 2 * HALO for v in lens)


def eager(gen, ids, xl, seed, ns, ls):
    """infer(seed=) on x padded to max_tokens -> clones of what the replay is compared with"""
    xp = torch.zeros(GB, GTX, dtype=ids.dtype)
    xp[:, :ids.shape[1]] = ids
    (y, z_m, z_logs, _, z_mask), _, (attn, logw, logw_), _ = gen.infer(xp.to(dev()), xl.to(dev()), noise_scale=ns, length_scale=ls, seed=seed)
    torch.cuda.synchronize()
    return dict(y=y.clone(), z_m=z_m.clone(), z_logs=z_logs.clone(), attn=attn.clone(), logw=logw.clone(), logw_=logw_.clone(),
                lens=z_mask.squeeze(1).sum(1).long().tolist())


@functools.lru_cache(maxsize=None)
def graph_setup():
    """as setup() of tests/test_synthesis_graph_gpu.py: the eager path is run once to learn the lengths, the capacities hold them, the
    eager references are computed with rows_cfg.row_round = max_rows (the same R and row0 as the graph's capacity context)"""
    gen, P = build_generator()
    assert gen.store_inverse(fused_reverse=True, device_front=True) == (True, True)
    tx = [text(Tx, xl, seed=21 + i) + (seed, ns, ls) for i, (Tx, xl, seed, ns, ls) in enumerate(GCALLS)]
    probe = [eager(gen, *t)["lens"] for t in tx]
    max_frames = (max(max(v) for v in probe) + 1) // 2 * 2
    max_rows = -(-max(rows_needed(v) for v in probe) // 128) * 128
    gen.rows_cfg.row_round = max_rows
    refs = [eager(gen, *t) for t in tx]
    print(f"predicted lengths {probe}: max_frames {max_frames}, max_rows {max_rows}")
    synth = gen.compile_synthesis(GB, GTX, max_frames, max_rows=max_rows, aux=True)
    return gen, tx, refs, synth


def test_graph_at_520_tokens_equals_eager(built):
    gen, tx, refs, synth = graph_setup()
    assert synth.max_tokens == 520
    for (ids, xl, seed, ns, ls), ref in zip(tx, refs):
        h = synth(ids, xl, seed=seed, noise_scale=ns, length_scale=ls)
        lens = h.lengths()
        assert h.status == 0 and lens == ref["lens"]
        y = h.mel()
        assert y.shape == ref["y"].shape and y.dtype == ref["y"].dtype
        assert torch.equal(y, ref["y"])                                            # bit-identical
        a = h.aux()
        for k in ("attn", "logw", "logw_", "z_m", "z_logs"):
            assert a[k].shape == ref[k].shape, k
            assert torch.equal(a[k], ref[k]), k
    assert synth.overflows == 0 and synth.guards_intact()
    assert max(refs[0]["lens"]) >= 520 and max(refs[1]["lens"]) > 64
    ids, xl = text(521, [521, 3])
    with pytest.raises(ValueError, match="max_tokens"):
        synth(ids, xl)


def test_compile_synthesis_limits(built):
    gen, tx, refs, synth = graph_setup()
    with pytest.raises(ValueError, match="4096"):
        gen.compile_synthesis(2, 4097, 64)
    with pytest.raises(ValueError, match=str(1024 * 4096 * 4096)):                 # the static attn buffer, before any allocation
        gen.compile_synthesis(1024, 4096, 4096, aux=True)


def test_full_model_graph_at_513_tokens_equals_eager(built):
    """cfg 5 cut to 2 decoder blocks / 2 encoder layers (tests/test_synthesis_graph_cfg5_gpu.py), x_lengths [513, 400]: the stochastic
    duration predictor, the frame-rate rows of the pitch / energy predictors and the contours, all past 512 tokens"""
    from test_synthesis_graph_cfg5_gpu import build_cfg5, frame_rows_needed, round_up
    from test_synthesis_graph_cfg5_gpu import eager as eager5
    from test_synthesis_graph_cfg5_gpu import rows_needed as rows_needed5
    gen, P = build_cfg5()
    g = torch.Generator().manual_seed(2)
    B, Tx = 2, 513
    xl = torch.tensor([513, 400])
    ids = torch.randint(1, 187, (B, Tx), generator=g) * (torch.arange(Tx)[None, :] < xl[:, None])
    cond = dict(g=torch.randn(B, 512, generator=g), emo=torch.randint(0, 5, (B,), generator=g),
                emo_cartesian=torch.rand(B, 3, generator=g) * torch.tensor([1.5, 3.1, 4.6]) + torch.tensor([0.0, 0.0, -1.55]),
                l=torch.randint(0, 3, (B,), generator=g))
    call = dict(seed=7, noise_scale=0.5, noise_scale_w=0.4, f0_noise_scale=0.6, energy_noise_scale=0.7, length_scale=1.0, pitch_scale=1.25,
                energy_scale=0.75)
    assert gen.set_synthesis_front(True, noise_key="frame") is True
    lens = eager5(gen, ids, xl, cond, **call)["lens"]
    print(f"cfg 5 at 513 tokens: predicted lengths {lens}")
    assert 513 <= max(lens) <= 4096
    max_frames = (max(lens) // 2 + 1) * 2 + 8
    X = round_up(frame_rows_needed(lens), 128)
    assert X >= rows_needed5(lens)
    gen.rows_cfg.row_round = X
    ref = eager5(gen, ids, xl, cond, **call)
    assert ref["lens"] == lens
    synth = gen.compile_synthesis(B, Tx, max_frames, max_rows=X, stochastic=True, max_frame_rows=X)
    h = synth(ids, xl, **cond, **call)
    assert h.lengths() == lens and h.status == 0
    y = h.mel()
    assert y.shape == ref["y"].shape and torch.equal(y, ref["y"])
    pitch, energy = h.prosody()
    assert pitch.shape == ref["pitch"].shape and torch.equal(pitch, ref["pitch"])
    assert energy.shape == ref["energy"].shape and torch.equal(energy, ref["energy"])
    assert ref["pitch"].abs().max().item() > 0 and ref["energy"].abs().max().item() > 0
    assert synth.overflows == 0 and synth.guards_intact()


# ---- the forward that stores no P ---------------------------------------------------------------------------------------------------
D, WIN, GUARD, CANARY = 96, 4, 8, 768.0


def attn_outs(T, lens, Hh, p):
    """gt_attn_fwd twice on the same operands in the guarded harness of tests/test_attn_long_fp64_gpu.py (ragged rows, guard rows,
    canaries on every row no store may touch): with P, and with P == NULL -> the two whole `out` buffers, the mask of the rows the
    utterances own, P"""
    from glow_tts_amd import _lib, ops
    L = _lib.lib()
    B, C = len(lens), Hh * D
    assert L.gt_attn_long_shape(T, D, WIN) == 1
    lens_t = torch.tensor(lens, dtype=torch.int32, device=dev())
    rc = ops.RowsCtx(lens_t, T, lengths_host=lens, round_to=128)
    R_ = rc.R
    g = torch.Generator().manual_seed(7 * T + D)
    qkv = ((torch.randn(R_, 3 * C, generator=g) * 0.5) * rc.rowmask[:, None].cpu()).to(torch.bfloat16)
    Ek, Ev = (torch.randn(2 * WIN + 1, D, generator=g) * 0.1).to(dev()), (torch.randn(2 * WIN + 1, D, generator=g) * 0.1).to(dev())
    row0 = rc.row0.cpu().tolist()
    written = torch.zeros(R_ + 2 * GUARD, dtype=torch.bool)
    for b in range(B):
        written[GUARD + row0[b] + ops.HALO:GUARD + row0[b] + ops.HALO + min(T, row0[b + 1] - row0[b] - ops.HALO)] = True
    qb = torch.full((R_ + 2 * GUARD, 3 * C), float("nan"), dtype=torch.bfloat16, device=dev())
    qb[GUARD:GUARD + R_] = qkv.to(dev())
    qv = qb[GUARD:GUARD + R_]
    q, k, v = qv[:, :C], qv[:, C:2 * C], qv[:, 2 * C:]
    st = _lib.current_stream(dev())
    P = torch.full((B, Hh, T, T), float("nan"), dtype=torch.float32, device=dev())
    outs = []
    for Pp in (P, None):
        ob = torch.full((R_ + 2 * GUARD, C), CANARY, dtype=torch.bfloat16, device=dev())
        _lib.check(L.gt_attn_fwd(_lib.ptr(q), _lib.ptr(k), _lib.ptr(v), 3 * C, _lib.ptr(Ek), _lib.ptr(Ev), _lib.ptr(rc.lengths),
                                 _lib.ptr(ob[GUARD:GUARD + R_]), C, _lib.ptr(Pp), B, T, rc.Tp, _lib.ptr(rc.row0), Hh, D, WIN, p, 0x51ED270B,
                                 None, st), "gt_attn_fwd")
        torch.cuda.synchronize()
        outs.append(ob.cpu())
    return outs[0], outs[1], written, P


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("T", [506, 512, 513])
def test_forward_without_p_writes_the_same_out(built, T, p):
    with_p, without, written, P = attn_outs(T, [T - 7, T], 2, p)
    assert bool(torch.isfinite(P).all())
    for buf in (with_p, without):
        assert bool((buf[~written].float() == CANARY).all()), "a store outside the rows the utterances own"
        assert bool(torch.isfinite(buf[written].float()).all())
    assert torch.equal(with_p, without)
    assert with_p[written].float().abs().max().item() > 0


def test_forward_without_p_at_the_token_limit(built):
    with_p, without, written, P = attn_outs(4096, [4089], 1, 0.0)
    assert bool((without[~written].float() == CANARY).all())
    assert torch.equal(with_p, without)
    assert with_p[written].float().abs().max().item() > 0


# ---- the encoder ---------------------------------------------------------------------------------------------------------------------
def test_encoder_keep_p_flag(built):
    from glow_tts_amd.text_models import _TextEncoderRunner
    gen, _ = build_generator()
    gen.prepare()
    te = gen.encoder
    assert not te.training
    ids, xl = text(513, [513, 260])
    ids, xl = ids.to(dev()), xl.to(dev())
    with torch.no_grad():
        kept = [t.clone() for t in te(ids, xl, prepared=True)]
        free = [t.clone() for t in te(ids, xl, prepared=True, keep_p=False)]
        torch.cuda.synchronize()
        for a, b, name in zip(kept, free, ("x", "x_m", "x_logs", "x_mask")):
            assert a.shape == b.shape and torch.equal(a, b), name
        assert kept[0].abs().max().item() > 0 and bool(torch.isfinite(kept[1]).all())

        def saved_p(Tx, lens, keep_p):
            i, l = text(Tx, lens)
            _, (rc, s_pre, s_layers, xb) = _TextEncoderRunner(te, i.to(dev()), l.to(dev()), False, seed=0, keep_p=keep_p).forward()
            assert len(s_layers) == 2
            return [s[0][5] for s in s_layers]                                     # P of each layer's attention tuple

        assert all(p is None for p in saved_p(513, [513, 260], False))
        assert all(p is not None and tuple(p.shape) == (2, 2, 513, 513) for p in saved_p(513, [513, 260], True))
        assert all(p is not None and tuple(p.shape) == (2, 2, 150, 150) for p in saved_p(150, [150, 90], False))
        torch.cuda.synchronize()
