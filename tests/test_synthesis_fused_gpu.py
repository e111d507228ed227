"""GPU tests of the fused synthesis path: gt_wn_boundary_rev (ONE kernel between consecutive WaveNets in the reverse direction,
csrc/wn_boundary.hip), gt_wn_stack_fwd without the backward's saves, flow_impl.decoder_rev_fused and the public switch
FlowSpecDecoder.set_fused_reverse / FlowGenerator.store_inverse(fused_reverse=True).

Tolerances are the project's existing ones for the reverse direction (tests/test_decoder_gpu.py): 3e-2 of the tensor's max-abs
against the float oracle (bf16 GEMM operands and bf16 hidden activations), 5e-3 * max(1, max|z|) for forward(reverse(z)) == z.
The fused path rounds where the launch sequence rounds (bf16 acts, wn_out, x0) and differs from it only in fp32 accumulation
order, so its error against the oracle may be at most twice the launch sequence's on the same inputs (floor 1e-3)."""
import ctypes
import os
import subprocess
import sys

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "golden"))
from fill import fill_module  # noqa: E402
from oracle import glowtts_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def dev():
    return torch.device("cuda:0")


def relerr(a, b):
    return (a - b).abs().max().item() / max(1e-6, b.abs().max().item())


def lens_mask(lengths, T):
    l = torch.tensor(lengths)
    return (torch.arange(T)[None, :] < l[:, None]).unsqueeze(1).float()


def cpu_state(mod, prefix=""):
    return {prefix + k: v.detach().cpu().float() for k, v in mod.state_dict().items()}


# (name, T, lengths, ragged rows layout): the lengths of test_fused_boundary_kernels_match_the_five_kernel_path (a 2-frame
# utterance; 370 uniform / 240 ragged rows, neither a multiple of 64) in both layouts, and uniform rows with an odd T
LAYOUTS = [("uniform", 140, [140, 66, 2, 128, 90], False), ("ragged", 140, [140, 66, 2, 128, 90], True), ("odd_T", 65, [65, 30, 2], False)]


def _reverse_both_ways(dec, z, m, g, lens, ragged, **contours):
    """dec(z, reverse=True) with the switch on and off -> (fused, launch sequence), on the rows layout asked for"""
    from glow_tts_amd import ops
    dec.rows_cfg = ops.RowsConfig(ragged=ragged, row_round=8)
    out = []
    try:
        for on in (True, False):
            assert dec.set_fused_reverse(on) == on
            if ragged:
                dec.rows_cfg.host_lengths["y"] = list(lens)
            x, ld = dec(z, m, g=g, reverse=True, **contours)
            torch.cuda.synchronize()
            assert ld is None
            out.append(x.clone())
    finally:
        dec.rows_cfg = ops.RowsConfig()
        dec.set_fused_reverse(False)
    return out


@pytest.mark.parametrize("ragged", [False, True])
@pytest.mark.parametrize("with_energy", [False, True])
@pytest.mark.parametrize("n_blocks", [2, 3])
def test_fused_reverse_with_pitch_and_energy_contours(built, n_blocks, with_energy, ragged):
    """cfg 5's decoder in the reverse direction with the switch on: every block is the chain wn(g) -> [wn_energy(energy)] ->
    wn_pitch(pitch) (attentions.py:152-154); the fused path runs a skip GEMM between chained WaveNets (wn acts-only, the
    affine-conditioned ones in the saving form) and gt_wn_boundary_rev behind the LAST of them (its skip-cat image and bias).  Pitch alone and pitch + energy,
    uniform and ragged rows, against oracle/glowtts_ref.decoder_rev(..., pitch=, energy=) and against the launch sequence with the
    bounds of the test above."""
    from glow_tts_amd import flow_impl, models
    B, T, lens = 3, 50, [50, 27, 12]
    dec = fill_module(models.FlowSpecDecoder(80, 192, 5, 1, n_blocks, 4, p_dropout=0.05, gin_channels=256, with_prosody_wn=True),
                      "decoder.").eval()
    P = cpu_state(dec, "decoder.")
    dec = dec.to(dev())
    gen = torch.Generator().manual_seed(21 + n_blocks)
    m = lens_mask(lens, T)
    z = torch.randn(B, 80, T, generator=gen) * m
    spk = torch.randn(B, 256, 1, generator=gen)
    pit = torch.randn(B, 1, T, generator=gen) * m
    ene = torch.randn(B, 1, T, generator=gen).abs() * m if with_energy else None
    want = R.decoder_rev(P, "decoder.", z, m, spk, n_blocks=n_blocks, pitch=pit, energy=ene)
    plain = R.decoder_rev(P, "decoder.", z, m, spk, n_blocks=n_blocks)
    assert relerr(plain, want) > 1e-2                                   # the contours matter at these weights
    flow_impl.BOUNDARY_TRACE = trace = []
    try:
        fused, seq = _reverse_both_ways(dec, z.to(dev()), m.to(dev()), spk.to(dev()), lens, ragged, pitch=pit.to(dev()),
                                        energy=None if ene is None else ene.to(dev()))
    finally:
        flow_impl.BOUNDARY_TRACE = None
    assert [name for name, _, _ in trace] == ["gt_wn_boundary_rev"] * (n_blocks + 1)     # the fused path ran, once
    chain_len = 3 if with_energy else 2
    last = [dec.flows[3 * b + 2].wn_pitch for b in range(n_blocks)]     # the boundary kernel reads the LAST WaveNet's skip image
    for k, (_, _, kw) in enumerate(trace[1:], start=1):
        assert kw["w_skip"].data_ptr() == last[n_blocks - k].pc_skipcat_frag.fwd.data_ptr(), k
    e_f, e_s, d = relerr(fused.cpu(), want), relerr(seq.cpu(), want), relerr(fused, seq)
    print(f"fused reverse, contours [{n_blocks} blocks, chain of {chain_len}, ragged={ragged}]: "
          f"fused vs oracle {e_f:.3e}, launch sequence vs oracle {e_s:.3e}, fused vs launch sequence {d:.3e}")
    assert torch.isfinite(fused).all()
    assert e_s < 3e-2, e_s
    assert e_f < 3e-2, e_f
    assert e_f <= max(2 * e_s, 1e-3), (e_f, e_s)


@pytest.mark.parametrize("sigmoid_scale", [False, True])
@pytest.mark.parametrize("speaker", [False, True])
@pytest.mark.parametrize("n_blocks", [2, 3, 12])
def test_fused_reverse_vs_oracle_and_launch_sequence(built, n_blocks, speaker, sigmoid_scale):
    """The fused reverse pass and round 1's launch sequence on the same module and inputs (eval mode), each against
    oracle/glowtts_ref.decoder_rev: 2 / 3 / 12 blocks (head-only, full and tail-only launches all run), speaker vector on / off,
    sigmoid_scale on / off; ragged lengths with a 2-frame utterance in both rows layouts and uniform rows with an odd T."""
    from glow_tts_amd import models
    gin = 256 if speaker else 0
    dec = fill_module(models.FlowSpecDecoder(80, 192, 5, 1, n_blocks, 4, p_dropout=0.05, sigmoid_scale=sigmoid_scale, gin_channels=gin),
                      "decoder.").eval()
    P = cpu_state(dec, "decoder.")
    dec = dec.to(dev())
    assert dec.fused_reverse is False                                   # opt-in: the default is the launch sequence
    for name, T, lens, ragged in LAYOUTS:
        B = len(lens)
        gen = torch.Generator().manual_seed(9 + n_blocks)
        m = lens_mask(lens, T)
        z = torch.randn(B, 80, T, generator=gen) * m
        g = torch.randn(B, gin, 1, generator=gen) if speaker else None
        want = R.decoder_rev(P, "decoder.", z, m, g, n_blocks=n_blocks, sigmoid_scale=sigmoid_scale)
        fused, seq = _reverse_both_ways(dec, z.to(dev()), m.to(dev()), None if g is None else g.to(dev()), lens, ragged)
        assert fused.shape == want.shape == seq.shape
        e_f, e_s, d = relerr(fused.cpu(), want), relerr(seq.cpu(), want), relerr(fused, seq)
        print(f"fused reverse [{n_blocks} blocks, speaker={speaker}, sigmoid_scale={sigmoid_scale}, {name}]: "
              f"fused vs oracle {e_f:.3e}, launch sequence vs oracle {e_s:.3e}, fused vs launch sequence {d:.3e}")
        assert torch.isfinite(fused).all()
        assert e_s < 3e-2, (name, e_s)
        assert e_f < 3e-2, (name, e_f)
        assert e_f <= max(2 * e_s, 1e-3), (name, e_f, e_s)
        pad = ~(m[:, :, :fused.shape[2]].bool().expand_as(fused.cpu()))
        assert fused.cpu()[pad].abs().max().item() == 0                 # frames past an utterance's length stay zero


def test_round_trip_with_the_switch_on(built):
    """forward(reverse_fused(z)) == z at 12 blocks, to the 5e-3 * max(1, max|z|) of test_decoder_reverse_vs_oracle_and_round_trip."""
    from glow_tts_amd import models
    n_blocks, T, lens = 12, 65, [65, 30, 2]
    dec = fill_module(models.FlowSpecDecoder(80, 192, 5, 1, n_blocks, 4, p_dropout=0.05), "decoder.").eval().to(dev())
    assert dec.set_fused_reverse(True) is True
    B = len(lens)
    m = lens_mask(lens, T)
    z = torch.randn(B, 80, T, generator=torch.Generator().manual_seed(9)) * m
    x, _ = dec(z.to(dev()), m.to(dev()), reverse=True)
    with torch.no_grad():
        z2, _ = dec(x, m.to(dev())[:, :, :x.shape[2]])
    T2 = x.shape[2]
    valid = (m[:, :, :T2] * (torch.arange(T2)[None, None, :] < (torch.tensor(lens) // 2 * 2)[:, None, None])).bool().expand(B, 80, T2)
    err = (z2.cpu() - z[:, :, :T2])[valid].abs().max().item()
    print("round trip through the fused reverse, 12 blocks:", err)
    assert err < 5e-3 * max(1.0, z.abs().max().item()), err


def test_uninitialised_actnorm_falls_back_to_the_launch_sequence(built):
    from glow_tts_amd import flow_impl, models
    dec = fill_module(models.FlowSpecDecoder(80, 192, 5, 1, 2, 4), "decoder.").eval().to(dev())
    assert dec.set_fused_reverse(True)
    m = lens_mask([40, 22], 40).to(dev())
    z = torch.randn(2, 80, 40, device=dev()) * m
    flow_impl.BOUNDARY_TRACE = trace = []
    try:
        x1, _ = dec(z, m, reverse=True)
        n_fused = len(trace)
        dec.flows[3].initialized = False
        x2, _ = dec(z, m, reverse=True)
    finally:
        flow_impl.BOUNDARY_TRACE = None
        dec.flows[3].initialized = True
    assert n_fused == 3 and len(trace) == 3                            # the second call launched no reverse boundary kernel
    assert relerr(x1, x2) < 1e-2
    small = models.FlowSpecDecoder(80, 128, 5, 1, 2, 4)                # a shape the kernels are not built for
    assert small.set_fused_reverse(True) is False


def test_reverse_boundary_kernel_keeps_to_its_rows(built):
    """gt_wn_boundary_rev called directly in its three variants (the launches of a real 2-block pass, recorded and re-issued):
    x, h_next and the [B, 80, T] output between canary guards, acts and the incoming flow state exactly R rows long between NaN
    guards.  No byte outside the operands changes, no guard row is read, the results equal the unguarded pass, and rows past the
    last utterance's frames (and every halo row) come out zero."""
    from glow_tts_amd import _lib, flow_impl, models, modules, ops
    L = _lib.lib()
    GUARD, CAN = 8, 768.0
    dec = fill_module(models.FlowSpecDecoder(80, 192, 5, 1, 2, 4, p_dropout=0.05), "decoder.").eval().to(dev())
    modules.prepare_all(dec)
    lens, T = [70, 33, 1, 64, 45], 140                                 # squeezed lengths; T = un-squeezed frames
    B = len(lens)
    rc = ops.RowsCtx(torch.tensor(lens, dtype=torch.int32, device=dev()), T // 2, lengths_host=lens, round_to=8)
    assert rc.R % 64 != 0 and rc.R > sum(lens) + 4 * B                  # the last utterance owns rounding rows
    z = torch.randn(B, 80, T, generator=torch.Generator().manual_seed(4)).to(dev()) * lens_mask([2 * v for v in lens], T).to(dev())
    x_ref = torch.zeros(B, 80, T, device=dev())
    flow_impl.BOUNDARY_TRACE = trace = []
    try:
        flow_impl.decoder_rev_fused(rc, dec, None, [None, None], z_bct=z, x_bct=x_ref)
    finally:
        flow_impl.BOUNDARY_TRACE = None
    torch.cuda.synchronize()
    assert [bool(kw.get("acts") is not None) for _, _, kw in trace] == [False, True, True]
    assert [bool(kw.get("h_next") is not None) for _, _, kw in trace] == [True, True, False]

    def guarded(t, fill):
        buf = torch.full((t.shape[0] + 2 * GUARD,) + tuple(t.shape[1:]), fill, dtype=t.dtype, device=dev())
        buf[GUARD:GUARD + t.shape[0]] = t
        return buf, buf[GUARD:GUARD + t.shape[0]]

    masked = rc.rowmask == 0
    assert masked[-4:].all()
    for name, _, kw in trace:
        kw = dict(kw)
        ins, outs = {}, {}
        for k in ("acts", "z"):                                        # inputs: NaN outside the R rows
            if kw.get(k) is not None:
                ins[k], kw[k] = guarded(kw[k], float("nan"))
        for k in ("x", "h_next"):                                      # outputs: canaries outside, canaries inside (every row < R is written)
            if kw.get(k) is not None:
                outs[k] = (kw[k],) + guarded(torch.full_like(kw[k], CAN), CAN)
                kw[k] = outs[k][2]
        if kw.get("x_bct") is not None:
            flat = torch.full((B * 80 * T + 2 * 4096,), CAN, device=dev())
            flat[4096:4096 + B * 80 * T] = 0                            # pre-zeroed by the caller
            outs["x_bct"] = (kw["x_bct"], flat, flat[4096:4096 + B * 80 * T].view(B, 80, T))
            kw["x_bct"] = outs["x_bct"][2]
        args = _lib.fill_args(_lib.BoundaryRevArgs, **kw)
        _lib.check(L.gt_wn_boundary_rev(ctypes.byref(args), _lib.current_stream(dev())), name)
        torch.cuda.synchronize()
        for k, (ref, buf, view) in outs.items():
            if k == "x_bct":
                assert (buf[:4096] == CAN).all() and (buf[4096 + B * 80 * T:] == CAN).all(), k
            else:
                assert (buf[:GUARD].float() == CAN).all() and (buf[GUARD + rc.R:].float() == CAN).all(), k
                assert (view[masked].float() == 0).all(), k               # halo rows and the rows past the last utterance
            assert torch.isfinite(view.float()).all(), k                  # no NaN guard row was read, no canary is left inside
            assert not (view.float() == CAN).any() or k == "x_bct", k
            assert torch.equal(view, ref), k
    assert x_ref.abs().max().item() > 0


def _stack_call(rc, wn, h0, cond, per_row, acts, ts, ss, xs, affine=None):
    """gt_wn_stack_fwd on explicit output lists (None entries = NULL) -> return code; affine = (aff_w [O], aff_b [O], aff_sig [R, 2])
    instead of cond: the per-frame conditioning formed in the kernel"""
    from glow_tts_amd import _lib
    n, H = wn.n_layers, 192
    pad = [None] * (4 - n)
    args = _lib.fill_args(
        _lib.WnStackFwdArgs, x0=h0, w_in=[il.pc.fwd for il in wn.in_layers] + pad, b_in=[il.bias for il in wn.in_layers] + pad,
        w_res=[rs.pc_res.fwd for rs in wn.res_skip_layers[:n - 1]] + [None] + pad, b_res=[rs.bias for rs in wn.res_skip_layers[:n - 1]] + [None] + pad,
        cond=cond, ldc=0 if cond is None else cond.stride(0), row0=rc.row0 if (cond is not None and not per_row) else None,
        B=0 if (per_row or cond is None) else rc.B, Tp=rc.Tp, rowmask=rc.rowmask, acts=acts, ldacts=acts.stride(0),
        gate_t=ts + pad, gate_s=ss + pad, x_out=xs + [None] + pad, R=rc.R, H=H, taps=5, n_layers=n, drop_p=0.0, drop_seed=0,
        **({} if affine is None else dict(aff_w=affine[0], aff_b=affine[1], aff_sig=affine[2])))
    rcode = _lib.lib().gt_wn_stack_fwd(ctypes.byref(args), _lib.current_stream(dev()))
    torch.cuda.synchronize()
    return rcode


@pytest.mark.parametrize("n", [2, 4])
@pytest.mark.parametrize("mode", ["none", "speaker", "per_row"])
def test_wn_stack_without_the_backwards_saves(built, mode, n):
    """gt_wn_stack_fwd with NULL gate_t / gate_s / x_out against the saving call on the same inputs: acts EQUAL, for the three
    conditioning modes (none, per utterance, per row), 2 and 4 layers, ragged rows, and row counts on both sides of the 32-row / 64-row form
    (gt_wn_stack_row_blocks); a mixed NULL / non-NULL set is GT_E_INVAL and launches nothing."""
    from glow_tts_amd import _lib, modules, ops
    L = _lib.lib()
    H = 192
    gin = 256 if mode == "speaker" else 0
    wn = fill_module(modules.WN(160, H, 5, 1, n, gin, 0.05), "wn.").to(dev()).eval()
    modules.prepare_all(wn)
    forms = set()
    for lens in ([131, 70, 2, 1, 64, 97], [640, 601, 2, 577, 640, 333, 512, 640, 498, 640, 620, 611]):
        rc = ops.RowsCtx(torch.tensor(lens, dtype=torch.int32, device=dev()), max(lens), lengths_host=lens, round_to=8)
        forms.add(L.gt_wn_stack_row_blocks(rc.R, n, 1))
        g = torch.Generator().manual_seed(31 + n)
        h0 = ((torch.randn(rc.R, H, generator=g)).to(dev()) * rc.rowmask[:, None]).to(torch.bfloat16)
        cond = None
        if mode == "speaker":
            cond = (torch.randn(rc.B, 2 * H * n, generator=g) * 0.3).to(dev())
        elif mode == "per_row":
            cond = (torch.randn(rc.R, 2 * H * n, generator=g) * 0.3).to(dev())
        aff = None
        bf = dict(dtype=torch.bfloat16, device=dev())
        mk = lambda k: [torch.zeros(rc.R, H, **bf) for _ in range(k)]
        a_save, a_none = torch.zeros(rc.R, n * H, **bf), torch.zeros(rc.R, n * H, **bf)
        ts, ss, xs = mk(n), mk(n), mk(n - 1)
        assert _stack_call(rc, wn, h0, cond, mode == "per_row", a_save, ts, ss, xs, aff) == 0
        assert _stack_call(rc, wn, h0, cond, mode == "per_row", a_none, [None] * n, [None] * n, [None] * (n - 1), aff) == 0
        assert a_save.float().abs().max().item() > 0 and ts[0].float().abs().max().item() > 0
        assert torch.equal(a_save, a_none)
        a_mix = torch.full((rc.R, n * H), 768.0, **bf)
        assert _stack_call(rc, wn, h0, cond, mode == "per_row", a_mix, mk(n), [None] * n, mk(n - 1), aff) == -1      # GT_E_INVAL
        assert _stack_call(rc, wn, h0, cond, mode == "per_row", a_mix, [None] * n, [None] * n, mk(n - 1), aff) == -1
        assert (a_mix.float() == 768.0).all()                                                                    # nothing was launched
    assert forms == {1, 2}, forms


def test_wn_stack_acts_only_is_not_offered_with_affine_conditioning(built):
    """The acts-only form is built where its acts equal the saving form's bit for bit.  With the affine per-frame conditioning formed in
    the kernel they did not (measured: 16 of 4.9 M acts one bf16 ulp apart in the 64-row form at 4 layers, none in the other three
    cases — the compiler fuses `b + contour * w` differently per instantiation), so that combination is GT_E_UNSUPPORTED and launches
    nothing; the saving call with the same arguments runs."""
    from glow_tts_amd import modules, ops
    H, n = 192, 4
    wn = fill_module(modules.WN(160, H, 5, 1, n, 0, 0.05), "wn.").to(dev()).eval()
    modules.prepare_all(wn)
    lens = [131, 70, 2, 1, 64, 97]
    rc = ops.RowsCtx(torch.tensor(lens, dtype=torch.int32, device=dev()), max(lens), lengths_host=lens, round_to=8)
    g = torch.Generator().manual_seed(5)
    h0 = ((torch.randn(rc.R, H, generator=g)).to(dev()) * rc.rowmask[:, None]).to(torch.bfloat16)
    aff = ((torch.randn(H * n, generator=g) * 0.3).to(dev()), (torch.randn(H * n, generator=g) * 0.3).to(dev()), torch.randn(rc.R, 2, generator=g).to(dev()))
    bf = dict(dtype=torch.bfloat16, device=dev())
    mk = lambda k: [torch.zeros(rc.R, H, **bf) for _ in range(k)]
    acts = torch.full((rc.R, n * H), 768.0, **bf)
    assert _stack_call(rc, wn, h0, None, False, acts, [None] * n, [None] * n, [None] * (n - 1), aff) == -2         # GT_E_UNSUPPORTED
    assert (acts.float() == 768.0).all()
    assert _stack_call(rc, wn, h0, None, False, acts, mk(n), mk(n), mk(n - 1), aff) == 0
    assert not (acts.float() == 768.0).all()


def test_infer_with_the_switch_on(built):
    """The model of test_infer_generates_mel_through_the_reverse_flow, noise_scale = 0: store_inverse(fused_reverse=True) leaves
    attn, z_m and the durations as they are with the switch off, and the mel stays within 3e-2 of the oracle's reverse decoder."""
    from glow_tts_amd import models
    gen = fill_module(models.FlowGenerator(148, 192, 768, 256, 80, use_sdp=False, kernel_size=3, n_heads=2, n_layers_enc=2, p_dropout=0.1,
                                           n_blocks_dec=2, kernel_size_dec=5, dilation_rate=1, n_block_layers=4,
                                           p_dropout_dec=0.05, n_sqz=2, window_size=4, mean_only=True, prenet=True), "").eval()
    P = cpu_state(gen)
    g = torch.Generator().manual_seed(3)
    ids = torch.randint(1, 148, (2, 19), generator=g); xl = torch.tensor([19, 11])
    ids = ids * (torch.arange(19)[None, :] < xl[:, None])
    gen = gen.to(dev())
    res = []
    for on in (False, True):
        assert gen.store_inverse(fused_reverse=on) is on
        assert gen.decoder.fused_reverse is on
        (y, z_m, z_logs, ld, z_mask), (x_m, x_logs, x_mask), (attn, logw, logw_), _ = gen.infer(ids.to(dev()), xl.to(dev()), noise_scale=0.0)
        torch.cuda.synchronize()
        res.append((y.clone(), z_m.clone(), attn.clone(), logw.clone(), z_mask.clone()))
    (y0, zm0, at0, lw0, zk0), (y1, zm1, at1, lw1, zk1) = res
    assert torch.equal(at0, at1) and torch.equal(zm0, zm1) and torch.equal(lw0, lw1) and torch.equal(zk0, zk1)
    y_want = R.decoder_rev(P, "decoder.", zm1.cpu() * zk1.cpu(), zk1.cpu(), n_blocks=2)
    e0, e1 = relerr(y0.cpu(), y_want), relerr(y1.cpu(), y_want)
    print(f"infer mel vs oracle: launch sequence {e0:.3e}, fused reverse {e1:.3e}, between them {relerr(y1, y0):.3e}")
    assert torch.isfinite(y1).all() and e1 < 3e-2, e1


CFG5 = dict(hidden_channels=192, filter_channels=768, filter_channels_dp=256, kernel_size=3, p_dropout=0.1, n_blocks_dec=12,
            n_layers_enc=10, n_heads=2, p_dropout_dec=0.05, dilation_rate=1, kernel_size_dec=5, n_block_layers=4, n_sqz=2,
            prenet=True, mean_only=True, hidden_channels_enc=192, hidden_channels_dec=192, window_size=4, gin_channels=512,
            use_sdp=True, use_spk_embeds=True, use_lang_embeds=True, use_emo_embeds=True, lin_channels=4, emoin_channels=1024,
            use_spp=True, use_sep=True)      # == configs/base_blank_emo_lang_pitch.json "model"


def test_voice_conversion_with_the_switch_on(built):
    """The model of test_voice_conversion_round_trip: with the reverse half on the fused path, same speaker on both sides stays
    an identity to 5e-3 of max|y|, another target gives another mel, padded frames stay zero."""
    from glow_tts_amd import flow_impl, models
    cfg = dict(CFG5, n_blocks_dec=3, n_layers_enc=1, gin_channels=64, use_emo_embeds=False, use_spp=False, use_sep=False, use_sdp=False)
    gen = models.FlowGenerator(n_vocab=187, out_channels=80, n_lang=10, **cfg)
    gen.emb_g = torch.nn.Linear(512, 64)
    gen = fill_module(gen, "").eval().to(dev())
    for b in range(3):                                                    # a coupling that does something (end is zero-initialised)
        torch.nn.init.normal_(gen.decoder.flows[3 * b + 2].end.weight, std=0.02)
    assert gen.store_inverse(fused_reverse=True) is True
    g = torch.Generator().manual_seed(11)
    yl = torch.tensor([40, 32])
    y = (torch.randn(2, 80, 40, generator=g) * lens_mask(yl.tolist(), 40)).to(dev())
    e_src, e_tgt = torch.randn(2, 512, generator=g).to(dev()), torch.randn(2, 512, generator=g).to(dev())
    flow_impl.BOUNDARY_TRACE = trace = []
    try:
        same = gen.voice_conversion(y, yl.to(dev()), e_src, e_src)
    finally:
        flow_impl.BOUNDARY_TRACE = None
    assert sum(name == "gt_wn_boundary_rev" for name, _, _ in trace) == 4    # the reverse half ran the fused path (3 blocks)
    err = (same - y).abs().max().item()
    print("same-speaker voice conversion through the fused reverse:", err / y.abs().max().item())
    assert same.shape == y.shape and err < 5e-3 * y.abs().max().item()
    other = gen.voice_conversion(y, yl.to(dev()), e_src, e_tgt)
    assert torch.isfinite(other).all() and (other - y).abs().max().item() > 1e-2
    assert other[1, :, 32:].abs().max().item() == 0.0


_CHILD = r"""
import os, sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], "tests", "golden"))
import torch
from fill import fill_module
from glow_tts_amd import models, ops
dev = torch.device("cuda:0")
dec = fill_module(models.FlowSpecDecoder(80, 192, 5, 1, 12, 4, p_dropout=0.05), "decoder.").eval().to(dev)
dec.store_inverse(fused_reverse=True)
assert dec.fused_reverse
lens, T = [140, 66, 2, 128, 90], 140
m = (torch.arange(T)[None, :] < torch.tensor(lens)[:, None]).unsqueeze(1).float().to(dev)
z = torch.randn(len(lens), 80, T, device=dev) * m
dec.rows_cfg = ops.RowsConfig(ragged=True)
dec.rows_cfg.host_lengths["y"] = list(lens)
x, _ = dec(z, m, reverse=True)                     # warm-up: the rows context, allocator
torch.cuda.synchronize()
from glow_tts_amd import _lib
assert type(_lib.lib()).__name__ == "_Traced", "GT_TRACE_CALLS is not in effect"
dec.rows_cfg.host_lengths["y"] = list(lens)
with _lib.record_calls() as names:
    x, _ = dec(z, m, reverse=True)
torch.cuda.synchronize()
assert torch.isfinite(x).all()
open(sys.argv[2], "w").write("\n".join(names) + "\n")
"""


def test_launch_count_of_a_fused_reverse_pass(built, tmp_path):
    """A fresh child process with GT_TRACE_CALLS set (every C-ABI entry goes through the binding's tracer) runs one 12-block fused
    reverse pass after store_inverse on ragged rows with an even T: exactly 13 gt_wn_boundary_rev and 12 gt_wn_stack_fwd entries,
    and none of the launch sequence's GEMM / coupling / ActNorm / squeeze / unsqueeze entries."""
    log = tmp_path / "entries.txt"
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
    names = log.read_text().split()
    count = lambda n: sum(v == n for v in names)
    print("entries of one fused 12-block reverse pass:", {n: count(n) for n in sorted(set(names))})
    assert count("gt_wn_boundary_rev") == 13 and count("gt_wn_stack_fwd") == 12, names
    for banned in ("gt_conv_gemm_bf16", "gt_coupling_rev", "gt_actnorm_invconv_rev", "gt_squeeze_rows_f32", "gt_unsqueeze_rows_f32"):
        assert count(banned) == 0, (banned, names)
