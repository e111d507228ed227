"""dev: synthesis time of the flow decoder, reverse=True, launch sequence vs fused path (FlowSpecDecoder.set_fused_reverse).

A cfg 2 decoder (12 blocks x 4 layers, H = 192) after store_inverse; `dec(z, mask, reverse=True)` with the switch off and on,
alternating in the same process, every shape warmed up first, device events around >= 0.5 s of calls per variant and a
synchronise behind them, two repeats.  Two shapes: the bench batch (B = 32, train.synth_batch lengths, T_y <= 800) and one
utterance of 800 frames (the latency case).  The rows context of a shape is built once and reused by both variants
(RowsConfig.prebuilt), so neither pays for the pinned staging buffer of a ragged context inside the timed loop.
Per variant: time per call, C-ABI launches per call, HBM bytes per call computed from the shapes below (activations read and
written by every launch + each launch's weight images once; L2 hits and halo re-reads are not modelled).

    python tools/synth_bench.py [--json out.json] [--seconds 0.5] [--repeats 2] [--shape both|batch|single]

--infer: whole FlowGenerator.infer calls instead (text in, mel out, the call's device-to-host readback included), graph-free, same
warm-up and repeat rule, fused_reverse on: the device front end (set_synthesis_front) off and on, alternating.  A cfg 2 model whose
duration predictor is pinned to 5 frames per token (zero projection weight, bias log 4.9), so the mel lengths are 5 x the text
lengths: the bench batch (B = 32, train.synth_batch's text lengths, T_y <= 750) and one utterance of 160 tokens = 800 frames.
Per variant: wall time per call, what one call puts on the device (C-ABI entries + aten operators on device tensors).  On a tree
without set_synthesis_front only the front-off variant is measured (the parent's numbers for the run-to-run spread).

--graph: whole calls again, three variants alternating in one process with the same windows and repeats: eager infer with the device
front end on (the call's readback included), the captured graph of FlowGenerator.compile_synthesis replayed call by call (each call's
upload, replay and readback, `mel()` taken before the next call), and N calls queued before the first is read (--queue N; every
handle is kept and its mel read afterwards, so each call but the last also pays the device copy that moves its outputs aside).  The
same model and the same two shapes as --infer; the batch is compiled at its own sizes (150 tokens, 750 frames), the single utterance
at 160 tokens and 800 frames and, to show what unused capacity costs, at 1600 frames.  Every repeat is recorded; output defaults to
profiles/synth_graph_bench.json.

--cfg5 [--graph]: the FULL model (tests/test_synthesis_fused_gpu.py's CFG5: emotion front end, stochastic duration predictor in
reverse, stochastic pitch / energy predictors at the frame rate, 10 encoder layers, 12 decoder blocks), whole infer calls on the same
two shapes with the same windows and repeats, the variants alternating in one process.  The stochastic duration predictor keeps all
its work but its last flow (the elementwise affine, log_scale = 20) maps every draw to log w = 0, so with length_scale = 4.9 every
token gets 5 frames.  Variants: eager with noise_key="row" (the path before DESIGN.md 4.14: row-keyed noise, uniform frame rows, four
launches per contour), eager with noise_key="frame" on uniform frame rows (rows_cfg.frame_rows_ragged = False) and on ragged ones
(the default), and with --graph the captured graph of compile_synthesis(stochastic=True) replayed call by call.  Three ratios per
shape: replay over eager-frame, eager-frame over eager-row, ragged over uniform frame rows.  Every repeat is recorded; output defaults
to profiles/synth_graph_cfg5_bench.json.

--graph --wav: whole calls to SAMPLES, 30 Griffin-Lim iterations, the same model and the same two shapes, three
ways alternating in one process, three windows of >= 0.5 s each, a host clock ending in a synchronise: (a) what a caller had before
compile_synthesis(vocoder=) — the graph replayed to the mel, the lengths read back, GriffinLim.from_mel with torch phases; (a') the
same with phases="counter" (one gt_gl_from_mel launch instead of the ATen ops and the phase tensor); (b) the ONE graph of
compile_synthesis(vocoder=GriffinLim, vocoder_iters=30) and h.wav(); and, to split (a') into its parts, the text-to-mel replay alone
and from_mel(phases="counter") alone on the batch's own mel.  The bench batch is RAGGED (train.synth_batch's text lengths, 5 frames per
token, the longest at the capacity): the JSON records every utterance's frames, their total and the seconds of audio.  For the single
utterance (b) is also compiled at 1600 frames, to show what unused capacity costs a loop whose every launch is sized by it.  Every window is recorded; output defaults to
profiles/synth_wav_bench.json.

--tokens BxT[,BxT...] (--infer, --graph): texts of a given length instead of the two shapes above, e.g. `--tokens 1x1024,8x600` (long
texts); --front off|on|both picks the variants of --infer.

Kernel times come from separate runs, one per shape, under
`rocprofv3 --kernel-trace --stats -- python tools/synth_bench.py --seconds 0.1 --repeats 1 --shape batch` (or `single`)."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from glow_tts_amd import _lib, models, ops, train  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--json", default=None)
ap.add_argument("--seconds", type=float, default=0.5)
ap.add_argument("--repeats", type=int, default=2)
ap.add_argument("--infer", action="store_true", help="time whole infer calls, device front end off / on")
ap.add_argument("--graph", action="store_true", help="time eager infer against the captured synthesis graph (compile_synthesis)")
ap.add_argument("--cfg5", action="store_true", help="the full cfg 5 model: eager row / frame keyed calls (and with --graph the captured graph)")
ap.add_argument("--wav", action="store_true", help="--graph: time whole calls to samples, mel graph + from_mel against the one graph with a vocoder")
ap.add_argument("--queue", type=int, default=16, help="--graph: replays queued before one synchronisation")
ap.add_argument("--tokens", default=None, help="--infer / --graph: the shapes as BxT[,BxT...], B texts of T tokens each (5 T frames), "
                "e.g. 1x1024,8x600, instead of the two default shapes")
ap.add_argument("--front", choices=["both", "off", "on"], default="both", help="--infer: the variants to time")
ap.add_argument("--shape", choices=["both", "batch", "single"], default="both", help="one shape only (a kernel-trace run per shape)")
opt = ap.parse_args()

dev = torch.device("cuda:0")
NB, NL, H, C = 12, 4, 192, 160
torch.manual_seed(0)
if not opt.infer and not opt.graph and not opt.cfg5:
    dec = models.FlowSpecDecoder(80, H, 5, 1, NB, NL, p_dropout=0.05).to(dev).eval()
    for b in range(NB):                                                # a coupling that does something (end is zero-initialised)
        torch.nn.init.normal_(dec.flows[3 * b + 2].end.weight, std=0.01)
    dec.store_inverse()


def numel_bytes(t):
    return t.numel() * t.element_size()


def weight_bytes():
    """bytes of the packed images one block's launches read: (WaveNet, skip-cat, end, start)"""
    cb = dec.flows[2]
    wn = cb.wn
    wnb = sum(numel_bytes(il.pc.fwd) for il in wn.in_layers) + sum(numel_bytes(rs.pc_res.fwd) for rs in wn.res_skip_layers[:NL - 1])
    return wnb, numel_bytes(wn.pc_skipcat_frag.fwd), numel_bytes(cb.end.pc_frag.fwd), numel_bytes(cb.start.pc_frag.fwd)


def hbm_bytes(R, B, T, fused):
    """HBM bytes of one reverse pass from the shapes: every launch's activation reads + writes and its weight images once (ragged rows,
    even T: the fused path's first / last launch squeeze / unsqueeze)."""
    wn_w, skip_w, end_w, start_w = weight_bytes()
    f32row, bct = R * C * 4, B * 80 * T * 4
    h, x0, acts = R * H * 2, R * 80 * 2, R * NL * H * 2
    if not fused:
        per_block = (x0 + start_w + h) \
            + (h + wn_w + acts + 2 * NL * h + (NL - 1) * h) \
            + (acts + skip_w + h) \
            + (h + end_w + f32row) \
            + (2 * f32row + f32row) \
            + (f32row + f32row + x0)
        return NB * per_block + (bct + f32row) + (f32row // 2 + x0) + (f32row + bct)
    wn = h + wn_w + acts                                               # acts only
    full = acts + skip_w + end_w + f32row + f32row + start_w + h
    head = bct + f32row + start_w + h
    tail = acts + skip_w + end_w + f32row + bct
    return NB * wn + (NB - 1) * full + head + tail


def shape(name, lens, T):
    B = len(lens)
    m = (torch.arange(T)[None, :] < torch.tensor(lens)[:, None]).unsqueeze(1).float().to(dev)
    z = torch.randn(B, 80, T, device=dev) * m
    sq = [v // 2 for v in lens]
    rc = ops.RowsCtx(torch.tensor(sq, dtype=torch.int32, device=dev), T // 2, lengths_host=sq, round_to=128)
    return dict(name=name, B=B, T=T, z=z, m=m, rc=rc)


def run(sh, on, n):
    dec.set_fused_reverse(on)
    for _ in range(n):
        dec(sh["z"], sh["m"], reverse=True)


def main():
    _, _, _, t_y = train.synth_batch(32, 150, 800, 0, "cpu")
    shapes = ([shape("bench batch: B = 32, T_y <= 800", [int(v) for v in t_y], 800)] if opt.shape != "single" else []) + \
        ([shape("one utterance, 800 frames", [800], 800)] if opt.shape != "batch" else [])
    out = dict(device=torch.cuda.get_device_name(0), decoder="cfg 2: 12 blocks x 4 layers, H = 192, eval, store_inverse", rows_ctx="prebuilt, ragged, round 128",
               seconds_per_variant=opt.seconds, shapes=[])
    dec.rows_cfg = ops.RowsConfig(ragged=True)
    for sh in shapes:
        dec.rows_cfg.prebuilt["y"] = sh["rc"]
        rec = dict(name=sh["name"], B=sh["B"], T=sh["T"], rows=sh["rc"].R, workgroups_per_boundary_launch=(sh["rc"].R + 63) // 64, variants={})
        xs = {}
        for on in (False, True):                                       # warm-up, launch count, result
            assert dec.set_fused_reverse(on) == on
            run(sh, on, 3)
            with _lib.record_calls() as names:
                xs[on], _ = dec(sh["z"], sh["m"], reverse=True)
            torch.cuda.synchronize()
            rec["variants"]["fused" if on else "launch_sequence"] = dict(
                launches_per_call=len(names), launches={k: names.count(k) for k in sorted(set(names))},
                hbm_bytes_per_call=hbm_bytes(sh["rc"].R, sh["B"], sh["T"], on), ms_per_call=[])
        rec["max_abs_difference"] = (xs[True] - xs[False]).abs().max().item()
        rec["max_abs_output"] = xs[False].abs().max().item()
        for rep in range(opt.repeats):
            for on in (False, True):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(); run(sh, on, 5); e1.record(); torch.cuda.synchronize()
                n = max(5, int(opt.seconds * 1e3 / (e0.elapsed_time(e1) / 5)) + 1)
                e0.record(); run(sh, on, n); e1.record(); torch.cuda.synchronize()
                rec["variants"]["fused" if on else "launch_sequence"]["ms_per_call"].append(round(e0.elapsed_time(e1) / n, 4))
        for v in rec["variants"].values():
            t = v["ms_per_call"]
            v["ms_mean"], v["ms_spread"] = round(sum(t) / len(t), 4), round(max(t) - min(t), 4)
        a, b = rec["variants"]["launch_sequence"], rec["variants"]["fused"]
        rec["fused_over_launch_sequence_time"] = round(b["ms_mean"] / a["ms_mean"], 4)
        print(f'{sh["name"]}: rows {sh["rc"].R}; launch sequence {a["ms_mean"]:.3f} ms (+- {a["ms_spread"]:.3f}), {a["launches_per_call"]} launches, '
              f'{a["hbm_bytes_per_call"] / 1e6:.1f} MB; fused {b["ms_mean"]:.3f} ms (+- {b["ms_spread"]:.3f}), {b["launches_per_call"]} launches, '
              f'{b["hbm_bytes_per_call"] / 1e6:.1f} MB', flush=True)
        out["shapes"].append(rec)
    dec.rows_cfg = ops.RowsConfig()
    dec.set_fused_reverse(False)
    if opt.json:
        os.makedirs(os.path.dirname(os.path.abspath(opt.json)), exist_ok=True)
        with open(opt.json, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


def token_cases():
    """--tokens BxT[,BxT...] -> [(name, ids [B, T], x_lengths [B])]"""
    g = torch.Generator().manual_seed(5)
    out = []
    for spec in opt.tokens.split(","):
        B, T = (int(v) for v in spec.lower().split("x"))
        out.append((f"{B} x {T} tokens = {5 * T} frames each", torch.randint(1, 148, (B, T), generator=g), torch.full((B,), T)))
    return out


def infer_main():
    import math
    import time
    from torch.utils._python_dispatch import TorchDispatchMode
    gen = models.FlowGenerator(148, 192, 768, 256, 80, use_sdp=False, kernel_size=3, n_heads=2, n_layers_enc=6, p_dropout=0.1,
                               n_blocks_dec=NB, kernel_size_dec=5, dilation_rate=1, n_block_layers=NL, p_dropout_dec=0.05, n_sqz=2,
                               window_size=4, mean_only=True, prenet=True).eval()
    with torch.no_grad():
        for b in range(NB):
            torch.nn.init.normal_(gen.decoder.flows[3 * b + 2].end.weight, std=0.01)
        gen.encoder.proj_w.proj.weight.zero_()                         # 5 frames per token: ceil(4.9)
        gen.encoder.proj_w.proj.bias.fill_(math.log(4.9))
    gen = gen.to(dev)
    has_front = hasattr(gen, "set_synthesis_front")
    gen.store_inverse(fused_reverse=True)
    # aten operators that only make a view, an allocation or a host-side answer: no kernel
    free = {"view", "_unsafe_view", "reshape", "_reshape_alias", "transpose", "t", "permute", "squeeze", "unsqueeze", "expand", "slice",
            "select", "as_strided", "detach", "alias", "empty", "empty_like", "empty_strided", "new_empty", "new_empty_strided",
            "unbind", "split", "split_with_sizes", "narrow", "is_pinned", "_local_scalar_dense", "lift_fresh", "_pin_memory", "resize_",
            "set_", "is_same_size", "record_stream"}

    class Count(TorchDispatchMode):
        n = 0

        def __torch_dispatch__(self, func, types, args=(), kwargs=None):
            res = func(*args, **(kwargs or {}))
            flat = list(args) + list((kwargs or {}).values()) + (list(res) if isinstance(res, (tuple, list)) else [res])
            if func.overloadpacket.__name__ not in free and any(isinstance(t, torch.Tensor) and t.is_cuda for t in flat):
                self.n += 1
            return res

    ids_b, t_x, _, _ = train.synth_batch(32, 150, 800, 0, "cpu")
    g = torch.Generator().manual_seed(5)
    cases = [("bench batch: B = 32, T_x <= 150, 5 frames per token", ids_b, t_x),
             ("one utterance, 160 tokens = 800 frames", torch.randint(1, 148, (1, 160), generator=g), torch.tensor([160]))]
    if opt.tokens:
        cases = token_cases()
    variants = [v for v in ([False, True] if has_front else [False]) if opt.front in ("both", "on" if v else "off")]
    name_of = {False: "front_off", True: "front_on"}

    def call(ids, xl, front, n):
        if has_front:
            gen.set_synthesis_front(front)
        for _ in range(n):
            res = gen.infer(ids, xl, noise_scale=0.667)
        return res

    out = dict(device=torch.cuda.get_device_name(0), model="cfg 2: 6 encoder layers, 12 blocks x 4 layers, H = 192, eval, store_inverse(fused_reverse=True)",
               seconds_per_variant=opt.seconds, device_front_available=has_front, shapes=[])
    for name, ids, xl in cases:
        ids, xl = ids.to(dev), xl.to(dev)
        rec = dict(name=name, B=int(ids.shape[0]), Tx=int(ids.shape[1]), variants={})
        for front in variants:
            res = call(ids, xl, front, 3)
            with _lib.record_calls() as names, Count() as cnt:
                res = call(ids, xl, front, 1)
            torch.cuda.synchronize()
            assert torch.isfinite(res[0][0]).all()
            rec["T_y"] = int(res[0][0].shape[2])
            rec["variants"][name_of[front]] = dict(c_abi_entries=len(names), aten_device_ops=cnt.n, launches_per_call=len(names) + cnt.n,
                                                   ms_per_call=[])
        for rep in range(opt.repeats):
            for front in variants:
                torch.cuda.synchronize(); t0 = time.perf_counter(); call(ids, xl, front, 5); torch.cuda.synchronize()
                n = max(5, int(opt.seconds / ((time.perf_counter() - t0) / 5)) + 1)
                torch.cuda.synchronize(); t0 = time.perf_counter(); call(ids, xl, front, n); torch.cuda.synchronize()
                rec["variants"][name_of[front]]["ms_per_call"].append(round((time.perf_counter() - t0) * 1e3 / n, 4))
        for v in rec["variants"].values():
            t = v["ms_per_call"]
            v["ms_mean"], v["ms_spread"] = round(sum(t) / len(t), 4), round(max(t) - min(t), 4)
        if len(variants) == 2:
            rec["front_on_over_front_off_time"] = round(rec["variants"]["front_on"]["ms_mean"] / rec["variants"]["front_off"]["ms_mean"], 4)
        print(f'{name}: T_y {rec["T_y"]}; ' + "; ".join(f'{k} {v["ms_mean"]:.3f} ms (+- {v["ms_spread"]:.3f}), {v["launches_per_call"]} launches '
                                                        f'({v["c_abi_entries"]} C-ABI + {v["aten_device_ops"]} aten)' for k, v in rec["variants"].items()), flush=True)
        out["shapes"].append(rec)
    if has_front:
        gen.set_synthesis_front(False)
    if opt.json:
        os.makedirs(os.path.dirname(os.path.abspath(opt.json)), exist_ok=True)
        with open(opt.json, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


def graph_main():
    import math
    import time
    gen = models.FlowGenerator(148, 192, 768, 256, 80, use_sdp=False, kernel_size=3, n_heads=2, n_layers_enc=6, p_dropout=0.1,
                               n_blocks_dec=NB, kernel_size_dec=5, dilation_rate=1, n_block_layers=NL, p_dropout_dec=0.05, n_sqz=2,
                               window_size=4, mean_only=True, prenet=True).eval()
    with torch.no_grad():
        for b in range(NB):
            torch.nn.init.normal_(gen.decoder.flows[3 * b + 2].end.weight, std=0.01)
        gen.encoder.proj_w.proj.weight.zero_()                         # 5 frames per token: ceil(4.9)
        gen.encoder.proj_w.proj.bias.fill_(math.log(4.9))
    gen = gen.to(dev)
    assert gen.store_inverse(fused_reverse=True, device_front=True) == (True, True)
    ids_b, t_x, _, _ = train.synth_batch(32, 150, 800, 0, "cpu")
    g = torch.Generator().manual_seed(5)
    one = torch.randint(1, 148, (1, 160), generator=g)
    cases = []
    if opt.shape != "single":
        cases.append(("bench batch: B = 32, T_x <= 150, 5 frames per token", ids_b, t_x, [(int(ids_b.shape[1]), 5 * int(ids_b.shape[1]))]))
    if opt.shape != "batch":
        cases.append(("one utterance, 160 tokens = 800 frames", one, torch.tensor([160]), [(160, 800), (160, 1600)]))
    if opt.tokens:
        cases = [(name, ids, xl, [(int(ids.shape[1]), 5 * int(ids.shape[1]))]) for name, ids, xl in token_cases()]
    out = dict(device=torch.cuda.get_device_name(0), model="cfg 2: 6 encoder layers, 12 blocks x 4 layers, H = 192, eval, "
               "store_inverse(fused_reverse=True, device_front=True)", seconds_per_variant=opt.seconds, queued_calls=opt.queue, shapes=[])
    for name, ids, xl, caps in cases:
        ids_d, xl_d = ids.to(dev), xl.to(dev)
        B = int(ids.shape[0])

        def eager(n):
            for _ in range(n):
                res = gen.infer(ids_d, xl_d, noise_scale=0.667, seed=7)     # synchronises inside: its one readback
            return res[0][0]

        rec = dict(name=name, B=B, Tx=int(ids.shape[1]), variants={})
        want = eager(3)
        with _lib.record_calls() as names:
            eager(1)
        torch.cuda.synchronize()
        rec["T_y"] = int(want.shape[2])
        runs = {"eager_front_on": eager}
        rec["variants"]["eager_front_on"] = dict(c_abi_entries_per_call=len(names), ms_per_call=[])
        for Tx_cap, Ty_cap in caps:
            synth = gen.compile_synthesis(B, Tx_cap, Ty_cap)

            def replay(n, synth=synth):
                for _ in range(n):
                    y = synth(ids, xl, seed=7, noise_scale=0.667).mel()     # waits for this call's readback
                return y

            def queued(n, synth=synth):
                hs = [synth(ids, xl, seed=7, noise_scale=0.667) for _ in range(n)]     # every handle is kept and read: each unread call's
                return [h.mel() for h in hs][-1]                                       # mel is copied aside before the next replay

            got = replay(3)
            tag = f"{Tx_cap}x{Ty_cap}"
            rec["variants"]["replay_" + tag] = dict(max_tokens=Tx_cap, max_frames=Ty_cap, max_rows=synth.max_rows, launches_per_call="1 upload + 1 graph replay + 1 readback",
                                                    c_abi_entries_inside_the_graph=synth.captured_entries,
                                                    max_abs_difference_to_eager=(got - want).abs().max().item(), overflows=synth.overflows, ms_per_call=[])
            rec["variants"]["queued_" + tag] = dict(max_tokens=Tx_cap, max_frames=Ty_cap, max_rows=synth.max_rows, calls_per_synchronisation=opt.queue, ms_per_call=[])
            runs["replay_" + tag] = replay
            runs["queued_" + tag] = queued
        for rep in range(opt.repeats):
            for k, fn in runs.items():
                unit = opt.queue if k.startswith("queued_") else 1
                torch.cuda.synchronize(); t0 = time.perf_counter(); fn(5 * unit) if unit == 1 else [fn(unit) for _ in range(2)]; torch.cuda.synchronize()
                per = (time.perf_counter() - t0) / (5 if unit == 1 else 2 * unit)
                n = max(5, int(opt.seconds / per) + 1)
                torch.cuda.synchronize(); t0 = time.perf_counter()
                if unit == 1:
                    fn(n)
                else:
                    n = -(-n // unit) * unit
                    for _ in range(n // unit):
                        fn(unit)
                torch.cuda.synchronize()
                rec["variants"][k]["ms_per_call"].append(round((time.perf_counter() - t0) * 1e3 / n, 4))
        for v in rec["variants"].values():
            t = v["ms_per_call"]
            v["ms_mean"], v["ms_spread"] = round(sum(t) / len(t), 4), round(max(t) - min(t), 4)
        base = rec["variants"]["eager_front_on"]["ms_mean"]
        for k, v in rec["variants"].items():
            if k != "eager_front_on":
                v["over_eager_time"] = round(v["ms_mean"] / base, 4)
        print(f'{name}: T_y {rec["T_y"]}; ' + "; ".join(f'{k} {v["ms_mean"]:.3f} ms (+- {v["ms_spread"]:.3f})' for k, v in rec["variants"].items()), flush=True)
        out["shapes"].append(rec)
    path = opt.json or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "synth_graph_bench.json")
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


def wav_main():
    import math
    import time
    from glow_tts_amd import audio
    iters, windows = 30, max(3, opt.repeats)
    gen = models.FlowGenerator(148, 192, 768, 256, 80, use_sdp=False, kernel_size=3, n_heads=2, n_layers_enc=6, p_dropout=0.1,
                               n_blocks_dec=NB, kernel_size_dec=5, dilation_rate=1, n_block_layers=NL, p_dropout_dec=0.05, n_sqz=2,
                               window_size=4, mean_only=True, prenet=True).eval()
    with torch.no_grad():
        for b in range(NB):
            torch.nn.init.normal_(gen.decoder.flows[3 * b + 2].end.weight, std=0.01)
        gen.encoder.proj_w.proj.weight.zero_()                         # 5 frames per token: ceil(4.9)
        gen.encoder.proj_w.proj.bias.fill_(math.log(4.9))
    gen = gen.to(dev)
    assert gen.store_inverse(fused_reverse=True, device_front=True) == (True, True)
    voc = audio.GriffinLim(audio.TacotronSTFT(n_mel_channels=80)).to(dev)
    ids_b, t_x, _, _ = train.synth_batch(32, 150, 800, 0, "cpu")
    g = torch.Generator().manual_seed(5)
    one = torch.randint(1, 148, (1, 160), generator=g)
    cases = []
    if opt.shape != "single":
        cases.append(("bench batch: B = 32, T_x <= 150, 5 frames per token", ids_b, t_x, int(ids_b.shape[1]), 5 * int(ids_b.shape[1]), ()))
    if opt.shape != "batch":
        cases.append(("one utterance, 160 tokens = 800 frames", one, torch.tensor([160]), 160, 800, (1600,)))
    out = dict(device=torch.cuda.get_device_name(0), model="cfg 2: 6 encoder layers, 12 blocks x 4 layers, H = 192, eval, "
               "store_inverse(fused_reverse=True, device_front=True); GriffinLim over TacotronSTFT(80 mel channels)", griffin_lim_iterations=iters,
               seconds_per_window=opt.seconds, windows=windows, clock="time.perf_counter between two torch.cuda.synchronize()", shapes=[])
    for name, ids, xl, Tx_cap, Ty_cap, spare_caps in cases:
        B = int(ids.shape[0])
        plain = gen.compile_synthesis(B, Tx_cap, Ty_cap)
        whole = gen.compile_synthesis(B, Tx_cap, Ty_cap, vocoder=voc, vocoder_iters=iters)

        def two_steps(n, phases):
            for _ in range(n):
                h = plain(ids, xl, seed=7, noise_scale=0.667)
                frames = [2 * (v // 2) for v in h.lengths()]                       # the readback
                wav, _ = voc.from_mel(h.mel(), torch.tensor(frames, dtype=torch.int32, device=dev), mel_lengths_host=frames, n_iters=iters, seed=7,
                                      phases=phases)
            return wav

        def one_graph(n):
            for _ in range(n):
                wav, _ = whole(ids, xl, seed=7, noise_scale=0.667).wav()           # waits for this call's readback
            return wav

        h0 = plain(ids, xl, seed=7, noise_scale=0.667)
        frames0 = [2 * (v // 2) for v in h0.lengths()]                             # the batch is ragged: what the loop really works on
        mel0 = h0.mel(clone=True)
        frames0_dev = torch.tensor(frames0, dtype=torch.int32, device=dev)

        def mel_alone(n):
            for _ in range(n):
                y = plain(ids, xl, seed=7, noise_scale=0.667).mel()
            return y

        def loop_alone(n):                                                         # the eager counter path on a mel that is already there
            for _ in range(n):
                wav, _ = voc.from_mel(mel0, frames0_dev, mel_lengths_host=frames0, n_iters=iters, seed=7, phases="counter")
            return wav

        runs = {"mel_graph_then_from_mel_torch": lambda n: two_steps(n, "torch"), "mel_graph_then_from_mel_counter": lambda n: two_steps(n, "counter"),
                "one_graph_wav": one_graph, "mel_graph_alone": mel_alone, "from_mel_counter_alone": loop_alone}
        spare = {}
        for cap in spare_caps:                                                     # the same call in a graph of unused capacity: every launch of the loop is sized by it
            spare[cap] = gen.compile_synthesis(B, Tx_cap, cap, vocoder=voc, vocoder_iters=iters)
            runs[f"one_graph_wav_max_frames_{cap}"] = lambda n, w=spare[cap]: [w(ids, xl, seed=7, noise_scale=0.667).wav()[0] for _ in range(n)][-1]
        rec = dict(name=name, B=B, Tx=int(ids.shape[1]), max_tokens=Tx_cap, max_frames=Ty_cap, frames_per_utterance=frames0,
                   frames_total=sum(frames0), frames_mean_over_max_frames=round(sum(frames0) / (B * Ty_cap), 4),
                   audio_seconds_at_22050_hz=round(sum(256 * (F - 1) for F in frames0) / 22050.0, 2), variants={})
        res = {k: fn(2) for k, fn in runs.items()}
        torch.cuda.synchronize()
        rec["wav_samples_per_row"] = int(res["one_graph_wav"].shape[1])
        rec["one_graph_equals_from_mel_counter"] = bool(torch.equal(res["one_graph_wav"], res["mel_graph_then_from_mel_counter"]))
        with _lib.record_calls() as names:
            two_steps(1, "torch")
        rec["variants"]["mel_graph_then_from_mel_torch"] = dict(c_abi_entries_outside_the_graph=len([n for n in names if not n.endswith("_bytes")]), ms_per_call=[])
        with _lib.record_calls() as names:
            two_steps(1, "counter")
        rec["variants"]["mel_graph_then_from_mel_counter"] = dict(c_abi_entries_outside_the_graph=len([n for n in names if not n.endswith("_bytes")]), ms_per_call=[])
        rec["variants"]["one_graph_wav"] = dict(c_abi_entries_inside_the_graph=whole.captured_entries, c_abi_entries_outside_the_graph=0,
                                                overflows=whole.overflows, ms_per_call=[])
        rec["variants"]["mel_graph_alone"] = dict(what="the text-to-mel graph replayed and its mel taken, no vocoder", ms_per_call=[])
        rec["variants"]["from_mel_counter_alone"] = dict(what="from_mel(phases=\"counter\") on this batch's mel and lengths, no text-to-mel call",
                                                         c_abi_entries=2 + 2 * iters, ms_per_call=[])
        for cap, w in spare.items():
            rec["variants"][f"one_graph_wav_max_frames_{cap}"] = dict(max_frames=cap, c_abi_entries_inside_the_graph=w.captured_entries,
                                                                      equals_one_graph_wav=bool(torch.equal(res[f"one_graph_wav_max_frames_{cap}"], res["one_graph_wav"])),
                                                                      ms_per_call=[])
        for _ in range(windows):
            for k, fn in runs.items():
                torch.cuda.synchronize(); t0 = time.perf_counter(); fn(3); torch.cuda.synchronize()
                n = max(3, int(opt.seconds / ((time.perf_counter() - t0) / 3)) + 1)
                torch.cuda.synchronize(); t0 = time.perf_counter(); fn(n); torch.cuda.synchronize()
                rec["variants"][k]["ms_per_call"].append(round((time.perf_counter() - t0) * 1e3 / n, 4))
        for v in rec["variants"].values():
            t = v["ms_per_call"]
            v["ms_mean"], v["ms_spread"] = round(sum(t) / len(t), 4), round(max(t) - min(t), 4)
        base = rec["variants"]["mel_graph_then_from_mel_torch"]["ms_mean"]
        for k, v in rec["variants"].items():
            if k != "mel_graph_then_from_mel_torch":
                v["over_mel_graph_then_from_mel_torch_time"] = round(v["ms_mean"] / base, 4)
        print(f'{name}: ' + "; ".join(f'{k} {v["ms_mean"]:.3f} ms (+- {v["ms_spread"]:.3f})' for k, v in rec["variants"].items()), flush=True)
        out["shapes"].append(rec)
        del plain, whole, spare
    path = opt.json or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "synth_wav_bench.json")
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


def cfg5_main():
    import time
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "tests"))
    sys.path.insert(0, os.path.join(root, "tests", "golden"))
    from test_synthesis_fused_gpu import CFG5
    gen = models.FlowGenerator(n_vocab=187, out_channels=80, n_lang=10, **CFG5).eval()
    with torch.no_grad():
        for b in range(CFG5["n_blocks_dec"]):
            torch.nn.init.normal_(gen.decoder.flows[3 * b + 2].end.weight, std=0.01)
        ea = gen.encoder.proj_w.flows[0]                               # log w = (z - translation) * exp(-log_scale) ~ 0: 5 frames per token
        ea.log_scale.fill_(20.0)
        ea.translation.zero_()
    gen = gen.to(dev)
    assert gen.store_inverse(fused_reverse=True, device_front=True) == (True, True)
    ids_b, t_x, _, _ = train.synth_batch(32, 150, 800, 0, "cpu")
    g = torch.Generator().manual_seed(5)
    one = torch.randint(1, 148, (1, 160), generator=g)
    cases = []
    if opt.shape != "single":
        cases.append(("bench batch: B = 32, T_x <= 150, 5 frames per token", ids_b, t_x))
    if opt.shape != "batch":
        cases.append(("one utterance, 160 tokens = 800 frames", one, torch.tensor([160])))
    scal = dict(noise_scale=0.667, noise_scale_w=0.8, f0_noise_scale=0.8, energy_noise_scale=0.8, length_scale=4.9, pitch_scale=1.1,
                energy_scale=0.9)
    out = dict(device=torch.cuda.get_device_name(0), model="cfg 5: emotion front end, SDP (last flow pinned: 5 frames per token), SPP, SEP, "
               "10 encoder layers, 12 blocks x 4 layers, H = 192, eval, store_inverse(fused_reverse=True, device_front=True)",
               seconds_per_variant=opt.seconds, call=scal, shapes=[])
    for name, ids, xl in cases:
        B, Tx = int(ids.shape[0]), int(ids.shape[1])
        cond = dict(g=torch.randn(B, 512, generator=g), emo=torch.randint(0, 5, (B,), generator=g),
                    emo_cartesian=torch.rand(B, 3, generator=g) * torch.tensor([1.5, 3.1, 4.6]) + torch.tensor([0.0, 0.0, -1.55]),
                    l=torch.randint(0, 3, (B,), generator=g))
        ids_d, xl_d, cond_d = ids.to(dev), xl.to(dev), {k: v.to(dev) for k, v in cond.items()}

        def eager(n, key, ragged=True):
            gen.set_synthesis_front(True, noise_key=key)
            gen.rows_cfg.frame_rows_ragged = ragged
            for _ in range(n):
                res = gen.infer(ids_d, xl_d, seed=7, **cond_d, **scal)      # synchronises inside: its one readback
            gen.rows_cfg.frame_rows_ragged = True
            return res

        runs = {"eager_row": lambda n: eager(n, "row"), "eager_frame_uniform": lambda n: eager(n, "frame", False),
                "eager_frame": lambda n: eager(n, "frame")}
        rec = dict(name=name, B=B, Tx=Tx, variants={})
        for k, fn in runs.items():
            res = fn(3)
            with _lib.record_calls() as names:
                res = fn(1)
            torch.cuda.synchronize()
            assert torch.isfinite(res[0][0]).all() and torch.isfinite(res[3][0]).all()
            rec["T_y"] = int(res[0][0].shape[2])
            rec["variants"][k] = dict(c_abi_entries_per_call=len(names), ms_per_call=[])
            if k == "eager_frame":
                want, frame_rows = res, gen._front_last["rc_frames"].R
        rec["frame_rows_ragged"] = frame_rows
        rec["frame_rows_uniform"] = B * (int(want[3][0].shape[1]) + 2 * ops.HALO)
        if opt.graph:
            gen.set_synthesis_front(True, noise_key="frame")
            rcy = gen._front_last["rc"]
            # the default capacities (`batch` utterances of max_frames frames each) and, where that differs, the rows this batch needs
            caps = [("replay", None, None)] + ([("replay_fit", rcy.R, frame_rows)] if B > 1 else [])
            for tag, max_rows, max_frame_rows in caps:
                synth = gen.compile_synthesis(B, Tx, 5 * Tx, max_rows=max_rows, stochastic=True, max_frame_rows=max_frame_rows)

                def replay(n, synth=synth):
                    for _ in range(n):
                        h = synth(ids, xl, seed=7, **cond, **scal)
                        y = h.mel()                                         # waits for this call's readback
                    return h, y

                h, y = replay(3)
                pitch, energy = h.prosody()
                rec["variants"][tag] = dict(max_tokens=Tx, max_frames=5 * Tx, max_rows=synth.max_rows, max_frame_rows=synth.max_frame_rows,
                                            launches_per_call="1 upload + 1 graph replay + 1 readback",
                                            c_abi_entries_inside_the_graph=synth.captured_entries, status=h.status, overflows=synth.overflows,
                                            max_abs_difference_to_eager=dict(mel=(y - want[0][0]).abs().max().item(),
                                                                             pitch=(pitch - want[3][0]).abs().max().item(),
                                                                             energy=(energy - want[3][1]).abs().max().item()),
                                            ms_per_call=[])
                runs[tag] = replay
        for rep_i in range(opt.repeats):
            for k, fn in runs.items():
                torch.cuda.synchronize(); t0 = time.perf_counter(); fn(3); torch.cuda.synchronize()
                n = max(3, int(opt.seconds / ((time.perf_counter() - t0) / 3)) + 1)
                torch.cuda.synchronize(); t0 = time.perf_counter(); fn(n); torch.cuda.synchronize()
                rec["variants"][k]["ms_per_call"].append(round((time.perf_counter() - t0) * 1e3 / n, 4))
        for v in rec["variants"].values():
            t = v["ms_per_call"]
            v["ms_mean"], v["ms_spread"] = round(sum(t) / len(t), 4), round(max(t) - min(t), 4)
        ms = {k: v["ms_mean"] for k, v in rec["variants"].items()}
        rec["eager_frame_over_eager_row_time"] = round(ms["eager_frame"] / ms["eager_row"], 4)
        rec["ragged_over_uniform_frame_rows_time"] = round(ms["eager_frame"] / ms["eager_frame_uniform"], 4)
        for tag in ("replay", "replay_fit"):
            if tag in ms:
                rec[tag + "_over_eager_frame_time"] = round(ms[tag] / ms["eager_frame"], 4)
        print(f'{name}: T_y {rec["T_y"]}; ' + "; ".join(f'{k} {v["ms_mean"]:.3f} ms (+- {v["ms_spread"]:.3f})' for k, v in rec["variants"].items()), flush=True)
        out["shapes"].append(rec)
    gen.set_synthesis_front(True, noise_key="row")
    path = opt.json or os.path.join(root, "profiles", "synth_graph_cfg5_bench.json")
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


cfg5_main() if opt.cfg5 else wav_main() if opt.graph and opt.wav else graph_main() if opt.graph else infer_main() if opt.infer else main()
