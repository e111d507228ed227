"""dev: time of the WaveGlow vocoder (audio.WaveGlow on csrc/waveglow.hip and gt_voc_conv) against the same network and
weights as plain PyTorch-ROCm conv1d / conv_transpose1d on the same device.

Two shapes, the published configuration with random weights (tests' kind of initialisation: a non-zero `end`): the bench batch
(B = 32 utterances of 800 frames) and ONE 800-frame utterance.  Per shape:
  kernel      WaveGlow.run (206 launches) captured in one graph and replayed; device events around >= --seconds of replays with a
              synchronise behind them, --repeats windows, the best and every window recorded.
  split       the same launches cut by kind — upsample (1 gt_voc_conv), gate (96 gt_wg_gate), res_skip (96 gt_voc_conv), boundary
              (13 gt_wg_boundary) — one graph each: time, the FLOP its MFMAs are asked for, and the rate that gives.
  yardstick   gt_wg_gate against the same 8 layers of one WaveNet as two gt_voc_conv launches each (in_layer on a dense fp32 copy of
              the residual stream, then the conditioning slice accumulated onto it, fp32 [B, L, 2C] in memory) plus an elementwise
              tanh * sigmoid -> bf16 in PyTorch.
  torch       the published `infer` with F.conv1d / F.conv_transpose1d on the padded batch from the SAME latent (drawn by the
              boundary kernel), fp32 and under bf16 autocast; its cond_layer output is [B, 4096, L] per flow.
Outputs are compared once per shape: relative L2 of the kernel path and of the bf16 torch path against the fp32 torch result.

    python tools/waveglow_bench.py [--json profiles/waveglow_bench.json] [--seconds 0.5] [--repeats 3] [--shapes a,b] [--no-torch]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402
from glow_tts_amd import _lib, audio  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--json", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "waveglow_bench.json"))
ap.add_argument("--seconds", type=float, default=0.5)
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--shapes", default="single_1x800,batch_32x800", help="which shapes to run; an existing --json keeps its other shapes")
ap.add_argument("--no-torch", action="store_true", help="skip the PyTorch formulations")
args = ap.parse_args()

if not torch.cuda.is_available():
    sys.exit("waveglow_bench needs the MI355X: there is nothing to time on a CPU")
dev = torch.device("cuda:0")
FRAMES, SEED = 800, 1
torch.manual_seed(0)
voc = audio.WaveGlow()
with torch.no_grad():                                                              # `end` is zero in the original's initialisation
    for p in voc.parameters():
        p.uniform_(-1.0, 1.0).mul_(1.0 / max(p[0].numel(), 1) ** 0.5 if p.dim() > 1 else 0.1)
    for j in range(voc.n_flows):
        c = voc.flow_channels[j]
        voc.convinv[j].conv.weight.copy_(torch.linalg.qr(torch.randn(c, c))[0][:, :, None])
        voc.WN[j].end.weight.normal_(0.0, 0.02)
voc = voc.to(dev)
C, n, Cs = voc.n_channels, voc.n_layers, voc.n_cond
T0 = time.time()


def say(*a):
    print(f"[{time.time() - T0:7.1f}s]", *a, flush=True)


def window(fn, per_call=1):
    """ms per call: `fn` repeated for >= args.seconds between two device events; a single call that already fills the window is the
    measurement"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); fn(); e1.record(); torch.cuda.synchronize()
    if e0.elapsed_time(e1) >= args.seconds * 1e3:
        return e0.elapsed_time(e1) / per_call
    k = 1
    while True:
        e0.record()
        for _ in range(k):
            fn()
        e1.record(); torch.cuda.synchronize()
        ms = e0.elapsed_time(e1)
        if ms >= args.seconds * 1e3:
            return ms / (k * per_call)
        k = max(k + 1, int(k * args.seconds * 1.2e3 / max(ms, 1e-3)))


class Only:
    """the C-ABI entries of a run restricted to one kind of launch: upsample, gate, res_skip or boundary"""

    def __init__(self, kind):
        self.kind, self.count = kind, 0

    def __enter__(self):
        self.saved = {k: getattr(audio.call, k) for k in ("gt_voc_conv", "gt_wg_gate", "gt_wg_boundary")}

        def entry(name, kind_of):
            def f(a, st):
                if kind_of(a) == self.kind:
                    self.count += 1
                    self.saved[name](a, st)
            return f
        audio.call.gt_voc_conv = entry("gt_voc_conv", lambda a: "upsample" if a.x_mel else "res_skip")
        audio.call.gt_wg_gate = entry("gt_wg_gate", lambda a: "gate")
        audio.call.gt_wg_boundary = entry("gt_wg_boundary", lambda a: "boundary")
        return self

    def __exit__(self, *exc):
        for k, v in self.saved.items():
            setattr(audio.call, k, v)


def flops(kind, B, L):
    """what the MFMAs of one run's launches of this kind are asked for"""
    if kind == "gate":
        return 2.0 * B * L * voc.n_flows * n * 2 * C * (3 * C + Cs)
    if kind == "res_skip":
        return 2.0 * B * L * voc.n_flows * C * (2 * C * (n - 1) + C)
    if kind == "upsample":
        return 2.0 * B * (L // 32) * 80 * 7 * 32 * Cs
    return 2.0 * B * L * sum(c * C + c * c + (c // 2) * C for c in voc.flow_channels)      # boundary: vector ALU


def latent(B, L):
    """Z [B, 8, L]: the kernels' own latent, all 8 slots drawn by one boundary launch (first and last form at once)"""
    A = torch.empty(B, L, 8, device=dev)
    state = torch.empty(4, device=dev)                                              # this form touches no state: never dereferenced
    nf = torch.full((B,), L // 32, dtype=torch.int32, device=dev)
    audio.call.gt_wg_boundary(_lib.fill_args(_lib.WgBoundaryArgs, state=state, st_stride_b=L * 2 * C, ld=2 * C, C=C, A=A, a_stride_b=8 * L,
                                             n_frames=nf, seed=SEED, sigma=voc.sigma, len_mul=32, B=B, L_cap=L, c_in=0, c_out=8),
                              _lib.current_stream(dev))
    return A.permute(0, 2, 1).contiguous()


def torch_infer(mel, Z):
    """the published infer on the module's own fp32 parameters"""
    s = F.conv_transpose1d(mel, voc.upsample.weight, voc.upsample.bias, stride=256)[:, :, :-768]
    s = s.unfold(2, 8, 8).permute(0, 2, 1, 3)
    spect = s.contiguous().view(s.size(0), s.size(1), -1).permute(0, 2, 1)
    a, used = Z[:, 8 - voc.n_remaining:], 8 - voc.n_remaining
    for k in reversed(range(voc.n_flows)):
        wn, h = voc.WN[k], a.size(1) // 2
        x = F.conv1d(a[:, :h], wn.start.weight, wn.start.bias)
        out = None
        cond = F.conv1d(spect, wn.cond_layer.weight, wn.cond_layer.bias)
        for i in range(n):
            acts = F.conv1d(x, wn.in_layers[i].weight, wn.in_layers[i].bias, padding=2 ** i, dilation=2 ** i) + cond[:, 2 * C * i:2 * C * (i + 1)]
            acts = torch.tanh(acts[:, :C]) * torch.sigmoid(acts[:, C:])
            rs = F.conv1d(acts, wn.res_skip_layers[i].weight, wn.res_skip_layers[i].bias)
            if i < n - 1:
                x, out = x + rs[:, :C], rs[:, C:] if out is None else out + rs[:, C:]
            else:
                out = out + rs
        del cond
        o = F.conv1d(out.float(), wn.end.weight, wn.end.bias)
        a = torch.cat([a[:, :h], (a[:, h:] - o[:, :h]) * torch.exp(-o[:, h:])], 1)
        a = F.conv1d(a.float(), torch.linalg.inv(voc.convinv[k].conv.weight[:, :, 0].double()).float()[:, :, None])
        if k % voc.n_early_every == 0 and k > 0:
            a = torch.cat((Z[:, used - 2:used], a), 1)
            used -= 2
    return a.permute(0, 2, 1).reshape(a.size(0), -1)


def torch_bf16(mel, Z):
    with torch.autocast("cuda", dtype=torch.bfloat16):
        return torch_infer(mel, Z).float()


def yardstick(B, L, bufs, n_frames):
    """one WaveNet's 8 gated layers as gt_voc_conv + gt_voc_conv + an elementwise gate, and as gt_wg_gate: two replayable closures"""
    wn = voc.WN[0]
    x = torch.randn(B, L, C, device=dev)
    acts = torch.empty(B, L, 2 * C, device=dev)
    g = bufs["g"].view(B, L, C)
    bufs["state"].view(B, L, 2 * C)[:, :, :C] = x
    imgs = [((audio.voc_pack(wn.in_layers[i].weight.detach()), wn.in_layers[i].bias.detach().contiguous()),
             (audio.voc_pack(wn.cond_layer.weight.detach()[2 * C * i:2 * C * (i + 1)]), wn.cond_layer.bias.detach()[2 * C * i:2 * C * (i + 1)].contiguous()))
            for i in range(n)]
    fused = voc.images()["flows"][0]["layers"]

    def conv(X, img, Cin, taps, dil, x_bf16, acc):
        audio.call.gt_voc_conv(_lib.fill_args(_lib.VocConvArgs, X=X, x_stride_b=L * Cin, W=img[0], bias=img[1], acc=acc, Y=acts, y_stride_b=L * 2 * C,
                                              ldy=2 * C, len_mul=32, n_frames=n_frames, B=B, L_cap=L, Cin=Cin, N=2 * C, taps=taps, dil=dil,
                                              x_bf16=x_bf16, slope=1.0, scale=1.0), _lib.current_stream(dev))   # the stream of the moment: a capture's

    def split():
        for i in range(n):
            conv(x, imgs[i][0], C, 3, 2 ** i, 0, None)
            conv(bufs["spect"], imgs[i][1], Cs, 1, 1, 1, acts)
            torch.mul(torch.tanh(acts[:, :, :C]), torch.sigmoid(acts[:, :, C:]), out=acts[:, :, :C])
            g.copy_(acts[:, :, :C])

    def one():
        for i, ly in enumerate(fused):
            audio.call.gt_wg_gate(_lib.fill_args(_lib.WgGateArgs, X=bufs["state"], x_stride_b=L * 2 * C, ldx=2 * C, Cs=Cs, S=bufs["spect"],
                                                 s_stride_b=L * Cs, W_in=ly["W_in"], W_cond=ly["W_cond"], b_in=ly["b_in"], b_cond=ly["b_cond"],
                                                 G=bufs["g"], g_stride_b=L * C, len_mul=32, n_frames=n_frames, B=B, L_cap=L, C=C, taps=3,
                                                 dil=2 ** i), _lib.current_stream(dev))
    return split, one, (x, acts, imgs)


result = {"device": torch.cuda.get_device_name(0), "frames_per_utterance": FRAMES, "launches": voc.launches,
          "tile_positions": audio.call.gt_wg_tile_positions(), "mflop_per_position": sum(flops(k, 1, 32) for k in ("gate", "res_skip", "upsample", "boundary")) / 32e6,
          "shapes": {}}
if os.path.exists(args.json):
    with open(args.json) as f:
        result["shapes"] = json.load(f).get("shapes", {})
for name, B in (("single_1x800", 1), ("batch_32x800", 32)):
    if name not in args.shapes.split(","):
        continue
    L = 32 * FRAMES
    g_ = torch.Generator().manual_seed(B)
    mel = (torch.rand(B, 80, FRAMES, generator=g_) * 13.0 - 11.5).to(dev)
    n_frames = torch.full((B,), FRAMES, dtype=torch.int32, device=dev)
    bufs = voc.workspace(B, FRAMES, dev)
    say(name, f"inputs ready, workspace {voc.workspace_bytes(B, FRAMES) / 1e9:.3f} GB")
    out_k = voc.run(mel, n_frames, bufs, seed=SEED).clone()
    torch.cuda.synchronize()
    say("kernel path ran once; finite:", bool(torch.isfinite(out_k).all()), "max |wav|", float(out_k.abs().max()))
    side = torch.cuda.Stream()
    graphs = {"kernel": torch.cuda.CUDAGraph()}
    with torch.cuda.graph(graphs["kernel"], stream=side):
        voc.run(mel, n_frames, bufs, seed=SEED)
    counts = {}
    for kind in ("upsample", "gate", "res_skip", "boundary"):
        graphs[kind] = torch.cuda.CUDAGraph()
        with Only(kind) as only, torch.cuda.graph(graphs[kind], stream=side):
            voc.run(mel, n_frames, bufs, seed=SEED)
        counts[kind] = only.count
    split, one, keep = yardstick(B, L, bufs, n_frames)
    split(); one(); torch.cuda.synchronize()
    for k, fn in (("gate_as_two_convs_and_eltwise", split), ("gate_fused_8_layers", one)):
        graphs[k] = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graphs[k], stream=side):
            fn()
    times = {}

    def measure(variants):
        for _ in range(args.repeats):
            for k, fn in variants.items():
                times.setdefault(k, []).append(window(fn))
                say(k, f"{times[k][-1]:.3f} ms")

    def record(check):
        best = {k: min(v) for k, v in times.items()}
        shape = {"B": B, "audio_seconds_at_22050": B * FRAMES * 256 / 22050.0, "workspace_bytes": voc.workspace_bytes(B, FRAMES),
                 "ms_best": best, "ms_windows": times, "outputs": check, "launch_counts": counts,
                 "split": {k: {"ms": best[k], "gflop": flops(k, B, L) * 1e-9, "tflops": flops(k, B, L) / best[k] * 1e-9}
                           for k in ("upsample", "gate", "res_skip", "boundary")},
                 "split_sum_share_of_kernel": sum(best[k] for k in ("upsample", "gate", "res_skip", "boundary")) / best["kernel"],
                 "kernel_tflops": sum(flops(k, B, L) for k in ("gate", "res_skip", "upsample")) / best["kernel"] * 1e-9,
                 "gate_fused_over_split": best["gate_fused_8_layers"] / best["gate_as_two_convs_and_eltwise"],
                 "real_time_factor": B * FRAMES * 256 / 22050.0 / (best["kernel"] * 1e-3)}
        for k in ("torch_fp32", "torch_bf16_autocast"):
            shape[k + "_over_kernel"] = best[k] / best["kernel"] if k in best else "not measured"
        result["shapes"][name] = shape
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:                                               # after every phase: a later failure keeps the earlier one
            json.dump(result, f, indent=1)
        return shape

    measure({k: gr.replay for k, gr in graphs.items()})
    shape = record({})
    if not args.no_torch:
        Z = latent(B, L)
        with torch.no_grad():
            out_t = torch_infer(mel, Z)
            torch.cuda.synchronize()
            say("torch fp32 ran once")
            out_b = torch_bf16(mel, Z)
            torch.cuda.synchronize()
            say("torch bf16 autocast ran once")
            nrm = torch.linalg.norm(out_t)
            check = {"kernel_vs_torch_fp32_rel_l2": (torch.linalg.norm(out_k - out_t) / nrm).item(),
                     "torch_bf16_vs_torch_fp32_rel_l2": (torch.linalg.norm(out_b - out_t) / nrm).item()}
            del out_t, out_b

            def t32():
                torch_infer(mel, Z)

            def t16():
                torch_bf16(mel, Z)
            measure({"kernel": graphs["kernel"].replay, "torch_fp32": t32, "torch_bf16_autocast": t16})
        shape = record(check)
    print(name, json.dumps(shape), flush=True)
    del bufs, graphs, keep
print("wrote", args.json)
