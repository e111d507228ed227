"""dev: time of the neural vocoder (audio.HiFiGAN on csrc/hifigan.hip) against the same generator and weights as plain
PyTorch-ROCm conv1d / conv_transpose1d on the same device.

Two shapes, V1 with random weights: the bench batch (B = 32 utterances of 800 frames) and ONE 800-frame utterance.  Per shape:
  kernel      HiFiGAN.run (78 gt_voc_conv launches) captured in one graph and replayed; device events around >= --seconds of replays
              with a synchronise behind them, --repeats windows, the best and every window recorded.  The single utterance rotates
              over three workspaces and mels (its 92 MB workspace alone would sit in the 256 MB Infinity Cache); the batch's
              2.9 GB workspace is cold by itself.
  stages      the same launches cut into conv_pre, the four upsampling stages (transposed convolution + three resblocks) and
              conv_post, one graph each: time, the FLOP its MFMAs are asked for (2 L taps Cin N per launch, padding of the
              tiles not counted), the bytes an ideal launch moves (input, output, res, acc once each, the weight image once), and the
              share of the floor max(FLOP / 2.5 PFLOP/s bf16 dense, bytes / 6.29 TB/s measured HBM copy rate) in the measured time.
  torch       eager F.conv1d / F.conv_transpose1d / leaky_relu on the padded batch (all utterances have one length, so the padded
              batch IS the per-utterance definition), fp32 and under bf16 autocast, alternating with the kernel in every repeat.
  griffin_lim audio.GriffinLim.run_from_mel, 30 iterations, as one graph: the vocoder that was there before, for context only.
Outputs are compared once per shape: relative L2 of the kernel path and of each torch path against the fp32 torch result.

    python tools/hifigan_bench.py [--json profiles/hifigan_bench.json] [--seconds 0.5] [--repeats 3] [--shapes a,b]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402
from glow_tts_amd import audio  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--json", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "hifigan_bench.json"))
ap.add_argument("--seconds", type=float, default=0.5)
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--shapes", default="single_1x800,batch_32x800", help="which shapes to run; an existing --json keeps its other shapes")
ap.add_argument("--no-torch", action="store_true", help="skip the PyTorch formulations (their first calls search for algorithms)")
args = ap.parse_args()

if not torch.cuda.is_available():
    sys.exit("hifigan_bench needs the MI355X: there is nothing to time on a CPU")
dev = torch.device("cuda:0")
FRAMES, PEAK_BF16, HBM = 800, 2.5e15, 6.29e12
torch.manual_seed(0)
voc = audio.HiFiGAN().to(dev)
gl = audio.GriffinLim(audio.TacotronSTFT()).to(dev)
K = len(voc.resblock_kernel_sizes)


def torch_generator(mel):
    """the published generator on the module's own fp32 parameters"""
    x = F.conv1d(mel, voc.conv_pre.weight, voc.conv_pre.bias, padding=3)
    for i, up in enumerate(voc.ups):
        x = F.conv_transpose1d(F.leaky_relu(x, 0.1), up.weight, up.bias, stride=up.stride[0], padding=up.padding[0])
        xs = None
        for j in range(K):
            rb, y = voc.resblocks[i * K + j], x
            for c1, c2 in zip(rb.convs1, rb.convs2):
                t = F.conv1d(F.leaky_relu(y, 0.1), c1.weight, c1.bias, padding=c1.padding[0], dilation=c1.dilation[0])
                y = F.conv1d(F.leaky_relu(t, 0.1), c2.weight, c2.bias, padding=c2.padding[0]) + y
            xs = y if xs is None else xs + y
        x = xs / K
    return torch.tanh(F.conv1d(F.leaky_relu(x), voc.conv_post.weight, voc.conv_post.bias, padding=3))[:, 0]


def torch_bf16(mel):
    with torch.autocast("cuda", dtype=torch.bfloat16):
        return torch_generator(mel).float()


def say(*a):
    print(f"[{time.time() - T0:7.1f}s]", *a, flush=True)


def window(fn, per_call):
    """ms per call: `fn` (= per_call calls) repeated for >= args.seconds between two device events; a single call that already fills
    the window is the measurement"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); fn(); e1.record(); torch.cuda.synchronize()
    if e0.elapsed_time(e1) >= args.seconds * 1e3:
        return e0.elapsed_time(e1) / per_call
    n = 1
    while True:
        e0.record()
        for _ in range(n):
            fn()
        e1.record(); torch.cuda.synchronize()
        ms = e0.elapsed_time(e1)
        if ms >= args.seconds * 1e3:
            return ms / (n * per_call)
        n = max(n + 1, int(n * args.seconds * 1.2e3 / max(ms, 1e-3)))


STAGES = [("conv_pre", 0, 1)] + [(f"stage{i}", 1 + i * (voc.launches - 2) // len(voc.ups), 1 + (i + 1) * (voc.launches - 2) // len(voc.ups))
                                 for i in range(len(voc.ups))] + [("conv_post", voc.launches - 1, voc.launches)]


class Only:
    """HiFiGAN._launch restricted to launches [lo, hi) of a run, counting what they are asked for"""

    def __init__(self, lo, hi):
        self.lo, self.hi, self.i, self.flop, self.bytes = lo, hi, 0, 0.0, 0.0
        self.orig = audio.HiFiGAN._launch

    def __call__(self, m, dev_, n_frames, B, L, mul, X, img, Y, Cin, N, taps, dil, slope, x_sb, y_sb, ldy, **kw):
        if self.lo <= self.i < self.hi:
            self.flop += 2.0 * B * L * taps * Cin * N
            self.bytes += B * L * (Cin * (2 if kw.get("x_bf16") else 4) + N * (2 if kw.get("y_bf16") else 4)
                                   + 4 * N * ((kw.get("res") is not None) + (kw.get("acc") is not None))) + img[0].numel() * 2
            self.orig(m, dev_, n_frames, B, L, mul, X, img, Y, Cin, N, taps, dil, slope, x_sb, y_sb, ldy, **kw)
        self.i += 1

    def __enter__(self):
        audio.HiFiGAN._launch = lambda m, *a, **k: self(m, *a, **k)
        return self

    def __exit__(self, *exc):
        audio.HiFiGAN._launch = self.orig


T0 = time.time()
result = {"device": torch.cuda.get_device_name(0), "frames_per_utterance": FRAMES, "launches": voc.launches,
          "tile_positions": audio.call.gt_voc_tile_positions(), "peak_bf16_flops": PEAK_BF16, "hbm_bytes_per_s": HBM, "shapes": {}}
if os.path.exists(args.json):
    with open(args.json) as f:
        result["shapes"] = json.load(f).get("shapes", {})
for name, B, rot in (("single_1x800", 1, 3), ("batch_32x800", 32, 1)):
    if name not in args.shapes.split(","):
        continue
    g = torch.Generator().manual_seed(B)
    mels = [(torch.rand(B, 80, FRAMES, generator=g) * 13.0 - 11.5).to(dev) for _ in range(rot)]
    n_frames = torch.full((B,), FRAMES, dtype=torch.int32, device=dev)
    works = [voc.workspace(B, FRAMES, dev) for _ in range(rot)]
    say(name, f"inputs ready, workspace {voc.workspace_bytes(B, FRAMES) / 1e9:.3f} GB x {rot}")
    out_k = voc.run(mels[0], n_frames, works[0]).clone()
    torch.cuda.synchronize()
    say("kernel path ran once")
    side = torch.cuda.Stream()
    g_all = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g_all, stream=side):
        for m, w in zip(mels, works):
            voc.run(m, n_frames, w)
    stage_graphs, asked = {}, {}
    for sname, lo, hi in STAGES:
        stage_graphs[sname] = torch.cuda.CUDAGraph()
        with Only(lo, hi) as only, torch.cuda.graph(stage_graphs[sname], stream=side):
            for m, w in zip(mels, works):
                only.i = 0
                voc.run(m, n_frames, w)
        asked[sname] = (only.flop / rot, only.bytes / rot)
    gl_bufs = gl.mel_workspace(B, FRAMES, dev)
    gl.run_from_mel(mels[0], n_frames, gl_bufs, 30)
    g_gl = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g_gl, stream=side):
        gl.run_from_mel(mels[0], n_frames, gl_bufs, 30)
    times = {}

    def measure(variants):
        for _ in range(args.repeats):                                                 # the variants alternate inside every repeat
            for k, (fn, per_call) in variants.items():
                times.setdefault(k, []).append(window(fn, per_call))
                say(k, f"{times[k][-1]:.3f} ms")

    def record(check):
        best = {k: min(v) for k, v in times.items()}
        stages = {}
        for sname, _, _ in STAGES:
            flop, nbytes = asked[sname]
            floor_ms = max(flop / PEAK_BF16, nbytes / HBM) * 1e3
            stages[sname] = {"ms": best[sname], "gflop": flop * 1e-9, "mbytes": nbytes * 1e-6, "tflops": flop / best[sname] * 1e-9,
                             "share_of_bf16_peak": flop / PEAK_BF16 * 1e3 / best[sname], "share_of_hbm_rate": nbytes / HBM * 1e3 / best[sname],
                             "floor_ms": floor_ms, "bound": "mfma" if flop / PEAK_BF16 > nbytes / HBM else "hbm",
                             "floor_share_of_time": floor_ms / best[sname]}
        tot_flop = sum(v[0] for v in asked.values())
        shape = {"B": B, "audio_seconds_at_22050": B * FRAMES * 256 / 22050.0, "ms_best": best, "ms_windows": times, "outputs": check,
                 "stages": stages, "kernel_tflops": tot_flop / best["kernel"] * 1e-9,
                 "stage_sum_share_of_kernel": sum(best[s] for s, _, _ in STAGES) / best["kernel"],
                 "real_time_factor": B * FRAMES * 256 / 22050.0 / (best["kernel"] * 1e-3)}
        for k in ("torch_fp32", "torch_bf16_autocast"):
            shape[k + "_over_kernel"] = best[k] / best["kernel"] if k in best else "not measured"
        result["shapes"][name] = shape
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:                                               # after every phase: a later failure keeps the earlier one
            json.dump(result, f, indent=1)
        return shape

    variants = {"kernel": (g_all.replay, rot), "griffin_lim_30": (g_gl.replay, 1)}
    variants.update({s: (gr.replay, rot) for s, gr in stage_graphs.items()})
    measure(variants)
    shape = record({})
    if not args.no_torch:
        with torch.no_grad():
            out_t = torch_generator(mels[0])
            torch.cuda.synchronize()
            say("torch fp32 ran once")
            out_b = torch_bf16(mels[0])
            torch.cuda.synchronize()
            say("torch bf16 autocast ran once")
        nrm = torch.linalg.norm(out_t)
        check = {"kernel_vs_torch_fp32_rel_l2": (torch.linalg.norm(out_k - out_t) / nrm).item(),
                 "torch_bf16_vs_torch_fp32_rel_l2": (torch.linalg.norm(out_b - out_t) / nrm).item()}
        del out_t, out_b
        rr = [0]

        def t32():
            with torch.no_grad():
                rr[0] += 1
                torch_generator(mels[rr[0] % rot])

        def t16():
            with torch.no_grad():
                rr[0] += 1
                torch_bf16(mels[rr[0] % rot])
        measure({"kernel": (g_all.replay, rot), "torch_fp32": (t32, 1), "torch_bf16_autocast": (t16, 1)})
        shape = record(check)
    print(name, json.dumps(shape), flush=True)
    del works, gl_bufs, stage_graphs, g_all, g_gl
print("wrote", args.json)
